"""The many-workgroup build of the inverse neighbour lists (include/nsdp_scatter.h, csrc/invert_wide.hip) and what it lifts: the
lists are the stable sort of the entry numbers by source index, exactly; the segment sums, the attention backward and
index_points' backward over more than 8192 source points go through them and return the same bits twice."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def _wide(idx, N):
    """nsdp_knn_invert_wide called directly: (offsets, entries) of idx [B, n, k] over N sources."""
    from nsdp_amd import _lib
    L = _lib.lib()
    B = idx.shape[0]
    E = idx.numel() // B
    L.nsdp_knn_invert_wide_workspace_bytes.restype = ctypes.c_size_t
    need = int(L.nsdp_knn_invert_wide_workspace_bytes(ctypes.c_int(B), ctypes.c_int(E), ctypes.c_int(N)))
    assert need > 0
    ws = torch.full((need,), 0xA5, dtype=torch.uint8, device=DEV)            # (the call initialises what it needs itself)
    off = torch.full((B, N + 1), -7, dtype=torch.int32, device=DEV)
    ent = torch.full((B, E), -7, dtype=torch.int32, device=DEV)
    _lib.check(L.nsdp_knn_invert_wide(_lib.iptr(idx, "idx"), ctypes.c_int(B), ctypes.c_int(E), ctypes.c_int(N),
                                      ctypes.c_void_p(ws.data_ptr()), _lib.iptr(off), _lib.iptr(ent), _lib.stream_ptr()),
               "nsdp_knn_invert_wide")
    return off, ent


def _truth(idx, N):
    """The stable sort of e by idx[b][e] on the CPU, and the exclusive scan of the counts (tests/list_sum_ref.py), as tensors."""
    from list_sum_ref import inverse_lists_ref
    off, ent = inverse_lists_ref(idx.cpu().numpy(), N)
    return torch.from_numpy(off), torch.from_numpy(ent)


def _check(idx, N):
    off, ent = _wide(idx, N)
    want_off, want_ent = _truth(idx, N)
    assert torch.equal(off.cpu(), want_off)
    assert torch.equal(ent.cpu(), want_ent)


def _random_idx(B, n, N, k, seed=None):
    g = torch.Generator().manual_seed(n + N if seed is None else seed)
    return torch.randint(0, N, (B, n, k), generator=g, dtype=torch.int32).to(DEV)


def _tile():
    from nsdp_amd import hip_attention as ha
    return ha.INVERT_WIDE_TILE


@pytest.mark.parametrize("B,n,N,k", [(1, 5, 1, 8), (3, 37, 5, 7), (2, 8193, 8193, 16), (1, 2100, 32769, 16)])
def test_lists_are_the_stable_sort(B, n, N, k):
    _check(_random_idx(B, n, N, k), N)


@pytest.mark.parametrize("delta", [-1, 0, 1])
def test_lists_around_the_scan_tile(delta):
    N = _tile() + delta
    _check(_random_idx(2, 700, N, 3), N)


def test_lists_over_several_scan_tiles_with_a_partial_last_one():
    N = 3 * _tile() + 17
    _check(_random_idx(2, 2000, N, 3), N)


@pytest.mark.parametrize("n", [1024, 1025])
def test_one_list_on_either_side_of_the_long_list_switch(n):
    N, k = 300, 4
    idx = _random_idx(2, n, N, k)
    idx[idx == 5] = 6
    idx[:, :, 0] = 5                       # the list of source 5 has exactly n entries
    assert int((idx[0] == 5).sum()) == n
    _check(idx, N)


def test_all_duplicate_cloud_gives_k_long_lists():
    B, n, N, k = 1, 20000, 20000, 16
    idx = torch.arange(k, dtype=torch.int32, device=DEV).repeat(B, n, 1).contiguous()      # every query: rows 0 .. k-1
    _check(idx, N)


def test_lists_of_an_unaligned_index_tensor():
    """E a multiple of 4 but the tensor 4 bytes off a 16-byte boundary: the scalar loads."""
    B, n, N, k = 1, 600, 9001, 8
    store = torch.zeros(B * n * k + 1, dtype=torch.int32, device=DEV)
    idx = store[1:].view(B, n, k)
    idx.copy_(_random_idx(B, n, N, k))
    assert idx.data_ptr() % 16 == 4
    _check(idx, N)


@pytest.mark.parametrize("B,n,N,k", [(2, 300, 700, 16), (3, 64, 2048, 10), (1, 500, 500, 16)])
def test_old_and_new_entries_agree(B, n, N, k):
    """The shapes of test_attention_gpu.test_inverse_lists_and_segment_sum: `force` against the one-workgroup entry."""
    from nsdp_amd import hip_attention as ha
    g = torch.Generator().manual_seed(n + N)
    idx = torch.randint(0, N, (B, n, k), generator=g, dtype=torch.int32).to(DEV)
    idx[:, :, 0] = 5
    with ha.invert_wide_mode("0"):
        old = ha.inverse_lists(idx.clone(), N)
    with ha.invert_wide_mode("force"):
        new = ha.inverse_lists(idx.clone(), N)
    assert torch.equal(old[0], new[0]) and torch.equal(old[1], new[1])
    want_off, want_ent = _truth(idx, N)
    assert torch.equal(new[0].cpu(), want_off) and torch.equal(new[1].cpu(), want_ent)


def test_inverse_lists_beyond_the_old_entry():
    """32 769 sources: the one-workgroup entry refuses them (and still does with the knob at 0)."""
    from nsdp_amd import _lib, hip_attention as ha
    idx = _random_idx(1, 2100, 32769, 16)
    with ha.invert_wide_mode("1"):
        off, ent = ha.inverse_lists(idx, 32769)
    want_off, want_ent = _truth(idx, 32769)
    assert torch.equal(off.cpu(), want_off) and torch.equal(ent.cpu(), want_ent)
    with ha.invert_wide_mode("0"), pytest.raises(_lib.NsdpHipError, match="knn_invert"):
        ha.inverse_lists(idx.clone(), 32769)


def test_segment_sum_over_wide_lists():
    from nsdp_amd import hip_attention as ha
    B, n, N, k, d = 2, 9000, 9000, 16, 32
    g = torch.Generator().manual_seed(n + N)
    idx = torch.randint(0, N, (B, n, k), generator=g, dtype=torch.int32).to(DEV)
    idx[:, :, 0] = 5
    for dt in (torch.float32, torch.bfloat16):
        src = torch.randn(B, n, k, d, generator=g).to(dt).to(DEV)
        with ha.invert_wide_mode("1"):
            assert ha._use_wide(B, n * k, N)
            out = ha.segment_sum(src, idx, N, -1.0)
            again = ha.segment_sum(src, idx.clone(), N, -1.0)                    # (a clone: the lists are built again)
        ref = torch.zeros(B, N, d, dtype=torch.float64, device=DEV)
        ref.scatter_add_(1, idx.long().reshape(B, n * k, 1).expand(B, n * k, d), -src.double().reshape(B, n * k, d))
        assert float((out.double() - ref).abs().max()) <= 1e-5 * (float(ref.abs().max()) + 1)
        assert torch.equal(out, again)


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16])
def test_attention_backward_of_a_large_cloud_is_reproducible_and_matches_the_atomic_kernels(dt):
    """The body of test_attention_gpu.test_attention_backward_through_inverse_lists_matches_the_atomic_kernels at 9000 points,
    the knob at 1 (lists) against 0 (atomics, what every cloud above 8192 points took before), and 1 twice."""
    from nsdp_amd import hip_attention as ha
    B, n, N, k, d = 1, 9000, 9000, 16, 32
    with ha.invert_wide_mode("1"):
        assert ha._use_inverse(torch.float32, False, 9000, 9000, 32) is True
    g = torch.Generator().manual_seed(11)
    mk = lambda *s: torch.randn(*s, generator=g).to(dt).to(DEV)
    idx = torch.randint(0, N, (B, n, k), generator=g, dtype=torch.int32).to(DEV)
    base = dict(q=mk(B, n, d), kf=mk(B, N, d), vf=mk(B, N, d), pos=mk(B, n, k, d), res=mk(B, n, d))
    w = mk(B, n, d).float()
    outs = []
    for mode in ("1", "0", "1"):
        with ha.invert_wide_mode(mode):
            assert ha._use_inverse(dt, False, n, N, d) == (mode == "1")
            t = {kk: v.clone().requires_grad_(True) for kk, v in base.items()}
            u = ha.attn_pre(t["q"], t["kf"], t["pos"], idx.clone(), None)
            y = ha.attn_post(u * 0.5, t["vf"], t["pos"], idx, residual=t["res"])
            (y.float() * w).sum().backward()
            outs.append({kk: v.grad.float() for kk, v in t.items()})
    floor = float(outs[1]["kf"].abs().max())
    for kk in outs[0]:
        scale = max(float(outs[1][kk].abs().max()), floor)
        assert float((outs[0][kk] - outs[1][kk]).abs().max()) <= (2e-2 if dt is torch.bfloat16 else 1e-4) * scale, kk
        assert torch.equal(outs[0][kk], outs[2][kk]), kk


@pytest.mark.parametrize("B,S,C,N", [(2, 20000, 3, 9000), (1, 9000, 32, 9000)])
def test_scatter_add_rows_of_a_large_cloud(B, S, C, N, monkeypatch):
    from nsdp_amd import hip_attention as ha, pointnet2_utils as pu
    g = torch.Generator().manual_seed(S + C)
    src = torch.randn(B, S, C, generator=g).to(DEV)
    idx = torch.randint(0, N, (B, S), generator=g, dtype=torch.int32).to(DEV)
    calls = []
    real = ha.segment_sum
    monkeypatch.setattr(ha, "segment_sum", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    with ha.invert_wide_mode("1"):
        out = pu.scatter_add_rows(src, idx, N)
        again = pu.scatter_add_rows(src, idx.clone(), N)
    assert len(calls) == 2                                                    # (through the lists, not the atomic kernel)
    ref = torch.zeros(B, N, C, dtype=torch.float64, device=DEV)
    ref.scatter_add_(1, idx.long()[:, :, None].expand(B, S, C), src.double())
    assert out.shape == (B, N, C)
    assert float((out.double() - ref).abs().max()) <= 1e-5 * (float(ref.abs().max()) + 1)
    assert torch.equal(out, again)
    with ha.invert_wide_mode("0"):
        atomic = pu.scatter_add_rows(src, idx, N)
    assert len(calls) == 2
    assert float((atomic.double() - ref).abs().max()) <= 1e-5 * (float(ref.abs().max()) + 1)


def test_captured_once_replayed_on_new_indices():
    """inverse_lists + segment_sum as nodes of one captured graph (a single serial chain): a replay after the index buffer was
    refilled in place gives the eager result of the new contents.  (The entry zeroes its counters by a kernel of its own: with a
    hipMemsetAsync node in that place the SECOND replay of this graph counted on top of the first one's cursors -- the node's
    zeroes were not in place when the next node read -- and the lists it then built pointed outside their tensors.)"""
    from nsdp_amd import hip_attention as ha
    B, n, N, k, d = 1, 9000, 9000, 16, 32
    g = torch.Generator().manual_seed(3)
    first = torch.randint(0, N, (B, n, k), generator=g, dtype=torch.int32).to(DEV)
    second = torch.randint(0, N, (B, n, k), generator=g, dtype=torch.int32).to(DEV)
    src = torch.randn(B, n, k, d, generator=g).to(DEV)
    idx = first.clone()
    with ha.invert_wide_mode("1"):
        ha.segment_sum(src, idx.clone(), N, 1.0)                              # (warm: the library is loaded before the capture)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            out = ha.segment_sum(src, idx, N, 1.0)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, ha.segment_sum(src, first.clone(), N, 1.0))
        idx.copy_(second)
        graph.replay()
        torch.cuda.synchronize()
        want = ha.segment_sum(src, second.clone(), N, 1.0)
        assert torch.equal(out, want)
    assert not torch.equal(want, ha.segment_sum(src, first.clone(), N, 1.0))


def test_train_step_of_a_large_cloud_is_bit_reproducible():
    """A `forward` model over 8448 surface points: one train step twice from the same weights -- the same loss and gradient
    bits; with the knob at 0 (fp32 atomics above 8192 points) the same loss bits, the forward being untouched, and gradients
    within the bar test_attention_gpu.py uses between summation orders."""
    from helpers import build_product, model_cfg, nondeterministic_knobs, restore_model, snapshot_model, to_dev
    from nsdp_amd import hip_attention as ha, synth
    from nsdp_amd.model import optimizer_factory
    if nondeterministic_knobs():
        pytest.skip("knob run: fp32 atomics are back in the train step")
    cfg = model_cfg("forward", [8448, 128, 64])
    data = to_dev(synth.make_batch(41, 2, 8448, 256), DEV)
    model, train_fn, _ = build_product(cfg, 41, DEV)
    model.train()
    snap = snapshot_model(model)

    def step(mode):
        restore_model(model, snap)
        _, opt = optimizer_factory({"optimizer": "Adam", "lr": 5e-4}, model.parameters())
        with ha.invert_wide_mode(mode):
            loss = train_fn(model, opt, data, cfg)
        return loss, {kk: p.grad.detach().clone() for kk, p in model.named_parameters() if p.grad is not None}

    (l1, g1), (l2, g2), (l0, g0) = step("1"), step("1"), step("0")
    assert l1 == l2 and sorted(g1) == sorted(g2) and g1
    differ = [kk for kk in g1 if not torch.equal(g1[kk], g2[kk])]
    assert not differ, differ
    assert l0 == l1
    for kk in g1:
        assert float((g1[kk] - g0[kk]).abs().max()) <= 2e-5 * (float(g0[kk].abs().max()) + 1.0), kk
