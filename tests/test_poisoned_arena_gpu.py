"""Every kernel-launching entry of include/nsdp_hip.h inside the poisoned arena of tests/poison_arena.py.

Each call gets its operands from one 0xFF-filled allocation with 256 KiB guards around every operand, workspaces of exactly the
byte count the size query returned, and outputs that are NaN / -1 until the kernel writes them.  After the call: no byte
outside the outputs and workspaces changed (guards, inputs, rows an output's contract leaves alone), no element of a
written-whole output still holds the poison, every result is finite and equals a plain fp64 / exact reference within the
tolerance the kernel's own test file already asserts.  Shapes: the smallest that select each kernel's edge forms.

COVERAGE (entry -> test function) is data: tests/test_poison_arena_cpu.py holds it against the header without a GPU, and the
last test of this file holds it against what the recording proxy saw."""
import contextlib
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from poison_arena import PoisonArena

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
BF = torch.bfloat16
LL = ctypes.c_longlong

COVERAGE = {
    # exact fp32 GEMM and packs
    "nsdp_linear_f32": "test_linear_f32_and_packs",
    "nsdp_linear_wp_f32": "test_linear_f32_and_packs",
    "nsdp_pack_weight_f32": "test_linear_f32_and_packs",
    "nsdp_pack_weight_bf16x3": "test_pack_kernels_write_every_byte_of_the_declared_buffers",
    "nsdp_pack_weights_batched": "test_pack_kernels_write_every_byte_of_the_declared_buffers",
    "nsdp_pack_weights_bf16": "test_bf16_storage_dense_kernels",
    # bf16x3 forward
    "nsdp_linear_bf16x3_f32": "test_bf16x3_forward_entries",
    "nsdp_linear_bf16x3_gather_f32": "test_bf16x3_forward_entries",
    "nsdp_linear_bf16x3_signed_f32": "test_bf16x3_forward_entries",
    "nsdp_linear_bf16x3_addend_f32": "test_bf16x3_forward_entries",
    "nsdp_linear_bf16x3_h0_f32": "test_bf16x3_recomputed_hidden_layer_entries",
    "nsdp_linear_bf16x3_k4tail_f32": "test_bf16x3_recomputed_hidden_layer_entries",
    "nsdp_linear_wgrad_bf16x3_h0_f32": "test_bf16x3_recomputed_hidden_layer_entries",
    # G16
    "nsdp_layout_g16_f32": "test_g16_layout_kernel",
    "nsdp_linear_bf16x3_g16_f32": "test_g16_gemm_and_weight_gradient",
    "nsdp_linear_wgrad_bf16x3_g16_f32": "test_g16_gemm_and_weight_gradient",
    # weight gradients
    "nsdp_linear_wgrad_f32": "test_wgrad_f32",
    "nsdp_linear_wgrad_partials_f32": "test_wgrad_f32",
    "nsdp_wgrad_bf16_reduce_batched": "test_wgrad_f32",
    "nsdp_linear_wgrad_k4_remask_f32": "test_wgrad_k4_remask",
    "nsdp_linear_wgrad_bf16x3_f32": "test_wgrad_bf16x3",
    "nsdp_linear_wgrad_bf16x3_partials_f32": "test_wgrad_bf16x3",
    "nsdp_wgrad_bf16x3_reduce_batched": "test_wgrad_bf16x3",
    "nsdp_linear_bf16": "test_bf16_storage_dense_kernels",
    "nsdp_linear_wgrad_bf16": "test_bf16_storage_dense_kernels",
    "nsdp_linear_wgrad_bf16_partials": "test_bf16_storage_dense_kernels",
    "nsdp_linear_k4_bf16": "test_k4_bf16_kernels",
    "nsdp_linear_wgrad_k4_bf16": "test_k4_bf16_kernels",
    # BatchNorm
    "nsdp_bn_stats": "test_batchnorm",
    "nsdp_bn_train_fwd": "test_batchnorm",
    "nsdp_bn_apply": "test_batchnorm",
    "nsdp_bn_backward": "test_batchnorm",
    "nsdp_bn_stats_bf16": "test_batchnorm",
    "nsdp_bn_train_fwd_bf16": "test_batchnorm",
    "nsdp_bn_apply_bf16": "test_batchnorm",
    "nsdp_bn_backward_bf16": "test_batchnorm",
    # attention glue
    "nsdp_attn_pre_fwd": "test_attention_glue",
    "nsdp_attn_pre_bwd": "test_attention_glue",
    "nsdp_attn_pre_bwd_sub": "test_attention_glue",
    "nsdp_attn_post_fwd": "test_attention_glue",
    "nsdp_attn_post_bwd": "test_attention_glue",
    "nsdp_attn_post_bwd_det": "test_attention_glue",
    "nsdp_attn_pre_fwd_bf16": "test_attention_glue",
    "nsdp_attn_pre_bwd_bf16": "test_attention_glue",
    "nsdp_attn_pre_bwd_sub_bf16": "test_attention_glue",
    "nsdp_attn_post_fwd_bf16": "test_attention_glue",
    "nsdp_attn_post_bwd_bf16": "test_attention_glue",
    "nsdp_attn_post_bwd_det_bf16": "test_attention_glue",
    "nsdp_attn_post_fwd_q": "test_attention_post_from_u",
    "nsdp_attn_post_bwd_q": "test_attention_post_from_u",
    "nsdp_knn_invert": "test_inverse_lists_and_segment_sums",
    "nsdp_segment_sum_rows": "test_inverse_lists_and_segment_sums",
    "nsdp_segment_sum_rows_add": "test_inverse_lists_and_segment_sums",
    "nsdp_segment_sum_rows_bf16": "test_inverse_lists_and_segment_sums",
    "nsdp_segment_sum_rows_add_bf16": "test_inverse_lists_and_segment_sums",
    "nsdp_scatter_rows_onehot_f32": "test_onehot_scatters",
    "nsdp_scatter_rows_onehot_bf16": "test_onehot_scatters",
    # geometry
    "nsdp_furthest_point_sampling": "test_fps",
    "nsdp_knn": "test_knn",
    "nsdp_ball_query": "test_ball_query",
    "nsdp_three_nn": "test_three_nn",
    "nsdp_gather_points": "test_gather_group_interpolate",
    "nsdp_gather_points_grad": "test_gather_group_interpolate",
    "nsdp_group_points": "test_gather_group_interpolate",
    "nsdp_group_points_grad": "test_gather_group_interpolate",
    "nsdp_three_interpolate": "test_gather_group_interpolate",
    "nsdp_three_interpolate_grad": "test_gather_group_interpolate",
    "nsdp_scatter_cm_lists": "test_gather_group_interpolate",
    "nsdp_three_interpolate_grad_lists": "test_gather_group_interpolate",
    "nsdp_gather_rows": "test_row_gather_scatter_and_rel_coords",
    "nsdp_scatter_add_rows": "test_row_gather_scatter_and_rel_coords",
    "nsdp_rel_coords4": "test_row_gather_scatter_and_rel_coords",
    "nsdp_knn_ragged": "test_ragged_geometry",
    "nsdp_furthest_point_sampling_ragged": "test_ragged_geometry",
    "nsdp_knn_ragged_source": "test_ragged_geometry",
    # fused decoder
    "nsdp_decoder_fused_fwd": "test_fused_decoder",
    "nsdp_decoder_fused_fwd_bf16": "test_fused_decoder",
    "nsdp_decoder_fused_fwd_ragged": "test_fused_decoder",
    "nsdp_decoder_fused_fwd_bf16_ragged": "test_fused_decoder",
    # optimizer, device query
    "nsdp_adam_multi_f32": "test_adam",
    "nsdp_device_count": "test_device_count",
}

_SEEN: dict[str, set] = {}


def _modules():
    from nsdp_amd import hip_attention, hip_batchnorm, hip_decoder, hip_linear, hip_linear_bf16, pointnet2_utils
    return hip_linear, hip_linear_bf16, hip_attention, hip_batchnorm, hip_decoder, pointnet2_utils


@contextlib.contextmanager
def _arena(test, mb=64):
    """An arena with the wrapper modules' allocations and the library routed through it; notes what `test` called."""
    a = PoisonArena(DEV, mb << 20)
    with a.routed(*_modules()):
        yield a
    _SEEN.setdefault(test, set()).update(a.called)


def _call(name, *args):
    """One C-ABI call: tensors as device pointers, None as NULL, int -> int, float -> float; other widths as ctypes values."""
    from nsdp_amd import _lib
    conv = []
    for v in args:
        if v is None:
            conv.append(ctypes.c_void_p(0))
        elif isinstance(v, torch.Tensor):
            assert v.is_cuda and v.is_contiguous()
            conv.append(ctypes.c_void_p(v.data_ptr()))
        elif isinstance(v, (bool, int)):
            conv.append(ctypes.c_int(int(v)))
        elif isinstance(v, float):
            conv.append(ctypes.c_float(v))
        else:
            conv.append(v)
    _lib.check(getattr(_lib.lib(), name)(*conv, _lib.stream_ptr()), name)


def _bytes(name, *args):
    from nsdp_amd import _lib
    fn = getattr(_lib.lib(), name)
    fn.restype = ctypes.c_size_t
    return int(fn(*[v if isinstance(v, ctypes._SimpleCData) else ctypes.c_int(int(v)) for v in args]))


def _gen(seed):
    return torch.Generator(device="cpu").manual_seed(seed)


def _rand(g, *shape, scale=1.0):
    return torch.randn(*shape, generator=g) * scale


def _ins(a, /, **kw):
    """Arena inputs for the given CPU tensors (None passes through), as a dict."""
    return {k: (None if v is None else a.input(k, v)) for k, v in kw.items()}


def _d(t):
    return None if t is None else t.to(DEV).double()


def _finite(t, what):
    assert bool(torch.isfinite(t.float()).all()), f"{what}: non-finite values"


def _rel_err(y, ref, what):
    _finite(y, what)
    return float((y.double() - ref).abs().max()) / (float(ref.abs().max()) + 1e-30)


def _ref64(x, w, b, res, mask, out_mask, relu_in, relu_out):
    xi = _d(x)
    if mask is not None:
        xi = xi * (_d(mask) > 0)
    if relu_in:
        xi = F.relu(xi)
    y = xi @ _d(w).t()
    if b is not None:
        y = y + _d(b)
    if res is not None:
        y = y + _d(res)
    if relu_out:
        y = F.relu(y)
    if out_mask is not None:
        y = y * (_d(out_mask) > 0)
    return y


# ---------------------------------------------------------------------------------------------------------------------------------
# exact fp32 GEMM and the weight packs
# ---------------------------------------------------------------------------------------------------------------------------------
def _pack_f32_ref(w):
    """Wp[((tn * ceil(K/16) + kb) * 64 + 16 g + li) * 4 + c] = W[16 tn + li][16 kb + 4 g + c], zero padded (include/nsdp_hip.h)."""
    N, K = w.shape
    TN, KB = (N + 15) // 16, (K + 15) // 16
    p = torch.zeros(TN * 16, KB * 16, dtype=w.dtype)
    p[:N, :K] = w
    return p.reshape(TN, 16, KB, 4, 4).permute(0, 2, 3, 1, 4).contiguous().reshape(-1)


def _check_x3_pack(buf, w, what):
    """[ceil(K/32)][ceil(N/16)][plane h,m,l][lane 16 g + li][8 bf16] = planes of W[16 tn + li][32 kb + kperm(g, j)], kperm(g, j) =
    16 (j / 4) + 4 g + j % 4: the planes sum to W within 2^-22 relative, every plane of the padding is exactly zero."""
    N, K = w.shape
    KB, TN = (K + 31) // 32, (N + 15) // 16
    assert buf.numel() == KB * TN * 3 * 64 * 8 * 2, (what, buf.numel())
    planes = buf.cpu().view(BF).reshape(KB, TN, 3, 4, 16, 8)
    assert bool(torch.isfinite(planes.float()).all()), f"{what}: non-finite pack"
    p = torch.zeros(TN * 16, KB * 32, dtype=torch.float64)
    p[:N, :K] = w.double()
    rows = (16 * torch.arange(TN)[:, None] + torch.arange(16)[None, :])                              # tn, li
    j = torch.arange(8)
    cols = 32 * torch.arange(KB)[:, None, None] + (16 * (j // 4) + j % 4)[None, None, :] + 4 * torch.arange(4)[None, :, None]   # kb, g, j
    want = p[rows[None, :, None, :, None], cols[:, None, :, None, :]]                                # kb, tn, g, li, j
    inside = (rows[None, :, None, :, None] < N) & (cols[:, None, :, None, :] < K)
    assert not bool((planes.float() != 0).any(2)[~inside].any()), f"{what}: padding is not zero"
    got = planes.double().sum(2)
    assert bool(((got - want).abs() <= 2.0 ** -22 * want.abs()).all()), f"{what}: h + m + l != W"


@pytest.mark.parametrize("M,K,N", [(33, 256, 256), (64, 4, 120), (777, 200, 200), (5000, 128, 3)])
def test_linear_f32_and_packs(M, K, N):
    from nsdp_amd import hip_linear as hl
    g = _gen(M + 7 * K + N)
    x, w, b, r = _rand(g, M, K), _rand(g, N, K, scale=K ** -0.5), _rand(g, N), _rand(g, M, N)
    with _arena("test_linear_f32_and_packs") as a:
        t = _ins(a, x=x, w=w, b=b, r=r)
        y = hl._fwd(t["x"], t["w"], t["b"], t["r"], None, None, False, True)
        n_floats = _bytes("nsdp_packed_weight_floats", N, K)
        assert n_floats == ((N + 15) // 16) * ((K + 15) // 16) * 256
        wp, wpt = hl.pack_weight(t["w"], True, True)
        y_wp = hl._fwd_wp(t["x"], wp, N, t["b"], t["r"], None, None, False, True)
        outs = [y, wp, wpt, y_wp]
        if N % 4 == 0:      # dX = dY W through the pack of W^T, against the row-major kernel on W^T
            wt = a.input("wt", w.t().contiguous())
            dx_wp = hl._fwd_wp(t["r"], wpt, K, None, None, None, None, False, False)
            dx = hl._fwd(t["r"], wt, None, None, None, None, False, False)
            outs += [dx_wp, dx]
        a.check(written=outs)
    ref = _ref64(x, w, b, r, None, None, False, True)
    scale = float(ref.abs().max()) + 1e-6
    _finite(y, "y")
    assert float((y.double() - ref).abs().max()) <= 2e-6 * scale * max(1.0, K ** 0.5 / 4)
    assert torch.equal(y_wp, y)
    assert torch.equal(wp.cpu(), _pack_f32_ref(w)) and torch.equal(wpt.cpu(), _pack_f32_ref(w.t()))      # padding exactly zero
    if N % 4 == 0:
        assert torch.equal(dx_wp, dx)
        refx = _d(r) @ _d(w)
        assert float((dx.double() - refx).abs().max()) <= 2e-6 * float(refx.abs().max()) * max(1.0, N ** 0.5 / 4)


@pytest.mark.parametrize("N,K", [(3, 128), (120, 3), (200, 200), (256, 36)])
def test_pack_kernels_write_every_byte_of_the_declared_buffers(N, K):
    """nsdp_pack_weight_bf16x3, nsdp_pack_weight_f32 and nsdp_pack_weights_batched (kinds 0, 1, 3) into buffers of exactly the declared size: the whole
    buffer against the header's index formula built on the host, the padding exactly zero, batched == single bit for bit."""
    from nsdp_amd import hip_linear as hl
    g = _gen(N * 1000 + K)
    w = _rand(g, N, K)
    with _arena("test_pack_kernels_write_every_byte_of_the_declared_buffers") as a:
        wd = a.input("w", w)
        nb = [_bytes("nsdp_packed_weight_bf16x3_bytes", N, K, t) for t in (0, 1)]
        x3, x3t = hl.pack_weight_x3(wd, True, True)
        assert x3.numel() == nb[0] and x3t.numel() == nb[1]
        n_floats = _bytes("nsdp_packed_weight_floats", N, K)
        f1, f1t = hl.pack_weight(wd, True, True)                     # nsdp_pack_weight_f32, the single call
        assert f1.numel() == f1t.numel() == n_floats
        bufs = {"f": a.output("batched.f32.Wp", (n_floats,)), "ft": a.output("batched.f32.WpT", (n_floats,)),
                "x": a.output("batched.x3.Wp", (nb[0],), torch.uint8), "xt": a.output("batched.x3.WpT", (nb[1],), torch.uint8)}
        kinds = [(0, bufs["f"], bufs["ft"]), (1, bufs["x"], None), (1, None, bufs["xt"])]
        if K <= 4:
            bufs["w4"] = a.output("batched.w4", (N, 4))
            kinds.append((3, bufs["w4"], None))
        descs = (hl._PackDesc * len(kinds))()
        for d, (kind, p, pt) in zip(descs, kinds):
            d.W, d.N, d.K, d.kind = wd.data_ptr(), N, K, kind
            d.Wp = p.data_ptr() if p is not None else None
            d.WpT = pt.data_ptr() if pt is not None else None
        _call("nsdp_pack_weights_batched", descs, len(kinds))
        a.check(written=[x3.view(torch.int16), x3t.view(torch.int16), f1, f1t, bufs["f"], bufs["ft"], bufs["x"].view(torch.int16),
                         bufs["xt"].view(torch.int16), bufs.get("w4")])
    _check_x3_pack(x3, w, "Wp")
    _check_x3_pack(x3t, w.t(), "WpT")
    assert torch.equal(bufs["x"], x3) and torch.equal(bufs["xt"], x3t)
    assert torch.equal(bufs["f"].cpu(), _pack_f32_ref(w)) and torch.equal(bufs["ft"].cpu(), _pack_f32_ref(w.t()))
    assert torch.equal(f1, bufs["f"]) and torch.equal(f1t, bufs["ft"])
    if K <= 4:
        assert torch.equal(bufs["w4"].cpu(), F.pad(w, (0, 4 - K)))


# ---------------------------------------------------------------------------------------------------------------------------------
# bf16x3 forward
# ---------------------------------------------------------------------------------------------------------------------------------
X3_SHAPES = [(300, 36, 200), (1000, 200, 200), (4099, 120, 120)]


@pytest.mark.parametrize("M,K,N", X3_SHAPES + [(256 * 256 * 2 + 33, 200, 200)])
def test_bf16x3_forward_entries(M, K, N):
    """The plain, gather (both forms), signed and addend entries; at the persistent multi-block shape the plain entry with mask +
    out_mask once (four [M, 200] operands in the arena)."""
    from nsdp_amd import hip_linear as hl
    g = _gen(M + 13 * K + 101 * N)
    big = M > 100000
    x, w, b = _rand(g, M, K), _rand(g, N, K, scale=K ** -0.5), _rand(g, N)
    with _arena("test_bf16x3_forward_entries", mb=640 if big else 96) as a:
        t = _ins(a, x=x, w=w, b=b)
        wp = hl.pack_weight_x3(t["w"])[0]
        if big:
            m, o = _rand(g, M, K), _rand(g, M, N)
            t.update(_ins(a, m=m, o=o))
            y = hl._fwd_x3(t["x"], wp, N, t["b"], None, t["m"], t["o"], False, False)
            a.check(written=[y])
            sel = torch.cat([torch.arange(0, 512), torch.arange(M - 512, M), torch.randint(0, M, (4096,), generator=g)])
            ref = _ref64(x[sel], w, b, None, m[sel], o[sel], False, False)
            _finite(y, "y")
            assert float((y[sel.to(DEV)].double() - ref).abs().max()) / float(ref.abs().max()) <= 1.5e-6
            return
        r, m, o, ad = _rand(g, M, N), _rand(g, M, K), _rand(g, M, N), _rand(g, M, N)
        nsrc, rps = 37, 100                        # gather tables: rows_per_shape = 100 rows, 37 sources per shape
        shapes = (M + rps - 1) // rps
        gq, gk = _rand(g, (M + 3) // 4, N, scale=2.0), _rand(g, shapes * nsrc, N, scale=2.0)
        gidx = torch.randint(0, nsrc, (M,), generator=g).int()
        t.update(_ins(a, r=r, m=m, o=o, ad=ad, gq=gq, gk=gk, gidx=gidx))
        y_plain = hl._fwd_x3(t["x"], wp, N, t["b"], t["r"], None, None, False, True)
        y_relu_in = hl._fwd_x3(t["x"], wp, N, None, None, None, None, True, False)
        y_g2 = hl._fwd_x3_gather(t["x"], wp, N, t["b"], (t["gq"], 4, t["gk"], t["gidx"], rps, nsrc), False, False)
        y_g1 = hl._fwd_x3_gather(t["x"], wp, N, t["b"], (None, 1, t["gk"], t["gidx"], rps, nsrc), False, False)
        y_sg = hl._fwd_x3(t["x"], wp, N, t["b"], t["r"], None, None, False, False, res_sign=-1.0)
        y_ad = hl._fwd_x3(t["x"], wp, N, None, t["r"], t["m"], t["o"], False, False, addend=t["ad"])
        a.check(written=[wp.view(torch.int16), y_plain, y_relu_in, y_g2, y_g1, y_sg, y_ad])
    rows = torch.arange(M)
    kidx = (rows // rps) * nsrc + gidx.long()
    cases = {"plain": (y_plain, _ref64(x, w, b, r, None, None, False, True)),
             "relu_in": (y_relu_in, _ref64(x, w, None, None, None, None, True, False)),
             "gather2": (y_g2, _ref64(x, w, b, gq[rows // 4] - gk[kidx], None, None, False, False)),
             "gather1": (y_g1, _ref64(x, w, b, gk[kidx], None, None, False, False)),
             "signed": (y_sg, _ref64(x, w, b, -r, None, None, False, False)),
             "addend": (y_ad, _ref64(x, w, None, r, m, o, False, False) + _d(ad))}
    for name, (y, ref) in cases.items():
        assert _rel_err(y, ref, name) <= 1.5e-6, name


@pytest.mark.parametrize("M,K,N", X3_SHAPES + [(65536 + 17, 200, 200)])
def test_bf16x3_recomputed_hidden_layer_entries(M, K, N):
    """nsdp_linear_bf16x3_h0_f32 (plain and with both forms of the gathered addend), nsdp_linear_wgrad_bf16x3_h0_f32 and
    nsdp_linear_bf16x3_k4tail_f32 wherever their predicates take the shape (nsdp_linear_bf16x3_k4tail_ok wants 65536 rows: the
    last case is taken by all three).  The ReLU decisions of the recomputed hidden layer are the K = 4 kernel's by contract, so
    the references take the mask from that kernel's output and do everything else in fp64.
    nsdp_linear_f32 takes its K = 4 kernel from 4096 rows on (below, the general kernel with another rounding of the four
    products), so shorter inputs are handed to it zero-padded to 4096 rows: every row is computed on its own."""
    from nsdp_amd import _lib, hip_linear as hl
    g = _gen(M + K + N)
    x4 = _rand(g, M, 4)
    x4[:, 3] = 0
    w0, b0 = F.pad(_rand(g, K, 3), (0, 1)), _rand(g, K)                 # first layer Linear(3, K), zero-padded rows
    w, b, dy = _rand(g, N, K, scale=K ** -0.5), _rand(g, N), _rand(g, M, N)
    nsrc, rps = 37, 100                            # gather tables as in test_bf16x3_forward_entries
    shapes = (M + rps - 1) // rps
    gq, gk = _rand(g, (M + 3) // 4, N, scale=2.0), _rand(g, shapes * nsrc, N, scale=2.0)
    gidx = torch.randint(0, nsrc, (M,), generator=g).int()
    L = _lib.lib()
    did = []
    with _arena("test_bf16x3_recomputed_hidden_layer_entries", mb=768 if M > 10000 else 64) as a:
        t = _ins(a, x4=x4, w0=w0, b0=b0, w=w, b=b, dy=dy)
        x4p = t["x4"] if M >= 4096 else a.input("x4.padded", F.pad(x4, (0, 0, 0, 4096 - M)))
        h0_all = hl._fwd(x4p, t["w0"], t["b0"], None, None, None, False, True)           # the K = 4 kernel: [max(M, 4096), K]
        h0 = h0_all[:M]
        wp, wpt = hl.pack_weight_x3(t["w"], True, True)
        written = [h0_all]
        if L.nsdp_linear_bf16x3_h0_supported(LL(M), N, K):
            y = hl._fwd_x3_h0(t["x4"], t["w0"], t["b0"], wp, N, K, t["b"], None)
            y2 = hl._fwd_x3(h0, wp, N, t["b"], None, None, None, False, False)
            t.update(_ins(a, gq=gq, gk=gk, gidx=gidx))
            two, one = (t["gq"], 4, t["gk"], t["gidx"], rps, nsrc), (None, 1, t["gk"], t["gidx"], rps, nsrc)
            y_g2 = hl._fwd_x3_h0(t["x4"], t["w0"], t["b0"], wp, N, K, t["b"], two)      # the producer with the gathered addend
            y_g1 = hl._fwd_x3_h0(t["x4"], t["w0"], t["b0"], wp, N, K, t["b"], one)      # ... and its one-table form
            y2_g2 = hl._fwd_x3_gather(h0, wp, N, t["b"], two, False, False)
            y2_g1 = hl._fwd_x3_gather(h0, wp, N, t["b"], one, False, False)
            written += [y, y2, y_g2, y_g1, y2_g2, y2_g1]
            did.append("h0")
        if L.nsdp_linear_wgrad_bf16x3_h0_supported(LL(M), N, K):
            dw, db = hl._wgrad_h0_fn(t["w0"], t["b0"], K)(t["dy"], t["x4"], None, False, True)
            written += [dw, db]
            did.append("wgrad_h0")
        if L.nsdp_linear_bf16x3_k4tail_ok(LL(M), K, N):
            # dY [M, N] W [N, K] -> d(h0) [M, K] (never written); dW0 [K, 3], db0 [K] accumulate into finite prefills
            nbytes = _bytes("nsdp_linear_bf16x3_k4tail_workspace_bytes", LL(M), K)
            ws = a.workspace("k4tail.ws", nbytes)
            pre_w, pre_b = _rand(g, K, 3), _rand(g, K)
            dw0, db0 = a.accum("dW0", pre_w), a.accum("db0", pre_b)
            _call("nsdp_linear_bf16x3_k4tail_f32", t["dy"], wpt, t["x4"], t["w0"], t["b0"], dw0, db0, LL(M), K, N, 3, 1, ws,
                  ctypes.c_size_t(nbytes))
            written += [dw0, db0]
            did.append("k4tail")
        a.check(written=written)
    if M > 65536:
        assert did == ["h0", "wgrad_h0", "k4tail"], did
    h64 = _d(h0)
    if "h0" in did:
        assert torch.equal(y, y2)                                    # bit for bit the two-launch form
        plain = h64 @ _d(w).t() + _d(b)
        assert _rel_err(y, plain, "h0") <= 1.5e-6
        kidx = ((torch.arange(M) // rps) * nsrc + gidx.long()).to(DEV)
        rows4 = (torch.arange(M) // 4).to(DEV)
        assert torch.equal(y_g2, y2_g2) and torch.equal(y_g1, y2_g1)
        assert _rel_err(y_g2, plain + _d(gq)[rows4] - _d(gk)[kidx], "h0 gather, two tables") <= 1.5e-6
        assert _rel_err(y_g1, plain + _d(gk)[kidx], "h0 gather, one table") <= 1.5e-6
    if "wgrad_h0" in did:
        rw, rb = _d(dy).t() @ h64, _d(dy).sum(0)
        assert _rel_err(dw, rw, "dW(h0)") <= 3e-6 and _rel_err(db, rb, "db(h0)") <= 3e-6
    if "k4tail" in did:
        dh = (_d(dy) @ _d(w)) * (h64 > 0)
        rw, rb = dh.t() @ _d(x4)[:, :3] + _d(pre_w), dh.sum(0) + _d(pre_b)
        assert _rel_err(dw0, rw, "dW0") <= 2e-5 and _rel_err(db0, rb, "db0") <= 2e-5


# ---------------------------------------------------------------------------------------------------------------------------------
# G16
# ---------------------------------------------------------------------------------------------------------------------------------
def _g16_ref(t):
    M, C = t.shape
    return t.reshape(M // 16, 16, C // 4, 4).permute(0, 2, 1, 3).contiguous().reshape(M, C)


def _bits_ref(h):
    """[M / 16][ceil(C / 32)][64] bytes, byte (group, kb, 4 * row + g) = bits 0-3 [h > 0] at channels 32 kb + 4 g .. + 3, bits 4-7
    at 32 kb + 16 + 4 g .. + 3 (include/nsdp_hip.h)."""
    M, C = h.shape
    KB = (C + 31) // 32
    pos = torch.zeros(M, KB * 32, dtype=torch.bool, device=h.device)
    pos[:, :C] = h > 0
    p = pos.reshape(M // 16, 16, KB, 2, 4, 4)
    nib = (p.to(torch.int32) * torch.tensor([1, 2, 4, 8], device=h.device, dtype=torch.int32)).sum(-1)
    byte = nib[:, :, :, 0, :] + 16 * nib[:, :, :, 1, :]
    return byte.permute(0, 2, 1, 3).contiguous().reshape(-1).to(torch.uint8)


@pytest.mark.parametrize("M,C", [(48, 200), (65536 + 16, 120)])
def test_g16_layout_kernel(M, C):
    from nsdp_amd import hip_linear as hl
    x = _rand(_gen(M + C), M, C)
    with _arena("test_g16_layout_kernel", mb=128) as a:
        xd = a.input("x", x)
        xg = hl.to_g16(xd)
        back = hl.to_g16(xg, back=True)
        a.check(written=[xg, back])
    assert torch.equal(xg.cpu(), _g16_ref(x)) and torch.equal(back.cpu(), x)


def test_g16_gemm_and_weight_gradient():
    """The G16 GEMM with bits_out (layout 2), with mask_bits (layout 1), and the G16 weight gradient with `bits` (layout 1) and
    with X in G16 (layout 2), at a row count that is no multiple of the 256-row workgroup tile; the bits buffer has exactly nsdp_relu_bits_bytes bytes."""
    from nsdp_amd import _lib, hip_linear as hl
    M, K, N = 32768 + 32, 200, 200
    L = _lib.lib()
    for lay, msk, rin in ((2, 0, 0), (1, 1, 0)):
        assert L.nsdp_linear_bf16x3_g16_supported(LL(M), N, K, lay, msk, rin)
    assert L.nsdp_linear_wgrad_bf16x3_g16_supported(LL(M), N, K, 1, 1) and L.nsdp_linear_wgrad_bf16x3_g16_supported(LL(M), N, K, 2, 0)
    g = _gen(M)
    x, w, b, dy, res = _rand(g, M, K), _rand(g, N, K, scale=K ** -0.5), _rand(g, N), _rand(g, M, N), _rand(g, M, K)
    with _arena("test_g16_gemm_and_weight_gradient", mb=512) as a:
        t = _ins(a, x=x, w=w, b=b, dy_g16=_g16_ref(dy), res=res, x_g16=_g16_ref(x))
        wp, wpt = hl.pack_weight_x3(t["w"], True, True)
        nbits = _bytes("nsdp_relu_bits_bytes", LL(M), N)
        assert nbits == (M // 16) * ((N + 31) // 32) * 64
        bits = a.output("bits", (nbits,), torch.uint8)
        h = hl._fwd_x3_g16(t["x"], wp, N, t["b"], None, None, None, False, True, hl.LAY_Y, bits_out=bits)     # h [M, N] in G16
        dx = hl._fwd_x3_g16(t["dy_g16"], wpt, K, None, t["res"], None, None, False, False, hl.LAY_X, mask_bits=bits)
        dw, db = hl._wgrad_g16_fn(1, bits)(t["dy_g16"], t["x"], None, True, True)
        dw2, db2 = hl._wgrad_g16_fn(2)(t["dy_g16"], t["x_g16"], None, False, True)      # (row-major "dY" = the G16 bytes, as values)
        a.check(written=[h, dx, dw, db, dw2, db2])      # (bits: 0xFF is a legal byte there; compared whole below)
    href = F.relu(_ref64(x, w, b, None, None, None, False, False))
    hrow = h.cpu().reshape(M // 16, N // 4, 16, 4).permute(0, 2, 1, 3).reshape(M, N)          # G16 -> row-major
    assert _rel_err(hrow.to(DEV), href, "h") <= 1.5e-6
    assert torch.equal(bits.cpu(), _bits_ref(hrow))
    mask = (hrow > 0).to(DEV)
    assert _rel_err(dx, (_d(dy) * mask) @ _d(w) + _d(res), "dx") <= 1.5e-6
    dym = _d(dy) * mask
    assert _rel_err(dw, dym.t() @ F.relu(_d(x)), "dW") <= 3e-6 and _rel_err(db, dym.sum(0), "db") <= 3e-6
    dyv = _d(_g16_ref(dy))
    assert _rel_err(dw2, dyv.t() @ _d(x), "dW layout 2") <= 3e-6 and _rel_err(db2, dyv.sum(0), "db layout 2") <= 3e-6


# ---------------------------------------------------------------------------------------------------------------------------------
# weight gradients
# ---------------------------------------------------------------------------------------------------------------------------------
def _wgrad_ref(dy, x, mask, relu_x):
    dyp = _d(dy) * (_d(mask) > 0) if mask is not None else _d(dy)
    xp = F.relu(_d(x)) if relu_x else _d(x)
    return dyp.t() @ xp, dyp.sum(0)


@contextlib.contextmanager
def _pending_reduce(hl):
    """hip_linear's weight-gradient routines hand their partial sums to this batch instead of reducing them."""
    batch = hl._new_reduce_batch()
    prev, hl._cur_reduce = hl._cur_reduce, batch
    try:
        yield batch
    finally:
        hl._cur_reduce = prev


@pytest.mark.parametrize("M,N,K,mask,relu_x", [(33, 40, 24, False, True), (777, 200, 120, True, False), (2049, 120, 4, True, True)])
def test_wgrad_f32(M, N, K, mask, relu_x):
    """nsdp_linear_wgrad_f32 (fresh and accumulate = 1) and the _partials_f32 + nsdp_wgrad_bf16_reduce_batched pair."""
    assert K == 4 or M <= 2048                     # (the two kernel forms whose bounds are applied below)
    from nsdp_amd import hip_linear as hl
    g = _gen(M * 7 + N + K)
    dy, x = _rand(g, M, N), _rand(g, M, K)
    mk = _rand(g, M, N) if mask else None
    pre_w, pre_b = _rand(g, N, K), _rand(g, N)
    with _arena("test_wgrad_f32") as a:
        t = _ins(a, dy=dy, x=x, mk=mk)
        dw, db = hl._wgrad(t["dy"], t["x"], t["mk"], relu_x, True)
        acc = (a.accum("acc.dW", pre_w), a.accum("acc.db", pre_b))
        got = hl._wgrad(t["dy"], t["x"], t["mk"], relu_x, True, out=acc)
        assert got[0] is acc[0] and got[1] is acc[1]
        with _pending_reduce(hl) as batch:
            dwp, dbp = hl._wgrad(t["dy"], t["x"], t["mk"], relu_x, True)
            hl._flush_reduce(batch)
        a.check(written=[dw, db, acc[0], acc[1], dwp, dbp])
    rw, rb = _wgrad_ref(dy, x, mk, relu_x)
    for name, got_, ref, pre in (("dW", dw, rw, None), ("db", db, rb, None), ("dW acc", acc[0], rw, pre_w), ("db acc", acc[1], rb, pre_b)):
        _finite(got_, name)
        top = float(ref.abs().max())
        # the bound of the kernel form the shape selects: K = 4 the streaming kernel (test_wgrad_k4_stream_kernel), up to 2048 rows
        # the output-stationary one (test_output_stationary_weight_gradient_for_few_rows), both of tests/test_linear_gpu.py
        bound = 3e-6 * top + 1e-5 if K == 4 else 2e-6 * (top + 1e-6) * max(1.0, M ** 0.5 / 8)
        if pre is not None:      # in-place accumulation: one more fp32 rounding of the sum (1e-6 of it, as that test allows)
            ref = ref + _d(pre)
            bound += 1e-6 * float(ref.abs().max())
        assert float((got_.double() - ref).abs().max()) <= bound, (name, bound)
    assert torch.equal(dwp, dw) and torch.equal(dbp, db)


def test_wgrad_k4_remask():
    from nsdp_amd import hip_linear as hl
    M, N = 8192, 256
    g = _gen(M + N)
    dy, x4, w4, b = _rand(g, M, N), F.pad(_rand(g, M, 3), (0, 1)), F.pad(_rand(g, N, 3), (0, 1)), _rand(g, N)
    with _arena("test_wgrad_k4_remask") as a:
        t = _ins(a, dy=dy, x4=x4, w4=w4, b=b)
        h = hl._fwd(t["x4"], t["w4"], t["b"], None, None, None, False, True)        # the mask decisions are this kernel's
        dw, db = hl._wgrad_k4_remask(t["w4"], t["b"], 4)(t["dy"], t["x4"], None, False, True)
        a.check(written=[h, dw, db])
    rw, rb = _wgrad_ref(dy, x4, h, False)
    _finite(dw, "dW"), _finite(db, "db")
    assert torch.allclose(dw.double(), rw, rtol=1e-4, atol=1e-4 * float(rw.abs().max()))
    assert torch.allclose(db.double(), rb, rtol=1e-4, atol=1e-4 * float(rb.abs().max()))


@pytest.mark.parametrize("M,N,K,mask,relu_x", [(4099, 120, 128, True, True), (2500, 256, 200, False, True), (4096, 120, 128, True, True)])
def test_wgrad_bf16x3(M, N, K, mask, relu_x):
    """nsdp_linear_wgrad_bf16x3_f32 fresh and with accumulate = 1, and the _partials_f32 + _reduce_batched pair (bit-equal)."""
    from nsdp_amd import hip_linear as hl
    g = _gen(M + N + K)
    dy, x = _rand(g, M, N), _rand(g, M, K)
    mk = _rand(g, M, N) if mask else None
    pre_w, pre_b = _rand(g, N, K), _rand(g, N)
    with _arena("test_wgrad_bf16x3", mb=128) as a:
        t = _ins(a, dy=dy, x=x, mk=mk)
        dw, db = hl._wgrad_x3(t["dy"], t["x"], t["mk"], relu_x, True)
        acc = (a.accum("acc.dW", pre_w), a.accum("acc.db", pre_b))
        hl._wgrad_x3(t["dy"], t["x"], t["mk"], relu_x, True, out=acc)
        with _pending_reduce(hl) as batch:
            dwp, dbp = hl._wgrad_x3(t["dy"], t["x"], t["mk"], relu_x, True)
            assert len(batch["descs"]) == 1
            hl._flush_reduce(batch)
        a.check(written=[dw, db, acc[0], acc[1], dwp, dbp])
    rw, rb = _wgrad_ref(dy, x, mk, relu_x)
    assert _rel_err(dw, rw, "dW") <= 3e-6 and _rel_err(db, rb, "db") <= 3e-6
    assert _rel_err(acc[0], rw + _d(pre_w), "dW acc") <= 3e-6 and _rel_err(acc[1], rb + _d(pre_b), "db acc") <= 3e-6
    assert torch.equal(dwp, dw) and torch.equal(dbp, db)


BF_WG = [(4096, 120, 120, False, False), (5000, 200, 200, True, False), (4099, 256, 256, False, True), (33, 128, 200, True, True),
         (3200, 256, 120, False, False), (31, 8, 8, False, False), (4097, 256, 256, True, True), (65, 200, 200, True, False),
         (63, 64, 64, False, False)]      # the WG shapes of tests/test_bf16_gpu.py with M <= 5000


@pytest.mark.parametrize("M,N,K,mask,relu_x", BF_WG)
def test_bf16_storage_dense_kernels(M, N, K, mask, relu_x):
    """nsdp_pack_weights_bf16, nsdp_linear_bf16, nsdp_linear_wgrad_bf16 and its _partials + reduce pair, on bf16 inputs against fp64
    arithmetic on the same bf16 values."""
    from nsdp_amd import hip_linear as hl, hip_linear_bf16 as hb
    g = _gen(M + 3 * N + 5 * K)
    dy, x = _rand(g, M, N).to(BF), _rand(g, M, K).to(BF)
    mk = _rand(g, M, N).to(BF).clamp_min(0) if mask else None
    w, b = _rand(g, N, K, scale=K ** -0.5), _rand(g, N)
    with _arena("test_bf16_storage_dense_kernels", mb=96) as a:
        t = _ins(a, dy=dy, x=x, mk=mk, w=w, b=b)
        wp, wpt = hb.pack_weight_b16(t["w"], True, True)
        written = [wp.view(torch.int16), wpt.view(torch.int16)]
        y = None
        if hb.supported(N, K):
            y = hb.run(t["x"], wp, N, t["b"], None, None, None, False, True)
            written.append(y)
        dw, db = hb.wgrad(t["dy"], t["x"], t["mk"], relu_x, True)
        with _pending_reduce(hl) as batch:
            dwp, dbp = hb.wgrad(t["dy"], t["x"], t["mk"], relu_x, True)
            hl._flush_reduce(batch)
        written += [dw, db, dwp, dbp]
        a.check(written=written)
    if y is not None:
        ref = F.relu(_d(x) @ w.to(BF).to(DEV).double().t() + _d(b))
        _finite(y, "y")
        assert bool(((y.double() - ref).abs() <= 2 ** -8 * ref.abs() + 1e-5).all())      # one bf16 rounding of the result
    rw, rb = _wgrad_ref(dy, x, mk, relu_x)
    grow = max(1.0, (M / 4096) ** 0.5)
    _finite(dw, "dW"), _finite(db, "db")
    assert float((dw.double() - rw).abs().max()) <= 3e-6 * (float(rw.abs().max()) + 1e-6) * grow + 1e-6
    assert float((db.double() - rb).abs().max()) <= 3e-6 * (float(rb.abs().max()) + 1) * grow
    assert torch.equal(dwp, dw) and torch.equal(dbp, db)


@pytest.mark.parametrize("M,N,relu,mask", [(5000, 200, True, True), (4096, 256, False, False), (33, 8, True, True)])
def test_k4_bf16_kernels(M, N, relu, mask):
    from nsdp_amd import hip_linear_bf16 as hb
    g = _gen(M + N)
    x4, w4, b, dy = F.pad(_rand(g, M, 3), (0, 1)), _rand(g, N, 4), _rand(g, N), _rand(g, M, N).to(BF)
    with _arena("test_k4_bf16_kernels") as a:
        t = _ins(a, x4=x4, w4=w4, b=b, dy=dy)
        y = hb.k4_forward(t["x4"], t["w4"], t["b"], relu)
        dw, db = hb.k4_wgrad(t["dy"], t["x4"], y if mask else None, False, True)
        a.check(written=[y, dw, db])
    ref = _d(x4) @ _d(w4).t() + _d(b)
    ref = F.relu(ref) if relu else ref
    _finite(y, "y")
    assert bool(((y.double() - ref).abs() <= 2 ** -8 * ref.abs() + 1e-5).all())
    rw, rb = _wgrad_ref(dy, x4, y if mask else None, False)
    grow = max(1.0, (M / 4096) ** 0.5)
    _finite(dw, "dW"), _finite(db, "db")
    assert float((dw.double() - rw).abs().max()) <= 1e-5 * (float(rw.abs().max()) + 1) * grow
    assert float((db.double() - rb).abs().max()) <= 1e-5 * (float(rb.abs().max()) + 1) * grow


# ---------------------------------------------------------------------------------------------------------------------------------
# BatchNorm, fp32 and bf16 storage
# ---------------------------------------------------------------------------------------------------------------------------------
def _bn_close(got, ref, dt, what, abs_tol=None):
    """fp32 outputs (in bf16 storage too: statistics, parameter gradients and running statistics are fp32 sums of the same rounded
    inputs the fp64 reference reads): the bounds of tests/test_batchnorm_gpu.py; bf16 outputs: that of tests/test_bf16_gpu.py
    (1.5e-2 of the scale)."""
    _finite(got, what)
    err = float((got.double() - ref).abs().max())
    if got.dtype is BF:
        assert err <= 1.5e-2 * (float(ref.abs().max()) + 1e-6), (what, err)
    elif abs_tol is not None:
        assert err < abs_tol, (what, err)
    else:
        assert err <= 2e-5 * (float(ref.abs().max()) + 1.0), (what, err)


@pytest.mark.parametrize("dt", [torch.float32, BF], ids=["f32", "bf16"])
@pytest.mark.parametrize("C", [8, 120, 256])
@pytest.mark.parametrize("R", [7, 4096, 4097, 16385])
def test_batchnorm(R, C, dt):
    """train_fwd (updates = 2), stats, apply and backward (training and eval) with and without addend + ReLU; the running statistics
    and the batch counter live in the arena as accumulated operands, the workspace has exactly nsdp_bn_workspace_bytes(C) bytes."""
    sfx = "_bf16" if dt is BF else ""
    eps, mom = 1e-5, 0.1
    g = _gen(R * 7 + C)
    gamma, beta = torch.rand(C, generator=g) + 0.5, _rand(g, C, scale=0.1)
    rm0, rv0 = _rand(g, C, scale=0.1), torch.rand(C, generator=g) + 0.5
    nws = _bytes("nsdp_bn_workspace_bytes", C)
    for full in (False, True):
        x = (_rand(g, R, C) * 2 + 0.5).to(dt)
        ad = _rand(g, R, C).to(dt) if full else None
        dy = _rand(g, R, C).to(dt)
        s = _d(x) + _d(ad) if full else _d(x)
        mean, var = s.mean(0), s.var(0, unbiased=False)
        invstd = (var + eps).rsqrt()
        xhat = (s - mean) * invstd
        yref = xhat * _d(gamma) + _d(beta)
        yref = F.relu(yref) if full else yref
        y_in = yref.to(dt).cpu()                                     # the forward output the backward reads its ReLU mask from
        with _arena("test_batchnorm", mb=24 + (10 * R * C * 4 >> 20)) as a:
            t = _ins(a, x=x, ad=ad, dy=dy, gamma=gamma, beta=beta, mean=mean.float().cpu(), invstd=invstd.float().cpu(),
                     y_in=y_in if full else None)
            rm, rv, nbt = a.accum("running_mean", rm0), a.accum("running_var", rv0), a.accum("nbt", torch.tensor(5))
            rm2, rv2, nbt2 = a.accum("running_mean.2", rm0), a.accum("running_var.2", rv0), a.accum("nbt.2", torch.tensor(9))
            y, m1, i1 = a.output("y", (R, C), dt), a.output("mean", (C,)), a.output("invstd", (C,))
            _call("nsdp_bn_train_fwd" + sfx, t["x"], t["ad"], LL(R), C, eps, mom, 2, rm, rv, nbt, t["gamma"], t["beta"], int(full),
                  y, m1, i1, a.workspace("ws.train", nws))
            m2, i2 = a.output("mean.2", (C,)), a.output("invstd.2", (C,))
            _call("nsdp_bn_stats" + sfx, t["x"], t["ad"], LL(R), C, eps, mom, rm2, rv2, m2, i2, a.workspace("ws.stats", nws), nbt2)
            y2 = a.output("y.apply", (R, C), dt)
            _call("nsdp_bn_apply" + sfx, t["x"], t["ad"], t["mean"], t["invstd"], t["gamma"], t["beta"], LL(R), C, int(full), y2)
            outs = [y, m1, i1, m2, i2, y2]
            bwd = {}
            for training in (1, 0):
                dx, dg, db = (a.output(f"dx.{training}", (R, C), dt), a.output(f"dgamma.{training}", (C,)),
                              a.output(f"dbeta.{training}", (C,)))
                _call("nsdp_bn_backward" + sfx, t["dy"], t["y_in"], t["x"], t["ad"], t["mean"], t["invstd"], t["gamma"], LL(R), C,
                      training, dx, dg, db, a.workspace(f"ws.bwd.{training}", nws))
                bwd[training] = (dx, dg, db)
                outs += [dx, dg, db]
            a.check(written=outs)
        for name, got in (("y", y), ("y.apply", y2)):
            if dt is BF:
                _finite(got, name)
                assert bool(((got.double() - yref).abs() <= 2 ** -7 * yref.abs() + 1e-3).all()), name
            else:
                _bn_close(got, yref, dt, name, abs_tol=2e-5)
        for name, got, ref in (("mean", m1, mean), ("invstd", i1, invstd), ("mean.stats", m2, mean), ("invstd.stats", i2, invstd)):
            _bn_close(got, ref, dt, name)
        unb = var * R / (R - 1)
        for n_upd, grm, grv, gn, n0 in ((2, rm, rv, nbt, 5), (1, rm2, rv2, nbt2, 9)):
            erm, erv = _d(rm0), _d(rv0)
            for _ in range(n_upd):
                erm, erv = (1 - mom) * erm + mom * mean, (1 - mom) * erv + mom * unb
            _bn_close(grm, erm, dt, "running_mean", abs_tol=1e-6)
            _bn_close(grv, erv, dt, "running_var", abs_tol=1e-5)
            assert int(gn) == n0 + n_upd
        dyp = _d(dy) * (y_in.to(DEV).double() > 0) if full else _d(dy)
        rdg, rdb = (dyp * xhat).sum(0), dyp.sum(0)
        gi = _d(gamma) * invstd
        for training, rdx in ((1, gi * (dyp - rdb / R - xhat * rdg / R)), (0, gi * dyp)):
            dx, dg, db = bwd[training]
            _bn_close(dx, rdx, dt, f"dx.{training}")
            _bn_close(dg, rdg, dt, f"dgamma.{training}")
            _bn_close(db, rdb, dt, f"dbeta.{training}")


# ---------------------------------------------------------------------------------------------------------------------------------
# attention glue, fp32 and bf16 storage
# ---------------------------------------------------------------------------------------------------------------------------------
ATTN_SHAPES = [(2, 37, 50, 10, 120), (3, 16, 16, 16, 256), (2, 130, 20, 7, 200)]


def _gather(x, idx):      # x [B,N,d], idx [B,n,k] -> [B,n,k,d]
    B, n, k = idx.shape
    return torch.gather(x, 1, idx.reshape(B, n * k, 1).expand(-1, -1, x.shape[-1]).long()).reshape(B, n, k, -1)


def _post_ref(a, val, a_g, v_g, res):
    """y, lse of softmax over the neighbours (and the global token) of the logits a, values val."""
    if a_g is not None:
        B, n, k, d = a.shape
        a = torch.cat([a, a_g[:, None, None, :].expand(B, n, 1, d)], dim=2)
        val = torch.cat([val, v_g[:, None, None, :].expand(B, n, 1, d)], dim=2)
    y = (F.softmax(a, dim=2) * val).sum(dim=2)
    return (y if res is None else y + res), torch.logsumexp(a, dim=2)


def _post_bwd_ref(a, val, a_g, v_g, y_att, lse, dy):
    """The backward of _post_ref from the saved y (without the residual) and lse, as the kernels form it: w = exp(a - lse),
    d(val) = w dy, da = d(val) (val - y); the global token likewise, summed over the centres."""
    w = torch.exp(a - lse.unsqueeze(2))
    dval = w * dy.unsqueeze(2)
    da = dval * (val - y_att.unsqueeze(2))
    if a_g is None:
        return da, dval, None, None
    dvg = torch.exp(a_g.unsqueeze(1) - lse) * dy
    return da, dval, (dvg * (v_g.unsqueeze(1) - y_att)).sum(1), dvg.sum(1)


def _attn_close(got, ref, dt, what, tol, floor=0.0, fwd_atol=None):
    """fp32: tests/test_attention_gpu.py's bounds (`tol`); bf16 storage: tests/test_bf16_gpu.py's (an ulp of bf16 forward, 2e-2 of the
    scale of the du-sized gradients backward)."""
    _finite(got, what)
    err = (got.double() - ref).abs()
    if dt is BF and fwd_atol is not None:
        assert bool((err <= 2 ** -7 * ref.abs() + fwd_atol).all()), what
    elif fwd_atol is not None:                  # forward values in fp32: an absolute bound
        assert float(err.max()) < tol, (what, float(err.max()))
    elif dt is BF:
        assert float(err.max()) <= 2e-2 * (max(float(ref.abs().max()), floor) + 1e-6), (what, float(err.max()))
    else:
        assert float(err.max()) <= tol * (float(ref.abs().max()) + 1.0), (what, float(err.max()))


@pytest.mark.parametrize("dt", [torch.float32, BF], ids=["f32", "bf16"])
@pytest.mark.parametrize("B,n,N,k,d", ATTN_SHAPES)
def test_attention_glue(B, n, N, k, d, dt):
    """pre fwd / bwd (per-point and per-shape queries, with and without the d(pos) accumulator), _sub, post fwd / bwd (with a
    residual; with the global token) and _det with its workspace.  The backward entries read y and lse of the fp64 reference."""
    sfx = "_bf16" if dt is BF else ""
    g = _gen(B * 1000 + n + d)
    mk = lambda *s: _rand(g, *s).to(dt)
    idx = torch.randint(0, N, (B, n, k), generator=g).int()
    q, q1, kf, vf, pos, a_ = mk(B, n, d), mk(B, 1, d), mk(B, N, d), mk(B, N, d), mk(B, n, k, d), mk(B, n, k, d)
    du, dq_sub, acc0, res, a_g, v_g, dy = mk(B, n, k, d), mk(B, n, d), mk(B, n, k, d), mk(B, n, d), mk(B, d), mk(B, d), mk(B, n, d)
    # fp64 references (autograd of the plain composition)
    idx_d = idx.to(DEV)
    u_ref = {qb: _d(qq).expand(B, n, d).unsqueeze(2) - _gather(_d(kf), idx_d) + _d(pos) for qb, qq in ((0, q), (1, q1))}
    dkf_ref = torch.zeros(B, N, d, dtype=torch.float64, device=DEV).scatter_add_(
        1, idx_d.long().reshape(B, n * k, 1).expand(B, n * k, d), -_d(du).reshape(B, n * k, d))
    dq_ref = {0: _d(du).sum(2), 1: _d(du).sum((1, 2)).unsqueeze(1)}
    post = {}
    for glob in (False, True):
        ins = [t.to(DEV).double().requires_grad_(True) for t in ((a_, vf, pos, a_g, v_g) if glob else (a_, vf, pos))]
        yv, lse = _post_ref(ins[0], _gather(ins[1], idx_d) + ins[2], ins[3] if glob else None, ins[4] if glob else None,
                            None if glob else _d(res))
        auto = [t_.detach() for t_ in torch.autograd.grad(yv, ins, _d(dy))]
        yv, lse = yv.detach(), lse.detach()
        val = (_gather(ins[1], idx_d) + ins[2]).detach()
        scat = lambda dval: torch.zeros(B, N, d, dtype=torch.float64, device=DEV).scatter_add_(
            1, idx_d.long().reshape(B, n * k, 1).expand(B, n * k, d), dval.reshape(B, n * k, d))
        ag64, vg64 = (_d(a_g), _d(v_g)) if glob else (None, None)
        rs64 = 0.0 if glob else _d(res)
        da, dval, dag, dvg = _post_bwd_ref(_d(a_), val, ag64, vg64, yv - rs64, lse, _d(dy))
        for mine, theirs in zip((da, scat(dval), dval, dag, dvg), auto):      # the formula IS the derivative (exact y, lse)
            assert float((mine - theirs).abs().max()) <= 1e-9 * (float(theirs.abs().max()) + 1.0)
        # ... and what the kernels are given: y and lse as stored (rounded to the storage type / fp32)
        y_st, lse_st = yv.to(dt), lse.float()
        da, dval, dag, dvg = _post_bwd_ref(_d(a_), val, ag64, vg64, y_st.double() - rs64, lse_st.double(), _d(dy))
        post[glob] = (yv, lse, [da, scat(dval), dval, dag, dvg], y_st.cpu(), lse_st.cpu())
    with _arena("test_attention_glue", mb=160) as a:
        t = _ins(a, q=q, q1=q1, kf=kf, vf=vf, pos=pos, a=a_, du=du, dq_sub=dq_sub, res=res, a_g=a_g, v_g=v_g, dy=dy, idx=idx)
        outs, pre = [], {}
        for qb, qq in ((0, t["q"]), (1, t["q1"])):
            u = a.output(f"u.{qb}", (B, n, k, d), dt)
            _call("nsdp_attn_pre_fwd" + sfx, qq, t["kf"], t["pos"], t["idx"], B, n, N, k, d, qb, u)
            dq, dkf = a.output(f"dq.{qb}", (B, 1 if qb else n, d)), a.output(f"dkf.{qb}", (B, N, d))
            acc = a.accum(f"dpos_acc.{qb}", acc0) if qb == 0 else None
            _call("nsdp_attn_pre_bwd" + sfx, t["du"], t["idx"], B, n, N, k, d, qb, dq, dkf, acc)
            pre[qb] = (u, dq, dkf, acc)
            outs += [u, dq, dkf]
        dq_only = a.output("dq.only", (B, n, d))                     # the dq-only form: dkf and dpos_acc NULL
        _call("nsdp_attn_pre_bwd" + sfx, t["du"], t["idx"], B, n, N, k, d, 0, dq_only, None, None)
        dq_s = a.output("dq.sub", (B, n, d))
        _call("nsdp_attn_pre_bwd_sub" + sfx, t["du"], t["idx"], B, n, N, k, d, t["dq_sub"], dq_s)
        outs += [dq_only, dq_s]
        got = {}
        for glob in (False, True):
            yv, lse, _, y_st, lse_st = post[glob]
            ag, vg, rs = (t["a_g"], t["v_g"], None) if glob else (None, None, t["res"])
            y, ls = a.output(f"y.{glob}", (B, n, d), dt), a.output(f"lse.{glob}", (B, n, d))
            _call("nsdp_attn_post_fwd" + sfx, t["a"], t["vf"], t["pos"], t["idx"], ag, vg, rs, B, n, N, k, d, y, ls)
            y_in, lse_in = a.input(f"y_in.{glob}", y_st), a.input(f"lse_in.{glob}", lse_st)
            da, dpos, dvf = a.output(f"da.{glob}", (B, n, k, d), dt), a.output(f"dpos.{glob}", (B, n, k, d), dt), a.output(f"dvf.{glob}", (B, N, d))
            dag, dvg = (a.output("da_g", (B, d)), a.output("dv_g", (B, d))) if glob else (None, None)
            _call("nsdp_attn_post_bwd" + sfx, t["dy"], t["a"], t["vf"], t["pos"], t["idx"], ag, vg, y_in, rs, lse_in, B, n, N, k, d,
                  da, dpos, dvf, dag, dvg)
            nws = _bytes("nsdp_attn_post_bwd_det_workspace_bytes", B, n, k, d)
            da2, dpos2 = a.output(f"det.da.{glob}", (B, n, k, d), dt), a.output(f"det.dpos.{glob}", (B, n, k, d), dt)
            dag2, dvg2 = (a.output("det.da_g", (B, d)), a.output("det.dv_g", (B, d))) if glob else (None, None)
            _call("nsdp_attn_post_bwd_det" + sfx, t["dy"], t["a"], t["vf"], t["pos"], t["idx"], ag, vg, y_in, rs, lse_in, B, n, N, k, d,
                  da2, dpos2, dag2, dvg2, a.workspace(f"det.ws.{glob}", nws), ctypes.c_size_t(nws))
            got[glob] = (y, ls, da, dpos, dvf, dag, dvg, da2, dpos2, dag2, dvg2)
            outs += [o for o in got[glob] if o is not None]
        a.check(written=outs)
    floor = float(dkf_ref.abs().max())
    for qb in (0, 1):
        u, dq, dkf, acc = pre[qb]
        _attn_close(u, u_ref[qb], dt, f"u.{qb}", 1e-5, fwd_atol=1e-6)
        _attn_close(dq, dq_ref[qb], dt, f"dq.{qb}", 1e-5, floor)
        _attn_close(dkf, dkf_ref, dt, f"dkf.{qb}", 1e-5, floor)
        if acc is not None:
            _attn_close(acc, _d(acc0) + _d(du), dt, "dpos_acc", 1e-5, floor)
    _attn_close(dq_only, dq_ref[0], dt, "dq.only", 1e-5, floor)
    _attn_close(dq_s, dq_ref[0] - _d(dq_sub), dt, "dq.sub", 1e-5, floor)
    for glob in (False, True):
        yv, lse, grads = post[glob][:3]
        y, ls, da, dpos, dvf, dag, dvg, da2, dpos2, dag2, dvg2 = got[glob]
        pfloor = float(grads[2].abs().max())
        _attn_close(y, yv, dt, "y", 2e-5, fwd_atol=1e-3)
        _attn_close(ls, lse, dt, "lse", 2e-5, fwd_atol=1e-3)
        for name, o, r_ in (("da", da, grads[0]), ("dvf", dvf, grads[1]), ("dpos", dpos, grads[2]), ("det.da", da2, grads[0]),
                            ("det.dpos", dpos2, grads[2])):
            _attn_close(o, r_, dt, name, 2e-5, pfloor)
        if glob:
            for name, o, r_ in (("da_g", dag, grads[3]), ("dv_g", dvg, grads[4]), ("det.da_g", dag2, grads[3]), ("det.dv_g", dvg2, grads[4])):
                _attn_close(o, r_, dt, name, 2e-5, pfloor)


@pytest.mark.parametrize("B,n,N,k,d", ATTN_SHAPES)
def test_attention_post_from_u(B, n, N, k, d):
    """nsdp_attn_post_fwd_q / _bwd_q: values = u + vk[idx] - qsub_i."""
    g = _gen(B * 31 + n + d)
    mk = lambda *s: _rand(g, *s)
    idx = torch.randint(0, N, (B, n, k), generator=g).int()
    a_, vk, u, qsub, res, dy = mk(B, n, k, d), mk(B, N, d), mk(B, n, k, d), mk(B, n, d), mk(B, n, d), mk(B, n, d)
    idx_d = idx.to(DEV)
    ins = [t.to(DEV).double().requires_grad_(True) for t in (a_, vk, u)]
    yv, lse = _post_ref(ins[0], ins[2] + _gather(ins[1], idx_d) - _d(qsub).unsqueeze(2), None, None, _d(res))
    grads = torch.autograd.grad(yv, ins, _d(dy))
    with _arena("test_attention_post_from_u", mb=96) as a:
        t = _ins(a, a=a_, vk=vk, u=u, qsub=qsub, res=res, dy=dy, idx=idx, y_in=yv.detach().float().cpu(), lse_in=lse.detach().float().cpu())
        y, ls = a.output("y", (B, n, d)), a.output("lse", (B, n, d))
        _call("nsdp_attn_post_fwd_q", t["a"], t["vk"], t["u"], t["idx"], t["qsub"], t["res"], B, n, N, k, d, y, ls)
        da, dpos, dvf = a.output("da", (B, n, k, d)), a.output("dpos", (B, n, k, d)), a.output("dvf", (B, N, d))
        _call("nsdp_attn_post_bwd_q", t["dy"], t["a"], t["vk"], t["u"], t["idx"], t["qsub"], t["y_in"], t["res"], t["lse_in"],
              B, n, N, k, d, da, dpos, dvf)
        da2, dpos2 = a.output("da.nodvf", (B, n, k, d)), a.output("dpos.nodvf", (B, n, k, d))      # dvf NULL: the caller scatters
        _call("nsdp_attn_post_bwd_q", t["dy"], t["a"], t["vk"], t["u"], t["idx"], t["qsub"], t["y_in"], t["res"], t["lse_in"],
              B, n, N, k, d, da2, dpos2, None)
        a.check(written=[y, ls, da, dpos, dvf, da2, dpos2])
    _attn_close(y, yv.detach(), torch.float32, "y", 2e-5, fwd_atol=1e-3)
    _attn_close(ls, lse.detach(), torch.float32, "lse", 2e-5, fwd_atol=1e-3)
    for name, o, r_ in (("da", da, grads[0]), ("dvf", dvf, grads[1]), ("dpos", dpos, grads[2]), ("da.nodvf", da2, grads[0]),
                        ("dpos.nodvf", dpos2, grads[2])):
        _attn_close(o, r_, torch.float32, name, 2e-5)


@pytest.mark.parametrize("B,n,N,k,d", ATTN_SHAPES)
def test_inverse_lists_and_segment_sums(B, n, N, k, d):
    """nsdp_knn_invert against the exact lists (counting sort, ascending positions), and the four segment sums over those lists."""
    g = _gen(n + N + d)
    E = n * k
    idx = torch.randint(0, N, (B, E), generator=g).int()
    idx[:, ::3] = 5                                                  # one hot source; others stay empty
    order = torch.sort(idx.long(), dim=1, stable=True).indices.int()
    counts = torch.stack([torch.bincount(idx[b].long(), minlength=N) for b in range(B)])
    offs = F.pad(counts.cumsum(1), (1, 0)).int()
    src, addend = _rand(g, B, E, d), _rand(g, B, N, d)
    with _arena("test_inverse_lists_and_segment_sums", mb=96) as a:
        t = _ins(a, idx=idx, offs=offs, order=order, src=src, src_bf=src.to(BF), addend=addend)
        o_out, e_out = a.output("offsets", (B, N + 1), torch.int32), a.output("entries", (B, E), torch.int32)
        _call("nsdp_knn_invert", t["idx"], B, E, N, o_out, e_out)
        sums = {}
        for sfx, s_in in (("", t["src"]), ("_bf16", t["src_bf"])):
            o1, o2 = a.output("sum" + sfx, (B, N, d)), a.output("sum_add" + sfx, (B, N, d))
            _call("nsdp_segment_sum_rows" + sfx, s_in, t["offs"], t["order"], B, E, N, d, -1.0, o1)
            _call("nsdp_segment_sum_rows_add" + sfx, s_in, t["offs"], t["order"], B, E, N, d, -1.0, t["addend"], o2)
            sums[sfx] = (o1, o2)
        a.check(written=[o_out, e_out] + [o for v in sums.values() for o in v])
    assert torch.equal(o_out.cpu(), offs) and torch.equal(e_out.cpu(), order)
    for sfx, s_val in (("", src), ("_bf16", src.to(BF))):
        ref = torch.zeros(B, N, d, dtype=torch.float64, device=DEV).scatter_add_(
            1, idx.to(DEV).long()[:, :, None].expand(B, E, d), -_d(s_val))
        o1, o2 = sums[sfx]
        _finite(o1, "sum"), _finite(o2, "sum_add")
        assert float((o1.double() - ref).abs().max()) <= 1e-5 * (float(ref.abs().max()) + 1)
        assert torch.equal(o2, o1 + addend.to(DEV))                  # bit-identical to the call followed by the addition (scale -1)


@pytest.mark.parametrize("B,rows,N,d,takes", [(3, 1000, 100, 200, {"bf16", "f32"}), (1, 33, 8, 8, {"bf16"}), (1, 33, 8, 20, {"f32"})])
def test_onehot_scatters(B, rows, N, d, takes):
    """Both one-hot scatters are CALLED at every shape; `takes` is what the header promises (fp32: 16 < d <= 208, bf16:
    d % 8 == 0).  Outside its range an entry must refuse before it launches anything -- the library answers, not a predicate
    restated from the wrapper; d = 20 is the narrowest table the fp32 entry takes."""
    from nsdp_amd import _lib, hip_attention as ha
    g = _gen(rows + N + d)
    src = _rand(g, B, rows, d) * torch.exp(2.0 * _rand(g, B, rows, 1))
    idx = torch.randint(0, N, (B, rows), generator=g).int()
    idx[:, : min(rows, N) - 1] = torch.arange(min(rows, N) - 1, dtype=torch.int32)        # (the last table row may stay empty)
    forms = [("bf16", src.to(BF)), ("f32", src)]
    with _arena("test_onehot_scatters") as a:
        t = _ins(a, idx=idx, **{name: s for name, s in forms})
        tables = {}
        for name, _ in forms:
            try:
                tables[name] = ha.onehot_scatter(t[name], t["idx"], N)
            except _lib.NsdpHipError as e:
                assert name not in takes, e
        a.check(written=list(tables.values()))
    assert set(tables) == takes
    forms = [(name, s_) for name, s_ in forms if name in tables]
    sel = idx.to(DEV).long()[:, :, None].expand(-1, -1, d)
    for name, s in forms:
        ref = torch.zeros(B, N, d, dtype=torch.float64, device=DEV).scatter_add_(1, sel, _d(s))
        mag = torch.zeros(B, N, d, dtype=torch.float64, device=DEV).scatter_add_(1, sel, _d(s).abs())
        _finite(tables[name], name)
        # fp32 accumulation of the selected rows in a fixed order: a few ulps of the sum of magnitudes
        assert float(((tables[name].double() - ref).abs() / (mag + 1e-30)).max()) <= 3e-6, name


# ---------------------------------------------------------------------------------------------------------------------------------
# geometry (indices and gathers exact against oracle.pointnet2_ref, index guards hold 0)
# ---------------------------------------------------------------------------------------------------------------------------------
def _cloud(seed, b, n):
    from nsdp_amd import synth
    return np.ascontiguousarray(synth.uniform(seed, "cloud", (b, n, 3), -0.5, 0.5), dtype=np.float32)


def _t(x):
    return torch.from_numpy(np.ascontiguousarray(x))


def _lists(idx2, N):
    """The inverse lists of idx2 [B, E] over N targets (what nsdp_knn_invert builds): offsets [B, N + 1], entries [B, E]."""
    order = torch.sort(idx2.long(), dim=1, stable=True).indices.int()
    counts = torch.stack([torch.bincount(row.long(), minlength=N) for row in idx2])
    return F.pad(counts.cumsum(1), (1, 0)).int(), order


@pytest.mark.parametrize("B,N,m", [(3, 513, 77), (1, 8193, 16)])
def test_fps(B, N, m):
    from oracle import pointnet2_ref as ref
    xyz = _cloud(N * 7 + m, B, N)
    with _arena("test_fps") as a:
        x = a.input("xyz", _t(xyz))
        tmp = a.workspace("tmp", B * N * 4) if N > 8192 else None     # (B, N) f32, only touched when N > 8192
        out = a.output("idx", (B, m), torch.int32)
        _call("nsdp_furthest_point_sampling", x, B, N, m, tmp, out)
        a.check(written=[out])
    np.testing.assert_array_equal(out.cpu().numpy(), ref.furthest_point_sampling(xyz, m))


@pytest.mark.parametrize("B,n,m,k", [(2, 5, 9, 3), (2, 257, 1025, 5), (2, 70, 70, 64)])
def test_knn(B, n, m, k):
    from oracle import pointnet2_ref as ref
    q = _cloud(n + k, B, n)
    s = q if n == m else _cloud(m + 5 * k, B, m)
    with _arena("test_knn") as a:
        t = _ins(a, q=_t(q), s=_t(s))
        idx, d2 = a.output("idx", (B, n, k), torch.int32), a.output("dist2", (B, n, k))
        _call("nsdp_knn", t["q"], t["s"], B, n, m, k, idx, d2)
        idx_only = a.output("idx.only", (B, n, k), torch.int32)
        _call("nsdp_knn", t["q"], t["s"], B, n, m, k, idx_only, None)
        a.check(written=[idx, d2, idx_only])
    ridx, rd2 = ref.knn(q, s, k, return_dist=True)
    np.testing.assert_array_equal(idx.cpu().numpy(), ridx)
    np.testing.assert_array_equal(idx_only.cpu().numpy(), ridx)
    assert np.array_equal(d2.cpu().numpy().view(np.uint32), rd2.view(np.uint32))


@pytest.mark.parametrize("nsample", [32, 65])
def test_ball_query(nsample):
    from oracle import pointnet2_ref as ref
    B, N, M, radius = 2, 1025, 65, 0.3
    xyz, new_xyz = _cloud(100 + N, B, N), _cloud(200 + M, B, M)
    with _arena("test_ball_query") as a:
        t = _ins(a, xyz=_t(xyz), new_xyz=_t(new_xyz))
        out = a.output("idx", (B, M, nsample), torch.int32)
        _call("nsdp_ball_query", t["new_xyz"], t["xyz"], B, N, M, float(radius), nsample, out)
        a.check(written=[out])
    np.testing.assert_array_equal(out.cpu().numpy(), ref.ball_query(new_xyz, xyz, radius, nsample))


@pytest.mark.parametrize("B,n,m", [(2, 65, 1025), (1, 50, 1)])
def test_three_nn(B, n, m):
    from oracle import pointnet2_ref as ref
    unknown, known = _cloud(300 + n, B, n), _cloud(400 + m, B, m)
    with _arena("test_three_nn") as a:
        t = _ins(a, u=_t(unknown), k=_t(known))
        d2, idx = a.output("dist2", (B, n, 3)), a.output("idx", (B, n, 3), torch.int32)
        _call("nsdp_three_nn", t["u"], t["k"], B, n, m, d2, idx)
        a.check(written=[d2] + ([idx] if m >= 3 else []))      # (fewer than three known points: the oracle says what the slots hold)
    rd2, ridx = ref.three_nn(unknown, known)
    np.testing.assert_array_equal(idx.cpu().numpy(), ridx)
    np.testing.assert_array_equal(d2.cpu().numpy(), rd2)


@pytest.mark.parametrize("B,C,N,M,NS", [(3, 13, 1000, 257, 3), (2, 6, 8192, 2048, 32)])
def test_gather_group_interpolate(B, C, N, M, NS):
    """gather / group / three_interpolate and their gradients, atomic and list forms ((2, 6, 8192, 2048, 32): rows of 65536 entries,
    the sliced list kernel).  The gradient entries zero-fill their output themselves."""
    from nsdp_amd import _lib, synth
    from oracle import pointnet2_ref as ref
    L = _lib.lib()
    feats = synth.normal(41, "feats", (B, C, N)).astype(np.float32)
    idx = (synth.uniform01(42, "idx", (B, M)) * N).astype(np.int32)
    gidx = (synth.uniform01(43, "gidx", (B, M, NS)) * N).astype(np.int32)
    gidx[:, : M // 3, 0] = N - 1                                     # a hot source point
    iidx = (synth.uniform01(52, "i", (B, M, 3)) * N).astype(np.int32)
    w = synth.uniform(53, "w", (B, M, 3), 0.0, 1.0).astype(np.float32)
    go_g = synth.normal(44, "go", (B, C, M)).astype(np.float32)
    go_gr = synth.normal(45, "go2", (B, C, M, NS)).astype(np.float32)
    E = M * NS
    offs_g, ent_g = _lists(_t(idx), N)
    offs_gr, ent_gr = _lists(_t(gidx).reshape(B, E), N)
    offs_i, ent_i = _lists(_t(iidx).reshape(B, 3 * M), N)
    with _arena("test_gather_group_interpolate", mb=128) as a:
        t = _ins(a, feats=_t(feats), idx=_t(idx), gidx=_t(gidx), iidx=_t(iidx), w=_t(w), go_g=_t(go_g), go_gr=_t(go_gr),
                 offs_g=offs_g, ent_g=ent_g, offs_gr=offs_gr, ent_gr=ent_gr, offs_i=offs_i, ent_i=ent_i)
        o = {"gather": a.output("gather", (B, C, M)), "group": a.output("group", (B, C, M, NS)), "interp": a.output("interp", (B, C, M))}
        _call("nsdp_gather_points", t["feats"], t["idx"], B, C, N, M, o["gather"])
        _call("nsdp_group_points", t["feats"], t["gidx"], B, C, N, M, NS, o["group"])
        _call("nsdp_three_interpolate", t["feats"], t["iidx"], t["w"], B, C, N, M, o["interp"])
        for name in ("gather_grad", "group_grad", "interp_grad"):
            o[name] = a.output(name, (B, C, N))
        _call("nsdp_gather_points_grad", t["go_g"], t["idx"], B, C, N, M, o["gather_grad"])
        _call("nsdp_group_points_grad", t["go_gr"], t["gidx"], B, C, N, M, NS, o["group_grad"])
        _call("nsdp_three_interpolate_grad", t["go_g"], t["iidx"], t["w"], B, C, M, N, o["interp_grad"])
        assert L.nsdp_scatter_cm_lists_supported(B, C, N, M) and L.nsdp_scatter_cm_lists_supported(B, C, N, E)
        assert L.nsdp_three_interpolate_grad_lists_supported(B, C, M, N)
        for name in ("gather_lists", "group_lists", "interp_lists"):
            o[name] = a.output(name, (B, C, N))
        _call("nsdp_scatter_cm_lists", t["go_g"], t["offs_g"], t["ent_g"], B, C, N, M, o["gather_lists"])
        _call("nsdp_scatter_cm_lists", t["go_gr"], t["offs_gr"], t["ent_gr"], B, C, N, E, o["group_lists"])
        _call("nsdp_three_interpolate_grad_lists", t["go_g"], t["w"], t["offs_i"], t["ent_i"], B, C, M, N, o["interp_lists"])
        a.check(written=list(o.values()))
    got = {k_: v.cpu().numpy() for k_, v in o.items()}
    np.testing.assert_array_equal(got["gather"], ref.gather_points(feats, idx))
    np.testing.assert_array_equal(got["group"], ref.group_points(feats, gidx))
    np.testing.assert_array_equal(got["interp"], ref.three_interpolate(feats, iidx, w))
    want = {"gather": ref.gather_points_grad(go_g, idx, N), "group": ref.group_points_grad(go_gr, gidx, N),
            "interp": ref.three_interpolate_grad(go_g, iidx, w, N)}
    for name, wv in want.items():
        for form in ("_grad", "_lists"):
            assert np.isfinite(got[name + form]).all(), name + form
            np.testing.assert_allclose(got[name + form], wv, rtol=1e-5, atol=1e-5 * max(1.0, float(np.abs(wv).max())), err_msg=name + form)


@pytest.mark.parametrize("C", [3, 120, 256])
def test_row_gather_scatter_and_rel_coords(C):
    from nsdp_amd import synth
    B, N, S, n, k = 2, 300, 90, 64, 7
    pts = synth.normal(50 + C, "p", (B, N, C)).astype(np.float32)
    idx = (synth.uniform01(51 + C, "i", (B, S)) * N).astype(np.int32)
    go = synth.normal(52 + C, "g", (B, S, C)).astype(np.float32)
    q, s_ = _cloud(61 + C, B, n), _cloud(62 + C, B, N)
    nidx = (synth.uniform01(63, "i", (B, n, k)) * N).astype(np.int32)
    with _arena("test_row_gather_scatter_and_rel_coords") as a:
        t = _ins(a, pts=_t(pts), idx=_t(idx), go=_t(go), q=_t(q), s=_t(s_), nidx=_t(nidx))
        rows, grad = a.output("rows", (B, S, C)), a.output("grad", (B, N, C))
        _call("nsdp_gather_rows", t["pts"], t["idx"], B, N, C, S, rows)
        _call("nsdp_scatter_add_rows", t["go"], t["idx"], B, N, C, S, grad)           # (zero-filled first by the entry itself)
        rel = {sign: a.output(f"rel4.{sign}", (B, n, k, 4)) for sign in (1.0, -1.0)}
        for sign, out in rel.items():
            _call("nsdp_rel_coords4", t["q"], t["s"], t["nidx"], B, n, N, k, sign, out)
        a.check(written=[rows, grad] + list(rel.values()))
    np.testing.assert_array_equal(rows.cpu().numpy(), np.take_along_axis(pts, idx[..., None].astype(np.int64), axis=1))
    want = np.zeros_like(pts)
    for b in range(B):
        np.add.at(want[b], idx[b], go[b])
    np.testing.assert_allclose(grad.cpu().numpy(), want, rtol=1e-5, atol=1e-6)
    gathered = np.take_along_axis(s_[:, None, :, :].repeat(n, 1), nidx[..., None].astype(np.int64), axis=2)
    for sign, out in rel.items():
        got = out.cpu().numpy()
        np.testing.assert_array_equal(got[..., :3], (q[:, :, None, :] - gathered) if sign > 0 else (gathered - q[:, :, None, :]))
        assert not got[..., 3].any()


@pytest.mark.parametrize("counts,n_max", [((301, 0, 1, 257), 512), ((8193, 700), 8193)])
def test_ragged_geometry(counts, n_max):
    """The three packed entries with cap > total: per shape the bits of the rectangular entries (through the oracle), rows at or
    beyond offsets[B] left alone -- they must still hold the poison."""
    from oracle import pointnet2_ref as ref
    B, total = len(counts), sum(counts)
    cap, m, k, ns = total + 300, 16, 7, 5
    clouds = [_cloud(70 + b, 1, n_b)[0] for b, n_b in enumerate(counts)]
    packed = np.zeros((cap, 3), np.float32)
    packed[:total] = np.concatenate(clouds)
    offsets = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    anchors = _cloud(72, B, m)
    rq = _cloud(73, B, 33)                                           # rectangular queries against the packed sources
    big = n_max > 8192
    with _arena("test_ragged_geometry") as a:
        t = _ins(a, packed=_t(packed), offsets=_t(offsets), anchors=_t(anchors), rq=_t(rq))
        idx, d2 = a.output("knn_ragged.idx", (cap, k), torch.int32, rows=total), a.output("knn_ragged.d2", (cap, k), rows=total)
        _call("nsdp_knn_ragged", t["packed"], t["offsets"], t["anchors"], B, cap, m, k, idx, d2)
        fps = a.output("fps_ragged.idx", (B, ns), torch.int32)
        tmp = a.workspace("fps_ragged.tmp", cap * 4) if big else None
        _call("nsdp_furthest_point_sampling_ragged", t["packed"], t["offsets"], B, cap, n_max, ns, tmp, fps)
        written = [idx[:total], d2[:total], fps]
        if not big:
            ks = 1                                                   # (k <= every non-empty shape's row count)
            sidx, sd2 = a.output("self.idx", (cap, ks), torch.int32, rows=total), a.output("self.d2", (cap, ks), rows=total)
            _call("nsdp_knn_ragged_source", t["packed"], t["offsets"], t["packed"], t["offsets"], B, 0, cap, cap, n_max, ks, sidx, sd2)
            written += [sidx[:total], sd2[:total]]
        else:
            ridx_o, rd2_o = a.output("rect.idx", (B, 33, k), torch.int32), a.output("rect.d2", (B, 33, k))
            _call("nsdp_knn_ragged_source", t["rq"], None, t["packed"], t["offsets"], B, 33, 0, cap, n_max, k, ridx_o, rd2_o)
            written += [ridx_o, rd2_o]
        a.check(written=written)
    assert bool((idx[total:] == -1).all()) and bool(torch.isnan(d2[total:]).all())
    lo = 0
    for b, n_b in enumerate(counts):
        if n_b:
            wi, wd = ref.knn(clouds[b][None], anchors[b:b + 1], k, return_dist=True)
            np.testing.assert_array_equal(idx[lo:lo + n_b].cpu().numpy(), wi[0])
            assert np.array_equal(d2[lo:lo + n_b].cpu().numpy().view(np.uint32), wd[0].view(np.uint32))
            np.testing.assert_array_equal(fps[b].cpu().numpy() - lo, ref.furthest_point_sampling(clouds[b][None], ns)[0])
            if not big:
                wi, wd = ref.knn(clouds[b][None], clouds[b][None], ks, return_dist=True)
                np.testing.assert_array_equal(sidx[lo:lo + n_b].cpu().numpy() - lo, wi[0])
                assert np.array_equal(sd2[lo:lo + n_b].cpu().numpy().view(np.uint32), wd[0].view(np.uint32))
            else:
                wi, wd = ref.knn(rq[b:b + 1], clouds[b][None], k, return_dist=True)
                np.testing.assert_array_equal(ridx_o[b].cpu().numpy() - lo, wi[0])
                assert np.array_equal(rd2_o[b].cpu().numpy().view(np.uint32), wd[0].view(np.uint32))
        else:
            assert bool((fps[b] == min(lo, cap - 1)).all())          # a shape without rows: offsets[b] in every slot
        lo += n_b
    if not big:
        assert bool((sidx[total:] == -1).all()) and bool(torch.isnan(sd2[total:]).all())


# ---------------------------------------------------------------------------------------------------------------------------------
# fused decoder
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,NQ,A", [(1, 1, 7), (3, 333, 32)])
def test_fused_decoder(B, NQ, A):
    """The four fused entries through hip_decoder with the queries, the encoding, the weight packs, the tables and the outputs in
    the arena.  fp32 against the oracle (1e-4, tests/test_decoder_gpu.py); bf16 operands within 0.1 of the fp32 kernel everywhere
    and, where there are rows enough for the statistic, no worse than 1.25 x the layered bf16 decoder (tests/test_decoder_bf16_gpu.py);
    the packed forms give every row the rectangular call's bits and leave the rows beyond the total alone."""
    from nsdp_amd import hip_decoder, precision
    # The memory contract of the four entries does not depend on the process's knobs: fp32 storage and the fused decoder are
    # switched on for the test (the modes are selected below) and put back behind it.
    with contextlib.ExitStack() as cfg:
        cfg.enter_context(precision.storage(torch.float32))
        cfg.callback(setattr, hip_decoder, "ENABLED", hip_decoder.ENABLED)
        hip_decoder.ENABLED = True
        _fused_decoder_case(B, NQ, A)


def _fused_decoder_case(B, NQ, A):
    from helpers import l2_err
    from nsdp_amd import hip_decoder, precision
    from nsdp_amd.ragged import RaggedPoints
    from oracle import tdnet_ref
    from test_decoder_gpu import KW, _decoder, _inputs
    dec, state = _decoder(11)
    dec = dec.to(DEV)
    xyz_q, anchors, feats, z = _inputs(5, B, NQ, A)
    counts = [NQ, max(NQ - 17, 0), 1][:B]
    total, cap = sum(counts), sum(counts) + 40
    packed = np.zeros((cap, 3), np.float32)
    packed[:total] = np.concatenate([xyz_q[b, :n_b] for b, n_b in enumerate(counts)])
    offsets = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    out = {}
    with _arena("test_fused_decoder", mb=96) as a:
        t = _ins(a, xyz_q=_t(xyz_q), anchors=_t(anchors), feats=_t(feats), z=_t(z), packed=_t(packed), offsets=_t(offsets))
        enc = {"z": t["z"], "anchors": t["anchors"], "anchor_feats": t["feats"]}
        pts = RaggedPoints(t["packed"], t["offsets"], counts)
        written = []
        for mode, frag in (("f32", hip_decoder._frag), ("bf16", hip_decoder._frag_bf16)):
            pack = hip_decoder._Pack(frag).get(dec)                  # the weight packs as arena inputs
            pack.tensors = [a.input(f"weights.{mode}[{i}]", w.cpu()) for i, w in enumerate(pack.tensors)]
            pack.ptrs = (ctypes.c_void_p * len(pack.tensors))(*[w.data_ptr() for w in pack.tensors])
            dec.__dict__["_fused_pack_bf16" if mode == "bf16" else "_fused_pack"] = pack
            with torch.no_grad(), hip_decoder.mode(mode):
                rect = hip_decoder.decoder_forward(dec, t["xyz_q"], enc)
                rag = a.output(f"ragged.out.{mode}", (cap, 3), rows=total)
                hip_decoder.decoder_forward_ragged(dec, pts, enc, out=rag)
            out[mode] = (rect, rag)
            written += [rect, rag[:total]]
        a.check(written=written)
    enc_d = {"z": _t(z).to(DEV), "anchors": _t(anchors).to(DEV), "anchor_feats": _t(feats).to(DEV)}
    for mode, (rect, rag) in out.items():
        _finite(rect, mode)
        lo = 0
        for b, n_b in enumerate(counts):
            assert torch.equal(rag[lo:lo + n_b], rect[b, :n_b]), (mode, b)
            lo += n_b
        assert bool(torch.isnan(rag[total:]).all()), mode
    sd = tdnet_ref._SD({k_: torch.from_numpy(v) for k_, v in state.items()}, "", False)
    enc_cpu = {"z": _t(z), "anchors": _t(anchors), "anchor_feats": _t(feats)}
    oracle = tdnet_ref.cross_transformer_decoder(sd, _t(xyz_q), enc_cpu, KW).numpy()
    f32, b16 = out["f32"][0].cpu().numpy(), out["bf16"][0].cpu().numpy()
    assert l2_err(f32, oracle) <= 1e-4
    assert float(np.abs(b16 - f32).max()) < 0.1
    if NQ >= 333:
        for slot in ("_fused_pack", "_fused_pack_bf16"):
            dec.__dict__.pop(slot, None)
        enc16 = dict(enc_d, z=enc_d["z"].to(BF), anchor_feats=enc_d["anchor_feats"].to(BF))
        with torch.no_grad(), hip_decoder.mode("f32"), precision.storage(BF):
            layered = dec(_t(xyz_q).to(DEV), enc16).float().cpu().numpy()
        e_new, e_lay = l2_err(b16, f32), l2_err(layered, f32)
        assert e_lay > 0 and e_new <= 1.25 * e_lay, (e_new, e_lay)


# ---------------------------------------------------------------------------------------------------------------------------------
# Adam, device query, and the accounting of this file
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("weight_decay,misaligned,lr_tensor", [(0.0, False, False), (0.01, True, True)])
def test_adam(weight_decay, misaligned, lr_tensor):
    """One nsdp_adam_multi_f32 launch over the shape list of tests/test_adam_gpu.py (every other tensor a view 4 bytes into its
    allocation when `misaligned`), from a state of three earlier steps, against the update in fp64; `done` is zero on exit."""
    from nsdp_amd import _lib, hip_adam
    from test_adam_gpu import SHAPES
    lr, b1, b2, eps, step0 = 5e-4, 0.9, 0.999, 1e-8, 3.0
    g = _gen(3)
    chunk = int(_lib.lib().nsdp_adam_chunk_elems())
    host, rows = [], []
    with _arena("test_adam") as a:
        for i, shp in enumerate(SHAPES):
            n = int(np.prod(shp))
            off = 1 if (misaligned and i % 2 == 1) else 0
            vals = {"param": _rand(g, n + off), "grad": _rand(g, n + off) * 10.0 ** ((i % 5) - 3), "exp_avg": _rand(g, n + off) * 1e-2,
                    "exp_avg_sq": _rand(g, n + off).square() * 1e-3}
            dev = {k_: (a.input if k_ == "grad" else a.accum)(f"{k_}[{i}]", v) for k_, v in vals.items()}
            step = a.accum(f"step[{i}]", torch.tensor(step0))
            host.append((vals, dev, step, off, n))
            rows.append(tuple(dev[k_][off:].data_ptr() for k_ in ("param", "grad", "exp_avg", "exp_avg_sq")) + (step.data_ptr(), n))
        descs = np.array(rows, dtype=hip_adam._DESC_DTYPE)
        counts = (descs["numel"] + chunk - 1) // chunk
        tensor_of = np.repeat(np.arange(len(rows), dtype=np.int32), counts)
        chunk_of = (np.arange(tensor_of.size) - np.repeat(np.cumsum(counts) - counts, counts)).astype(np.int32)
        chunks = np.stack([tensor_of, chunk_of], axis=1).astype(np.int32)
        # (zero guards: an over-read of the chunk list names chunk 0 of tensor 0, of the descriptors a null pointer's row)
        d_dev = a.input("descs", torch.from_numpy(descs.view(np.uint8).reshape(-1).copy()).view(torch.int64))
        c_dev = a.input("chunks", torch.from_numpy(chunks))
        done = a.accum("done", torch.zeros(len(rows), dtype=torch.int32))
        lr_dev = a.input("lr", torch.tensor(lr, dtype=torch.float32)) if lr_tensor else None
        _call("nsdp_adam_multi_f32", d_dev, c_dev, int(chunks.shape[0]), done, lr_dev, ctypes.c_double(0.0 if lr_tensor else lr),
              ctypes.c_double(b1), ctypes.c_double(b2), ctypes.c_double(eps), ctypes.c_double(weight_decay), 0)
        a.check()
    assert int(done.abs().sum()) == 0
    lr = float(torch.tensor(lr, dtype=torch.float32)) if lr_tensor else lr
    for i, (vals, dev, step, off, n) in enumerate(host):
        p, gr, m, v = (vals[k_].double() for k_ in ("param", "grad", "exp_avg", "exp_avg_sq"))
        gr = gr + weight_decay * p
        m = m + (1 - b1) * (gr - m)
        v = b2 * v + (1 - b2) * gr * gr
        tt = step0 + 1
        p = p - (lr / (1 - b1 ** tt)) * m / (v.sqrt() / (1 - b2 ** tt) ** 0.5 + eps)
        assert float(step) == tt
        for name, want in (("param", p), ("exp_avg", m), ("exp_avg_sq", v)):
            got = dev[name].cpu()
            _finite(got, name)
            if off:
                assert torch.equal(got[:1], vals[name][:1]), f"{name}[{i}]: the element in front of the view changed"
            if name == "param":
                torch.testing.assert_close(got[off:], want[off:].float(), rtol=0, atol=6e-7)
            else:
                torch.testing.assert_close(got[off:], want[off:].float(), rtol=1e-6, atol=4e-7 * float(want.abs().max()))


def test_device_count():
    from nsdp_amd import _lib
    with _arena("test_device_count", mb=2):
        assert _lib.lib().nsdp_device_count() == torch.cuda.device_count() >= 1


def test_every_claimed_entry_was_called(request):
    """COVERAGE against the recording proxy: every test of the table that this session selected (all of them when the file is
    run whole) did enter its arena -- one that skipped, or left before it, is reported -- and every entry the table assigns to
    it was fetched from the library inside that arena."""
    selected = {getattr(item, "originalname", None) or item.name for item in request.session.items
                if item.fspath == request.node.fspath}
    absent = sorted(t for t in set(COVERAGE.values()) if t in selected and t not in _SEEN)
    assert not absent, f"selected, but never entered the arena (skipped?): {absent}"
    missing = {e: t for e, t in COVERAGE.items() if t in _SEEN and e not in _SEEN[t]}
    assert not missing, missing
