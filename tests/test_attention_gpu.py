"""Fused vector-attention glue kernels vs a plain PyTorch composition of the same ops (fwd + bwd)."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def _gather(x, idx):  # x [B,N,d], idx [B,n,k] -> [B,n,k,d]
    B, n, k = idx.shape
    return torch.gather(x, 1, idx.reshape(B, n * k, 1).expand(-1, -1, x.shape[-1]).long()).reshape(B, n, k, -1)


def _ref_pre(q, kf, pos, idx):
    return q.unsqueeze(2) - _gather(kf, idx) + pos


def _ref_post(a, vf, pos, idx, a_g, v_g, residual):
    val = pos if vf is None else _gather(vf, idx) + pos
    if a_g is not None:
        B, n, k, d = a.shape
        a = torch.cat([a, a_g[:, None, None, :].expand(B, n, 1, d)], dim=2)
        val = torch.cat([val, v_g[:, None, None, :].expand(B, n, 1, d)], dim=2)
    y = (F.softmax(a, dim=2) * val).sum(dim=2)
    return y if residual is None else y + residual


@pytest.mark.parametrize("B,n,N,k,d", [(2, 37, 50, 10, 120), (3, 16, 16, 16, 256), (1, 100, 100, 100, 256),
                                       (2, 130, 20, 7, 200), (1, 5, 9, 3, 8)])
def test_attn_pre(B, n, N, k, d):
    from nsdp_amd.hip_attention import attn_pre
    g = torch.Generator().manual_seed(B * 1000 + n + d)
    q = torch.randn(B, n, d, generator=g).to(DEV).double().requires_grad_(True)
    kf = torch.randn(B, N, d, generator=g).to(DEV).double().requires_grad_(True)
    pos = torch.randn(B, n, k, d, generator=g).to(DEV).double().requires_grad_(True)
    idx = torch.randint(0, N, (B, n, k), generator=g).to(DEV).int()
    ref = _ref_pre(q, kf, pos, idx)
    qf, kff, posf = (t.detach().float().requires_grad_(True) for t in (q, kf, pos))
    out = attn_pre(qf, kff, posf, idx)
    assert float((out.double() - ref).abs().max()) < 1e-5
    go = torch.randn(B, n, k, d, generator=g).to(DEV)
    gr = torch.autograd.grad(ref, [q, kf, pos], go.double())
    gm = torch.autograd.grad(out, [qf, kff, posf], go)
    for a_, e_ in zip(gm, gr):
        assert float((a_.double() - e_).abs().max()) <= 1e-5 * (float(e_.abs().max()) + 1.0)


@pytest.mark.parametrize("B,n,N,k,d,has_v,has_g,has_res", [
    (2, 37, 50, 10, 120, True, False, True), (2, 33, 40, 10, 120, False, False, False),
    (3, 16, 16, 16, 256, True, False, True), (1, 100, 100, 100, 256, True, False, True),
    (2, 130, 20, 7, 200, True, True, False), (1, 5, 9, 3, 8, True, True, True)])
def test_attn_post(B, n, N, k, d, has_v, has_g, has_res):
    from nsdp_amd.hip_attention import attn_post
    g = torch.Generator().manual_seed(B * 77 + n + d + k)
    mk = lambda *s: torch.randn(*s, generator=g).to(DEV).double().requires_grad_(True)
    a, pos = mk(B, n, k, d), mk(B, n, k, d)
    vf = mk(B, N, d) if has_v else None
    a_g, v_g = (mk(B, d), mk(B, d)) if has_g else (None, None)
    res = mk(B, n, d) if has_res else None
    idx = torch.randint(0, N, (B, n, k), generator=g).to(DEV).int()
    ref = _ref_post(a, vf, pos, idx, a_g, v_g, res)
    f32 = lambda t: None if t is None else t.detach().float().requires_grad_(True)
    af, vff, posf, agf, vgf, resf = map(f32, (a, vf, pos, a_g, v_g, res))
    out = attn_post(af, vff, posf, idx, agf, vgf, resf)
    assert float((out.double() - ref).abs().max()) < 2e-5
    go = torch.randn(B, n, d, generator=g).to(DEV)
    ins64 = [t for t in (a, vf, pos, a_g, v_g, res) if t is not None]
    ins32 = [t for t in (af, vff, posf, agf, vgf, resf) if t is not None]
    gr = torch.autograd.grad(ref, ins64, go.double())
    gm = torch.autograd.grad(out, ins32, go)
    for a_, e_ in zip(gm, gr):
        assert float((a_.double() - e_).abs().max()) <= 2e-5 * (float(e_.abs().max()) + 1.0), a_.shape


def test_attn_pre_query_per_shape():
    """Decoder form: one query vector per shape, (B,1,d), shared by all centres."""
    from nsdp_amd.hip_attention import attn_pre
    g = torch.Generator().manual_seed(5)
    B, n, N, k, d = 3, 300, 100, 7, 200
    q = torch.randn(B, 1, d, generator=g).to(DEV).requires_grad_(True)
    kf = torch.randn(B, N, d, generator=g).to(DEV).requires_grad_(True)
    pos = torch.randn(B, n, k, d, generator=g).to(DEV).requires_grad_(True)
    idx = torch.randint(0, N, (B, n, k), generator=g).to(DEV).int()
    out = attn_pre(q, kf, pos, idx)
    q64, kf64, pos64 = (t.detach().double().requires_grad_(True) for t in (q, kf, pos))
    ref = _ref_pre(q64.expand(B, n, d), kf64, pos64, idx)
    assert float((out.double() - ref).abs().max()) < 1e-5
    go = torch.randn(B, n, k, d, generator=g).to(DEV)
    gm = torch.autograd.grad(out, [q, kf, pos], go)
    gr = torch.autograd.grad(ref, [q64, kf64, pos64], go.double())
    for a_, e_ in zip(gm, gr):
        assert a_.shape == e_.shape
        assert float((a_.double() - e_).abs().max()) <= 2e-5 * (float(e_.abs().max()) + 1.0)


@pytest.mark.parametrize("B,n,N,k,d,per_shape", [
    (2, 96, 40, 8, 32, False),         # generic kernel
    (2, 640, 100, 16, 64, False),      # LDS-table kernel (n >= 4 N)
    (3, 4096, 100, 7, 200, True),      # decoder form: register-table scatter
])
def test_pos_gradient_link_matches_autograd_sum(B, n, N, k, d, per_shape):
    """d(pos) handed from attn_post to attn_pre (summed inside the attn_pre_bwd kernel) == autograd's own sum."""
    from nsdp_amd.hip_attention import attn_post, attn_pre, pos_grad_link
    g = torch.Generator().manual_seed(B * n + d)
    mk = lambda *s: torch.randn(*s, generator=g).to(DEV)
    q0, kf0, vf0, pos0 = mk(B, 1 if per_shape else n, d), mk(B, N, d), mk(B, N, d), mk(B, n, k, d)
    w = mk(d, d) * 0.2
    idx = torch.randint(0, N, (B, n, k), generator=g).to(DEV).int()
    go = mk(B, n, d)

    def run(use_link):
        q, kf, vf, pos = (t.clone().requires_grad_(True) for t in (q0, kf0, vf0, pos0))
        link = pos_grad_link() if use_link else None
        u = attn_pre(q, kf, pos, idx, link)
        out = attn_post(u @ w, vf, pos, idx, link=link)
        return torch.autograd.grad(out, [q, kf, vf, pos], go)

    plain, fused = run(False), run(True)
    for a_, e_ in zip(fused, plain):
        assert a_.shape == e_.shape
        # (dq / dkf come from fp32 atomics in both runs: summation order, not the hand-over, sets this tolerance)
        assert float((a_ - e_).abs().max()) <= 2e-5 * (float(e_.abs().max()) + 1.0)
    assert torch.equal(fused[3], plain[3])        # d(pos): the same two addends, added once, in either path


@pytest.mark.parametrize("B,n,N,k,d", [(2, 300, 700, 16, 120), (3, 64, 2048, 10, 120), (1, 500, 500, 16, 256)])
def test_inverse_lists_and_segment_sum(B, n, N, k, d):
    """nsdp_knn_invert / nsdp_segment_sum_rows: complete, sorted lists; the scatter-add they replace; determinism."""
    from nsdp_amd import hip_attention as ha
    g = torch.Generator().manual_seed(n + N)
    idx = torch.randint(0, N, (B, n, k), generator=g, dtype=torch.int32).to(DEV)
    idx[:, :, 0] = 5                                     # one hot source, many empty ones
    off, ent = ha.inverse_lists(idx, N)
    off_c, ent_c, flat = off.cpu(), ent.cpu(), idx.reshape(B, -1).cpu()
    from list_sum_ref import inverse_lists_ref
    want_off, want_ent = inverse_lists_ref(flat.numpy(), N)      # every list, whole: the stable sort of e by idx[b][e]
    assert torch.equal(off_c, torch.from_numpy(want_off)) and torch.equal(ent_c, torch.from_numpy(want_ent))
    for b in range(B):
        assert off_c[b, 0] == 0 and off_c[b, N] == n * k
        assert torch.equal(torch.sort(ent_c[b]).values, torch.arange(n * k, dtype=torch.int32))     # a permutation
        for s_ in (0, 5, N - 1, int(flat[b, 7])):
            lst = ent_c[b, off_c[b, s_]:off_c[b, s_ + 1]]
            assert bool((flat[b, lst.long()] == s_).all()) and bool((lst[1:] > lst[:-1]).all())      # right rows, ascending
        assert torch.equal(torch.bincount(flat[b].long(), minlength=N).int(), (off_c[b, 1:] - off_c[b, :-1]))
    for dt in (torch.float32, torch.bfloat16):
        src = torch.randn(B, n, k, d, generator=g).to(dt).to(DEV)
        out = ha.segment_sum(src, idx, N, -1.0)
        ref = torch.zeros(B, N, d, dtype=torch.float64, device=DEV)
        ref.scatter_add_(1, idx.long().reshape(B, n * k, 1).expand(B, n * k, d), -src.double().reshape(B, n * k, d))
        assert float((out.double() - ref).abs().max()) <= 1e-5 * (float(ref.abs().max()) + 1)
        assert torch.equal(out, ha.segment_sum(src, idx, N, -1.0))


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16])
def test_folded_corrections_of_the_pre_backward_are_the_separate_launches_bit_for_bit(dt):
    """nsdp_segment_sum_rows_add / nsdp_attn_pre_bwd_sub: `out = -sum + addend` and `dq = sum_j du - dy` inside the kernels against
    the plain calls followed by the elementwise launches they replace (hip_attention._AttnPre.backward, NSDP_FOLD_PRE_BWD)."""
    import ctypes
    from nsdp_amd import hip_attention as ha
    B, n, N, k, d = 3, 257, 700, 16, 120
    g = torch.Generator().manual_seed(11)
    idx = torch.randint(0, N, (B, n, k), generator=g, dtype=torch.int32).to(DEV)
    du = torch.randn(B, n, k, d, generator=g).to(dt).to(DEV)
    dvf = torch.randn(B, N, d, generator=g).to(DEV)
    dy = torch.randn(B, n, d, generator=g).to(dt).to(DEV)
    want = ha.segment_sum(du, idx, N, -1.0).add_(dvf)
    assert torch.equal(ha.segment_sum(du, idx, N, -1.0, addend=dvf), want)
    L = ha.lib()
    ci = ctypes.c_int
    dq0 = torch.empty(B, n, d, device=DEV)
    dq1 = torch.empty(B, n, d, device=DEV)
    ha.check(ha._fn("nsdp_attn_pre_bwd", dt)(ha._p(du, dt), ha.iptr(idx), ci(B), ci(n), ci(N), ci(k), ci(d), ci(0), ha.fptr(dq0),
                                              ctypes.c_void_p(0), ctypes.c_void_p(0), ha.stream_ptr()), "nsdp_attn_pre_bwd")
    dq0.sub_(dy)
    ha.check(ha._fn("nsdp_attn_pre_bwd_sub", dt)(ha._p(du, dt), ha.iptr(idx), ci(B), ci(n), ci(N), ci(k), ci(d), ha._p(dy, dt),
                                                  ha.fptr(dq1), ha.stream_ptr()), "nsdp_attn_pre_bwd_sub")
    assert torch.equal(dq0, dq1)
    assert L is not None


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16])
def test_attention_backward_through_inverse_lists_matches_the_atomic_kernels(dt):
    from nsdp_amd import hip_attention as ha
    B, n, N, k, d = 2, 300, 700, 16, 120
    g = torch.Generator().manual_seed(11)
    mk = lambda *s: torch.randn(*s, generator=g).to(dt).to(DEV)
    idx = torch.randint(0, N, (B, n, k), generator=g, dtype=torch.int32).to(DEV)
    base = dict(q=mk(B, n, d), kf=mk(B, N, d), vf=mk(B, N, d), pos=mk(B, n, k, d), res=mk(B, n, d))
    w = mk(B, n, d).float()
    outs = []
    was = ha.INVERSE_LISTS
    for mode in ("1", "0"):
        ha.INVERSE_LISTS = mode
        try:
            t = {kk: v.clone().requires_grad_(True) for kk, v in base.items()}
            u = ha.attn_pre(t["q"], t["kf"], t["pos"], idx, None)
            y = ha.attn_post(u * 0.5, t["vf"], t["pos"], idx, residual=t["res"])
            (y.float() * w).sum().backward()
            outs.append({kk: v.grad.float() for kk, v in t.items()})
        finally:
            ha.INVERSE_LISTS = was
    floor = float(outs[1]["kf"].abs().max())
    for kk in outs[0]:
        scale = max(float(outs[1][kk].abs().max()), floor)
        assert float((outs[0][kk] - outs[1][kk]).abs().max()) <= (2e-2 if dt is torch.bfloat16 else 1e-4) * scale, kk


@pytest.mark.parametrize("B,rows,N,d", [(2, 4096, 100, 200), (3, 1000, 100, 200), (1, 57344, 100, 200), (2, 777, 128, 128),
                                        (2, 2048, 7, 120), (1, 33, 100, 20)])
def test_onehot_scatter_fp32_is_the_exact_sum_in_a_fixed_order(B, rows, N, d):
    """nsdp_scatter_rows_onehot_f32 (scatter as a GEMM, three bf16 planes of the source x the exact one-hot operand):
    against an fp64 index_add -- error at fp32 summation level, nothing like a bf16's -- and bit-identical run to run
    (no atomics: the decoder's anchor-table gradients are reproducible, which the fp32-atomic kernels were not)."""
    from nsdp_amd.hip_attention import onehot_scatter
    g = torch.Generator().manual_seed(rows + N + d)
    src = (torch.randn(B, rows, d, generator=g) * torch.exp(2.0 * torch.randn(B, rows, 1, generator=g))).to(DEV)
    idx = torch.randint(0, N, (B, rows), generator=g).to(DEV).int()
    idx[:, : min(rows, N)] = torch.arange(min(rows, N), device=DEV, dtype=torch.int32)        # every table row is hit
    t1 = onehot_scatter(src, idx, N)
    t2 = onehot_scatter(src, idx, N)
    assert t1.shape == (B, N, d) and torch.equal(t1, t2)
    ref = torch.zeros(B, N, d, dtype=torch.float64, device=DEV)
    ref.scatter_add_(1, idx.long()[:, :, None].expand(-1, -1, d), src.double())
    mag = torch.zeros(B, N, d, dtype=torch.float64, device=DEV)
    mag.scatter_add_(1, idx.long()[:, :, None].expand(-1, -1, d), src.double().abs())
    # fp32 accumulation of up to rows / N x 3 addends per entry: a few ulps of the sum of magnitudes
    err = ((t1.double() - ref).abs() / (mag + 1e-30)).max()
    assert float(err) <= 3e-6, float(err)


@pytest.mark.parametrize("B,n,N,k,d", [(3, 4096, 100, 7, 200), (2, 130, 20, 7, 200), (1, 8192, 100, 7, 200)])
def test_decoder_attention_backward_is_bit_reproducible_and_matches_the_atomic_path(B, n, N, k, d):
    """The decoder form (one query vector per shape, global token): with the one-hot scatters and the partial-sum
    global-token reduction the backward has no atomics -- two runs are bit-equal -- and equals the atomic kernels' result
    up to their summation order."""
    from nsdp_amd import hip_attention as ha
    g = torch.Generator().manual_seed(B * n + d)
    mk = lambda *s: torch.randn(*s, generator=g).to(DEV)
    q0, kf0, vf0, pos0 = mk(B, 1, d), mk(B, N, d), mk(B, N, d), mk(B, n, k, d)
    ag0, vg0 = mk(B, d), mk(B, d)
    w = mk(d, d) * 0.2
    idx = torch.randint(0, N, (B, n, k), generator=g).to(DEV).int()
    go = mk(B, n, d)

    def run():
        from nsdp_amd import hip_linear
        ts = [t.clone().requires_grad_(True) for t in (q0, kf0, vf0, pos0, ag0, vg0)]
        q, kf, vf, pos, a_g, v_g = ts
        link = ha.pos_grad_link()
        link.grad_sum = hip_linear.InputGradSum()
        u = ha.attn_pre(q, kf, pos, idx, link)
        a = hip_linear.linear(u, w, grad_sum=link.grad_sum)
        out = ha.attn_post(a, vf, pos, idx, a_g, v_g, link=link)
        return torch.autograd.grad(out, ts, go)

    was = ha.ONEHOT_SCATTER_F32
    try:
        ha.ONEHOT_SCATTER_F32 = True
        r1, r2 = run(), run()
        ha.ONEHOT_SCATTER_F32 = False
        ra = run()
    finally:
        ha.ONEHOT_SCATTER_F32 = was
    for x, y in zip(r1, r2):
        assert torch.equal(x, y)
    for x, e in zip(r1, ra):
        assert x.shape == e.shape
        assert float((x - e).abs().max()) <= 3e-5 * (float(e.abs().max()) + 1.0)


@pytest.mark.parametrize("B,n,N,k,d,per_shape,has_res,has_g", [
    (2, 300, 300, 16, 200, False, True, False),       # transformer block: per-point queries, residual
    (2, 130, 500, 10, 120, False, False, False),      # set abstraction
    (1, 640, 100, 16, 64, False, True, False),        # n >= 4 N (the plain path's LDS-table kernel; qsub takes the generic one)
    (3, 4096, 100, 7, 200, True, False, True),        # decoder: one query per shape folds into the table, global token
])
def test_attn_post_rebuilds_the_values_from_u(B, n, N, k, d, per_shape, has_res, has_g):
    """attn_post(sub=(k, q)) reads u = q_i - k_j + pos where the plain call reads pos: same output, same gradients for the
    logits, the value table and pos (k and q are constants of that node)."""
    from nsdp_amd.hip_attention import attn_post
    g = torch.Generator().manual_seed(B * 31 + n + d)
    mk = lambda *s: torch.randn(*s, generator=g).to(DEV)
    a0, vf0, pos0, kf, q = mk(B, n, k, d), mk(B, N, d), mk(B, n, k, d), mk(B, N, d), mk(B, 1 if per_shape else n, d)
    res = mk(B, n, d) if has_res else None
    a_g, v_g = (mk(B, d), mk(B, d)) if has_g else (None, None)
    idx = torch.randint(0, N, (B, n, k), generator=g).to(DEV).int()
    go = mk(B, n, d)
    u0 = _ref_pre(q.expand(B, n, d), kf, pos0, idx)

    def run(p0, sub):
        a, vf, p = (t.clone().requires_grad_(True) for t in (a0, vf0, p0))
        out = attn_post(a, vf, p, idx, a_g=a_g, v_g=v_g, residual=res, sub=sub)
        return (out,) + torch.autograd.grad(out, [a, vf, p], go)

    plain, fused = run(pos0, None), run(u0, (kf, q))
    for name, a_, e_ in zip(("out", "da", "dvf", "dpos"), fused, plain):
        assert a_.shape == e_.shape
        # u - q + (v + k) against v + pos: two more fp32 roundings on values of a few units
        assert float((a_ - e_).abs().max()) <= 1e-5 * (float(e_.abs().max()) + 1.0), name


@pytest.mark.parametrize("B,n,N,k,d,second,combined", [(4, 1024, 1024, 16, 200, False, False), (8, 512, 2048, 16, 200, True, False),
                                                        (8, 512, 2048, 16, 200, True, True)])
def test_vector_attention_without_the_attn_pre_pass(B, n, N, k, d, second, combined, monkeypatch):
    """ops.vector_attention with u coming straight out of the position-encoding GEMM (FUSE_PRE) against the layered
    attn_pre pass: outputs and every gradient (inputs and the two MLPs' weights); `second`: a second attention reusing the
    first one's position encoding through PosAsU (the set-abstraction pair)."""
    from torch import nn
    from nsdp_amd.model import ops
    from nsdp_amd import hip_linear
    if (ops.PAIR_MASK or not ops.FUSE_PRE or (combined and not ops.COMBINE_TABLES)
            or not hip_linear.gather_init_ok(B * n * k, d, d)):      # (NSDP_BF16X3=0: no kernel to take the gathered addend)
        pytest.skip("knob run: the fused path is off")
    g = torch.Generator().manual_seed(n + N)
    mk = lambda *s: torch.randn(*s, generator=g).to(DEV)
    torch.manual_seed(3)
    fc_delta = nn.Sequential(nn.Linear(3, d), nn.ReLU(), nn.Linear(d, d)).to(DEV)
    fc_gamma = nn.Sequential(nn.Linear(d, d), nn.ReLU(), nn.Linear(d, d)).to(DEV)
    fc_gamma2 = nn.Sequential(nn.Linear(d, d), nn.ReLU(), nn.Linear(d, d)).to(DEV)
    rel0, q0, kf0, vf0 = mk(B, n, k, 3) * 0.1, mk(B, n, d), mk(B, N, d), mk(B, N, d)
    q20, kf20, vf20 = mk(B, n, d), mk(B, N, d), mk(B, N, d)
    idx = torch.randint(0, N, (B, n, k), generator=g).to(DEV).int()
    go = mk(B, n, d)
    params = [p for m in (fc_delta, fc_gamma, fc_gamma2) for p in m.parameters()]

    def run(fuse):
        monkeypatch.setattr(ops, "FUSE_PRE", fuse)
        for p in params:
            p.grad = None
        ins = [t.clone().requires_grad_(True) for t in (rel0, q0, kf0, vf0, q20, kf20, vf20)]
        rel, q, kf, vf, q2, kf2, vf2 = ins
        comb = combined and fuse      # the encoder blocks' form: the projections deliver v + k, q2 - q1, k2 - k1, v2 + k1 themselves
        assert ops.fused_pre_applies(idx, d) == (fuse and ops.COMBINE_TABLES)
        out, pos = ops.vector_attention(rel, q, kf, vf + kf.detach() if comb else vf, idx, fc_delta, fc_gamma, combined=comb)
        assert isinstance(pos, ops.PosAsU) == fuse
        if second:
            if comb:
                out2, _ = ops.vector_attention(None, q2 - pos.q, kf2 - pos.kf, vf2 + pos.kf, idx, None, fc_gamma2, residual=out,
                                               pos=pos, combined=True)
            else:
                out2, _ = ops.vector_attention(rel, q2, kf2, vf2, idx, fc_delta, fc_gamma2, residual=out, pos=pos)
            out = out2
        else:
            ins = ins[:4]
        (out * go).sum().backward()
        torch.cuda.synchronize()
        return [out.detach()] + [t.grad for t in ins] + [p.grad.clone() for p in params if p.grad is not None]

    layered, fused = run(False), run(True)
    assert len(layered) == len(fused)
    for i, (a_, e_) in enumerate(zip(fused, layered)):
        assert a_.shape == e_.shape
        # u may differ in its last bit between the two paths (one more rounding of q - k + pos in the layered one), so among
        # the 10^7 hidden activations of fc_gamma a ReLU can sit on the other side of zero (measured: none, 2.4e-6 norm-wise):
        # a norm-wise bound, and a loose element-wise one a wrong term would still break
        # (absolute floors: the last bias of fc_gamma has NO gradient in exact arithmetic -- softmax is shift invariant -- and
        # both paths deliver 4e-5 of rounding noise there)
        assert float((a_ - e_).norm()) <= 1e-4 * float(e_.norm()) + 2e-4, i
        assert float((a_ - e_).abs().max()) <= 1e-2 * float(e_.abs().max()) + 1e-4, i
