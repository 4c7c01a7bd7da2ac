"""Every form of the vector-attention kernels (csrc/attention.hip) against the fp64 reference of tests/attention_ref.py.

The bound is per element: E = max |got - ref64| / env <= 4 max(1, E_EMUL), env the first-order rounding envelope of the
formulas the kernel header states and E_EMUL what a plain fp32 implementation of them reaches (attention_ref.py).  Every case
asserts the kernel that ran through the variant trace; forms are selected by the module attributes of hip_attention, so the
file does not depend on the knob matrix."""
import contextlib
import ctypes
import itertools

import pytest
import torch

import attention_ref as ar

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
F32, BF = torch.float32, torch.bfloat16
BOUND = ar.gpu_bound()
_ci = ctypes.c_int

POST_NAMES = {"attn_post_bwd_lds", "attn_post_bwd_stream", "attn_post_bwd_atomic", "attn_post_bwd_det"}
PRE_NAMES = {"attn_pre_bwd_lds", "attn_pre_bwd_stream", "attn_pre_bwd_atomic", "scatter_rows_regtab<8>"}


class _Trace:
    """Context manager around nsdp_trace_*: ``names`` = the kernel variants launched inside."""

    def __enter__(self):
        from nsdp_amd import _lib
        self.L = _lib.lib()
        self.names = set()
        self.L.nsdp_trace_enable(1)
        return self

    def __exit__(self, *exc):
        self.L.nsdp_trace_enable(0)
        n = self.L.nsdp_trace_read(None, 0)
        buf = ctypes.create_string_buffer(n)
        self.L.nsdp_trace_read(buf, n)
        self.names = set(x for x in buf.value.decode().split("\n") if x)
        return False


DEFAULT_KNOBS = {"INVERSE_LISTS": "1", "ONEHOT_SCATTER": True, "ONEHOT_SCATTER_F32": True, "NATIVE_BF16": True}


@contextlib.contextmanager
def _knobs(**kw):
    """The default dispatch of hip_attention (whatever the environment of this run set), with ``kw`` on top."""
    from nsdp_amd import hip_attention as ha
    kw = dict(DEFAULT_KNOBS, **kw)
    was = {kk: getattr(ha, kk) for kk in kw}
    try:
        for kk, v in kw.items():
            setattr(ha, kk, v)
        yield
    finally:
        for kk, v in was.items():
            setattr(ha, kk, v)


def _report(what, E):
    print(f"\nE[{what}] " + " ".join(f"{kk}={v:.3f}" for kk, v in sorted(E.items())))


def _ran(names, family, want):
    """Of the kernels of one family (post / pre backward) exactly ``want`` ran (None: none of them)."""
    got = names & family
    assert got == (set() if want is None else {want}), (want, sorted(names))


# ----------------------------------------------------------------------------------------------------------------------
# running the kernels
# ----------------------------------------------------------------------------------------------------------------------
def run_post(c, sub=None):
    """attn_post forward + backward on the case ``c`` (attention_ref.make_post_case) -> ({name: tensor}, traced names)."""
    from nsdp_amd import hip_attention as ha
    keys = [kk for kk in ("a", "vf", "pos", "a_g", "v_g", "residual") if c.get(kk) is not None]
    t = {kk: c[kk].detach().clone().requires_grad_(True) for kk in keys}
    with _Trace() as tr:
        y = ha.attn_post(t["a"], t.get("vf"), t["pos"], c["idx"], t.get("a_g"), t.get("v_g"), t.get("residual"), sub=sub)
        grads = torch.autograd.grad(y, [t[kk] for kk in keys], c["dy"])
        torch.cuda.synchronize()
    got = {"y": y.detach()}
    got.update({{"a": "da", "vf": "dvf", "pos": "dpos", "a_g": "da_g", "v_g": "dv_g", "residual": "dres"}[kk]: g
                for kk, g in zip(keys, grads)})
    if "dres" in got:
        assert torch.equal(got.pop("dres"), c["dy"])          # the residual's gradient is dy itself
    for kk, g in got.items():
        assert g.dtype is c["a"].dtype, kk
    return got, tr.names


def check_post(c, want, what, sub=None, twice=False):
    got, names = run_post(c, sub)
    _ran(names, POST_NAMES, want)
    ref, env = ar.post_reference(**c, sub=sub)
    _report(what, ar.measure(got, ref, env))
    E = ar.assert_within(got, ref, env, BOUND, what)
    if twice:          # a form documented as atomic-free: bit-equal run to run
        again, _ = run_post(c, sub)
        for kk in got:
            assert torch.equal(got[kk], again[kk]), (what, kk)
    return E


def run_pre(q, kf, pos, idx, du, acc=None, fused=None):
    """attn_pre forward + backward -> ({u, dq, dkf, dpos}, traced names).  ``acc``: d(pos) parked by attn_post (the kernel adds
    du into it); ``fused`` = (dvf, dy): the hand-over in which du is the total d(pos) and the value path's share is undone."""
    from nsdp_amd import hip_attention as ha
    t = [x.detach().clone().requires_grad_(True) for x in (q, kf, pos)]
    link = ha.pos_grad_link() if (acc is not None or fused is not None) else None
    with _Trace() as tr:
        u = ha.attn_pre(t[0], t[1], t[2], idx, link)
        if acc is not None:
            link.dpos = acc.clone()
        if fused is not None:
            link.fused, link.dvf, link.dy = True, fused[0].clone(), fused[1]
        dq, dkf, dpos = torch.autograd.grad(u, t, du)
        torch.cuda.synchronize()
    return {"u": u.detach(), "dq": dq, "dkf": dkf, "dpos": dpos}, tr.names


def check_pre(q, kf, pos, idx, du, want, what, acc=None, twice=False):
    got, names = run_pre(q, kf, pos, idx, du, acc)
    _ran(names, PRE_NAMES, want)
    ref, env = ar.pre_reference(q, kf, pos, idx, du, acc)
    if acc is None:
        assert torch.equal(got.pop("dpos"), du)          # handed through
    _report(what, ar.measure(got, ref, env))
    ar.assert_within(got, ref, env, BOUND, what)
    if twice:
        again, _ = run_pre(q, kf, pos, idx, du, acc)
        for kk in got:
            assert torch.equal(got[kk], again[kk]), (what, kk)


def make_pre_case(shape, seed, dtype=F32, qb=False, integer=False, hot=False, same=False):
    B, n, N, k, d = shape
    g = torch.Generator().manual_seed(seed)
    mk = lambda *s: torch.randn(*s, generator=g).to(dtype).to(DEV)
    q, kf, pos = mk(B, 1 if qb else n, d), mk(B, N, d), mk(B, n, k, d)
    du = torch.randint(-8, 9, (B, n, k, d), generator=g).to(dtype).to(DEV) if integer else mk(B, n, k, d)
    idx = torch.randint(0, N, (B, n, k), generator=g, dtype=torch.int32).to(DEV)
    if hot:
        idx[:, :, 0] = min(5, N - 1)
    if same:
        idx[:] = N - 1
    return q, kf, pos, idx, du


# ----------------------------------------------------------------------------------------------------------------------
# 3a. every form against fp64
# ----------------------------------------------------------------------------------------------------------------------
POST_FORMS = [
    # id, (B, n, N, k, d), token, residual scale, has_v, knobs, traced form, atomic-free
    ("lds-110KiB-n=4N", (2, 440, 110, 5, 256), None, 1.0, True, {}, "attn_post_bwd_lds", False),
    ("lds-token-d8", (3, 20, 5, 3, 8), "rand", 1.0, True, {}, "attn_post_bwd_lds", False),
    ("stream-past-lds", (2, 444, 111, 5, 256), None, 1.0, True, {}, "attn_post_bwd_stream", True),
    ("stream-n=4N-1", (2, 439, 110, 5, 256), None, 0.0, True, {}, "attn_post_bwd_stream", True),
    ("stream", (2, 37, 50, 10, 120), None, 1.0, True, {}, "attn_post_bwd_stream", True),
    ("atomic-knob", (2, 37, 50, 10, 120), None, 1.0, True, {"INVERSE_LISTS": "0"}, "attn_post_bwd_atomic", False),
    ("atomic-token-d8", (3, 19, 5, 3, 8), "rand", 1.0, True, {}, "attn_post_bwd_atomic", False),
    ("atomic-pos-only", (2, 33, 40, 10, 120), None, 0.0, False, {}, "attn_post_bwd_atomic", False),
    ("det-token", (3, 130, 20, 7, 200), "rand", 0.0, True, {}, "attn_post_bwd_det", True),
    ("det-token-res", (3, 130, 20, 7, 200), "rand", 1.0, True, {}, "attn_post_bwd_det", True),
    ("det-n1", (2, 1, 128, 3, 20), "rand", 1.0, True, {}, "attn_post_bwd_det", True),
    ("det-d208", (2, 33, 100, 5, 208), "rand", 0.0, True, {}, "attn_post_bwd_det", True),
    ("det-d208-res", (2, 33, 100, 5, 208), "rand", 1.0, True, {}, "attn_post_bwd_det", True),
]


def _bf16_has(case):
    """bf16 reaches the det form through its scatter-as-GEMM, which needs an even N and d % 8 == 0."""
    B, n, N, k, d = case[1]
    return case[6] != "attn_post_bwd_det" or (N % 2 == 0 and d % 8 == 0)


POST_FORM_RUNS = [(c, F32) for c in POST_FORMS] + [(c, BF) for c in POST_FORMS if _bf16_has(c)]


@pytest.mark.parametrize("case,dtype", POST_FORM_RUNS, ids=[f"{c[0]}-{'bf16' if dt is BF else 'fp32'}" for c, dt in POST_FORM_RUNS])
def test_post_form_against_fp64(case, dtype):
    name, shape, token, rscale, has_v, knobs, want, det = case
    from nsdp_amd import _lib
    if dtype is BF and want == "attn_post_bwd_det" and not hasattr(_lib.lib(), "nsdp_scatter_rows_onehot_bf16"):
        pytest.skip("this build lacks nsdp_scatter_rows_onehot_bf16")
    c = ar.make_post_case(shape, 31 + len(name), dtype, DEV, rscale=rscale, token=token, has_v=has_v, hot=True)
    with _knobs(**knobs):
        check_post(c, want, f"{name}/{dtype}", twice=det)


def _det_direct(c):
    """nsdp_attn_post_fwd + nsdp_attn_post_bwd_det through the C ABI (shapes the autograd wrapper routes elsewhere)."""
    from nsdp_amd._lib import check, fptr, iptr, lib, stream_ptr
    B, n, k, d = c["a"].shape
    N = c["vf"].shape[1]
    L = lib()
    y = torch.empty(B, n, d, device=DEV)
    lse = torch.empty(B, n, d, device=DEV)
    r = c["residual"]
    rp = ctypes.c_void_p(0) if r is None else fptr(r)
    check(L.nsdp_attn_post_fwd(fptr(c["a"]), fptr(c["vf"]), fptr(c["pos"]), iptr(c["idx"]), fptr(c["a_g"]), fptr(c["v_g"]), rp,
                               _ci(B), _ci(n), _ci(N), _ci(k), _ci(d), fptr(y), fptr(lse), stream_ptr()), "nsdp_attn_post_fwd")
    L.nsdp_attn_post_bwd_det_workspace_bytes.restype = ctypes.c_size_t
    nbytes = int(L.nsdp_attn_post_bwd_det_workspace_bytes(_ci(B), _ci(n), _ci(k), _ci(d)))
    ws = torch.empty(max(nbytes // 4, 1), device=DEV)
    da, dpos = torch.empty_like(c["a"]), torch.empty_like(c["a"])
    da_g, dv_g = torch.empty(B, d, device=DEV), torch.empty(B, d, device=DEV)
    with _Trace() as tr:
        check(L.nsdp_attn_post_bwd_det(fptr(c["dy"]), fptr(c["a"]), fptr(c["vf"]), fptr(c["pos"]), iptr(c["idx"]), fptr(c["a_g"]),
                                       fptr(c["v_g"]), fptr(y), rp, fptr(lse), _ci(B), _ci(n), _ci(N), _ci(k), _ci(d), fptr(da),
                                       fptr(dpos), fptr(da_g), fptr(dv_g), fptr(ws), ctypes.c_size_t(nbytes), stream_ptr()),
              "nsdp_attn_post_bwd_det")
        torch.cuda.synchronize()
    return {"y": y, "da": da, "dpos": dpos, "da_g": da_g, "dv_g": dv_g}, tr.names, nbytes


def test_post_det_with_grown_iters_against_fp64():
    """B n above iters_for(k) 4096 per_iter centres: shape_plan lengthens the workgroups' walks (the production decoder's
    regime, B = 32, n = 8192, d = 200) -- here at d = 4, k = 1: 256 centres per workgroup iteration, 8 -> 9 iterations."""
    shape = B, n, N, k, d = (2, 4300000, 4, 1, 4)
    assert B * n > 8 * 4096 * 256
    c = ar.make_post_case(shape, 5, F32, DEV, rscale=1.0, token="rand")
    got, names, nbytes = _det_direct(c)
    _ran(names, POST_NAMES, "attn_post_bwd_det")
    iters = -(-B * n // (4096 * 256))
    assert iters == 9 and nbytes == B * (-(-n // (iters * 256))) * 2 * d * 4          # the grown plan, not 8 iterations
    ref, env = ar.post_reference(**c, want_dvf=False)          # (the scatter is another entry's; the forms above cover it)
    _report("det-grown-iters", ar.measure(got, ref, env))
    ar.assert_within(got, ref, env, BOUND, "det-grown-iters")
    # 4.3 M addends per token sum make its envelope (L u sum |addend|) a quarter of the sum: a lost workgroup partial would
    # pass.  With dy zero but at a few centres -- the ends of a shape, both sides of the first workgroup boundary (9 x 256),
    # the middle -- the sums have eight addends each and the partials of the other 1860 workgroups must be exact zeros.
    dy = torch.zeros_like(c["dy"])
    for i in (0, 1, iters * 256 - 1, iters * 256, n // 2, n - 2, n - 1):
        dy[:, i] = c["dy"][:, i]
    c["dy"] = dy
    got, _, _ = _det_direct(c)
    ref, env = ar.post_reference(**c, want_dvf=False)
    _report("det-grown-iters-sparse", ar.measure(got, ref, env))
    ar.assert_within(got, ref, env, BOUND, "det-grown-iters-sparse")
    del got, ref, env, c
    torch.cuda.empty_cache()


@pytest.mark.parametrize("shape,per_shape,token,want", [
    ((2, 64, 64, 16, 200), False, None, "attn_post_bwd_stream"),      # per-point queries: nsdp_attn_post_fwd_q / _bwd_q
    ((3, 130, 20, 7, 200), True, "rand", "attn_post_bwd_det"),         # one query per shape, folded into the table
], ids=["per-point", "per-shape-folded"])
def test_post_sub_form_against_fp64(shape, per_shape, token, want):
    """attn_post(sub=(kf, q)): `pos` holds u = q_i - k_j + pos and the values are rebuilt as u + (v + k)[idx] - q_i."""
    from nsdp_amd import hip_attention as ha
    B, n, N, k, d = shape
    c = ar.make_post_case(shape, 17, F32, DEV, rscale=1.0, token=token)
    g = torch.Generator().manual_seed(3)
    q, kf = torch.randn(B, 1 if per_shape else n, d, generator=g).to(DEV), torch.randn(B, N, d, generator=g).to(DEV)
    with torch.no_grad():
        c["pos"] = ha.attn_pre(q, kf, c["pos"], c["idx"])
    with _knobs():
        check_post(c, want, f"sub-{'per-shape' if per_shape else 'per-point'}", sub=(kf, q), twice=True)


PRE_FORMS = [
    # id, (B, n, N, k, d), per-shape query, knobs, traced form, accumulator also, atomic-free
    ("regtab-n4096", (2, 4096, 3, 1, 4), True, {}, "scatter_rows_regtab<8>", True, False),
    ("regtab-d256", (2, 586, 128, 7, 256), True, {}, "scatter_rows_regtab<8>", True, False),
    ("lds-under-regtab", (2, 4095, 3, 1, 4), True, {}, "attn_pre_bwd_lds", True, False),
    ("lds-per-shape-q", (3, 300, 20, 7, 200), True, {}, "attn_pre_bwd_lds", True, False),
    ("lds-per-point-q", (2, 640, 100, 16, 64), False, {}, "attn_pre_bwd_lds", True, False),
    ("stream", (2, 37, 50, 10, 120), False, {}, "attn_pre_bwd_stream", False, True),
    ("atomic-knob", (2, 37, 50, 10, 120), False, {"INVERSE_LISTS": "0"}, "attn_pre_bwd_atomic", True, False),
    ("atomic-per-shape-q", (3, 19, 5, 3, 8), True, {}, "attn_pre_bwd_atomic", True, False),
]


@pytest.mark.parametrize("dtype", [F32, BF], ids=["fp32", "bf16"])
@pytest.mark.parametrize("case", PRE_FORMS, ids=[c[0] for c in PRE_FORMS])
def test_pre_form_against_fp64(case, dtype):
    name, shape, qb, knobs, want, with_acc, det = case
    q, kf, pos, idx, du = make_pre_case(shape, 7 + len(name), dtype, qb, hot=True)
    with _knobs(**knobs):
        check_pre(q, kf, pos, idx, du, want, f"pre-{name}/{dtype}", twice=det)
        if with_acc:          # the d(pos) accumulator of pos_grad_link: the kernel adds du into the tensor attn_post parked
            acc = torch.randn(du.shape, generator=torch.Generator().manual_seed(1)).to(dtype).to(DEV)
            check_pre(q, kf, pos, idx, du, want, f"pre-{name}+acc/{dtype}", acc=acc)


@pytest.mark.parametrize("dtype", [F32, BF], ids=["fp32", "bf16"])
def test_pre_stream_form_with_the_accumulator(dtype):
    """nsdp_attn_pre_bwd with dkf = NULL (the caller scatters through the inverse lists) and a d(pos) accumulator."""
    from nsdp_amd import hip_attention as ha
    shape = B, n, N, k, d = (2, 37, 50, 10, 120)
    q, kf, pos, idx, du = make_pre_case(shape, 9, dtype)
    acc = torch.randn(du.shape, generator=torch.Generator().manual_seed(2)).to(dtype).to(DEV)
    got_acc = acc.clone()
    dq = torch.empty(B, n, d, device=DEV)
    with _Trace() as tr:
        ha.check(ha._fn("nsdp_attn_pre_bwd", dtype)(ha._p(du, dtype), ha.iptr(idx), _ci(B), _ci(n), _ci(N), _ci(k), _ci(d), _ci(0),
                                                     ha.fptr(dq), ctypes.c_void_p(0), ha._p(got_acc, dtype), ha.stream_ptr()),
                 "nsdp_attn_pre_bwd")
        dkf = ha.segment_sum(du, idx, N, -1.0)
        torch.cuda.synchronize()
    _ran(tr.names, PRE_NAMES, "attn_pre_bwd_stream")
    ref, env = ar.pre_reference(q, kf, pos, idx, du, acc)
    ref.pop("u"), env.pop("u")
    if dtype is BF:          # (dq / dkf leave these two entries in fp32: no storage rounding of the sums)
        for kk in ("dq", "dkf"):
            env[kk] = env[kk] - ar.U_BF16 * ref[kk].abs()
    got = {"dq": dq, "dkf": dkf, "dpos": got_acc}
    _report(f"pre-stream+acc/{dtype}", ar.measure(got, ref, env))
    ar.assert_within(got, ref, env, BOUND, "pre-stream+acc")


@pytest.mark.parametrize("dtype", [BF, F32], ids=["bf16", "fp32"])
def test_pre_fused_decoder_form_through_the_one_hot_scatter(dtype):
    """The decoder's fused hand-over (one query per shape, du = the total d(pos)): dkf = -scatter(du) + dvf and
    dq = sum du - sum_a dvf[a] out of one scatter-as-GEMM pass, no attention kernel and no atomics."""
    from nsdp_amd import _lib
    sym = "nsdp_scatter_rows_onehot_bf16" if dtype is BF else "nsdp_scatter_rows_onehot_f32"
    if not hasattr(_lib.lib(), sym):
        pytest.skip(f"this build lacks {sym}")
    shape = B, n, N, k, d = (3, 130, 20, 7, 200)
    q, kf, pos, idx, du = make_pre_case(shape, 13, dtype, qb=True, hot=True)
    g = torch.Generator().manual_seed(4)
    dvf_in, dy_in = torch.randn(B, N, d, generator=g).to(DEV), torch.randn(B, n, d, generator=g).to(dtype).to(DEV)
    with _knobs(ONEHOT_SCATTER=True, ONEHOT_SCATTER_F32=True):
        got, names = run_pre(q, kf, pos, idx, du, fused=(dvf_in, dy_in))
        again, _ = run_pre(q, kf, pos, idx, du, fused=(dvf_in, dy_in))
    _ran(names, PRE_NAMES, None)
    assert torch.equal(got.pop("dpos"), du)
    ref, env = ar.pre_reference(q, kf, pos, idx, du)
    uo = ar.U_BF16 if dtype is BF else 0.0
    u = ar.U32
    # the table and its column sum in fp32, then the two corrections: one rounding each, and the N-term sums of torch
    e_tab = env["dkf"] - uo * ref["dkf"].abs()
    dkf = ref["dkf"] + dvf_in.double()
    dq = ref["dq"] - dvf_in.double().sum(1, keepdim=True)
    env["dkf"] = e_tab + (u + uo) * dkf.abs()
    env["dq"] = (e_tab.sum(1, keepdim=True) + N * u * (ref["dkf"].abs() + dvf_in.double().abs()).sum(1, keepdim=True)
                 + (u + uo) * dq.abs() + ar.FLOOR)
    ref["dkf"], ref["dq"] = dkf, dq
    _report(f"pre-fused-onehot/{dtype}", ar.measure(got, ref, env))
    ar.assert_within(got, ref, env, BOUND, "pre-fused-onehot")
    for kk in got:
        assert torch.equal(got[kk], again[kk]), kk


# ----------------------------------------------------------------------------------------------------------------------
# 3b. lane and tail grid (default dispatch, forward and backward)
# ----------------------------------------------------------------------------------------------------------------------
GRID_D = (4, 8, 12, 120, 132, 200, 252, 256)
GRID_K = (1, 2, 3, 5, 15, 16, 17, 31, 32, 33, 63, 64, 65)
GRID_BN = ((1, 1), (7, 3), (70, 3), (2, 129), (5, 257))


def _pairwise_grid():
    """A deterministic greedy cover: every pair of levels of (d, k, (B, n)) that some admissible case holds appears in a case.
    Admissible: under 1 M elements, and (70, 3) only with d = 4."""
    ok = [(d, k, bn) for d, k, bn in itertools.product(GRID_D, GRID_K, GRID_BN)
          if bn[0] * bn[1] * k * d < (1 << 20) and (bn != (70, 3) or d == 4)]
    pairs = lambda t: {("dk", t[0], t[1]), ("db", t[0], t[2]), ("kb", t[1], t[2])}
    todo = set().union(*(pairs(t) for t in ok))
    chosen = []
    while todo:
        best = max(ok, key=lambda t: (len(pairs(t) & todo), -ok.index(t)))
        chosen.append(best)
        todo -= pairs(best)
    return chosen


GRID = _pairwise_grid()


def _expect_post(dtype, token, has_v, B, n, N, k, d):
    """The documented dispatch of hip_attention._AttnPost.backward / attn_post_bwd_t, restated."""
    fits = N * d * 4 <= 110 * 1024 and n >= 4 * N
    if dtype is F32:
        onehot = has_v and token and N <= 128 and 16 < d <= 208
    else:
        onehot = has_v and token and N <= 128 and N % 2 == 0 and d % 8 == 0
    if onehot:
        return "attn_post_bwd_det"
    if has_v and not token and not fits:
        return "attn_post_bwd_stream"
    return "attn_post_bwd_lds" if (has_v and fits) else "attn_post_bwd_atomic"


def _expect_pre(qb, B, n, N, k, d):
    if qb and N <= 128 and n * k >= 4096:
        return "scatter_rows_regtab<8>"
    fits = N * d * 4 <= 110 * 1024 and n >= 4 * N
    if not qb and not fits:
        return "attn_pre_bwd_stream"
    return "attn_pre_bwd_lds" if fits else "attn_pre_bwd_atomic"


def _grid_case(i, d, k, bn, token, qb, dtype=F32):
    B, n = bn
    N = (3, 1, 40)[i % 3] if n > 1 else 3          # a table in LDS (n >= 4 N), a single source row, more sources than centres
    shape = (B, n, N, k, d)
    qb = qb and n != 1          # (a single centre: (B, 1, d) is the per-point form)
    c = ar.make_post_case(shape, 1000 + i, dtype, DEV, rscale=float(i % 2), token="rand" if token else None)
    with _knobs():
        check_post(c, _expect_post(dtype, token, True, *shape), f"grid-post {shape} token={token}")
        q, kf, pos, idx, du = make_pre_case(shape, 2000 + i, dtype, qb)
        check_pre(q, kf, pos, idx, du, _expect_pre(qb, *shape), f"grid-pre {shape} qb={qb}")


@pytest.mark.parametrize("i", range(len(GRID)), ids=[f"d{d}-k{k}-B{bn[0]}n{bn[1]}" for d, k, bn in GRID])
def test_lane_and_tail_grid(i):
    d, k, bn = GRID[i]
    _grid_case(i, d, k, bn, token=i % 2 == 1, qb=i % 4 >= 2)


@pytest.mark.parametrize("token,qb", [(True, True), (True, False), (False, True)], ids=["token+shape-q", "token", "shape-q"])
def test_one_lane_crosses_dozens_of_shape_boundaries(token, qb):
    """(B, n) = (70, 3), d = 4, k = 1: 64 points per wave and 8 groups per wave, so one lane walks centres of up to 8 shapes
    and a wave holds 22: every flush of the per-shape partials (token sums, per-shape dq) is used."""
    for i in range(3):          # N = 3, 1, 40
        _grid_case(i, 4, 1, (70, 3), token, qb)


def test_grid_covers_every_level_pair():
    seen_iters = {(1 if k >= 64 else 2 if k >= 32 else 4 if k >= 16 else 8) for _, k, _ in GRID}
    assert seen_iters == {1, 2, 4, 8}
    assert {d for d, _, _ in GRID} == set(GRID_D) and {k for _, k, _ in GRID} == set(GRID_K)
    assert {bn for _, _, bn in GRID} == set(GRID_BN)
    assert all(bn[0] * bn[1] * k * d < (1 << 20) for d, k, bn in GRID)


# ----------------------------------------------------------------------------------------------------------------------
# 3c. conditioning sweep, one shape per `post` backward form
# ----------------------------------------------------------------------------------------------------------------------
SWEEP_FORM = {"lds": ("attn_post_bwd_lds", {}), "stream": ("attn_post_bwd_stream", {}),
              "atomic": ("attn_post_bwd_atomic", {"INVERSE_LISTS": "0"}), "det": ("attn_post_bwd_det", {})}


@pytest.mark.parametrize("form", list(ar.SWEEP_SHAPES))
def test_conditioning_sweep(form):
    """Logit spread {0, 1, 30} x common offset {0, +-1000} x residual scale {0, 1, 2^6, 2^12}, and a token logit 40 above /
    below every neighbour's.  The envelope holds the |lse| and |y| + |r| terms: passing means the kernels lose what the
    formulation costs (fp32 lse, yb = y - residual) and nothing more."""
    shape, token = ar.SWEEP_SHAPES[form]
    want, knobs = SWEEP_FORM[form]
    worst, fails = {}, []
    with _knobs(**knobs):
        for i, (sp, off, rs, tok) in enumerate(ar.conditioning_cases(token)):
            c = ar.make_post_case(shape, 100 + i, F32, DEV, sp, off, rs, tok)
            got, names = run_post(c)
            _ran(names, POST_NAMES, want)
            ref, env = ar.post_reference(**c)
            E = ar.measure(got, ref, env)
            for kk, v in E.items():
                if v >= worst.get(kk, (0.0,))[0]:
                    worst[kk] = (v, sp, off, rs, tok)
                if not v <= BOUND:
                    fails.append((kk, v, sp, off, rs, tok))
    for kk, v in sorted(worst.items()):
        print(f"\nE[sweep-{form}] {kk}={v[0]:.3f} at spread {v[1]}, offset {v[2]}, residual {v[3]}, token {v[4]}")
    assert not fails, fails


# ----------------------------------------------------------------------------------------------------------------------
# 3d. exact probes, no tolerance
# ----------------------------------------------------------------------------------------------------------------------
def _int_sum(src, idx, N):
    """int64 index_add of the rows of an integer-valued src [B,n,k,d] by idx."""
    return ar.scatter(src.double().round().long(), idx, N)


EXACT_POST = [(name, shape[:3] + (1,) + shape[4:], token, knobs, want) for name, shape, token, _, has_v, knobs, want, _ in POST_FORMS
              if has_v and not name.endswith("-res")] + [("sub-per-point", (2, 64, 64, 1, 200), None, {}, "attn_post_bwd_stream")]


@pytest.mark.parametrize("index", ["hot", "same"])
@pytest.mark.parametrize("case", EXACT_POST, ids=[c[0] for c in EXACT_POST])
def test_post_exact_probe(case, index):
    """k = 1 and finite logits: w = 1 exactly (a global token 200 below the logit has weight exp(-200) = 0 in fp32), so
    dpos == dy bit for bit and, with integer dy, dvf is an exact integer sum in any order: a lost, doubled or misrouted update
    cannot hide behind a bound.  Index sets: one hot row (idx[..., 0] = 5) and all entries equal."""
    from nsdp_amd import hip_attention as ha
    name, shape, token, knobs, want = case
    B, n, N, k, d = shape
    c = ar.make_post_case(shape, 3 + len(name), F32, DEV, rscale=0.0, token=token, hot=True)
    if index == "same":
        c["idx"][:] = N - 1
    g = torch.Generator().manual_seed(8)
    c["dy"] = torch.randint(-8, 9, (B, n, d), generator=g).float().to(DEV)
    if token:
        c["a_g"] = c["a"].amin(dim=(1, 2)) - 200.0
    sub = None
    if name == "sub-per-point":
        q, kf = torch.randn(B, n, d, generator=g).to(DEV), torch.randn(B, N, d, generator=g).to(DEV)
        with torch.no_grad():
            c["pos"] = ha.attn_pre(q, kf, c["pos"], c["idx"])
        sub = (kf, q)
    with _knobs(**knobs):
        got, names = run_post(c, sub)
    _ran(names, POST_NAMES, want)
    assert torch.equal(got["dpos"], c["dy"].unsqueeze(2))
    assert torch.equal(got["dvf"].long(), _int_sum(c["dy"].unsqueeze(2), c["idx"], N)) and torch.equal(got["dvf"], got["dvf"].round())
    if token:
        assert not bool(got["da_g"].any()) and not bool(got["dv_g"].any())


@pytest.mark.parametrize("index", ["hot", "same"])
@pytest.mark.parametrize("dtype", [F32, BF], ids=["fp32", "bf16"])
@pytest.mark.parametrize("case", PRE_FORMS, ids=[c[0] for c in PRE_FORMS])
def test_pre_exact_probe(case, dtype, index):
    """Integer du (|value| <= 8, sums under 2^24): dkf, dq per point and dq per shape are exact integer sums in any order."""
    name, shape, qb, knobs, want, _, _ = case
    B, n, N, k, d = shape
    q, kf, pos, idx, du = make_pre_case(shape, 5 + len(name), dtype, qb, integer=True, hot=index == "hot", same=index == "same")
    with _knobs(**knobs):
        got, names = run_pre(q, kf, pos, idx, du)
    _ran(names, PRE_NAMES, want)
    dul = du.double().round().long()
    dq = dul.sum(dim=(1, 2)).unsqueeze(1) if qb else dul.sum(dim=2)
    # (bf16: the exact fp32 sum, rounded once to the storage type)
    assert torch.equal(got["dkf"], (-_int_sum(du, idx, N)).float().to(dtype))
    assert torch.equal(got["dq"], dq.float().to(dtype))
    assert torch.equal(got["dpos"], du)


@pytest.mark.parametrize("dtype", [F32, BF], ids=["fp32", "bf16"])
def test_one_hot_scatter_exact_probe(dtype):
    """The scatter-as-GEMM on integer rows: exact (its bf16 planes hold small integers exactly), hot row and all-equal set."""
    from nsdp_amd import _lib
    from nsdp_amd.hip_attention import onehot_scatter
    sym = "nsdp_scatter_rows_onehot_bf16" if dtype is BF else "nsdp_scatter_rows_onehot_f32"
    if not hasattr(_lib.lib(), sym):
        pytest.skip(f"this build lacks {sym}")
    B, rows, N, d = 3, 910, 20, 200
    g = torch.Generator().manual_seed(6)
    src = torch.randint(-8, 9, (B, rows, 1, d), generator=g).to(dtype).to(DEV)
    for same in (False, True):
        idx = torch.randint(0, N, (B, rows, 1), generator=g, dtype=torch.int32).to(DEV)
        idx[:, ::2] = 5
        if same:
            idx[:] = N - 1
        t1 = onehot_scatter(src.reshape(B, rows, d), idx.reshape(B, rows), N)
        assert torch.equal(t1.long(), _int_sum(src, idx, N)) and torch.equal(t1, t1.round())
        assert torch.equal(t1, onehot_scatter(src.reshape(B, rows, d), idx.reshape(B, rows), N))
