"""Every form of the dense-layer kernels (csrc/gemm.hip, gemm_bf16x3.hip / x3_kernel.h, wgrad_bf16x3.hip, gemm_bf16.hip, k4*.h)
against the fp64 reference of tests/dense_ref.py.

The bound is per element: E = max |got - ref64| / env <= BOUND = 2 max(1, E_EMUL), env the first-order rounding envelope of a dot
product in fp32 (no absolute constant, no scaling by the tensor's maximum) and E_EMUL what CPU emulations of the documented
arithmetic reach (dense_ref.py; tests/test_dense_ref_cpu.py proves for every case here that a lost product of the bf16x3 split
and a neighbour's bias / residual lie outside BOUND).  Every case asserts the kernel variant that ran through the variant trace;
forms are selected by shape, by nsdp_debug_set and by module attributes (restored in ``finally``), so the file does not depend
on the knob matrix.  Integer operands are compared exactly.

Branches of launch_x3 (csrc/gemm_bf16x3.hip) and the case that reaches each:

    resident weights (NT <= 8, K <= 128), prologue 0 / 2        resident-pre0 / resident-pre2
    two 4-wave workgroups (NT <= 8, K > 128), prologue 0 / 2    two-wg-pre0 / two-wg-pre2
    NT = 13 register-activation form, prologue 0 / 2            nt13-xreg / nt13-xreg-pre2
    NT = 13 8-wave form (M > 2^19)                              nt13-8wave
    NT = 16, three / two row tiles per wave                     nt16-wide / nt16-narrow
    masked prologue at NT <= 8 / NT = 13 / NT = 16              mask-nt8 / mask-nt13 / mask-nt16

each at one workgroup tile with a ragged last row tile and at num_cus * wgs_per_cu * rows_per_workgroup + 77 rows.
"""
import contextlib
import ctypes

import pytest
import torch

import dense_ref as dr

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
F32, BF = torch.float32, torch.bfloat16
_ci = ctypes.c_int


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


@contextlib.contextmanager
def _x3_debug(value):
    """nsdp_debug_set(6, value) around a launch (0 = the default dispatch of launch_x3)."""
    from nsdp_amd import _lib
    _lib.lib().nsdp_debug_set(_ci(6), _ci(value))
    try:
        yield
    finally:
        _lib.lib().nsdp_debug_set(_ci(6), _ci(0))


@contextlib.contextmanager
def _attrs(mod, **kw):
    was = {kk: getattr(mod, kk) for kk in kw}
    try:
        for kk, v in kw.items():
            setattr(mod, kk, v)
        yield
    finally:
        for kk, v in was.items():
            setattr(mod, kk, v)


def _ran(names, want, prefix=False):
    hit = [n for n in names if (n.startswith(want) if prefix else n == want)]
    assert hit, (want, sorted(names))


def _num_cus():
    return torch.cuda.get_device_properties(DEV).multi_processor_count


# ----------------------------------------------------------------------------------------------------------------------
# running the kernels
# ----------------------------------------------------------------------------------------------------------------------
def run_x3(c, dbg=0):
    from nsdp_amd import hip_linear as hl
    wp = hl.pack_weight_x3(c["w"])[0]
    with _x3_debug(dbg), _Trace() as tr:
        if c["gather"] is not None:
            y = hl._fwd_x3_gather(c["x"], wp, c["N"], c["b"], c["gather"], c["relu_in"], c["relu_out"])
        else:
            y = hl._fwd_x3(c["x"], wp, c["N"], c["b"], c["res"], c["mask"], c["out_mask"], c["relu_in"], c["relu_out"],
                           res_sign=c["res_sign"], addend=c["addend"])
        torch.cuda.synchronize()
    return y, tr.names


def run_f32(c, packed):
    from nsdp_amd import hip_linear as hl
    with _Trace() as tr:
        if packed:
            y = hl._fwd_wp(c["x"], hl.pack_weight(c["w"])[0], c["N"], c["b"], c["res"], c["mask"], c["out_mask"], c["relu_in"],
                           c["relu_out"])
        else:
            y = hl._fwd(c["x"], c["w"], c["b"], c["res"], c["mask"], c["out_mask"], c["relu_in"], c["relu_out"])
        torch.cuda.synchronize()
    return y, tr.names


def run_bf16(c, out_f32):
    from nsdp_amd import hip_linear_bf16 as hb
    with _Trace() as tr:
        y = hb.run(c["x"], hb.pack_weight_b16(c["w"])[0], c["N"], c["b"], c["res"], c["mask"], c["out_mask"], c["relu_in"],
                   c["relu_out"], out_f32=out_f32)
        torch.cuda.synchronize()
    return y, tr.names


def run_wgrad(c, family):
    """(dw, db), traced names; with an existing gradient the kernels accumulate into copies of it."""
    from nsdp_amd import hip_linear as hl, hip_linear_bf16 as hb
    out = None if c["acc_w"] is None else (c["acc_w"].clone(), c["acc_b"].clone())
    with _Trace() as tr:
        if family == "x3":
            got = hl._wgrad_x3(c["dy"], c["x"], c["mask"], c["relu_x"], True, out)
        elif family == "bf16":
            got = hb.wgrad(c["dy"], c["x"], c["mask"], c["relu_x"], True, out)
        else:
            with _attrs(hl, _USE_X3=False):          # (the exact-fp32 kernels at every row count)
                got = hl._wgrad(c["dy"], c["x"], c["mask"], c["relu_x"], True, out)
        torch.cuda.synchronize()
    assert out is None or got[0] is out[0]
    return got, tr.names


# ----------------------------------------------------------------------------------------------------------------------
# judging
# ----------------------------------------------------------------------------------------------------------------------
def _sample(M):
    """Above 100 000 rows: the first and last 256 rows and 4096 sampled ones."""
    if M <= 100_000:
        return None
    g = torch.Generator(device=DEV).manual_seed(M)
    return torch.cat([torch.arange(0, 256, device=DEV), torch.arange(M - 256, M, device=DEV),
                      torch.randint(0, M, (4096,), device=DEV, generator=g)])


def judge_forward(c, got, family, what, fails, out_dtype=None):
    """Bounded kinds: E against BOUND (printed, collected in ``fails``); exact kinds: equality with the rounded fp64 result."""
    kind = c["kind"]
    idx = _sample(c["M"])
    if idx is not None:
        c, got = dr.take_rows(c, idx), got[idx]
    ref, env = dr.forward_reference(c, out_dtype=out_dtype)
    if kind == "ints":
        assert torch.equal(got, ref.to(got.dtype)), (what, float((got.double() - ref).abs().max()))
        return
    if kind == "predicates":          # whole-number operands: a wrong decision is an error of one at least
        tol = dr.predicate_tolerance(c, ref, got.dtype, c["K"])
        err = got.double() - ref
        zero = ref.abs() < 0.5
        assert float(tol[~zero].max()) < 0.5 or got.dtype is BF, (what, float(tol.max()))
        print(f"\npredicates[{what}] max |err| = {float(err.abs().max()):.3g}, towards zero at {int((err * ref.sign() < 0).sum())}, "
              f"away at {int((err * ref.sign() > 0).sum())} of {err.numel()} elements")
        assert bool((err.abs() <= tol).all()), (what, float(err.abs().max()))
        return
    E = dr.measure(got, ref, env)
    B = dr.bound("fwd", family, kind, c["K"])
    print(f"\nE[{what}] = {E:.3f} (bound {B:g})")
    if kind == "floor":
        _, rel = dr.forward_reference(c, out_dtype=out_dtype, with_floor=False)
        print(f"E[{what}, without the floor term] = {dr.measure(got, ref, rel):.3f}")
    if not E <= B:
        fails.append((what, E, B))


def judge_wgrad(c, got, family, what, fails):
    kind = c["kind"]
    ref, env = dr.wgrad_reference(c)
    if kind == "ints":
        for g, kk in zip(got, ("dw", "db")):
            assert torch.equal(g, ref[kk].float()), (what, kk, float((g.double() - ref[kk]).abs().max()))
        return
    if kind == "predicates":
        tol = dr.predicate_tolerance(c, None, F32, c["M"])
        tol["db"] = torch.zeros_like(tol["db"])          # (column sums of whole numbers: no addend carries a subnormal)
        for g, kk in zip(got, ("dw", "db")):
            err = g.double() - ref[kk]
            assert float(tol[kk].max()) < 0.5, (what, kk, float(tol[kk].max()))
            print(f"\npredicates[{what}] {kk}: max |err| = {float(err.abs().max()):.3g}, towards zero at "
                  f"{int((err * ref[kk].sign() < 0).sum())}, away at {int((err * ref[kk].sign() > 0).sum())} of {err.numel()} elements")
            assert bool((err.abs() <= tol[kk]).all()), (what, kk, float(err.abs().max()))
        return
    E = {kk: dr.measure(g, ref[kk], env[kk]) for g, kk in zip(got, ("dw", "db"))}
    B = dr.bound("wgrad", family, kind)
    print(f"\nE[{what}] dw={E['dw']:.3f} db={E['db']:.3f} (bound {B:g})")
    if kind == "floor":
        _, rel = dr.wgrad_reference(c, with_floor=False)
        print(f"E[{what}, without the floor term] dw={dr.measure(got[0], ref['dw'], rel['dw']):.3f}")
    if not max(E.values()) <= B:
        fails.append((what, E, B))


# ----------------------------------------------------------------------------------------------------------------------
# 1. the exact-fp32 forward kernels
# ----------------------------------------------------------------------------------------------------------------------
F32_TRACE = {(1, 4, 16): "linear_nt<4,1,0>", (37, 120, 120): "linear_nt<1,4,0>", (129, 256, 256): "linear_nt<1,4,0>",
             (300, 128, 3): "linear_nt<4,1,2>"}


@pytest.mark.parametrize("packed", [False, True], ids=["row-major", "packed"])
@pytest.mark.parametrize("shape,flags", dr.F32_FORWARD, ids=[f"{m}x{k}x{n}" for (m, k, n), _ in dr.F32_FORWARD])
def test_linear_f32_against_fp64(shape, flags, packed):
    """nsdp_linear_f32 / nsdp_linear_wp_f32, every kind; integers exactly and bit-equal run to run."""
    M, K, N = shape
    fails = []
    for kind in dr.BOUNDED_KINDS + ("ints",):
        c = dr.make_case(kind, M, K, N, flags, dr.case_seed(f"f32-{M}x{K}x{N}", kind), DEV)
        y, names = run_f32(c, packed)
        _ran(names, F32_TRACE[shape] + (" wp" if packed else ""), prefix=True)
        judge_forward(c, y, "f32", f"f32{'-wp' if packed else ''} {M}x{K}x{N} {kind}", fails)
        if kind == "ints":
            assert torch.equal(y, run_f32(c, packed)[0])
    assert not fails, fails


# ----------------------------------------------------------------------------------------------------------------------
# 2. bf16x3 forward: every branch of launch_x3, two row counts
# ----------------------------------------------------------------------------------------------------------------------
def _x3_rows(entry, rows):
    _, _, _, _, _, per_wg, wgs, _, grid_rows = entry
    return per_wg - 5 if rows == "tile" else _num_cus() * wgs * grid_rows + 77


@pytest.mark.parametrize("rows", ["tile", "grid"])
@pytest.mark.parametrize("entry", dr.X3_FORWARD, ids=[e[0] for e in dr.X3_FORWARD])
def test_bf16x3_form_against_fp64(entry, rows):
    name, _, (K, N), flags, variant, _, _, dbg, _ = entry
    M = _x3_rows(entry, rows)
    fails = []
    for kind in dr.BOUNDED_KINDS + ("ints",):
        c = dr.make_case(kind, M, K, N, flags, dr.case_seed(name, kind), DEV)
        y, names = run_x3(c, dbg)
        _ran(names, variant)
        judge_forward(c, y, "x3", f"x3 {name} {rows} M={M} {kind}", fails)
        if kind == "ints":
            assert torch.equal(y, run_x3(c, dbg)[0])
    assert not fails, fails


def test_bf16x3_eight_wave_form_against_fp64():
    """13 n tiles above 2^19 rows: the 8-wave form, at the smallest row count that reaches it; sampled rows."""
    name, _, (M, K, N), flags, variant = dr.X3_EIGHT_WAVE
    fails = []
    for kind in dr.BOUNDED_KINDS + ("ints",):
        c = dr.make_case(kind, M, K, N, flags, dr.case_seed(name, kind), DEV)
        y, names = run_x3(c)
        _ran(names, variant)
        judge_forward(c, y, "x3", f"x3 {name} M={M} {kind}", fails)
        if kind == "ints":
            assert torch.equal(y, run_x3(c)[0])
        del c, y
    torch.cuda.empty_cache()
    assert not fails, fails


@pytest.mark.parametrize("entry", dr.X3_EPILOGUES, ids=[e[0] for e in dr.X3_EPILOGUES])
def test_bf16x3_epilogue_against_fp64(entry):
    """Output mask, signed residual, addend after the mask and both gather forms, at the smallest row count hip_linear routes
    to the bf16x3 kernel."""
    from nsdp_amd import hip_linear as hl
    name, (_, K, N), flags, variant = entry
    M = hl._X3_MIN_ROWS + 77
    with _attrs(hl, _USE_X3=True):
        assert hl._x3_ok(M, N, K) and not hl._x3_ok(hl._X3_MIN_ROWS - 1, N, K)
        if "gather" in flags or "gather1" in flags:
            assert hl.gather_init_ok(M, N, K)
    fails = []
    for kind in dr.BOUNDED_KINDS + ("ints",):
        c = dr.make_case(kind, M, K, N, flags, dr.case_seed(name, kind), DEV)
        y, names = run_x3(c)
        _ran(names, variant)
        judge_forward(c, y, "x3", f"x3 {name} M={M} {kind}", fails)
        if kind == "ints":
            assert torch.equal(y, run_x3(c)[0])
    assert not fails, fails


# ----------------------------------------------------------------------------------------------------------------------
# 3. the bf16 pair
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("out_f32", [False, True], ids=["bf16-out", "fp32-out"])
@pytest.mark.parametrize("shape", dr.BF16_FORWARD, ids=[f"{m}x{k}x{n}" for m, k, n in dr.BF16_FORWARD])
def test_linear_bf16_against_fp64(shape, out_f32):
    M, K, N = shape
    fails = []
    for kind in dr.BOUNDED_KINDS + ("ints",):
        flags = tuple(f for f in dr.BF16_FLAGS if not (out_f32 and f == "res"))          # (fp32 output: no residual)
        c = dr.make_case(kind, M, K, N, flags, dr.case_seed(f"bf16-{M}x{K}x{N}", kind), DEV, dtype=BF)
        y, names = run_bf16(c, out_f32)
        _ran(names, "linear_bf16<", prefix=True)
        judge_forward(c, y, "bf16", f"bf16 {M}x{K}x{N} {kind} out={'f32' if out_f32 else 'bf16'}", fails,
                      out_dtype=F32 if out_f32 else BF)
        if kind == "ints":
            assert torch.equal(y, run_bf16(c, out_f32)[0])
    assert not fails, fails


# ----------------------------------------------------------------------------------------------------------------------
# 4. weight gradients
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("acc", [False, True], ids=["fresh", "accumulate"])
@pytest.mark.parametrize("entry", dr.WGRAD, ids=[e[0] for e in dr.WGRAD])
def test_weight_gradient_against_fp64(entry, acc):
    """dW, db of every weight-gradient kernel; ``accumulate``: into an existing gradient of 2^20 times the update, whose
    rounding unit the envelope then carries."""
    name, family, (M, N, K), flags, variant = entry
    dt = BF if family == "bf16" else F32
    fails = []
    for kind in dr.BOUNDED_KINDS + ("ints",):
        c = dr.make_case(kind, M, K, N, flags + (("acc",) if acc else ()), dr.case_seed(name, kind), DEV, dtype=dt, op="wgrad")
        got, names = run_wgrad(c, family)
        _ran(names, variant, prefix=True)
        judge_wgrad(c, got, family, f"wgrad {name} {kind}{' acc' if acc else ''}", fails)
        if kind == "ints":
            again, _ = run_wgrad(c, family)
            assert torch.equal(got[0], again[0]) and torch.equal(got[1], again[1])
    assert not fails, fails


# ----------------------------------------------------------------------------------------------------------------------
# 5. the floor of the split
# ----------------------------------------------------------------------------------------------------------------------
def test_bf16x3_forward_at_the_floor():
    """Rows at 2^-118: within the bound with the floor term; E without it is printed (DESIGN 4g records what the hardware does
    with planes below the smallest normal bf16)."""
    entry = dr.X3_FORWARD[2]
    name, _, (K, N), flags, variant, _, _, dbg, _ = entry
    M = _x3_rows(entry, "tile")
    c = dr.make_case("floor", M, K, N, flags, dr.case_seed(name, "floor"), DEV)
    y, names = run_x3(c, dbg)
    _ran(names, variant)
    fails = []
    judge_forward(c, y, "x3", f"x3 {name} floor", fails)
    assert not fails, fails


def test_bf16x3_weight_gradient_at_the_floor():
    entry = dr.WGRAD[3]
    name, family, (M, N, K), flags, variant = entry
    assert family == "x3"
    c = dr.make_case("floor", M, K, N, flags, dr.case_seed(name, "floor"), DEV, op="wgrad")
    got, names = run_wgrad(c, family)
    _ran(names, variant, prefix=True)
    fails = []
    judge_wgrad(c, got, family, f"wgrad {name} floor", fails)
    assert not fails, fails


# ----------------------------------------------------------------------------------------------------------------------
# 6. predicates: signed zeros and the smallest subnormals in masks and pre-ReLU inputs
# ----------------------------------------------------------------------------------------------------------------------
PRED_FLAGS = (("mask", "omask", "bias"), ("relu_in", "relu_out", "bias", "res"), ("mask", "omask", "addend"))
PRED_FLAGS_BF16 = ((("mask", "bias"), True), (("relu_in", "relu_out", "bias"), True), (("mask", "omask", "bias", "res"), False))


@pytest.mark.parametrize("family", ["f32", "x3", "bf16"])
def test_forward_predicates(family):
    """``mask > 0`` and ``max(x, 0)`` at -0.0, +0.0 and the smallest subnormals of either sign, on integer operands: the result
    is the reference's up to the subnormal addends themselves."""
    shapes = {"f32": [(129, 120, 120)], "x3": [(123, 36, 120), (187, 200, 200), (123, 256, 256)], "bf16": [(129, 120, 120)]}[family]
    dt = BF if family == "bf16" else F32
    for M, K, N in shapes:
        for fl, out_f32 in (PRED_FLAGS_BF16 if family == "bf16" else [(f, True) for f in PRED_FLAGS]):
            if "addend" in fl and family != "x3":
                continue
            c = dr.make_case("predicates", M, K, N, fl, dr.case_seed(family, "predicates") + K, DEV, dtype=dt)
            if family == "x3":
                y, names = run_x3(c)
                _ran(names, "linear_bf16x3<", prefix=True)
            elif family == "bf16":          # (fp32 output where the kernel has it: a bf16 output rounds whole numbers above 256)
                y, names = run_bf16(c, out_f32)
                _ran(names, "linear_bf16", prefix=True)
            else:
                y, names = run_f32(c, True)
                _ran(names, "linear_nt<", prefix=True)
            judge_forward(c, y, family, f"{family} predicates {M}x{K}x{N} {fl}", [], out_dtype=y.dtype)


@pytest.mark.parametrize("family", ["f32", "x3", "bf16"])
def test_weight_gradient_predicates(family):
    dt = BF if family == "bf16" else F32
    for entry in (e for e in dr.WGRAD if e[1] == family and e[2][2] > 4):
        name, _, (M, N, K), _, _ = entry
        M = min(M, 2049)          # (the tolerance grows with the number of addends: kept under half a unit)
        c = dr.make_case("predicates", M, K, N, ("mask", "relu_x"), dr.case_seed(name, "predicates"), DEV, dtype=dt, op="wgrad")
        got, names = run_wgrad(c, family)
        _ran(names, {"f32": "linear_wgrad", "x3": "wgrad_bf16x3<", "bf16": "wgrad_bf16"}[family], prefix=True)
        judge_wgrad(c, got, family, f"wgrad {name} predicates", [])


# ----------------------------------------------------------------------------------------------------------------------
# 7. exact probes of the remaining forms: G16, H0, the K = 4 tail
# ----------------------------------------------------------------------------------------------------------------------
def test_g16_pair_on_integers():
    """Linear -> ReLU -> Linear with the hidden tensor in the G16 layout (_fwd_x3_g16): the fp64 result exactly."""
    from nsdp_amd import hip_linear as hl
    M, K, H, N = hl._X3_MIN_ROWS + 16, 120, 120, 120
    with _attrs(hl, _USE_X3=True, G16=True):
        assert hl.g16_pair_ok(M, K, H, N, train=False)
    c0 = dr.make_case("ints", M, K, H, ("bias", "relu_out"), 11, DEV)
    c1 = dr.make_case("ints", M, H, N, ("bias", "res"), 12, DEV)
    c1["w"] = torch.randint(-1, 2, (N, H), generator=torch.Generator().manual_seed(3)).float().to(DEV)      # (sums below 2^24)
    h_ref, _ = dr.forward_reference(c0)
    c1["x"] = h_ref.float()
    y_ref, _ = dr.forward_reference(c1)
    assert float(y_ref.abs().max()) < 2.0 ** 24
    for _ in range(2):
        with _Trace() as tr:
            h = hl._fwd_x3_g16(c0["x"], hl.pack_weight_x3(c0["w"])[0], H, c0["b"], None, None, None, False, True, hl.LAY_Y)
            y = hl._fwd_x3_g16(h, hl.pack_weight_x3(c1["w"])[0], N, c1["b"], c1["res"], None, None, False, False, hl.LAY_X)
            torch.cuda.synchronize()
        assert any(n.endswith(" g16:y") for n in tr.names) and any(n.endswith(" g16:x") for n in tr.names), sorted(tr.names)
        assert torch.equal(hl.to_g16(h, back=True), h_ref.float())
        assert torch.equal(y, y_ref.float())


def _int_mlp(k, d, seed):
    g = torch.Generator().manual_seed(seed)
    seq = torch.nn.Sequential(torch.nn.Linear(k, d), torch.nn.ReLU(), torch.nn.Linear(d, d)).to(DEV)
    with torch.no_grad():
        for p, hi in zip(seq.parameters(), (2, 2, 1, 2)):
            p.copy_(torch.randint(-hi, hi + 1, p.shape, generator=g).float())
    seq64 = torch.nn.Sequential(torch.nn.Linear(k, d), torch.nn.ReLU(), torch.nn.Linear(d, d)).to(DEV).double()
    seq64.load_state_dict(seq.state_dict())
    return seq, seq64, g


def _mlp_exact(fn, seq, seq64, x, t, want):
    """Forward and all four parameter gradients of the two-layer MLP equal fp64 exactly; a second run is bit-equal."""
    (seq64(x[:, :seq64[0].in_features].double()) * t.double()).sum().backward()
    runs = []
    for _ in range(2):
        seq.zero_grad()
        with _Trace() as tr:
            y = fn()
            (y * t).sum().backward()
            torch.cuda.synchronize()
        assert any(want(n) for n in tr.names), sorted(tr.names)
        runs.append([y.detach()] + [p.grad.clone() for p in seq.parameters()])
    with torch.no_grad():
        assert torch.equal(runs[0][0], seq64(x[:, :seq64[0].in_features].double()).float())
    for a, b, p64 in zip(runs[0][1:], runs[1][1:], seq64.parameters()):
        assert float(p64.grad.abs().max()) < 2.0 ** 24
        assert torch.equal(a, p64.grad.float()) and torch.equal(a, b)


def test_h0_form_on_integers():
    """ops.pos_mlp with the hidden layer recomputed inside the second GEMM and its weight gradient (H0_RECOMPUTE = 2)."""
    from nsdp_amd import hip_linear as hl
    from nsdp_amd.model import ops
    k, d, M = 4, 128, hl._X3_MIN_ROWS + 77
    seq, seq64, g = _int_mlp(k, d, 21)
    x = torch.randint(-2, 3, (M, k), generator=g).float().to(DEV)
    t = torch.randint(-1, 2, (M, d), generator=g).float().to(DEV)
    with _attrs(hl, H0_RECOMPUTE=2, K4_LINK=True, K4_TAIL=True, REMASK_K4=True, _USE_X3=True, _PARAM_GRADS_DIRECT=True), \
            _attrs(ops, PAIR_MASK=False):
        y = ops.pos_mlp(x, seq)
        assert y is not None
        _mlp_exact(lambda: ops.pos_mlp(x, seq), seq, seq64, x, t,
                   lambda n: n.startswith("linear_bf16x3<") and n.split("<")[1].split(",")[2] == "3")


def test_k4_tail_on_integers():
    """ops.mlp2 on coordinates without a gradient: the second layer's dX GEMM forms the first layer's dW / db in its epilogue."""
    from nsdp_amd import hip_linear as hl
    from nsdp_amd.model import ops
    k, d, M = 4, 200, 65_536 + 17
    seq, seq64, g = _int_mlp(k, d, 22)
    x = torch.randint(-2, 3, (M, k), generator=g).float().to(DEV)
    t = torch.randint(-1, 2, (M, d), generator=g).float().to(DEV)
    with _attrs(hl, H0_RECOMPUTE=0, K4_LINK=True, K4_TAIL=True, REMASK_K4=True, _USE_X3=True, _PARAM_GRADS_DIRECT=True), \
            _attrs(ops, PAIR_MASK=False):
        _mlp_exact(lambda: ops.mlp2(x, seq), seq, seq64, x, t, lambda n: "k4tail" in n)
