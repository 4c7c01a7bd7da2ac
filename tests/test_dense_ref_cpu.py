"""The error envelope of tests/dense_ref.py against CPU emulations of the dense kernels' documented arithmetic.

This validates the envelope and the cases, not the kernels.  Four duties:

* envelope validity: the emulations of the three families (bf16x3 split, exact-fp32 chain, bf16 operands), each in its two
  accumulation models, stay within E_EMUL envelopes of the fp64 reference for every kind and K in {36, 200, 256}, and on every
  case of tests/test_dense_forms_gpu.py;
* the GPU bound is BOUND = 2 max(1, E_EMUL) -- fixed here, from the reference's own emulation, never from a kernel's output;
* condition: for every case the GPU file runs, each single-product mutation of the split (one of the six plane products
  dropped) lies outside BOUND, and so does the bias of the neighbouring column / the residual of the neighbouring row;
* exactness: on integer operands every emulation equals fp64 exactly.
"""
import pytest
import torch

import dense_ref as dr

FAMILY_DTYPE = {"x3": dr.F32, "f32": dr.F32, "bf16": dr.BF}
SWEEP_FLAGS = (("bias", "res", "relu_out"), ("bias", "mask", "omask"), ("relu_in",))
SWEEP_N = 64
MODELS = ("block", "product")


def _fwd_E(c, family, model, **kw):
    """E of one emulated forward case with fp32 output (the bf16 family has both output types: the smaller E of a mutation, the
    larger of a faithful emulation, are what the callers compare -- ``pick``)."""
    pick = kw.pop("pick", max)
    E = []
    for out in ((dr.F32, dr.BF) if family == "bf16" else (dr.F32,)):
        ref, env = dr.forward_reference(c, out_dtype=out)
        E.append(dr.measure(dr.emulate_forward(c, family, model, out_dtype=out, **kw), ref, env))
    return pick(E)


def _forward_cases_of(family, kc):
    return [c for c in dr.forward_cases() if c[1] == family and dr.k_class(c[3]) == kc]


@pytest.mark.parametrize("kc", [36, 200, 256])
@pytest.mark.parametrize("kind", dr.BOUNDED_KINDS + ("floor",))
@pytest.mark.parametrize("family", ["x3", "f32", "bf16"])
def test_emulations_stay_inside_the_envelope(family, kind, kc):
    """E of both accumulation models over the conditioning shapes (96 x K x 64, three flag sets) and the GPU file's cases."""
    dt = FAMILY_DTYPE[family]
    todo = [(f"sweep{i}", kc, SWEEP_N, fl) for i, fl in enumerate(SWEEP_FLAGS)]
    todo += [(name, K, N, fl) for name, _, _, K, N, fl in _forward_cases_of(family, kc)]
    worst = (0.0, None)
    for name, K, N, fl in todo:
        c = dr.make_case(kind, dr.CPU_ROWS, K, N, fl, dr.case_seed(name, kind), dtype=dt)
        for model in MODELS:
            E = _fwd_E(c, family, model)
            worst = max(worst, (E, f"{name} {model}"))
    print(f"\nE_emul[fwd {family} {kind} K<={kc}] = {worst[0]:.2f} at {worst[1]}")
    assert worst[0] <= dr.e_emul("fwd", family, kind, kc), worst
    if kind != "floor":          # (at 2^-118 the floor term is 2^16 relative envelopes wide: it states a precondition, it pins nothing)
        assert worst[0] >= 0.05, "the envelope is far wider than what fp32 arithmetic does: it would pin nothing"


def _wgrad_case(entry, kind, acc=False):
    name, family, (M, N, K), fl, _ = entry
    fl = fl + (("acc",) if acc else ())
    return dr.make_case(kind, M, K, N, fl, dr.case_seed(name, kind), dtype=FAMILY_DTYPE[family], op="wgrad")


def _wgrad_E(c, family, model, **kw):
    ref, env = dr.wgrad_reference(c)
    got = dr.emulate_wgrad(c, family, model, **kw)
    return {kk: dr.measure(got[kk], ref[kk], env[kk]) for kk in ref}


@pytest.mark.parametrize("kind", dr.BOUNDED_KINDS + ("floor",))
@pytest.mark.parametrize("family", ["x3", "f32", "bf16"])
def test_wgrad_emulations_stay_inside_the_envelope(family, kind):
    """The GPU file's own weight-gradient cases (slabs, per-workgroup partials, ordered sum), both models."""
    worst = (0.0, None)
    for entry in (e for e in dr.WGRAD if e[1] == family):
        c = _wgrad_case(entry, kind)
        for model in MODELS:
            if model == "product" and entry[2][0] > 3000:          # (thousands of sequential outer products: the block model only)
                continue
            E = _wgrad_E(c, family, model)
            worst = max(worst, (max(E.values()), f"{entry[0]} {model} {E}"))
    print(f"\nE_emul[wgrad {family} {kind}] = {worst[0]:.2f} at {worst[1]}")
    assert worst[0] <= dr.e_emul("wgrad", family, kind), worst


def test_accumulating_into_a_large_gradient_is_one_rounding_of_it():
    """accumulate: the existing gradient is 2^20 times the update, so u |existing| is the whole envelope and the emulation's
    error is the final addition's: E <= 1 for every family."""
    for entry in dr.WGRAD:
        if entry[2][0] > 3000:
            continue
        c = _wgrad_case(entry, "unit", acc=True)
        ref, _ = dr.wgrad_reference(dict(c, acc_w=None, acc_b=None))
        assert float((c["acc_w"].double().abs() / ref["dw"].abs().clamp_min(1e-300)).median()) > 2.0 ** 19
        E = _wgrad_E(c, entry[1], "block")
        assert max(E.values()) <= 1.0, (entry[0], E)


def test_bound_is_twice_the_emulation():
    for op, fams in dr.E_EMUL.items():
        for family, kinds in fams.items():
            for kind, e in kinds.items():
                for K, v in (e.items() if isinstance(e, dict) else [(None, e)]):
                    assert dr.bound(op, family, kind, K) == 2.0 * max(1.0, v)
                    assert 0.0 < v <= 12.0          # (an emulation dozens of envelopes off would mean a wrong envelope)


X3_FWD = [c for c in dr.forward_cases() if c[1] == "x3"]


@pytest.mark.parametrize("kind", dr.BOUNDED_KINDS)
@pytest.mark.parametrize("case", X3_FWD, ids=[c[0] for c in X3_FWD])
def test_a_lost_split_product_lies_outside_the_bound(case, kind):
    name, family, dt, K, N, fl = case
    c = dr.make_case(kind, dr.CPU_ROWS, K, N, fl, dr.case_seed(name, kind), dtype=dt)
    B = dr.bound("fwd", "x3", kind, K)
    E = [_fwd_E(c, "x3", "block", drop=i) for i in range(6)]
    print(f"\nmutations[{name} {kind}] bound {B:g}: " + " ".join(f"{n}={e:.1f}" for n, e in zip(dr.PLANE_NAMES, E)))
    assert min(E) > B, (B, dict(zip(dr.PLANE_NAMES, E)))


X3_WG = [e for e in dr.WGRAD if e[1] == "x3"]


@pytest.mark.parametrize("kind", dr.BOUNDED_KINDS)
@pytest.mark.parametrize("entry", X3_WG, ids=[e[0] for e in X3_WG])
def test_a_lost_split_product_of_the_weight_gradient_lies_outside_the_bound(entry, kind):
    c = _wgrad_case(entry, kind)
    B = dr.bound("wgrad", "x3", kind)
    E = [_wgrad_E(c, "x3", "block", drop=i)["dw"] for i in range(6)]
    print(f"\nmutations[{entry[0]} {kind}] bound {B:g}: " + " ".join(f"{n}={e:.1f}" for n, e in zip(dr.PLANE_NAMES, E)))
    assert min(E) > B, (B, dict(zip(dr.PLANE_NAMES, E)))


WITH_SIDE = [c for c in dr.forward_cases() if "bias" in c[5] or "res" in c[5] or "res-" in c[5]]


@pytest.mark.parametrize("kind", dr.BOUNDED_KINDS)
@pytest.mark.parametrize("case", WITH_SIDE, ids=[c[0] for c in WITH_SIDE])
def test_a_neighbours_bias_or_residual_lies_outside_the_bound(case, kind):
    name, family, dt, K, N, fl = case
    c = dr.make_case(kind, dr.CPU_ROWS, K, N, fl, dr.case_seed(name, kind), dtype=dt)
    B = dr.bound("fwd", family, kind, K)
    for which in (("bias",) if c["b"] is not None else ()) + (("res",) if c["res"] is not None else ()):
        if which == "bias" and N == 1:
            continue
        E = _fwd_E(c, family, "block", neighbour=which)
        assert E > B, (which, E, B)


def test_cancel_kind_cancels():
    """|y| <= 2^-10 sum |x||w| for the products of the cancel kind, with and without the prologues."""
    for fl in ((), ("mask",), ("relu_in",)):
        c = dr.make_case("cancel", 64, 200, 40, fl, 5)
        xp = dr._pre(c["x"].double(), c["mask"], c["relu_in"])
        y, mag = xp @ c["w"].double().t(), xp.abs() @ c["w"].double().abs().t()
        assert bool((y.abs() <= 2.0 ** -10 * mag).all())
    c = dr.make_case("cancel", 201, 40, 24, ("mask",), 5, op="wgrad")
    ref, env = dr.wgrad_reference(c)
    assert bool((ref["dw"].abs() <= 2.0 ** -10 * env["dw"] / dr.U32).all())


def test_the_split_has_an_underflow_floor():
    """Rows at 2^-118: the m and l planes fall into or under the bf16 subnormals and the split emulation (which keeps
    subnormals) is dozens of RELATIVE envelopes off, while the exact-fp32 chain is not -- the floor term states this."""
    c = dr.make_case("floor", dr.CPU_ROWS, 200, 64, (), 3)
    ref, env = dr.forward_reference(c, with_floor=False)
    e_x3 = dr.measure(dr.emulate_forward(c, "x3", "block"), ref, env)
    e_f32 = dr.measure(dr.emulate_forward(c, "f32", "block"), ref, env)
    print(f"\nE without the floor term at 2^-118: split {e_x3:.1f}, exact fp32 {e_f32:.2f}")
    assert e_x3 > 20.0 and e_f32 < 20.0
    c = dr.make_case("tiny", dr.CPU_ROWS, 200, 64, (), 3)
    ref, env = dr.forward_reference(c, with_floor=False)
    assert dr.measure(dr.emulate_forward(c, "x3", "block"), ref, env) <= 1.3 * dr.e_emul("fwd", "x3", "tiny", 200)


@pytest.mark.parametrize("kind", ["ints", "predicates"])
@pytest.mark.parametrize("family", ["x3", "f32", "bf16"])
def test_integer_operands_are_exact(family, kind):
    """Every emulation equals fp64 exactly on integers of [-8, 8] (sums below 2^24); with the special values of the predicates
    kind up to the subnormal addends an fp32 accumulator holding an integer rounds away."""
    dt = FAMILY_DTYPE[family]
    tol = 0.0 if kind == "ints" else 16 * 256 * float(dr.special_values(dt)[2])
    for name, fam, _, K, N, fl in dr.forward_cases():
        if fam != family:
            continue
        c = dr.make_case(kind, 40, K, N, fl, dr.case_seed(name, kind), dtype=dt)
        ref, _ = dr.forward_reference(c, out_dtype=dr.F32)
        for model in MODELS:
            got = dr.emulate_forward(c, family, model, out_dtype=dr.F32)
            assert float((got.double() - ref).abs().max()) <= tol, (name, model)
    for entry in (e for e in dr.WGRAD if e[1] == family):
        name, _, (M, N, K), fl, _ = entry
        for acc in ((), ("acc",)):
            c = dr.make_case(kind, min(M, 300), K, N, fl + acc, dr.case_seed(name, kind), dtype=dt, op="wgrad")
            ref, _ = dr.wgrad_reference(c)
            for model in MODELS:
                got = dr.emulate_wgrad(c, family, model)
                assert float((got["dw"].double() - ref["dw"]).abs().max()) <= tol, (name, model)
                assert float((got["db"].double() - ref["db"]).abs().max()) <= tol, (name, model)


def test_measure_rejects_one_element():
    c = dr.make_case("rows", 32, 36, 40, ("bias", "omask"), 1)
    ref, env = dr.forward_reference(c)
    got = ref.clone()
    assert dr.measure(got, ref, env) == 0.0
    i = int((env > 0).flatten().nonzero()[0])
    got.view(-1)[i] += 16.0 * env.view(-1)[i]
    assert 15.9 < dr.measure(got, ref, env) < 16.1
    j = int((env == 0).flatten().nonzero()[0])          # a gated element: no envelope, must be exact
    got = ref.clone()
    got.view(-1)[j] = 1e-30
    assert dr.measure(got, ref, env) == float("inf")
