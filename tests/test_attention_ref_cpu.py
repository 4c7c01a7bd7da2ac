"""The error envelope of tests/attention_ref.py against a plain fp32 implementation of the kernels' formulas, on the CPU.

This validates the envelope, not the kernels: the online softmax / saved lse / yb = y - r formulation evaluated in torch
fp32 stays within E_EMUL envelopes of the fp64 autograd reference from residual scale 0 to 2^12 and logit offset 0 to +-1000,
and the comparison helper rejects a single element 16 envelopes off while accepting one a quarter of an envelope off."""
import pytest
import torch

import attention_ref as ar


def _sweep(dtype):
    worst = {}
    for form, (shape, token) in ar.SWEEP_SHAPES.items():
        if form == "atomic":          # (the shape of "stream")
            continue
        for i, (sp, off, rs, tok) in enumerate(ar.conditioning_cases(token)):
            c = ar.make_post_case(shape, 100 + i, dtype, "cpu", sp, off, rs, tok)
            ref, env = ar.post_reference(**c)
            E = ar.measure(ar.emulate_post(**c), ref, env)
            for name, v in E.items():
                if v >= worst.get(name, (0.0,))[0]:
                    worst[name] = (v, form, sp, off, rs, tok)
    return worst


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_emulation_stays_inside_the_envelope(dtype):
    worst = _sweep(dtype)
    for name, v in sorted(worst.items()):
        print(f"{dtype} {name}: E = {v[0]:.3f} at form {v[1]}, spread {v[2]}, offset {v[3]}, residual {v[4]}, token {v[5]}")
    assert set(worst) == {"y", "da", "dvf", "dpos", "da_g", "dv_g"}
    top = max(v[0] for v in worst.values())
    assert top <= ar.E_EMUL, worst
    assert top >= 0.05, "the envelope is far wider than what fp32 arithmetic does: it would pin nothing"


def test_envelope_sees_the_two_sensitivities():
    """yb = y - r and the fp32 lse cost what the envelope says: the measured error grows with the residual scale / the common
    offset about as the envelope does (E stays of order one), while the envelope of the well-conditioned case is far smaller."""
    shape = ar.SWEEP_SHAPES["stream"][0]
    base = ar.make_post_case(shape, 7, rscale=1.0)
    big_r = ar.make_post_case(shape, 7, rscale=2.0 ** 12)
    big_o = ar.make_post_case(shape, 7, offset=1000.0)
    e = {}
    for name, c in (("base", base), ("r", big_r), ("o", big_o)):
        ref, env = ar.post_reference(**c)
        got = ar.emulate_post(**c)
        err = {kk: (got[kk].double() - ref[kk]).abs() for kk in ("da", "dpos")}
        e[name] = {kk: float((err[kk] / ref[kk].abs().clamp_min(1e-30)).median()) for kk in err}
        assert max(ar.measure(got, ref, env).values()) <= ar.E_EMUL
    assert e["r"]["da"] > 100 * e["base"]["da"]          # 2^12 x the residual: ~1000 x the error of da
    assert e["o"]["dpos"] > 20 * e["base"]["dpos"]        # |lse| = 1000: ~100 x the error of the weights


@pytest.mark.parametrize("shape,token,qb", [((7, 3, 4, 2, 12), False, False), ((3, 20, 5, 3, 8), True, True)])
def test_pre_and_sub_forms(shape, token, qb):
    B, n, N, k, d = shape
    g = torch.Generator().manual_seed(3)
    mk = lambda *s: torch.randn(*s, generator=g)
    q, kf, pos, du = mk(B, 1 if qb else n, d), mk(B, N, d), mk(B, n, k, d), mk(B, n, k, d)
    idx = torch.randint(0, N, (B, n, k), generator=g, dtype=torch.int32)
    ref, env = ar.pre_reference(q, kf, pos, idx, du)
    ar.assert_within(ar.emulate_pre(q, kf, pos, idx, du), ref, env, ar.E_EMUL, "pre")
    # sub=(kf, q): `pos` holds u, the values are u + (v + k)[idx] - q: the same numbers as the plain form on pos
    c = ar.make_post_case(shape, 5, token="rand" if token and qb else None)
    u = ar.emulate_pre(q, kf, c["pos"], idx)["u"]
    cs = dict(c, pos=u, idx=idx, sub=(kf, q))
    ref_s, env_s = ar.post_reference(**cs)
    ref_p, _ = ar.post_reference(**dict(c, idx=idx))
    for name in ref_p:
        assert float((ref_s[name] - ref_p[name]).abs().max()) <= 1e-5 * (1 + float(ref_p[name].abs().max())), name
    ar.assert_within(ar.emulate_post(**cs), ref_s, env_s, ar.E_EMUL, "sub")


def test_comparison_helper_rejects_16_envelopes_and_accepts_a_quarter():
    shape, token = ar.SWEEP_SHAPES["lds"]
    c = ar.make_post_case(shape, 11, token="lo")
    ref, env = ar.post_reference(**c)
    for name in ref:
        flat = ref[name].reshape(-1)
        for pos in (0, flat.numel() // 2, flat.numel() - 1):
            for factor, ok in ((16.0, False), (0.25, True)):
                got = {kk: v.clone() for kk, v in ref.items()}
                got[name].reshape(-1)[pos] += factor * env[name].reshape(-1)[pos]
                if ok:
                    assert ar.assert_within(got, ref, env, ar.gpu_bound())[name] == pytest.approx(0.25, rel=1e-6)
                else:
                    with pytest.raises(AssertionError, match=name):
                        ar.assert_within(got, ref, env, ar.gpu_bound())
    # the regime the old `2e-5 (max + 1)` bound hid: a token gradient ~1e-17 of the others is still judged at its own scale
    assert float(ref["dv_g"].abs().max()) < 1e-12 and float((env["dv_g"] / ref["dv_g"].abs()).max()) < 1e-2
