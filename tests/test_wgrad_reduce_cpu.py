"""CPU: the emulation of the weight-gradient reductions' two documented orders (tests/wgrad_reduce_ref.py) is a sum -- within
S units of roundoff of the partials' absolute mass against fp64 -- and is sensitive to the order: on values of mixed magnitude
it differs in bits from a plain left-to-right sum and from the other order.  That keeps the GPU test's bit assertions
(tests/test_wgrad_reduce_gpu.py) honest: they can see a changed order."""
import numpy as np
import pytest

import wgrad_reduce_ref as ref

U = 2.0 ** -24


def _mixed(rng, shape):
    """fp32 values over sixteen binades: reassociating their sum changes its rounding."""
    return (rng.standard_normal(shape) * np.exp2(rng.integers(-8, 9, shape))).astype(np.float32)


def _left_to_right(parts):
    t = np.zeros(parts.shape[1:], np.float32)
    for s in range(parts.shape[0]):
        t = t + parts[s]
    return t


@pytest.mark.parametrize("S", [1, 3, 7, 8, 9, 13, 20, 37])
def test_both_orders_are_sums_to_S_units_of_roundoff(S):
    parts = _mixed(np.random.default_rng(40 + S), (S, 500))
    exact, mass = parts.astype(np.float64).sum(axis=0), np.abs(parts.astype(np.float64)).sum(axis=0)
    for name, fn in (("eight chains", ref.sum_eight_chains), ("eight ranges", ref.sum_eight_ranges)):
        got = fn(parts)
        assert got.dtype == np.float32 and got.shape == (500,)
        err = np.abs(got.astype(np.float64) - exact)
        print(f"S = {S}, {name}: worst error / bound {float((err / (S * U * mass)).max()):.3f}")
        assert bool((err <= S * U * mass).all())


def test_the_orders_differ_in_bits_from_a_plain_sum_and_from_each_other():
    parts = _mixed(np.random.default_rng(7), (37, 4096))
    chains, ranges, plain = ref.sum_eight_chains(parts), ref.sum_eight_ranges(parts), _left_to_right(parts)
    for a, b, what in ((chains, plain, "eight chains / plain"), (ranges, plain, "eight ranges / plain"),
                       (chains, ranges, "eight chains / eight ranges")):
        differ = int((a.view(np.uint32) != b.view(np.uint32)).sum())
        print(f"{what}: {differ} of {a.size} sums differ in bits")
        assert differ > a.size // 10


def test_layout_walks_agree_with_the_strided_sums():
    """linear_reduce / fragment_reduce on a workspace = the order's sum over each element's own partials, db from part 0."""
    rng = np.random.default_rng(3)
    S, N, K = 9, 6, 10
    ws = _mixed(rng, S * (N * K + N))
    dw, db = ref.linear_reduce(ws, S, N, K)
    assert np.array_equal(dw, ref.sum_eight_chains(ws.reshape(S, -1)[:, : N * K]).reshape(N, K))
    assert np.array_equal(db, ref.sum_eight_chains(ws.reshape(S, -1)[:, N * K:]))
    S, nta, ktb, N, K = 13, 16, 8, 40, 256          # two column parts
    stride = ref.fragment_stride(nta, ktb)
    ws = _mixed(rng, 2 * S * stride)
    base_w, base_b = _mixed(rng, (N, K)), _mixed(rng, N)
    dw, db = ref.fragment_reduce(ws, S, nta, ktb, N, K, base_w, base_b, accumulate=True)
    for n, k in ((0, 0), (5, 127), (17, 128), (39, 255)):
        mine = np.array([ws[ref.fragment_offset(S, nta, ktb, n, k) + s * stride] for s in range(S)], np.float32)
        assert dw[n, k] == np.float32(base_w[n, k] + ref.sum_eight_ranges(mine))
    assert ref.fragment_offset(S, nta, ktb, 0, 128) == S * stride
    assert db[7] == np.float32(base_b[7] + ref.sum_eight_ranges(ws[nta * ktb * 256 + 7:S * stride:stride]))
    offs = {ref.fragment_offset(S, nta, ktb, n, k) for n in range(N) for k in range(K)}
    assert len(offs) == N * K and max(o % (S * stride) for o in offs) < nta * ktb * 256
