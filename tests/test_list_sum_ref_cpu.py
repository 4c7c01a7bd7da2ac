"""CPU: the host reference of the list reductions (tests/list_sum_ref.py) checked on itself -- its sums against fp64 within the
derived bound, its lists against a brute-force search, its sliced rule against a literal walk, and its sensitivity to the order
of the additions on the data the GPU tests generate: without the last an exact GPU comparison could pass for any order."""
import numpy as np
import pytest
import torch

import list_sum_ref as R

# (B, E, N, d, hot source, its entries): the shapes of the GPU tests' generator, small and with a hot source
CASES = [(3, 528, 53, 12, 10, 300), (2, 700, 97, 5, 5, 200), (1, 3000, 1025, 3, 1000, 1030), (2, 36, 5, 4, 2, 9)]


def _case(B, E, N, d, hot, count, seed=0, bf16=False):
    idx = R.make_idx(1000 + seed + E, B, E, N, hot=hot, hot_count=count, empty=(0, N - 1))
    return idx, R.make_terms(2000 + seed + E, (B, E, d), bf16=bf16), R.inverse_lists_ref(idx, N)


@pytest.mark.parametrize("B,E,N,d,hot,count", CASES)
def test_inverse_lists_are_the_brute_force_lists(B, E, N, d, hot, count):
    idx, _, (off, ent) = _case(B, E, N, d, hot, count)
    assert off.dtype == np.int32 and ent.dtype == np.int32 and off.shape == (B, N + 1) and ent.shape == (B, E)
    for b in range(B):
        assert off[b, 0] == 0 and off[b, N] == E
        for s in range(N):
            np.testing.assert_array_equal(ent[b, off[b, s]:off[b, s + 1]], np.nonzero(idx[b] == s)[0])
        assert off[b, hot + 1] - off[b, hot] == count and off[b, 1] == 0 and off[b, N] == off[b, N - 1]


@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
@pytest.mark.parametrize("B,E,N,d,hot,count", CASES)
def test_list_sums_are_sums_within_the_bound(B, E, N, d, hot, count, bf16):
    idx, terms, (off, ent) = _case(B, E, N, d, hot, count, bf16=bf16)
    for b in range(B):
        got = R.list_sums(terms[b], off[b], ent[b])
        assert got.dtype == np.float32 and got.shape == (N, d)
        brute = np.zeros((N, d))
        for e in range(E):
            brute[idx[b, e]] += terms[b, e].astype(np.float64)
        exact = R.exact_sums(terms[b], off[b], ent[b])
        np.testing.assert_allclose(exact, brute, rtol=1e-13, atol=1e-13)
        err, lim = np.abs(got.astype(np.float64) - exact), R.bound(terms[b], off[b], ent[b])
        print(f"worst error / bound {float((err / lim).max()):.3f}")
        assert bool((err <= lim).all())
        empty = np.diff(off[b]) == 0
        assert empty.any() and not got[empty].any() and not np.signbit(got[empty]).any()       # +0, exactly


def test_list_sums_add_one_term_after_the_other():
    """Against the plain loop, bit for bit; and the interpolation form's product is rounded before it is added."""
    idx, terms, (off, ent) = _case(1, 259, 7, 3, 4, 120)
    want = np.zeros((7, 3), dtype=np.float32)
    for s in range(7):
        for e in ent[0, off[0, s]:off[0, s + 1]]:
            want[s] = want[s] + terms[0, e]
    assert np.array_equal(R.list_sums(terms[0], off[0], ent[0]).view(np.int32), want.view(np.int32))
    n = 86
    idx3 = R.make_idx(5, 1, 3 * n, 7, hot=4, hot_count=100)
    off3, ent3 = R.inverse_lists_ref(idx3, 7)
    rows, w = R.make_terms(6, (n, 3)), R.make_weights(7, (3 * n,))
    want = np.zeros((7, 3), dtype=np.float32)
    for s in range(7):
        for e in ent3[0, off3[0, s]:off3[0, s + 1]]:
            want[s] = want[s] + np.float32(w[e]) * rows[e // 3]
    got = R.list_sums(rows, off3[0], ent3[0], w)
    assert np.array_equal(got.view(np.int32), want.view(np.int32))
    err = np.abs(got.astype(np.float64) - R.exact_sums(rows, off3[0], ent3[0], w))
    assert bool((err <= R.bound(rows, off3[0], ent3[0], w)).all())


@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
@pytest.mark.parametrize("B,E,N,d,hot,count", CASES)
def test_the_reference_is_sensitive_to_the_order(B, E, N, d, hot, count, bf16):
    """The same lists summed in descending order: other bits in at least one element of every shape of every case, for the
    generator's fp32 terms and for its bf16 ones."""
    idx, terms, (off, ent) = _case(B, E, N, d, hot, count, bf16=bf16)
    if bf16:
        assert torch.equal(torch.from_numpy(terms).to(torch.bfloat16).float(), torch.from_numpy(terms))
    for b in range(B):
        rev = R.reversed_lists(off[b], ent[b])
        for s in (hot, int(idx[b, 0])):
            np.testing.assert_array_equal(rev[off[b, s]:off[b, s + 1]], ent[b, off[b, s]:off[b, s + 1]][::-1])
        assert R.order_matters(terms[b], off[b], ent[b])
        assert not np.array_equal(R.list_sums(terms[b], off[b], ent[b]), R.list_sums(terms[b], off[b], rev))


def test_sliced_rule_on_a_permuted_long_list():
    """A list over sort_max entries in scrambled order: slice after slice, the stored order inside a slice (a literal walk); the
    same as list order when the list is ascending; other bits than the stored order otherwise, so a kernel test can tell."""
    E, N, hot, count, width = 400, 9, 3, 150, 64
    idx = R.make_idx(11, 1, E, N, hot=hot, hot_count=count)
    terms = R.make_terms(12, (E, 4))
    off, ent = (a[0] for a in R.inverse_lists_ref(idx, N))
    np.testing.assert_array_equal(R.sliced_list_sums(terms, off, ent, slice=width, sort_max=100), R.list_sums(terms, off, ent))
    mixed = ent.copy()
    mixed[off[hot]:off[hot + 1]] = np.random.default_rng(13).permutation(mixed[off[hot]:off[hot + 1]])
    got = R.sliced_list_sums(terms, off, mixed, slice=width, sort_max=100)
    want = R.list_sums(terms, off, mixed)                       # every other list: list order
    acc = np.zeros(4, dtype=np.float32)
    for e0 in range(0, E, width):
        for e in mixed[off[hot]:off[hot + 1]]:
            if e0 <= e < e0 + width:
                acc = acc + terms[e]
    assert not np.array_equal(want[hot], acc)
    want[hot] = acc
    assert np.array_equal(got.view(np.int32), want.view(np.int32))
    # a long list at or under sort_max is left alone
    np.testing.assert_array_equal(R.sliced_list_sums(terms, off, mixed, slice=width, sort_max=count), R.list_sums(terms, off, mixed))
