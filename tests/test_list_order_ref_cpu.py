"""CPU: the emulation of the list reduction's documented order (tests/list_order_ref.py) against a plain fp64 sum -- within
depth(T) units of roundoff of the sum of the terms' absolute values, at the lengths either side of both switches.  It keeps the
yardstick of the GPU tests' bit assertions honest without a GPU."""
import numpy as np
import pytest
import torch

import list_order_ref

U = 2.0 ** -24


@pytest.mark.parametrize("T", [0, 1, 32, 33, 1024, 1025])
def test_ordered_sum_is_a_sum_to_its_depth(T):
    terms = np.random.default_rng(100 + T).standard_normal((T, 3)).astype(np.float32)
    got = list_order_ref.ordered_sum(terms)
    assert got.dtype == np.float32 and got.shape == (3,)
    exact, mass = terms.astype(np.float64).sum(axis=0), np.abs(terms.astype(np.float64)).sum(axis=0)
    d = int(list_order_ref.depth(torch.tensor([T]))[0])
    assert d == {0: 0, 1: 0, 32: 31, 33: 6, 1024: 21, 1025: 12}[T]
    err = np.abs(got.astype(np.float64) - exact)
    print(f"T = {T}: depth {d}, worst error / bound {float((err / np.maximum(d * U * mass, 1e-300)).max()):.3f}")
    assert bool((err <= d * U * mass).all())
