"""The documented order of the fixed-order list reduction (nsdp_amd/csrc/list_reduce.h), once, for the tests of every loss whose
backward calls it:

  * ``LANE_MAX`` / ``WAVE_MAX`` / ``depth``: the list lengths at which the reduction switches its form and the additions a term
    passes through in each;
  * ``ordered_sum``: a numpy fp32 emulation of that order -- what the kernel's sum is held to, bit for bit.
"""
import numpy as np
import torch

LANE_MAX, WAVE_MAX = 32, 1024   # the list lengths at which the kernel switches its form


def depth(lengths):
    """Additions a term of a list of that length passes through (tensor of lengths -> tensor)."""
    T = lengths.long()
    lane = (T - 1).clamp_min(0)
    wave = (T + 63) // 64 + 5
    group = (T + 255) // 256 + 7
    return torch.where(T <= LANE_MAX, lane, torch.where(T <= WAVE_MAX, wave, group))


def ordered_sum(terms):
    """terms [T, 3] fp32, the terms of one list in ascending order -> their sum [3] fp32 in the kernel's order.  T <= 32: added
    to 0 one after the other.  T <= 1024: 64 partial sums, partial t of terms t, t + 64, ... added to 0 in that order, then
    halved (a[:32] + a[32:], ...) down to one -- the butterfly, since both partners hold the same bits after every level.
    T > 1024: 256 such partial sums and the same halving, the tree in LDS."""
    terms = np.ascontiguousarray(terms, dtype=np.float32).reshape(-1, 3)
    T = terms.shape[0]
    width = 1 if T <= LANE_MAX else (64 if T <= WAVE_MAX else 256)
    rounds = -(-T // width)
    # (a partial sum starts at +0 and x + (-x) rounds to +0, so it is never -0 and the +0 padding of the last round adds nothing)
    padded = np.zeros((rounds * width, 3), dtype=np.float32)
    padded[:T] = terms
    part = np.zeros((width, 3), dtype=np.float32)
    for block in padded.reshape(rounds, width, 3):
        part = part + block
    while part.shape[0] > 1:
        half = part.shape[0] // 2
        part = part[:half] + part[half:]
    assert part.dtype == np.float32
    return part[0]
