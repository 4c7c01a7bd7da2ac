"""Numpy emulation of the two fixed summation orders of the weight-gradient reductions, written from the prose at the head of
nsdp_amd/csrc/wgrad_reduce.h (not from the kernels).  Every partial sum is one fp32 addition in the documented sequence, so a
kernel that follows the contract gives these bits and one that reassociates does not.

Linear order (workspace [S][N K + N], nsdp_wgrad_bf16_reduce_batched): eight chains, chain u takes the partials s = 8 j + u of
the whole groups of eight in rising j, the S % 8 partials behind the last whole group go to chain 0 in rising s, and the chains
combine as ((a0 + a1) + (a2 + a3)) + ((a4 + a5) + (a6 + a7)).

Fragment order (workspace [column parts][S][nta ktb 256 + nta 16], nsdp_wgrad_bf16x3_reduce_batched): the partials are cut into
eight ranges of ceil(S / 8) (the last ones shorter or empty); inside a range four chains, chain u taking s = first + 4 j + u of
the whole groups of four, the remainder into chain 0, combined as (c0 + c1) + (c2 + c3); the eight range sums combine through the
tree of the linear order.

Both: the target receives the sum, or target + sum (one more addition) when the descriptor accumulates."""
import numpy as np

F = np.float32


def _tree8(a):
    return ((a[0] + a[1]) + (a[2] + a[3])) + ((a[4] + a[5]) + (a[6] + a[7]))


def sum_eight_chains(parts):
    """parts [S, ...] fp32 -> the eight-chain sum over axis 0."""
    parts = np.asarray(parts)
    assert parts.dtype == F
    S = parts.shape[0]
    a = [np.zeros(parts.shape[1:], F) for _ in range(8)]
    c = 0
    while c + 8 <= S:
        for u in range(8):
            a[u] = a[u] + parts[c + u]
        c += 8
    while c < S:
        a[0] = a[0] + parts[c]
        c += 1
    return _tree8(a)


def sum_four_chains(parts):
    """parts [S, ...] fp32 -> the four-chain sum over axis 0 (S may be 0)."""
    parts = np.asarray(parts)
    assert parts.dtype == F
    S = parts.shape[0]
    a = [np.zeros(parts.shape[1:], F) for _ in range(4)]
    c = 0
    while c + 4 <= S:
        for u in range(4):
            a[u] = a[u] + parts[c + u]
        c += 4
    while c < S:
        a[0] = a[0] + parts[c]
        c += 1
    return (a[0] + a[1]) + (a[2] + a[3])


def sum_eight_ranges(parts):
    """parts [S, ...] fp32 -> eight ranges of ceil(S / 8), four chains in each, the tree over the range sums."""
    parts = np.asarray(parts)
    S = parts.shape[0]
    per = (S + 7) // 8
    return _tree8([sum_four_chains(parts[min(q * per, S):min(q * per + per, S)]) for q in range(8)])


def _store(target, total, accumulate):
    return (target + total).astype(F) if accumulate else total


def linear_reduce(ws, S, N, K, dW=None, db=None, accumulate=False, want_db=True):
    """ws: flat fp32, [S][N K + N].  Returns (dW [N, K], db [N] or None)."""
    parts = np.asarray(ws)[: S * (N * K + N)].reshape(S, N * K + N)
    total = sum_eight_chains(parts)
    out_w = _store(None if dW is None else dW.reshape(-1), total[: N * K], accumulate).reshape(N, K)
    out_b = _store(db, total[N * K:], accumulate) if want_db else None
    return out_w, out_b


def fragment_stride(nta, ktb):
    return nta * ktb * 256 + nta * 16


def fragment_offset(S, nta, ktb, n, k):
    """Offset of partial 0 of dW[n][k] in the workspace: column part k / (16 ktb), then the accumulator tile (n / 16, k / 16 of
    the part), lane 16 ((n % 16) / 4) + k % 16, register n % 4 (the MFMA's C/D layout: row = 4 (lane / 16) + register)."""
    part, kl = k // (16 * ktb), k % (16 * ktb)
    return (part * S * fragment_stride(nta, ktb) + ((n // 16) * ktb + kl // 16) * 256
            + (16 * ((n % 16) // 4) + kl % 16) * 4 + n % 4)


def fragment_reduce(ws, S, nta, ktb, N, K, dW=None, db=None, accumulate=False, want_db=True):
    """ws: flat fp32, [column parts][S][stride].  Returns (dW [N, K], db [N] or None); db from column part 0."""
    ws = np.asarray(ws)
    stride = fragment_stride(nta, ktb)
    n, k = np.meshgrid(np.arange(N), np.arange(K), indexing="ij")
    first = fragment_offset(S, nta, ktb, n, k)
    steps = (np.arange(S) * stride).reshape(S, 1, 1)
    out_w = _store(dW, sum_eight_ranges(ws[first[None] + steps]), accumulate)
    out_b = None
    if want_db:
        slot = nta * ktb * 256 + np.arange(N)
        out_b = _store(db, sum_eight_ranges(ws[slot[None] + steps.reshape(S, 1)]), accumulate)
    return out_w, out_b
