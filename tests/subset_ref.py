"""The numpy emulation of nsdp_subset_draw, from the construction written out in include/nsdp_batch.h (unsigned 32-bit integer
arithmetic only): shared by tests/test_datastore_cpu.py and tests/test_datastore_gpu.py.  Vectorised over rows AND over samples,
so that the 4096-key uniformity cases cost one pass."""
import numpy as np

SURFACE, SPACE = 0, 1
MAX_ROWS = 1 << 20
ROUNDS = 8
_U = np.uint32


def mix32(x):
    x = np.asarray(x, dtype=_U).copy()
    x ^= x >> _U(16)
    x *= _U(0x7FEB352D)
    x ^= x >> _U(15)
    x *= _U(0x846CA68B)
    x ^= x >> _U(16)
    return x


def absorb(h, v):
    with np.errstate(over="ignore"):
        return mix32((np.asarray(h, dtype=_U) ^ np.asarray(v, dtype=_U)) + _U(0x9E3779B9))


def keys(seed, epoch, step, b, which):
    """The key of every sample of ``b`` (array of sample numbers)."""
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    h = _U(0x4E534450)
    for v in (seed & 0xFFFFFFFF, seed >> 32, int(epoch) & 0xFFFFFFFF, int(step) & 0xFFFFFFFF):
        h = absorb(h, v)
    return absorb(absorb(h, np.asarray(b, dtype=_U)), which)


def half_bits(n):
    """h of every n: half of w rounded up, w = the smallest integer with 2^w >= n = the bit length of n - 1; at least 1."""
    w = np.array([(int(v) - 1).bit_length() for v in np.asarray(n).reshape(-1)], dtype=np.int64)
    return np.maximum(1, (w + 1) // 2)


def draw(n_full, n_keep, seed, epoch, step, which, b0=0):
    """rows (B, n_keep) int32 of the samples b0 .. b0 + B - 1 with ``n_full`` (B,) rows each."""
    n = np.clip(np.asarray(n_full, dtype=np.int64).reshape(-1), 1, MAX_ROWS)
    B = n.shape[0]
    key = keys(seed, epoch, step, b0 + np.arange(B), which).reshape(B, 1)
    with np.errstate(over="ignore"):
        rk = [mix32(key + _U(0x85EBCA6B) * _U(r + 1)) for r in range(ROUNDS)]
    h = half_bits(n).astype(_U).reshape(B, 1)
    mask = (_U(1) << h) - _U(1)
    nn = n.astype(_U).reshape(B, 1)
    x = (np.arange(n_keep, dtype=np.int64)[None, :] % n[:, None]).astype(_U)
    todo = np.ones(x.shape, dtype=bool)
    while todo.any():
        L, R = x >> h, x & mask
        for r in range(ROUNDS):
            L, R = R, L ^ (mix32(R ^ rk[r]) >> (_U(32) - h))
        x = np.where(todo, (L << h) | R, x)
        todo &= x >= nn
    return x.astype(np.int32)


def uniformity_violations(rows, n_full, n_keep, sigmas=6.0):
    """Rows whose inclusion count, or count as the FIRST drawn row, over the K samples of ``rows`` (K, n_keep) lies beyond ``sigmas``
    standard deviations of Binomial(K, n_keep / n_full), Binomial(K, 1 / n_full): under a uniform draw a row fails with
    probability below 2e-9, and every case has at most 2000 counts."""
    K = rows.shape[0]
    bad = []
    for what, counts, p in (("inclusion", np.bincount(rows.reshape(-1), minlength=n_full), n_keep / n_full),
                            ("first", np.bincount(rows[:, 0], minlength=n_full), 1.0 / n_full)):
        z = np.abs(counts - K * p) / np.sqrt(K * p * (1.0 - p))
        print(f"n_full={n_full} n_keep={n_keep} {what}: largest deviation {z.max():.2f} sigma")
        bad += [(what, int(r), float(z[r])) for r in np.nonzero(z > sigmas)[0]]
    return bad
