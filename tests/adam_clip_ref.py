"""Host reference of the clipped Adam step (include/nsdp_optim.h): the sum of squares S with float64 additions in EXACTLY the
order the header writes out, the rule (norm, coef, the skip decision), and Adam on g * coef through
``torch.optim.Adam(foreach=False)`` on CPU tensors -- the yardstick tests/test_adam_gpu.py already holds the update to.

Padding with zeros is the order's own: a lane that owns no element keeps its 0.0, and adding +0.0 to a double (a square is never
-0.0) returns its bits, so "the elements a lane owns, ascending" and "four groups of four per lane, absent ones 0" are the same
sequence of roundings."""
import math

import numpy as np
import torch

CHUNK = 4096          # nsdp_adam_chunk_elems()
LANES = 256

# the shapes of tests/test_adam_gpu.py: 1 to 70 001 elements, across the chunk edge; every other tensor misaligned on the GPU
SHAPES = [(1,), (3,), (120, 3), (200, 200), (4095,), (4096,), (4097,), (256, 256), (3, 128), (17, 5, 1), (70001,)]
NUMEL = sum(int(np.prod(s)) for s in SHAPES)


def _halving(a):
    """a[l] += a[l + s] for s = 128, 64, ..., 1 over 256 doubles."""
    a = a.copy()
    s = LANES // 2
    while s >= 1:
        a[:s] = a[:s] + a[s:2 * s]
        s //= 2
    return a[0]


def chunk_partial(g):
    """One chunk (<= 4096 fp32 values): lane l adds the squares of elements 4 (l + 256 j) .. + 3 in ascending order, then the
    halving."""
    g = np.asarray(g, dtype=np.float32).reshape(-1)
    assert 0 < g.size <= CHUNK
    d = np.zeros(CHUNK, dtype=np.float64)
    d[:g.size] = g.astype(np.float64)
    with np.errstate(all="ignore"):
        sq = d * d
    sq = sq.reshape(CHUNK // (4 * LANES), LANES, 4)        # [j, l, k]: element 4 (l + 256 j) + k
    acc = np.zeros(LANES, dtype=np.float64)
    with np.errstate(all="ignore"):                             # (an inf or a NaN among the values is ordinary data)
        for j in range(sq.shape[0]):
            for k in range(4):
                acc = acc + sq[j, :, k]
        return _halving(acc)


def partials(grads):
    """The partials buffer: chunks of every tensor with a gradient in table order (tensor after tensor, chunk after chunk)."""
    out = []
    for g in grads:
        if g is None:
            continue
        flat = np.asarray(g.detach().cpu().numpy() if torch.is_tensor(g) else g, dtype=np.float32).reshape(-1)
        for first in range(0, flat.size, CHUNK):
            out.append(chunk_partial(flat[first:first + CHUNK]))
    return np.array(out, dtype=np.float64)


def sum_partials(p):
    """One workgroup over the partials: lane l takes l, l + 256, ... ascending, then the halving."""
    p = np.asarray(p, dtype=np.float64)
    rows = max(1, -(-p.size // LANES))
    d = np.zeros(rows * LANES, dtype=np.float64)
    d[:p.size] = p
    acc = np.zeros(LANES, dtype=np.float64)
    with np.errstate(all="ignore"):
        for row in d.reshape(rows, LANES):
            acc = acc + row
        return float(_halving(acc))


def ordered_sumsq(grads):
    return sum_partials(partials(grads))


def rule(S, max_norm, skip_nonfinite=False):
    """(norm: double, coef: np.float32, apply: bool) from S."""
    norm = math.sqrt(S) if S == S and S >= 0 else float("nan")
    with np.errstate(all="ignore"):
        c = float(np.float64(max_norm) / (np.float64(norm) + np.float64(1e-6)))
    coef = np.float32(c) if (c < 1.0 or c != c) else np.float32(1.0)
    apply = not (skip_nonfinite and not math.isfinite(S))
    return norm, coef, apply


def grads(seed, step, scale=1.0):
    """The gradient sequence of tests/test_adam_gpu.py (magnitudes 1e-3 ... 10 over the tensors)."""
    g = torch.Generator().manual_seed(1000 * seed + step)
    return [scale * torch.randn(shp, generator=g) * (10.0 ** ((i % 5) - 3)) for i, shp in enumerate(SHAPES)]


def params(seed):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(shp, generator=g) for shp in SHAPES]


def params_agreeing_with(values, first_grads):
    """``values`` with the signs of ``first_grads`` (tensors without a gradient keep theirs): the initial parameters of a run WITH
    weight decay that is compared with the CPU across devices.

    Why: Adam's first step is lr * g' / (|g'| + eps), a sign function wherever |g'| is of the order of eps = 1e-8, and with
    weight decay g' = g * coef + wd * p CANCELS on some of 190 000 random elements.  There the rounding of that one addition --
    fused on the CPU (Tensor.add(param, alpha=wd)), two roundings in the kernel -- is the whole of g': the two devices then take
    first steps that differ by up to 2 lr, and wd carries that into the moments for good (seen with random signs: one element of
    the 200 x 200 tensor, g' = 1.9e-9 against 2.3e-9, parameters apart by 1.5e-5 and its first moment by 1.0e-7 after 12 steps,
    reproduced bit for bit by restating the kernel's operations in numpy on the host -- the kernel does what it says; the
    comparison is ill-conditioned, for either device).  With agreeing signs nothing cancels: the addition's rounding is 2^-24 of
    g', and the step's sensitivity eps * dg' / (|g'| + eps)^2 <= 2^-26 for any |g'|.  Later steps divide by a second moment with
    a history and are smooth in g'."""
    return [v if g is None else v.abs() * torch.where(g < 0, -1.0, 1.0) for v, g in zip(values, first_grads)]


def run(values, grad_steps, max_norm=None, skip_nonfinite=False, **kw):
    """Adam on g * coef on the CPU.  ``values``: initial parameter tensors; ``grad_steps``: per step a list of gradients (None:
    the parameter has none).  Returns (parameters, optimizer, per-step list of (S, norm, coef, apply))."""
    ps = [v.detach().clone().requires_grad_(True) for v in values]
    opt = torch.optim.Adam(ps, foreach=False, **kw)
    log = []
    for gs in grad_steps:
        S = ordered_sumsq(gs)
        norm, coef, apply = rule(S, float("inf") if max_norm is None else max_norm, skip_nonfinite)
        log.append((S, norm, coef, apply))
        if not apply:
            continue
        for p, g in zip(ps, gs):
            # one fp32 multiplication by the fp32 factor (coef == 1: the gradient's own bits)
            p.grad = None if g is None else g.detach().clone() * torch.tensor(coef, dtype=torch.float32)
        opt.step()
    return ps, opt, log
