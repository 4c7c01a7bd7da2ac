"""The yardstick of the Chamfer-loss tests: CPU, fp64, evaluated on the fp32 inputs as they are.

  * ``dist2_64``: brute-force squared distances [B, n, m];
  * ``loss64``: the loss through torch's fp64 autograd (min over the brute-force matrix) -> (loss, terms [B]);
  * ``closed_form``: the gradient in closed form for index sets that are GIVEN -- so a near-tie that fp32 and fp64 resolve
    differently never needs a case to be left out: the kernel's own indices go in, after ``assert_minimisers`` has held them to be
    minimisers in fp64 up to the rounding of an fp32 distance.  It also returns, per element, the sum of the absolute values of
    the terms (what an error envelope scales with) and, per row, the length of its list;
  * ``depth`` / ``envelope_c``: the number of roundings a term of the kernel's gradient goes through, from the operation order
    documented in include/nsdp_chamfer.h (``depth`` and the switches are tests/list_order_ref.py's);
  * ``ordered``: the gradient rebuilt in fp32 in exactly that order, for index sets that are given -- what the kernel's bits
    are held to.
"""
import numpy as np
import torch

from list_order_ref import LANE_MAX, WAVE_MAX, depth, ordered_sum      # noqa: F401  (re-exported: the tests read them here)

U = 2.0 ** -24                  # unit roundoff of fp32, round to nearest
DIST_SLACK = 16 * U             # five roundings in ((dx^2 + dy^2) + dz^2) of rounded differences, on either side, and room


def dist2_64(P, Q):
    P, Q = P.double(), Q.double()
    return ((P[:, :, None, :] - Q[:, None, :, :]) ** 2).sum(-1)


def loss64(P, Q, w_pt=1.0, w_tp=1.0):
    """(loss, terms [B]) in fp64; differentiable with respect to P and Q where they require a gradient (fp64 leaves)."""
    d = dist2_64(P, Q)
    terms = w_pt * (d.min(dim=2).values / 2.0).mean(dim=1) + w_tp * (d.min(dim=1).values / 2.0).mean(dim=1)
    return terms.mean(), terms


def autograd64(P, Q, w_pt=1.0, w_tp=1.0):
    """(loss, dP, dQ) through fp64 autograd."""
    P64, Q64 = P.double().requires_grad_(True), Q.double().requires_grad_(True)
    loss, _ = loss64(P64, Q64, w_pt, w_tp)
    loss.backward()
    return loss.detach(), P64.grad, Q64.grad


def _operand(X, Y, idx_x, idx_y, w_direct, w_list, g):
    """d L / d X for X [B, nx, 3], Y [B, ny, 3], idx_x [B, nx] (nearest Y of X), idx_y [B, ny] (nearest X of Y)."""
    X, Y = X.double(), Y.double()
    B, nx, ny = X.shape[0], X.shape[1], Y.shape[1]
    s_d, s_l = g * w_direct / (B * nx), g * w_list / (B * ny)
    direct = X - torch.gather(Y, 1, idx_x.long()[:, :, None].expand(B, nx, 3))
    owner = idx_y.long()[:, :, None].expand(B, ny, 3)
    diffs = torch.gather(X, 1, owner) - Y                       # x_{c(l)} - y_l for every l
    summed = torch.zeros_like(X).scatter_add_(1, owner, diffs)
    summed_abs = torch.zeros_like(X).scatter_add_(1, owner, diffs.abs())
    lengths = torch.zeros(B, nx, dtype=torch.int64).scatter_add_(1, idx_y.long(), torch.ones(B, ny, dtype=torch.int64))
    grad = s_d * direct + s_l * summed
    mass = abs(s_d) * direct.abs() + abs(s_l) * summed_abs
    return grad, mass, lengths


def closed_form(P, Q, idx_pt, idx_tp, w_pt=1.0, w_tp=1.0, g=1.0):
    """-> {'dP', 'dQ'} each (grad [., ., 3] fp64, sum of |terms| [., ., 3] fp64, list length per row [., .] int64)."""
    return {"dP": _operand(P, Q, idx_pt, idx_tp, w_pt, w_tp, g), "dQ": _operand(Q, P, idx_tp, idx_pt, w_tp, w_pt, g)}


def assert_minimisers(P, Q, idx_pt, idx_tp):
    """Every given index is a minimiser of the fp64 distance up to DIST_SLACK, relative."""
    d = dist2_64(P, Q)
    got = torch.gather(d, 2, idx_pt.long()[:, :, None]).squeeze(2)
    best = d.min(dim=2).values
    assert bool((got <= best * (1 + DIST_SLACK)).all()), float(((got - best) / best.clamp_min(1e-300)).max())
    got = torch.gather(d, 1, idx_tp.long()[:, None, :]).squeeze(1)
    best = d.min(dim=1).values
    assert bool((got <= best * (1 + DIST_SLACK)).all()), float(((got - best) / best.clamp_min(1e-300)).max())


def _ordered_operand(X, Y, idx_x, idx_y, w_direct, w_list, g):
    """d L / d X [B, nx, 3] in fp32, every operation rounded once and in the kernel's order: fl(fl(g s_d) d) + fl(fl(g s_l) S)
    with s_d = fp32(w_direct / (B nx)) and s_l = fp32(w_list / (B ny)) divided in double, d = x - y[idx_x] and S the ordered
    sum of x - y_l over the rows l of Y that name x, ascending."""
    X, Y, idx_x, idx_y = X.numpy(), Y.numpy(), idx_x.long().numpy(), idx_y.long().numpy()
    B, nx, ny = X.shape[0], X.shape[1], Y.shape[1]
    gd = np.float32(g) * np.float32(np.float64(np.float32(w_direct)) / (np.float64(B) * nx))
    gl = np.float32(g) * np.float32(np.float64(np.float32(w_list)) / (np.float64(B) * ny))
    out = np.empty_like(X)
    for b in range(B):
        direct = X[b] - Y[b][idx_x[b]]
        summed = np.stack([ordered_sum(X[b, i] - Y[b][np.flatnonzero(idx_y[b] == i)]) for i in range(nx)])
        out[b] = gd * direct + gl * summed
    assert out.dtype == np.float32
    return torch.from_numpy(out)


def ordered(P, Q, idx_pt, idx_tp, w_pt=1.0, w_tp=1.0, g=1.0):
    """-> {'dP', 'dQ'}: the gradients [., ., 3] fp32 with the bits the kernel's documented order gives."""
    return {"dP": _ordered_operand(P, Q, idx_pt, idx_tp, w_pt, w_tp, g), "dQ": _ordered_operand(Q, P, idx_tp, idx_pt, w_tp, w_pt, g)}


def envelope_c(lengths):
    """c of |grad - exact| <= c * 2^-24 * sum |terms|.  A term goes through: the scale s = fp32(w / (B n)) (1), g * s (1), the
    difference (1), depth(T) additions of the list sum, the product with the scale (1) and the final addition (1) -- 5 + depth
    first-order roundings; one more unit covers the second-order part of (1 + u)^c - 1 (c <= 4200 at the limits: below 3e-4 of
    c) and the yardstick's own fp64 rounding."""
    return (6 + depth(lengths)).double()
