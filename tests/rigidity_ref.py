"""The yardstick of the local-rigidity tests: CPU, fp64, evaluated on the fp32 inputs as they are.

  * ``resid64``: the residuals r = |p_i - p_l|^2 - |s_i - s_l|^2 [B, n, K] with the two squared lengths (what the residual's
    error envelope scales with: r itself cancels);
  * ``loss64``: the loss through plain fp64 torch -> (loss, terms [B]), differentiable with respect to P;
  * ``from_resid``: terms and loss in fp64 for residuals that are GIVEN;
  * ``closed_form``: the gradient in closed form **with the residuals given** -- the kernel's own fp32 residuals go in, so the
    gradient check is about the gather-reduce and nothing else, and no case is ever left out because a residual cancels.  It
    also returns, per element, the sum of the absolute values of the terms and, per row, the length of its list (its in-degree);
  * ``depth`` / ``envelope_c`` and the constants: the roundings a number goes through, from the operation order documented in
    include/nsdp_rigidity.h (``depth`` and the switches are tests/list_order_ref.py's);
  * ``ordered``: the gradient rebuilt in fp32 in exactly that order, the residuals given -- what the kernel's bits are held to.
"""
import numpy as np
import torch

from list_order_ref import LANE_MAX, WAVE_MAX, depth, ordered_sum      # noqa: F401  (re-exported: the tests read them here)

U = 2.0 ** -24                  # unit roundoff of fp32, round to nearest
# |resid - exact| <= RESID_C * U * (cur + rest): five first-order roundings in ((dx^2 + dy^2) + dz^2) of rounded differences
# (2 from a rounded difference squared, the product, two additions) on either side and the subtraction's one, 6 in all; 8 leaves
# the kind of room chamfer_ref.DIST_SLACK leaves (16 over 10) for second-order terms and the yardstick's own rounding.
RESID_C = 8
# terms and loss are reduced in double (products of two fp32 are exact there; n K <= 2^25 additions at 2^-53 each stay below
# 2^-28) and rounded to fp32 once: 1 first-order rounding, one more unit for the double reduction and the yardstick.
TERMS_C = 2
# gradient: a term passes c = fp32(w / (B n K)) (1), g * c (1), the difference (1), the product with r (1), own + list (1), the
# final product (1) = 6, plus the additions of its sum; one more unit covers the second-order part and the yardstick.
GRAD_C0 = 7


def _gather(X, idx):
    """X [B, n, 3], idx [B, n, K] -> X[b, idx[b, i, j]] [B, n, K, 3]."""
    B, n, K = idx.shape
    return torch.gather(X, 1, idx.long().reshape(B, n * K, 1).expand(B, n * K, 3)).reshape(B, n, K, 3)


def resid64(P, S, idx):
    """-> (r, cur, rest) [B, n, K] in fp64."""
    P, S = P.double(), S.double()
    cur = ((P[:, :, None, :] - _gather(P, idx)) ** 2).sum(-1)
    rest = ((S[:, :, None, :] - _gather(S, idx)) ** 2).sum(-1)
    return cur - rest, cur, rest


def from_resid(resid, weight=1.0):
    """(loss, terms [B]) in fp64 for given residuals [B, n, K]."""
    terms = (resid.double() ** 2 / 4.0).mean(dim=(1, 2))
    return weight * terms.mean(), terms


def loss64(P, S, idx, weight=1.0):
    """(loss, terms [B]) in fp64; differentiable with respect to P where it is an fp64 leaf."""
    return from_resid(resid64(P, S, idx)[0], weight)


def autograd64(P, S, idx, weight=1.0):
    """(loss, dP) through fp64 autograd."""
    P64 = P.double().requires_grad_(True)
    loss, _ = loss64(P64, S, idx, weight)
    loss.backward()
    return loss.detach(), P64.grad


def in_degrees(idx):
    B, n, K = idx.shape
    return torch.zeros(B, n, dtype=torch.int64).scatter_add_(1, idx.long().reshape(B, n * K), torch.ones(B, n * K, dtype=torch.int64))


def closed_form(P, idx, resid, weight=1.0, g=1.0):
    """-> (grad [B, n, 3] fp64, sum of |terms| [B, n, 3] fp64, list length per row [B, n] int64) for residuals [B, n, K] given:
    dL/dp_i = g c ( sum_j r_ij (p_i - p_idx[i,j])  +  sum_{e in list(i)} r_e (p_i - p_{e div K}) ),  c = w / (B n K)."""
    P, r = P.double(), resid.double()
    B, n, K = idx.shape
    c = g * weight / (B * n * K)
    edge = r[:, :, :, None] * (P[:, :, None, :] - _gather(P, idx))          # r_ij (p_i - p_l): to row i; its negative: to row l
    to = idx.long().reshape(B, n * K, 1).expand(B, n * K, 3)
    flat = edge.reshape(B, n * K, 3)
    grad = edge.sum(dim=2) + torch.zeros_like(P).scatter_add_(1, to, -flat)
    mass = edge.abs().sum(dim=2) + torch.zeros_like(P).scatter_add_(1, to, flat.abs())
    return c * grad, abs(c) * mass, in_degrees(idx)


def ordered(P, idx, resid, weight=1.0, g=1.0):
    """d L / d P [B, n, 3] in fp32, every operation rounded once and in the kernel's order: fl(fl(g c) fl(own + S)) with
    c = fp32(w / (B n K)) divided in double, own the row's K columns r_ij (p_i - p_idx[i,j]) added to 0 in column order and S
    the ordered sum of r_e (p_i - p_{e div K}) over the entries e that name row i, ascending."""
    P, idx, r = P.numpy(), idx.long().numpy(), resid.numpy()
    B, n, K = idx.shape
    gc = np.float32(g) * np.float32(np.float64(np.float32(weight)) / (np.float64(B) * n * K))
    out = np.empty_like(P)
    for b in range(B):
        own = np.zeros((n, 3), dtype=np.float32)
        for j in range(K):
            own = own + r[b, :, j, None] * (P[b] - P[b][idx[b, :, j]])
        flat, rf = idx[b].reshape(-1), r[b].reshape(-1)
        lists = [np.flatnonzero(flat == i) for i in range(n)]
        summed = np.stack([ordered_sum(rf[e, None] * (P[b, i] - P[b][e // K])) for i, e in enumerate(lists)])
        out[b] = gc * (own + summed)
    assert out.dtype == np.float32
    return torch.from_numpy(out)


def envelope_c(lengths, K):
    """c of |grad - exact| <= c * 2^-24 * sum |terms|, per row: GRAD_C0 + the deeper of the two sums of the row -- the own
    columns (K - 1 additions) and the list (depth(T))."""
    return (GRAD_C0 + depth(lengths).clamp_min(K - 1)).double()
