"""What is done with the deformation gradient J = d f / d x of a decoded deformation (``decode(..., jacobian=True)``,
include/nsdp_jacobian.h): plain torch on ``[..., 3, 3]`` tensors, any device and floating dtype.  A packed set (RaggedPoints
over ``[cap, 9]``, what the ragged decode returns) is taken as its ``[cap, 3, 3]`` rows and, where the result is per point, comes
back packed over the same offsets.

    cofactor(J)              cof(J) = det(J) J^-T, formed from cross products of J's columns: no inverse, defined for singular J
    transform_normals(J, n)  the normal of a surface element carried through the deformation, n' = cof(J) n / |cof(J) n|
    determinant(J)           local volume change; det <= 0 is a fold-over
    fold_overs(J, offsets)   count of det <= 0 per shape
    compose(J2, J1)          chain rule of two deformations applied one after the other: J2 @ J1
"""
from __future__ import annotations

import torch

from .ragged import RaggedPoints


def _rows(J):
    """[..., 3, 3] view of a Jacobian operand (a RaggedPoints over [cap, 9] -> [cap, 3, 3])."""
    if isinstance(J, RaggedPoints):
        J = J.packed
        if J.dim() != 2 or J.shape[1] != 9:
            raise ValueError(f"a packed Jacobian set is [cap, 9] rows, got {tuple(J.shape)}")
        return J.view(-1, 3, 3)
    if J.dim() < 2 or tuple(J.shape[-2:]) != (3, 3):
        raise ValueError(f"a Jacobian is [..., 3, 3], got {tuple(J.shape)}")
    return J


def cofactor(J):
    """cof(J)[:, j] = J[:, j+1] x J[:, j+2] (indices mod 3): the matrix with J^T cof(J) = det(J) I."""
    M = _rows(J)
    c0, c1, c2 = M[..., :, 0], M[..., :, 1], M[..., :, 2]
    return torch.stack([torch.linalg.cross(c1, c2), torch.linalg.cross(c2, c0), torch.linalg.cross(c0, c1)], dim=-1)


def determinant(J):
    """det J = J[:, 0] . (J[:, 1] x J[:, 2]) -> [...]."""
    M = _rows(J)
    return (M[..., :, 0] * torch.linalg.cross(M[..., :, 1], M[..., :, 2])).sum(-1)


def transform_normals(J, n):
    """Unit normals n [..., 3] carried through the deformation: cof(J) n, normalised.  No inverse is formed, so a singular J
    gives a finite result (the zero vector where cof(J) n vanishes).  A packed J with a RaggedPoints n -> a RaggedPoints."""
    packed = n if isinstance(n, RaggedPoints) else None
    v = packed.packed if packed is not None else n
    out = torch.nn.functional.normalize((cofactor(J) @ v.unsqueeze(-1)).squeeze(-1), dim=-1, eps=1e-30)
    return packed.like(out) if packed is not None else out


def fold_overs(J, offsets=None):
    """Count of points with det J <= 0 per shape -> int64 [B].  J [B, V, 3, 3]: per leading row.  A RaggedPoints, or J [cap, 3, 3]
    with ``offsets`` [B + 1]: per shape of the packed set (rows at or beyond offsets[B] are not counted)."""
    if isinstance(J, RaggedPoints):
        offsets = J.offsets if offsets is None else offsets
    M = _rows(J)
    bad = determinant(M) <= 0
    if offsets is None:
        if M.dim() != 4:
            raise ValueError(f"fold_overs without offsets takes [B, V, 3, 3], got {tuple(M.shape)}")
        return bad.sum(dim=1)
    if M.dim() != 3:
        raise ValueError(f"fold_overs with offsets takes packed [cap, 3, 3] rows, got {tuple(M.shape)}")
    offsets = offsets.to(device=M.device, dtype=torch.int64)
    csum = torch.cat([bad.new_zeros(1, dtype=torch.int64), bad.to(torch.int64).cumsum(0)])
    return csum[offsets[1:]] - csum[offsets[:-1]]


def compose(J2, J1):
    """The Jacobian of x -> f2(f1(x)): J2 (taken at f1(x)) @ J1 (taken at x).  Two packed sets -> a packed set."""
    out = _rows(J2) @ _rows(J1)
    if isinstance(J1, RaggedPoints):
        return J1.like(out.reshape(-1, 9))
    return out
