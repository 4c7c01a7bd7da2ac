"""Dense-inference metrics on the GPU (mirror of the reference's utils/eval_metric.py).

``chamfer_distance`` runs the two nearest-neighbour searches on the hand-written HIP kNN kernel (nsdp_knn, k = 1) instead
of two scipy KD-trees on the host; everything stays on the device and only three scalars come back.  ``trimesh`` is
not needed: face normals and the area-weighted surface sampling are computed here.

The ``*_batch`` functions take a whole batch of meshes -- rectangular ``[B, V, 3]`` tensors or the ``RaggedPoints`` a ragged
dense-inference call returns -- in one call: the two searches of the Chamfer metric run on the nearest-neighbour-distance
kernel (nsdp_nn_dist2, include/nsdp_eval.h), the per-shape means on nsdp_segment_mean_f32 (double accumulation in a fixed
order: a shape's numbers do not depend on what else is in the batch), everything between is elementwise on the packed rows,
and nothing is read back: ``{'l2', 'fnc', 'cd'}`` come as ``[B]`` fp32 device tensors and the caller's ``.tolist()`` is the only
synchronisation.  The host never reads an offsets tensor.
"""
from __future__ import annotations

import torch

from . import pointnet2_utils
from ._lib import NsdpHipError
from .ragged import RaggedPoints, shape_ids


def compute_dist_square(vertices: torch.Tensor, vertices_gt: torch.Tensor) -> torch.Tensor:
    """utils/eval_metric.py:6-8."""
    return ((vertices - vertices_gt) ** 2).sum(-1).mean()


def normal_consistency(normals_src: torch.Tensor, normals_tgt: torch.Tensor) -> torch.Tensor:
    """utils/eval_metric.py:11-21 (absolute cosine: flipped normals count as consistent)."""
    a = normals_src / normals_src.norm(dim=-1, keepdim=True)
    b = normals_tgt / normals_tgt.norm(dim=-1, keepdim=True)
    return (a * b).sum(-1).abs().mean()


def nn_distance(query: torch.Tensor, source: torch.Tensor) -> torch.Tensor:
    """Euclidean distance of every query point (n,3) to its nearest source point (m,3) -- HIP kNN kernel, k = 1."""
    q = query.reshape(1, -1, 3).contiguous().float()
    s = source.reshape(1, -1, 3).contiguous().float()
    _, d2 = pointnet2_utils.knn(q, s, 1, return_dist=True)
    return d2.reshape(-1).clamp_min(0).sqrt()


def chamfer_distance(points: torch.Tensor, points_gt: torch.Tensor) -> torch.Tensor:
    """utils/eval_metric.py:23-30: 0.5 * (mean_gt min_p |gt - p| + mean_p min_gt |p - gt|)."""
    completeness = nn_distance(points, points_gt)
    accuracy = nn_distance(points_gt, points)
    return 0.5 * (accuracy.mean() + completeness.mean())


def face_normals(verts: torch.Tensor, faces: torch.Tensor) -> torch.Tensor:
    """Unit normals of the triangles (what ``trimesh.Trimesh(...).face_normals`` supplies to the reference)."""
    v = verts[faces.long()]
    n = torch.cross(v[:, 1] - v[:, 0], v[:, 2] - v[:, 0], dim=-1)
    return n / n.norm(dim=-1, keepdim=True).clamp_min(1e-30)


def sample_surface(verts: torch.Tensor, faces: torch.Tensor, count: int, generator=None):
    """Area-weighted face indices and Dirichlet(1,1,1) barycentric weights (utils/eval_metric.py:52-57: the reference
    takes the face indices from ``mesh_pred.sample`` and draws its own ``np.random.dirichlet`` weights)."""
    v = verts[faces.long()]
    area = torch.cross(v[:, 1] - v[:, 0], v[:, 2] - v[:, 0], dim=-1).norm(dim=-1)
    face_idx = torch.multinomial(area / area.sum(), count, replacement=True, generator=generator)
    e = -torch.log(torch.rand(count, 3, device=verts.device, generator=generator).clamp_min(1e-12))
    return face_idx, e / e.sum(-1, keepdim=True)


def compute_evaluation_metrics(out_dict, pointcloud_size: int = 30000, generator=None):
    """utils/eval_metric.py:33-61: {'l2', 'fnc', 'cd'} for one predicted mesh (same faces as the ground truth)."""
    verts_pred = out_dict["verts_tgt_pred"].squeeze().detach().float()
    verts_gt = out_dict["verts_tgt"].squeeze().float().to(verts_pred.device)
    faces = out_dict["faces"].squeeze().to(verts_pred.device)
    fn_pred, fn_gt = face_normals(verts_pred, faces), face_normals(verts_gt, faces)
    face_idx, alpha = sample_surface(verts_pred, faces, pointcloud_size, generator)
    tri = faces.long()[face_idx]
    points_pred = (alpha[:, :, None] * verts_pred[tri]).sum(1)
    points_gt = (alpha[:, :, None] * verts_gt[tri]).sum(1)
    return {"l2": float(compute_dist_square(verts_pred, verts_gt)),
            "fnc": float(normal_consistency(fn_pred, fn_gt)),
            "cd": float(chamfer_distance(points_pred, points_gt))}


# ------------------------------------------------------------------------------------------------------------------------
# a whole batch of meshes in one call
# ------------------------------------------------------------------------------------------------------------------------
def _rect_offsets(B: int, rows: int, device) -> torch.Tensor:
    """The offsets of B shapes of `rows` rows each, made on the device."""
    return torch.arange(B + 1, device=device, dtype=torch.int32) * int(rows)


def _points(what: str, t, need_gpu: bool = True):
    """The checks every point operand gets -> 'ragged' or 'rect'."""
    ragged = isinstance(t, RaggedPoints)
    x = t.packed if ragged else t
    if not torch.is_tensor(x):
        raise TypeError(f"{what} must be a [B, n, 3] tensor or a RaggedPoints, got {type(t).__name__}")
    if x.shape[-1] != 3 or x.dim() != (2 if ragged else 3):
        raise NsdpHipError(f"{what} must be {'packed [capacity, 3]' if ragged else '[B, n, 3]'}, got {tuple(x.shape)}")
    if x.dtype != torch.float32:
        raise NsdpHipError(f"{what} must be torch.float32, got {x.dtype}")
    if need_gpu and not x.is_cuda:
        raise NsdpHipError(f"{what} must be a GPU tensor (CPU not supported, no fallback)")
    return "ragged" if ragged else "rect"


def _same_batch(what: str, a, b):
    """Both rectangular over one B, or both packed over one batch on one device."""
    la, lb = _points(what + " (first)", a), _points(what + " (second)", b)
    if la != lb:
        raise NsdpHipError(f"{what}: mismatched layouts, one operand is {'packed' if la == 'ragged' else 'rectangular'} and the "
                           f"other {'packed' if lb == 'ragged' else 'rectangular'}")
    if a.device != b.device:
        raise NsdpHipError(f"{what}: operands on {a.device} and {b.device}")
    Ba, Bb = (a.batch, b.batch) if la == "ragged" else (int(a.shape[0]), int(b.shape[0]))
    if Ba != Bb:
        raise NsdpHipError(f"{what}: mismatched layouts, {Ba} shapes against {Bb}")
    return la


def _same_rows(a: RaggedPoints, b: RaggedPoints) -> bool:
    """``RaggedPoints.same_layout`` without its read-back: one offsets tensor, or equal host counts where both sets have them;
    two sets that know their sizes on the device alone are taken at their word (same batch, same capacity)."""
    if a.batch != b.batch or a.capacity != b.capacity:
        return False
    if a.offsets is b.offsets or a._counts is None or b._counts is None:
        return True
    return a._counts == b._counts


def nn_distance2_batch(query, source, return_index: bool = False):
    """Squared distance of every query point to the nearest source point of its own shape.  ``[B, n, 3]`` / ``[B, m, 3]``
    tensors -> ``[B, n]``; two ``RaggedPoints`` over the same batch -> a ``RaggedPoints`` ([capacity, 1]) over the query's
    offsets, rows beyond its total unwritten.  ``return_index``: the index of that source point as well (int32; a packed
    source row in the ragged form) -- the smallest among exact ties."""
    layout = _same_batch("nn_distance2_batch", query, source)
    if layout == "rect":
        return pointnet2_utils.nn_dist2(query.contiguous(), source.contiguous(), return_index)
    out = pointnet2_utils.nn_dist2_ragged(query.packed.contiguous(), query.offsets, source.packed.contiguous(), source.offsets,
                                          return_index)
    if return_index:
        return query.like(out[0].unsqueeze(1)), query.like(out[1].unsqueeze(1))
    return query.like(out.unsqueeze(1))


def chamfer_distance_batch(points, points_gt) -> torch.Tensor:
    """``chamfer_distance`` per shape, ``[B]`` fp32 on the device: 0.5 * (mean accuracy + mean completeness) over each shape's
    own points.  Rectangular ``[B, n, 3]`` / ``[B, m, 3]`` or two ``RaggedPoints`` over the same batch."""
    layout = _same_batch("chamfer_distance_batch", points, points_gt)
    if layout == "rect":
        B, dev = int(points.shape[0]), points.device
        comp = pointnet2_utils.nn_dist2(points.contiguous(), points_gt.contiguous()).reshape(-1)
        acc = pointnet2_utils.nn_dist2(points_gt.contiguous(), points.contiguous()).reshape(-1)
        off_p, off_g = _rect_offsets(B, points.shape[1], dev), _rect_offsets(B, points_gt.shape[1], dev)
    else:
        comp = pointnet2_utils.nn_dist2_ragged(points.packed.contiguous(), points.offsets, points_gt.packed.contiguous(),
                                               points_gt.offsets)
        acc = pointnet2_utils.nn_dist2_ragged(points_gt.packed.contiguous(), points_gt.offsets, points.packed.contiguous(),
                                              points.offsets)
        off_p, off_g = points.offsets, points_gt.offsets
    return 0.5 * (pointnet2_utils.segment_mean(acc, off_g, sqrt=True) + pointnet2_utils.segment_mean(comp, off_p, sqrt=True))


def _mesh_rows(what: str, verts, faces, need_gpu: bool):
    """Vertices and faces of either layout as packed rows -> (verts [R, 3], vertex offsets [B + 1], faces [Q, 3] int64 of LOCAL
    vertex indices, face offsets [B + 1], B).  A rectangular batch gets offsets made on the device."""
    layout = _points(what + ": verts", verts, need_gpu)
    if (layout == "ragged") != isinstance(faces, RaggedPoints):
        raise NsdpHipError(f"{what}: mismatched layouts, the vertices are {'packed' if layout == 'ragged' else 'rectangular'} and "
                           f"the faces are not")
    f = faces.packed if layout == "ragged" else faces
    if not torch.is_tensor(f) or f.dtype not in (torch.int32, torch.int64) or f.shape[-1] != 3 or f.dim() != (2 if layout == "ragged" else 3):
        raise NsdpHipError(f"{what}: faces must be {'packed [capacity, 3]' if layout == 'ragged' else '[B, F, 3]'} int32 / int64 "
                           f"rows of vertex indices, got {tuple(getattr(f, 'shape', ()))} {getattr(f, 'dtype', None)}")
    if f.device != verts.device:
        raise NsdpHipError(f"{what}: vertices on {verts.device}, faces on {f.device}")
    if layout == "ragged":
        if faces.batch != verts.batch:
            raise NsdpHipError(f"{what}: mismatched layouts, {verts.batch} meshes of vertices against {faces.batch} of faces")
        return verts.packed, verts.offsets, f.long(), faces.offsets, verts.batch
    B, V, F = int(verts.shape[0]), int(verts.shape[1]), int(f.shape[1])
    if int(f.shape[0]) != B:
        raise NsdpHipError(f"{what}: mismatched layouts, {B} meshes of vertices against {int(f.shape[0])} of faces")
    return verts.reshape(B * V, 3), _rect_offsets(B, V, verts.device), f.reshape(B * F, 3).long(), _rect_offsets(B, F, f.device), B


def _face_corners(verts_rows, voff, faces_rows, foff, B):
    """The three corners [Q, 3] of every packed face row (rows beyond the last mesh: in-bounds rows of no meaning)."""
    ids = shape_ids(foff, faces_rows.shape[0]).clamp(max=B - 1)
    rows = (faces_rows + voff.long()[ids].unsqueeze(1)).clamp(0, max(int(verts_rows.shape[0]) - 1, 0))
    return verts_rows[rows[:, 0]], verts_rows[rows[:, 1]], verts_rows[rows[:, 2]]


def _cross_rows(a, b):
    """a x b per row, written out (elementwise: a row's bits do not depend on the rows around it)."""
    return torch.stack((a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2],
                        a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]), dim=1)


def _dot_rows(a, b):
    return (a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2]


def sample_surface_batch(verts, faces, count: int, generator=None):
    """``sample_surface`` for every mesh of a batch: -> (face_idx [B, count] int64, bary [B, count, 3]).  ``face_idx`` indexes
    each mesh's OWN faces, drawn in proportion to their areas by the inverse CDF of that mesh (one cumulative sum over the
    packed face rows, in double); ``bary`` are Dirichlet(1,1,1) weights.  Rectangular (verts [B, V, 3], faces [B, F, 3]) or
    ragged (``RaggedPoints`` vertices, faces a ``RaggedPoints`` of int rows with indices local to their mesh).  Torch
    operations only, on whatever device the mesh is, and no host synchronisation."""
    vr, voff, fr, foff, B = _mesh_rows("sample_surface_batch", verts, faces, need_gpu=False)
    count, dev = int(count), vr.device
    v0, v1, v2 = _face_corners(vr, voff, fr, foff, B)
    n = _cross_rows(v1 - v0, v2 - v0).double()
    area = _dot_rows(n, n).sqrt()
    Q = int(fr.shape[0])
    ids = shape_ids(foff, Q)
    cdf = torch.cumsum(torch.where(ids < B, area, torch.zeros_like(area)), dim=0)
    lo = foff.long().clamp(0, Q)
    first, last = lo[:-1], torch.maximum(lo[1:], lo[:-1])
    zero = torch.zeros(1, dtype=cdf.dtype, device=dev)
    cdf0 = torch.cat((zero, cdf))                                   # cdf0[r] = the area of the rows before r
    start, stop = cdf0[first], cdf0[last]
    u = torch.rand(B, count, device=dev, generator=generator, dtype=torch.float64)
    target = start.unsqueeze(1) + u * (stop - start).unsqueeze(1)
    row = torch.searchsorted(cdf, target.reshape(-1).contiguous(), right=True).reshape(B, count)
    row = torch.minimum(torch.maximum(row, first.unsqueeze(1)), (last - 1).clamp(min=0).unsqueeze(1))
    face_idx = (row - first.unsqueeze(1)).clamp(min=0)
    e = -torch.log(torch.rand(B, count, 3, device=dev, generator=generator).clamp_min(1e-12))
    return face_idx, e / e.sum(-1, keepdim=True)


def sample_points(verts, faces, face_idx: torch.Tensor, bary: torch.Tensor) -> torch.Tensor:
    """The points ``[B, count, 3]`` that ``(face_idx, bary)`` of ``sample_surface_batch`` name on the given mesh batch (either
    layout): ``(b0 v0 + b1 v1) + b2 v2`` of the face's corners, elementwise."""
    vr, voff, fr, foff, B = _mesh_rows("sample_points", verts, faces, need_gpu=False)
    if face_idx.dim() != 2 or int(face_idx.shape[0]) != B or tuple(bary.shape) != tuple(face_idx.shape) + (3,):
        raise NsdpHipError(f"sample_points: face_idx [B, count] and bary [B, count, 3] for {B} meshes, got {tuple(face_idx.shape)}, "
                           f"{tuple(bary.shape)}")
    Q, R = int(fr.shape[0]), int(vr.shape[0])
    frow = (face_idx.long() + foff.long()[:-1].unsqueeze(1)).clamp(0, max(Q - 1, 0))
    rows = (fr[frow] + voff.long()[:-1].reshape(B, 1, 1)).clamp(0, max(R - 1, 0))       # [B, count, 3] packed vertex rows
    bary = bary.to(vr.dtype)
    return (bary[:, :, 0:1] * vr[rows[:, :, 0]] + bary[:, :, 1:2] * vr[rows[:, :, 1]]) + bary[:, :, 2:3] * vr[rows[:, :, 2]]


def compute_evaluation_metrics_batch(out_dict, pointcloud_size: int = 30000, generator=None, samples=None):
    """``compute_evaluation_metrics`` for a whole batch in one call: {'l2', 'fnc', 'cd'}, each ``[B]`` fp32 on the device (the
    caller's ``.tolist()`` is the only synchronisation).  ``verts_tgt_pred`` / ``verts_tgt`` are ``[B, V, 3]`` with ``faces``
    ``[B, F, 3]``, or ``RaggedPoints`` over one layout with ``faces`` a ``RaggedPoints`` of int32 rows (indices local to their
    mesh, their own offsets).  ``samples = (face_idx, bary)`` supplies the surface draws (``sample_surface_batch``'s form);
    otherwise ``pointcloud_size`` points per mesh are drawn on the predicted surfaces with ``generator``.  With the same
    ``samples`` a mesh gets the same bits alone, in a rectangular batch and in a ragged one."""
    pred, gt, faces = out_dict["verts_tgt_pred"], out_dict["verts_tgt"], out_dict["faces"]
    if isinstance(pred, RaggedPoints):
        pred = pred.like(pred.packed.detach())
    elif torch.is_tensor(pred):
        pred = pred.detach()
    layout = _same_batch("compute_evaluation_metrics_batch: verts_tgt_pred / verts_tgt", pred, gt)
    if layout == "ragged" and not _same_rows(pred, gt):
        raise NsdpHipError("compute_evaluation_metrics_batch: mismatched layouts, verts_tgt_pred and verts_tgt do not hold the same "
                           "shapes in the same rows")
    if layout == "rect" and pred.shape != gt.shape:
        raise NsdpHipError(f"compute_evaluation_metrics_batch: mismatched layouts, verts_tgt_pred {tuple(pred.shape)} against "
                           f"verts_tgt {tuple(gt.shape)}")
    vp, voff, fr, foff, B = _mesh_rows("compute_evaluation_metrics_batch", pred, faces, need_gpu=True)
    vg = gt.packed if layout == "ragged" else gt.reshape(-1, 3)
    d = vp - vg
    l2 = pointnet2_utils.segment_mean(_dot_rows(d, d).contiguous(), voff)
    p0, p1, p2 = _face_corners(vp, voff, fr, foff, B)
    g0, g1, g2 = _face_corners(vg, voff, fr, foff, B)
    n_p, n_g = _cross_rows(p1 - p0, p2 - p0), _cross_rows(g1 - g0, g2 - g0)
    cos = _dot_rows(n_p, n_g).abs() / (_dot_rows(n_p, n_p).sqrt() * _dot_rows(n_g, n_g).sqrt()).clamp_min(1e-30)
    fnc = pointnet2_utils.segment_mean(cos.contiguous(), foff)
    if samples is None:
        samples = sample_surface_batch(pred, faces, pointcloud_size, generator)
    face_idx, bary = samples
    cd = chamfer_distance_batch(sample_points(pred, faces, face_idx, bary).contiguous(),
                                sample_points(gt, faces, face_idx, bary).contiguous())
    return {"l2": l2, "fnc": fnc, "cd": cd}


# ------------------------------------------------------------------------------------------------------------------------
# a prediction against a scan (or a mesh of another topology): no correspondences
# ------------------------------------------------------------------------------------------------------------------------
def scan_metrics_batch(verts_pred, faces, scan, pointcloud_size: int = 30000, generator=None, samples=None):
    """A batch of predicted meshes against scans that share no rows with them: {'p2s', 's2p', 'cd_surface'}, each ``[B]`` fp32
    on the device, no host synchronisation.  ``p2s``: the per-shape mean (``segment_mean``, sqrt transform) of the EXACT distance
    from every scan point to the predicted surface (``surface_distance.closest_on_mesh``); ``s2p``: the mean distance from
    ``pointcloud_size`` samples of the predicted surface (``sample_surface_batch`` / ``sample_points``, or ``samples =
    (face_idx, bary)``) to their nearest scan point (``nn_dist2``); ``cd_surface``: half their sum.  ``verts_pred`` / ``faces``
    rectangular or ``RaggedPoints`` as for ``compute_evaluation_metrics_batch``; ``scan`` in the same layout with its own
    counts ([B, m, 3], or a ``RaggedPoints`` over the same batch)."""
    from . import surface_distance
    pred = verts_pred
    if isinstance(pred, RaggedPoints):
        pred = pred.like(pred.packed.detach())
    elif torch.is_tensor(pred):
        pred = pred.detach()
    layout = _same_batch("scan_metrics_batch: verts_pred / scan", pred, scan)
    _mesh_rows("scan_metrics_batch", pred, faces, need_gpu=True)
    d2, _, _ = surface_distance.closest_on_mesh(scan, pred, faces, return_bary=False)
    if layout == "ragged":
        B, dev = pred.batch, pred.device
        d2, scan_rows, scan_off = d2.packed.reshape(-1).contiguous(), scan.packed.contiguous(), scan.offsets
    else:
        B, dev = int(pred.shape[0]), pred.device
        d2, scan_rows, scan_off = d2.reshape(-1).contiguous(), scan.reshape(-1, 3).contiguous(), _rect_offsets(B, scan.shape[1], dev)
    p2s = pointnet2_utils.segment_mean(d2, scan_off, sqrt=True)
    if samples is None:
        samples = sample_surface_batch(pred, faces, pointcloud_size, generator)
    face_idx, bary = samples
    pts = sample_points(pred, faces, face_idx, bary).contiguous()                  # [B, count, 3]
    count = int(pts.shape[1])
    back = pointnet2_utils.nn_dist2_ragged(pts.reshape(-1, 3), _rect_offsets(B, count, dev), scan_rows, scan_off)
    s2p = pointnet2_utils.segment_mean(back, _rect_offsets(B, count, dev), sqrt=True)
    return {"p2s": p2s, "s2p": s2p, "cd_surface": 0.5 * (p2s + s2p)}
