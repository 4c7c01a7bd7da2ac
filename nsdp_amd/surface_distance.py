"""Exact point-to-mesh distance (include/nsdp_surface.h, csrc/surface_distance.hip): for every query point the closest point
of a triangle mesh -- its squared distance, its face and its barycentric coordinates -- and what is built on it:

``closest_on_mesh``          the search, rectangular or ragged
``transfer_vertex_labels``   vertex labels carried to a cloud through ``(face, bary)`` (the form ``EditSession.set_handles`` takes)
``point_to_surface_loss``    the fitting / evaluation recipe: the search without autograd, then the squared distance recomputed in
                             torch with ``(face, bary)`` held constant, so autograd reaches the points and the vertices

``eval_metric.scan_metrics_batch`` scores a predicted mesh against a scan with it.  There is no CPU path and no fallback.

``NSDP_SURFACE_CULL=0`` turns the culling by blocks of faces off (the plain scan: the same bits, the yardstick of the culled
form); docs/KNOBS.md.
"""
from __future__ import annotations

import ctypes
import os

import torch

from ._lib import NsdpHipError, check, fptr, iptr, lib, on_device, optptr, stream_ptr
from .ragged import RaggedPoints, shape_ids

_ci = ctypes.c_int

MAX_BATCH = 65535
MAX_ROWS = 1 << 20              # queries, vertices or faces of one shape
NO_CULL, NO_BOUND = 1, 2        # flags of nsdp_mesh_closest: the plain scan; culling without the bound pass
# The default dispatch, from the sizes the host knows (profiles/surface_distance.txt, docs/EXPERIMENTS.md): with at least this many
# exact tests in the plain scan -- query rows x face rows / shapes -- the call culls by blocks of faces AND reorders queries and
# faces along a Morton curve (a stable sort in torch, once per call; the culling vote is per wave of 64 queries and per block of
# 64 faces, so it needs both to be compact); below it the plain scan is the fastest form: the sort and the two extra passes cost
# more than the culling saves.
AUTO_MIN_TESTS = 1 << 29


def _cull_default():
    """``NSDP_SURFACE_CULL``: 1 -> True (cull whatever the size), 0 -> False (the plain scan), unset -> None (by size)."""
    v = os.environ.get("NSDP_SURFACE_CULL")
    if v is None:
        return None
    if v in ("0", "1"):
        return v == "1"
    raise NsdpHipError(f"NSDP_SURFACE_CULL={v!r}: 0 (the plain scan) or 1 (culling by blocks of faces); unset: by size")


def _large(B: int, qcap: int, fcap: int) -> bool:
    return qcap * fcap >= AUTO_MIN_TESTS * B


def refusal(query, verts, faces):
    """Why ``closest_on_mesh`` cannot take these operands (None: it can), each reason named."""
    given = {"query": query, "verts": verts, "faces": faces}
    ragged = [isinstance(t, RaggedPoints) for t in given.values()]
    if any(ragged) and not all(ragged):
        return ("mismatched layouts: " + ", ".join(f"{n} is {'packed' if r else 'rectangular'}" for n, r in zip(given, ragged))
                + " -- all three are [B, rows, 3] tensors or all three RaggedPoints over one batch")
    rag = all(ragged)
    rows = {n: (t.packed if rag else t) for n, t in given.items()}
    for name, t in rows.items():
        if not torch.is_tensor(t):
            return f"{name} must be a torch.Tensor or a RaggedPoints, got {type(given[name]).__name__}"
    for name in ("query", "verts"):
        if rows[name].dtype is not torch.float32:
            return f"dtype: {name} must be torch.float32, got {rows[name].dtype}"
    if rows["faces"].dtype not in (torch.int32, torch.int64):
        return f"dtype: faces must be torch.int32 or torch.int64 rows of vertex indices, got {rows['faces'].dtype}"
    for name, t in rows.items():
        if t.dim() != (2 if rag else 3) or t.shape[-1] != 3:
            return f"shape: {name} must be {'packed [capacity, 3]' if rag else '[B, rows, 3]'}, got {tuple(t.shape)}"
    batches = {n: (given[n].batch if rag else int(rows[n].shape[0])) for n in given}
    if len(set(batches.values())) != 1:
        return "mismatched batches: " + ", ".join(f"{n} holds {b} shapes" for n, b in batches.items())
    B = batches["query"]
    if not 1 <= B <= MAX_BATCH:
        return f"limits: B = {B} shapes, the entry takes 1 .. {MAX_BATCH}"
    for name, t in rows.items():
        if rag:
            counts = given[name]._counts
            most = max(counts, default=0) if counts is not None else -(-int(t.shape[0]) // B)
            if int(t.shape[0]) < 1:
                return f"limits: {name} has a capacity of 0 rows, the entry takes 1 .. {MAX_ROWS} per shape"
        else:
            most = int(t.shape[1])
            if most < 1:
                return f"limits: {name} holds 0 rows per shape, the entry takes 1 .. {MAX_ROWS}"
        if most > MAX_ROWS or int(t.shape[0]) * (1 if rag else int(t.shape[1])) >= 1 << 31:
            return f"limits: {name} holds {most} rows in a shape, the entry takes 1 .. {MAX_ROWS}"
    for name, t in rows.items():
        if not t.is_cuda:
            return f"CPU tensors: {name} is on the CPU -- the search has no CPU path and there is no fallback"
    for name, t in rows.items():
        if t.device != rows["query"].device:
            return f"devices: query on {rows['query'].device}, {name} on {t.device}"
    return None


def mesh_closest_raw(query, qoff, verts, voff, faces, foff, return_bary: bool = True, cull=None, bound: bool = True):
    """One nsdp_mesh_closest call on packed contiguous GPU operands (faces int32, local indices), outside autograd ->
    (dist2 [qcap], face [qcap] int32 packed face rows, bary [qcap, 3] or None).  ``cull`` None: ``NSDP_SURFACE_CULL``, else by size;
    ``bound`` False: culling without the bound pass (tools/bench_surface.py's comparison)."""
    B, qcap, vcap, fcap = int(qoff.numel()) - 1, int(query.shape[0]), int(verts.shape[0]), int(faces.shape[0])
    if cull is None:
        cull = _cull_default()
    cull = _large(B, qcap, fcap) if cull is None else bool(cull)
    dev = query.device
    L = lib()
    L.nsdp_mesh_closest_workspace_bytes.restype = ctypes.c_size_t
    need = int(L.nsdp_mesh_closest_workspace_bytes(_ci(B), _ci(qcap), _ci(fcap)))
    with on_device(query):
        ws = torch.empty((max(need // 4, 2),), dtype=torch.float32, device=dev)
        dist2 = torch.empty((qcap,), dtype=torch.float32, device=dev)
        face = torch.empty((qcap,), dtype=torch.int32, device=dev)
        bary = torch.empty((qcap, 3), dtype=torch.float32, device=dev) if return_bary else None
        check(L.nsdp_mesh_closest(fptr(query, "query"), iptr(qoff, "query_offsets"), fptr(verts, "verts"), iptr(voff, "vert_offsets"),
                                  iptr(faces, "faces"), iptr(foff, "face_offsets"), _ci(B), _ci(qcap), _ci(vcap), _ci(fcap),
                                  _ci((0 if cull else NO_CULL) | (0 if bound else NO_BOUND)), ctypes.c_void_p(ws.data_ptr()), fptr(dist2), iptr(face), optptr(bary),
                                  stream_ptr()), "nsdp_mesh_closest")
        del ws      # (stream-ordered: the allocator hands the block on behind the launches; a graph's pool keeps it)
    return dist2, face, bary


def _rect_offsets(B, rows, device):
    return torch.arange(B + 1, device=device, dtype=torch.int32) * int(rows)


def _morton_order(points, offsets):
    """A permutation of the packed rows that keeps every shape's rows in its own range (padding rows last) and orders them
    inside it by a 30-bit Morton code of the point in the bounding box of its own shape's rows (so the order of a shape's rows
    is a function of that shape alone); a STABLE sort: equal codes keep their order."""
    cap, B = int(points.shape[0]), int(offsets.numel()) - 1
    ids = shape_ids(offsets, cap)
    # the boxes by atomic minima / maxima (exact, so order-independent) into S slots per shape, rows dealt round over the slots:
    # one slot per shape would serialise a shape's rows on three addresses
    S = max(1, min(256, 4096 // (B + 1)))
    where = (ids * S + torch.arange(cap, device=points.device) % S).unsqueeze(1).expand(-1, 3)
    lo = torch.full(((B + 1) * S, 3), float("inf"), dtype=points.dtype, device=points.device).scatter_reduce(0, where, points, "amin")
    hi = torch.full(((B + 1) * S, 3), float("-inf"), dtype=points.dtype, device=points.device).scatter_reduce(0, where, points, "amax")
    lo, hi = lo.view(B + 1, S, 3).amin(dim=1), hi.view(B + 1, S, 3).amax(dim=1)
    lo, hi = lo[ids], hi[ids]
    q = ((points - lo) / (hi - lo).clamp_min(1e-30) * 1023.0).clamp(0, 1023).long()

    def spread(x):
        x = (x | (x << 16)) & 0x030000FF
        x = (x | (x << 8)) & 0x0300F00F
        x = (x | (x << 4)) & 0x030C30C3
        return (x | (x << 2)) & 0x09249249

    code = spread(q[:, 0]) | (spread(q[:, 1]) << 1) | (spread(q[:, 2]) << 2)
    key = (ids << 30) | code
    return torch.sort(key, stable=True).indices


def closest_on_mesh(query, verts, faces, return_bary: bool = True, cull=None, reorder=None, bound: bool = True):
    """The closest point of mesh ``b`` for every query point of shape ``b``: ``(dist2, face, bary)`` in the query's layout.

    Rectangular: ``query [B, n, 3]``, ``verts [B, V, 3]`` fp32, ``faces [B, F, 3]`` int32 / int64 -> ``dist2 [B, n]`` fp32,
    ``face [B, n]`` int32, ``bary [B, n, 3]`` fp32 (None without ``return_bary``).  Ragged: three ``RaggedPoints`` over one batch,
    the faces int rows with vertex indices local to their mesh -> ``RaggedPoints`` over the query's offsets ([capacity, 1],
    [capacity, 1] int32, [capacity, 3]), rows beyond its total unwritten.  ``face`` is local to its mesh; a mesh without faces
    gives ``FLT_MAX``, -1 and 0.  The arithmetic, its envelope and the tie rule are include/nsdp_surface.h's: among faces whose
    ``dist2`` bits tie, the first in the order the kernel saw wins -- the given order, or with ``reorder`` the Morton order of
    the face centroids (a stable sort, so faces with equal codes keep their order); ``dist2`` is the same bits either way.
    ``cull`` None: ``NSDP_SURFACE_CULL``, and without it by size -- culling from ``AUTO_MIN_TESTS`` exact tests of the plain
    scan on, the plain scan below; ``reorder`` None: wherever the call culls and is that large.  The culled and the plain scan
    give the same bits, and so does ``bound=False`` (culling without the bound pass: the slower form
    tools/bench_surface.py compares).  No host synchronisation; no autograd (``point_to_surface_loss`` for that)."""
    why = refusal(query, verts, faces)
    if why is not None:
        raise NsdpHipError("closest_on_mesh: " + why)
    rag = isinstance(query, RaggedPoints)
    with torch.no_grad():
        if rag:
            B = query.batch
            q, qoff, v, voff, f, foff = query.packed, query.offsets, verts.packed, verts.offsets, faces.packed, faces.offsets
        else:
            B, n, V, F = int(query.shape[0]), int(query.shape[1]), int(verts.shape[1]), int(faces.shape[1])
            dev = query.device
            q, v, f = query.reshape(B * n, 3), verts.reshape(B * V, 3), faces.reshape(B * F, 3)
            qoff, voff, foff = _rect_offsets(B, n, dev), _rect_offsets(B, V, dev), _rect_offsets(B, F, dev)
        q, v, f = q.detach().contiguous(), v.detach().contiguous(), f.to(torch.int32).contiguous()
        if cull is None:
            cull = _cull_default()
        large = _large(B, int(q.shape[0]), int(f.shape[0]))
        cull = large if cull is None else bool(cull)
        if reorder is None:
            reorder = cull and large
        if reorder:
            vrows = (f.long() + voff.long()[shape_ids(foff, int(f.shape[0])).clamp(max=B - 1)].unsqueeze(1)).clamp(0, int(v.shape[0]) - 1)
            centroid = (v[vrows[:, 0]] + v[vrows[:, 1]]) + v[vrows[:, 2]]
            fperm, qperm = _morton_order(centroid, foff), _morton_order(q, qoff)
            d2s, fs, bs = mesh_closest_raw(q[qperm].contiguous(), qoff, v, voff, f[fperm].contiguous(), foff, return_bary, cull, bound)
            d2, face = torch.empty_like(d2s), torch.empty_like(fs)
            d2[qperm] = d2s
            face[qperm] = torch.where(fs >= 0, fperm[fs.long().clamp(0, int(f.shape[0]) - 1)].to(torch.int32), fs)
            bary = None
            if return_bary:
                bary = torch.empty_like(bs)
                bary[qperm] = bs
        else:
            d2, face, bary = mesh_closest_raw(q, qoff, v, voff, f, foff, return_bary, cull, bound)
        # packed face rows -> indices local to their mesh
        first = foff[:-1].clamp(0, int(f.shape[0]))
        if rag:
            base = first[shape_ids(qoff, int(q.shape[0])).clamp(max=B - 1)]
        else:
            base = first.repeat_interleave(n)
        face = torch.where(face >= 0, face - base, face)
    if rag:
        return query.like(d2.unsqueeze(1)), query.like(face.unsqueeze(1)), (query.like(bary) if return_bary else None)
    return d2.reshape(B, n), face.reshape(B, n), (bary.reshape(B, n, 3) if return_bary else None)


def transfer_vertex_labels(vert_labels, faces, face, bary):
    """Vertex labels carried to the queries of ``closest_on_mesh``: one byte per query, the label of the winning face's corner
    with the largest barycentric weight (the first corner among equal weights); a query without a face (-1) gets 0.  One mesh
    (``vert_labels [V]``, ``faces [F, 3]``, ``face [n]``, ``bary [n, 3]``) or a rectangular batch (a leading B on all four).
    The output (uint8, ``[n]`` / ``[B, n]``) is the cloud's ``labels`` of ``EditSession.set_handles(labels=..., vert_labels=...)``
    beside the mesh's own ``vert_labels``.  Plain torch, on whatever device the operands are."""
    if not all(torch.is_tensor(t) for t in (vert_labels, faces, face, bary)):
        raise NsdpHipError("transfer_vertex_labels: vert_labels, faces, face and bary must be tensors")
    single = vert_labels.dim() == 1
    if single:
        vert_labels, faces, face, bary = vert_labels[None], faces[None], face[None], bary[None]
    if vert_labels.dim() != 2 or faces.dim() != 3 or faces.shape[-1] != 3 or face.dim() != 2 or tuple(bary.shape) != tuple(face.shape) + (3,) \
            or not (vert_labels.shape[0] == faces.shape[0] == face.shape[0]):
        raise NsdpHipError(f"transfer_vertex_labels: vert_labels [B, V], faces [B, F, 3], face [B, n], bary [B, n, 3] (or all without "
                           f"B), got {tuple(vert_labels.shape)}, {tuple(faces.shape)}, {tuple(face.shape)}, {tuple(bary.shape)}")
    F, V = int(faces.shape[1]), int(vert_labels.shape[1])
    found = face >= 0
    rows = face.long().clamp(0, max(F - 1, 0))
    corner = torch.argmax(bary, dim=-1, keepdim=True)      # (the first of several equal maxima, as torch documents)
    tri = torch.gather(faces.long(), 1, rows.unsqueeze(-1).expand(-1, -1, 3)) if F else rows.new_zeros(rows.shape + (3,))
    vert = torch.gather(tri, 2, corner).squeeze(-1).clamp(0, max(V - 1, 0))
    out = torch.gather(vert_labels, 1, vert) if V else vert_labels.new_zeros(vert.shape)
    out = torch.where(found, out, torch.zeros_like(out)).to(torch.uint8)
    return out[0] if single else out


def point_to_surface_loss(points, verts, faces):
    """The fitting and evaluation recipe: the mean squared distance from ``points`` to the surface, ``(loss, per_shape [B])``.
    The search runs without autograd; then ``|p - ((b0 v0 + b1 v1) + b2 v2)|^2`` is recomputed in torch with ``(face, bary)``
    held constant, so autograd reaches ``points`` and ``verts`` -- at the minimiser the derivative through ``bary`` vanishes (an
    interior or edge optimum) or is blocked by its constraint (a clamped one), so this is the gradient of the exact distance
    wherever the closest face is unique.  Rectangular ``[B, n, 3]`` / ``[B, V, 3]`` / ``[B, F, 3]``.  ``per_shape`` are the
    per-shape means, ``loss`` their mean.  Not wired into ``training:`` -- the train step's ``data_dict`` carries no faces."""
    if isinstance(points, RaggedPoints):
        raise NsdpHipError("point_to_surface_loss: ragged inputs: the recipe is rectangular, [B, n, 3] / [B, V, 3] / [B, F, 3]")
    _, face, bary = closest_on_mesh(points, verts, faces, return_bary=True)
    B, F = int(verts.shape[0]), int(faces.shape[1])
    rows = face.long().clamp(0, max(F - 1, 0))
    tri = torch.gather(faces.long(), 1, rows.unsqueeze(-1).expand(-1, -1, 3))                       # [B, n, 3] vertex indices
    corners = [torch.gather(verts, 1, tri[:, :, k:k + 1].expand(-1, -1, 3)) for k in range(3)]
    c = (bary[:, :, 0:1] * corners[0] + bary[:, :, 1:2] * corners[1]) + bary[:, :, 2:3] * corners[2]
    d = points - c
    per_shape = ((d[:, :, 0] * d[:, :, 0] + d[:, :, 1] * d[:, :, 1]) + d[:, :, 2] * d[:, :, 2]).mean(dim=1)
    return per_shape.mean(), per_shape
