"""Self-intersections of predicted meshes on the device (include/nsdp_selfintersect.h, csrc/self_intersect.hip).

    plan = SelfIntersectionPlan(faces, verts)           # once per topology: ONE host read (validation), the Morton order
    res = self_intersections(verts, plan)               # capturable, no host read: res.pairs, res.hits, res.faces_hit, ...

Two faces of one mesh intersect when they share no corner (as coordinates), their boxes overlap and an edge of one pierces
the other -- strict signs of five fp32 determinants with one rounding per operation; the header is the definition and
tests/self_intersect_ref.py reproduces every byte in numpy.  Faces that share a corner can still fold through each other: the
rule does not report that.  The layouts are ``vertex_normals``' three (nsdp_amd/mesh_normals.py): shared faces ``[F, 3]`` with
``[..., V, 3]``, faces of their own ``[B, F, 3]`` with ``[..., B, V, 3]``, and a ``RaggedPoints`` of faces with a
``RaggedPoints`` of vertices (or poses ``[..., capacity, 3]``).

The work guard.  A face with more than ``budget`` candidate partners (faces that pass adjacency and the box test) is SKIPPED:
``hits = -1``; a pair counts only where both faces are within the budget, so the answer stays symmetric and a function of the
input.  ``DEFAULT_BUDGET`` comes from a measurement (profiles/self_intersect.txt); ``budget=0`` turns the guard off.

``NSDP_SELFINT_CULL=0`` visits every block of 64 faces instead of those whose boxes overlap (the same bytes, the yardstick of
the culled form); docs/KNOBS.md.  There is no CPU path and no fallback.
"""
from __future__ import annotations

import ctypes
import os
from dataclasses import dataclass

import torch

from ._lib import NsdpHipError, check, fptr, iptr, lib, on_device, optptr, stream_ptr
from .mesh_normals import MeshTopology
from .ragged import RaggedPoints, shape_ids
from .surface_distance import _morton_order

_ci = ctypes.c_int
NO_CULL = 1                     # flag of nsdp_mesh_self_intersections: visit every block
MAX_POSES = 65535
# The largest power of two b for which 2^20 faces with b candidates each -- the most narrow tests a guarded call at the entry's
# face limit can run -- stay under about a second at the measured rate, 3.9e10 narrow tests a second on an all-candidate input
# (tools/bench_selfintersect.py, profiles/self_intersect.txt): 2^20 * 32768 / 3.9e10 = 0.88 s.
DEFAULT_BUDGET = 32768


class SelfIntersectError(NsdpHipError):
    pass


def _cull_default():
    """``NSDP_SELFINT_CULL``: 0 -> the unculled form, 1 or unset -> culling by blocks of faces."""
    v = os.environ.get("NSDP_SELFINT_CULL")
    if v is None or v == "1":
        return True
    if v == "0":
        return False
    raise SelfIntersectError(f"NSDP_SELFINT_CULL={v!r}: 0 (every block is visited) or 1 (culling by blocks of faces, the default)")


def mesh_self_intersections(verts, vert_offsets, faces, face_offsets, face_ids=None, budget: int = 0, cull: bool = True):
    """One nsdp_mesh_self_intersections call: verts (P, vcap, 3) fp32, faces (fcap, 3) int32 (local indices), offsets (B + 1)
    int32, face_ids (fcap) int32 or None -> (cand, hits, partner (P, fcap) int32, pairs (P, B) int64, skipped (P, B) int32);
    partner is a PACKED reported face row."""
    if not isinstance(verts, torch.Tensor) or not verts.is_cuda:
        raise SelfIntersectError("verts must be a GPU tensor (CPU not supported, no fallback)")
    if verts.dim() != 3 or verts.shape[2] != 3 or faces.dim() != 2 or faces.shape[1] != 3:
        raise SelfIntersectError(f"verts must be (P, vcap, 3) and faces (fcap, 3), got {tuple(verts.shape)} and {tuple(faces.shape)}")
    P, vcap, fcap, B, dev = int(verts.shape[0]), int(verts.shape[1]), int(faces.shape[0]), int(face_offsets.numel()) - 1, verts.device
    if vert_offsets.numel() != B + 1:
        raise SelfIntersectError(f"{B} shapes of faces against {vert_offsets.numel() - 1} of vertices")
    if face_ids is not None and face_ids.numel() != fcap:
        raise SelfIntersectError(f"face_ids holds {face_ids.numel()} rows against {fcap} face rows")
    if int(budget) < 0:
        raise SelfIntersectError(f"budget={budget} is negative (0: no guard)")
    for name, t in (("faces", faces), ("face_offsets", face_offsets), ("vert_offsets", vert_offsets), ("face_ids", face_ids)):
        if t is not None and t.device != dev:
            raise SelfIntersectError(f"{name} lives on {t.device}, verts on {dev}: one launch reads them all")
    L = lib()
    L.nsdp_mesh_self_intersections_workspace_bytes.restype = ctypes.c_size_t
    need = int(L.nsdp_mesh_self_intersections_workspace_bytes(_ci(P), _ci(B), _ci(fcap)))
    if need <= 0:
        raise SelfIntersectError(f"nsdp_mesh_self_intersections_workspace_bytes refused P={P}, B={B}, fcap={fcap}")
    with on_device(verts):
        ws = torch.empty(need // 4, dtype=torch.int32, device=dev)
        cand = torch.empty((P, fcap), dtype=torch.int32, device=dev)
        hits = torch.empty((P, fcap), dtype=torch.int32, device=dev)
        partner = torch.empty((P, fcap), dtype=torch.int32, device=dev)
        pairs = torch.empty((P, B), dtype=torch.int64, device=dev)
        skipped = torch.empty((P, B), dtype=torch.int32, device=dev)
        check(L.nsdp_mesh_self_intersections(fptr(verts, "verts"), _ci(P), iptr(vert_offsets, "vert_offsets"), iptr(faces, "faces"),
                                             iptr(face_offsets, "face_offsets"), optptr(face_ids), _ci(B), _ci(vcap), _ci(fcap),
                                             _ci(int(budget)), _ci(0 if cull else NO_CULL), ctypes.c_void_p(ws.data_ptr()), iptr(cand),
                                             iptr(hits), iptr(partner), ctypes.c_void_p(pairs.data_ptr()), iptr(skipped), stream_ptr()),
              "nsdp_mesh_self_intersections")
        del ws      # (stream-ordered: the allocator hands the block on behind the launches; a graph's pool keeps it)
    return cand, hits, partner, pairs, skipped


class SelfIntersectionPlan:
    """What ``self_intersections`` needs beside the positions, built once per topology: the validated faces (the ONE host read,
    ``MeshTopology``'s; pass ``topology=`` to share one that exists) and, where ``verts`` holds positions and not only a layout,
    the faces reordered along a Morton curve of their centroids on that pose (``surface_distance._morton_order``: a stable sort
    inside every mesh's own range) with ``face_ids`` carrying the caller's rows -- blocks of 64 consecutive faces are then
    compact and the culling by block boxes has something to skip.  ``reorder=False`` keeps the given order."""

    def __init__(self, faces, verts, topology: MeshTopology | None = None, validate: bool = True, reorder: bool = True):
        if topology is None:
            try:
                topology = MeshTopology(faces, verts, validate=validate)
            except SelfIntersectError:
                raise
            except NsdpHipError as e:
                raise SelfIntersectError(str(e).replace("MeshTopology", "SelfIntersectionPlan")) from None
        elif not isinstance(topology, MeshTopology):
            raise SelfIntersectError("SelfIntersectionPlan: topology must be a MeshTopology")
        self.topology, self.device = topology, topology.device
        self.faces, self.face_ids = topology.faces, None
        has_positions = isinstance(verts, RaggedPoints) or (isinstance(verts, torch.Tensor) and verts.is_floating_point())
        if reorder and has_positions:
            poses, _ = topology.poses(verts)
            with torch.no_grad():
                v, f, B = poses[0], topology.faces, topology.shapes
                owner = shape_ids(topology.face_offsets, topology.fcap).clamp(max=B - 1)
                rows = (f.long() + topology.vert_offsets.long()[owner].unsqueeze(1)).clamp(0, topology.vcap - 1)
                centroid = (v[rows[:, 0]] + v[rows[:, 1]]) + v[rows[:, 2]]
                perm = _morton_order(centroid, topology.face_offsets)
                self.faces = f[perm].contiguous()
                self.face_ids = perm.to(torch.int32).contiguous()
        # the first packed face row of every mesh, per face row: what turns a packed partner row into a local one
        first = topology.face_offsets[:-1].clamp(0, topology.fcap)
        self._first = first[shape_ids(topology.face_offsets, topology.fcap).clamp(max=topology.shapes - 1)].to(torch.int32)
        self._ids = shape_ids(topology.face_offsets, topology.fcap)

    def __repr__(self):
        return f"SelfIntersectionPlan({self.topology!r}, reordered={self.face_ids is not None})"


@dataclass
class SelfIntersections:
    """Per face (the faces' layout without the trailing 3, poses in front): ``cand`` candidate partners, ``hits`` faces it
    intersects (-1: skipped by the guard), ``partner`` the smallest such face, local to its mesh (-1: none).  Per mesh (poses
    in front; a shared face table has one mesh): ``pairs`` int64 unordered intersecting pairs, ``skipped`` faces over the
    budget, ``faces_hit`` faces with at least one hit."""
    hits: torch.Tensor
    partner: torch.Tensor
    cand: torch.Tensor
    pairs: torch.Tensor
    skipped: torch.Tensor
    faces_hit: torch.Tensor


def self_intersections(verts, plan: SelfIntersectionPlan, budget=None, cull=None) -> SelfIntersections:
    """The self-intersections of ``verts`` (the plan's layout; every leading index a pose).  ``budget`` None: DEFAULT_BUDGET,
    0: no guard.  ``cull`` None: ``NSDP_SELFINT_CULL``.  No synchronisation and no allocation whose size depends on device
    data: capturable."""
    if not isinstance(plan, SelfIntersectionPlan):
        raise SelfIntersectError("self_intersections: plan must be a SelfIntersectionPlan (build it once from the faces)")
    topo = plan.topology
    try:
        poses, lead = topo.poses(verts)
    except NsdpHipError as e:
        raise SelfIntersectError(str(e).replace("vertex_normals", "self_intersections")) from None
    P = int(poses.shape[0])
    if not 1 <= P <= MAX_POSES:
        raise SelfIntersectError(f"self_intersections: {P} poses outside [1, {MAX_POSES}]")
    budget = DEFAULT_BUDGET if budget is None else int(budget)
    cull = _cull_default() if cull is None else bool(cull)
    with torch.no_grad():
        cand, hits, partner, pairs, skipped = mesh_self_intersections(poses, topo.vert_offsets, plan.faces, topo.face_offsets,
                                                                      plan.face_ids, budget, cull)
        partner = torch.where(partner >= 0, partner - plan._first, partner)
        B = topo.shapes
        if topo.kind == "ragged":
            faces_hit = torch.zeros((P, B + 1), dtype=torch.int32, device=poses.device)
            faces_hit.index_add_(1, plan._ids, (hits > 0).to(torch.int32))      # (integer atomics: order-independent)
            faces_hit = faces_hit[:, :B]
        else:
            faces_hit = (hits > 0).reshape(P, B, -1).sum(dim=2, dtype=torch.int32)
    per_face = topo.face_shape(lead)[:-1]
    per_mesh = lead if topo.kind == "shared" else lead + (B,)
    return SelfIntersections(hits=hits.reshape(per_face), partner=partner.reshape(per_face), cand=cand.reshape(per_face),
                             pairs=pairs.reshape(per_mesh), skipped=skipped.reshape(per_mesh), faces_hit=faces_hit.reshape(per_mesh))
