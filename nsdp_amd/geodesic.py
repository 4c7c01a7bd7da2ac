"""Geodesic distances over the edges of predicted meshes on the device (include/nsdp_geodesic.h, csrc/geodesic.hip): how far a
vertex is from a set of seed vertices ALONG the surface, and what is built on that:

    plan = GeodesicPlan(faces, verts)                         # once per topology: ONE validating host read, the Morton order
    dist = geodesic_distances(verts, plan, seeds)             # the edge table once, then rounds of the relaxation
    mask = geodesic_ball(verts, plan, seeds, radius)          # uint8: dist <= radius -- a brush
    nbr, length = edge_lengths(verts, plan)                   # the table itself (in the plan's numbering: plan.order)

The rule is the header's: the distance of a vertex is the minimum over edge paths from a seed of the left-to-right fp32 sum of
the start value and the edge lengths -- the unique fixed point of the relaxation, so its bits depend neither on the order of
relaxation nor on the numbering of the vertices nor on ``rounds_per_call``; tests/geodesic_ref.py reproduces every bit with a
heap Dijkstra.  The kernel relaxes a block of ``BLOCK`` consecutive vertex rows to convergence per launch, so the number of
launches is about the number of blocks a shortest path crosses: the plan puts the vertices in Morton order of the given pose
(``reorder=False`` keeps the caller's order; the same bits) and answers in the caller's numbering.

The layouts are ``vertex_normals``' three (nsdp_amd/mesh_normals.py): faces ``[F, 3]`` with vertices ``[..., V, 3]``; faces
``[B, F, 3]`` with ``[..., B, V, 3]``; a ``RaggedPoints`` of faces with a ``RaggedPoints`` of vertices.

``NSDP_GEODESIC_ROUNDS`` (1 .. 1024, default ``DEFAULT_ROUNDS``): the rounds one call of the entry runs before the host reads
the four bytes of its counter; docs/KNOBS.md.  There is no CPU path and no fallback.
"""
from __future__ import annotations

import ctypes
import os

import torch

from ._lib import NsdpHipError, check, fptr, iptr, lib, on_device, optptr, stream_ptr
from .mesh_normals import MeshTopology, mesh_corner_lists
from .ragged import RaggedPoints, shape_ids
from .surface_distance import _morton_order

_ci = ctypes.c_int
BLOCK = 256                     # NSDP_GEODESIC_BLOCK: the vertex rows one workgroup relaxes to convergence (1024 measured: 2.2x slower)
NO_LOCAL = 1                    # NSDP_GEODESIC_NO_LOCAL: one relaxation per round
MAX_ROUNDS = 1024               # rounds of one call
DEFAULT_ROUNDS = 8              # (profiles/geodesic.txt: 4.20 ms at 1, 3.30 at 8, flat beyond, on 99 683 vertices)


class GeodesicError(NsdpHipError):
    pass


def _rounds_default():
    """``NSDP_GEODESIC_ROUNDS``: the rounds per call of the entry, 1 .. 1024; unset: ``DEFAULT_ROUNDS``."""
    v = os.environ.get("NSDP_GEODESIC_ROUNDS")
    if v is None:
        return DEFAULT_ROUNDS
    try:
        n = int(v)
    except ValueError:
        n = 0
    if not 1 <= n <= MAX_ROUNDS:
        raise GeodesicError(f"NSDP_GEODESIC_ROUNDS={v!r}: an integer in 1 .. {MAX_ROUNDS} (rounds per call; unset: {DEFAULT_ROUNDS})")
    return n


def mesh_edge_lengths(verts, faces, face_offsets, vert_offsets, list_offsets, list_entries, want_nbr=True):
    """nsdp_mesh_edge_lengths: verts (P, vcap, 3) fp32 -> (nbr (6 fcap) int32 or None, len (P, 6 fcap) fp32)."""
    if not isinstance(verts, torch.Tensor) or not verts.is_cuda:
        raise GeodesicError("verts must be a GPU tensor (CPU not supported, no fallback)")
    if verts.dim() != 3 or verts.shape[2] != 3:
        raise GeodesicError(f"verts must be (P, vcap, 3), got {tuple(verts.shape)}")
    P, vcap, fcap, B, dev = int(verts.shape[0]), int(verts.shape[1]), int(faces.shape[0]), int(face_offsets.numel()) - 1, verts.device
    if list_offsets.numel() != vcap + 1 or list_entries.numel() != 3 * fcap:
        raise GeodesicError(f"corner lists of {list_offsets.numel() - 1} rows / {list_entries.numel()} corners against "
                            f"{vcap} vertex rows / {3 * fcap} corners")
    nbr = torch.empty((6 * fcap,), dtype=torch.int32, device=dev) if want_nbr else None
    length = torch.empty((P, 6 * fcap), dtype=torch.float32, device=dev)
    with on_device(verts):
        check(lib().nsdp_mesh_edge_lengths(fptr(verts, "verts"), _ci(P), iptr(faces, "faces"), iptr(face_offsets, "face_offsets"),
                                           iptr(vert_offsets, "vert_offsets"), _ci(B), _ci(vcap), _ci(fcap),
                                           iptr(list_offsets, "list_offsets"), iptr(list_entries, "list_entries"), optptr(nbr),
                                           fptr(length), stream_ptr()), "nsdp_mesh_edge_lengths")
    return nbr, length


def mesh_geodesic_relax(list_offsets, nbr, length, vert_offsets, dist, changed, limit=float("inf"), rounds=1, flags=0):
    """nsdp_mesh_geodesic_relax on dist (P, vcap) fp32 in place: ``rounds`` rounds; ``changed`` (1,) int32 gets the number of
    vertices the last of them lowered."""
    if not isinstance(dist, torch.Tensor) or not dist.is_cuda:
        raise GeodesicError("dist must be a GPU tensor (CPU not supported, no fallback)")
    if dist.dim() != 2 or length.dim() != 2 or length.shape[0] != dist.shape[0] or nbr.numel() != length.shape[1] or nbr.numel() % 6:
        raise GeodesicError(f"dist (P, vcap) with len (P, 6 fcap) and nbr (6 fcap), got {tuple(dist.shape)}, {tuple(length.shape)}, "
                            f"{tuple(nbr.shape)}")
    P, vcap, fcap, B = int(dist.shape[0]), int(dist.shape[1]), int(nbr.numel()) // 6, int(vert_offsets.numel()) - 1
    if list_offsets.numel() != vcap + 1:
        raise GeodesicError(f"list offsets of {list_offsets.numel() - 1} rows against {vcap} vertex rows")
    with on_device(dist):
        check(lib().nsdp_mesh_geodesic_relax(iptr(list_offsets, "list_offsets"), iptr(nbr, "nbr"), fptr(length, "len"),
                                             iptr(vert_offsets, "vert_offsets"), _ci(B), _ci(vcap), _ci(fcap), _ci(P),
                                             ctypes.c_float(limit), _ci(rounds), _ci(flags), fptr(dist, "dist"), iptr(changed, "changed"),
                                             stream_ptr()), "nsdp_mesh_geodesic_relax")
    return dist


class GeodesicPlan:
    """What ``geodesic_distances`` needs beside the positions, built once per topology: the validated faces (the ONE validating
    host read is ``MeshTopology``'s, which also brings the largest vertex count, the bound of the iteration; pass ``topology=``
    to share one that exists), the vertices put in Morton order of the given pose inside every mesh's own range
    (``surface_distance._morton_order``) so that a block of consecutive rows is a compact patch, the faces renumbered to it,
    their corner lists (``mesh_corner_lists``) and, at the first use, the neighbour table.  ``order[k]`` is the caller's row of
    the plan's row k, ``rank`` its inverse; answers come back in the caller's numbering.  ``reorder=False`` keeps the caller's
    order: the same bits, more rounds."""

    def __init__(self, faces, verts, topology: MeshTopology | None = None, validate: bool = True, reorder: bool = True):
        if topology is None:
            try:
                topology = MeshTopology(faces, verts, validate=validate)
            except GeodesicError:
                raise
            except NsdpHipError as e:
                raise GeodesicError(str(e).replace("MeshTopology", "GeodesicPlan")) from None
        elif not isinstance(topology, MeshTopology):
            raise GeodesicError("GeodesicPlan: topology must be a MeshTopology")
        self.topology, self.device = topology, topology.device
        vcap, fcap, B = topology.vcap, topology.fcap, topology.shapes
        has_positions = isinstance(verts, RaggedPoints) or (isinstance(verts, torch.Tensor) and verts.is_floating_point())
        self.order = self.rank = None
        self.faces, self.list_offsets, self.list_entries = topology.faces, topology.list_offsets, topology.list_entries
        with torch.no_grad():
            if reorder and has_positions:
                poses, _ = topology.poses(verts)
                self.order = _morton_order(poses[0], topology.vert_offsets)
                self.rank = torch.empty_like(self.order)
                self.rank[self.order] = torch.arange(vcap, device=self.device)
                owner = shape_ids(topology.face_offsets, fcap).clamp(max=B - 1)
                first = topology.vert_offsets.long().clamp(0, vcap)[owner].unsqueeze(1)
                rows = (topology.faces.long() + first).clamp(0, vcap - 1)
                self.faces = (self.rank[rows] - first).to(torch.int32).contiguous()      # (a Morton sort stays inside a mesh's range)
                self.list_offsets, self.list_entries = mesh_corner_lists(self.faces, topology.face_offsets, topology.vert_offsets, vcap)
            if topology.kind == "ragged":
                counts = topology._vert_layout.counts      # (the host's copy where the set has one, one read otherwise)
                self.max_vertices = max(counts, default=0)
            else:
                self.max_vertices = vcap // B
        self.reordered = self.order is not None
        self.nbr = None

    def to_plan(self, t):
        """(P, vcap, ...) in the caller's rows -> the plan's rows."""
        return t if self.order is None else t[:, self.order].contiguous()

    def to_caller(self, t):
        return t if self.rank is None else t[:, self.rank].contiguous()

    def __repr__(self):
        return f"GeodesicPlan({self.topology!r}, reordered={self.reordered}, block={BLOCK})"


def _poses(verts, plan, what):
    if not isinstance(plan, GeodesicPlan):
        raise GeodesicError(f"{what}: plan must be a GeodesicPlan (build it once from the faces)")
    try:
        return plan.topology.poses(verts)
    except NsdpHipError as e:
        raise GeodesicError(str(e).replace("vertex_normals", what)) from None


def edge_lengths(verts, plan: GeodesicPlan):
    """The edge table of ``verts`` (nsdp_mesh_edge_lengths): ``(nbr [6 F'] int32, length [P, 6 F'] fp32)`` in the PLAN's rows
    (``plan.order``, ``plan.list_offsets``): entries ``2 list_offsets[r] .. 2 list_offsets[r + 1]`` are the edges of plan row
    r, once per face that has them -- for stretch statistics against another pose, position by position.  One launch."""
    poses, _ = _poses(verts, plan, "edge_lengths")
    topo = plan.topology
    with torch.no_grad():
        nbr, length = mesh_edge_lengths(plan.to_plan(poses), plan.faces, topo.face_offsets, topo.vert_offsets, plan.list_offsets,
                                        plan.list_entries, want_nbr=plan.nbr is None)
    if plan.nbr is None:
        plan.nbr = nbr
    return plan.nbr, length


def _start(plan, P, lead, seeds, seed_dist, ragged):
    """The start array (P, vcap) in the caller's rows: ``seed_dist`` or +inf, 0 at the seeds."""
    topo, dev = plan.topology, plan.device
    vcap, B = topo.vcap, topo.shapes
    if seeds is None and seed_dist is None:
        raise GeodesicError("geodesic_distances: no seeds (seeds: vertex indices per shape; seed_dist: a full start array)")
    if seed_dist is not None:
        t = seed_dist.packed if isinstance(seed_dist, RaggedPoints) else seed_dist
        if not torch.is_tensor(t) or not t.is_cuda or t.dtype != torch.float32 or t.numel() != P * vcap:
            raise GeodesicError(f"geodesic_distances: seed_dist must be a float32 GPU tensor over the vertices ({P * vcap} values)")
        start = torch.empty((P * vcap + 1,), dtype=torch.float32, device=dev)
        start[:P * vcap] = t.reshape(-1)
    else:
        start = torch.full((P * vcap + 1,), float("inf"), dtype=torch.float32, device=dev)
    if seeds is not None:
        if not torch.is_tensor(seeds) or not seeds.is_cuda or seeds.dtype not in (torch.int32, torch.int64):
            raise GeodesicError("geodesic_distances: seeds must be an int32 / int64 GPU tensor of local vertex indices (-1: none)")
        s = seeds.long()
        if topo.kind == "shared":
            s = s.reshape(1, 1, -1) if s.dim() <= 1 else s.reshape(-1, 1, s.shape[-1])
        else:
            if s.dim() < 2 or s.shape[-2] != B:
                raise GeodesicError(f"geodesic_distances: seeds {tuple(seeds.shape)} against {B} shapes: [{B}, s] (-1: none)")
            s = s.reshape(-1, B, s.shape[-1])
        if s.shape[0] not in (1, P):
            raise GeodesicError(f"geodesic_distances: seeds with the leading shape {tuple(seeds.shape[:-1])} against {P} pose(s)")
        s = s.expand(P, -1, -1)
        first = topo.vert_offsets.long().clamp(0, vcap)
        count = (first[1:] - first[:-1]).clamp(min=0).view(1, B, 1)
        ok = (s >= 0) & (s < count)
        row = torch.arange(P, device=dev).view(P, 1, 1) * vcap + first[:-1].view(1, B, 1) + s
        start[torch.where(ok, row, torch.full_like(row, P * vcap)).reshape(-1)] = 0.0      # (an index outside its shape: the spare slot)
    return start[:P * vcap].view(P, vcap)


def geodesic_distances(verts, plan: GeodesicPlan, seeds=None, seed_dist=None, limit: float = float("inf"), rounds_per_call=None,
                       return_stats: bool = False, no_local: bool = False):
    """The geodesic distance of every vertex over the mesh's edges, in the verts' shape without the trailing 3 (a
    ``RaggedPoints`` of one column for packed vertices); +inf where no path arrives or the distance exceeds ``limit``.

    ``seeds``: local vertex indices per shape at distance 0 -- ``[s]`` (or ``[..., s]`` per pose) with shared faces,
    ``[B, s]`` (``[..., B, s]``) with faces of their own or packed; -1 or an index outside its shape: none.  ``seed_dist``: a
    full start array in the result's shape instead or as well (any non-negative value is a start value, everything else +inf).
    The edge-length call runs once; then the relax call runs ``rounds_per_call`` rounds at a time (``NSDP_GEODESIC_ROUNDS``)
    and its counter, four bytes, is read back once per call until it is 0.  The rule cannot lower anything beyond as many
    rounds as the largest mesh has vertices: past that (+ 1) the loop raises instead of launching on.  ``return_stats``:
    ``(dist, {"rounds", "calls"})``.  ``no_local``: one relaxation per round, the plain form (the same bytes)."""
    poses, lead = _poses(verts, plan, "geodesic_distances")
    topo = plan.topology
    P, vcap = int(poses.shape[0]), topo.vcap
    limit = float(limit)
    if not limit >= 0.0:
        raise GeodesicError(f"geodesic_distances: limit={limit} is NaN or negative")
    per_call = _rounds_default() if rounds_per_call is None else int(rounds_per_call)
    if not 1 <= per_call <= MAX_ROUNDS:
        raise GeodesicError(f"geodesic_distances: rounds_per_call={rounds_per_call} outside 1 .. {MAX_ROUNDS}")
    ragged = verts if isinstance(verts, RaggedPoints) else None
    with torch.no_grad():
        start = _start(plan, P, lead, seeds, seed_dist, ragged)
        nbr, length = edge_lengths(verts, plan)
        dist = plan.to_plan(start)      # (a tensor of this call's own: the entry relaxes it in place)
        changed = torch.empty((1,), dtype=torch.int32, device=plan.device)
        bound, rounds, calls = plan.max_vertices + 1, 0, 0
        while True:
            if rounds >= bound:
                raise GeodesicError(f"geodesic_distances: {rounds} rounds and vertices still fall -- a mesh of {plan.max_vertices} "
                                    "vertices cannot need them (a changed table under a running call?)")
            n = min(per_call, bound - rounds)
            mesh_geodesic_relax(plan.list_offsets, nbr, length, topo.vert_offsets, dist, changed, limit, n, NO_LOCAL if no_local else 0)
            rounds, calls = rounds + n, calls + 1
            if int(changed.item()) == 0:
                break
        out = plan.to_caller(dist)
    if ragged is not None:
        out = ragged.like(out.reshape(vcap, 1))
    else:
        out = out.reshape(tuple(verts.shape[:-1]))
    return (out, {"rounds": rounds, "calls": calls}) if return_stats else out


def geodesic_ball(verts, plan: GeodesicPlan, seeds, radius, **kw):
    """uint8 in ``geodesic_distances``' shape: 1 where the geodesic distance from ``seeds`` is <= ``radius`` (closed at the
    radius, as the rule's limit is)."""
    dist = geodesic_distances(verts, plan, seeds, limit=radius, **kw)
    if isinstance(dist, RaggedPoints):
        return dist.like((dist.packed <= float(radius)).to(torch.uint8))
    return (dist <= float(radius)).to(torch.uint8)
