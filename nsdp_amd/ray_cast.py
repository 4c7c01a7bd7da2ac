"""Rays against predicted meshes on the device (include/nsdp_raycast.h, csrc/ray_cast.hip): where a ray meets a mesh and how
often it crosses it, and what is built on that:

    plan = RayCastPlan(faces, verts)                     # once per topology: ONE validating host read, the Morton order, open_edges
    hits = cast_rays(origins, directions, verts, plan)   # capturable, no host read: hits.t, .face, .bary, .crossings, .hit
    inside = contains(points, verts, plan)               # the parity of the crossings along one direction
    iou, a, b, both = volume_iou(verts_a, verts_b, plan, 20000)      # sampled volume IoU of two poses of the topology

The rule is the header's: an fp32 shear into the ray's frame, EXACT signs of the three edge functions for a symbolically
displaced ray (no ray passes through an edge or a vertex, none is counted twice or dropped), the depth in fp64;
tests/ray_cast_ref.py reproduces every byte in numpy.  On a closed mesh the number of covered faces is even for every ray.

The layouts are ``vertex_normals``' three (nsdp_amd/mesh_normals.py): shared faces ``[F, 3]`` with vertices ``[..., V, 3]`` and
rays ``[..., n, 3]``; faces of their own ``[B, F, 3]`` with ``[..., B, V, 3]`` and rays ``[..., B, n, 3]``; a ``RaggedPoints``
of faces with ``RaggedPoints`` of vertices and of rays over one batch.  The rays of a shape meet the mesh of that shape.

``NSDP_RAYCAST_CULL`` (``1`` culling by blocks of 64 faces, ``0`` the plain scan -- the same bytes, unset: by size, from
``AUTO_MIN_TESTS`` ray x face tests on); docs/KNOBS.md.  There is no CPU path and no fallback.
"""
from __future__ import annotations

import ctypes
import os
from dataclasses import dataclass

import torch

from ._lib import NsdpHipError, check, fptr, iptr, lib, on_device, optptr, stream_ptr
from .mesh_normals import MeshTopology
from .ragged import RaggedPoints, offsets_of, shape_ids
from .surface_distance import _morton_order

_ci = ctypes.c_int
NO_CULL = 1                     # flag of nsdp_mesh_ray_cast: visit every block
MAX_BATCH = 65535
MAX_ROWS = 1 << 20              # rays, vertices or faces of one shape
# The default dispatch, from the sizes the host knows (profiles/ray_cast.txt, docs/EXPERIMENTS.md): with at least this many
# exact tests in the plain scan -- ray rows x face rows / shapes -- the call culls by blocks of faces; below it the plain scan
# is at least as fast (the boxes pass and the interval test per block cost more than the skipped blocks save).  Where a call
# culls by this rule it also reorders its rays (``_ray_order``): the vote on a block is per wave of 64 rays, so it needs rays
# that run close to each other in one wave.
AUTO_MIN_TESTS = 1 << 29


class RayCastError(NsdpHipError):
    pass


def _cull_default():
    """``NSDP_RAYCAST_CULL``: 1 -> True (cull whatever the size), 0 -> False (the plain scan), unset -> None (by size)."""
    v = os.environ.get("NSDP_RAYCAST_CULL")
    if v is None:
        return None
    if v in ("0", "1"):
        return v == "1"
    raise RayCastError(f"NSDP_RAYCAST_CULL={v!r}: 0 (the plain scan) or 1 (culling by blocks of faces); unset: by size")


def _large(B: int, qcap: int, fcap: int) -> bool:
    return qcap * fcap >= AUTO_MIN_TESTS * B


def _dispatch(B: int, qcap: int, fcap: int, cull, reorder):
    """(cull, reorder) of a call: ``NSDP_RAYCAST_CULL`` over the size rule; reordering wherever the call culls and is large."""
    if cull is None:
        cull = _cull_default()
    large = _large(B, qcap, fcap)
    cull = large if cull is None else bool(cull)
    return cull, (cull and large) if reorder is None else bool(reorder)


def mesh_ray_cast(origins, dirs, ray_offsets, verts, vert_offsets, faces, face_offsets, return_bary: bool = True,
                  count: bool = True, cull=None):
    """One nsdp_mesh_ray_cast call on packed contiguous GPU operands (faces int32, local indices) -> (t [qcap] fp32, face
    [qcap] int32 packed face rows, bary [qcap, 3] or None, count [qcap] int32 or None).  ``cull`` None: ``NSDP_RAYCAST_CULL``,
    else by size."""
    if not isinstance(origins, torch.Tensor) or not origins.is_cuda:
        raise RayCastError("origins must be a GPU tensor (CPU not supported, no fallback)")
    B, qcap, vcap, fcap = int(ray_offsets.numel()) - 1, int(origins.shape[0]), int(verts.shape[0]), int(faces.shape[0])
    if tuple(dirs.shape) != tuple(origins.shape) or origins.dim() != 2 or origins.shape[1] != 3:
        raise RayCastError(f"origins and dirs must both be (qcap, 3), got {tuple(origins.shape)} and {tuple(dirs.shape)}")
    if vert_offsets.numel() != B + 1 or face_offsets.numel() != B + 1:
        raise RayCastError(f"{B} shapes of rays against {vert_offsets.numel() - 1} of vertices and {face_offsets.numel() - 1} of faces")
    dev = origins.device
    for name, t in (("dirs", dirs), ("ray_offsets", ray_offsets), ("verts", verts), ("vert_offsets", vert_offsets), ("faces", faces),
                    ("face_offsets", face_offsets)):
        if t.device != dev:
            raise RayCastError(f"{name} lives on {t.device}, origins on {dev}: one launch reads them all")
    if cull is None:
        cull = _cull_default()
    cull = _large(B, qcap, fcap) if cull is None else bool(cull)
    L = lib()
    L.nsdp_mesh_ray_cast_workspace_bytes.restype = ctypes.c_size_t
    need = int(L.nsdp_mesh_ray_cast_workspace_bytes(_ci(B), _ci(qcap), _ci(fcap)))
    if need <= 0:
        raise RayCastError(f"limits: nsdp_mesh_ray_cast_workspace_bytes refused B={B}, qcap={qcap}, fcap={fcap} "
                           f"(1 .. {MAX_BATCH} shapes, 1 .. {MAX_ROWS} rows per shape)")
    with on_device(origins):
        ws = torch.empty(((need + 7) // 8,), dtype=torch.int64, device=dev)
        t = torch.empty((qcap,), dtype=torch.float32, device=dev)
        face = torch.empty((qcap,), dtype=torch.int32, device=dev)
        bary = torch.empty((qcap, 3), dtype=torch.float32, device=dev) if return_bary else None
        cnt = torch.empty((qcap,), dtype=torch.int32, device=dev) if count else None
        check(L.nsdp_mesh_ray_cast(fptr(origins, "origins"), fptr(dirs, "dirs"), iptr(ray_offsets, "ray_offsets"), fptr(verts, "verts"),
                                   iptr(vert_offsets, "vert_offsets"), iptr(faces, "faces"), iptr(face_offsets, "face_offsets"), _ci(B),
                                   _ci(qcap), _ci(vcap), _ci(fcap), _ci(0 if cull else NO_CULL), ctypes.c_void_p(ws.data_ptr()), fptr(t),
                                   iptr(face), optptr(bary), optptr(cnt), stream_ptr()), "nsdp_mesh_ray_cast")
        del ws      # (stream-ordered: the allocator hands the block on behind the launches; a graph's pool keeps it)
    return t, face, bary, cnt


def _open_edges(faces, ids, B):
    """[B] int64: per mesh the undirected edges not used by exactly two faces.  ``faces`` (fcap, 3) int32 local indices, ``ids``
    (fcap) the mesh of every face row (B: a padding row).  Every tensor has a size the host knows -- no masked selection, no
    ``unique`` -- so nothing is read back: the 3 fcap edges become the keys (mesh << 40 | smaller vertex << 20 | larger vertex),
    a sort puts equal edges side by side, and a run of equal keys is counted where it begins, minus the runs that are
    exactly two long."""
    f = faces.long().clamp(0, MAX_ROWS - 1)
    e = torch.cat([f[:, 0:2], f[:, 1:3], torch.stack([f[:, 2], f[:, 0]], dim=1)])      # (slices: an index list would be uploaded)
    key = (ids.repeat(3) << 40) | (e.amin(dim=1) << 20) | e.amax(dim=1)
    key = torch.sort(key).values
    n = int(key.numel())
    differs = key[1:] != key[:-1]
    true = torch.ones(1, dtype=torch.bool, device=key.device)
    start, end = torch.cat([true, differs]), torch.cat([differs, true])      # the first / the last key of its run
    pair = start & ~end & torch.cat([end[1:], ~true])                        # a run of exactly two: begins here, ends at the next key
    assert start.numel() == n and pair.numel() == n
    return torch.zeros(B + 1, dtype=torch.int64, device=key.device).index_add_(0, key >> 40, start.long() - pair.long())[:B]


def _ray_order(o, d, roff, v, voff):
    """A permutation of the packed rays that keeps every shape's rays in its own range and orders them along a Morton curve of
    the point where each ray passes closest to the centre of its mesh's vertices (``surface_distance._morton_order``: a stable
    sort) -- neighbours in it run close to each other near the mesh, whether they share an eye or a direction.  The order
    changes which rays share a wave and nothing else: every ray's result is a function of that ray alone."""
    M = int(roff.numel()) - 1
    ids = shape_ids(voff, int(v.shape[0]))
    sums = torch.zeros((M + 1, 3), dtype=torch.float32, device=v.device).index_add_(0, ids, v)
    rows = torch.zeros((M + 1,), dtype=torch.float32, device=v.device).index_add_(0, ids, torch.ones_like(v[:, 0]))
    centre = (sums / rows.clamp(min=1).unsqueeze(1))[shape_ids(roff, int(o.shape[0])).clamp(max=M - 1)]
    along = ((centre - o) * d).sum(dim=1) / (d * d).sum(dim=1).clamp_min(1e-30)
    return _morton_order(o + along.unsqueeze(1) * d, roff)


def _cast_reordered(o, d, roff, v, voff, faces, foff, return_bary, count, cull, reorder):
    """``mesh_ray_cast`` behind the ray reordering, its outputs back in the given order."""
    if not reorder:
        return mesh_ray_cast(o, d, roff, v, voff, faces, foff, return_bary, count, cull)
    perm = _ray_order(o, d, roff, v, voff)
    got = mesh_ray_cast(o[perm].contiguous(), d[perm].contiguous(), roff, v, voff, faces, foff, return_bary, count, cull)
    back = []
    for x in got:
        if x is not None:
            y = torch.empty_like(x)
            y[perm] = x
            x = y
        back.append(x)
    return tuple(back)


class RayCastPlan:
    """What ``cast_rays`` needs beside the positions, built once per topology: the validated faces (int64 converted, the ONE
    validating host read is ``MeshTopology``'s; pass ``topology=`` to share one that exists), the faces reordered along a Morton
    curve of their centroids on the given pose (``surface_distance._morton_order``: a stable sort inside every mesh's own range)
    so that blocks of 64 consecutive faces are compact -- results are reported in the caller's numbering -- and
    ``open_edges``: the number of undirected edges not used by exactly two faces (0: every mesh is closed, the condition under
    which ``contains`` is an inside test), counted once here on the device (``open_edges_per_mesh``, ``_open_edges``: tensors of
    host-known sizes only) and read back at its first use; the constructor itself makes no host read beyond
    ``MeshTopology``'s validation, none with ``validate=False``."""

    def __init__(self, faces, verts, topology: MeshTopology | None = None, validate: bool = True, reorder: bool = True):
        if topology is None:
            try:
                topology = MeshTopology(faces, verts, validate=validate)
            except RayCastError:
                raise
            except NsdpHipError as e:
                raise RayCastError(str(e).replace("MeshTopology", "RayCastPlan")) from None
        elif not isinstance(topology, MeshTopology):
            raise RayCastError("RayCastPlan: topology must be a MeshTopology")
        self.topology, self.device = topology, topology.device
        B, fcap = topology.shapes, topology.fcap
        self.faces, perm = topology.faces, None
        has_positions = isinstance(verts, RaggedPoints) or (isinstance(verts, torch.Tensor) and verts.is_floating_point())
        with torch.no_grad():
            ids = shape_ids(topology.face_offsets, fcap)
            owner = ids.clamp(max=B - 1)
            if reorder and has_positions:
                poses, _ = topology.poses(verts)
                v, f = poses[0], topology.faces
                rows = (f.long() + topology.vert_offsets.long()[owner].unsqueeze(1)).clamp(0, topology.vcap - 1)
                centroid = (v[rows[:, 0]] + v[rows[:, 1]]) + v[rows[:, 2]]
                perm = _morton_order(centroid, topology.face_offsets)
                self.faces = f[perm].contiguous()
            # the caller's LOCAL face number of every kernel row (a Morton sort stays inside a mesh's own range)
            first = topology.face_offsets[:-1].clamp(0, fcap).long()[owner]
            caller = perm if perm is not None else torch.arange(fcap, device=self.device)
            self._local = (caller - first).to(torch.int32).contiguous()
            self.open_edges_per_mesh = _open_edges(topology.faces, ids, B)
        self._open_edges = None
        self.reordered = perm is not None
        self._tiled, self._rect = {}, {}

    @property
    def open_edges(self) -> int:
        """Undirected edges not used by exactly two faces, over all meshes (``open_edges_per_mesh``: [shapes] int64 on the
        device); read back once, at the first use."""
        if self._open_edges is None:
            self._open_edges = int(self.open_edges_per_mesh.sum())
        return self._open_edges

    def tiled(self, P: int):
        """The faces of P poses of a rectangular topology as P * shapes meshes: (faces, face_offsets, vert_offsets), kept."""
        if P not in self._tiled:
            topo = self.topology
            M, F, V = P * topo.shapes, topo.fcap // topo.shapes, topo.vcap // topo.shapes
            self._tiled[P] = (self.faces.repeat(P, 1).contiguous(), self.rect_offsets(M, F), self.rect_offsets(M, V))
        return self._tiled[P]

    def rect_offsets(self, M: int, n: int):
        """The offsets of M shapes of n rows each, kept (built outside a capture: a replayed call makes no host copy)."""
        if (M, n) not in self._rect:
            self._rect[(M, n)] = offsets_of([n] * M, self.device)
        return self._rect[(M, n)]

    def __repr__(self):
        return f"RayCastPlan({self.topology!r}, reordered={self.reordered}, open_edges={self.open_edges})"


@dataclass
class RayHits:
    """Per ray, in the rays' layout without the trailing 3 (a ``RaggedPoints`` of one column for packed rays): ``t`` the
    parameter of the first hit (``o + t d``; FLT_MAX without one), ``face`` the hit face in the caller's numbering, local to its
    mesh (-1: none), ``bary`` the weights of its three corners (None without ``return_bary``), ``crossings`` the number of hit
    faces (None without ``count``), ``hit`` = ``face >= 0``."""
    t: object
    face: object
    bary: object
    crossings: object
    hit: object


def refusal(origins, directions, verts, plan):
    """Why ``cast_rays`` cannot take these operands (None: it can), each reason named."""
    if not isinstance(plan, RayCastPlan):
        return "plan must be a RayCastPlan (build it once from the faces)"
    topo = plan.topology
    rag = [isinstance(t, RaggedPoints) for t in (origins, directions)]
    if rag[0] != rag[1] or rag[0] != (topo.kind == "ragged"):
        return (f"mismatched layouts: origins is {'packed' if rag[0] else 'rectangular'}, directions is "
                f"{'packed' if rag[1] else 'rectangular'}, the plan's topology is {topo.kind}")
    o, d = (origins.packed, directions.packed) if rag[0] else (origins, directions)
    for name, t in (("origins", o), ("directions", d)):
        if not torch.is_tensor(t):
            return f"{name} must be a torch.Tensor or a RaggedPoints, got {type(t).__name__}"
        if t.dtype is not torch.float32:
            return f"dtype: {name} must be torch.float32, got {t.dtype}"
        if not t.is_cuda:
            return f"CPU tensors: {name} is on the CPU -- the cast has no CPU path and there is no fallback"
        if t.device != plan.device:
            return f"devices: the plan on {plan.device}, {name} on {t.device}"
    if tuple(o.shape) != tuple(d.shape):
        return f"shape: origins {tuple(o.shape)} against directions {tuple(d.shape)}"
    if rag[0]:
        if o.dim() != 2 or o.shape[1] != 3:
            return f"shape: packed rays must be [capacity, 3], got {tuple(o.shape)}"
        if origins.batch != topo.shapes or directions.batch != topo.shapes:
            return f"mismatched batches: rays of {origins.batch} shapes against meshes of {topo.shapes}"
        if o.shape[0] < 1:
            return f"limits: the rays have a capacity of 0 rows, the entry takes 1 .. {MAX_ROWS} per shape"
    else:
        k = 2 if topo.kind == "shared" else 3
        if o.dim() < k or o.shape[-1] != 3 or (topo.kind == "batched" and o.shape[-3] != topo.shapes):
            return (f"shape: rays {tuple(o.shape)} against a {topo.kind} topology: [..., n, 3] go with shared faces, "
                    f"[..., {topo.shapes}, n, 3] with faces of their own")
        if not 1 <= o.shape[-2] <= MAX_ROWS:
            return f"limits: {o.shape[-2]} rays per shape, the entry takes 1 .. {MAX_ROWS}"
    return None


def cast_rays(origins, directions, verts, plan: RayCastPlan, return_bary: bool = True, count: bool = True, cull=None,
              reorder=None) -> RayHits:
    """The first face of mesh ``b`` that every ray ``origins + t directions`` (t > 0) of shape ``b`` meets, and with ``count``
    the number of faces it crosses.  ``verts`` in the plan's layout (every leading index a pose; the rays carry the same leading
    indices); directions need not be normalised, a zero direction misses.  ``count=False`` is the first-hit mode: blocks behind
    the origin and beyond the best hit are skipped too.  Among faces whose ``t`` bits tie the first in the order the kernel saw
    wins (the plan's Morton order, or the given one with ``reorder=False``).  ``cull`` None: ``NSDP_RAYCAST_CULL``, and without
    it by size -- culling from ``AUTO_MIN_TESTS`` exact tests of the plain scan on; ``reorder`` None: the rays are reordered for
    the call (``_ray_order``: a sort in torch, the same bytes in the given order) wherever it culls and is that large.  No
    synchronisation and no allocation whose size depends on device data: capturable."""
    why = refusal(origins, directions, verts, plan)
    if why is not None:
        raise RayCastError("cast_rays: " + why)
    topo = plan.topology
    try:
        poses, lead = topo.poses(verts)
    except NsdpHipError as e:
        raise RayCastError(str(e).replace("vertex_normals", "cast_rays")) from None
    P = int(poses.shape[0])
    with torch.no_grad():
        if topo.kind == "ragged":
            if lead != ():
                raise RayCastError(f"cast_rays: packed rays go with ONE pose of the packed vertices, got the leading shape {lead}")
            o, d = origins.packed.detach().contiguous(), directions.packed.detach().contiguous()
            roff, M = origins.offsets, topo.shapes
            cull, reorder = _dispatch(M, int(o.shape[0]), topo.fcap, cull, reorder)
            t, face, bary, cnt = _cast_reordered(o, d, roff, poses[0].contiguous(), topo.vert_offsets, plan.faces, topo.face_offsets,
                                                 return_bary, count, cull, reorder)
        else:
            k = 2 if topo.kind == "shared" else 3
            if tuple(origins.shape[:-k]) != lead:
                raise RayCastError(f"cast_rays: shape: rays with the leading shape {tuple(origins.shape[:-k])} against vertices "
                                   f"with {lead}")
            n, M = int(origins.shape[-2]), P * topo.shapes
            if M > MAX_BATCH:
                raise RayCastError(f"cast_rays: limits: {M} meshes in one call, the entry takes 1 .. {MAX_BATCH}")
            faces, foff, voff = plan.tiled(P)
            o, d = origins.detach().reshape(M * n, 3).contiguous(), directions.detach().reshape(M * n, 3).contiguous()
            cull, reorder = _dispatch(M, M * n, int(faces.shape[0]), cull, reorder)
            t, face, bary, cnt = _cast_reordered(o, d, plan.rect_offsets(M, n), poses.reshape(-1, 3), voff, faces, foff,
                                                 return_bary, count, cull, reorder)
        # packed kernel rows -> the caller's local face numbers
        face = torch.where(face >= 0, plan._local[(face.long() % topo.fcap).clamp(min=0)], face)
    if topo.kind == "ragged":
        wrap = lambda x, c: origins.like(x.reshape(-1, c))
        return RayHits(t=wrap(t, 1), face=wrap(face, 1), bary=wrap(bary, 3) if return_bary else None,
                       crossings=wrap(cnt, 1) if count else None, hit=wrap(face >= 0, 1))
    shape = tuple(origins.shape[:-1])
    return RayHits(t=t.reshape(shape), face=face.reshape(shape), bary=bary.reshape(shape + (3,)) if return_bary else None,
                   crossings=cnt.reshape(shape) if count else None, hit=(face >= 0).reshape(shape))


def hit_vertices(hits: RayHits, plan: RayCastPlan):
    """Per ray the hit face's corner of the largest barycentric weight, the lowest corner on ties, as a vertex index local to
    its mesh (int32, -1 without a hit), in the layout of ``hits.face``; needs ``hits.bary``.  What a click turns into."""
    topo = plan.topology
    if hits.bary is None:
        raise RayCastError("hit_vertices: the hits carry no barycentric weights (cast_rays(..., return_bary=True))")
    rag = isinstance(hits.face, RaggedPoints)
    face, bary = (hits.face.packed[:, 0], hits.bary.packed) if rag else (hits.face, hits.bary)
    F = topo.fcap // topo.shapes
    if rag:
        owner = shape_ids(hits.face.offsets, hits.face.capacity).clamp(max=topo.shapes - 1)
        first = topo.face_offsets[:-1].long().clamp(0, topo.fcap)[owner]
    elif topo.kind == "batched":
        first = (torch.arange(topo.shapes, device=face.device) * F).unsqueeze(1)
    else:
        first = 0
    rows = (face.long().clamp(min=0) + first).clamp(max=topo.fcap - 1)
    tri = topo.faces[rows]                                                   # (the caller's face order: the topology's own table)
    corner = torch.argmax(bary, dim=-1, keepdim=True)                        # (the first of several equal maxima, as torch documents)
    vert = torch.where(face >= 0, torch.gather(tri, -1, corner).squeeze(-1), torch.full_like(face, -1))
    return hits.face.like(vert.unsqueeze(1)) if rag else vert


def contains(points, verts, plan: RayCastPlan, direction=(0.0, 0.0, 1.0), cull=None):
    """Is every point of shape ``b`` inside mesh ``b``: the parity of the crossings of the ray from the point along
    ``direction`` -> a bool tensor in the points' layout without the trailing 3 (a ``RaggedPoints`` for packed points).  An
    inside test only on closed meshes (``plan.open_edges == 0``); there the parity of the COVERED faces is exact for every
    ray, and what rounds is the depth of each crossing: a point within the rule's ``t`` envelope of the surface -- about
    6 * 2^-24 of the largest coordinate difference to the crossed face's corners -- is undecided by nature, it may come out on
    either side.  One direction; voting over several is not built."""
    pts = points.packed if isinstance(points, RaggedPoints) else points
    if not torch.is_tensor(pts):
        raise RayCastError(f"contains: points must be a torch.Tensor or a RaggedPoints, got {type(points).__name__}")
    if len(direction) != 3:
        raise RayCastError(f"contains: direction must hold three numbers, got {direction!r}")
    d = torch.empty_like(pts, memory_format=torch.contiguous_format)
    for k in range(3):
        d[..., k] = float(direction[k])                                  # (fills on the device: nothing is copied from the host)
    dirs = points.like(d) if isinstance(points, RaggedPoints) else d
    hits = cast_rays(points, dirs, verts, plan, return_bary=False, count=True, cull=cull)
    if isinstance(points, RaggedPoints):
        return points.like((hits.crossings.packed & 1) == 1)
    return (hits.crossings & 1) == 1


def iou_samples(verts_a, verts_b, plan: RayCastPlan, points: int, generator=None):
    """``points`` uniform samples per shape in the joint bounding box of the two poses, in the layout ``contains`` takes with
    either pose: ``lo + u * (hi - lo)``, ``u`` from ``torch.rand`` with ``generator`` (a generator of the plan's device)."""
    topo, N = plan.topology, int(points)
    if N < 1:
        raise RayCastError(f"volume_iou: points = {points} samples per shape, at least 1")
    try:
        pa, lead_a = topo.poses(verts_a)
        pb, lead_b = topo.poses(verts_b)
    except NsdpHipError as e:
        raise RayCastError(str(e).replace("vertex_normals", "volume_iou")) from None
    if lead_a != lead_b:
        raise RayCastError(f"volume_iou: shape: poses with the leading shapes {lead_a} and {lead_b}")
    with torch.no_grad():
        if topo.kind == "ragged":
            if lead_a != ():
                raise RayCastError(f"volume_iou: packed vertices are ONE pose each, got the leading shape {lead_a}")
            B = topo.shapes
            both = torch.cat([pa[0], pb[0]])
            where = shape_ids(topo.vert_offsets, topo.vcap).repeat(2).unsqueeze(1).expand(-1, 3)
            lo = torch.full((B + 1, 3), float("inf"), device=plan.device).scatter_reduce(0, where, both, "amin")[:B]
            hi = torch.full((B + 1, 3), float("-inf"), device=plan.device).scatter_reduce(0, where, both, "amax")[:B]
            u = torch.rand((B, N, 3), generator=generator, device=plan.device)
            pts = (lo[:, None] + u * (hi - lo)[:, None]).reshape(B * N, 3)
            return RaggedPoints(pts, plan.rect_offsets(B, N), [N] * B)
        V = topo.vcap // topo.shapes
        va, vb = pa.reshape(-1, V, 3), pb.reshape(-1, V, 3)
        lo, hi = torch.minimum(va.amin(dim=1), vb.amin(dim=1)), torch.maximum(va.amax(dim=1), vb.amax(dim=1))
        u = torch.rand((va.shape[0], N, 3), generator=generator, device=plan.device)
        pts = lo[:, None] + u * (hi - lo)[:, None]
        return pts.reshape(lead_a + ((N, 3) if topo.kind == "shared" else (topo.shapes, N, 3)))


def volume_iou(verts_a, verts_b, plan: RayCastPlan, points: int, generator=None, cull=None):
    """The volume IoU of two poses of the plan's topology, per shape, from ``points`` uniform samples per shape in the joint
    bounding box of the two vertex sets (``iou_samples``): ``(iou, inside_a, inside_b, both)`` -- ``iou`` float64 =
    ``both / (inside_a + inside_b - both)``, 0 where the union is empty; the three counts int64, integer sums on the device.
    Shapes: the poses' leading shape (and ``B`` behind it for faces of their own or packed meshes).  No synchronisation."""
    pts = iou_samples(verts_a, verts_b, plan, points, generator)
    ia, ib = contains(pts, verts_a, plan, cull=cull), contains(pts, verts_b, plan, cull=cull)
    if isinstance(pts, RaggedPoints):
        ia, ib = ia.packed.reshape(plan.topology.shapes, -1), ib.packed.reshape(plan.topology.shapes, -1)
    a, b, both = ia.sum(dim=-1), ib.sum(dim=-1), (ia & ib).sum(dim=-1)
    union = a + b - both
    iou = torch.where(union > 0, both.double() / union.clamp(min=1).double(), torch.zeros_like(both, dtype=torch.float64))
    return iou, a, b, both
