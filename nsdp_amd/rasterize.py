"""Predicted meshes rasterised on the device (include/nsdp_raster.h, csrc/rasterize.hip): depth, face and weight images of
packed meshes, and what is built on them:

    cam = Camera.fit(verts, direction=(0, 0, -1), width=512, height=512)    # or Camera.look_at / Camera.orthographic
    plan = RasterPlan(faces, verts)                       # once per topology: ONE validating host read, the Morton order
    r = rasterize(verts, plan, cam, 512, 512)             # capturable, no host read: r.depth, .face, .bary, .count, .dropped, .hit
    rgb = shade(r, verts, plan, colors=error_colors(err)) # uint8 [..., H, W, 3]: head-light Lambert times the colour
    write_png("view.png", rgb[0])

The rule is the header's: an fp32 corner per vertex and camera, snapped to 1/256 of a pixel; EXACT integer edge signs with the
ray cast's symbolic tie-break, so a closed mesh covers every pixel an even number of times and a centre on a shared edge is
never counted twice or missed; the depth and the perspective-correct weights in fp64.  tests/raster_ref.py reproduces every
byte in numpy.  THERE IS NO NEAR-PLANE CLIPPING: a face with a corner at or behind the camera plane (W <= 0), with a
non-finite corner or with a corner more than 65 536 pixels off the origin is dropped whole and counted in ``dropped`` -- a mesh
that passes through the camera plane loses those faces.  No anti-aliasing, no textures, no backward pass.

The layouts are ``vertex_normals``' three (nsdp_amd/mesh_normals.py): shared faces ``[F, 3]`` with vertices ``[..., V, 3]``,
faces of their own ``[B, F, 3]`` with ``[..., B, V, 3]``, a ``RaggedPoints`` of faces with a ``RaggedPoints`` of vertices.
There is no CPU path and no fallback."""
from __future__ import annotations

import ctypes
import math
import struct
import zlib
from dataclasses import dataclass

import numpy as np
import torch

from ._lib import NsdpHipError, check, fptr, iptr, lib, on_device, optptr, stream_ptr
from .mesh_normals import MeshTopology, vertex_normals
from .ragged import RaggedPoints
from .ray_cast import MAX_BATCH, MAX_ROWS, RayCastError, RayCastPlan

_ci = ctypes.c_int
FRONT_ONLY = 1                  # flag of nsdp_mesh_rasterize: only faces whose corners run counter-clockwise on the screen
MAX_SIDE = 4096
MAX_IMAGES = 65535
SUBPIXEL = 256                  # snapped units per pixel


class RasterError(NsdpHipError):
    pass


# ---------------------------------------------------------------------------------------------------------------------- cameras
def _unit(v, what):
    v = np.asarray(v, np.float64).reshape(3)
    n = float(np.linalg.norm(v))
    if not math.isfinite(n) or n == 0.0:
        raise RasterError(f"Camera: {what} {v.tolist()} has no direction")
    return v / n


class Camera:
    """A 4 x 4 matrix with rows X, Y, Z, W, built on the host in float64 and rounded once to fp32: a vertex p lands at the pixel
    coordinates (X / W, Y / W) -- column first, the centre of pixel (row j, column i) at (i + 1/2, j + 1/2), rows running down
    the image -- and row Z is the distance from the eye along the viewing direction, so ``depth`` is metric.  The matrix is the
    input of the rule; how it was built is not part of the bytes."""

    def __init__(self, matrix, width: int, height: int):
        m = np.asarray(matrix, np.float64)
        if m.shape != (4, 4) or not np.isfinite(m).all():
            raise RasterError(f"Camera: the matrix must be 4 x 4 and finite, got shape {m.shape}")
        self.matrix, self.width, self.height = m.astype(np.float32), int(width), int(height)

    @staticmethod
    def _frame(eye, target, up):
        eye = np.asarray(eye, np.float64).reshape(3)
        f = _unit(np.asarray(target, np.float64).reshape(3) - eye, "target - eye")
        side = np.cross(f, _unit(up, "up"))
        if np.linalg.norm(side) < 1e-12:
            raise RasterError("Camera: up is parallel to the viewing direction")
        r = _unit(side, "right")
        return eye, f, r, np.cross(r, f)

    @classmethod
    def look_at(cls, eye, target, up, fov_deg: float, width: int, height: int):
        """A pinhole at ``eye`` looking at ``target``; ``fov_deg`` is the vertical field of view."""
        if not 0.0 < float(fov_deg) < 180.0:
            raise RasterError(f"Camera.look_at: fov_deg = {fov_deg} outside (0, 180)")
        eye, f, r, u = cls._frame(eye, target, up)
        focal = 0.5 * height / math.tan(math.radians(float(fov_deg)) / 2)
        row = lambda axis: np.concatenate([axis, [-axis @ eye]])
        xv, yv, zv = row(r), row(u), row(f)
        return cls(np.stack([focal * xv + 0.5 * width * zv, -focal * yv + 0.5 * height * zv, zv, zv]), width, height)

    @classmethod
    def orthographic(cls, eye, target, up, extent: float, width: int, height: int):
        """Parallel rays along ``target - eye``; ``extent`` is the height of the image in world units."""
        if not float(extent) > 0.0:
            raise RasterError(f"Camera.orthographic: extent = {extent}, a positive length")
        eye, f, r, u = cls._frame(eye, target, up)
        scale = height / float(extent)
        row = lambda axis: np.concatenate([axis, [-axis @ eye]])
        one = np.array([0.0, 0.0, 0.0, 1.0])
        return cls(np.stack([scale * row(r) + 0.5 * width * one, -scale * row(u) + 0.5 * height * one, row(f), one]), width, height)

    @classmethod
    def fit_box(cls, lo, hi, direction, width: int, height: int, margin: float = 0.05):
        """``fit`` for a bounding box the host already holds: corners ``lo`` and ``hi``."""
        box = np.stack([np.asarray(lo, np.float64).reshape(3), np.asarray(hi, np.float64).reshape(3)])
        if not np.isfinite(box).all():
            raise RasterError("Camera.fit: the vertices are not finite")
        d = _unit(direction, "direction")
        centre, radius = box.mean(axis=0), max(0.5 * float(np.linalg.norm(box[1] - box[0])), 1e-6)
        up = (0.0, 1.0, 0.0) if abs(d[1]) < 0.9 else (0.0, 0.0, 1.0)
        extent = 2 * radius / max(1.0 - 2 * float(margin), 1e-3) * max(1.0, height / width)
        return cls.orthographic(centre - 2 * radius * d, centre, up, extent, width, height)

    @classmethod
    def fit(cls, verts, direction, width: int, height: int, margin: float = 0.05):
        """An orthographic camera looking along ``direction`` that holds the bounding box of the device vertices ``verts``
        (any tensor [..., 3], or a RaggedPoints) with ``margin`` of the image free on every side: ONE host read."""
        pts = verts.packed if isinstance(verts, RaggedPoints) else verts
        if not torch.is_tensor(pts) or pts.shape[-1] != 3 or pts.numel() == 0:
            raise RasterError("Camera.fit: verts must be a tensor [..., 3] with at least one vertex")
        flat = pts.detach().reshape(-1, 3).double()
        box = torch.stack([flat.amin(dim=0), flat.amax(dim=0)]).cpu().numpy()
        return cls.fit_box(box[0], box[1], direction, width, height, margin)

    def __repr__(self):
        return f"Camera({self.width} x {self.height})"


def camera_tensor(cameras, device):
    """Cameras as one fp32 device tensor [..., 4, 4]: a ``Camera``, a sequence of them (-> [K, 4, 4]), or a tensor as it is."""
    if isinstance(cameras, Camera):
        cameras = [cameras]
    if isinstance(cameras, (list, tuple)):
        if not cameras or not all(isinstance(c, Camera) for c in cameras):
            raise RasterError("rasterize: cameras must be a Camera, a non-empty sequence of Cameras or a tensor [..., K, 4, 4]")
        return torch.from_numpy(np.stack([c.matrix for c in cameras])).to(device)
    return cameras


# ------------------------------------------------------------------------------------------------------------------------ entry
def mesh_rasterize(verts, vert_offsets, faces, face_offsets, cams, image_shape, height: int, width: int, return_bary: bool = True,
                   count: bool = False, flags: int = 0):
    """One nsdp_mesh_rasterize call on packed contiguous GPU operands (faces int32, local indices; cams [I, 16] fp32;
    image_shape [I] int32) -> (depth [I, H, W] fp32, face [I, H, W] int32 packed face rows, bary [I, H, W, 3] or None, count
    [I, H, W] int32 or None, dropped [I] int32)."""
    if not isinstance(verts, torch.Tensor) or not verts.is_cuda:
        raise RasterError("verts must be a GPU tensor (CPU not supported, no fallback)")
    B, I, vcap, fcap = int(vert_offsets.numel()) - 1, int(cams.shape[0]), int(verts.shape[0]), int(faces.shape[0])
    H, W = int(height), int(width)
    if cams.dim() != 2 or cams.shape[1] != 16 or image_shape.numel() != I or face_offsets.numel() != B + 1:
        raise RasterError(f"shape: cams {tuple(cams.shape)} must be (I, 16) with image_shape (I), offsets of {B} + 1 entries")
    if not (1 <= H <= MAX_SIDE and 1 <= W <= MAX_SIDE) or not 1 <= I <= MAX_IMAGES or I * H * W >= 1 << 31:
        raise RasterError(f"limits: {I} images of {H} x {W}: 1 .. {MAX_SIDE} pixels a side, 1 .. {MAX_IMAGES} images, fewer than "
                          "2^31 pixels in all")
    dev = verts.device
    for name, t in (("vert_offsets", vert_offsets), ("faces", faces), ("face_offsets", face_offsets), ("cams", cams),
                    ("image_shape", image_shape)):
        if t.device != dev:
            raise RasterError(f"{name} lives on {t.device}, verts on {dev}: one launch reads them all")
    L = lib()
    L.nsdp_mesh_rasterize_workspace_bytes.restype = ctypes.c_size_t
    need = int(L.nsdp_mesh_rasterize_workspace_bytes(_ci(B), _ci(I), _ci(fcap)))
    if need <= 0:
        raise RasterError(f"limits: nsdp_mesh_rasterize_workspace_bytes refused B={B}, I={I}, fcap={fcap} "
                          f"(1 .. {MAX_BATCH} shapes, 1 .. {MAX_IMAGES} images, 1 .. {MAX_ROWS} rows per shape)")
    with on_device(verts):
        ws = torch.empty(((need + 15) // 16 * 2,), dtype=torch.int64, device=dev)
        depth = torch.empty((I, H, W), dtype=torch.float32, device=dev)
        face = torch.empty((I, H, W), dtype=torch.int32, device=dev)
        bary = torch.empty((I, H, W, 3), dtype=torch.float32, device=dev) if return_bary else None
        cnt = torch.empty((I, H, W), dtype=torch.int32, device=dev) if count else None
        dropped = torch.empty((I,), dtype=torch.int32, device=dev)
        check(L.nsdp_mesh_rasterize(fptr(verts, "verts"), iptr(vert_offsets, "vert_offsets"), iptr(faces, "faces"),
                                    iptr(face_offsets, "face_offsets"), fptr(cams, "cams"), iptr(image_shape, "image_shape"), _ci(B),
                                    _ci(I), _ci(vcap), _ci(fcap), _ci(H), _ci(W), _ci(flags), ctypes.c_void_p(ws.data_ptr()),
                                    fptr(depth), iptr(face), optptr(bary), optptr(cnt), iptr(dropped), stream_ptr()),
              "nsdp_mesh_rasterize")
        del ws      # (stream-ordered: the allocator hands the block on behind the launches; a graph's pool keeps it)
    return depth, face, bary, cnt, dropped


class RasterPlan(RayCastPlan):
    """What ``rasterize`` needs beside the positions, built once per topology.  It IS the ray cast's plan -- the validated faces
    (ONE validating host read, ``MeshTopology``'s; pass ``topology=`` to share one that exists), reordered along a Morton curve
    of their centroids on the given pose so that a block of 64 consecutive faces covers a small part of the screen, answers in
    the caller's numbering -- plus the image-to-mesh tables of a call, kept.  ``rasterize`` takes a ``RayCastPlan`` as well."""

    def __init__(self, faces, verts, topology: MeshTopology | None = None, validate: bool = True, reorder: bool = True):
        try:
            super().__init__(faces, verts, topology=topology, validate=validate, reorder=reorder)
        except RayCastError as e:
            raise RasterError(str(e).replace("RayCastPlan", "RasterPlan")) from None

    def __repr__(self):
        return f"RasterPlan({self.topology!r}, reordered={self.reordered})"


def _image_shape(plan, M: int, K: int):
    """[M * K] int32: image i looks at mesh i // K; kept on the plan (built outside a capture: a replay makes no host copy)."""
    kept = plan.__dict__.setdefault("_image_shape", {})
    if (M, K) not in kept:
        kept[(M, K)] = torch.arange(M, dtype=torch.int32, device=plan.device).repeat_interleave(K).contiguous()
    return kept[(M, K)]


@dataclass
class Raster:
    """Per pixel, ``[..., K, H, W]`` (the vertices' leading indices, the batch index for faces of their own or packed meshes,
    then the view): ``depth`` row Z of the camera at the nearest covering face (FLT_MAX where empty), ``face`` that face in the
    caller's numbering, local to its mesh (-1: none), ``bary`` ``[..., K, H, W, 3]`` the perspective-correct weights of its
    corners (None without ``return_bary``), ``count`` the number of covering faces (None without ``count``), ``hit`` =
    ``face >= 0``; ``dropped`` ``[..., K]`` the faces of the view's mesh the rule dropped (no near-plane clipping)."""
    depth: torch.Tensor
    face: torch.Tensor
    bary: object
    count: object
    dropped: torch.Tensor
    hit: torch.Tensor
    cameras: object = None      # the matrices the images were made with, [K, 4, 4] or [..., K, 4, 4] (``shade`` reads row Z)


def refusal(verts, plan, cameras, height, width):
    """Why ``rasterize`` cannot take these operands (None: it can), each reason named."""
    if not isinstance(plan, RayCastPlan):
        return "plan must be a RasterPlan (build it once from the faces)"
    v = verts.packed if isinstance(verts, RaggedPoints) else verts
    if not torch.is_tensor(v):
        return f"verts must be a torch.Tensor or a RaggedPoints, got {type(verts).__name__}"
    if v.dtype is not torch.float32:
        return f"dtype: verts must be torch.float32, got {v.dtype} (bf16 storage is not rasterised)"
    if not v.is_cuda:
        return "CPU tensors: verts is on the CPU -- the rasteriser has no CPU path and there is no fallback"
    if not torch.is_tensor(cameras):
        return f"cameras must be a Camera, a sequence of Cameras or a tensor [..., K, 4, 4], got {type(cameras).__name__}"
    if cameras.dtype is not torch.float32:
        return f"dtype: cameras must be torch.float32, got {cameras.dtype}"
    if cameras.device != v.device or plan.device != v.device:
        return f"devices: verts on {v.device}, cameras on {cameras.device}, the plan on {plan.device}"
    if cameras.dim() < 3 or tuple(cameras.shape[-2:]) != (4, 4) or cameras.shape[-3] < 1:
        return f"shape: cameras {tuple(cameras.shape)} must be [K, 4, 4] or [..., K, 4, 4] with K >= 1"
    if not (isinstance(height, int) and isinstance(width, int)) or not (1 <= height <= MAX_SIDE and 1 <= width <= MAX_SIDE):
        return f"limits: an image of {height} x {width}: 1 .. {MAX_SIDE} pixels a side"
    return None


def rasterize(verts, plan: RayCastPlan, cameras, height: int, width: int, return_bary: bool = True, count: bool = False,
              front_only: bool = False) -> Raster:
    """Every mesh of ``verts`` (the plan's layout; every leading index a pose) under its cameras: ``cameras`` ``[K, 4, 4]`` are
    the same K views of every mesh, ``[..., K, 4, 4]`` -- the leading shape of the images -- views of their own.  Faces of both
    orientations cover a pixel; ``front_only`` keeps those whose corners run counter-clockwise as the viewer sees them.  Faces
    with a corner at or behind the camera plane are dropped whole (``dropped``): there is no near-plane clipping.  Among faces
    of equal depth bits the first in the order the kernel saw wins (the plan's Morton order).  Three launches, no
    synchronisation and no allocation whose size depends on device data: capturable."""
    cameras = camera_tensor(cameras, (verts.packed if isinstance(verts, RaggedPoints) else verts).device
                            if isinstance(verts, (RaggedPoints, torch.Tensor)) else "cpu")
    why = refusal(verts, plan, cameras, height, width)
    if why is not None:
        raise RasterError("rasterize: " + why)
    topo = plan.topology
    try:
        poses, lead = topo.poses(verts)
    except NsdpHipError as e:
        raise RasterError(str(e).replace("vertex_normals", "rasterize")) from None
    P, K = int(poses.shape[0]), int(cameras.shape[-3])
    M = P * topo.shapes
    mesh_shape = lead + (() if topo.kind == "shared" else (topo.shapes,))
    if topo.kind == "ragged" and lead != ():
        raise RasterError(f"rasterize: packed vertices are ONE pose, got the leading shape {lead}")
    if M > MAX_BATCH or M * K > MAX_IMAGES:
        raise RasterError(f"rasterize: limits: {M} meshes and {M * K} images in one call, the entry takes 1 .. {MAX_BATCH} and "
                          f"1 .. {MAX_IMAGES}")
    if cameras.dim() == 3:
        cams = cameras.reshape(1, K, 16).expand(M, K, 16)
    elif tuple(cameras.shape[:-3]) == mesh_shape:
        cams = cameras.reshape(M, K, 16)
    else:
        raise RasterError(f"rasterize: shape: cameras {tuple(cameras.shape)} against meshes of the leading shape {mesh_shape}: "
                          f"[K, 4, 4] or {list(mesh_shape) + ['K', 4, 4]}")
    with torch.no_grad():
        cams = cams.detach().reshape(M * K, 16).contiguous()
        if topo.kind == "ragged":
            faces, foff, voff = plan.faces, topo.face_offsets, topo.vert_offsets
        else:
            faces, foff, voff = plan.tiled(P)
        depth, face, bary, cnt, dropped = mesh_rasterize(poses.detach().reshape(-1, 3), voff, faces, foff, cams, _image_shape(plan, M, K),
                                                         height, width, return_bary, count, FRONT_ONLY if front_only else 0)
        # packed kernel rows -> the caller's local face numbers
        face = torch.where(face >= 0, plan._local[(face.long() % topo.fcap).clamp(min=0)], face)
    shape = mesh_shape + (K, height, width)
    return Raster(depth=depth.reshape(shape), face=face.reshape(shape), bary=bary.reshape(shape + (3,)) if return_bary else None,
                  count=cnt.reshape(shape) if count else None, dropped=dropped.reshape(mesh_shape + (K,)),
                  hit=(face >= 0).reshape(shape), cameras=cameras)


# ---------------------------------------------------------------------------------------------------------------------- shading
def _corner_rows(raster: Raster, plan: RayCastPlan):
    """Per pixel the three PACKED vertex rows of its face within one pose ([M', K, H, W, 3] int64, M' = poses x shapes
    flattened) and the pose of every mesh; pixels without a face name row 0 of their mesh."""
    topo = plan.topology
    K, H, W = raster.face.shape[-3:]
    face = raster.face.reshape(-1, topo.shapes, K, H, W).long().clamp(min=0)                 # [P, S, K, H, W]
    first_face = topo.face_offsets[:-1].long().clamp(0, topo.fcap).view(1, -1, 1, 1, 1)
    first_vert = topo.vert_offsets[:-1].long().clamp(0, topo.vcap).view(1, -1, 1, 1, 1, 1)
    tri = topo.faces.long()[(face + first_face).clamp(max=topo.fcap - 1)]                   # (the caller's order: the topology's table)
    return (tri + first_vert).clamp(max=topo.vcap - 1)                                        # [P, S, K, H, W, 3]


def interpolate(raster: Raster, plan: RayCastPlan, attr):
    """Per-vertex ``attr`` (``[V, C]`` shared by every pose, or the vertices' own layout with C in place of 3; a RaggedPoints
    for packed meshes) at every pixel by the perspective-correct weights -> ``[..., K, H, W, C]``, 0 where the pixel is empty.
    A torch gather: capturable, not the hot path.  Needs ``raster.bary``."""
    if raster.bary is None:
        raise RasterError("interpolate: the raster carries no weights (rasterize(..., return_bary=True))")
    topo = plan.topology
    a = attr.packed if isinstance(attr, RaggedPoints) else attr
    if not torch.is_tensor(a) or a.dim() < 2:
        raise RasterError("interpolate: attr must be a tensor [..., V, C] or a RaggedPoints")
    C = int(a.shape[-1])
    rows = _corner_rows(raster, plan)                                                         # [P, S, K, H, W, 3]
    Pn = rows.shape[0]
    a = a.reshape(-1, topo.vcap, C) if a.numel() == Pn * topo.vcap * C else a.reshape(1, topo.vcap, C).expand(Pn, topo.vcap, C)
    pose = torch.arange(Pn, device=rows.device).view(-1, 1, 1, 1, 1, 1)
    got = a[pose, rows]                                                                       # [P, S, K, H, W, 3, C]
    w = raster.bary.reshape(rows.shape).unsqueeze(-1).to(got.dtype)
    out = (got * w).sum(dim=-2)
    return out.reshape(tuple(raster.face.shape) + (C,))


def shade(raster: Raster, verts, plan: RayCastPlan, colors=None, normals=None, background=(255, 255, 255)):
    """uint8 ``[..., K, H, W, 3]``: a head-light Lambert term -- |n . view direction|, n the interpolated unit ``normals``
    (``vertex_normals`` of ``verts`` where none are given) and the view direction row Z of the raster's camera -- times the interpolated
    ``colors`` (float [V, 3] in 0 .. 1; white without); ``background`` where the pixel is empty.  Torch gathers: capturable."""
    topo = plan.topology
    cameras = raster.cameras
    if normals is None:
        normals = vertex_normals(verts, topo)
    n = interpolate(raster, plan, normals)
    n = n / n.norm(dim=-1, keepdim=True).clamp_min(1e-20)
    K = raster.face.shape[-3]
    view = cameras[..., 2, :3]
    view = view / view.norm(dim=-1, keepdim=True).clamp_min(1e-20)                            # [..., K, 3]
    view = view.reshape(view.shape[:-1] + (1, 1, 3)) if view.dim() > 2 else view.reshape(K, 1, 1, 3)
    light = (n * view).sum(dim=-1, keepdim=True).abs()
    base = interpolate(raster, plan, colors).clamp(0, 1) if colors is not None else torch.ones_like(n)
    rgb = to_uint8(base * (0.25 + 0.75 * light))
    if torch.is_tensor(background):
        bg = background.to(rgb.device)
    else:                                                                                     # (fill kernels: nothing is copied from the host, capturable)
        bg = torch.stack([torch.full((), int(background[k]), dtype=torch.uint8, device=rgb.device) for k in range(3)])
    return torch.where(raster.hit.unsqueeze(-1), rgb, bg.expand_as(rgb))


# ----------------------------------------------------------------------------------------------------------------- error colours
def error_colors(err, vmax: float = 0.2, use_max: bool = False):
    """The jet colours of per-vertex errors ``err`` ``[...]`` -> float32 ``[..., 3]`` in 0 .. 1: blue at 0 through cyan, green
    (at vmax / 2) and yellow to red at ``vmax`` and beyond (errors are clipped into 0 .. vmax) -- the rule of the reference's
    error maps.  ``use_max`` takes ``vmax`` from the largest error, on the device.  Computed in float64, rounded once; works on
    any device (a torch expression, no kernel of its own)."""
    e = err.detach().double()
    top = e.max().clamp_min(1e-300) if use_max else torch.tensor(float(vmax), dtype=torch.float64, device=e.device)
    x = 4.0 * (torch.minimum(e.clamp_min(0.0), top) / top)
    r, g, b = (x - 2.0).clamp(0, 1), torch.minimum(x, 4.0 - x).clamp(0, 1), (2.0 - x).clamp(0, 1)
    return torch.stack([r, g, b], dim=-1).float()


def vertex_errors(pred, target):
    """Per-vertex distance |pred - target| of two vertex sets [..., 3], in float64 (what ``error_colors`` colours: the error of
    the reference's coloured prediction, sqrt(sum((pred - tgt)^2)))."""
    d = pred.detach().double() - target.detach().double()
    return (d * d).sum(dim=-1).sqrt()


def to_uint8(colors):
    """Float colours in 0 .. 1 -> uint8 by round(255 c) (what ``meshio.write_mesh(colors=)`` and ``write_png`` take)."""
    return (colors.clamp(0, 1) * 255.0).round().to(torch.uint8)


# -------------------------------------------------------------------------------------------------------------------------- png
def write_png(path, image):
    """An 8-bit PNG of ``image``: uint8 ``[H, W, 3]`` (RGB) or ``[H, W]`` (grey), a tensor or an array; filter 0 on every row,
    one zlib stream.  numpy and zlib only."""
    if torch.is_tensor(image):
        image = image.detach().cpu().numpy()
    a = np.ascontiguousarray(image)
    if a.dtype != np.uint8 or a.ndim not in (2, 3) or (a.ndim == 3 and a.shape[2] != 3) or a.shape[0] < 1 or a.shape[1] < 1:
        raise RasterError(f"write_png: {path}: an image must be uint8 [H, W] or [H, W, 3], got {a.dtype} {a.shape}")
    h, w = a.shape[:2]
    rows = np.concatenate([np.zeros((h, 1), np.uint8), a.reshape(h, -1)], axis=1).tobytes()

    def chunk(kind, data):
        return struct.pack(">I", len(data)) + kind + data + struct.pack(">I", zlib.crc32(kind + data) & 0xFFFFFFFF)

    head = struct.pack(">IIBBBBB", w, h, 8, 2 if a.ndim == 3 else 0, 0, 0, 0)
    with open(path, "wb") as f:
        f.write(b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", head) + chunk(b"IDAT", zlib.compress(rows, 6)) + chunk(b"IEND", b""))
