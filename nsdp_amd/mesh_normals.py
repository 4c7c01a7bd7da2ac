"""Per-vertex normals of predicted meshes on the device (include/nsdp_meshnormals.h, csrc/mesh_normals.hip).

    topo = MeshTopology(faces, verts)                  # once per topology: the corner lists, ONE host read (validate=True)
    normals = vertex_normals(verts, topo)              # two launches, capturable, no atomics: bit-reproducible

The area-weighted normal of a vertex is the sum of its incident faces' cross products in a FIXED order (its ascending list of
corners, csrc/list_reduce.h's order), divided by its length; tests/mesh_normals_ref.py reproduces every bit in numpy.  Three
layouts, one mechanism (P poses of one packed topology):

  * ``faces [F, 3]`` with vertices ``[V, 3]`` -- or ``[..., V, 3]``: every leading index is a pose of the ONE face table (a
    rectangular batch that shares its faces, the T poses of a track);
  * ``faces [B, F, 3]`` with vertices ``[B, V, 3]`` (``[..., B, V, 3]``): B meshes of equal counts with faces of their own,
    packed internally;
  * a ``RaggedPoints`` of faces (indices local to their shape) with a ``RaggedPoints`` of vertices: meshes of different sizes,
    the layout of ``MeshStore.whole_meshes`` and the packed editing session.  Poses ``[..., capacity, 3]`` are taken as well.

There is no fallback: CPU tensors are refused, a missing library is an error.
"""
from __future__ import annotations

import ctypes

import torch

from ._lib import NsdpHipError, check, fptr, iptr, lib, on_device, optptr, stream_ptr
from .ragged import RaggedPoints, offsets_of, shape_ids

MAX_ROWS, MAX_CORNERS, MAX_SHAPES, MAX_POSES = 1 << 20, 1 << 25, 65535, 65535


class MeshNormalsError(NsdpHipError):
    pass


def _ci(v):
    return ctypes.c_int(int(v))


def mesh_corner_lists(faces, face_offsets, vert_offsets, vcap):
    """nsdp_mesh_corner_lists: faces (fcap, 3) int32, face_offsets / vert_offsets (B + 1) int32 on the device -> (list_offsets
    (vcap + 1), list_entries (3 fcap)) int32: the ascending list of the corners that name every packed vertex row."""
    if not isinstance(faces, torch.Tensor) or not faces.is_cuda:
        raise MeshNormalsError("faces must be a GPU tensor (CPU not supported, no fallback)")
    if faces.dim() != 2 or faces.shape[1] != 3:
        raise MeshNormalsError(f"faces must be (fcap, 3), got {tuple(faces.shape)}")
    B, vcap, fcap, dev = face_offsets.numel() - 1, int(vcap), faces.shape[0], faces.device
    if vert_offsets.numel() != B + 1:
        raise MeshNormalsError(f"{B} shapes of faces against {vert_offsets.numel() - 1} of vertices")
    _sizes(B, vcap, fcap)
    L = lib()
    L.nsdp_mesh_corner_lists_workspace_bytes.restype = ctypes.c_size_t
    need = int(L.nsdp_mesh_corner_lists_workspace_bytes(_ci(B), _ci(vcap), _ci(fcap)))
    if need <= 0:
        raise MeshNormalsError(f"nsdp_mesh_corner_lists_workspace_bytes refused B={B}, vcap={vcap}, fcap={fcap}")
    ws = torch.empty(need // 4, dtype=torch.int32, device=dev)
    list_offsets = torch.empty(vcap + 1, dtype=torch.int32, device=dev)
    list_entries = torch.empty(3 * fcap, dtype=torch.int32, device=dev)
    with on_device(faces):
        check(L.nsdp_mesh_corner_lists(iptr(faces, "faces"), iptr(face_offsets, "face_offsets"), iptr(vert_offsets, "vert_offsets"),
                                       _ci(B), _ci(vcap), _ci(fcap), ctypes.c_void_p(ws.data_ptr()), iptr(list_offsets),
                                       iptr(list_entries), stream_ptr()), "nsdp_mesh_corner_lists")
    return list_offsets, list_entries


def mesh_vertex_normals(verts, faces, face_offsets, vert_offsets, list_offsets, list_entries, want_sums=False, out=None):
    """nsdp_mesh_vertex_normals: verts (P, vcap, 3) fp32 -> (normals (P, vcap, 3), sums (P, vcap, 3) or None, face_normals
    (P, fcap, 3)).  ``out``: the normals' tensor."""
    if not isinstance(verts, torch.Tensor) or not verts.is_cuda:
        raise MeshNormalsError("verts must be a GPU tensor (CPU not supported, no fallback)")
    if verts.dim() != 3 or verts.shape[2] != 3:
        raise MeshNormalsError(f"verts must be (P, vcap, 3), got {tuple(verts.shape)}")
    P, vcap, fcap, B, dev = verts.shape[0], verts.shape[1], faces.shape[0], face_offsets.numel() - 1, verts.device
    _sizes(B, vcap, fcap)
    if not 1 <= P <= MAX_POSES:
        raise MeshNormalsError(f"{P} poses outside [1, {MAX_POSES}]")
    if list_offsets.numel() != vcap + 1 or list_entries.numel() != 3 * fcap:
        raise MeshNormalsError(f"corner lists of {list_offsets.numel() - 1} rows / {list_entries.numel()} corners against "
                               f"{vcap} vertex rows / {3 * fcap} corners")
    for name, t in (("faces", faces), ("face_offsets", face_offsets), ("vert_offsets", vert_offsets), ("list_offsets", list_offsets),
                    ("list_entries", list_entries)):
        if t.device != dev:
            raise MeshNormalsError(f"{name} lives on {t.device}, verts on {dev}: one launch reads them all")
    face_normals = torch.empty((P, fcap, 3), dtype=torch.float32, device=dev)
    sums = torch.empty((P, vcap, 3), dtype=torch.float32, device=dev) if want_sums else None
    if out is None:
        out = torch.empty((P, vcap, 3), dtype=torch.float32, device=dev)
    elif not isinstance(out, torch.Tensor) or out.device != dev or out.numel() != verts.numel():
        raise MeshNormalsError(f"out must hold {tuple(verts.shape)} fp32 values on {dev}")
    with on_device(verts):
        check(lib().nsdp_mesh_vertex_normals(fptr(verts, "verts"), _ci(P), iptr(faces, "faces"), iptr(face_offsets, "face_offsets"),
                                             iptr(vert_offsets, "vert_offsets"), _ci(B), _ci(vcap), _ci(fcap),
                                             iptr(list_offsets, "list_offsets"), iptr(list_entries, "list_entries"),
                                             fptr(face_normals), optptr(sums), fptr(out, "out"), stream_ptr()),
              "nsdp_mesh_vertex_normals")
    return out, sums, face_normals


def _sizes(B, vcap, fcap):
    if not 1 <= B <= MAX_SHAPES:
        raise MeshNormalsError(f"{B} shapes outside [1, {MAX_SHAPES}]")
    if not 1 <= vcap <= MAX_ROWS:
        raise MeshNormalsError(f"{vcap} vertex rows outside [1, {MAX_ROWS}]: the corner lists are built for at most 2^20 rows")
    if not 1 <= fcap or 3 * fcap > MAX_CORNERS:
        raise MeshNormalsError(f"{fcap} face rows outside [1, {MAX_CORNERS // 3}]: the corner lists hold at most 2^25 corners")


def _shape_of(layout):
    if isinstance(layout, torch.Tensor):
        return tuple(layout.shape)
    return tuple(int(s) for s in layout)


class MeshTopology:
    """The faces of a mesh (or of a batch of meshes) with their corner lists, on the device -- what ``vertex_normals`` needs
    beside the positions, built once.  ``verts_layout``: the vertices the topology goes with (a tensor, its shape, or a
    RaggedPoints); only the layout is read.  ``validate=True`` reads the device ONCE and refuses a face index outside its shape;
    nothing reads the device afterwards."""

    def __init__(self, faces, verts_layout, validate: bool = True):
        if isinstance(faces, RaggedPoints) != isinstance(verts_layout, RaggedPoints):
            raise MeshNormalsError("MeshTopology: packed faces go with a packed vertex layout (a RaggedPoints each)")
        if isinstance(faces, RaggedPoints):
            packed, layout = faces.packed, verts_layout
            if packed.dim() != 2 or packed.shape[1] != 3:
                raise MeshNormalsError(f"MeshTopology: packed faces must be [capacity, 3], got {tuple(packed.shape)}")
            if faces.batch != layout.batch:
                raise MeshNormalsError(f"MeshTopology: faces of {faces.batch} shapes against vertices of {layout.batch}")
            self._check_tensor(packed, layout.packed.device)
            self.kind, self.shapes = "ragged", faces.batch
            self.vcap, self.fcap = layout.capacity, faces.capacity
            self.face_offsets, self.vert_offsets = faces.offsets, layout.offsets
            self.inner = (self.vcap,)
            self._vert_layout, self._face_layout = layout, faces
        else:
            if not isinstance(faces, torch.Tensor):
                raise MeshNormalsError("MeshTopology: faces must be a tensor or a RaggedPoints")
            vshape = _shape_of(verts_layout)
            if faces.dim() == 2 and faces.shape[1] == 3 and len(vshape) >= 2 and vshape[-1] == 3:
                self.kind, self.shapes, V, F = "shared", 1, vshape[-2], faces.shape[0]
                self.inner = (V,)
            elif faces.dim() == 3 and faces.shape[2] == 3 and len(vshape) >= 3 and vshape[-1] == 3 and vshape[-3] == faces.shape[0]:
                self.kind, self.shapes, V, F = "batched", faces.shape[0], vshape[-2], faces.shape[1]
                self.inner = (self.shapes, V)
            else:
                raise MeshNormalsError(f"MeshTopology: faces {tuple(faces.shape)} with vertices {vshape}: faces [F, 3] go with "
                                       "[..., V, 3], faces [B, F, 3] with [..., B, V, 3]")
            self._check_tensor(faces, verts_layout.device if isinstance(verts_layout, torch.Tensor) else faces.device)
            packed = faces.reshape(-1, 3)
            self.vcap, self.fcap = self.shapes * V, self.shapes * F
            if V < 1 or F < 1:
                raise MeshNormalsError(f"MeshTopology: a mesh of {V} vertices and {F} faces has no normals")
            self.face_offsets = offsets_of([F] * self.shapes, faces.device)
            self.vert_offsets = offsets_of([V] * self.shapes, faces.device)
            self._vert_layout = self._face_layout = None
        _sizes(self.shapes, self.vcap, self.fcap)
        self.device = packed.device
        self.faces = packed.to(torch.int32).contiguous()      # (int64 faces are converted once, here)
        if validate:
            self._validate(packed)
        self.list_offsets, self.list_entries = mesh_corner_lists(self.faces, self.face_offsets, self.vert_offsets, self.vcap)

    @staticmethod
    def _check_tensor(faces, device):
        if not faces.is_cuda:
            raise MeshNormalsError("MeshTopology: faces must be a GPU tensor (the lists are built and kept on the device: "
                                   "CPU not supported, no fallback)")
        if faces.dtype not in (torch.int32, torch.int64):
            raise MeshNormalsError(f"MeshTopology: faces must be int32 or int64, got {faces.dtype}")
        if torch.device(device) != faces.device:
            raise MeshNormalsError(f"MeshTopology: faces on {faces.device}, vertices on {device}")

    def _validate(self, faces):
        """ONE host read: the first face row with an index outside its shape, if there is one."""
        rows = faces.shape[0]
        ids = shape_ids(self.face_offsets, rows)
        live = ids < self.shapes
        owner = ids.clamp(max=self.shapes - 1)
        counts = (self.vert_offsets[1:] - self.vert_offsets[:-1]).to(torch.int64)[owner]
        f64 = faces.to(torch.int64)
        bad = live & ((f64 < 0) | (f64 >= counts[:, None])).any(dim=1)
        q = torch.argmax(bad.to(torch.uint8))
        report = torch.cat([bad.sum().reshape(1), q.reshape(1), owner[q].reshape(1), counts[q].reshape(1), f64[q]]).tolist()
        if report[0]:
            n_bad, row, shape, count = report[:4]
            raise MeshNormalsError(f"MeshTopology: face row {row} of shape {shape} names the vertices {report[4:]}, outside "
                                   f"[0, {count}) ({n_bad} such face(s)): face indices are local to their shape")

    # ------------------------------------------------------------------ poses
    def poses(self, verts):
        """verts of this topology's layout -> (tensor (P, vcap, 3), leading shape)."""
        if isinstance(verts, RaggedPoints):
            if self.kind != "ragged" or verts.capacity != self.vcap or verts.batch != self.shapes:
                raise MeshNormalsError(f"vertex_normals: a packed set of {verts.batch} shapes in {verts.capacity} rows against a "
                                       f"{self.kind} topology of {self.shapes} shape(s) in {self.vcap} rows")
            verts = verts.packed
        if not isinstance(verts, torch.Tensor) or not verts.is_cuda:
            raise MeshNormalsError("vertex_normals: verts must be a GPU tensor (CPU not supported, no fallback)")
        if verts.dtype != torch.float32:
            raise MeshNormalsError(f"vertex_normals: verts must be float32, got {verts.dtype} (bf16 storage has no normals)")
        k = len(self.inner) + 1
        if verts.dim() < k or tuple(verts.shape[-k:]) != self.inner + (3,):
            raise MeshNormalsError(f"vertex_normals: verts {tuple(verts.shape)} against a topology over [..., "
                                   f"{', '.join(str(s) for s in self.inner)}, 3]")
        lead = tuple(verts.shape[:-k])
        return verts.contiguous().reshape(-1, self.vcap, 3), lead

    def face_shape(self, lead):
        return lead + ((self.fcap // self.shapes, 3) if self.kind == "shared" else
                       (self.shapes, self.fcap // self.shapes, 3) if self.kind == "batched" else (self.fcap, 3))

    def __repr__(self):
        return f"MeshTopology({self.kind}, shapes={self.shapes}, vertex_rows={self.vcap}, face_rows={self.fcap}, device={self.device})"


def vertex_normals(verts, topology: MeshTopology, return_sums: bool = False, return_face_normals: bool = False, out=None):
    """Unit area-weighted vertex normals of ``verts`` in the verts' own shape (a RaggedPoints for a RaggedPoints); a vertex
    without a normal (isolated, degenerate or cancelling faces) gets zeros.  ``return_sums`` / ``return_face_normals`` add the
    unnormalised sums (the verts' shape) and the faces' cross products to the result, in that order.  Two launches, no
    synchronisation and no allocation whose size depends on device data: capturable."""
    if not isinstance(topology, MeshTopology):
        raise MeshNormalsError("vertex_normals: topology must be a MeshTopology (build it once from the faces)")
    ragged = verts if isinstance(verts, RaggedPoints) else None
    poses, lead = topology.poses(verts)
    if out is not None:
        target = out.packed if isinstance(out, RaggedPoints) else out
        want = tuple((ragged.packed if ragged is not None else verts).shape)
        if not isinstance(target, torch.Tensor) or tuple(target.shape) != want or target.dtype != torch.float32 or not target.is_contiguous():
            raise MeshNormalsError(f"vertex_normals: out must be a contiguous float32 tensor of shape {want}")
        out = target
    normals, sums, fn = mesh_vertex_normals(poses, topology.faces, topology.face_offsets, topology.vert_offsets,
                                            topology.list_offsets, topology.list_entries, want_sums=return_sums, out=out)
    shape = tuple((ragged.packed if ragged is not None else verts).shape)
    wrap = (lambda t: ragged.like(t.reshape(shape))) if ragged is not None else (lambda t: t.reshape(shape))
    result = [wrap(normals)]
    if return_sums:
        result.append(wrap(sums))
    if return_face_normals:
        fn = fn.reshape(topology.face_shape(lead))
        result.append(topology._face_layout.like(fn) if ragged is not None else fn)
    return result[0] if len(result) == 1 else tuple(result)


def face_normals(verts, topology: MeshTopology):
    """The faces' area-weighted normals N_q = (p_b - p_a) x (p_c - p_a), unnormalised (twice the area long); rows no shape owns
    are zero."""
    return vertex_normals(verts, topology, return_face_normals=True)[1]
