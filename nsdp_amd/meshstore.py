"""Mesh sequences on disk, resident on the device, sampled afresh for every batch: the second data path beside
``datastore.SampleStore``.

The reference's preprocessing turns every mesh sequence into frozen pools of 100 000 surface and 200 000 near-surface rows per
frame: the (face, barycentric weight, normal offset) of a row is drawn once per template and reused for every frame and epoch.
``MeshStore`` keeps the MESHES instead -- every distinct frame's vertices once, one face block per topology, and the
area thresholds of every canonical frame (include/nsdp_meshbatch.h writes the packing out) -- and ``nsdp_mesh_batch_sample``
draws face, weight and offset per row inside the launch that writes ``datastore.batch_assemble``'s tensors: fresh
correspondences every step, 16 bytes per vertex and frame on the device, no preprocessing between a directory of mesh
sequences and training.  The pair rules, the epoch order and the loader's behaviour are ``datastore``'s own (imported, not
copied); ``MeshLoader`` yields exactly ``batch_assemble``'s keys and shapes.

Each frame directory holds ``data["mesh_file"]`` (.obj, .ply or .off, nsdp_amd/meshio.py) and ``data["norm_params_file"]``, as
dataset/dataset_deform4d_flow.py:159-167 reads them: unless "norm" is in the mesh file's name the vertices are mapped by
orig2world, in float64, and rounded ONCE to float32; ``fix_coord_system`` is then applied (exact).  ``data["space_sigma"]``
(default [0.1, 0.02], the preprocessing scripts' defaults) are the half-widths of the two halves of the space rows.

One deliberate difference from the reference's loader: the handle mask uses the bounding box of the canonical frame's VERTICES.
The reference takes the box of its 100 000 pre-sampled rows, which lies just inside the vertex box (a surface sample never leaves
it); its ``cano_vert_handle_mask`` uses the vertex box as well.

Whole meshes.  What the reference's loader adds with ``load_mesh`` -- every vertex of the three meshes of a sample, the handle
mask of the canonical vertices, the 7-wide vertex rows and the faces -- comes from the same arenas by ONE launch for a batch of
meshes of DIFFERENT sizes, packed back to back (include/nsdp_meshwhole.h; ``MeshStore.whole_meshes``).  ``eval_loader`` walks a
test split with such batches beside the sampled clouds and nsdp_amd/evaluate.py is the loop around it (the reference's test.py).
The user-handle data sets (``tosca``, ``dogrec``: single meshes to drag) are ``HandleMeshStore``.

Out of scope, refused by name where they can be asked for: ``load_mesh=True`` as a constructor argument (ask the store for
``whole_meshes``); partial shapes (``partial_shape_ratio < 1``); stores beyond device memory (every rank holds the whole store, a
store over its byte budget is refused before anything is allocated); sampling by the areas of any frame other than the canonical
one.
"""
from __future__ import annotations

import ctypes
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

from . import meshio
from ._lib import NsdpHipError, check, fptr, iptr, lib, on_device, optptr, stream_ptr
from .datastore import HANDLE_KINDS, DataStoreError, PairStore, StoreLoader, _batch_outputs, _data_dict, _f32, _fix_coord_system, _ptrs, form_pairs      # noqa: F401 (form_pairs: the pair rules, re-exported)

MESH_SURFACE, MESH_SPACE = 2, 3        # NSDP_DRAW_MESH_SURFACE / NSDP_DRAW_MESH_SPACE: the `which` of the two draws' keys
MAX_ELEMS = 1 << 21                    # NSDP_MESH_MAX_ELEMS: vertices of a frame, faces of a topology
MAX_ROWS = 1 << 20                     # NSDP_BATCH_MAX_ROWS: n and m
DEFAULT_SIGMA = (0.1, 0.02)


class MeshStoreError(DataStoreError):
    pass


# ---------------------------------------------------------------------------------------------------------------- packing
def area_thresholds(verts: np.ndarray, faces: np.ndarray) -> np.ndarray:
    """The thresholds of include/nsdp_meshbatch.h for a frame of fp32 ``verts`` (V, 3) and ``faces`` (F, 3): uint32 (F,),
    non-decreasing, 2^31 from the last face of positive area onwards, equal neighbours at faces of zero area.  A draw
    ``r`` in [0, 2^31) picks the first face with T[f] > r: face f with probability area[f] / total.  ValueError when the total
    area is not positive."""
    v = np.asarray(verts, dtype=np.float32).astype(np.float64)
    a, b, c = (v[faces[:, k]] for k in range(3))
    area = np.linalg.norm(np.cross(b - a, c - a), axis=1)
    cdf = np.cumsum(area)
    if not (np.isfinite(cdf[-1]) and cdf[-1] > 0.0):
        raise ValueError("the total face area is not positive")
    T = np.floor(cdf / cdf[-1] * 2147483648.0).astype(np.uint64)
    T[np.nonzero(area > 0.0)[0][-1]:] = 1 << 31
    return T.astype(np.uint32)


def pack(verts: list, topo_of: list, faces: list, cano: list, thresholds: dict = None) -> dict:
    """Host arrays of the store as the header lays them out.  ``verts[k]``: float32 (V_k, 3) of frame k; ``topo_of[k]``: its
    topology; ``faces[t]``: int32 (F_t, 3) of topology t; ``cano``: the frames that need thresholds (``thresholds``: those
    already computed, frame -> ``area_thresholds``' result; the others are computed here).  Returns vert_arena
    (sum V, 4) f32, face_arena (sum F, 4) i32, thr_arena u32, frame_table (frames, 6) i64, topo_table (topologies, 2) i64."""
    vert_arena = np.zeros((sum(v.shape[0] for v in verts), 4), dtype=np.float32)
    face_arena = np.zeros((sum(f.shape[0] for f in faces), 4), dtype=np.int32)
    frame_table = np.zeros((len(verts), 6), dtype=np.int64)
    topo_table = np.zeros((len(faces), 2), dtype=np.int64)
    at = 0
    for t, f in enumerate(faces):
        face_arena[at:at + f.shape[0], :3] = f
        topo_table[t] = (at, f.shape[0])
        at += f.shape[0]
    at, thr, thr_at = 0, [], 0
    wants = set(int(k) for k in cano)
    for k, v in enumerate(verts):
        v = np.asarray(v, dtype=np.float32)
        vert_arena[at:at + v.shape[0], :3] = v
        frame_table[k, 0] = at
        frame_table[k, 1] = v.shape[0] | (int(topo_of[k]) << 32)
        frame_table[k, 2] = -1
        if k in wants:
            thr.append(thresholds[k] if thresholds and k in thresholds else area_thresholds(v, faces[topo_of[k]]))
            frame_table[k, 2] = thr_at
            thr_at += thr[-1].shape[0]
        box = np.concatenate([v.min(axis=0), v.max(axis=0)]) if v.shape[0] else np.zeros(6, np.float32)
        frame_table[k, 3:6] = box.astype(np.float32).view(np.int64)
        at += v.shape[0]
    thr_arena = np.concatenate(thr) if thr else np.zeros(0, dtype=np.uint32)
    return {"vert_arena": vert_arena, "face_arena": face_arena, "thr_arena": thr_arena, "frame_table": frame_table, "topo_table": topo_table}


def read_frame(cfg_data: dict, frame_dir: str):
    """(verts float32 (V, 3), faces int32 (F, 3)) of the frame directory as the store holds them: ``mesh_file`` read, mapped by
    orig2world in float64 unless "norm" is in its name, rounded ONCE to float32, then ``fix_coord_system`` (exact)."""
    path = os.path.join(frame_dir, cfg_data["mesh_file"])
    if not os.path.isfile(path):
        raise MeshStoreError(f"MeshStore: missing mesh file {path}")
    try:
        verts, faces = meshio.read_mesh(path)
    except meshio.MeshError as e:
        raise MeshStoreError(f"MeshStore: {e}") from None
    if verts.shape[0] > MAX_ELEMS or faces.shape[0] > MAX_ELEMS:
        raise MeshStoreError(f"MeshStore: frame {frame_dir} has {verts.shape[0]} vertices / {faces.shape[0]} faces, more than the "
                             f"{MAX_ELEMS} a frame may hold")
    if "norm" not in cfg_data["mesh_file"]:
        norm_path = os.path.join(frame_dir, cfg_data["norm_params_file"])
        if not os.path.isfile(norm_path):
            raise MeshStoreError(f"MeshStore: missing file {norm_path}")
        o2w = np.reshape(np.loadtxt(norm_path), [4, 4]).astype(np.float32).astype(np.float64)      # (the reference's fp32 matrix)
        verts = (np.matmul(o2w[:3, :3], verts.T) + o2w[:3, 3:4]).T                                   # float64 throughout
    verts = verts.astype(np.float32)                                                                 # the ONE rounding
    if cfg_data["fix_coord_system"]:
        verts = _fix_coord_system(verts)
    return np.ascontiguousarray(verts), faces


# ---------------------------------------------------------------------------------------------------------------- the launch
def _table_ptr(t, name, cols):
    if t.dtype != torch.int64 or not t.is_contiguous() or not t.is_cuda or t.dim() != 2 or t.shape[1] != cols:
        raise NsdpHipError(f"{name} must be a contiguous int64 GPU tensor of {cols} columns")
    return ctypes.c_void_p(t.data_ptr())


def mesh_batch_sample(vert_arena, face_arena, thr_arena, frame_table, topo_table, frame_ids, n, m, seed, epoch, step, partial_range,
                      sigma1, sigma2, noise=None, noise_level=0.0) -> dict:
    """nsdp_mesh_batch_sample: vert_arena (rows, 4) fp32, face_arena (rows, 4) int32, thr_arena (rows,) int32 holding the uint32
    thresholds' bits, frame_table (frames, 6) and topo_table (topologies, 2) int64, frame_ids (3, B) int32 (cano, src, tgt:
    ``inverse`` already applied) -> the data_dict of ``datastore.batch_assemble``, n surface and m space rows per sample, drawn
    for (seed, epoch, step) -- tests/mesh_sample_ref.py reproduces it in numpy."""
    B = frame_ids.shape[1]
    dev = frame_ids.device
    n, m = int(n), int(m)
    if vert_arena.dtype != torch.float32 or vert_arena.dim() != 2 or vert_arena.shape[1] != 4 or not vert_arena.is_contiguous():
        raise NsdpHipError("vert_arena must be a contiguous (rows, 4) float32 GPU tensor")
    if face_arena.dim() != 2 or face_arena.shape[1] != 4 or thr_arena.dim() != 1:
        raise NsdpHipError("face_arena must be (rows, 4) and thr_arena (rows,)")
    if frame_ids.dim() != 2 or frame_ids.shape[0] != 3:
        raise NsdpHipError(f"frame_ids must be [3, B], got {tuple(frame_ids.shape)}")
    for name, t in (("vert_arena", vert_arena), ("face_arena", face_arena), ("thr_arena", thr_arena), ("frame_table", frame_table),
                    ("topo_table", topo_table), ("noise", noise)):
        if t is not None and t.device != dev:
            raise NsdpHipError(f"{name} lives on {t.device}, frame_ids on {dev}: one launch reads them all")
    if noise is not None and tuple(noise.shape) != (B, n, 3):
        raise NsdpHipError(f"noise must be [B, n, 3] = {(B, n, 3)}, got {tuple(noise.shape)}")
    outputs = _batch_outputs(B, n, m, dev)
    with on_device(frame_ids):
        check(lib().nsdp_mesh_batch_sample(
            fptr(vert_arena, "vert_arena"),
            ctypes.c_longlong(vert_arena.shape[0]), iptr(face_arena, "face_arena"), ctypes.c_longlong(face_arena.shape[0]),
            iptr(thr_arena, "thr_arena"), ctypes.c_longlong(thr_arena.shape[0]), _table_ptr(frame_table, "frame_table", 6),
            ctypes.c_int(frame_table.shape[0]), _table_ptr(topo_table, "topo_table", 2), ctypes.c_int(topo_table.shape[0]),
            iptr(frame_ids, "frame_ids"), ctypes.c_int(B), ctypes.c_int(n), ctypes.c_int(m),
            ctypes.c_uint64(int(seed) & 0xFFFFFFFFFFFFFFFF), ctypes.c_uint32(int(epoch) & 0xFFFFFFFF),
            ctypes.c_uint32(int(step) & 0xFFFFFFFF), ctypes.c_float(partial_range), ctypes.c_float(sigma1), ctypes.c_float(sigma2),
            optptr(None) if noise is None else ctypes.c_void_p(_f32(noise).data_ptr()), ctypes.c_float(noise_level), *_ptrs(outputs),
            stream_ptr()), "nsdp_mesh_batch_sample")
    return _data_dict(*outputs)


def mesh_batch_whole(vert_arena, face_arena, frame_table, topo_table, frame_ids, vcap, fcap, partial_range) -> dict:
    """nsdp_mesh_batch_whole (include/nsdp_meshwhole.h): the arenas and tables of ``mesh_batch_sample``, frame_ids (3, B) int32
    (cano, src, tgt: ``inverse`` already applied) -> every vertex and face of the B samples packed back to back, as device
    tensors: vert_offsets / face_offsets (B + 1) int32, verts (3, vcap, 3) fp32 (the canonical, source and target plane),
    handle (vcap,) uint8, inputs (vcap, 7) fp32, faces (fcap, 3) int32.  All of them are written whole: rows beyond the totals
    are zero.  A batch beyond ``vcap`` / ``fcap`` is truncated -- tests/mesh_whole_ref.py reproduces it in numpy."""
    if not isinstance(frame_ids, torch.Tensor) or not frame_ids.is_cuda:
        raise NsdpHipError("frame_ids must be a GPU tensor (CPU not supported, no fallback)")
    dev = frame_ids.device
    vcap, fcap = int(vcap), int(fcap)
    if vert_arena.dtype != torch.float32 or vert_arena.dim() != 2 or vert_arena.shape[1] != 4 or not vert_arena.is_contiguous():
        raise NsdpHipError("vert_arena must be a contiguous (rows, 4) float32 GPU tensor")
    if face_arena.dim() != 2 or face_arena.shape[1] != 4:
        raise NsdpHipError("face_arena must be (rows, 4)")
    if frame_ids.dim() != 2 or frame_ids.shape[0] != 3:
        raise NsdpHipError(f"frame_ids must be [3, B], got {tuple(frame_ids.shape)}")
    B = frame_ids.shape[1]
    if B < 1:
        raise NsdpHipError("frame_ids names no sample: a batch of whole meshes needs one")
    for name, t in (("vert_arena", vert_arena), ("face_arena", face_arena), ("frame_table", frame_table), ("topo_table", topo_table)):
        if t.device != dev:
            raise NsdpHipError(f"{name} lives on {t.device}, frame_ids on {dev}: one launch reads them all")
    if not (1 <= vcap < 1 << 27 and 1 <= fcap < 1 << 27):
        raise NsdpHipError(f"capacities of {vcap} vertex and {fcap} face rows outside [1, 2^27)")
    out = {"vert_offsets": torch.empty(B + 1, dtype=torch.int32, device=dev), "face_offsets": torch.empty(B + 1, dtype=torch.int32, device=dev),
           "verts": torch.empty((3, vcap, 3), dtype=torch.float32, device=dev), "handle": torch.empty(vcap, dtype=torch.uint8, device=dev),
           "inputs": torch.empty((vcap, 7), dtype=torch.float32, device=dev), "faces": torch.empty((fcap, 3), dtype=torch.int32, device=dev)}
    with on_device(frame_ids):
        check(lib().nsdp_mesh_batch_whole(
            fptr(vert_arena, "vert_arena"), ctypes.c_longlong(vert_arena.shape[0]), iptr(face_arena, "face_arena"),
            ctypes.c_longlong(face_arena.shape[0]), _table_ptr(frame_table, "frame_table", 6), ctypes.c_int(frame_table.shape[0]),
            _table_ptr(topo_table, "topo_table", 2), ctypes.c_int(topo_table.shape[0]), iptr(frame_ids, "frame_ids"), ctypes.c_int(B),
            ctypes.c_int(vcap), ctypes.c_int(fcap), ctypes.c_float(partial_range), *_ptrs(out.values()), stream_ptr()),
            "nsdp_mesh_batch_whole")
    return out


# ---------------------------------------------------------------------------------------------------------------- the store
class MeshFrames(PairStore):
    """What a store whose frames are MESHES holds and hands out, whatever its pairs are for: the frames read and packed as
    include/nsdp_meshbatch.h lays them out, ``mesh(k)``, and whole meshes of a batch (``whole_meshes``, ``eval_loader``).
    ``MeshStore`` (sequences, sampled for training) and ``HandleMeshStore`` (single meshes to drag) derive from it."""

    _error = MeshStoreError

    def _read_meshes(self):
        """Every frame's vertices (normalised, fp32) and the distinct topologies, on the host; the refusals that need the files."""
        data = self.cfg_data
        with ThreadPoolExecutor(max_workers=self._workers()) as ex:
            loaded = list(ex.map(lambda fr: read_frame(data, fr.dir), self.frames))
        verts, topo_of, faces, seen = [], [], [], {}
        for v, f in loaded:
            key = f.tobytes()                                      # byte-identical face arrays: one topology
            if key not in seen:
                seen[key] = len(faces)
                faces.append(f)
            verts.append(v)
            topo_of.append(seen[key])
        for info, (c, s, t) in zip(self.pairs, self.pair_frames):
            for other in (s, t):
                if topo_of[other] != topo_of[c]:
                    raise MeshStoreError(f"MeshStore: the frames {self.frames[c].dir} and {self.frames[other].dir} of one pair differ in "
                                         f"topology ({faces[topo_of[c]].shape[0]} and {faces[topo_of[other]].shape[0]} faces, or other "
                                         f"indices); a face index is the correspondence")
        return {"verts": verts, "topo_of": topo_of, "faces": faces, "cano": [], "thresholds": {}}

    def _upload(self, host):
        self._need_gpu()
        packed = pack(host["verts"], host["topo_of"], host["faces"], host["cano"], host["thresholds"])
        self.topo_of = np.asarray(host["topo_of"], dtype=np.int32)
        self.frame_table_host, self.topo_table_host = packed["frame_table"], packed["topo_table"]
        self.vert_arena = torch.from_numpy(packed["vert_arena"]).to(self.device)
        self.face_arena = torch.from_numpy(packed["face_arena"]).to(self.device)
        self.thr_arena = torch.from_numpy(packed["thr_arena"].view(np.int32)).to(self.device)      # (the uint32 thresholds' bits)
        self.frame_table = torch.from_numpy(packed["frame_table"]).to(self.device)
        self.topo_table = torch.from_numpy(packed["topo_table"]).to(self.device)

    def mesh(self, frame_id):
        """(verts fp32 (V, 3), faces int32 (F, 3)) of a frame as device tensors (for tests and tools)."""
        first, word = int(self.frame_table_host[frame_id, 0]), int(self.frame_table_host[frame_id, 1])
        f0, count = (int(x) for x in self.topo_table_host[word >> 32])
        return (self.vert_arena[first:first + (word & 0xFFFFFFFF), :3].contiguous(), self.face_arena[f0:f0 + count, :3].contiguous())

    # -------------------------------------------------------------------------------------------------------- whole meshes
    def mesh_counts(self, host_frame_ids):
        """(vertex counts, face counts) of the samples whose frames are ``host_frame_ids`` (3, B) on the host: the canonical
        frame's count and its topology's, from the host copy of the tables."""
        words = self.frame_table_host[np.asarray(host_frame_ids)[0], 1]
        return [int(w) & 0xFFFFFFFF for w in words], [int(self.topo_table_host[int(w) >> 32, 1]) for w in words]

    def whole_meshes(self, frame_ids, host_frame_ids=None, capacity=None, face_capacity=None) -> dict:
        """The reference's ``load_mesh`` keys for the samples whose (cano, src, tgt) frames are ``frame_ids`` (3, B) int32 on the
        device, as the pairs list them (``inverse`` is applied here), whole meshes of different sizes packed back to back by ONE
        call of nsdp_mesh_batch_whole: ``verts_cano`` / ``verts_src`` / ``verts_tgt`` (``RaggedPoints`` over one offsets tensor),
        ``cano_handle_vert_idx`` ([capacity, 1] bool), ``verts_flow_inputs`` (``RaggedPoints`` of [capacity, 7] rows) and
        ``faces`` (a ``RaggedPoints`` of int32 rows, indices local to their mesh, over the face offsets: what
        ``compute_evaluation_metrics_batch`` takes).

        ``host_frame_ids``: the same ids on the host.  The counts then come from ``frame_table_host``, the capacities default to
        the exact totals, a batch beyond a given capacity is refused before the launch, and the sets carry host counts.  Without
        it both capacities must be given and nothing is read back -- a captured call replays for any batch within them (one
        beyond them is truncated, include/nsdp_meshwhole.h)."""
        from .ragged import RaggedPoints
        name = type(self).__name__
        vcounts = fcounts = None
        if host_frame_ids is not None:
            host_frame_ids = np.asarray(host_frame_ids)
            if host_frame_ids.shape != tuple(frame_ids.shape):
                raise MeshStoreError(f"{name}.whole_meshes: host_frame_ids {host_frame_ids.shape} against frame_ids {tuple(frame_ids.shape)}")
            vcounts, fcounts = self.mesh_counts(host_frame_ids)
            capacity = max(sum(vcounts), 1) if capacity is None else int(capacity)
            face_capacity = max(sum(fcounts), 1) if face_capacity is None else int(face_capacity)
            if sum(vcounts) > capacity or sum(fcounts) > face_capacity:
                raise MeshStoreError(f"{name}.whole_meshes: {sum(vcounts)} vertices / {sum(fcounts)} faces do not fit the capacities "
                                     f"{capacity} / {face_capacity}")
        elif capacity is None or face_capacity is None:
            raise MeshStoreError(f"{name}.whole_meshes: without host_frame_ids the counts are on the device alone: capacity and "
                                 "face_capacity must be given")
        out = mesh_batch_whole(self.vert_arena, self.face_arena, self.frame_table, self.topo_table, self._oriented(frame_ids),
                               capacity, face_capacity, float(self.cfg_data["partial_range"]))
        voff = out["vert_offsets"]
        return {"verts_cano": RaggedPoints(out["verts"][0], voff, vcounts), "verts_src": RaggedPoints(out["verts"][1], voff, vcounts),
                "verts_tgt": RaggedPoints(out["verts"][2], voff, vcounts),
                "cano_handle_vert_idx": out["handle"].view(torch.bool).unsqueeze(1),
                "verts_flow_inputs": RaggedPoints(out["inputs"], voff, vcounts),
                "faces": RaggedPoints(out["faces"], out["face_offsets"], fcounts)}

    def eval_samples(self, frame_ids, seed, step) -> dict:
        """What a batch of the evaluation loader holds beside its whole meshes (``MeshStore``: the sampled clouds)."""
        return {}

    def eval_loader(self, batch, seed):
        return EvalLoader(self, batch, seed)


class MeshStore(MeshFrames):
    """The store of MESH frames: every distinct frame's vertices, one face block per topology and the area thresholds of every
    canonical frame.  The constructor's arguments, ``pairs``, ``sample_indices``, ``len()`` and ``pairs_only`` are as
    ``SampleStore``'s (both are ``datastore.PairStore``s).  ``nbytes``: what the arenas and tables take on the device;
    ``byte_budget``: the most they may (default: half of the device's memory)."""

    _refused = ("is not supported by this store (meshstore.HandleMeshStore reads them)",
                "load_mesh batches (whole meshes beside the samples) are not supported by the constructor: whole_meshes and "
                "eval_loader hand them out",
                "partial_shape_ratio < 1 (partial shapes) is not supported")

    def __init__(self, config, iden_split, motion_split, num_sampled_pairs=-1, device="cuda", load_mesh=False, byte_budget=None,
                 pairs_only=False):
        super().__init__(config, iden_split, motion_split, num_sampled_pairs, load_mesh)
        data = self.cfg_data
        self.m = int(data["num_space_samples"])
        if pairs_only:
            return
        if "mesh_file" not in data:
            self._refuse("the data section names no mesh_file")
        if not 0 <= self.n <= MAX_ROWS or not 0 <= self.m <= MAX_ROWS:
            self._refuse(f"num_surf_samples = {self.n} / num_space_samples = {self.m} outside [0, {MAX_ROWS}]")
        sigma = data.get("space_sigma", list(DEFAULT_SIGMA))
        if len(sigma) != 2 or not all(np.isfinite(float(s)) for s in sigma):
            self._refuse(f"space_sigma = {sigma} must be two finite numbers")
        self.sigma = (float(sigma[0]), float(sigma[1]))
        self.device = torch.device(device)
        self._index_frames()
        host = self._read()
        self.vert_rows = sum(v.shape[0] for v in host["verts"])
        self.face_rows = sum(f.shape[0] for f in host["faces"])
        self.thr_rows = sum(host["faces"][host["topo_of"][k]].shape[0] for k in host["cano"])
        self._judge_bytes(16 * self.vert_rows + 16 * self.face_rows + 4 * self.thr_rows + 48 * len(self.frames) + 16 * len(host["faces"]),
                          byte_budget)
        self._upload(host)

    # -------------------------------------------------------------------------------------------------------- frames
    def _read(self):
        """``_read_meshes`` and the area thresholds of every canonical frame."""
        host = self._read_meshes()
        verts, topo_of, faces = host["verts"], host["topo_of"], host["faces"]
        host["cano"] = sorted(set(int(c) for c in self.pair_frames[:, 0]))
        for k in host["cano"]:
            try:
                host["thresholds"][k] = area_thresholds(verts[k], faces[topo_of[k]])      # (once: pack takes them as they are)
            except ValueError:
                raise MeshStoreError(f"MeshStore: the canonical frame {self.frames[k].dir} has zero total area; its faces cannot be "
                                     f"drawn by area") from None
        return host

    # -------------------------------------------------------------------------------------------------------- batches
    def assemble(self, frame_ids, seed, epoch, step, noise=None) -> dict:
        """The data_dict of the samples whose (cano, src, tgt) frames are ``frame_ids`` (3, B) int32 on the device, as the pairs
        list them (``inverse`` is applied here, as ``prepare_batch`` applies it), with the rows of (seed, epoch, step)."""
        noise, level = self._noise_of(noise)
        return mesh_batch_sample(self.vert_arena, self.face_arena, self.thr_arena, self.frame_table, self.topo_table,
                                 self._oriented(frame_ids), self.n, self.m, seed, epoch, step, float(self.cfg_data["partial_range"]),
                                 self.sigma[0], self.sigma[1], noise, level)

    batch = assemble      # (a loader's plan is the frame ids alone: PairStore.plan_rows)

    def loader(self, batch, seed, noise_generator=None, shuffle=None):
        return MeshLoader(self, batch, seed, noise_generator, shuffle)

    def eval_samples(self, frame_ids, seed, step) -> dict:
        """``assemble(frame_ids, seed, 0, step)``; with ``noise_level > 0`` the source noise is drawn for (seed, step)."""
        noise = None
        if float(self.cfg_data["noise_level"]) > 0.0:
            g = torch.Generator(device=self.device).manual_seed((int(seed) * 1000003 + int(step)) & 0x7FFFFFFFFFFFFFFF)
            noise = torch.randn((frame_ids.shape[1], self.n, 3), device=self.device, generator=g)
        return self.assemble(frame_ids, seed, 0, step, noise)


class HandleMeshStore(MeshFrames):
    """The user-handle data sets (``data.type`` ``tosca`` / ``dogrec``, dataset/dataset_userhandle_flow.py): every directory the
    motion split lists is ONE mesh to drag, its frame ``0000`` being canonical, source and target at once, so ``whole_meshes``
    gives ``verts_cano`` = ``verts_src`` (= ``verts_tgt``: the target of a drag is made by the handle kernel, nsdp_amd.edit).
    No samples are drawn -- the cloud of such a mesh is its own vertex set -- and no thresholds are kept.  The constructor's
    arguments are ``MeshStore``'s; ``iden_split`` is not read, as in the reference."""

    _kinds = HANDLE_KINDS
    _refused = ("is not supported", "load_mesh is what this store does: ask it for whole_meshes / eval_loader",
                "partial_shape_ratio < 1 (partial shapes) is not supported")

    def __init__(self, config, iden_split, motion_split, num_sampled_pairs=-1, device="cuda", load_mesh=False, byte_budget=None,
                 pairs_only=False):
        super().__init__(config, iden_split, motion_split, num_sampled_pairs, load_mesh)
        if pairs_only:
            return
        if "mesh_file" not in self.cfg_data:
            self._refuse("the data section names no mesh_file")
        self.device = torch.device(device)
        self._index_frames()
        host = self._read_meshes()
        self.vert_rows = sum(v.shape[0] for v in host["verts"])
        self.face_rows = sum(f.shape[0] for f in host["faces"])
        self._judge_bytes(16 * self.vert_rows + 16 * self.face_rows + 48 * len(self.frames) + 16 * len(host["faces"]), byte_budget)
        self._upload(host)


class EvalLoader:
    """The test split in order, whole meshes beside the samples: walks ``store.sample_indices(0)`` ``batch`` pairs at a time (the
    last batch is what remains).  The plan goes up once and is sliced on the device; each batch is ``store.eval_samples`` (a
    ``MeshStore``: ``assemble(ids, seed, 0, step)``) plus the keys of ``store.whole_meshes`` (with host counts: exact capacities)
    plus ``index``, the positions into ``store.pairs`` (a host list)."""

    def __init__(self, store, batch, seed):
        if int(batch) < 1:
            raise DataStoreError(f"EvalLoader: batch = {batch} must be positive")
        self.store, self.batch, self.seed = store, int(batch), int(seed)
        self.samples = np.asarray(store.sample_indices(0), dtype=np.int64)

    def __len__(self):
        return -(-len(self.samples) // self.batch)

    def __iter__(self):
        st = self.store
        host = np.ascontiguousarray(st.pair_frames[self.samples].T, dtype=np.int32)
        plan = torch.from_numpy(host).to(st.device, non_blocking=True)      # one copy
        for step in range(len(self)):
            lo, hi = step * self.batch, min((step + 1) * self.batch, len(self.samples))
            ids = plan[:, lo:hi].contiguous()
            data_dict = st.eval_samples(ids, self.seed, step)
            data_dict.update(st.whole_meshes(ids, host[:, lo:hi]))
            data_dict["index"] = self.samples[lo:hi].tolist()
            yield data_dict


class MeshLoader(StoreLoader):
    """``StoreLoader`` over a ``MeshStore``: the same epochs, ``shuffle``, ``shard`` and partial last batch; the rows of batch
    ``step`` of epoch ``epoch`` are nsdp_mesh_batch_sample's for (seed, epoch, step), so two loaders with one seed give equal
    batches.  One plan copy per epoch, one launch per batch, nothing read back.  Nothing is overridden: the loader asks its store."""
