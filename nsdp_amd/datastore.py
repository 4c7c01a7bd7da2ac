"""A data set on disk, resident on the device: the reader of the reference's directory layout, the (canonical, source, target)
pair rules of its two flow data sets, and a loader whose batches touch only the rows they keep.

The reference reads six .npz files per SAMPLE on the host (dataset/dataset_deform4d_flow.py:137-264), 200 000 fp16 rows each, to
keep a few thousand rows of them.  An MI355X holds the data set: ``SampleStore`` loads every distinct frame ONCE, in the files' own
number format, into two packed device arenas (include/nsdp_batch.h: point and normal of a surface row share a record) beside a
frame table with each frame's first record, row counts and the bounding box of its FULL surface cloud -- what the handle mask
needs (:209, "before sub-sampling"), so a batch needs no reduction.  A batch is then two kinds of launches: ``nsdp_subset_draw``
(distinct random rows by a keyed bijection: no sort of ``B x N_full`` keys) and ``nsdp_batch_assemble`` (every tensor of
``dataset.prepare_batch`` for the whole batch).  Nothing is read back and nothing synchronises per batch; the frame ids and row
counts of a whole epoch go up in one copy.

Every rank of a data-parallel job holds the WHOLE store (each rank's loader takes its share of the batches, ``shard``); a store
larger than its byte budget is refused, by name, before anything is allocated on the device.  What does not depend on a frame
being a sample pool is ``PairStore``, the core that ``meshstore.MeshStore`` derives from as well.

Out of scope for THIS store, refused by name: the user-handle data sets (``tosca``, ``dogrec``) and ``load_mesh`` -- they need
meshes, which ``meshstore`` holds (``HandleMeshStore``; ``MeshStore.whole_meshes``, and nsdp_amd/evaluate.py walks a test split
with them) -- ``partial_shape_ratio < 1`` (the reference's own call site cannot run, see dataset.py), stores larger than device
memory.
"""
from __future__ import annotations

import ctypes
import os
import random
import zipfile
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

from . import cpu_budget
from ._lib import NsdpHipError, check, iptr, lib, on_device, optptr, stream_ptr

SURFACE, SPACE = 0, 1                  # nsdp_subset_draw's `which`
MAX_ROWS = 1 << 20                     # NSDP_BATCH_MAX_ROWS
SURFACE_RECORD, SPACE_RECORD = 6, 4    # elements per arena record
_KEYS = ("cano", "src", "tgt")
FLOW_KINDS, HANDLE_KINDS = ("deform4d", "deformtransfer"), ("tosca", "dogrec")      # data.type: sequences of frames / single meshes to drag


class DataStoreError(ValueError):
    pass


# ---------------------------------------------------------------------------------------------------------------- pair rules
def _read_split(cfg_data, split, refuse):
    path = os.path.join(cfg_data["split_dir"], cfg_data["type"], split + ".lst")
    if not os.path.isfile(path):
        refuse(f"missing split list {path}")
    with open(path) as f:
        return f.read().split("\n")


def _frame_names(cfg_data, seq):
    names = sorted(os.listdir(os.path.join(cfg_data["dataset_dir"], seq)))
    return [n for n in names if int(n) % cfg_data["interval"] == 0]


def _is_seq(cfg_data, name):
    return name != "" and os.path.isdir(os.path.join(cfg_data["dataset_dir"], name))


def form_pairs(cfg_data: dict, iden_split: str, motion_split: str, refuse=None) -> list:
    """``all_deform_pairs`` before any shuffle, as the reference's ``_load`` forms them: a list of ``pair_info`` tuples
    (idx_cano, cano sequence, cano frame, idx_motion, source sequence, source frame, target sequence, target frame).
    ``deform4d``: dataset_deform4d_flow.py:37-117; ``deformtransfer``: dataset_deformtransfer_flow.py:38-116 (no identity list:
    a sequence is its own canonical sequence; ``arbitrary`` has the evaluation rule only, with the per-animal source frame).
    ``tosca`` / ``dogrec`` (the user-handle data sets, dataset_userhandle_flow.py:39-95; ``meshstore.HandleMeshStore`` alone asks
    for them): every listed directory gives ONE pair whose canonical, source and target frame are all its frame 0000.
    ``refuse``: the store's refusal, for a missing split list (default: ``SampleStore``'s)."""
    refuse = refuse or SampleStore._refuse
    kind = cfg_data["type"]
    train = motion_split[:5] == "train"
    motion_names = _read_split(cfg_data, motion_split, refuse)
    motion_dirs = sorted(n for n in motion_names if _is_seq(cfg_data, n))       # (sorting the joined paths sorts the names)
    motion_index = {n: i for i, n in enumerate(motion_dirs)}
    cano_of = {}
    if kind == "deform4d":
        iden_dirs = sorted(n for n in _read_split(cfg_data, iden_split, refuse) if _is_seq(cfg_data, n))
        for i, seq in enumerate(iden_dirs):
            cano_of[seq.split("_")[0]] = (i, seq)                                # (a later sequence of one identity wins, as there)
    pairs = []
    for seq in motion_names:
        if not _is_seq(cfg_data, seq):
            continue
        if kind == "deform4d":
            iden = seq.split("_")[0]
            if iden not in cano_of:
                continue
            idx_cano, cano_seq = cano_of[iden]
        else:
            idx_cano, cano_seq = motion_index[seq], seq
        idx_motion = motion_index[seq]
        if kind in HANDLE_KINDS:      # (dataset_userhandle_flow.py:72-95: the mesh itself, dragged; no frame list is read)
            pairs.append((idx_cano, cano_seq, "0000", idx_motion, seq, "0000", seq, "0000"))
            continue
        frames = _frame_names(cfg_data, seq)
        if cfg_data["arbitrary"]:
            if kind == "deform4d" and train:
                for f0 in frames:
                    for f1 in frames:
                        pairs.append((idx_cano, cano_seq, "0000", idx_motion, seq, f0, seq, f1))
            else:
                if kind == "deform4d":
                    first = "0000"
                elif "cat" in seq or "lion" in seq:
                    first = "0003"
                elif "horse" in seq:
                    first = "0005"
                else:
                    first = "0001"
                for f in frames:
                    if int(f) > 0:
                        pairs.append((idx_cano, cano_seq, "0000", idx_motion, seq, first, seq, f))
        else:
            for f in frames:
                pairs.append((idx_cano, cano_seq, "0000", idx_motion, cano_seq, "0000", seq, f))
    return pairs


def shuffle_order(order: list, num_sampled_pairs: int = -1):
    """``random_shuffle_samples`` (:124-129) on a list, in place: ``random.Random(100).shuffle`` -- the permutation depends on the
    length alone -- and the prefix of ``num_sampled_pairs`` (all of it unless positive).  Returns the sampled list."""
    random.Random(100).shuffle(order)
    return order[:num_sampled_pairs] if num_sampled_pairs > 0 else order


def epoch_permutation(seed: int, epoch: int, count: int) -> np.ndarray:
    """What ``DataLoader(shuffle=True)`` becomes: a host permutation of ``count`` samples, a function of (seed, epoch) alone."""
    return np.random.Generator(np.random.PCG64([int(seed) & 0xFFFFFFFFFFFFFFFF, int(epoch), 0x4E534450])).permutation(count)


# ---------------------------------------------------------------------------------------------------------------- files
def _npz_member_header(path, key):
    """(shape, dtype) of array ``key`` of an .npz file, from the member's header alone."""
    if not os.path.isfile(path):
        raise DataStoreError(f"SampleStore: missing file {path}")
    with zipfile.ZipFile(path) as z:
        if key + ".npy" not in z.namelist():
            raise DataStoreError(f"SampleStore: {path} has no array '{key}'")
        with z.open(key + ".npy") as f:
            version = np.lib.format.read_magic(f)
            read = np.lib.format.read_array_header_1_0 if version == (1, 0) else np.lib.format.read_array_header_2_0
            shape, _, dtype = read(f)
    return tuple(shape), np.dtype(dtype)


def _fix_coord_system(p):
    """dataset/utils.py:29-32: (x, y, z) -> (x, -z, y); a negation and a move: exact in every format."""
    return np.stack([p[:, 0], -p[:, 2], p[:, 1]], axis=1)


class _Frame:
    __slots__ = ("seq", "name", "dir", "surf_rows", "space_rows", "surf_dtypes", "space_dtype", "surf_first", "space_first")


# ---------------------------------------------------------------------------------------------------------------- launches
def subset_draw(n_full: torch.Tensor, n_keep: int, seed: int, epoch: int, step: int, which: int) -> torch.Tensor:
    """``n_keep`` DISTINCT rows of [0, n_full[b]) for every sample b, without sorting (nsdp_subset_draw): n_full (B,) int32 on the
    device -> int32 (B, n_keep).  A function of (seed, epoch, step, b, which) -- tests/subset_ref.py reproduces it in numpy."""
    B = n_full.shape[0]
    out = torch.empty((B, int(n_keep)), dtype=torch.int32, device=n_full.device)
    with on_device(n_full):
        check(lib().nsdp_subset_draw(iptr(n_full, "n_full"), ctypes.c_int(B), ctypes.c_int(int(n_keep)),
                                     ctypes.c_uint64(int(seed) & 0xFFFFFFFFFFFFFFFF), ctypes.c_uint32(int(epoch) & 0xFFFFFFFF),
                                     ctypes.c_uint32(int(step) & 0xFFFFFFFF), ctypes.c_int(int(which)), iptr(out, "rows_out"),
                                     stream_ptr()), "nsdp_subset_draw")
    return out


def _arena_ptr(t, name):
    if not t.is_cuda or not t.is_contiguous() or t.dtype not in (torch.float16, torch.float32):
        raise NsdpHipError(f"{name} must be a contiguous fp16 / fp32 GPU tensor (CPU not supported, no fallback)")
    return ctypes.c_void_p(t.data_ptr())


def _batch_outputs(B, n, m, device):
    """What a batch launch writes, in the order both entries take the pointers (``_ptrs``): surface [6, B, n, 3], handle
    [B, n, 1] (bytes), inputs [B, n, 7], space [3, B, m, 3]."""
    f32 = dict(dtype=torch.float32, device=device)
    return (torch.empty((6, B, n, 3), **f32), torch.empty((B, n, 1), dtype=torch.uint8, device=device),
            torch.empty((B, n, 7), **f32), torch.empty((3, B, m, 3), **f32))


def _ptrs(tensors):
    return [ctypes.c_void_p(t.data_ptr()) for t in tensors]


def _data_dict(surface, handle, inputs, space) -> dict:
    """The data_dict of ``dataset.prepare_batch`` as views of ``_batch_outputs``' tensors."""
    out = dict(zip((f"{key}_{name}" for key in ("surface_samples", "surface_normals") for name in _KEYS), surface))      # six planes
    out["cano_handle_sample_idx"] = handle.view(torch.bool)
    out["surface_samples_inputs"] = inputs
    out.update(zip((f"space_samples_{name}" for name in _KEYS), space))
    return out


def batch_assemble(surface_arena, space_arena, frame_table, frame_ids, surf_idx, space_idx, m, partial_range, noise=None,
                   noise_level=0.0) -> dict:
    """nsdp_batch_assemble: the arenas (rows, 6) / (rows, 4) fp16 or fp32, frame_table (F, 6) int64, frame_ids (3, B) int32
    (cano, src, tgt: ``inverse`` already applied), surf_idx (B, n) int32, space_idx (B, m) int32 or None (rows 0 .. m-1) -> the
    data_dict of ``dataset.prepare_batch``."""
    B, n = surf_idx.shape
    dev = surf_idx.device
    if frame_table.dtype != torch.int64 or not frame_table.is_contiguous() or not frame_table.is_cuda:
        raise NsdpHipError("frame_table must be a contiguous int64 GPU tensor")
    if noise is not None and tuple(noise.shape) != (B, n, 3):
        raise NsdpHipError(f"noise must be [B, n, 3] = {(B, n, 3)}, got {tuple(noise.shape)}")
    if space_idx is not None:
        m = space_idx.shape[1]
    outputs = _batch_outputs(B, n, int(m), dev)
    with on_device(surf_idx):
        check(lib().nsdp_batch_assemble(
            _arena_ptr(surface_arena, "surface_arena"), ctypes.c_longlong(surface_arena.shape[0]),
            ctypes.c_int(surface_arena.dtype == torch.float16), _arena_ptr(space_arena, "space_arena"),
            ctypes.c_longlong(space_arena.shape[0]), ctypes.c_int(space_arena.dtype == torch.float16),
            ctypes.c_void_p(frame_table.data_ptr()), ctypes.c_int(frame_table.shape[0]), iptr(frame_ids, "frame_ids"), ctypes.c_int(B),
            iptr(surf_idx, "surf_idx"), ctypes.c_int(n), optptr(None) if space_idx is None else iptr(space_idx, "space_idx"),
            ctypes.c_int(int(m)), ctypes.c_float(partial_range), optptr(None) if noise is None else ctypes.c_void_p(_f32(noise).data_ptr()),
            ctypes.c_float(noise_level), *_ptrs(outputs), stream_ptr()), "nsdp_batch_assemble")
    return _data_dict(*outputs)


def _f32(t):
    if t.dtype != torch.float32 or not t.is_contiguous() or not t.is_cuda:
        raise NsdpHipError("noise must be a contiguous float32 GPU tensor")
    return t


# ---------------------------------------------------------------------------------------------------------------- the store
class PairStore:
    """A device-resident store of the (canonical, source, target) frames that the pairs of (iden_split, motion_split) of
    ``config["data"]`` reference, whatever a frame holds: ``SampleStore`` (sample pools) and ``meshstore.MeshStore`` (meshes)
    add what a frame IS, and for ``StoreLoader`` a ``batch(plan, seed, epoch, step, noise)`` of a slice of ``plan_rows``.

    ``pairs``: the pair_info tuples in the reference's ``all_deform_pairs`` order before its first shuffle; ``sample_indices(e)``:
    the positions (into ``pairs``) of ``sample_deform_pairs`` during epoch ``e`` -- the reference reshuffles when the last index of
    a train split is fetched, here that happens at the end of each epoch.  Each rank of a data-parallel job holds the whole store."""

    _error = DataStoreError
    # why THIS store cannot serve what every store refuses by name: the user-handle data sets, load_mesh, partial shapes
    _refused = (None, None, None)
    _kinds = FLOW_KINDS      # the data.type values this store reads (meshstore.HandleMeshStore: HANDLE_KINDS)

    def __init__(self, config, iden_split, motion_split, num_sampled_pairs, load_mesh):
        data = config["data"]
        self.cfg_data, self.iden_split, self.motion_split = data, iden_split, motion_split
        self.num_sampled_pairs = int(num_sampled_pairs)
        self.is_train = motion_split[:5] == "train"
        kind = data.get("type")
        no_handles, no_load_mesh, no_partial = self._refused
        if kind in HANDLE_KINDS and kind not in self._kinds:
            self._refuse(f"data type '{kind}' (the user-handle data sets) {no_handles}")
        if kind not in self._kinds:
            self._refuse(f"unknown data type '{kind}' ({' and '.join(self._kinds)} are read)")
        if load_mesh:
            self._refuse(no_load_mesh)
        if data.get("partial_shape_ratio", 1.0) < 1.0:
            self._refuse(no_partial)
        if not os.path.isdir(data["dataset_dir"]):
            self._refuse(f"missing dataset_dir {data['dataset_dir']}")
        self.pairs = form_pairs(data, iden_split, motion_split, self._refuse)
        if not self.pairs:
            self._refuse(f"the splits '{iden_split}' / '{motion_split}' form no deformation pair")
        self._orders = []                 # _orders[k]: `all_deform_pairs` as positions into self.pairs after k + 1 shuffles
        self.n = int(data["num_surf_samples"])

    @classmethod
    def _refuse(cls, text):
        raise cls._error(f"{cls.__name__}: {text}")

    def _need_gpu(self):
        if self.device.type != "cuda":
            raise NsdpHipError(f"{type(self).__name__} needs a GPU device (CPU not supported, no fallback)")

    # -------------------------------------------------------------------------------------------------------- sample lists
    def sample_indices(self, epoch: int = 0) -> list:
        """Positions into ``pairs`` of the samples of epoch ``epoch`` (the prefix of num_sampled_pairs after epoch + 1 shuffles of
        a train split or of a sampled one; a sampled non-train split is shuffled once; else the list as it was formed)."""
        if not (self.is_train or self.num_sampled_pairs > 0):
            return list(range(len(self.pairs)))
        order = self.order_after(epoch + 1 if self.is_train else 1)
        return order[:self.num_sampled_pairs] if self.num_sampled_pairs > 0 else order

    def order_after(self, shuffles: int) -> list:
        """``all_deform_pairs`` as positions into ``pairs`` after ``shuffles`` calls of ``random_shuffle_samples``."""
        while len(self._orders) < shuffles:
            order = list(self._orders[-1]) if self._orders else list(range(len(self.pairs)))
            shuffle_order(order)
            self._orders.append(order)
        return self._orders[shuffles - 1] if shuffles > 0 else list(range(len(self.pairs)))

    def sample_pairs(self, epoch: int = 0) -> list:
        return [self.pairs[i] for i in self.sample_indices(epoch)]

    def __len__(self):
        return len(self.sample_indices(0))

    # -------------------------------------------------------------------------------------------------------- frames
    def _index_frames(self):
        self.frames, self._frame_id = [], {}
        ids = np.empty((len(self.pairs), 3), dtype=np.int32)
        for p, info in enumerate(self.pairs):
            for c, (seq, name) in enumerate(((info[1], info[2]), (info[4], info[5]), (info[6], info[7]))):
                if (seq, name) not in self._frame_id:
                    fr = _Frame()
                    fr.seq, fr.name, fr.dir = seq, name, os.path.join(self.cfg_data["dataset_dir"], seq, name)
                    self._frame_id[(seq, name)] = len(self.frames)
                    self.frames.append(fr)
                ids[p, c] = self._frame_id[(seq, name)]
        self.pair_frames = ids

    def _workers(self):
        return max(1, min(16, cpu_budget.cpu_budget()))

    def frame_bbox(self, frame_id):
        """(bbox_min, bbox_max) float32 of a frame (a pool's full surface cloud, a mesh's vertices), from the host frame table."""
        box = self.frame_table_host[frame_id, 3:6].copy().view(np.float32)
        return box[:3], box[3:]

    def _judge_bytes(self, nbytes, byte_budget):
        """The byte budget (default: half of the device's memory), judged on the host: nothing has been allocated yet."""
        self.nbytes = int(nbytes)
        if byte_budget is None:
            self._need_gpu()
            byte_budget = torch.cuda.get_device_properties(self.device).total_memory // 2
        self.byte_budget = int(byte_budget)
        if self.nbytes > self.byte_budget:
            self._refuse(f"{len(self.frames)} frames need {self.nbytes} bytes on the device, more than the byte budget of "
                         f"{self.byte_budget} bytes (a store larger than device memory is not supported)")

    # -------------------------------------------------------------------------------------------------------- batches
    def plan_rows(self, samples):
        """An epoch's plan: a column per sample, its (cano, src, tgt) frame ids as the pairs list them (a store may add rows)."""
        return self.pair_frames[samples].T

    def _oriented(self, frame_ids):
        """``frame_ids`` (3, B) with ``inverse`` applied, as ``prepare_batch`` applies it: source and target swapped."""
        data = self.cfg_data
        return frame_ids[[0, 2, 1]].contiguous() if not data["arbitrary"] and data["inverse"] else frame_ids

    def _noise_of(self, noise):
        """(the noise tensor a launch gets, noise_level): no tensor unless ``noise_level > 0``, which needs one."""
        level = float(self.cfg_data["noise_level"])
        if level > 0.0 and noise is None:
            raise self._error(f"{type(self).__name__}.assemble: noise_level > 0 needs a noise tensor")
        return (noise if level > 0.0 else None), level


class SampleStore(PairStore):
    """The store of PRE-SAMPLED frames: each frame's surface pool (points and normals) and space pool in two packed arenas.
    ``byte_budget``: the most device memory the arenas may take (default: half of the device's memory)."""

    _refused = ("needs meshes and is not supported", "load_mesh is not supported (meshes are not read from a data set)",
                "partial_shape_ratio < 1 is not supported from disk (the reference's own call site cannot run, see "
                "nsdp_amd/dataset.py)")

    def __init__(self, config, iden_split, motion_split, num_sampled_pairs=-1, device="cuda", load_mesh=False, byte_budget=None,
                 pairs_only=False):
        super().__init__(config, iden_split, motion_split, num_sampled_pairs, load_mesh)
        if pairs_only:
            return
        self.device = torch.device(device)
        self._index_frames()
        self._judge(byte_budget)
        self._load()

    def _judge(self, byte_budget):
        """Everything that is refused, from the files' headers: nothing has been allocated yet."""
        data = self.cfg_data

        def header(fr):
            if not os.path.isdir(fr.dir):
                raise DataStoreError(f"SampleStore: missing frame directory {fr.dir}")
            sp, dp = _npz_member_header(os.path.join(fr.dir, data["surface_flow_file"]), "points")
            sn, dn = _npz_member_header(os.path.join(fr.dir, data["surface_flow_file"]), "normals")
            qp, dq = _npz_member_header(os.path.join(fr.dir, data["space_flow_file"]), "points")
            for shape, what in ((sp, "surface points"), (sn, "surface normals"), (qp, "space points")):
                if len(shape) != 2 or shape[1] != 3:
                    raise DataStoreError(f"SampleStore: {what} of {fr.dir} have shape {shape}, not (rows, 3)")
            if sp != sn:
                raise DataStoreError(f"SampleStore: {fr.dir} has {sp[0]} surface points but {sn[0]} surface normals")
            fr.surf_rows, fr.space_rows, fr.surf_dtypes, fr.space_dtype = sp[0], qp[0], (dp, dn), dq
            return fr

        with ThreadPoolExecutor(max_workers=self._workers()) as ex:
            list(ex.map(header, self.frames))
        for fr in self.frames:
            if fr.surf_rows > MAX_ROWS or fr.space_rows > MAX_ROWS:
                raise DataStoreError(f"SampleStore: frame {fr.dir} has {fr.surf_rows} surface / {fr.space_rows} space rows, more "
                                     f"than the {MAX_ROWS} a frame may hold")
            if fr.surf_rows < self.n:
                raise DataStoreError(f"SampleStore: frame {fr.dir} has {fr.surf_rows} surface rows, fewer than num_surf_samples = {self.n}")
        for info, ids in zip(self.pairs, self.pair_frames):
            for what, attr in (("surface", "surf_rows"), ("space", "space_rows")):
                rows = [getattr(self.frames[i], attr) for i in ids]
                if len(set(rows)) != 1:
                    self._refuse(f"the frames of pair {info[1]}/{info[2]}, {info[4]}/{info[5]}, {info[6]}/{info[7]} differ in {what} "
                                 f"count ({rows}); the row indices are correspondences")
        want = int(data["num_space_samples"])
        counts = sorted({fr.space_rows for fr in self.frames})
        if counts[0] > want:
            self.m, self.draw_space = want, True
        elif len(counts) == 1:
            self.m, self.draw_space = counts[0], False          # (utils.py:49: not more than requested -> every row, in order)
        else:
            raise DataStoreError(f"SampleStore: the frames' space counts ({counts[0]} .. {counts[-1]}) are neither all above "
                                 f"num_space_samples = {want} nor all equal; such samples cannot be stacked into a batch")
        f16 = np.dtype(np.float16)
        ok = (f16, np.dtype(np.float32))
        for fr in self.frames:
            for dt in fr.surf_dtypes + (fr.space_dtype,):
                if dt not in ok:
                    raise DataStoreError(f"SampleStore: {fr.dir} holds {dt} arrays; float16 and float32 are read")
        self.surface_dtype = torch.float16 if all(d == f16 for fr in self.frames for d in fr.surf_dtypes) else torch.float32
        self.space_dtype = torch.float16 if all(fr.space_dtype == f16 for fr in self.frames) else torch.float32
        self.surface_rows = sum(fr.surf_rows for fr in self.frames)
        self.space_rows = sum(fr.space_rows for fr in self.frames)
        self._judge_bytes(self.surface_rows * SURFACE_RECORD * (2 if self.surface_dtype == torch.float16 else 4)
                          + self.space_rows * SPACE_RECORD * (2 if self.space_dtype == torch.float16 else 4) + 48 * len(self.frames),
                          byte_budget)

    def _load(self):
        self._need_gpu()
        data = self.cfg_data
        fix = bool(data["fix_coord_system"])
        np_surf = np.float16 if self.surface_dtype == torch.float16 else np.float32
        np_space = np.float16 if self.space_dtype == torch.float16 else np.float32
        first_s = first_q = 0
        for fr in self.frames:
            fr.surf_first, fr.space_first = first_s, first_q
            first_s, first_q = first_s + fr.surf_rows, first_q + fr.space_rows
        self.surface_arena = torch.empty((self.surface_rows, SURFACE_RECORD), dtype=self.surface_dtype, device=self.device)
        self.space_arena = torch.empty((self.space_rows, SPACE_RECORD), dtype=self.space_dtype, device=self.device)
        table = np.zeros((len(self.frames), 6), dtype=np.int64)

        def read(k):
            fr = self.frames[k]
            with np.load(os.path.join(fr.dir, data["surface_flow_file"])) as z:
                pts, nrm = z["points"], z["normals"]
            with np.load(os.path.join(fr.dir, data["space_flow_file"])) as z:
                spc = z["points"]
            if fix:
                pts, nrm, spc = _fix_coord_system(pts), _fix_coord_system(nrm), _fix_coord_system(spc)
            surf = np.concatenate([pts.astype(np_surf, copy=False), nrm.astype(np_surf, copy=False)], axis=1)
            space = np.zeros((spc.shape[0], SPACE_RECORD), dtype=np_space)
            space[:, :3] = spc
            p32 = pts.astype(np.float32)
            box = np.concatenate([p32.min(axis=0), p32.max(axis=0)]) if len(p32) else np.zeros(6, np.float32)
            return k, surf, space, box.astype(np.float32)

        with ThreadPoolExecutor(max_workers=self._workers()) as ex:
            for k, surf, space, box in ex.map(read, range(len(self.frames))):
                fr = self.frames[k]
                self.surface_arena[fr.surf_first:fr.surf_first + fr.surf_rows].copy_(torch.from_numpy(surf))
                self.space_arena[fr.space_first:fr.space_first + fr.space_rows].copy_(torch.from_numpy(space))
                table[k, 0], table[k, 1] = fr.surf_first, fr.space_first
                table[k, 2] = fr.surf_rows | (fr.space_rows << 32)
                table[k, 3:6] = box.view(np.int64)
        self.frame_table_host = table
        self.frame_table = torch.from_numpy(table).to(self.device)
        self.surf_counts = np.array([fr.surf_rows for fr in self.frames], dtype=np.int32)
        self.space_counts = np.array([fr.space_rows for fr in self.frames], dtype=np.int32)

    # -------------------------------------------------------------------------------------------------------- batches
    def frame_arrays(self, frame_id):
        """A frame's arrays as fp32 device tensors {surface_samples, surface_normals, space_samples} (for tests and tools)."""
        fr = self.frames[frame_id]
        s = self.surface_arena[fr.surf_first:fr.surf_first + fr.surf_rows].float()
        q = self.space_arena[fr.space_first:fr.space_first + fr.space_rows].float()
        return {"surface_samples": s[:, :3].contiguous(), "surface_normals": s[:, 3:].contiguous(), "space_samples": q[:, :3].contiguous()}

    def assemble(self, frame_ids, surf_idx, space_idx=None, noise=None) -> dict:
        """The data_dict of the samples whose (cano, src, tgt) frames are ``frame_ids`` (3, B) int32 on the device, as the pairs
        list them: ``inverse`` is applied here, as ``prepare_batch`` applies it."""
        noise, level = self._noise_of(noise)
        return batch_assemble(self.surface_arena, self.space_arena, self.frame_table, self._oriented(frame_ids), surf_idx, space_idx,
                              self.m, float(self.cfg_data["partial_range"]), noise, level)

    def plan_rows(self, samples):
        """The frame ids, and below them the row counts of each sample's surface and space pool: what its draws are taken from."""
        ids = self.pair_frames[samples]
        return np.concatenate([ids.T, self.surf_counts[ids[:, 0]][None], self.space_counts[ids[:, 0]][None]], axis=0)

    def batch(self, plan, seed, epoch, step, noise=None) -> dict:
        """The batch of the samples in ``plan`` (columns of ``plan_rows``, on the device) with nsdp_subset_draw's rows for
        (seed, epoch, step)."""
        surf_idx = subset_draw(plan[3].contiguous(), self.n, seed, epoch, step, SURFACE)
        space_idx = subset_draw(plan[4].contiguous(), self.m, seed, epoch, step, SPACE) if self.draw_space else None
        return self.assemble(plan[:3].contiguous(), surf_idx, space_idx, noise)

    def loader(self, batch, seed, noise_generator=None, shuffle=None):
        return StoreLoader(self, batch, seed, noise_generator, shuffle)


class StoreLoader:
    """An iterable of data_dict batches on the store's device; every pass over it is one epoch (its number counts up from 0).
    ``shuffle`` (default: train splits) orders an epoch's samples by ``epoch_permutation(seed, epoch)``; the rows of batch ``step``
    of epoch ``epoch`` are the store's draw for (seed, epoch, step), so two loaders with one seed give equal batches.  One plan
    copy per epoch (``store.plan_rows``), then ``store.batch`` per step; nothing is read back.
    The last partial batch of an epoch is yielded as it is.  ``noise_generator``: a torch.Generator on the device for the
    source noise (``noise_level > 0``)."""

    def __init__(self, store, batch, seed, noise_generator=None, shuffle=None):
        if int(batch) < 1:
            raise DataStoreError(f"StoreLoader: batch = {batch} must be positive")
        self.store, self.batch, self.seed, self.noise_generator = store, int(batch), int(seed), noise_generator
        self.shuffle = store.is_train if shuffle is None else bool(shuffle)
        self.epoch = 0

    def __len__(self):
        return -(-len(self.store) // self.batch)

    def epoch_samples(self, epoch):
        """Positions into ``store.pairs`` of the epoch's samples, in the order they are batched."""
        samples = np.asarray(self.store.sample_indices(epoch), dtype=np.int64)
        if self.shuffle:
            samples = samples[epoch_permutation(self.seed, epoch, len(samples))]
        return samples

    def _batches(self, steps):
        st = self.store
        epoch, self.epoch = self.epoch, self.epoch + 1
        samples = self.epoch_samples(epoch)
        plan = torch.from_numpy(np.ascontiguousarray(st.plan_rows(samples), dtype=np.int32)).to(st.device, non_blocking=True)      # one copy per epoch
        level = float(st.cfg_data["noise_level"])
        for step in steps:
            lo, hi = step * self.batch, min((step + 1) * self.batch, len(samples))
            noise = None
            if level > 0.0:
                noise = torch.randn((hi - lo, st.n, 3), device=st.device, generator=self.noise_generator)
            yield st.batch(plan[:, lo:hi].contiguous(), self.seed, epoch, step, noise)

    def __iter__(self):
        return self._batches(range(len(self)))

    def shard(self, rank, world_size):
        """This rank's share of an epoch, with ``SyntheticLoader.shard``'s meaning: of every ``world_size`` consecutive batches the
        rank-th; a trailing partial group is dropped so that all ranks take the same number of steps."""
        groups = len(self) // world_size
        return self._batches([g * world_size + rank for g in range(groups)])
