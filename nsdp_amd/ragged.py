"""Packed ("ragged") query sets: a batch of meshes of different vertex counts decoded in one call.

    verts = RaggedPoints.from_list([v0, v1, v2])                    # [n_b, 3] tensors on the GPU
    data_dict["verts_src"] = verts
    loss, data_dict = test_on_batch(model, data_dict, config)       # test_on_batch_with_cano / _with_arbitrary
    for pred in data_dict["verts_tgt_pred"].split(): ...            # a RaggedPoints comes back: [n_b, 3] per mesh

Layout (include/nsdp_hip.h, csrc/ragged.h): the rows of all shapes concatenated, ``packed [capacity, 3]`` fp32, plus
``offsets [B + 1]`` int32 ON THE DEVICE -- shape ``b`` owns rows ``offsets[b] .. offsets[b + 1]``, ``offsets[B] = total``.
Rows at or beyond ``total`` are padding: no kernel reads them as results or writes them.  The kernels take the capacity and
``B`` from the host (they fix the launch grid) and everything else from ``offsets`` on the device, so ONE captured graph
serves every batch of ``B`` meshes whose vertices sum to at most the capacity (``RaggedTestOnBatch(graph=True)``).  A
decoder wave's 16 queries and a kNN workgroup's 256 belong to one shape and a shape's last tile is partial, exactly like
the tail of the rectangular call: every row gets the bits the rectangular call gives it.  Inference only.

The surface cloud may be packed as well -- shapes that bring different numbers of surface samples (every vertex of a mesh as
the user-handle data does, a partial scan), which cannot be padded: extra points change the sampling, every neighbourhood and
the max-pool.

    surf = RaggedPoints.from_rows([s0, s1, s2])                     # [n_b, 7] rows: source, target, handle mask
    data_dict["surface_samples_inputs"] = surf
    data_dict["surface_samples_src"] = surf.columns(0, 3)
    loss, data_dict = test_on_batch(model, data_dict, config)       # surface_samples_tgt_pred comes back packed as well

Only the encoder's first level is ragged (PointTransformerEncoder.forward): farthest-point sampling and the neighbour searches
run over the packed rows (pointnet2_utils.furthest_point_sample_ragged / knn_ragged_source, sizes from the offsets on the
device), the first attention block and the first set abstraction see the rows as one shape [1, total, .], and from the first
down-sampled level on every tensor is [B, n1, .] again.  With eval-mode BatchNorm (a per-row affine map) every shape gets what
its own batch-1 call gives it.  The encoder works on the tight rows ``packed[:total]``, so a call with ragged surfaces reads
the counts on the host and is not captured into a graph (RaggedTestOnBatch runs it eagerly).
"""
from __future__ import annotations

import torch


class RaggedPoints:
    """``packed [capacity, C]`` + ``offsets [B + 1]`` int32 on the same device (+ the host's copy of the counts, if it has
    one).  Built from device offsets alone it carries no host counts: ``split()`` / ``padded()`` / ``counts`` then read the
    offsets back -- one synchronisation, never on a replayed path."""

    def __init__(self, packed: torch.Tensor, offsets: torch.Tensor, counts=None):
        if not torch.is_tensor(packed) or packed.dim() != 2:
            raise ValueError(f"RaggedPoints: packed must be [capacity, C], got {tuple(getattr(packed, 'shape', ()))}")
        if not torch.is_tensor(offsets) or offsets.dim() != 1 or offsets.numel() < 1 or offsets.dtype != torch.int32:
            raise ValueError("RaggedPoints: offsets must be a [B + 1] int32 tensor")
        if offsets.device != packed.device:
            raise ValueError(f"RaggedPoints: packed on {packed.device}, offsets on {offsets.device}")
        self.packed, self.offsets = packed, offsets
        self._counts = None
        if counts is not None:
            counts = tuple(int(c) for c in counts)
            if len(counts) != self.batch or min(counts, default=0) < 0 or sum(counts) > self.capacity:
                raise ValueError(f"RaggedPoints: counts {counts} do not describe {self.batch} shapes within {self.capacity} rows")
            self._counts = counts

    @classmethod
    def from_list(cls, tensors, capacity=None):
        """[n_b, 3] tensors (one device, one dtype; n_b = 0 is legal) -> a packed set of ``capacity`` rows (default: their
        sum; padding rows are zero).  Validated on the host: the offsets are monotone and fit the capacity by construction."""
        tensors = list(tensors)
        if not tensors:
            raise ValueError("RaggedPoints.from_list: no shapes")
        for t in tensors:
            if not torch.is_tensor(t) or t.dim() != 2 or t.shape[1] != 3:
                raise ValueError(f"RaggedPoints.from_list: every shape must be [n, 3], got {tuple(getattr(t, 'shape', ()))}")
            if t.device != tensors[0].device or t.dtype != tensors[0].dtype:
                raise ValueError("RaggedPoints.from_list: the shapes must share a device and a dtype")
        counts = [int(t.shape[0]) for t in tensors]
        total = sum(counts)
        capacity = total if capacity is None else int(capacity)
        if total > capacity:
            raise ValueError(f"RaggedPoints.from_list: {total} rows do not fit the capacity {capacity}")
        packed = tensors[0].new_zeros((capacity, 3))
        if total:
            torch.cat(tensors, dim=0, out=packed[:total])
        return cls(packed, offsets_of(counts, packed.device), counts)

    @classmethod
    def from_rows(cls, tensors, capacity=None):
        """``from_list`` for rows of any one width: [n_b, C] tensors (a surface cloud's [n_b, 7] rows) -> packed [capacity, C]."""
        tensors = list(tensors)
        if not tensors:
            raise ValueError("RaggedPoints.from_rows: no shapes")
        for t in tensors:
            if not torch.is_tensor(t) or t.dim() != 2 or t.shape[1] != tensors[0].shape[1] or t.shape[1] < 1:
                raise ValueError(f"RaggedPoints.from_rows: every shape must be [n, C] with one C, got {tuple(getattr(t, 'shape', ()))}")
            if t.device != tensors[0].device or t.dtype != tensors[0].dtype:
                raise ValueError("RaggedPoints.from_rows: the shapes must share a device and a dtype")
        counts = [int(t.shape[0]) for t in tensors]
        total = sum(counts)
        capacity = total if capacity is None else int(capacity)
        if total > capacity:
            raise ValueError(f"RaggedPoints.from_rows: {total} rows do not fit the capacity {capacity}")
        packed = tensors[0].new_zeros((capacity, int(tensors[0].shape[1])))
        if total:
            torch.cat(tensors, dim=0, out=packed[:total])
        return cls(packed, offsets_of(counts, packed.device), counts)

    def columns(self, lo: int, hi: int) -> "RaggedPoints":
        """Columns [lo, hi) of every row as a packed set of their own (a contiguous copy) over the same offsets and counts:
        the coordinates ``columns(0, 3)`` of a [capacity, 7] surface input."""
        lo, hi = int(lo), int(hi)
        if not 0 <= lo < hi <= self.packed.shape[1]:
            raise ValueError(f"RaggedPoints.columns: [{lo}, {hi}) of {self.packed.shape[1]} columns")
        return RaggedPoints(self.packed[:, lo:hi].contiguous(), self.offsets, self._counts)

    def same_layout(self, other) -> bool:
        """Do the two sets describe the same shapes in the same rows (one offsets tensor, or equal host counts)?"""
        if not isinstance(other, RaggedPoints) or other.batch != self.batch or other.capacity != self.capacity:
            return False
        return other.offsets is self.offsets or other.counts == self.counts

    @property
    def capacity(self) -> int:
        return int(self.packed.shape[0])

    @property
    def batch(self) -> int:
        return int(self.offsets.numel()) - 1

    @property
    def device(self):
        return self.packed.device

    @property
    def is_cuda(self) -> bool:
        return self.packed.is_cuda

    @property
    def counts(self):
        """Rows per shape on the host (read back from the device offsets once if this set was built from them alone; clamped
        like the kernels clamp them)."""
        if self._counts is None:
            offs, cap = [int(v) for v in self.offsets.tolist()], self.capacity
            prev, counts = min(max(offs[0], 0), cap), []
            for o in offs[1:]:
                o = min(max(o, prev), cap)
                counts.append(o - prev)
                prev = o
            self._counts = tuple(counts)
        return self._counts

    @property
    def total(self) -> int:
        return sum(self.counts)

    def like(self, packed: torch.Tensor) -> "RaggedPoints":
        """The same offsets over new rows (what a decode returns)."""
        if packed.shape[0] != self.capacity:
            raise ValueError(f"RaggedPoints.like: {packed.shape[0]} rows against a capacity of {self.capacity}")
        return RaggedPoints(packed, self.offsets, self._counts)

    def split(self):
        """The shapes as a list of [n_b, C] views."""
        return list(torch.split(self.packed[:self.total], list(self.counts), dim=0))

    def padded(self, fill: float = 0.0) -> torch.Tensor:
        """[B, max_b n_b, C], rows beyond a shape's count = ``fill``."""
        counts = self.counts
        out = self.packed.new_full((self.batch, max(counts, default=0), self.packed.shape[1]), fill)
        for b, rows in enumerate(self.split()):
            out[b, :counts[b]] = rows
        return out

    def to(self, device) -> "RaggedPoints":
        return RaggedPoints(self.packed.to(device), self.offsets.to(device), self._counts)

    def __repr__(self):
        return f"RaggedPoints(batch={self.batch}, capacity={self.capacity}, counts={self._counts}, device={self.device})"


def offsets_of(counts, device) -> torch.Tensor:
    """[B + 1] int32 offsets of host counts, on ``device``."""
    offs = [0]
    for c in counts:
        if int(c) < 0:
            raise ValueError(f"negative vertex count {c}")
        offs.append(offs[-1] + int(c))
    if offs[-1] >= 2 ** 31:
        raise ValueError("a packed set holds fewer than 2^31 rows")
    return torch.tensor(offs, dtype=torch.int32).to(device)


def shape_ids(offsets: torch.Tensor, capacity: int) -> torch.Tensor:
    """[capacity] int64: the shape of every row, B for the padding rows.  On the device, no synchronisation."""
    rows = torch.arange(capacity, device=offsets.device, dtype=torch.int32)
    return torch.bucketize(rows, offsets[1:].contiguous(), right=True)


def l2_error(pred: RaggedPoints, target: RaggedPoints) -> torch.Tensor:
    """Mean over the shapes of the per-shape model.utils.compute_l2_error (what B calls at batch 1 average to); a shape
    without vertices is left out of the mean.  Computed on the device from the offsets (padding rows may hold anything)."""
    if pred.batch != target.batch:
        raise ValueError(f"ragged l2 error: {pred.batch} predicted shapes against {target.batch} targets")
    B, rows = pred.batch, min(pred.capacity, target.capacity)      # (both hold the `total` real rows; the rest is padding)
    ids = shape_ids(pred.offsets, rows)
    err = (pred.packed[:rows] - target.packed[:rows]).pow(2).sum(dim=1) / 2.0
    err = torch.where(ids < B, err, torch.zeros_like(err))
    sums = torch.zeros(B + 1, dtype=err.dtype, device=err.device).index_add_(0, ids, err)[:B]
    counts = (pred.offsets[1:] - pred.offsets[:-1]).to(err.dtype)
    some = counts > 0
    per_shape = torch.where(some, sums / counts.clamp(min=1), torch.zeros_like(sums))
    return per_shape.sum() / some.sum().clamp(min=1)


def as_ragged(verts, capacity=None) -> RaggedPoints:
    """A RaggedPoints as it is, a list of [n_b, 3] tensors packed."""
    return verts if isinstance(verts, RaggedPoints) else RaggedPoints.from_list(verts, capacity)


class RaggedTestOnBatch:
    """``fn(model, data_dict, config, compute_loss=False) -> (loss, data_dict)``: the reference-shaped dense-inference step
    for meshes of different sizes.  ``data_dict["verts_src"]`` (and ``["verts_tgt"]`` with ``compute_loss``) is a list of
    [n_b, 3] tensors or a RaggedPoints; ``data_dict["verts_tgt_pred"]`` comes back as a RaggedPoints of exactly ``total``
    rows, a tensor of the caller's own.

    ``graph=True``: the first call captures the step (graph_step.GraphedStep over frozen weights: the model must be in eval
    mode and its weights must not change afterwards) over a static [capacity, 3] vertex buffer, static offsets and static
    copies of the rectangular inputs.  Every later call with the same model, B and surface shapes and ``total <= capacity``
    copies its vertices and offsets into them and replays (``replays``) -- whatever the mix of sizes: the kernels read the
    sizes from the offsets on the device.  Anything else runs eagerly (``eager_calls``) -- a call whose SURFACE clouds are
    ragged (``surface_samples_inputs`` / ``surface_samples_src`` as RaggedPoints: passed through as they are, and
    ``surface_samples_tgt_pred`` comes back as one) among them: the encoder works on the tight rows of the cloud, whose number
    the host reads, so such a step is not captured."""

    RECT_INPUTS = ("surface_samples_inputs", "surface_samples_src")

    def __init__(self, test_on_batch, capacity: int, graph: bool = False, max_streams=None):
        self.fn, self.capacity, self.graph, self.max_streams = test_on_batch, int(capacity), bool(graph), max_streams
        if self.capacity <= 0:
            raise ValueError(f"RaggedTestOnBatch: capacity {capacity}")
        self._step = self._static = self._key = None
        self.replays = self.eager_calls = 0

    def _rect(self, data_dict):
        return {k: data_dict[k] for k in self.RECT_INPUTS if torch.is_tensor(data_dict.get(k))}

    def _run(self, model, dd, config):
        # (the step function writes its predictions into the dict it is given: a private one)
        _, out = self.fn(model, dd, config)
        return out["surface_samples_tgt_pred"], out["verts_tgt_pred"]

    def _replayed(self, model, data_dict, verts, config):
        rect = self._rect(data_dict)
        key = (id(model), verts.batch, tuple((k, tuple(v.shape), v.dtype, v.device) for k, v in rect.items()))
        if self._step is None:
            if model.training:
                raise ValueError("RaggedTestOnBatch(graph=True) replays frozen-weight inference: call model.eval() first")
            from .graph_step import GraphedStep
            dev = verts.device
            static = {k: v.clone() for k, v in rect.items()}
            # (captured over a legal set: everything in the first shape or, if this first call is too big, nothing at all)
            first = verts.total if verts.total <= self.capacity else 0
            static["verts_src"] = RaggedPoints(torch.zeros((self.capacity, 3), dtype=torch.float32, device=dev),
                                               offsets_of([first] + [0] * (verts.batch - 1), dev))
            self._key, self._static = key, static
            self._step = GraphedStep(lambda: self._run(model, dict(self._static), config), self.max_streams,
                                     weights_change=False).capture(warmup=1)
        if key != self._key or verts.total > self.capacity:
            return None
        static = self._static
        for k, v in rect.items():
            static[k].copy_(v, non_blocking=True)
        total = verts.total
        static["verts_src"].packed[:total].copy_(verts.packed[:total], non_blocking=True)
        static["verts_src"].offsets.copy_(verts.offsets, non_blocking=True)
        self.replays += 1
        surf, pred = self._step()
        return surf.clone(), pred.packed[:total].clone()      # (the replay overwrites its outputs: the caller keeps its own)

    @torch.no_grad()
    def __call__(self, model, data_dict, config, compute_loss=False):
        verts = as_ragged(data_dict["verts_src"])
        counts, total = verts.counts, verts.total
        ragged_surface = any(isinstance(data_dict.get(k), RaggedPoints) for k in self.RECT_INPUTS)
        out = self._replayed(model, data_dict, verts, config) if (self.graph and not ragged_surface) else None
        if out is None:
            self.eager_calls += 1
            tight = verts if verts.capacity == total else RaggedPoints(verts.packed[:total].contiguous(), verts.offsets, counts)
            dd = dict(data_dict)
            dd["verts_src"] = tight
            surf, pred = self._run(model, dd, config)
            out = surf, pred.packed
        data_dict["surface_samples_tgt_pred"] = out[0]
        data_dict["verts_tgt_pred"] = RaggedPoints(out[1], verts.offsets, counts)
        if compute_loss:
            loss = l2_error(data_dict["verts_tgt_pred"], as_ragged(data_dict["verts_tgt"])).item()
        else:
            loss = 0.0
        return loss, data_dict

    def close(self):
        if self._step is not None:
            self._step.close()
        self._step = self._static = self._key = None
