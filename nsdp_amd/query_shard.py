"""Dense inference split over GPUs by query point: one shape, N ranks.

Every shipped config decodes one shape per call (``test.batch_size: 1``), so sharding by shape leaves N - 1 GPUs idle.  Here
every rank encodes the SAME shapes (replicated: the encoder is deterministic, its output is bit-identical on every rank, no
collective) and decodes a contiguous slice of the query points; one all-gather puts the slices back together on every rank.

    shards = QueryShards(rank, world)                               # after dist.init_process_group
    step = query_sharded(test_on_batch, shards)                     # test_on_batch_with_cano / _with_arbitrary
    loss, data_dict = step(model, data_dict, config)                # the reference's signature; same predictions on every rank

Bit-identical to the single-process call: the fp32 inference decoder is one anchor kNN (one lane per query) and one fused kernel
in which a query's outputs depend on its own row alone (ragged tail lanes are clamped to the last valid query and not stored), so
a query decoded in a slice gets the bits it gets in the whole set.  bf16 storage decodes through the layered kernels, whose tile
shapes follow the row count: not supported here.
"""
from __future__ import annotations

import torch
import torch.distributed as dist


class QueryShards:
    """Rank ``rank`` of ``world`` decodes the contiguous query range ``bounds(nq)``; ``gather`` reassembles the whole set."""

    def __init__(self, rank: int, world: int, group=None):
        if not 0 <= int(rank) < int(world):
            raise ValueError(f"QueryShards: rank {rank} outside a world of {world}")
        self.rank, self.world, self.group = int(rank), int(world), group
        self.list_form = False          # (the last gather used the list-form all_gather: gloo and device tensors)

    def chunk(self, nq: int) -> int:
        """Rows every rank sends: ceil(nq / world)."""
        return -(-int(nq) // self.world)

    def bounds(self, nq: int):
        """(lo, hi) of this rank: contiguous, disjoint, in rank order, covering [0, nq).  Only the last ranks are short or empty
        -- the padding sits at the global tail, so the reassembly is one copy."""
        m = self.chunk(nq)
        return min(nq, self.rank * m), min(nq, (self.rank + 1) * m)

    def local(self, points: torch.Tensor) -> torch.Tensor:
        """This rank's rows of ``points`` [B, N, C] (contiguous: the decoder's input)."""
        lo, hi = self.bounds(points.shape[1])
        return points[:, lo:hi].contiguous()

    def gather(self, local: torch.Tensor, nq: int) -> torch.Tensor:
        """[B, hi - lo, C] of every rank -> [B, nq, C] on every rank: one all-gather of [B, ceil(nq / world), C] chunks, no host
        synchronisation (RCCL).  ``world == 1``: the identity."""
        lo, hi = self.bounds(nq)
        if local.dim() != 3 or local.shape[1] != hi - lo:
            raise ValueError(f"QueryShards.gather: rank {self.rank} holds rows [{lo}, {hi}) of {nq}, got {tuple(local.shape)}")
        if self.world == 1:
            return local
        B, _, C = local.shape
        m = self.chunk(nq)
        if m == 0:
            return local.new_empty((B, 0, C))
        send = local.contiguous()
        if hi - lo < m:
            send = torch.cat([send, send.new_zeros((B, m - (hi - lo), C))], dim=1)
        buf = send.new_empty((self.world, B, m, C))
        self.exchange(buf, send)
        # (the copy that reassembles the ranks' chunks; a second one drops the tail padding when there is any)
        return buf.permute(1, 0, 2, 3).reshape(B, self.world * m, C)[:, :nq].contiguous()

    def exchange(self, buf: torch.Tensor, send: torch.Tensor):
        """buf[r] = rank r's ``send`` [B, m, C] for every rank r (buf [world, B, m, C]), one collective.  The form follows from the
        backend and the tensor alone, so every rank picks the same one before anything is exchanged: all_gather_into_tensor
        (RCCL, and gloo with host tensors) into buf seen as the ranks' chunks concatenated along dim 0, [world * B, m, C];
        the list-form all_gather into buf's rows for device tensors under gloo."""
        self.list_form = send.is_cuda and dist.get_backend(self.group) == "gloo"
        if self.list_form:
            dist.all_gather(list(buf.unbind(0)), send, group=self.group)
        else:
            dist.all_gather_into_tensor(buf.view(-1, *send.shape[1:]), send, group=self.group)


def require_supported(net=None):
    """The sharded decode needs the encode / decode split and, for this library's networks, the fused fp32 decoder: the one
    decode whose rows are independent of each other.  The layered kernels (bf16 storage, NSDP_FUSED_DECODER=0, a decoder
    geometry the fused kernel was not built for) choose tile shapes from the row count -- bit equality with the unsharded call
    is not established there, so they are refused.  A network of the caller's own (``encode`` / ``decode`` duck-typed, not a
    Deformation_Networks) is taken to decode every query row on its own."""
    from . import hip_decoder, precision
    from .model import deformation_networks
    from .model.decoder.crosstransformer_decoder import CrossTransformerDecoder
    if not deformation_networks.ENCODE_ONCE:
        raise RuntimeError("query sharding encodes once per shape and decodes slices: it needs the encode / decode split, "
                           "which NSDP_ENCODE_ONCE=0 switches off")
    if precision.is_bf16():
        raise NotImplementedError("query sharding in bf16 storage: the layered decoder's tile shapes follow the row count, "
                                  "bit equality with the unsharded call is not established")
    if isinstance(net, deformation_networks.Deformation_Networks):
        dec = net.decoder
        if not (hip_decoder.ENABLED and isinstance(dec, CrossTransformerDecoder) and hip_decoder.supported(dec)):
            raise NotImplementedError("query sharding needs the fused fp32 decoder (NSDP_FUSED_DECODER=1, dim 200, hidden 128, "
                                      "5 blocks, 3 outputs): the layered kernels' tile shapes follow the row count, bit equality "
                                      "with the unsharded call is not established")


def decode_local(net, points: torch.Tensor, encoding: dict, shards: QueryShards) -> torch.Tensor:
    """``net.decode`` of this rank's slice of ``points`` (an empty slice decodes to [B, 0, C])."""
    require_supported(net)
    return net.decode(shards.local(points), encoding)


@torch.no_grad()
def decode_sharded(net, points: torch.Tensor, encoding: dict, shards: QueryShards) -> torch.Tensor:
    """``net.decode(points, encoding)`` with the query points split over the ranks: every rank passes the same ``points`` and
    ``encoding`` (replicated) and receives the whole [B, N, C] result.  For query sets other than the step functions' own."""
    return shards.gather(decode_local(net, points, encoding, shards), points.shape[1])


# ---- the reference's dense-inference step functions, sharded ------------------------------------------------------------
# Each local form returns {data_dict key: (this rank's rows, total rows)}; it enqueues GPU work only (capturable) and reads the
# data_dict entries named in its ``inputs`` -- nothing else (a replay copies exactly those into its static tensors).

def _local_with_cano(model, data_dict, shards):
    """test_on_batch_with_cano (reference model/deformation_networks.py:90-109): one encoder pass, two query sets."""
    require_supported(model)
    encoding = model.encode(data_dict["surface_samples_inputs"])
    surf, verts = data_dict["surface_samples_src"], data_dict["verts_src"]
    return {"surface_samples_tgt_pred": (decode_local(model, surf, encoding, shards), surf.shape[1]),
            "verts_tgt_pred": (decode_local(model, verts, encoding, shards), verts.shape[1])}


def _local_with_arbitrary(model, data_dict, shards):
    """test_on_batch_with_arbitrary (reference model/flow_arbitrary.py:65-85).  Network 2's encoder reads the WHOLE
    canonicalised surface, so network 1 decodes the whole surface plus this rank's vertices (one encode, one decode over the
    concatenation, as the unsharded call); network 2 decodes this rank's slices of both."""
    from .model.flow_arbitrary import _split
    net = model.model_deform
    require_supported(model.model_canonicalize)
    require_supported(net)
    src, tgt, mask = _split(data_dict)
    verts = data_dict["verts_src"]
    surf2cano, verts2cano = model.canonicalize([src, shards.local(verts)], src)
    encoding = net.encode(model.deform_input(surf2cano, tgt, mask))
    return {"surface_samples_tgt_pred": (decode_local(net, surf2cano, encoding, shards), surf2cano.shape[1]),
            "verts_tgt_pred": (net.decode(verts2cano.contiguous(), encoding), verts.shape[1])}


_local_with_cano.inputs = ("surface_samples_inputs", "surface_samples_src", "verts_src")
_local_with_arbitrary.inputs = ("surface_samples_inputs", "verts_src")


def _local_form(test_on_batch):
    from .model.deformation_networks import test_on_batch_with_cano
    from .model.flow_arbitrary import test_on_batch_with_arbitrary
    forms = {test_on_batch_with_cano: _local_with_cano, test_on_batch_with_arbitrary: _local_with_arbitrary}
    if test_on_batch not in forms:
        raise TypeError(f"query_sharded: no sharded form of {getattr(test_on_batch, '__name__', test_on_batch)} "
                        "(test_on_batch_with_cano and test_on_batch_with_arbitrary have one)")
    return forms[test_on_batch]


def _refuse_ragged(data_dict):
    from .ragged import RaggedPoints
    if isinstance(data_dict.get("verts_src"), RaggedPoints):
        raise NotImplementedError("query_sharded: splitting a ragged (packed) vertex set over ranks is not implemented -- "
                                  "decode it on one GPU (ragged.RaggedTestOnBatch) or pad the batch to a [B, max, 3] tensor")
    if any(isinstance(data_dict.get(k), RaggedPoints) for k in ("surface_samples_inputs", "surface_samples_src")):
        raise NotImplementedError("query_sharded: ragged (packed) surface clouds are not split over ranks -- run the step on one GPU")


class QueryShardedTestOnBatch:
    """``fn(model, data_dict, config, compute_loss=False) -> (loss, data_dict)`` with the query points split over the ranks
    (see ``query_sharded``).  ``graph=True``: the first call captures this rank's encode and local decode
    (graph_step.GraphedStep over frozen weights: the model must be in eval mode and its weights must not change afterwards)
    over static copies of the inputs it reads; every call whose inputs have the same shapes is a copy into them plus one replay
    (``replays``), and the gather runs eagerly behind it -- a collective cannot be captured.  Calls with other shapes run
    eagerly (``eager_calls``)."""

    def __init__(self, test_on_batch, shards: QueryShards, graph: bool = False, max_streams=None):
        self.local_fn = _local_form(test_on_batch)
        require_supported()
        self.shards, self.graph, self.max_streams = shards, bool(graph), max_streams
        self._step = self._static = self._key = None
        self.replays = self.eager_calls = 0

    def local(self, model, data_dict):
        """This rank's predictions, {key: (rows, total rows)}: enqueued on the current stream, nothing gathered."""
        require_supported()
        _refuse_ragged(data_dict)
        with torch.no_grad():
            return self.local_fn(model, data_dict, self.shards)

    def _replayed(self, model, data_dict):
        # (the key and the static copies cover the local form's inputs only: the predictions this call writes back into the
        # caller's dict, the targets and anything else in it neither decide the replay nor travel into the graph's buffers)
        inputs = {k: data_dict[k] for k in self.local_fn.inputs}
        key = (id(model), tuple((k, tuple(v.shape), v.dtype, v.device) for k, v in inputs.items()))
        if self._step is None:
            if model.training:
                raise ValueError("query_sharded(graph=True) replays frozen-weight inference: call model.eval() first")
            from .graph_step import GraphedStep
            self._key = key
            self._static = {k: v.clone() for k, v in inputs.items()}
            self._step = GraphedStep(lambda: self.local(model, self._static), self.max_streams,
                                     weights_change=False).capture(warmup=1)
        elif key != self._key:
            self.eager_calls += 1
            return self.local(model, data_dict)
        for k, v in self._static.items():
            v.copy_(inputs[k], non_blocking=True)
        self.replays += 1
        out = self._step()
        # (the replay overwrites its outputs: the caller keeps tensors of its own -- the gather makes them at world > 1)
        return out if self.shards.world > 1 else {k: (t.clone(), n) for k, (t, n) in out.items()}

    @torch.no_grad()
    def __call__(self, model, data_dict, config, compute_loss=False):
        from .model.utils import compute_l2_error
        _refuse_ragged(data_dict)
        if self.graph:
            local = self._replayed(model, data_dict)
        else:
            self.eager_calls += 1
            local = self.local(model, data_dict)
        for k, (t, n) in local.items():
            data_dict[k] = self.shards.gather(t, n)
        if compute_loss:
            loss = compute_l2_error(data_dict["verts_tgt_pred"], data_dict["verts_tgt"])
        else:
            loss = torch.zeros((1), dtype=torch.float32)
        return loss.item(), data_dict

    def close(self):
        if self._step is not None:
            self._step.close()
        self._step = self._static = self._key = None


def query_sharded(test_on_batch, shards: QueryShards, graph: bool = False, max_streams=None):
    """The reference-shaped dense-inference step ``test_on_batch(model, data_dict, config, compute_loss=False)`` with its query
    points (surface samples and mesh vertices) split over ``shards.world`` ranks: every rank encodes the shapes, decodes its
    slices and all-gathers the predictions -- ``data_dict['surface_samples_tgt_pred']``, ``data_dict['verts_tgt_pred']`` and the
    loss are the same on every rank and bit-identical to the unsharded call.  Every rank must pass the same batch."""
    return QueryShardedTestOnBatch(test_on_batch, shards, graph=graph, max_streams=max_streams)
