"""Editing session: drag handles on a mesh without re-encoding its source.

    python -m nsdp_amd.edit CONFIG [--vertices N] [--surface N] [--batch B] [--part P --translate dx,dy,dz] [--drags K]
                                   [--graph] [--weight_file F] [--out DIR]
    python -m nsdp_amd.edit CONFIG --vertex-counts n1,n2,... [--surface-counts s1,s2,... | --surface N] [--graph] ...

The reference's interactive editing (run.py, "Interactive Editing / Run-batch-processing"; config/tosca/*.yaml,
config/dogrec/*.yaml; dataset/dataset_userhandle_flow.py) takes one mesh, marks head, tail and feet as handles by a bounding-box
rule (dataset/utils.py: cano_handle_user_define), translates one of them and lets FlowArbitrary deform every vertex -- one whole
``test_on_batch_with_arbitrary`` per drag.  Most of that call does not depend on the drag:

  * network 1 (model_canonicalize) reads the source pose alone: its encoder and its decodes of the cloud and of the vertices;
  * network 2's geometry -- farthest-point sampling, every k-NN set of the pyramid, the final blocks' neighbours, each query's
    nearest anchors -- derives from columns 0:3 of its input, the canonicalised cloud.  A drag changes columns 3:7 only;
  * when the cloud IS the vertex set (the reference's user-handle data set), the second decode repeats the first: the decoder
    treats query rows independently.

An ``EditSession`` computes those once per source mesh and runs, per drag, the handle kernel (include/nsdp_handles.h),
network 2's encoder over cached index sets and one decode (two when the cloud is a separate set):

    s = EditSession(model, verts_src)                    # FlowArbitrary in eval mode, verts_src [B, V, 3] on the GPU
    out = s.drag(part="head", translation=(-0.15, -0.2, -0.2))
    out = s.drag(handle_mask=h, move_mask=m, translation=(0, 0, 0.1))
    s.close()

The drag parameters are read by the kernel from a [B, 8] device tensor, so with ``graph=True`` ONE captured graph (graph_step.
GraphedStep over frozen weights) replays every drag by rule: a drag is one small host-to-device copy and a replay.  A drag by
explicit masks launches the kernel's mask form -- other kernel arguments -- and is a second capture, made at the first such
drag; the two graphs share the session's buffers.

Staleness.  A session is valid for the WEIGHTS and the SOURCE it was opened with: it holds network 1's outputs, network 2's
index sets and (``graph=True``) graphs that froze the weight packs.  After ``load_state_dict`` or any other change of the
parameters call ``reopen()``; for another mesh open another session.

A batch of meshes of DIFFERENT vertex counts -- the reference's batch loop over its user-handle data set, where the cloud is each
mesh's own vertex set -- goes through a ``RaggedEditSession`` over packed sets (nsdp_amd.ragged, include/nsdp_handles_ragged.h):

    s = RaggedEditSession(model, RaggedPoints.from_list([v0, v1, v2]))
    out = s.drag(part=["head", "tail", "head"], translation=(-0.15, -0.2, -0.2))      # RaggedPoints come back

Every stage of a drag is the kernel the step function runs, on the same operands: the predictions are bit-equal to
``test_on_batch_with_arbitrary`` (``test_on_batch_with_cano`` for a single network) on the data_dict the drag stands for
(tests/test_edit_session_gpu.py, tests/test_edit_session_ragged_gpu.py).
"""
from __future__ import annotations

import argparse
import json
import os
import sys
from dataclasses import dataclass

PARTS = ("head", "tail", "frontleftfoot", "frontrightfoot", "behindleftfoot", "behindrightfoot")      # the reference's priority
SEED_DATA, SEED_WEIGHTS = 1000, 2048      # (nsdp_amd.infer's)


@dataclass(frozen=True)
class HandleSpec:
    """One drag of the bounding-box rule: which region moves, by how much, and the rule's two settings."""
    part: str
    translation: tuple
    partial_range: float = 0.1
    cliptail: bool = False

    def __post_init__(self):
        if self.part not in PARTS:
            raise ValueError(f"HandleSpec: part must be one of {PARTS}, got {self.part!r}")
        if len(self.translation) != 3:
            raise ValueError(f"HandleSpec: translation is (dx, dy, dz), got {self.translation!r}")

    @classmethod
    def from_config(cls, data_cfg):
        """From the ``data`` block of a reference user-handle config (config/tosca/head.yaml ...): the first of head, tail,
        frontleftfoot, frontrightfoot, behindleftfoot, behindrightfoot that is set -- the reference's if / elif chain -- moves by
        (xtrans, ytrans, ztrans).  No part set: ValueError (the reference fails on an unbound name there)."""
        if not isinstance(data_cfg, dict) or not isinstance(data_cfg.get("userhandle"), dict):
            raise ValueError("HandleSpec.from_config: the config's data block has no `userhandle` section")
        uh = data_cfg["userhandle"]
        part = next((p for p in PARTS if uh.get(p)), None)
        if part is None:
            raise ValueError(f"HandleSpec.from_config: none of {PARTS} is set in data.userhandle -- nothing to move")
        return cls(part=part, translation=tuple(float(uh.get(k, 0.0)) for k in ("xtrans", "ytrans", "ztrans")),
                   partial_range=float(data_cfg.get("partial_range", 0.1)), cliptail=bool(uh.get("cliptail", False)))


def pack_params(B, part, translation, partial_range, cliptail):
    """The [B, 8] int32 host array nsdp_handle_rows reads (include/nsdp_handles.h): ``part`` a name / index or one per shape,
    ``translation`` (dx, dy, dz) or [B, 3], ``partial_range`` and ``cliptail`` scalars or one per shape."""
    import numpy as np
    words = np.zeros((B, 8), dtype=np.int32)
    parts = [part] * B if isinstance(part, (str, int)) else list(part)
    if len(parts) != B:
        raise ValueError(f"drag: {len(parts)} parts for {B} shapes")
    for b, p in enumerate(parts):
        if isinstance(p, str):
            if p not in PARTS:
                raise ValueError(f"drag: part must be one of {PARTS}, got {p!r}")
            p = PARTS.index(p)
        if not 0 <= int(p) < len(PARTS):
            raise ValueError(f"drag: part index {p} outside 0..{len(PARTS) - 1}")
        words[b, 0] = int(p)
    d = np.asarray(translation, dtype=np.float32)
    if d.shape not in ((3,), (B, 3)):
        raise ValueError(f"drag: translation must be (dx, dy, dz) or [{B}, 3], got shape {d.shape}")
    words[:, 1] = np.broadcast_to(np.asarray(cliptail, dtype=bool), (B,)).astype(np.int32)
    f = words.view(np.float32)
    f[:, 2] = np.broadcast_to(np.asarray(partial_range, dtype=np.float32), (B,))
    f[:, 3:6] = np.broadcast_to(d, (B, 3))
    return words


def _networks_or_refusal(model):
    """The reasons that depend on the model alone -- its type, training mode, autograd -- as a string; without one, the list of
    the model's networks, the deformation network last."""
    import torch
    from .model.deformation_networks import Deformation_Networks
    from .model.flow_arbitrary import FlowArbitrary
    if isinstance(model, FlowArbitrary):
        nets = [model.model_canonicalize, model.model_deform]
    elif isinstance(model, Deformation_Networks):
        nets = [model]
    else:
        return f"the model must be a FlowArbitrary or a Deformation_Networks, got {type(model).__name__}"
    if model.training or any(m.training for m in model.modules()):
        return ("the model is in training mode: a session caches network 1's outputs and replays frozen weights, BatchNorm "
                "would take batch statistics -- call model.eval() first")
    if torch.is_grad_enabled():
        return ("autograd is enabled: a session runs the inference kernels over cached tensors and records no graph -- open it "
                "and drag under torch.no_grad()")
    return nets


def _network_refusal(net2, encoder_needs):
    """The reasons that depend on the storage type and the deformation network; ``encoder_needs``: the methods of its encoder
    the session's layout calls."""
    from . import precision
    if precision.is_bf16():
        return "bf16 storage (NSDP_STORAGE=bf16): the session is built and tested in fp32 storage only"
    if net2.no_input_corr:
        return "this network does not read the handle columns (no_input_corr: a backward-type network): a drag would change nothing"
    if not (all(hasattr(net2.encoder, m) for m in encoder_needs) and hasattr(net2.decoder, "geometry")):
        return (f"the {type(net2.encoder).__name__} / {type(net2.decoder).__name__} pair has no geometry(): it searches inside "
                "its forward pass only, so its index sets cannot be cached across drags")
    return None


def refusal(model, verts_src, surface=None, cano=None, surface_cano=None):
    """Why a session cannot be opened on these arguments (None: it can), each reason named."""
    import torch
    from .ragged import RaggedPoints
    nets = _networks_or_refusal(model)
    if isinstance(nets, str):
        return nets
    given = {"verts_src": verts_src, "surface": surface, "cano": cano, "surface_cano": surface_cano}
    for name, t in given.items():
        if isinstance(t, RaggedPoints):
            return (f"ragged inputs: {name} is a RaggedPoints -- an EditSession holds one rectangular [B, n, 3] set per role; "
                    "RaggedEditSession takes a packed batch of meshes of different sizes")
    why = _network_refusal(nets[-1], ("geometry",))
    if why is not None:
        return why
    for name, t in given.items():
        if t is None:
            continue
        if not torch.is_tensor(t):
            return f"{name} must be a torch.Tensor, got {type(t).__name__}"
        if t.dtype is not torch.float32 or t.dim() != 3 or t.shape[2] != 3:
            return f"{name} must be float32 [B, n, 3], got {t.dtype} {tuple(t.shape)}"
        if not t.is_cuda:
            return f"CPU tensors: {name} is on the CPU -- the session's kernels have no CPU path"
    B = verts_src.shape[0]
    if surface is not None and surface.shape[0] != B:
        return f"surface holds {surface.shape[0]} shapes, verts_src {B}"
    if cano is not None and cano.shape != verts_src.shape:
        return f"cano {tuple(cano.shape)} is not shaped like verts_src {tuple(verts_src.shape)}"
    if surface_cano is not None and (surface is None or surface_cano.shape != surface.shape):
        return "surface_cano goes with a surface of the same shape"
    return None


class _Session:
    """What an editing session is in either layout: the checks at open, the bookkeeping, one drag up to its dispatch -- the
    parameter copy, the mask buffers, capture or eager by (masks, vert_masks) -- and the end.  A layout (EditSession: rectangular
    sets; RaggedEditSession: packed ones) gives

      _refusal(model, verts_src, surface, cano, surface_cano)   why a session cannot be opened on these (None: it can);
      _hold(verts_src, surface, cano, surface_cano)             keeps the sets as it wants them, contiguous;
      _open()                                                   computes everything cached per source and weights;
      _layout()                                                 (B, the tensor that names the device, the shape of a mask over
                                                                the cloud, of one over the vertices);
      _enqueue(masks, vert_masks)                               the GPU work of a drag behind the copies;
      _result(pred, own, own_pred, have_verts, with_inputs)     the dict a drag returns;
      _cached                                                   the attributes close() lets go of."""

    def __init__(self, model, verts_src, surface=None, cano=None, surface_cano=None, partial_range=0.1, cliptail=False,
                 graph=False, max_streams=None):
        why = self._refusal(model, verts_src, surface, cano, surface_cano)
        if why is not None:
            raise ValueError(self._refused + why)
        from . import query_shard
        from .model.flow_arbitrary import FlowArbitrary
        self.model = model
        self.flow = isinstance(model, FlowArbitrary)
        self.net = model.model_deform if self.flow else model
        # one decode standing for two, and network 1 decoding one set where the step function decodes the concatenation: both
        # rest on the decoder treating every query row on its own -- the fused fp32 decoder (query_shard names what is not)
        for net in ([model.model_canonicalize, self.net] if self.flow else [self.net]):
            query_shard.require_supported(net)
        self._hold(verts_src, surface, cano, surface_cano)
        self.partial_range, self.cliptail = float(partial_range), bool(cliptail)
        self.graph, self.max_streams = bool(graph), max_streams
        self.replays = self.eager_calls = 0
        self._steps = {}
        self._open()

    @property
    def _refused(self):
        return type(self).__name__ + " refused: "

    def reopen(self):
        """Recompute everything the session caches (after the weights changed) and drop the captured graphs."""
        why = self._refusal(self.model, self.verts, None if self.same else self.surface)
        if why is not None:
            raise ValueError(self._refused + why)
        self._drop_graphs()
        self._open()
        return self

    # ------------------------------------------------------------------ one drag
    def _mask_buffer(self, name, like_rows, value, device):
        import torch
        buf = getattr(self, name)
        if buf is None:
            buf = torch.empty(like_rows, dtype=torch.uint8, device=device)
            setattr(self, name, buf)
        if not torch.is_tensor(value) or not value.is_cuda:
            raise ValueError(self._refused + "CPU tensors: the masks of a drag must be GPU tensors")
        if value.dtype not in (torch.bool, torch.uint8) or tuple(value.shape) != tuple(like_rows):
            raise ValueError(f"drag: a mask must be bool / uint8 {tuple(like_rows)}, got {value.dtype} {tuple(value.shape)}")
        buf.copy_(value, non_blocking=True)

    def drag(self, part=None, translation=(0.0, 0.0, 0.0), handle_mask=None, move_mask=None, vert_handle_mask=None,
             vert_move_mask=None, partial_range=None, cliptail=None, with_inputs=False, clone=True):
        """One drag of every shape.  By rule: ``part`` (a name of PARTS, one per shape, or a HandleSpec) moves by ``translation``
        ((dx, dy, dz) or [B, 3]).  By explicit regions: ``handle_mask`` / ``move_mask`` over the cloud (bool / uint8 on the GPU:
        [B, n] for a rectangular cloud, (scap,) for a packed one) replace the rule; with a separate cloud ``vert_handle_mask`` /
        ``vert_move_mask`` ([B, V], packed (cap,)) do so for the vertices (without them ``verts_tgt`` and
        ``cano_handle_vert_idx`` are None).

        Returns ``verts_tgt_pred``, ``surface_samples_tgt_pred``, ``verts_tgt``, ``cano_handle_vert_idx`` and
        ``cano_handle_sample_idx``, and with ``with_inputs`` ``surface_samples_inputs`` = [src | mask * tgt | mask], what the step
        function takes as it is -- shaped as the session's ``_result`` says.  The tensors are the caller's own; ``clone=False``
        hands out the session's buffers, overwritten by the next drag."""
        import torch
        from ._lib import on_device
        if torch.is_grad_enabled():
            raise ValueError(self._refused + "autograd is enabled -- drag under torch.no_grad()")
        if self.model.training:
            raise ValueError(self._refused + "the model is in training mode -- call model.eval() (and reopen() if the weights "
                             "changed)")
        if isinstance(part, HandleSpec):
            spec, part, translation = part, part.part, part.translation
            partial_range = spec.partial_range if partial_range is None else partial_range
            cliptail = spec.cliptail if cliptail is None else cliptail
        masks = handle_mask is not None or move_mask is not None
        B, on, cloud_rows, vert_rows = self._layout()
        if masks:
            if handle_mask is None or move_mask is None or part is not None:
                raise ValueError("drag: handle_mask and move_mask go together and replace `part`")
            if (vert_handle_mask is None) != (vert_move_mask is None) or (self.same and vert_handle_mask is not None):
                raise ValueError("drag: vert_handle_mask and vert_move_mask go together, with a separate cloud only")
            part = 0
        elif part is None:
            raise ValueError(f"drag: name the part that moves (one of {PARTS}) or give handle_mask and move_mask")
        elif vert_handle_mask is not None or vert_move_mask is not None:
            raise ValueError("drag: vertex masks go with handle_mask and move_mask")
        vert_masks = masks and vert_handle_mask is not None
        words = pack_params(B, part, translation, self.partial_range if partial_range is None else partial_range,
                            self.cliptail if cliptail is None else cliptail)
        with on_device(on):
            # the one host-to-device copy of a drag, stream-ordered in front of the kernels that read it (pageable memory: the
            # runtime has taken the bytes when copy_ returns, so the host array is free at once)
            self.params.copy_(torch.from_numpy(words), non_blocking=True)
            if masks:
                self._mask_buffer("_mask_h", cloud_rows, handle_mask, on.device)
                self._mask_buffer("_mask_m", cloud_rows, move_mask, on.device)
                if vert_masks:
                    self._mask_buffer("_vmask_h", vert_rows, vert_handle_mask, on.device)
                    self._mask_buffer("_vmask_m", vert_rows, vert_move_mask, on.device)
            key = (masks, vert_masks)
            if self.graph:
                if key not in self._steps:
                    from .graph_step import GraphedStep
                    self._steps[key] = GraphedStep(lambda: self._enqueue(*key), self.max_streams,
                                                   weights_change=False).capture(warmup=1)
                self.replays += 1
                pred = self._steps[key]()
            else:
                self.eager_calls += 1
                pred = self._enqueue(*key)
            own = (lambda t: t.clone()) if clone else (lambda t: t)      # the session's buffers: the next drag overwrites them
            own_pred = own if self.graph else (lambda t: t)              # (an eager drag's predictions are fresh tensors)
            return self._result(pred, own, own_pred, self.same or not masks or vert_masks, with_inputs)

    # ------------------------------------------------------------------ the end
    def _drop_graphs(self):
        for step in self._steps.values():
            step.close()
        self._steps = {}

    def close(self):
        self._drop_graphs()
        for name in self._cached:
            setattr(self, name, None)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


class EditSession(_Session):
    """See the module text.  ``verts_src`` [B, V, 3] fp32 on the GPU; ``surface`` [B, S, 3]: the cloud network 2 encodes (None:
    the vertex set itself, as in the reference's user-handle data set); ``cano`` / ``surface_cano``: the coordinates the
    bounding-box rule is evaluated on (None: the source coordinates -- what the reference does, every frame of its pairs being
    frame 0000).  ``partial_range`` / ``cliptail``: the rule's settings, defaults of every drag.

    ``model``: a FlowArbitrary in eval mode, or one Deformation_Networks of the forward type (no network 1: canonical = source,
    only the index sets are cached).

    ``graph=True``: the first drag captures everything behind the parameter copy; later drags are copy + replay (``replays``;
    ``eager_calls`` counts drags run op by op)."""

    _refusal = staticmethod(refusal)
    _cached = ("geometry", "buf", "_surf_idx")

    def _hold(self, verts_src, surface, cano, surface_cano):
        self.verts = verts_src.contiguous()
        self.same = surface is None
        self.surface = self.verts if self.same else surface.contiguous()
        self.verts_rule = self.verts if cano is None else cano.contiguous()
        self.surface_rule = (self.verts_rule if self.same else self.surface) if surface_cano is None else surface_cano.contiguous()

    def _layout(self):
        return self.verts.shape[0], self.verts, tuple(self.surface.shape[:2]), tuple(self.verts.shape[:2])

    # ------------------------------------------------------------------ the cached state
    def _open(self):
        import torch
        from . import pointnet2_utils as pu
        with torch.no_grad():
            dev = self.verts.device
            B, V, S = self.verts.shape[0], self.verts.shape[1], self.surface.shape[1]
            if self.flow:
                sets = [self.surface] if self.same else [self.surface, self.verts]
                outs = self.model.canonicalize(sets, self.surface)
                self.surf2cano, self.verts2cano = outs[0].contiguous(), outs[-1].contiguous()
            else:
                self.surf2cano, self.verts2cano = self.surface, self.verts
            # the deformation network's input rows: columns 0:3 written here, once; 3:7 by every drag's kernel
            self.buf = torch.zeros((B, S, 7), dtype=torch.float32, device=dev)
            self.buf[:, :, 0:3] = self.surf2cano
            self.geometry = self.net.geometry(self.verts2cano, self.buf)
            self._surf_idx = None if self.same else self.net.decoder.geometry(self.surf2cano, self.geometry["encoder"]["anchors"])["query_idx"]
            self.bounds = pu.handle_bounds(self.surface_rule)
            self.verts_bounds = self.bounds if self.same else pu.handle_bounds(self.verts_rule)
            self.params = torch.zeros((B, 8), dtype=torch.int32, device=dev)
            self.surface_tgt = torch.empty((B, S, 3), dtype=torch.float32, device=dev)
            self.surface_handle = torch.empty((B, S), dtype=torch.uint8, device=dev)
            self._mask_h = self._mask_m = self._vmask_h = self._vmask_m = None      # (made by the first drag by masks)
            if self.same:
                self.verts_tgt, self.verts_handle, self._vrows = self.surface_tgt, self.surface_handle, None
            else:
                self.verts_tgt = torch.empty((B, V, 3), dtype=torch.float32, device=dev)
                self.verts_handle = torch.empty((B, V), dtype=torch.uint8, device=dev)
                self._vrows = torch.empty((B, V, 7), dtype=torch.float32, device=dev)      # (the kernel's required output)

    # ------------------------------------------------------------------ one drag
    def _enqueue(self, masks, vert_masks):
        """Everything of a drag that runs on the GPU behind the parameter copy: capturable, reads device tensors only."""
        from . import pointnet2_utils as pu
        net = self.net
        hm, mm = (self._mask_h, self._mask_m) if masks else (None, None)
        pu.handle_rows(self.surface_rule, self.surface, self.bounds, self.params, self.buf, hm, mm, tgt=self.surface_tgt,
                       handle_out=self.surface_handle)
        if not self.same and (not masks or vert_masks):
            vh, vm = (self._vmask_h, self._vmask_m) if masks else (None, None)
            pu.handle_rows(self.verts_rule, self.verts, self.verts_bounds, self.params, self._vrows, vh, vm, tgt=self.verts_tgt,
                           handle_out=self.verts_handle)
        enc = net.encode(self.buf, geometry=self.geometry)
        out = {"verts_tgt_pred": net.decode(self.verts2cano, enc)}
        if not self.same:
            enc_s = dict(enc)
            enc_s["query_idx"], enc_s["query_points"] = self._surf_idx, self.surf2cano
            out["surface_samples_tgt_pred"] = net.decode(self.surf2cano, enc_s)
        return out

    def _result(self, pred, own, own_pred, have_verts, with_inputs):
        """``verts_tgt_pred`` [B, V, 3], ``surface_samples_tgt_pred`` [B, S, 3], ``verts_tgt``, ``cano_handle_vert_idx`` and
        ``cano_handle_sample_idx`` (bool), and with ``with_inputs`` the reference-shaped ``surface_samples_inputs`` [B, S, 7]
        = [src | mask * tgt | mask] (what test_on_batch_with_arbitrary and eval_metric take)."""
        import torch
        out = {"verts_tgt_pred": own_pred(pred["verts_tgt_pred"])}
        out["surface_samples_tgt_pred"] = (out["verts_tgt_pred"] if self.same
                                           else own_pred(pred["surface_samples_tgt_pred"]))
        out["verts_tgt"] = own(self.verts_tgt) if have_verts else None
        out["cano_handle_vert_idx"] = own(self.verts_handle).view(torch.bool) if have_verts else None
        out["cano_handle_sample_idx"] = (out["cano_handle_vert_idx"] if self.same
                                         else own(self.surface_handle).view(torch.bool))
        if with_inputs:
            out["surface_samples_inputs"] = torch.cat([self.surface, self.buf[:, :, 3:7]], dim=-1)
        return out


# ------------------------------------------------------------------------------------------- a packed batch of different meshes
def ragged_refusal(model, verts_src, surface=None, cano=None, surface_cano=None):
    """Why a RaggedEditSession cannot be opened on these arguments (None: it can), each reason named."""
    import torch
    from . import hip_decoder
    from .ragged import RaggedPoints
    nets = _networks_or_refusal(model)
    if isinstance(nets, str):
        return nets
    if not isinstance(verts_src, RaggedPoints):
        return (f"verts_src must be a RaggedPoints (B meshes packed), got {type(verts_src).__name__} -- EditSession takes a "
                "rectangular [B, V, 3] tensor")
    given = {"verts_src": verts_src, "surface": surface, "cano": cano, "surface_cano": surface_cano}
    for name, t in given.items():
        if (isinstance(t, RaggedPoints) or torch.is_tensor(t)) and not t.is_cuda:
            return f"CPU tensors: {name} is on the CPU -- the session's kernels have no CPU path"
    why = _network_refusal(nets[-1], ("geometry", "ragged_geometry"))
    if why is not None:
        return why
    for net in nets:      # (what encoding a packed cloud and decoding a packed query set refuse, by their own names)
        why = net.ragged_surface_refusal() if isinstance(surface, RaggedPoints) or surface is None else (
            hip_decoder.ragged_refusal(net.decoder) if hip_decoder.supported(net.decoder) else
            "decoder geometry: the packed vertices are decoded by the fused kernels, built for dim=200, hidden_dim=128, "
            "n_blocks=5, out_dim=3")
        if why is not None:
            return why
    B = verts_src.batch
    for name, t in given.items():
        if isinstance(t, RaggedPoints):
            if t.packed.dtype is not torch.float32 or t.packed.shape[1] != 3:
                return f"{name} must hold float32 [capacity, 3] rows, got {t.packed.dtype} {tuple(t.packed.shape)}"
        elif t is not None:
            if name == "cano":
                return f"{name} must be a RaggedPoints, got {type(t).__name__}"
            if not torch.is_tensor(t):
                return f"{name} must be a RaggedPoints or a torch.Tensor, got {type(t).__name__}"
            if t.dtype is not torch.float32 or t.dim() != 3 or t.shape[2] != 3:
                return f"{name} must be float32 [B, S, 3], got {t.dtype} {tuple(t.shape)}"
    if torch.is_tensor(surface) and surface.shape[0] != B:
        return f"surface holds {surface.shape[0]} shapes, verts_src {B}"
    if isinstance(surface, RaggedPoints) and surface.batch != B:
        return f"surface holds {surface.batch} shapes, verts_src {B}"
    if cano is not None and not verts_src.same_layout(cano):
        return f"cano ({cano!r}) is not over the same layout as verts_src ({verts_src!r})"
    if surface_cano is not None:
        if surface is None:
            return "surface_cano goes with a surface over the same layout"
        if isinstance(surface, RaggedPoints) != isinstance(surface_cano, RaggedPoints) or (
                not surface.same_layout(surface_cano) if isinstance(surface, RaggedPoints) else surface_cano.shape != surface.shape):
            return "surface_cano is not over the same layout as the surface"
    for name, t in (("verts_src", verts_src), ("surface", surface)):
        if isinstance(t, RaggedPoints):
            for b, n in enumerate(t.counts):
                if n == 0:
                    return f"an empty shape: shape {b} of {name} has no points"
    cloud = verts_src if surface is None else surface
    if isinstance(cloud, RaggedPoints):
        for net in nets:
            npoints, ks, _ = net.encoder._pyramid_args()
            tb = net.encoder.transformer_begin
            need = [(npoints[0], "points the first level samples")]
            need += [(k, "neighbours of " + what) for what, k in (("the first attention block", None if tb.group_all else tb.k),
                                                                  ("the first set abstraction", ks[0][0])) if k is not None]
            for b, n in enumerate(cloud.counts):
                for k, what in need:
                    if n < k:
                        return f"shape {b} of the cloud has {n} points, fewer than the {k} {what}"
    return None


class RaggedEditSession(_Session):
    """An EditSession over a PACKED batch of B meshes of different vertex counts (nsdp_amd.ragged) -- the reference's batch loop
    over its user-handle data set, where the cloud network 2 encodes is each mesh's own vertex set.  Opened once, it holds network
    1's outputs, network 2's index sets (Deformation_Networks.ragged_geometry) and the per-shape bounding boxes; a drag is one
    [B, 8] host-to-device copy, the packed handle kernel (include/nsdp_handles_ragged.h), network 2's encoder over the cached
    sets and one ragged decode (two with a separate cloud).  Nothing of a drag reads an offsets tensor back: the counts are the
    host's at open, so with ``graph=True`` the drags by rule replay one captured graph and the drags by masks a second.

    ``verts_src``: RaggedPoints [cap, 3] on the GPU.  ``surface``: None (the cloud is the vertex set), a RaggedPoints [scap, 3]
    of B clouds of different sample counts, or a rectangular [B, S, 3] tensor.  ``cano`` / ``surface_cano``: the coordinates the
    bounding-box rule is evaluated on, over the layouts of ``verts_src`` / ``surface`` (None: the source coordinates).

    The predictions are bit-equal to the step function on the ragged data_dict the drag stands for
    (tests/test_edit_session_ragged_gpu.py).  Staleness: as for EditSession -- ``reopen()`` after the weights changed."""

    _refusal = staticmethod(ragged_refusal)
    _cached = ("geometry", "buf", "inputs", "_vert_idx")

    def _hold(self, verts_src, surface, cano, surface_cano):
        import torch
        from .ragged import RaggedPoints
        tight = lambda r: RaggedPoints(r.packed.contiguous(), r.offsets, r.counts)      # (the host counts: read once, here)
        self.verts = tight(verts_src)
        self.same = surface is None
        self.rect = torch.is_tensor(surface)
        self.surface = self.verts if self.same else (surface.contiguous() if self.rect else tight(surface))
        self.verts_rule = self.verts if cano is None else tight(cano)
        if surface_cano is None:
            self.surface_rule = self.verts_rule if self.same else self.surface
        else:
            self.surface_rule = surface_cano.contiguous() if self.rect else tight(surface_cano)

    def _layout(self):
        cloud_rows = tuple(self.surface.shape[:2]) if self.rect else (self.surface.capacity,)
        return self.verts.batch, self.verts.packed, cloud_rows, (self.verts.capacity,)

    # ------------------------------------------------------------------ the cached state
    def _open(self):
        import torch
        from . import pointnet2_utils as pu
        with torch.no_grad():
            dev = self.verts.device
            verts, surface, net = self.verts, self.surface, self.net
            B, vcap = verts.batch, verts.capacity
            if self.flow:
                outs = self.model.canonicalize([surface] if self.same else [surface, verts], surface)
                self.surf2cano, self.verts2cano = outs[0], outs[-1]
            else:
                self.surf2cano, self.verts2cano = surface, verts
            # the deformation network's input rows: columns 0:3 written here, once; 3:7 by every drag's kernel
            if self.rect:
                S = surface.shape[1]
                self.buf = torch.zeros((B, S, 7), dtype=torch.float32, device=dev)
                self.buf[:, :, 0:3] = self.surf2cano
                self.inputs = self.buf
                self.geometry = {"encoder": net.encoder.geometry(self.buf)}      # (net.geometry's encoder part)
                anchors = self.geometry["encoder"]["anchors"]
                self.geometry["query_idx"] = net.decoder.geometry(self.surf2cano, anchors)["query_idx"]
                self.geometry["query_points"] = self.surf2cano
                self._vert_idx = net.query_geometry_ragged(self.verts2cano, anchors)["query_idx"]
                self.bounds = pu.handle_bounds(self.surface_rule)
                self.surface_tgt = torch.empty((B, S, 3), dtype=torch.float32, device=dev)
                self.surface_handle = torch.empty((B, S), dtype=torch.uint8, device=dev)
            else:
                scap, total = surface.capacity, surface.total
                self.buf = torch.zeros((scap, 7), dtype=torch.float32, device=dev)
                self.buf[:total, 0:3] = self.surf2cano.packed[:total]
                self.inputs = surface.like(self.buf)
                self.geometry = net.ragged_geometry(self.surf2cano, self.inputs)
                anchors = self.geometry["encoder"]["anchors"]
                self._vert_idx = (self.geometry["query_idx"] if self.same
                                  else net.query_geometry_ragged(self.verts2cano, anchors)["query_idx"])
                self.bounds = pu.handle_bounds_ragged(self.surface_rule.packed, surface.offsets, max(surface.counts))
                # (zeros: the padding rows, which no kernel writes, are handed out with the rest)
                self.surface_tgt = torch.zeros((scap, 3), dtype=torch.float32, device=dev)
                self.surface_handle = torch.zeros((scap,), dtype=torch.uint8, device=dev)
            self.params = torch.zeros((B, 8), dtype=torch.int32, device=dev)
            self._mask_h = self._mask_m = self._vmask_h = self._vmask_m = None      # (made by the first drag by masks)
            if self.same:
                self.verts_bounds, self.verts_tgt, self.verts_handle, self._vrows = self.bounds, self.surface_tgt, self.surface_handle, None
            else:
                self.verts_bounds = pu.handle_bounds_ragged(self.verts_rule.packed, verts.offsets, max(verts.counts))
                self.verts_tgt = torch.zeros((vcap, 3), dtype=torch.float32, device=dev)
                self.verts_handle = torch.zeros((vcap,), dtype=torch.uint8, device=dev)
                self._vrows = torch.empty((vcap, 7), dtype=torch.float32, device=dev)      # (the kernel's required output)

    # ------------------------------------------------------------------ one drag
    def _enqueue(self, masks, vert_masks):
        """Everything of a drag that runs on the GPU behind the parameter copy: capturable, reads device tensors only."""
        from . import pointnet2_utils as pu
        net = self.net
        hm, mm = (self._mask_h, self._mask_m) if masks else (None, None)
        if self.rect:
            pu.handle_rows(self.surface_rule, self.surface, self.bounds, self.params, self.buf, hm, mm, tgt=self.surface_tgt,
                           handle_out=self.surface_handle)
        else:
            pu.handle_rows_ragged(self.surface_rule.packed, self.surface.packed, self.surface.offsets, self.bounds, self.params,
                                  self.buf, hm, mm, tgt=self.surface_tgt, handle_out=self.surface_handle)
        if not self.same and (not masks or vert_masks):
            vh, vm = (self._vmask_h, self._vmask_m) if masks else (None, None)
            pu.handle_rows_ragged(self.verts_rule.packed, self.verts.packed, self.verts.offsets, self.verts_bounds, self.params,
                                  self._vrows, vh, vm, tgt=self.verts_tgt, handle_out=self.verts_handle)
        if self.rect:
            enc = net.encode(self.buf, geometry=self.geometry)
        else:
            enc = net.encode(self.inputs, ragged_geometry=self.geometry)
        enc_v = dict(enc)
        enc_v["query_idx"], enc_v["query_points"] = self._vert_idx, self.verts2cano
        out = {"verts_tgt_pred": net.decode(self.verts2cano, enc_v).packed}
        if not self.same:
            pred = net.decode(self.surf2cano, enc)      # (its query_idx / query_points are the cloud's)
            out["surface_samples_tgt_pred"] = pred if self.rect else pred.packed
        return out

    def _result(self, pred, own, own_pred, have_verts, with_inputs):
        """``verts_tgt_pred``, ``verts_tgt`` and ``cano_handle_vert_idx`` as RaggedPoints over the vertices' offsets (the handle
        as [cap, 1] bool rows), ``surface_samples_tgt_pred`` and ``cano_handle_sample_idx`` over the cloud's layout (the same
        objects when the cloud is the vertex set), and with ``with_inputs`` ``surface_samples_inputs``: a RaggedPoints of
        [scap, 7] rows (or [B, S, 7]) the step function takes as it is."""
        import torch
        over_cloud = (lambda t: t) if self.rect else self.surface.like
        out = {"verts_tgt_pred": self.verts.like(own_pred(pred["verts_tgt_pred"]))}
        out["surface_samples_tgt_pred"] = (out["verts_tgt_pred"] if self.same
                                           else over_cloud(own_pred(pred["surface_samples_tgt_pred"])))
        out["verts_tgt"] = self.verts.like(own(self.verts_tgt)) if have_verts else None
        out["cano_handle_vert_idx"] = self.verts.like(own(self.verts_handle).view(torch.bool).unsqueeze(-1)) if have_verts else None
        if self.same:
            out["cano_handle_sample_idx"] = out["cano_handle_vert_idx"]
        else:
            h = own(self.surface_handle).view(torch.bool)
            out["cano_handle_sample_idx"] = h if self.rect else self.surface.like(h.unsqueeze(-1))
        if with_inputs:
            if self.rect:
                out["surface_samples_inputs"] = torch.cat([self.surface, self.buf[:, :, 3:7]], dim=-1)
            else:
                out["surface_samples_inputs"] = self.surface.like(torch.cat([self.surface.packed, self.buf[:, 3:7]], dim=-1))
        return out


def reference_data_dict(verts_src, surface, spec_or_params, cano=None, surface_cano=None):
    """The data_dict one drag stands for, built with torch alone (the reference's cano_handle_user_define as array expressions):
    what the session's results are compared with.  ``spec_or_params``: a HandleSpec (the same drag for every shape) or the
    [B, 8] int32 array of pack_params."""
    import numpy as np
    import torch
    B = verts_src.shape[0]
    words = (pack_params(B, spec_or_params.part, spec_or_params.translation, spec_or_params.partial_range, spec_or_params.cliptail)
             if isinstance(spec_or_params, HandleSpec) else np.asarray(spec_or_params))
    dev = verts_src.device
    part = torch.from_numpy(words[:, 0].copy()).to(dev).view(B, 1)
    clip = torch.from_numpy(words[:, 1].copy() != 0).to(dev).view(B, 1)
    f = torch.from_numpy(words.view(np.float32).copy()).to(dev)
    r, d = f[:, 2:3], f[:, None, 3:6]

    def one(src, rule):
        rule = src if rule is None else rule
        lo, hi = rule.amin(dim=1), rule.amax(dim=1)
        x, y, z = rule[:, :, 0], rule[:, :, 1], rule[:, :, 2]
        head = y < lo[:, 1:2] + r
        tail = y > hi[:, 1:2] - r
        tail = torch.where(clip, tail & (z > -r), tail)
        foot = z < lo[:, 2:3] + r
        handle = head | tail | foot
        left, right, front, behind = foot & (x > 0), foot & (x < 0), foot & (y < 0), foot & (y > 0)
        regions = (head, tail, left & front, right & front, left & behind, right & behind)
        move = torch.zeros_like(head)
        for i, reg in enumerate(regions):
            move = torch.where(part == i, reg, move)
        tgt = src + d * move[:, :, None].float()
        return handle, tgt

    vh, vt = one(verts_src, cano)
    sh, st = (vh, vt) if surface is None else one(surface, surface_cano)
    surf = surface if surface is not None else verts_src
    maskf = sh[:, :, None].float()
    return {"surface_samples_inputs": torch.cat([surf, st * maskf, maskf], dim=-1).contiguous(),
            "surface_samples_src": surf.contiguous(), "verts_src": verts_src.contiguous(), "verts_tgt": vt,
            "cano_handle_vert_idx": vh, "cano_handle_sample_idx": sh}


# ---------------------------------------------------------------------------------------------------------------- the tool
def build_parser():
    ap = argparse.ArgumentParser(description="Drag handles on a (synthetic) mesh through an editing session, timed")
    ap.add_argument("config_file")
    ap.add_argument("--vertices", type=int, default=25000, help="mesh vertices per shape (default 25000)")
    ap.add_argument("--surface", type=int, default=None,
                    help="samples of a separate surface cloud (default: none -- the cloud is the vertex set, as in the "
                         "reference's user-handle data set)")
    ap.add_argument("--batch", type=int, default=None, help="shapes per call (default: the config's test.batch_size, else 1)")
    ap.add_argument("--vertex-counts", default=None, metavar="n1,n2,...",
                    help="a packed batch of meshes of these vertex counts through a RaggedEditSession (replaces --vertices and "
                         "--batch; the cloud is the vertex set unless --surface-counts or --surface is given)")
    ap.add_argument("--surface-counts", default=None, metavar="s1,s2,...",
                    help="with --vertex-counts: a separate packed cloud of these sample counts, one per mesh")
    ap.add_argument("--part", default=None, choices=PARTS, help="the region that moves (default: the config's data.userhandle)")
    ap.add_argument("--translate", default=None, metavar="dx,dy,dz",
                    help="its translation (default: the config's xtrans, ytrans, ztrans)")
    ap.add_argument("--drags", type=int, default=10, help="timed drags (each with another translation)")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--graph", action="store_true", help="capture the drag once and replay it")
    ap.add_argument("--weight_file", default=None, help="weights of the whole model (default: procedural weights)")
    ap.add_argument("--out", default=None, help="directory for the last drag's predictions (<key>.npy)")
    return ap


def spec_from_args(args, config):
    """The drag of the command line: --part / --translate over the config's data.userhandle; without either, head by
    (-0.15, -0.2, -0.2) -- config/tosca/head.yaml's."""
    data = config.get("data") or {}
    base = HandleSpec.from_config(data) if isinstance(data.get("userhandle"), dict) and any(data["userhandle"].get(p) for p in PARTS) \
        else HandleSpec("head", (-0.15, -0.2, -0.2), float(data.get("partial_range", 0.1)),
                        bool((data.get("userhandle") or {}).get("cliptail", False)))
    part = args.part or base.part
    translation = base.translation
    if args.translate is not None:
        try:
            translation = tuple(float(v) for v in args.translate.split(","))
        except ValueError:
            translation = ()
        if len(translation) != 3:
            sys.exit(f"nsdp_amd.edit: --translate wants dx,dy,dz, got {args.translate!r}")
    return HandleSpec(part, translation, base.partial_range, base.cliptail)


def counts_from_args(args):
    """(--vertex-counts, --surface-counts) as lists of positive integers, (None, None) without --vertex-counts."""
    def numbers(text, flag):
        try:
            vals = [int(v) for v in text.split(",")]
        except ValueError:
            vals = []
        if not vals or min(vals) < 1:
            sys.exit(f"nsdp_amd.edit: {flag} wants positive integers n1,n2,..., got {text!r}")
        return vals
    if args.vertex_counts is None:
        if args.surface_counts is not None:
            sys.exit("nsdp_amd.edit: --surface-counts goes with --vertex-counts")
        return None, None
    verts = numbers(args.vertex_counts, "--vertex-counts")
    surf = None if args.surface_counts is None else numbers(args.surface_counts, "--surface-counts")
    if surf is not None and (len(surf) != len(verts) or args.surface is not None):
        sys.exit("nsdp_amd.edit: --surface-counts wants one count per mesh of --vertex-counts, and not --surface beside it")
    return verts, surf


def _setup(args, smallest_cloud):
    """What both forms of the command line do first: the thread cap, the GPU, the config and its drag, the pyramid cut to the
    smallest cloud, the model (procedural weights without --weight_file) -- and the two helpers of the timed windows."""
    from .cpu_budget import cap_thread_pools
    cap_thread_pools(16)
    import torch
    if not torch.cuda.is_available():
        sys.exit("nsdp_amd.edit: needs a GPU (the session has no CPU path)")
    device = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    from . import synth
    from .config import load_config
    from .infer import _pyramid
    from .model import build_model
    config = load_config(args.config_file)
    spec = spec_from_args(args, config)
    _pyramid(config, smallest_cloud)
    model, _, _, test_fn = build_model(config, weight_file=args.weight_file, device="cpu")
    if args.weight_file is None:
        state = synth.procedural_state_dict(model.state_dict(), SEED_WEIGHTS)
        model.load_state_dict({k: torch.from_numpy(v) for k, v in state.items()})
    model.to(device).eval()

    def timed(fn, n=1):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for i in range(n):
            fn(i)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / max(1, n)

    def translation(i):      # (another drag every time: nothing of a previous one can be reused)
        return tuple(v * (1.0 + 0.01 * i) for v in spec.translation)

    return device, config, spec, model, test_fn, timed, translation


def main_ragged(args, vertex_counts, surface_counts):
    """--vertex-counts: the packed session on synthetic meshes, timed against the parent's two alternatives -- the ragged step
    function per drag, and one batch-1 EditSession per mesh dragged in turn."""
    B = len(vertex_counts)
    cloud_counts = surface_counts or ([args.surface] * B if args.surface else vertex_counts)
    device, config, spec, model, test_fn, timed, translation = _setup(args, min(cloud_counts))
    import numpy as np
    import torch
    from . import pointnet2_utils, synth
    from .infer import _checksum
    from .ragged import RaggedPoints
    meshes = [torch.from_numpy(synth.uniform(SEED_DATA + b, "mesh_verts", (1, n, 3), -0.5, 0.5)).to(device)
              for b, n in enumerate(vertex_counts)]
    verts = RaggedPoints.from_list([m[0] for m in meshes])
    clouds, surface = None, None
    if surface_counts is not None:
        clouds = [torch.from_numpy(synth.uniform(SEED_DATA + b, "mesh_surface", (1, n, 3), -0.5, 0.5)).to(device)
                  for b, n in enumerate(surface_counts)]
        surface = RaggedPoints.from_list([c[0] for c in clouds])
    elif args.surface is not None:
        clouds = [torch.from_numpy(synth.uniform(SEED_DATA + b, "mesh_surface", (1, args.surface, 3), -0.5, 0.5)).to(device)
                  for b in range(B)]
        surface = torch.cat(clouds, dim=0)

    warm = max(args.warmup, 1)
    with torch.no_grad():
        box = {}
        timed(lambda i: box.update(s=RaggedEditSession(model, verts, surface, partial_range=spec.partial_range,
                                                       cliptail=spec.cliptail, graph=args.graph)))      # (also packs the weights)
        session = box["s"]
        ms_open = timed(lambda i: session.reopen())
        out = {}
        for i in range(warm):      # (--graph: the first drag captures)
            session.drag(spec.part, translation(i))
        ms_drag = timed(lambda i: out.update(session.drag(spec.part, translation(i), clone=False)), args.drags)
        out = session.drag(spec.part, translation(args.drags - 1), with_inputs=True)
        inputs = out["surface_samples_inputs"]
        dd = {"surface_samples_inputs": inputs, "verts_src": verts,
              "surface_samples_src": inputs.columns(0, 3) if isinstance(inputs, RaggedPoints) else inputs[:, :, 0:3].contiguous()}
        for _ in range(warm):
            test_fn(model, dict(dd), config)
        full = {}
        ms_full = timed(lambda i: full.update(test_fn(model, dict(dd), config)[1]), args.drags)
        packed = lambda t: t.packed if isinstance(t, RaggedPoints) else t
        equal = all(torch.equal(packed(out[k]), packed(full[k])) for k in ("verts_tgt_pred", "surface_samples_tgt_pred"))
        # the parent's other alternative: one batch-1 session per mesh, dragged in turn
        singles = [EditSession(model, m, None if clouds is None else clouds[b], partial_range=spec.partial_range,
                               cliptail=spec.cliptail, graph=args.graph) for b, m in enumerate(meshes)]
        for i in range(warm):
            for s1 in singles:
                s1.drag(spec.part, translation(i))
        ms_singles = timed(lambda i: [s1.drag(spec.part, translation(i), clone=False) for s1 in singles], args.drags)
        for s1 in singles:
            s1.close()
        pointnet2_utils.check_fps_cluster()
    if args.out:
        os.makedirs(args.out, exist_ok=True)
        for k in ("verts_tgt_pred", "surface_samples_tgt_pred", "verts_tgt"):
            np.save(os.path.join(args.out, k + ".npy"), packed(out[k]).cpu().numpy())
    line = {"metric": "edit_session_ragged", "model_type": config["model"]["type"], "graph": bool(args.graph), "batch": B,
            "vertex_counts": vertex_counts, "surface_counts": surface_counts, "surface": args.surface,
            "cloud_is_vertex_set": surface is None, "part": spec.part, "translation": list(spec.translation),
            "partial_range": spec.partial_range, "cliptail": spec.cliptail, "drags": args.drags, "warmup": args.warmup,
            "handle_points": int(packed(out["cano_handle_sample_idx"]).sum()),
            "ms_per_drag": round(ms_drag, 4), "ms_open": round(ms_open, 4), "ms_full_call": round(ms_full, 4),
            "ms_per_mesh_sessions": round(ms_singles, 4),
            "full_call_over_drag": round(ms_full / ms_drag, 3) if ms_drag > 0 else None,
            "per_mesh_sessions_over_drag": round(ms_singles / ms_drag, 3) if ms_drag > 0 else None,
            "replays": session.replays, "eager_calls": session.eager_calls, "equal_to_full_call": bool(equal),
            "checksum": _checksum(packed(out["verts_tgt_pred"]))}
    print(json.dumps(line), flush=True)
    session.close()
    return 0


def main(argv=None):
    args = build_parser().parse_args(list(sys.argv[1:] if argv is None else argv))
    vertex_counts, surface_counts = counts_from_args(args)
    if vertex_counts is not None:
        if (args.surface is not None and args.surface < 1) or args.drags < 1:
            sys.exit("nsdp_amd.edit: --surface and --drags want positive integers")
        return main_ragged(args, vertex_counts, surface_counts)
    if args.vertices < 1 or (args.surface is not None and args.surface < 1) or args.drags < 1:
        sys.exit("nsdp_amd.edit: --vertices, --surface and --drags want positive integers")
    device, config, spec, model, test_fn, timed, translation = _setup(args, args.surface or args.vertices)
    import numpy as np
    import torch
    from . import pointnet2_utils, synth
    from .infer import _checksum
    batch = args.batch or int((config.get("test") or {}).get("batch_size", 1) or 1)
    verts = torch.from_numpy(synth.uniform(SEED_DATA, "mesh_verts", (batch, args.vertices, 3), -0.5, 0.5)).to(device)
    surface = None if args.surface is None else \
        torch.from_numpy(synth.uniform(SEED_DATA, "mesh_surface", (batch, args.surface, 3), -0.5, 0.5)).to(device)
    with torch.no_grad():
        box = {}
        timed(lambda i: box.update(s=EditSession(model, verts, surface, partial_range=spec.partial_range, cliptail=spec.cliptail,
                                                 graph=args.graph)))      # (the first open also packs the weights)
        session = box["s"]
        ms_open = timed(lambda i: session.reopen())
        out = {}
        for i in range(max(args.warmup, 1)):      # (--graph: the first drag captures)
            session.drag(spec.part, translation(i))
        ms_drag = timed(lambda i: out.update(session.drag(spec.part, translation(i), clone=False)), args.drags)
        out = session.drag(spec.part, translation(args.drags - 1), with_inputs=True)
        dd = {"surface_samples_inputs": out["surface_samples_inputs"], "verts_src": verts,
              "surface_samples_src": out["surface_samples_inputs"][:, :, 0:3].contiguous()}
        for _ in range(max(args.warmup, 1)):
            test_fn(model, dict(dd), config)
        full = {}
        ms_full = timed(lambda i: full.update(test_fn(model, dict(dd), config)[1]), args.drags)
        equal = all(torch.equal(out[k], full[k]) for k in ("verts_tgt_pred", "surface_samples_tgt_pred"))
        pointnet2_utils.check_fps_cluster()
    if args.out:
        os.makedirs(args.out, exist_ok=True)
        for k in ("verts_tgt_pred", "surface_samples_tgt_pred", "verts_tgt"):
            np.save(os.path.join(args.out, k + ".npy"), out[k].cpu().numpy())
    line = {"metric": "edit_session", "model_type": config["model"]["type"], "graph": bool(args.graph), "batch": batch,
            "vertices": args.vertices, "surface": args.surface, "cloud_is_vertex_set": surface is None, "part": spec.part,
            "translation": list(spec.translation), "partial_range": spec.partial_range, "cliptail": spec.cliptail,
            "drags": args.drags, "warmup": args.warmup, "handle_points": int(out["cano_handle_sample_idx"].sum()),
            "ms_per_drag": round(ms_drag, 4), "ms_open": round(ms_open, 4), "ms_full_call": round(ms_full, 4),
            "full_call_over_drag": round(ms_full / ms_drag, 3) if ms_drag > 0 else None,
            "replays": session.replays, "eager_calls": session.eager_calls, "equal_to_full_call": bool(equal),
            "checksum": _checksum(out["verts_tgt_pred"])}
    print(json.dumps(line), flush=True)
    session.close()
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
