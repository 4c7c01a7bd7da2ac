"""Two-network composition source -> canonical -> target
(mirror of the reference's model/flow_arbitrary.py)."""
from __future__ import annotations

import contextlib

import torch
import torch.nn as nn

from .. import hip_batchnorm, hip_decoder, precision
from . import deformation_networks
from ..ragged import RaggedPoints


class FlowArbitrary(nn.Module):
    """reference model/flow_arbitrary.py:8-27."""

    def __init__(self, cfg, model_canonicalize, model_deform):
        super().__init__()
        self.model_canonicalize = model_canonicalize
        self.model_deform = model_deform

    def _canonicalize_storage(self):
        # mixed storage (see nsdp_amd/precision.py): the network whose output points feed the second network's geometry
        # runs in fp32 storage; inputs and outputs are fp32 coordinates in either mode, so there is nothing to cast
        if precision.is_bf16() and precision.canonicalize_f32():
            return precision.storage(torch.float32)
        return contextlib.nullcontext()

    def canonicalize(self, query_sets, surface_samples_src, jacobian=False):
        """model_canonicalize applied to several query sets against the SAME source cloud: ONE encoder pass, ONE decoder pass
        over the concatenated queries (the decoder has no BatchNorm and treats query points independently).  The reference
        runs the whole network once per set (model/flow_arbitrary.py:19-20); in training mode the two encoder passes see the
        same batch, produce the same tensors and differ only in what they leave in the BatchNorm buffers -- two momentum
        updates from the same batch statistics, num_batches_tracked += 2 -- which hip_batchnorm.running_updates reproduces.
        Autograd sums the decoder paths into one encoder backward.
        ``jacobian``: True, or one flag per query set -- a flagged set comes back as (points, deformation gradient) (see
        Deformation_Networks.decode).  One encoding then and one decode per set: the decoder treats query points independently,
        so every set gets the bits the concatenated pass gives it."""
        net = self.model_canonicalize
        flags = [bool(jacobian)] * len(query_sets) if isinstance(jacobian, bool) else [bool(j) for j in jacobian]
        if len(flags) != len(query_sets):
            raise ValueError(f"canonicalize(): {len(flags)} jacobian flags for {len(query_sets)} query sets")
        with self._canonicalize_storage(), hip_decoder.canonicalize_mode():
            if any(flags):
                with hip_batchnorm.running_updates(len(query_sets)):
                    encoding = net.encode(surface_samples_src)
                return [self._decode_canonical(net, q if isinstance(q, RaggedPoints) else q.contiguous(), encoding, jacobian=j)
                        for q, j in zip(query_sets, flags)]
            if not deformation_networks.ENCODE_ONCE:
                return [net(q, surface_samples_src) for q in query_sets]
            if any(isinstance(q, RaggedPoints) for q in query_sets):
                # a packed vertex set beside the (rectangular) surface: one encoding, one decode per set
                with hip_batchnorm.running_updates(len(query_sets)):
                    encoding = net.encode(surface_samples_src)
                return [self._decode_canonical(net, q if isinstance(q, RaggedPoints) else q.contiguous(), encoding)
                        for q in query_sets]
            queries = query_sets[0] if len(query_sets) == 1 else torch.cat(list(query_sets), dim=1)
            queries = queries if queries.is_contiguous() else queries.contiguous()
            with hip_batchnorm.running_updates(len(query_sets)):      # (inert on eval-mode norms)
                encoding = net.encode(surface_samples_src, queries=queries)
            out = self._decode_canonical(net, queries, encoding)
            if len(query_sets) == 1:
                return [out]
            return list(torch.split(out, [q.shape[1] for q in query_sets], dim=1))

    @staticmethod
    def _decode_canonical(net, queries, encoding, jacobian=False):
        kw = {"jacobian": True} if jacobian else {}      # (the plain call stays the call it was: decode(queries, encoding))
        if precision.is_bf16() and precision.canonicalize_decoder_f32():
            # the middle point of the mixed storage (precision.py): bf16 encoder, fp32 decoder -- the encoding (one latent
            # code and 100 anchor features per shape) is cast once, the per-point chain runs in fp32 storage
            with precision.storage(torch.float32):
                enc32 = {k: (v.float() if torch.is_tensor(v) and v.dtype is torch.bfloat16 else v) for k, v in encoding.items()}
                return net.decode(queries, enc32, **kw)
        return net.decode(queries, encoding, **kw)

    def deform_input(self, surf_src2cano, surface_samples_tgt, cano_handle_sample_mask):
        if isinstance(surf_src2cano, RaggedPoints):      # ragged surface clouds: the packed [capacity, 7] concatenation
            return surf_src2cano.like(torch.cat([surf_src2cano.packed, surface_samples_tgt.packed,
                                                 cano_handle_sample_mask.packed], dim=-1))
        return torch.cat([surf_src2cano, surface_samples_tgt, cano_handle_sample_mask], dim=-1).contiguous()

    def forward(self, space_samples_src, surface_samples_src, surface_samples_tgt, cano_handle_sample_mask):
        space_src2cano, surf_src2cano = self.canonicalize([space_samples_src, surface_samples_src], surface_samples_src)
        deform_in = self.deform_input(surf_src2cano, surface_samples_tgt, cano_handle_sample_mask)
        return self.model_deform(space_src2cano if isinstance(space_src2cano, RaggedPoints) else space_src2cano.contiguous(), deform_in)


def _split(data_dict):
    s = data_dict["surface_samples_inputs"]
    if isinstance(s, RaggedPoints):      # ragged surface clouds: three packed sets over the same offsets
        if s.packed.shape[1] != 7:
            raise ValueError(f"ragged surface_samples_inputs must be [total, 7] rows, got {tuple(s.packed.shape)}")
        s.counts      # (read back once if the set came with device offsets alone: the three views share the host copy)
        return s.columns(0, 3), s.columns(3, 6), s.columns(6, 7)
    return s[:, :, 0:3], s[:, :, 3:6], s[:, :, 6:7]


def _loss_with_arbitrary(model, data_dict, config):
    """forward + loss of train_on_batch_with_arbitrary (reference :33-43), as a tensor: the l2 loss, or what
    ``config["training"]["loss"]`` names (chamfer.training_loss), plus the regulariser of ``config["training"]["rigidity"]``."""
    src, tgt, mask = _split(data_dict)
    pred = model(data_dict["space_samples_src"], src, tgt, mask)
    return deformation_networks._configured_loss(config, pred, data_dict)


def _train_step_with_arbitrary(model, optimizer, data_dict, config):
    """train_on_batch_with_arbitrary without the host read-back of the loss (what nsdp_amd.graph_step captures)."""
    optimizer.zero_grad()
    loss = _loss_with_arbitrary(model, data_dict, config)
    loss.backward()
    optimizer.step()
    return loss


def train_on_batch_with_arbitrary(model, optimizer, data_dict, config):
    """reference model/flow_arbitrary.py:30-48."""
    return _train_step_with_arbitrary(model, optimizer, data_dict, config).item()


train_on_batch_with_arbitrary.tensor_step = _train_step_with_arbitrary
train_on_batch_with_arbitrary.loss_fn = _loss_with_arbitrary


@torch.no_grad()
def validate_on_batch_with_arbitrary(model, data_dict, config):
    """reference model/flow_arbitrary.py:51-63; reports the configured loss (chamfer.training_loss) plus the configured regulariser."""
    src, tgt, mask = _split(data_dict)
    pred = model(data_dict["space_samples_src"], src, tgt, mask)
    return deformation_networks._configured_loss(config, pred, data_dict).item()


@torch.no_grad()
def test_on_batch_with_arbitrary(model, data_dict, config, compute_loss=False, jacobian=False):
    """reference model/flow_arbitrary.py:65-85.  ``data_dict["verts_src"]`` may be a RaggedPoints (meshes of different vertex
    counts, packed): both networks decode it ragged and ``verts_tgt_pred`` is one.  ``surface_samples_inputs`` may be a
    RaggedPoints of [total, 7] rows (clouds of different sample counts): the packed form travels between the two networks and
    ``surface_samples_tgt_pred`` comes back as a RaggedPoints.
    ``jacobian=True`` also writes ``data_dict["verts_tgt_jacobian"]`` ([B,V,3,3], or a RaggedPoints over [cap,9] for a packed
    ``verts_src``): the chain rule J2(q1) @ J1(q) over the two networks (network 2's encoding does not depend on the vertex
    queries); ``verts_tgt_pred`` keeps its bits.  Surface samples get none."""
    src, tgt, mask = _split(data_dict)
    if jacobian:
        from .. import deformation_gradient
        surf2cano, (verts2cano, jac1) = model.canonicalize([src, data_dict["verts_src"]], src, jacobian=[False, True])
        encoding = model.model_deform.encode(model.deform_input(surf2cano, tgt, mask))
        data_dict["surface_samples_tgt_pred"] = model.model_deform.decode(
            surf2cano if isinstance(surf2cano, RaggedPoints) else surf2cano.contiguous(), encoding)
        deformed_verts, jac2 = model.model_deform.decode(
            verts2cano if isinstance(verts2cano, RaggedPoints) else verts2cano.contiguous(), encoding, jacobian=True)
        data_dict["verts_tgt_jacobian"] = deformation_gradient.compose(jac2, jac1)
    elif deformation_networks.ENCODE_ONCE:
        # the reference's two model() calls (:71, :76) run six encoder passes over two distinct clouds: the source cloud
        # (four times) and the canonicalised surface + target + mask (twice).  Two passes here.
        surf2cano, verts2cano = model.canonicalize([src, data_dict["verts_src"]], src)
        encoding = model.model_deform.encode(model.deform_input(surf2cano, tgt, mask))
        data_dict["surface_samples_tgt_pred"] = model.model_deform.decode(
            surf2cano if isinstance(surf2cano, RaggedPoints) else surf2cano.contiguous(), encoding)
        deformed_verts = model.model_deform.decode(
            verts2cano if isinstance(verts2cano, RaggedPoints) else verts2cano.contiguous(), encoding)
    else:
        data_dict["surface_samples_tgt_pred"] = model(src, src, tgt, mask)
        deformed_verts = model(data_dict["verts_src"], src, tgt, mask)
    data_dict["verts_tgt_pred"] = deformed_verts
    if compute_loss:
        loss = deformation_networks.l2_error_of(deformed_verts, data_dict["verts_tgt"])
    else:
        loss = torch.zeros((1), dtype=torch.float32)
    return loss.item(), data_dict
