"""Deformation network = encoder + decoder, and its step functions
(mirror of the reference's model/deformation_networks.py)."""
from __future__ import annotations

import inspect
import os

import torch
import torch.nn as nn

from .decoder import decoder_dict
from .encoder import encoder_dict
from ..chamfer import training_loss
from ..rigidity import training_regulariser
from .utils import compute_l2_error
from .. import ragged
from ..ragged import RaggedPoints

# One encoder pass per distinct surface cloud (NSDP_ENCODE_ONCE=0: one per module call, the reference's op sequence -- A/B)
ENCODE_ONCE = os.environ.get("NSDP_ENCODE_ONCE", "1") != "0"
# NSDP_DECODER_PREFETCH=1: the decoder's anchor-only work (anchor search, relative coordinates, position-encoding MLP: ~1.8 ms
# at B = 32) on its own stream beside the encoder's forward chain instead of behind it.  OFF by default -- measured on one box,
# interleaved: B = 32 41.30 / 41.38 ms against 40.91 / 41.03 (41.06-41.18 with the prefetch GEMM confined to half the chip), bf16
# +0.1 ms, FlowArbitrary +1 ms; B = 8 14.73 / 14.76 against 14.86 / 14.90 (the only win).  The encoder's forward is not idle
# under it: its 500- and 100-point levels are 256 k- and 320 k-row GEMMs that fill the chip, so the two chains time-share, and
# the early launch gives up the q - k + pos epilogue of the position-encoding GEMM (docs/EXPERIMENTS.md, round 5).
DECODER_PREFETCH = os.environ.get("NSDP_DECODER_PREFETCH", "0") == "1"


class Deformation_Networks(nn.Module):
    """reference model/deformation_networks.py:12-60 (input-channel logic :17-30)."""

    def __init__(self, cfg, no_input_corr=False):
        super().__init__()
        self.no_input_corr = no_input_corr
        use_normals = cfg["model"]["use_normals"]
        if no_input_corr:
            has_features, inp_feat_dim = (True, 3) if use_normals else (False, 0)
        else:
            has_features, inp_feat_dim = (True, 7) if use_normals else (True, 4)
        self.encoder = encoder_dict[cfg["model"]["encoder"]](
            has_features=has_features, inp_feat_dim=inp_feat_dim, **cfg["model"]["encoder_kwargs"])
        self.decoder = decoder_dict[cfg["model"]["decoder"]](**cfg["model"]["decoder_kwargs"])

    @torch.no_grad()
    def geometry(self, points, surface_samples_inputs, training=None):
        """Every index set forward(points, surface_samples_inputs) derives from its two coordinate inputs alone (the encoder's
        sampling / grouping pyramid and neighbour sets, the queries' anchor neighbours, the inverse lists of the backward pass
        when ``training``), on the current stream.  forward(geometry=) takes it instead of searching: a host that knows the next
        batch computes this beside the current step (nsdp_amd.graph_step.PipelinedGeometry) -- FPS is a chain of ~600 dependent
        iterations that no batch size shortens.  ``points`` must be the very tensor forward() is then called with."""
        if isinstance(surface_samples_inputs, RaggedPoints):
            raise ValueError("ragged surface cloud refused: geometry() / PipelinedGeometry compute the index sets of rectangular "
                             "clouds only")
        x = surface_samples_inputs[:, :, 0:3].contiguous() if self.no_input_corr else surface_samples_inputs
        if not (hasattr(self.encoder, "geometry") and hasattr(self.decoder, "geometry")):
            raise NotImplementedError("geometry(): this encoder / decoder pair searches inside its forward pass only")
        g = {"encoder": self.encoder.geometry(x, training)}
        g.update(self.decoder.geometry(points, g["encoder"]["anchors"]))
        g["query_points"] = points
        return g

    @torch.no_grad()
    def ragged_geometry(self, points, surface_samples_inputs):
        """geometry() for a PACKED surface cloud (a RaggedPoints of [total, C] rows): the encoder's index sets
        (PointTransformerEncoder.ragged_geometry) and, for ``points`` -- a RaggedPoints of queries -- each query's nearest anchors
        (``query_idx`` [cap, k], ``query_points`` = points).  ``encode(cloud, ragged_geometry=g)`` then searches nothing, and
        ``decode(points, encoding)`` takes the cached neighbours when ``points`` is the very object given here.  The cloud's
        coordinates (columns 0:3) must be the ones these sets were made from; its other columns may change between calls."""
        if not isinstance(surface_samples_inputs, RaggedPoints) or not isinstance(points, RaggedPoints):
            raise ValueError("ragged_geometry(): a RaggedPoints of queries and a RaggedPoints surface cloud (geometry() takes the "
                             "rectangular ones)")
        why = self.ragged_surface_refusal()
        if why is not None:
            raise ValueError("ragged surface cloud refused: " + why)
        cloud = surface_samples_inputs.columns(0, 3) if self.no_input_corr else surface_samples_inputs
        g = {"encoder": self.encoder.ragged_geometry(cloud)}
        g.update(self.query_geometry_ragged(points, g["encoder"]["anchors"]))
        return g

    def query_geometry_ragged(self, points, anchors):
        """The decoder side of ragged_geometry() alone: packed queries against anchors [B, A, 3] -> ``query_idx`` [cap, k]
        (hip_decoder.decoder_forward_ragged's search, on its operands) and ``query_points``."""
        from .. import pointnet2_utils as pu
        if points.batch != anchors.shape[0]:
            raise ValueError(f"ragged_geometry(): {points.batch} shapes of queries against anchors of {anchors.shape[0]}")
        xyz_q = points.packed.contiguous().float()
        idx = pu.knn_ragged(xyz_q, points.offsets, anchors.contiguous().float(), self.decoder.ct1.nneigh)
        return {"query_idx": idx, "query_points": points}

    def encode(self, surface_samples_inputs, queries=None, geometry=None, ragged_geometry=None):
        """The encoding {'z', 'anchors', 'anchor_feats'} of a surface cloud -- the half of forward() that does not depend on
        the query points.  Callers that decode several query sets against ONE cloud (FlowArbitrary, the dense-inference step
        functions) encode once and call decode() per set; the reference re-runs the whole module each time.
        ``queries``: the points decode() will be called with next -- the decoder's anchor-only work is then launched beside the
        encoder's forward chain (CrossTransformerDecoder.prefetch, NSDP_DECODER_PREFETCH=0 switches it off).
        ``surface_samples_inputs`` may be a RaggedPoints of [total, C] rows (clouds of different sample counts, nsdp_amd.ragged):
        inference only, refused with its reason where it cannot run (ragged_surface_refusal).  ``ragged_geometry``: the index
        sets of that packed cloud computed ahead (ragged_geometry()); the encoding then carries ``query_idx`` / ``query_points``."""
        if isinstance(surface_samples_inputs, RaggedPoints):
            why = self.ragged_surface_refusal(geometry)
            if why is not None:
                raise ValueError("ragged surface cloud refused: " + why)
            if ragged_geometry is not None:
                cloud = surface_samples_inputs.columns(0, 3) if self.no_input_corr else surface_samples_inputs
                enc = self.encoder._forward_ragged(cloud, ragged_geometry=ragged_geometry["encoder"])
                enc["query_idx"], enc["query_points"] = ragged_geometry.get("query_idx"), ragged_geometry.get("query_points")
                return enc
            surface_samples_inputs.counts      # (read back once, here: a column view made below shares the host copy)
            return self.encoder(surface_samples_inputs.columns(0, 3) if self.no_input_corr else surface_samples_inputs)
        if ragged_geometry is not None:
            raise ValueError("ragged_geometry= goes with a packed surface cloud (a RaggedPoints); geometry= with a rectangular one")
        x = surface_samples_inputs[:, :, 0:3].contiguous() if self.no_input_corr else surface_samples_inputs
        if geometry is not None:
            enc = self.encoder(x, geometry=geometry["encoder"])
            enc["query_idx"], enc["query_points"] = geometry["query_idx"], geometry["query_points"]
            return enc
        if (DECODER_PREFETCH and torch.is_tensor(queries) and queries.is_cuda and hasattr(self.decoder, "prefetch")
                and "on_anchors" in inspect.signature(self.encoder.forward).parameters):
            return self.encoder(x, on_anchors=lambda anchors, after: self.decoder.prefetch(queries, anchors, after))
        return self.encoder(x)

    def ragged_surface_refusal(self, geometry=None):
        """Why this network cannot encode a packed surface cloud right now (None: it can): what the encoder's ragged first level
        and the ragged decoder (hip_decoder.ragged_refusal: it decodes the surface samples) refuse, named."""
        from .. import hip_decoder
        from .encoder.pointransformer import PointTransformerEncoder
        if geometry is not None:
            return "geometry= (index sets computed ahead of the pass, PipelinedGeometry) exists for rectangular clouds only"
        if not isinstance(self.encoder, PointTransformerEncoder):
            return f"the {type(self.encoder).__name__} encoder (pointnet++ alternate) has no ragged first level"
        if torch.is_grad_enabled():
            return "autograd is enabled: ragged surface clouds are inference only -- call under torch.no_grad()"
        if self.training or self.encoder.training:
            return ("the model is in training mode: BatchNorm would take batch statistics over the packed rows of all shapes -- "
                    "call model.eval() first")
        return hip_decoder.ragged_refusal(self.decoder) if hip_decoder.supported(self.decoder) else (
            "decoder geometry: the packed surface samples are decoded by the fused kernels, built for dim=200, hidden_dim=128, "
            "n_blocks=5, out_dim=3")

    def decode(self, points, encoding, jacobian=False):
        """points [B,NQ,3] -> [B,NQ,3]; a RaggedPoints (meshes of different sizes, nsdp_amd.ragged) -> a RaggedPoints.
        ``jacobian=True``: -> (that, the deformation gradient [B,NQ,3,3] / a RaggedPoints over [cap,9]), cross-attention
        decoder only (CrossTransformerDecoder.forward)."""
        if jacobian:
            if "jacobian" not in inspect.signature(self.decoder.forward).parameters:
                raise ValueError(f"decode(jacobian=True): the {type(self.decoder).__name__} computes no Jacobian (the cross-attention "
                                 "decoder does)")
            return self.decoder(points, encoding, jacobian=True)
        return self.decoder(points, encoding)

    def forward(self, points, surface_samples_inputs, geometry=None):
        if not isinstance(points, RaggedPoints):
            points = points if points.is_contiguous() else points.contiguous()
        return self.decoder(points, self.encode(surface_samples_inputs, queries=points, geometry=geometry))


def _loss_with_cano(model, data_dict, config, geometry=None):
    """forward + loss of train_on_batch_with_cano (reference :66-72), as a tensor: the l2 loss, or what
    ``config["training"]["loss"]`` names (chamfer.training_loss), plus the regulariser of ``config["training"]["rigidity"]``.
    ``geometry``: model.geometry() of this batch's inputs, computed ahead of the step."""
    if geometry is not None:
        pred = model(data_dict["space_samples_src"], data_dict["surface_samples_inputs"], geometry=geometry)
    else:
        pred = model(data_dict["space_samples_src"], data_dict["surface_samples_inputs"])
    return _configured_loss(config, pred, data_dict)


def _configured_loss(config, pred, data_dict):
    """The data term ``config["training"]["loss"]`` names and, where ``config["training"]["rigidity"]`` is set, the local-rigidity
    regulariser of the prediction against ``space_samples_src`` (rigidity.training_regulariser; without the key nothing is added)."""
    loss = training_loss(config)(pred, data_dict["space_samples_tgt"])
    reg = training_regulariser(config)
    if reg is not None:
        loss = loss + reg(pred, data_dict["space_samples_src"])
    return loss


def _train_step_with_cano(model, optimizer, data_dict, config, geometry=None):
    """The step of train_on_batch_with_cano up to (not including) the host read-back of the loss: everything that is
    enqueued on the GPU.  This is what nsdp_amd.graph_step captures and replays."""
    optimizer.zero_grad()
    loss = _loss_with_cano(model, data_dict, config, geometry)
    loss.backward()
    optimizer.step()
    return loss


def train_on_batch_with_cano(model, optimizer, data_dict, config):
    """reference model/deformation_networks.py:63-77."""
    return _train_step_with_cano(model, optimizer, data_dict, config).item()


train_on_batch_with_cano.tensor_step = _train_step_with_cano
train_on_batch_with_cano.loss_fn = _loss_with_cano      # (data-parallel replay: two graphs around the gradient exchange)


@torch.no_grad()
def validate_on_batch_with_cano(model, data_dict, config):
    """reference model/deformation_networks.py:80-88; reports the configured loss (chamfer.training_loss) plus the configured
    regulariser (rigidity.training_regulariser): the sum the train step minimises."""
    pred = model(data_dict["space_samples_src"], data_dict["surface_samples_inputs"])
    return _configured_loss(config, pred, data_dict).item()


def l2_error_of(pred, target):
    """compute_l2_error of a dense-inference step; for a packed vertex set (RaggedPoints) the mean over the shapes of the
    per-shape error, on the device (ragged.l2_error)."""
    if isinstance(pred, RaggedPoints):
        return ragged.l2_error(pred, ragged.as_ragged(target))
    return compute_l2_error(pred, target)


def check_ragged_surface(inputs, src):
    """A ragged ``surface_samples_inputs`` goes with a ``surface_samples_src`` packed over the same offsets (and a rectangular
    one with a tensor): the step functions decode the source samples against the encoding of the inputs, shape by shape."""
    if isinstance(inputs, RaggedPoints) != isinstance(src, RaggedPoints):
        raise ValueError("surface_samples_inputs and surface_samples_src must both be RaggedPoints or both be tensors")
    if isinstance(inputs, RaggedPoints) and not inputs.same_layout(src):
        raise ValueError(f"surface_samples_src ({src!r}) is not packed like surface_samples_inputs ({inputs!r})")


@torch.no_grad()
def test_on_batch_with_cano(model, data_dict, config, compute_loss=False, jacobian=False):
    """Dense inference: surface samples, then all mesh vertices (reference :90-109).  ``data_dict["verts_src"]`` may be a
    RaggedPoints (meshes of different vertex counts, packed): ``verts_tgt_pred`` is then one too.  Independently,
    ``surface_samples_inputs`` may be a RaggedPoints of [total, 7] rows (clouds of different sample counts) with
    ``surface_samples_src`` packed over the same offsets: ``surface_samples_tgt_pred`` then comes back as a RaggedPoints.
    ``jacobian=True`` also writes ``data_dict["verts_tgt_jacobian"]``, the deformation gradient at every vertex ([B,V,3,3], or a
    RaggedPoints over [cap,9] for a packed ``verts_src``); ``verts_tgt_pred`` keeps its bits.  Surface samples get none."""
    inputs = data_dict["surface_samples_inputs"]
    check_ragged_surface(inputs, data_dict["surface_samples_src"])
    if jacobian:
        # (one encoding whatever ENCODE_ONCE says: the A/B switch of the reference's op sequence has no Jacobian form)
        encoding = model.encode(inputs)
        data_dict["surface_samples_tgt_pred"] = model.decode(data_dict["surface_samples_src"], encoding)
        deformed_verts, data_dict["verts_tgt_jacobian"] = model.decode(data_dict["verts_src"], encoding, jacobian=True)
    elif ENCODE_ONCE:
        # the reference runs the module twice on the same surface input (:96, :101): same encoding both times
        encoding = model.encode(inputs)
        data_dict["surface_samples_tgt_pred"] = model.decode(data_dict["surface_samples_src"], encoding)
        deformed_verts = model.decode(data_dict["verts_src"], encoding)
    else:
        data_dict["surface_samples_tgt_pred"] = model(data_dict["surface_samples_src"], inputs)
        deformed_verts = model(data_dict["verts_src"], inputs)
    data_dict["verts_tgt_pred"] = deformed_verts
    if compute_loss:
        loss = l2_error_of(deformed_verts, data_dict["verts_tgt"])
    else:
        loss = torch.zeros((1), dtype=torch.float32)
    return loss.item(), data_dict
