"""The Chamfer training loss (include/nsdp_chamfer.h, csrc/chamfer.hip): a loss between a predicted cloud and a target cloud
that needs no row-for-row correspondence,

    L = (1/B) sum_b [ w_pt (1/n) sum_i min_j |p_i - q_j|^2 / 2  +  w_tp (1/m) sum_j min_i |q_j - p_i|^2 / 2 ]

for predictions ``[B, n, 3]`` and targets ``[B, m, 3]``, fp32, ``m`` not tied to ``n``.  Squared distances (the metric's square
root has no gradient at zero and stays in eval_metric.py); the ``/ 2`` is ``compute_l2_error``'s, so that with ``w_tp = 0`` and
every nearest neighbour the true correspondent the loss IS the l2 loss, up to rounding.

Forward: one native call -- the two searches of ``nsdp_nn_dist2`` with indices, the per-shape terms and the scalar reduced in
double in a fixed order.  Backward: one kernel launch per operand that needs a gradient, a gather-reduce over the inverse lists
(``hip_attention.ascending_inverse_lists``) of the opposite direction's index map, in a fixed order and without floating-point
atomics: two runs give the same bits, and a captured step replays to the bits of the eager one.  While a stream capture is
running the list build is a node of the graph (``inverse_lists`` caches nothing then).

``training_loss(config)`` is what the step functions call: ``config["training"]["loss"]`` absent or ``"l2"`` ->
``compute_l2_error`` itself, ``"chamfer"`` -> this loss with the weights of ``config["training"]["chamfer"]``.
"""
from __future__ import annotations

import ctypes
import functools

import torch

from . import hip_attention
from ._lib import NsdpHipError, check, fptr, iptr, lib, on_device, stream_ptr
from .ragged import RaggedPoints

_ci, _cf = ctypes.c_int, ctypes.c_float

MAX_BATCH = 65535
MAX_POINTS = 1 << 20            # per shape and cloud: the limit of the searches and of the list build
LOSSES = ("l2", "chamfer")


def refusal(pred, target):
    """Why ``chamfer_loss`` cannot take these operands (None: it can), each reason named."""
    given = {"pred": pred, "target": target}
    for name, t in given.items():
        if isinstance(t, RaggedPoints):
            return (f"ragged inputs: {name} is a RaggedPoints -- training is rectangular here, the Chamfer loss takes [B, n, 3] "
                    "predictions and [B, m, 3] targets (the per-shape Chamfer METRIC of packed sets is eval_metric.chamfer_distance_batch)")
    for name, t in given.items():
        if not torch.is_tensor(t):
            return f"{name} must be a torch.Tensor, got {type(t).__name__}"
        if t.dtype is not torch.float32:
            return f"dtype: {name} must be torch.float32, got {t.dtype} (the step functions hand over their fp32 prediction)"
        if t.dim() != 3 or t.shape[2] != 3:
            return f"shape: {name} must be [B, points, 3], got {tuple(t.shape)}"
    if pred.shape[0] != target.shape[0]:
        return f"mismatched B: pred holds {pred.shape[0]} shapes, target {target.shape[0]}"
    B, n, m = int(pred.shape[0]), int(pred.shape[1]), int(target.shape[1])
    if not 1 <= B <= MAX_BATCH:
        return f"limits: B = {B} shapes, the entries take 1 .. {MAX_BATCH}"
    for name, count in (("n", n), ("m", m)):
        if not 1 <= count <= MAX_POINTS:
            return f"limits: {name} = {count} points per shape, the entries take 1 .. {MAX_POINTS}"
    if B * max(n, m) >= 1 << 31:
        return f"limits: B * max(n, m) = {B * max(n, m)} rows, the searches take fewer than 2^31"
    for name, t in given.items():
        if not t.is_cuda:
            return f"CPU tensors: {name} is on the CPU -- the loss's kernels have no CPU path and there is no fallback"
    if pred.device != target.device:
        return f"devices: pred on {pred.device}, target on {target.device}"
    return None


def forward_raw(pred, target, w_pt: float = 1.0, w_tp: float = 1.0):
    """One nsdp_chamfer_forward call on contiguous fp32 GPU operands, outside autograd: -> (loss [1], terms [B], dist2_pt [B, n],
    idx_pt [B, n] int32, dist2_tp [B, m], idx_tp [B, m] int32) -- distances and indices are ``nn_dist2(..., return_index=True)``'s
    of either direction, bit for bit."""
    B, n, m = int(pred.shape[0]), int(pred.shape[1]), int(target.shape[1])
    dev = pred.device
    L = lib()
    L.nsdp_chamfer_forward_workspace_bytes.restype = ctypes.c_size_t
    need = int(L.nsdp_chamfer_forward_workspace_bytes(_ci(B)))
    with on_device(pred):
        ws = torch.empty((need // 4,), dtype=torch.float32, device=dev)
        d_pt = torch.empty((B, n), dtype=torch.float32, device=dev)
        i_pt = torch.empty((B, n), dtype=torch.int32, device=dev)
        d_tp = torch.empty((B, m), dtype=torch.float32, device=dev)
        i_tp = torch.empty((B, m), dtype=torch.int32, device=dev)
        terms = torch.empty((B,), dtype=torch.float32, device=dev)
        loss = torch.empty((1,), dtype=torch.float32, device=dev)
        check(L.nsdp_chamfer_forward(fptr(pred, "pred"), fptr(target, "target"), _ci(B), _ci(n), _ci(m), _cf(w_pt), _cf(w_tp),
                                     ctypes.c_void_p(ws.data_ptr()), fptr(d_pt), iptr(i_pt), fptr(d_tp), iptr(i_tp), fptr(terms),
                                     fptr(loss), stream_ptr()), "nsdp_chamfer_forward")
        del ws      # (stream-ordered: the allocator hands the block on behind the launches; a graph's pool keeps it)
    return loss, terms, d_pt, i_pt, d_tp, i_tp


class _ChamferLoss(torch.autograd.Function):
    """(pred, target, w_pt, w_tp) -> (loss [], terms [B]); ``terms`` carries no gradient.  The indices are kept for backward."""

    @staticmethod
    def forward(ctx, pred, target, w_pt, w_tp):
        loss, terms, _, i_pt, _, i_tp = forward_raw(pred, target, w_pt, w_tp)
        ctx.save_for_backward(pred, target, i_pt, i_tp)
        ctx.weights = (float(w_pt), float(w_tp))
        ctx.mark_non_differentiable(terms)
        return loss.reshape(()), terms

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_loss, _g_terms):
        pred, target, i_pt, i_tp = ctx.saved_tensors
        w_pt, w_tp = ctx.weights
        g = g_loss.to(torch.float32).reshape(1).contiguous()      # (stays on the device: the kernel reads it)
        d_pred = d_target = None
        with on_device(pred):
            if ctx.needs_input_grad[0]:
                d_pred = backward_operand(pred, target, i_pt, i_tp, g, w_pt, w_tp)
            if ctx.needs_input_grad[1]:
                d_target = backward_operand(target, pred, i_tp, i_pt, g, w_tp, w_pt)
        return d_pred, d_target, None, None


def backward_operand(x, y, idx_x, idx_y, g, w_direct, w_list):
    """One nsdp_chamfer_backward call, d L / d x: x [B, n_self, 3], y the other cloud, idx_x [B, n_self] the nearest y of every x, idx_y [B, n_other] the
    nearest x of every y (its inverse lists are built here unless ``w_list`` is 0), g [1] the upstream gradient on the device."""
    B, n_self, n_other = int(x.shape[0]), int(x.shape[1]), int(y.shape[1])
    offsets = entries = None
    if float(_cf(w_list).value) != 0.0:
        offsets, entries = hip_attention.ascending_inverse_lists(idx_y, n_self, who="chamfer_loss")
    grad = torch.empty((B, n_self, 3), dtype=torch.float32, device=x.device)
    null = ctypes.c_void_p(0)
    check(lib().nsdp_chamfer_backward(fptr(x, "self"), fptr(y, "other"), iptr(idx_x, "idx_self"),
                                      null if offsets is None else iptr(offsets, "offsets"),
                                      null if entries is None else iptr(entries, "entries"), fptr(g, "g"), _ci(B), _ci(n_self),
                                      _ci(n_other), _cf(w_direct), _cf(w_list), fptr(grad), stream_ptr()), "nsdp_chamfer_backward")
    return grad


def chamfer_loss(pred, target, w_pred_to_target: float = 1.0, w_target_to_pred: float = 1.0, return_per_shape: bool = False):
    """The Chamfer loss of predictions ``pred [B, n, 3]`` against targets ``target [B, m, 3]`` (fp32, on the GPU): a 0-dim
    tensor autograd can differentiate with respect to ``pred`` and -- only where it requires a gradient -- ``target``.
    ``return_per_shape``: ``(loss, terms [B])`` with the per-shape terms (each a function of its own shape's rows alone; they
    carry no gradient).  Anything else is refused by name (``refusal``)."""
    why = refusal(pred, target)
    if why is not None:
        raise NsdpHipError("chamfer_loss: " + why)
    loss, terms = _ChamferLoss.apply(pred.contiguous(), target.contiguous(), float(w_pred_to_target), float(w_target_to_pred))
    return (loss, terms) if return_per_shape else loss


def composed_loss(pred, target, w_pred_to_target: float = 1.0, w_target_to_pred: float = 1.0, indices=None):
    """The same loss composed from existing operations -- ``nn_dist2`` with indices, ``index_points`` through autograd,
    elementwise torch: a dozen launches and three ``[B, n, 3]`` temporaries per direction, and a gradient summed in whatever
    order those operations use.  The comparison partner of ``chamfer_loss`` (tools/bench_chamfer.py, the train-step tests), not
    a path the step functions take.  ``indices = (idx_pt, idx_tp)``: use these index sets; otherwise they are searched."""
    from . import pointnet2_utils
    from .model.utils import index_points
    if indices is None:
        with torch.no_grad():
            indices = (pointnet2_utils.nn_dist2(pred.detach().contiguous(), target.detach().contiguous(), True)[1],
                       pointnet2_utils.nn_dist2(target.detach().contiguous(), pred.detach().contiguous(), True)[1])
    idx_pt, idx_tp = indices
    pt = ((pred - index_points(target, idx_pt)).pow(2).sum(dim=2) / 2.0).mean(dim=1)
    tp = ((target - index_points(pred, idx_tp)).pow(2).sum(dim=2) / 2.0).mean(dim=1)
    return (w_pred_to_target * pt + w_target_to_pred * tp).mean()


def training_loss(config):
    """The loss function ``(pred, target) -> 0-dim tensor`` a training / validation step applies to its prediction and
    ``space_samples_tgt``.  ``config["training"]["loss"]`` absent or ``"l2"``: ``compute_l2_error`` itself (today's path, row-for-row
    correspondences); ``"chamfer"``: ``chamfer_loss`` with ``config["training"]["chamfer"]``'s ``w_pred_to_target`` /
    ``w_target_to_pred`` (both default to 1), and ``space_samples_tgt`` may then be ``[B, m, 3]`` with any ``m``."""
    from .model.utils import compute_l2_error
    training = (config or {}).get("training") or {}
    name = training.get("loss", "l2")
    if name is None or name == "l2":
        return compute_l2_error
    if name != "chamfer":
        raise ValueError(f"config['training']['loss'] = {name!r}: one of {LOSSES}")
    weights = training.get("chamfer") or {}
    unknown = sorted(set(weights) - {"w_pred_to_target", "w_target_to_pred"})
    if unknown:
        raise ValueError(f"config['training']['chamfer']: unknown keys {unknown} (w_pred_to_target, w_target_to_pred)")
    return functools.partial(chamfer_loss, w_pred_to_target=float(weights.get("w_pred_to_target", 1.0)),
                             w_target_to_pred=float(weights.get("w_target_to_pred", 1.0)))
