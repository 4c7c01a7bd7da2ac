"""The local-rigidity training regulariser (include/nsdp_rigidity.h, csrc/rigidity.hip): an as-isometric-as-possible energy
over the neighbour edges of the query set,

    L = w (1/B) sum_b (1 / (n K)) sum_i sum_j ( |p_i - p_l|^2 - |s_i - s_l|^2 )^2 / 4,        l = idx[b, i, j]

for predictions ``[B, n, 3]``, sources ``[B, n, 3]`` (fp32, row ``i`` of the prediction the image of row ``i`` of the source)
and neighbour sets ``idx [B, n, K]``.  Every pair of neighbouring source points should keep its distance under the
deformation: the term that ties a prediction to the source's local geometry where the data term (l2, or the correspondence-free
Chamfer loss) does not.  Squared lengths: ``|p_i - p_l|`` has no gradient at ``p_i = p_l``, the collapsed case this term exists
for; the ``/ 4`` leaves the gradient free of factors.  It needs no second derivatives, and no gradient flows to the source.

Forward: one native call -- the residuals, the per-shape terms and the scalar reduced in double in a fixed order.  Backward:
one kernel launch, the point's own K columns plus a gather-reduce over the ascending inverse lists of ``idx``
(``hip_attention.ascending_inverse_lists``), in a fixed order and without floating-point
atomics: two runs give the same bits, and a captured step replays to the bits of the eager one.  While a stream capture is
running the list build is a node of the graph.

``training_regulariser(config)`` is what the step functions call: ``config["training"]["rigidity"]`` absent or ``None`` ->
``None`` (the step is untouched), ``{weight, k}`` -> a callable ``(pred, source)``.
"""
from __future__ import annotations

import ctypes

import torch

from . import hip_attention
from ._lib import NsdpHipError, check, fptr, iptr, lib, on_device, stream_ptr
from .ragged import RaggedPoints

_ci, _cf = ctypes.c_int, ctypes.c_float

MAX_BATCH = 65535
MAX_POINTS = 1 << 20            # per shape: the limit of the search and of the list build
MAX_K = 32                      # neighbours per point
MAX_ENTRIES = 1 << 25           # n * K per shape: the bound of the list build
SEARCH_MAX_K = 64               # the self-search's own limit on its k (= K + 1: column 0 is the point itself)


def refusal(pred, source, idx=None):
    """Why ``local_rigidity_loss`` cannot take these operands (None: it can), each reason named.  ``idx`` None: not judged."""
    given = {"pred": pred, "source": source}
    if idx is not None:
        given["idx"] = idx
    for name, t in given.items():
        if isinstance(t, RaggedPoints):
            return (f"ragged inputs: {name} is a RaggedPoints -- training is rectangular here, the rigidity loss takes [B, n, 3] "
                    "predictions and sources and [B, n, K] neighbour sets")
    for name, t in given.items():
        if not torch.is_tensor(t):
            return f"{name} must be a torch.Tensor, got {type(t).__name__}"
    for name, t in (("pred", pred), ("source", source)):
        if t.dtype is not torch.float32:
            return f"dtype: {name} must be torch.float32, got {t.dtype} (the step functions hand over their fp32 prediction)"
        if t.dim() != 3 or t.shape[2] != 3:
            return f"shape: {name} must be [B, points, 3], got {tuple(t.shape)}"
    if pred.shape[0] != source.shape[0]:
        return f"mismatched B: pred holds {pred.shape[0]} shapes, source {source.shape[0]}"
    if pred.shape[1] != source.shape[1]:
        return (f"mismatched n: pred holds {pred.shape[1]} points per shape, source {source.shape[1]} -- row i of the prediction "
                "is the image of row i of the source")
    B, n = int(pred.shape[0]), int(pred.shape[1])
    if not 1 <= B <= MAX_BATCH:
        return f"limits: B = {B} shapes, the entries take 1 .. {MAX_BATCH}"
    if not 1 <= n <= MAX_POINTS:
        return f"limits: n = {n} points per shape, the entries take 1 .. {MAX_POINTS}"
    if idx is not None:
        if idx.dtype is not torch.int32:
            return f"dtype: idx must be torch.int32, got {idx.dtype}"
        if idx.dim() != 3 or idx.shape[0] != B or idx.shape[1] != n:
            return f"shape: idx must be [B, n, K] = [{B}, {n}, K], got {tuple(idx.shape)}"
        K = int(idx.shape[2])
        if not 1 <= K <= MAX_K:
            return f"limits: K = {K} neighbours per point, the entries take 1 .. {MAX_K}"
        if n * K > MAX_ENTRIES:
            return f"limits: n * K = {n * K} entries per shape, the list build takes up to {MAX_ENTRIES}"
        if B * n * K >= 1 << 31:
            return f"limits: B * n * K = {B * n * K} entries, the entries take fewer than 2^31"
    for name, t in given.items():
        if not t.is_cuda:
            return f"CPU tensors: {name} is on the CPU -- the loss's kernels have no CPU path and there is no fallback"
    for name, t in given.items():
        if t.device != pred.device:
            return f"devices: pred on {pred.device}, {name} on {t.device}"
    return None


def neighbour_sets(source, k: int = 8):
    """The k nearest OTHER rows of every source row, ``[B, n, k]`` int32: the exact self-search ``knn(source, source, k + 1)``
    (the cell grid for large clouds) with column 0 dropped -- column 0 is the point itself, or an exact duplicate of it with a
    smaller index (then the point itself sits in a later column and contributes exactly 0)."""
    from . import pointnet2_utils
    if not torch.is_tensor(source) or source.dim() != 3 or source.shape[2] != 3:
        raise NsdpHipError(f"neighbour_sets: source must be a [B, n, 3] tensor, got {tuple(getattr(source, 'shape', ()))}")
    k, n = int(k), int(source.shape[1])
    if not 1 <= k <= MAX_K:
        raise NsdpHipError(f"neighbour_sets: limits: k = {k} neighbours per point, the loss takes 1 .. {MAX_K}")
    if k + 1 > SEARCH_MAX_K:
        raise NsdpHipError(f"neighbour_sets: limits: the self-search needs k + 1 = {k + 1} columns, it takes up to {SEARCH_MAX_K}")
    if k + 1 > n:
        raise NsdpHipError(f"neighbour_sets: limits: k + 1 = {k + 1} columns of the self-search exceed the n = {n} points of a shape")
    with torch.no_grad():
        idx = pointnet2_utils.knn(source.detach().contiguous(), source.detach().contiguous(), k + 1)
        return idx[:, :, 1:].contiguous()


def forward_raw(pred, source, idx, weight: float = 1.0):
    """One nsdp_rigidity_forward call on contiguous GPU operands, outside autograd: -> (loss [1], terms [B], resid [B, n, K])."""
    B, n, K = int(idx.shape[0]), int(idx.shape[1]), int(idx.shape[2])
    dev = pred.device
    L = lib()
    L.nsdp_rigidity_forward_workspace_bytes.restype = ctypes.c_size_t
    need = int(L.nsdp_rigidity_forward_workspace_bytes(_ci(B)))
    with on_device(pred):
        ws = torch.empty((need // 4,), dtype=torch.float32, device=dev)
        resid = torch.empty((B, n, K), dtype=torch.float32, device=dev)
        terms = torch.empty((B,), dtype=torch.float32, device=dev)
        loss = torch.empty((1,), dtype=torch.float32, device=dev)
        check(L.nsdp_rigidity_forward(fptr(pred, "pred"), fptr(source, "source"), iptr(idx, "idx"), _ci(B), _ci(n), _ci(K),
                                      _cf(weight), ctypes.c_void_p(ws.data_ptr()), fptr(resid), fptr(terms), fptr(loss),
                                      stream_ptr()), "nsdp_rigidity_forward")
        del ws      # (stream-ordered: the allocator hands the block on behind the launches; a graph's pool keeps it)
    return loss, terms, resid


def backward_raw(pred, idx, resid, g, weight: float = 1.0):
    """One nsdp_rigidity_backward call, d L / d pred [B, n, 3]: the inverse lists of ``idx`` are built here; g [1] is the upstream
    gradient on the device."""
    B, n, K = int(idx.shape[0]), int(idx.shape[1]), int(idx.shape[2])
    # (ascending lists of idx viewed as [B, n * K]: the many-workgroup build by name beyond 1024 entries or 8192 points per shape)
    offsets, entries = hip_attention.ascending_inverse_lists(idx.view(B, n * K), n, who="local_rigidity_loss")
    grad = torch.empty((B, n, 3), dtype=torch.float32, device=pred.device)
    check(lib().nsdp_rigidity_backward(fptr(pred, "pred"), iptr(idx, "idx"), fptr(resid, "resid"), iptr(offsets, "offsets"),
                                       iptr(entries, "entries"), fptr(g, "g"), _ci(B), _ci(n), _ci(K), _cf(weight), fptr(grad),
                                       stream_ptr()), "nsdp_rigidity_backward")
    return grad


class _RigidityLoss(torch.autograd.Function):
    """(pred, source, idx, weight) -> (loss [], terms [B]); only ``pred`` gets a gradient.  The residuals are kept for backward."""

    @staticmethod
    def forward(ctx, pred, source, idx, weight):
        loss, terms, resid = forward_raw(pred, source, idx, weight)
        ctx.save_for_backward(pred, idx, resid)
        ctx.weight = float(weight)
        ctx.mark_non_differentiable(terms)
        return loss.reshape(()), terms

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_loss, _g_terms):
        pred, idx, resid = ctx.saved_tensors
        if not ctx.needs_input_grad[0]:
            return None, None, None, None
        g = g_loss.to(torch.float32).reshape(1).contiguous()      # (stays on the device: the kernel reads it)
        with on_device(pred):
            d_pred = backward_raw(pred, idx, resid, g, ctx.weight)
        return d_pred, None, None, None


def local_rigidity_loss(pred, source, k: int = 8, weight: float = 1.0, idx=None, return_per_shape: bool = False):
    """The local-rigidity loss of predictions ``pred [B, n, 3]`` of the sources ``source [B, n, 3]`` (fp32, on the GPU, row for
    row the same points): a 0-dim tensor autograd can differentiate with respect to ``pred``.  ``idx [B, n, K]`` int32: the
    neighbour sets, entries in [0, n); otherwise ``neighbour_sets(source, k)``.  ``return_per_shape``: ``(loss, terms [B])``, each
    term a function of its own shape's rows alone, without the weight and without a gradient.  Anything else is refused by
    name (``refusal``)."""
    why = refusal(pred, source, idx)
    if why is not None:
        raise NsdpHipError("local_rigidity_loss: " + why)
    if idx is None:
        idx = neighbour_sets(source, k)
    loss, terms = _RigidityLoss.apply(pred.contiguous(), source.detach().contiguous(), idx.contiguous(), float(weight))
    return (loss, terms) if return_per_shape else loss


def composed_loss(pred, source, idx, weight: float = 1.0):
    """The same loss composed from existing operations -- ``index_points`` through autograd and elementwise torch: a dozen
    launches, ``[B, n, K, 3]`` temporaries and a gradient scattered in whatever order those operations use.  The comparison
    partner of ``local_rigidity_loss`` (tools/bench_rigidity.py, the train-step tests), not a path the step functions take."""
    from .model.utils import index_points
    cur = (pred[:, :, None, :] - index_points(pred, idx)).pow(2).sum(dim=3)
    src = source.detach()
    rest = (src[:, :, None, :] - index_points(src, idx)).pow(2).sum(dim=3)
    return weight * ((cur - rest).pow(2) / 4.0).mean(dim=(1, 2)).mean()


class _Regulariser:
    """``(pred, source) -> 0-dim tensor``: ``local_rigidity_loss`` with a config's weight and k (looked up when called)."""

    def __init__(self, weight: float, k: int):
        self.weight, self.k = float(weight), int(k)

    def __call__(self, pred, source):
        return local_rigidity_loss(pred, source, k=self.k, weight=self.weight)

    def __repr__(self):
        return f"rigidity regulariser(weight={self.weight}, k={self.k})"


def training_regulariser(config):
    """What a training / validation step adds to its data term: None where ``config["training"]["rigidity"]`` is absent or None
    (the step is today's), else a callable ``(pred, space_samples_src)`` for ``{"weight": w, "k": 8}`` -- ``weight`` is required,
    ``k`` defaults to 8, unknown keys raise."""
    training = (config or {}).get("training") or {}
    section = training.get("rigidity")
    if section is None:
        return None
    if not isinstance(section, dict):
        raise ValueError(f"config['training']['rigidity'] must be a mapping {{weight, k}}, got {type(section).__name__}")
    unknown = sorted(set(section) - {"weight", "k"})
    if unknown:
        raise ValueError(f"config['training']['rigidity']: unknown keys {unknown} (weight, k)")
    if "weight" not in section:
        raise ValueError("config['training']['rigidity']: 'weight' is required")
    k = int(section.get("k", 8))
    if not 1 <= k <= MAX_K:
        raise ValueError(f"config['training']['rigidity']: k = {k}, one of 1 .. {MAX_K}")
    return _Regulariser(float(section["weight"]), k)
