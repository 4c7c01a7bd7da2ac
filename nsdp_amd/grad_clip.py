"""Global gradient-norm clipping and non-finite-step skipping of the optimizer step: the two config keys, their refusal
messages, and the host-side optimizers for everything that is not `HipAdam`.

    training:
      clip_grad_norm: 1.0            # a bound on the L2 norm of ALL gradients together (torch.nn.utils.clip_grad_norm_)
      skip_nonfinite_steps: true     # a step whose gradient holds an inf or a NaN changes nothing and is counted

Both keys are extensions (the reference's ``config.get`` never asks for them); either alone enables the path, with both absent
`optimizer_factory` returns what it always returned.  GPU fp32 parameters under ``optimizer: Adam`` get
``HipAdam(max_grad_norm=, skip_nonfinite=)``: the rule decided on the device inside the step, capturable (include/nsdp_optim.h).
Everything else -- CPU parameters (host tests, the gloo harness), ``optimizer: SGD``, ``NSDP_HIP_ADAM=0`` -- gets
`ClippedAdam` / `ClippedSGD` below: the torch optimizer with ``clip_grad_norm_`` and the skip rule at the head of ``step()``.
The clip is in ``step()``, not in a step pre-hook, so the data-parallel exchange (a pre-hook) still runs before it and the
norm is the averaged gradient's.  These two DO rewrite the gradients, as torch does; `HipAdam` does not.
"""
from __future__ import annotations

import math

import torch

CLIP_KEY = "clip_grad_norm"
SKIP_KEY = "skip_nonfinite_steps"


def checked_max_norm(value, what):
    """``value`` as a float bound (None stays None: no bound).  +inf is allowed -- with the skip rule it is the guard alone;
    a bound that is <= 0 or NaN, or no number at all, is refused by name."""
    if value is None:
        return None
    if isinstance(value, bool) or not isinstance(value, (int, float)):
        raise ValueError(f"{what} must be a positive number, got {value!r}")
    value = float(value)
    if math.isnan(value) or value <= 0.0:
        raise ValueError(f"{what} must be a positive number (+inf allowed), got {value!r}")
    return value


def settings(training):
    """(max_norm or None, skip_nonfinite) from a config's ``training`` section."""
    max_norm = checked_max_norm(training.get(CLIP_KEY), f"training.{CLIP_KEY}")
    skip = training.get(SKIP_KEY, False)
    if skip is None:
        skip = False
    if not isinstance(skip, bool):
        raise ValueError(f"training.{SKIP_KEY} must be true or false, got {skip!r}")
    return max_norm, skip


def enabled(training):
    max_norm, skip = settings(training)
    return max_norm is not None or skip


def _unhooked(step):
    """A torch optimizer class's ``step`` without the hook-running wrapper ``Optimizer.__init__`` puts around it: the hooks of
    this optimizer have run by the time the subclass's ``step`` calls it."""
    while getattr(step, "hooked", False) and hasattr(step, "__wrapped__"):
        step = step.__wrapped__
    return step


class _ClippedStep:
    """Mixin in front of a torch optimizer: ``clip_grad_norm_`` over every parameter of every group, the skip rule, then the
    update.  The settings are attributes, not ``param_groups`` keys: ``state_dict()`` is the torch optimizer's, and a state dict
    written without them (the reference's) loads and leaves them alone."""

    def _init_clip(self, max_grad_norm, skip_nonfinite):
        self.max_grad_norm = checked_max_norm(max_grad_norm, f"{type(self).__name__}: max_grad_norm")
        self.skip_nonfinite = bool(skip_nonfinite)
        self._stats = {"norm": 0.0, "coef": 1.0, "steps": 0, "clipped": 0, "skipped": 0}

    def grad_stats(self):
        """As `HipAdam.grad_stats`: norm and factor of the last step, steps run / scaled / skipped so far."""
        return dict(self._stats)

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        params = [p for group in self.param_groups for p in group["params"] if p.grad is not None]
        if any(p.is_cuda for p in params) and torch.cuda.is_current_stream_capturing():
            raise RuntimeError(f"{type(self).__name__}: the clip / skip rule of this optimizer reads the gradient norm on the host "
                               "and cannot be captured; HipAdam (optimizer: Adam on GPU parameters) decides it on the device")
        if params:
            max_norm = float("inf") if self.max_grad_norm is None else self.max_grad_norm
            # (clip_grad_norm_ is these two calls; the skip rule sits between them, before anything is rewritten)
            total = torch.nn.utils.get_total_norm([p.grad for p in params], norm_type=2)
            norm = float(total)                                  # the host read a capture cannot make
            coef = float(torch.clamp(max_norm / (total + 1e-6), max=1.0))
            self._stats.update(norm=norm, coef=coef)
            self._stats["steps"] += 1
            if self.skip_nonfinite and not math.isfinite(norm):
                self._stats["skipped"] += 1
                return loss
            torch.nn.utils.clip_grads_with_norm_(params, max_norm, total)
            self._stats["clipped"] += 1 if coef < 1.0 else 0
        _unhooked(self._base.step)(self)
        return loss


class ClippedAdam(_ClippedStep, torch.optim.Adam):
    _base = torch.optim.Adam

    def __init__(self, params, *args, max_grad_norm=None, skip_nonfinite=False, **kwargs):
        torch.optim.Adam.__init__(self, params, *args, **kwargs)
        self._init_clip(max_grad_norm, skip_nonfinite)


class ClippedSGD(_ClippedStep, torch.optim.SGD):
    _base = torch.optim.SGD

    def __init__(self, params, *args, max_grad_norm=None, skip_nonfinite=False, **kwargs):
        torch.optim.SGD.__init__(self, params, *args, **kwargs)
        self._init_clip(max_grad_norm, skip_nonfinite)
