"""Global gradient-norm clipping and non-finite-step skipping on the host: the ordered-sum reference of tests/adam_clip_ref.py
against ``torch.nn.utils.clip_grad_norm_`` in float64, what ``optimizer_factory`` returns with and without the two config keys,
the torch-optimizer subclasses of nsdp_amd/grad_clip.py, and the per-epoch line of ``train.fit``."""
import argparse
import copy
import math

import numpy as np
import pytest
import torch

import adam_clip_ref as ref
from nsdp_amd import grad_clip, train


def _f32_ulp(x):
    return float(np.spacing(np.float32(abs(x))))


# ---------------------------------------------------------------------------------------------------------- reference vs torch
@pytest.mark.parametrize("max_norm,reached", [(1.0, True), (1e6, False)])
def test_reference_agrees_with_clip_grad_norm_in_float64(max_norm, reached):
    """S and norm within N * 2^-52 relative of torch's float64 result, N the element count.  Derived, not measured: the square
    of an fp32 value is exact in double, and a sum of N non-negative doubles in ANY order is within (N - 1) * 2^-53 relative of
    the exact sum -- so two orders differ by at most (N - 1) * 2^-52; torch's norm of per-tensor norms adds a rounding per
    tensor and per square root, a handful of units against N = 190 000."""
    gs = ref.grads(7, 0)
    N = ref.NUMEL
    S = ref.ordered_sumsq(gs)
    norm, coef, apply = ref.rule(S, max_norm)
    g64 = [torch.nn.Parameter(torch.zeros(g.shape, dtype=torch.float64)) for g in gs]
    for p, g in zip(g64, gs):
        p.grad = g.double().clone()
    total = float(torch.nn.utils.clip_grad_norm_(g64, max_norm, norm_type=2))
    bound = N * 2.0 ** -52
    assert abs(norm - total) <= bound * total
    assert abs(S - total * total) <= bound * total * total
    assert apply
    # torch's factor, read off the largest element it rewrote (a float64 quotient: 2^-52 relative)
    big = max(range(len(gs)), key=lambda i: float(gs[i].abs().max()))
    e = int(gs[big].abs().reshape(-1).argmax())
    factor = float(g64[big].grad.reshape(-1)[e]) / float(gs[big].double().reshape(-1)[e])
    assert (factor < 1.0) == reached
    if reached:
        assert coef.dtype == np.float32 and coef < 1.0 and abs(float(coef) - factor) <= _f32_ulp(factor)
    else:
        assert coef == np.float32(1.0) and factor == 1.0
        assert all(torch.equal(p.grad, g.double()) for p, g in zip(g64, gs))


def test_reference_sum_is_exact_on_integers_and_a_single_element():
    g = torch.Generator().manual_seed(3)
    ints = [torch.randint(-1000, 1001, shp, generator=g).float() for shp in ref.SHAPES]
    assert ref.ordered_sumsq(ints) == float(sum(int((t.long() ** 2).sum()) for t in ints))
    for t in range(len(ref.SHAPES)):
        for at in (0, 4095, 4096, -1):
            zeros = [torch.zeros(shp) for shp in ref.SHAPES]
            flat = zeros[t].reshape(-1)
            if at >= flat.numel():
                continue
            flat[at] = 3.25
            assert ref.ordered_sumsq(zeros) == 3.25 ** 2


@pytest.mark.parametrize("bad,coef_is", [(float("inf"), 0.0), (float("nan"), float("nan"))])
def test_reference_non_finite_cases_are_torchs(bad, coef_is):
    gs = ref.grads(7, 1)
    gs[10].reshape(-1)[-1] = bad
    S = ref.ordered_sumsq(gs)
    norm, coef, apply = ref.rule(S, 1.0)
    ps = [torch.nn.Parameter(torch.zeros(g.shape)) for g in gs]
    for p, g in zip(ps, gs):
        p.grad = g.clone()
    total = float(torch.nn.utils.clip_grad_norm_(ps, 1.0))
    assert not math.isfinite(S) and apply
    assert (math.isnan(total) and math.isnan(norm)) or total == norm == float("inf")
    assert (math.isnan(coef_is) and math.isnan(coef)) or float(coef) == coef_is
    # torch's rewritten gradient = g * coef: 0 * inf = NaN in that element and zeros elsewhere, or NaN everywhere
    mine = [g * torch.tensor(coef) for g in gs]
    assert all(torch.equal(torch.isnan(p.grad), torch.isnan(m)) for p, m in zip(ps, mine))
    assert not ref.rule(S, 1.0, skip_nonfinite=True)[2]
    assert ref.rule(S, float("inf"), skip_nonfinite=True)[2] is False
    assert ref.rule(ref.ordered_sumsq(ref.grads(7, 1)), float("inf"), skip_nonfinite=True)[1:] == (np.float32(1.0), True)


# ---------------------------------------------------------------------------------------------------------- optimizer_factory
def _cpu_params():
    return [torch.nn.Parameter(v) for v in ref.params(3)[:4]]


def test_factory_without_the_keys_returns_the_classes_it_always_returned():
    from nsdp_amd.model import optimizer_factory
    for extra in ({}, {"clip_grad_norm": None}, {"skip_nonfinite_steps": False}):
        _, adam = optimizer_factory(dict({"optimizer": "Adam", "lr": 5e-4}, **extra), _cpu_params())
        _, sgd = optimizer_factory(dict({"optimizer": "SGD", "lr": 0.1}, **extra), _cpu_params())
        assert type(adam) is torch.optim.Adam and type(sgd) is torch.optim.SGD
        assert not hasattr(adam, "grad_stats") and not hasattr(sgd, "grad_stats")


def test_factory_with_either_key_returns_the_clipping_subclass():
    from nsdp_amd.model import optimizer_factory
    for keys, want in (({"clip_grad_norm": 0.5}, (0.5, False)), ({"skip_nonfinite_steps": True}, (None, True)),
                       ({"clip_grad_norm": float("inf"), "skip_nonfinite_steps": True}, (float("inf"), True))):
        _, adam = optimizer_factory(dict({"optimizer": "Adam", "lr": 5e-4, "weight_decay": 0.01}, **keys), _cpu_params())
        _, sgd = optimizer_factory(dict({"optimizer": "SGD", "lr": 0.1}, **keys), _cpu_params())
        assert type(adam) is grad_clip.ClippedAdam and isinstance(adam, torch.optim.Adam)
        assert type(sgd) is grad_clip.ClippedSGD and isinstance(sgd, torch.optim.SGD)
        for opt in (adam, sgd):
            assert (opt.max_grad_norm, opt.skip_nonfinite) == want
            assert "max_grad_norm" not in opt.param_groups[0] and "skip_nonfinite" not in opt.param_groups[0]
        assert adam.param_groups[0]["weight_decay"] == 0.01 and sgd.param_groups[0]["momentum"] == 0.9


@pytest.mark.parametrize("bad", [0.0, -1.0, float("nan"), "1.0", True])
def test_a_bad_bound_is_refused_by_name(bad):
    from nsdp_amd.model import optimizer_factory
    with pytest.raises(ValueError, match=r"training\.clip_grad_norm"):
        optimizer_factory({"optimizer": "Adam", "clip_grad_norm": bad}, _cpu_params())
    with pytest.raises(ValueError, match="max_grad_norm"):
        grad_clip.ClippedAdam(_cpu_params(), max_grad_norm=bad)
    with pytest.raises(ValueError, match=r"training\.skip_nonfinite_steps"):
        optimizer_factory({"optimizer": "Adam", "skip_nonfinite_steps": "yes"}, _cpu_params())


def test_a_state_dict_without_the_settings_loads_and_keeps_them():
    """What the reference writes: torch.optim.Adam's state dict.  It loads into the clipping optimizer, whose settings are
    attributes and stay; and the clipping optimizer's own state dict is torch's, key for key."""
    from nsdp_amd.model import optimizer_factory
    cfg = {"optimizer": "Adam", "lr": 5e-4}
    ps = _cpu_params()
    _, plain = optimizer_factory(cfg, ps)
    for p, g in zip(ps, ref.grads(7, 0)):
        p.grad = g.clone()
    plain.step()
    written = copy.deepcopy(plain.state_dict())
    qs = _cpu_params()
    _, clipped = optimizer_factory(dict(cfg, clip_grad_norm=0.25, skip_nonfinite_steps=True), qs)
    clipped.load_state_dict(written)
    assert (clipped.max_grad_norm, clipped.skip_nonfinite) == (0.25, True)
    back = clipped.state_dict()
    assert back["param_groups"] == written["param_groups"]
    assert all(torch.equal(back["state"][i][k], written["state"][i][k]) for i in written["state"] for k in written["state"][i])
    for p, g in zip(qs, ref.grads(7, 1)):
        p.grad = g.clone()
    clipped.step()
    assert clipped.grad_stats()["clipped"] == 1 and float(clipped.state[qs[0]]["step"]) == 2.0


# ---------------------------------------------------------------------------------------------------------- the CPU subclasses
def _feed(ps, step, scale=1.0):
    for p, g in zip(ps, ref.grads(7, step)):
        p.grad = scale * g.clone()


@pytest.mark.parametrize("name", ["Adam", "SGD"])
def test_subclass_step_equals_clip_grad_norm_then_step_by_hand(name):
    from nsdp_amd.model import optimizer_factory
    cfg = {"optimizer": name, "lr": 1e-3, "weight_decay": 0.01}
    a, b = _cpu_params(), _cpu_params()
    _, mine = optimizer_factory(dict(cfg, clip_grad_norm=0.5), a)
    _, hand = optimizer_factory(cfg, b)
    for t in range(4):
        _feed(a, t)
        _feed(b, t)
        mine.step()
        norm = float(torch.nn.utils.clip_grad_norm_(b, 0.5))
        hand.step()
        st = mine.grad_stats()
        assert st["norm"] == norm and st["coef"] < 1.0 and st["steps"] == st["clipped"] == t + 1 and st["skipped"] == 0
        assert all(torch.equal(x, y) and torch.equal(x.grad, y.grad) for x, y in zip(a, b))
    assert all(torch.equal(mine.state[x][k], hand.state[y][k]) for x, y in zip(a, b) for k in hand.state[y])


def test_a_pre_hook_registered_after_construction_is_seen_by_the_clip():
    """The position of the data-parallel exchange: a step pre-hook.  One that multiplies every gradient by 10 must be seen by
    the norm -- and must run once, not again in the torch optimizer's own step underneath."""
    from nsdp_amd.model import optimizer_factory
    cfg = {"optimizer": "Adam", "lr": 1e-3}
    torch.optim.Adam([torch.nn.Parameter(torch.zeros(1))])      # (torch's own class has its step wrapped by now, whatever ran before)
    a, b = _cpu_params(), _cpu_params()
    _, hooked = optimizer_factory(dict(cfg, clip_grad_norm=0.5), a)
    _, fed = optimizer_factory(dict(cfg, clip_grad_norm=0.5), b)
    calls = []

    def times_ten(opt, args, kwargs):
        calls.append(1)
        for p in a:
            p.grad.mul_(10.0)
    hooked.register_step_pre_hook(times_ten)
    _feed(a, 0)
    _feed(b, 0, scale=10.0)
    want = float(torch.linalg.vector_norm(torch.cat([p.grad.reshape(-1) for p in b])))
    hooked.step()
    fed.step()
    assert len(calls) == 1
    assert hooked.grad_stats()["norm"] == fed.grad_stats()["norm"] and abs(hooked.grad_stats()["norm"] - want) <= 1e-5 * want
    assert all(torch.equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("name,bad", [("Adam", float("inf")), ("Adam", float("nan")), ("SGD", float("nan"))])
def test_a_skipped_step_leaves_everything_untouched_and_counts(name, bad):
    from nsdp_amd.model import optimizer_factory
    ps = _cpu_params()
    _, opt = optimizer_factory({"optimizer": name, "lr": 1e-3, "skip_nonfinite_steps": True}, ps)
    _feed(ps, 0)
    opt.step()
    before = copy.deepcopy(opt.state_dict())
    values = [p.detach().clone() for p in ps]
    _feed(ps, 1)
    ps[3].grad.reshape(-1)[-1] = bad
    kept = [p.grad.clone() for p in ps]
    opt.step()
    after = opt.state_dict()
    assert all(torch.equal(p, v) for p, v in zip(ps, values))
    assert all(torch.equal(p.grad.view(torch.int32), g.view(torch.int32)) for p, g in zip(ps, kept))      # (nothing rewritten)
    for i in before["state"]:
        for k, v in before["state"][i].items():
            assert torch.equal(torch.as_tensor(after["state"][i][k]), torch.as_tensor(v)), (i, k)
    st = opt.grad_stats()
    assert (st["steps"], st["clipped"], st["skipped"]) == (2, 0, 1) and not math.isfinite(st["norm"])
    _feed(ps, 2)
    opt.step()
    assert opt.grad_stats()["skipped"] == 1 and not torch.equal(ps[0], values[0])
    if name == "Adam":
        assert float(opt.state[ps[0]]["step"]) == 2.0


# ---------------------------------------------------------------------------------------------------------- fit's log
class _Stub(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.w = torch.nn.Parameter(torch.zeros(3))


def _train_on_batch(model, optimizer, sample, config):
    optimizer.zero_grad()
    loss = ((model.w - sample["t"]) ** 2).sum()
    loss.backward()
    optimizer.step()
    return loss.item()


def _fit_log(tmp_path, **keys):
    from nsdp_amd.model import optimizer_factory
    cfg = {"training": dict({"epochs": 2, "save_frequency": 20, "optimizer": "Adam", "lr": 0.1}, **keys), "validation": {"frequency": 10}}
    model = _Stub()
    tmp_path.mkdir()
    sched, opt = optimizer_factory(cfg["training"], model.parameters())
    loader = [{"t": torch.ones(3)}, {"t": 2 * torch.ones(3)}, {"t": torch.ones(3)}]
    args = argparse.Namespace(continue_from_epoch=0, best_val_loss=float("inf"))
    lines = []
    hist = train.fit(model, (_train_on_batch, None), sched, opt, loader, loader, cfg, str(tmp_path), args, "cpu",
                     log=lambda *a: lines.append(" ".join(str(x) for x in a)))
    return lines, hist


def test_fit_logs_one_gradient_line_per_epoch_with_the_key_and_none_without(tmp_path):
    with_key, hist = _fit_log(tmp_path / "a", clip_grad_norm=0.5)
    mine = [line for line in with_key if "gradient norm" in line]
    assert len(mine) == 2
    assert mine[0].startswith("epoch: 1 - ") and "clipped 3 / 3 steps" in mine[0] and "skipped 0" in mine[0]
    assert mine[1].startswith("epoch: 2 - ") and "/ 6 steps" in mine[1]
    assert [h[:2] for h in hist] == [("train", 0), ("train", 1)] and all(len(h) == 3 for h in hist)
    without, hist0 = _fit_log(tmp_path / "b")
    assert len(without) == 2 and not any("gradient norm" in line or "clipped" in line for line in without)
    assert [h[:2] for h in hist0] == [h[:2] for h in hist]


def test_fit_logs_nothing_for_an_optimizer_that_reports_no_statistics(tmp_path):
    """HipAdam built without the keys has the method and answers None: no line, and no device read."""
    class _Quiet(torch.optim.Adam):
        def grad_stats(self):
            return None
    from nsdp_amd.model import optimizer_factory
    model = _Stub()
    cfg = {"training": {"epochs": 1, "save_frequency": 20}, "validation": {"frequency": 10}}
    args = argparse.Namespace(continue_from_epoch=0, best_val_loss=float("inf"))
    lines = []
    sched, _ = optimizer_factory({"optimizer": "Adam", "lr": 0.1}, model.parameters())
    train.fit(model, (_train_on_batch, None), sched, _Quiet(model.parameters(), lr=0.1), [{"t": torch.ones(3)}], [], cfg,
              str(tmp_path), args, "cpu", log=lambda *a: lines.append(" ".join(str(x) for x in a)))
    assert len(lines) == 1 and "gradient norm" not in lines[0]


# ---------------------------------------------------------------------------------------------------------- the header's boundary
def test_the_header_declares_four_entries_the_library_exports_them_and_the_flags_reach_the_trainer():
    import ctypes
    from nsdp_amd import _lib, build
    entries = ["nsdp_adam_multi_clipped_f32", "nsdp_grad_clip_finalize", "nsdp_grad_sumsq_f32", "nsdp_grad_sumsq_workspace_bytes"]
    assert _lib.declared_symbols("nsdp_optim.h") == entries
    assert not set(entries) & set(_lib.declared_symbols())          # (nsdp_hip.h keeps its own table of entries)
    assert build.PER_FILE["adam.hip"] == build.EXACT               # one rounding per operation, in the sum and in g * coef
    so = ctypes.CDLL(_lib.SO_PATH)
    assert so.nsdp_abi_version() >= 25 and all(hasattr(so, e) for e in entries)
    so.nsdp_grad_sumsq_workspace_bytes.restype = ctypes.c_size_t
    assert [so.nsdp_grad_sumsq_workspace_bytes(ctypes.c_int(n)) for n in (-1, 0, 1, 4097)] == [0, 0, 8, 8 * 4097]
    so.nsdp_last_error.restype = ctypes.c_char_p
    # refused on the host, before anything is launched: no GPU is needed to be told
    assert so.nsdp_grad_clip_finalize(None, 0, ctypes.c_double(-1.0), 0, None, None) != 0
    assert b"max_norm" in so.nsdp_last_error()
    assert so.nsdp_grad_clip_finalize(None, 0, ctypes.c_double(1.0), 0, None, None) != 0
    assert b"clip state" in so.nsdp_last_error()


def test_the_command_line_flags_override_the_config(tmp_path, monkeypatch):
    import yaml
    seen = {}

    def fake_factory(training, parameters):
        seen.update(training)
        raise SystemExit(0)                      # nothing below optimizer_factory matters for this test
    monkeypatch.setattr(train, "build_model", lambda config, *a, **k: (_Stub(), None, None, None))
    monkeypatch.setattr(train, "optimizer_factory", fake_factory)
    path = tmp_path / "c.yaml"
    path.write_text(yaml.safe_dump({"model": {"type": "forward"}, "training": {"clip_grad_norm": 5.0}, "validation": {}}))
    for flags, want in (([], (5.0, None)), (["--clip-grad-norm", "0.25"], (0.25, None)), (["--skip-nonfinite"], (5.0, True))):
        seen.clear()
        with pytest.raises(SystemExit):
            train.main([str(path), str(tmp_path / "exp")] + flags)
        assert (seen.get("clip_grad_norm"), seen.get("skip_nonfinite_steps")) == want
