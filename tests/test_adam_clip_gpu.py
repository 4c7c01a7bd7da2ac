"""HipAdam(max_grad_norm=, skip_nonfinite=) on the GPU (include/nsdp_optim.h, csrc/adam.hip) against the host reference of
tests/adam_clip_ref.py: the sum of squares bit for bit in the written order, the rule, the update on g * coef, skipped steps,
replay and the step pre-hook.  Shapes: the list of tests/test_adam_gpu.py; with ``misaligned`` every other parameter AND its
gradient are views 4 bytes into their allocations (the scalar-load paths)."""
import math

import numpy as np
import pytest
import torch

import adam_clip_ref as ref

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
KW = dict(lr=5e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0)
SKIP = {2, 6}


def _on_device(t, misaligned):
    if not misaligned:
        return t.to(DEV)
    flat = torch.zeros(t.numel() + 1, device=DEV)
    flat[1:] = t.reshape(-1).to(DEV)
    out = flat[1:].view(t.shape)
    assert out.data_ptr() % 16 == 4
    return out


def _params(values, misaligned=False):
    return [_on_device(v, misaligned and i % 2 == 1).requires_grad_(True) for i, v in enumerate(values)]


def _feed(params, gs, misaligned=False):
    for i, (p, g) in enumerate(zip(params, gs)):
        p.grad = None if g is None else _on_device(g, misaligned and i % 2 == 1)


def _sequence(seed, steps, skip=()):
    return [[None if i in skip else g for i, g in enumerate(ref.grads(seed, t))] for t in range(steps)]


def _bits(t):
    return t.detach().contiguous().view(torch.int32)


def _same_bits(a, b):
    return torch.equal(_bits(a), _bits(b))


def _assert_state_bit_equal(pa, oa, pb, ob):
    for x, y in zip(pa, pb):
        assert _same_bits(x, y)
        assert oa.state[x].keys() == ob.state[y].keys()
        for k in oa.state[x]:
            assert _same_bits(oa.state[x][k], ob.state[y][k]), k


def _f32_ulp(x):
    return float(np.spacing(np.float32(abs(x))))


def _sumsq_on_device(gs, misaligned):
    from nsdp_amd.hip_adam import HipAdam
    params = _params([torch.zeros(s) for s in ref.SHAPES], misaligned)
    opt = HipAdam(params, max_grad_norm=1.0, **KW)
    _feed(params, gs, misaligned)
    opt.step()
    return opt.clip_state()["sumsq"], opt, params


def test_sum_of_squares_is_the_references_ordered_sum_bit_for_bit():
    gs = ref.grads(7, 0)
    want = ref.ordered_sumsq(gs)
    got, opt, _ = _sumsq_on_device(gs, False)
    assert got == want
    exact = math.fsum((np.concatenate([g.reshape(-1).numpy() for g in gs]).astype(np.float64) ** 2).tolist())
    assert abs(got - exact) <= ref.NUMEL * 2.0 ** -53 * exact
    assert _sumsq_on_device(gs, True)[0] == got                     # the same values 4 bytes off: the same bits
    opt.step()
    assert opt.clip_state()["sumsq"] == got                         # and again
    st = opt.grad_stats()
    assert sorted(st) == ["clipped", "coef", "norm", "skipped", "steps"] and st["steps"] == 2
    assert st["norm"] == float(np.float32(math.sqrt(want)))
    # integer-valued gradients: every partial sum is an integer below 2^53 -- exact in any order
    g = torch.Generator().manual_seed(3)
    ints = [torch.randint(-1000, 1001, shp, generator=g).float() for shp in ref.SHAPES]
    total = float(sum(int((t.long() ** 2).sum()) for t in ints))
    assert _sumsq_on_device(ints, False)[0] == total == _sumsq_on_device(ints, True)[0]


@pytest.mark.parametrize("misaligned", [False, True])
def test_one_nonzero_element_anywhere_is_found(misaligned):
    """A dropped tail, chunk edge or misaligned prefix loses exactly such an element."""
    from nsdp_amd.hip_adam import HipAdam
    params = _params([torch.zeros(s) for s in ref.SHAPES], misaligned)
    opt = HipAdam(params, max_grad_norm=1.0, **KW)
    _feed(params, [torch.zeros(s) for s in ref.SHAPES], misaligned)
    tried = 0
    for p in params:
        flat = p.grad.view(-1)
        for at in sorted({0, 4095, 4096, flat.numel() - 1}):
            if at >= flat.numel():
                continue
            flat[at] = 3.25
            opt.step()
            assert opt.clip_state()["sumsq"] == 3.25 ** 2, (tuple(p.shape), at)
            flat[at] = 0.0
            tried += 1
    assert tried > 25


def test_parameters_without_a_gradient_add_nothing_and_get_no_state():
    from nsdp_amd.hip_adam import HipAdam
    gs = _sequence(7, 1, SKIP)[0]
    params = _params(ref.params(3), True)
    opt = HipAdam(params, max_grad_norm=1.0, **KW)
    before = [p.detach().clone() for p in params]
    _feed(params, gs, True)
    opt.step()
    assert opt.clip_state()["sumsq"] == ref.ordered_sumsq(gs)
    for i, p in enumerate(params):
        assert (len(opt.state[p]) == 0 and _same_bits(p, before[i])) if i in SKIP else float(opt.state[p]["step"]) == 1.0


@pytest.mark.parametrize("misaligned", [False, True])
def test_within_the_bound_the_step_is_the_unclipped_launch_bit_for_bit(misaligned):
    from nsdp_amd.hip_adam import HipAdam
    seq = _sequence(7, 12, SKIP)
    bound = 10.0 * max(math.sqrt(ref.ordered_sumsq(gs)) for gs in seq)
    assert all(ref.rule(ref.ordered_sumsq(gs), bound)[1] == np.float32(1.0) for gs in seq)
    a, b = _params(ref.params(3), misaligned), _params(ref.params(3), misaligned)
    plain, clipped = HipAdam(a, **KW), HipAdam(b, max_grad_norm=bound, skip_nonfinite=True, **KW)
    for gs in seq:
        _feed(a, gs, misaligned)
        _feed(b, gs, misaligned)
        plain.step()
        clipped.step()
    _assert_state_bit_equal(a, plain, b, clipped)
    st = clipped.grad_stats()
    assert (st["steps"], st["clipped"], st["skipped"], st["coef"]) == (12, 0, 0, 1.0)
    assert float(clipped.state[b[0]]["step"]) == 12.0
    assert plain.grad_stats() is None
    with pytest.raises(RuntimeError, match="max_grad_norm"):
        plain.clip_state()


@pytest.mark.parametrize("weight_decay,misaligned,lr_tensor", [(0.0, False, False), (0.01, True, True)])
def test_beyond_the_bound_the_update_runs_on_the_scaled_gradient(weight_decay, misaligned, lr_tensor):
    from nsdp_amd.hip_adam import HipAdam
    kw = dict(KW, weight_decay=weight_decay)
    seq = _sequence(7, 12, SKIP)
    bound = 0.1 * min(math.sqrt(ref.ordered_sumsq(gs)) for gs in seq)
    # (with weight decay the initial parameters take the signs of the first gradient: where g * coef + wd * p cancels, Adam's
    # first step is ill-conditioned on EITHER device -- adam_clip_ref.params_agreeing_with has the figures)
    values = ref.params_agreeing_with(ref.params(3), seq[0]) if weight_decay else ref.params(3)
    cpu, want, log = ref.run(values, seq, max_norm=bound, **kw)
    assert all(coef < 1.0 and apply for _, _, coef, apply in log)
    gpu = _params(values, misaligned)
    opt = HipAdam(gpu, max_grad_norm=bound, **kw)
    if lr_tensor:
        opt.param_groups[0]["lr"] = torch.tensor(kw["lr"], dtype=torch.float32, device=DEV)
    for gs, (S, norm, coef, _) in zip(seq, log):
        _feed(gpu, gs, misaligned)
        kept = [None if p.grad is None else p.grad.clone() for p in gpu]
        opt.step()
        st = opt.clip_state()
        assert st["sumsq"] == S and st["apply"] == 1
        assert abs(st["coef"] - float(coef)) <= _f32_ulp(coef) and st["coef"] < 1.0
        assert all(k is None or _same_bits(p.grad, k) for p, k in zip(gpu, kept))      # p.grad is NOT rewritten
    assert opt.grad_stats()["clipped"] == 12
    for i, (a, b) in enumerate(zip(cpu, gpu)):
        if i in SKIP:
            assert len(opt.state[b]) == 0 and torch.equal(a.detach(), b.detach().cpu())
            continue
        sa, sb = want.state[a], opt.state[b]
        assert float(sb["step"]) == 12.0
        # the tolerances of tests/test_adam_gpu.py (the CPU's vectorised lerp_ / addcmul_ may fuse; |p| < 8, updates of 5e-4)
        for name in ("exp_avg", "exp_avg_sq"):
            torch.testing.assert_close(sb[name].cpu(), sa[name], rtol=1e-6, atol=4e-7 * float(sa[name].abs().max()))
        torch.testing.assert_close(b.detach().cpu(), a.detach(), rtol=0, atol=6e-7)


def _poisoned(seq, step, tensor, element, value):
    seq = [list(gs) for gs in seq]
    g = seq[step][tensor].clone()
    g.view(-1)[element] = value
    seq[step][tensor] = g
    return seq


@pytest.mark.parametrize("tensor,element,value", [(10, 70000, float("inf")), (10, 4096, float("nan"))])
def test_a_non_finite_gradient_is_skipped_or_is_torchs(tensor, element, value):
    from nsdp_amd.hip_adam import HipAdam
    clean = _sequence(7, 9)
    bound = 0.1 * min(math.sqrt(ref.ordered_sumsq(gs)) for gs in clean)
    seq = _poisoned(clean, 4, tensor, element, value)
    # with the guard: step 4 changes nothing, and steps 5 .. 8 are those of a run that never saw it
    a, b = _params(ref.params(3), True), _params(ref.params(3), True)
    guarded = HipAdam(a, max_grad_norm=bound, skip_nonfinite=True, **KW)
    never = HipAdam(b, max_grad_norm=bound, skip_nonfinite=True, **KW)
    for t, gs in enumerate(seq):
        _feed(a, gs, True)
        if t == 4:
            before = ([p.detach().clone() for p in a], [{k: v.clone() for k, v in guarded.state[p].items()} for p in a])
        guarded.step()
        if t == 4:
            st = guarded.clip_state()
            assert (st["apply"], st["skipped"], st["steps"], st["clipped"]) == (0, 1, 5, 4) and not math.isfinite(st["sumsq"])
            for p, v, s in zip(a, *before):
                assert _same_bits(p, v) and all(_same_bits(guarded.state[p][k], s[k]) for k in s)
                assert float(guarded.state[p]["step"]) == 4.0
            assert int(guarded._plans[0]["done"].abs().sum()) == 0
            continue
        _feed(b, gs, True)
        never.step()
    _assert_state_bit_equal(a, guarded, b, never)
    assert guarded.grad_stats()["skipped"] == 1 and never.grad_stats()["skipped"] == 0
    assert float(guarded.state[a[0]]["step"]) == 8.0
    # without it: NaNs exactly where clip_grad_norm_ + Adam put them
    cpu, want, log = ref.run(ref.params(3), seq[:5], max_norm=bound, **KW)
    assert log[4][3] and (math.isnan(log[4][2]) if math.isnan(value) else log[4][2] == 0.0)
    c = _params(ref.params(3), True)
    bare = HipAdam(c, max_grad_norm=bound, **KW)
    for gs in seq[:5]:
        _feed(c, gs, True)
        bare.step()
    st = bare.clip_state()
    assert st["apply"] == 1 and st["skipped"] == 0 and (math.isnan(st["coef"]) if math.isnan(value) else st["coef"] == 0.0)
    n_nan = 0
    for x, y in zip(cpu, c):
        assert torch.equal(torch.isnan(x.detach()), torch.isnan(y.detach().cpu()))
        for k in ("exp_avg", "exp_avg_sq"):
            assert torch.equal(torch.isnan(want.state[x][k]), torch.isnan(bare.state[y][k].cpu())), k
        n_nan += int(torch.isnan(y).sum())
    assert n_nan == (1 if math.isinf(value) else ref.NUMEL)


def test_replayed_clipped_step_equals_eager():
    """tests/test_adam_gpu.py's replay test with clipping active, a learning-rate change between replays and one non-finite step
    INSIDE the replayed sequence: the decision is made on the device, so the replay skips it as the eager step does."""
    from nsdp_amd.graph_step import GraphedStep, set_lr
    from nsdp_amd.hip_adam import HipAdam
    kw = dict(KW, lr=1e-3)
    seq = _poisoned([ref.grads(11, t) for t in range(6)], 4, 10, 70000, float("inf"))
    bound = 0.1 * min(math.sqrt(ref.ordered_sumsq(gs)) for gs in seq if math.isfinite(ref.ordered_sumsq(gs)))
    a, b = _params(ref.params(9)), _params(ref.params(9))
    static = [torch.zeros_like(p) for p in b]
    oa = HipAdam(a, max_grad_norm=bound, skip_nonfinite=True, **kw)
    ob = HipAdam(b, max_grad_norm=bound, skip_nonfinite=True, **kw)
    for o in (oa, ob):
        o.param_groups[0]["lr"] = torch.tensor(1e-3, dtype=torch.float32, device=DEV)

    def feed(t):
        for p, s, g in zip(a, static, seq[t]):
            p.grad = g.to(DEV)
            s.copy_(g)
    feed(0)
    for p, s in zip(b, static):
        p.grad = s.clone()
    oa.step()
    ob.step()                       # (first step eagerly: creates the state and the spare pinned table)

    def captured():
        for p, s in zip(b, static):
            p.grad = s * 1.0        # gradients born inside the graph's pool: tables and partials are rebuilt in the capture
        ob.step()
    step = GraphedStep(captured).capture(warmup=0)
    for t in range(1, 6):
        if t == 3:
            set_lr(oa, 2e-4)
            set_lr(ob, 2e-4)
        feed(t)
        oa.step()
        step()
        if t == 4:
            assert oa.clip_state()["apply"] == 0 == ob.clip_state()["apply"]
    torch.cuda.synchronize()
    sa, sb = oa.clip_state(), ob.clip_state()
    step.close()
    _assert_state_bit_equal(a, oa, b, ob)
    assert float(ob.state[b[0]]["step"]) == 5.0
    assert sa == sb and oa.grad_stats() == ob.grad_stats()
    assert (sb["steps"], sb["clipped"], sb["skipped"]) == (6, 5, 1)


def test_a_step_pre_hook_is_seen_by_the_norm():
    """The data-parallel exchange is a step pre-hook: what it leaves in p.grad is what the norm is taken of."""
    from nsdp_amd.hip_adam import HipAdam
    seq = _sequence(7, 3)
    bound = 0.5 * min(math.sqrt(ref.ordered_sumsq([10.0 * g for g in gs])) for gs in seq)
    a, b = _params(ref.params(3), True), _params(ref.params(3), True)
    hooked, fed = HipAdam(a, max_grad_norm=bound, **KW), HipAdam(b, max_grad_norm=bound, **KW)
    hooked.register_step_pre_hook(lambda *_: [p.grad.mul_(10.0) for p in a] and None)
    for gs in seq:
        _feed(a, gs, True)
        _feed(b, [10.0 * g for g in gs], True)
        hooked.step()
        fed.step()
        assert hooked.clip_state() == fed.clip_state() and fed.clip_state()["coef"] < 1.0
    _assert_state_bit_equal(a, hooked, b, fed)


def test_several_parameter_groups_share_one_norm():
    """Two groups (the sum once per group into consecutive ranges of one partials buffer, ONE finalize, two updates): the norm is
    that of all gradients together -- the bits of the one-group optimizer over the same tensors in the same order -- and with
    equal hyper-parameters so is every update; with a group of its own learning rate only that group moves differently."""
    from nsdp_amd.hip_adam import HipAdam
    seq = _sequence(7, 3, SKIP)
    bound = 0.1 * min(math.sqrt(ref.ordered_sumsq(gs)) for gs in seq)
    a, b, c = (_params(ref.params(3), True) for _ in range(3))
    one = HipAdam(a, max_grad_norm=bound, skip_nonfinite=True, **KW)
    two = HipAdam([{"params": b[:5]}, {"params": b[5:]}], max_grad_norm=bound, skip_nonfinite=True, **KW)
    other = HipAdam([{"params": c[:5]}, {"params": c[5:], "lr": 1e-3}], max_grad_norm=bound, skip_nonfinite=True, **KW)
    for gs in seq:
        for params, opt in ((a, one), (b, two), (c, other)):
            _feed(params, gs, True)
            opt.step()
        assert one.clip_state() == two.clip_state() == other.clip_state()
        assert one.clip_state()["sumsq"] == ref.ordered_sumsq(gs) and one.clip_state()["coef"] < 1.0
    _assert_state_bit_equal(a, one, b, two)
    _assert_state_bit_equal(a[:5], one, c[:5], other)
    assert not any(_same_bits(x, y) for i, (x, y) in enumerate(zip(a[5:], c[5:])) if i + 5 not in SKIP)
    assert "max_grad_norm" not in two.state_dict()["param_groups"][1]


def test_bad_settings_are_refused_by_name():
    from nsdp_amd.hip_adam import HipAdam
    for bad in (0.0, -2.0, float("nan")):
        with pytest.raises(ValueError, match="max_grad_norm"):
            HipAdam(_params(ref.params(3)[:2]), max_grad_norm=bad)
    opt = HipAdam(_params(ref.params(3)[:2]), max_grad_norm=float("inf"), skip_nonfinite=True)
    assert opt.clips and "max_grad_norm" not in opt.param_groups[0] and "max_grad_norm" not in opt.state_dict()["param_groups"][0]
