"""Training with ``training.clip_grad_norm`` / ``skip_nonfinite_steps`` at the tiny configuration of the train-step tests
(tests/helpers.py), for the forward and the arbitrary model types, as tests/test_rigidity_train_gpu.py holds the rigidity key:
the replayed clipped step against the eager one bit for bit, and a bound out of reach against the step of a config without the
key -- the same bits, and a captured step that is longer by exactly the norm launch and the finalize."""
import gc
import os

import pytest
import torch

from helpers import build_product, fixture_setup, nondeterministic_knobs, restore_model, snapshot_model, to_dev

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
HIP_ADAM = os.environ.get("NSDP_HIP_ADAM", "1") != "0"
OPT = {"optimizer": "Adam", "lr": 5e-5}


def _setup(mtype):
    _, cfg, seed, data = fixture_setup("tiny_" + mtype, mtype)
    model, train_fn, _ = build_product(cfg, seed, DEV)
    model.train()
    return cfg, model, train_fn, to_dev(data, DEV)


def _grads(model):
    return {k: p.grad.detach().clone() for k, p in model.named_parameters() if p.grad is not None}


@pytest.mark.skipif(not HIP_ADAM, reason="NSDP_HIP_ADAM=0: the host-side clip reads the norm and cannot be captured")
@pytest.mark.parametrize("mtype", ["forward", "arbitrary"])
def test_replayed_clipped_step_is_bit_equal_to_the_eager_step(mtype, monkeypatch):
    """A bound far below the gradient norm (coef < 1, read from grad_stats()): captured -- the norm launch, the finalize and the
    clipped update are nodes of the graph -- and replayed on 1 and 2 streams, two consecutive steps reproduce the eager steps'
    loss, every gradient, weight and BatchNorm buffer bit for bit."""
    if nondeterministic_knobs():
        pytest.skip("the step is not bit-reproducible under " + ", ".join(nondeterministic_knobs()))
    from nsdp_amd import hip_linear
    from nsdp_amd.graph_step import GraphedStep, capturable_adam
    from nsdp_amd.hip_adam import HipAdam
    from nsdp_amd.model import optimizer_factory
    if hip_linear._OVERLAP_WGRAD == "auto":      # (eager and captured steps take the weight-gradient stream alike)
        monkeypatch.setattr(hip_linear, "_OVERLAP_WGRAD", True)
    cfg, model, train_fn, data = _setup(mtype)
    _, opt = optimizer_factory(dict(OPT, clip_grad_norm=1e-4, skip_nonfinite_steps=True), model.parameters())
    assert isinstance(opt, HipAdam) and opt.clips
    capturable_adam(opt)

    def step():
        return train_fn.tensor_step(model, opt, data, cfg)

    snap = snapshot_model(model)
    step()                                     # creates the optimizer state (a capture must find it in place)
    torch.cuda.synchronize()

    def two_steps(run):
        restore_model(model, snap, opt)
        out = []
        for _ in range(2):
            loss = run()
            torch.cuda.synchronize()
            st = opt.grad_stats()
            assert st["coef"] < 1.0 and st["norm"] > 1e-4 and st["skipped"] == 0
            out.append({"loss": loss.detach().clone(), "grads": _grads(model), "state": snapshot_model(model),
                        "stats": (st["norm"], st["coef"])})
        return out

    def diff(a, b):
        bad = []
        for i, (x, y) in enumerate(zip(a, b)):
            if not torch.equal(x["loss"], y["loss"]):
                bad.append(f"step {i} loss {float(x['loss'])!r} vs {float(y['loss'])!r}")
            if x["stats"] != y["stats"]:
                bad.append(f"step {i} norm / coef {x['stats']} vs {y['stats']}")
            assert x["grads"].keys() == y["grads"].keys()
            bad += [f"step {i} grad {k}" for k in x["grads"] if not torch.equal(x["grads"][k], y["grads"][k])]
            bad += [f"step {i} state {k}" for k in x["state"] if not torch.equal(x["state"][k], y["state"][k])]
        return bad

    eager = two_steps(step)
    assert float(eager[0]["loss"]) > 0
    weights = {k for k, _ in model.named_parameters()}
    moved = [k for k in weights if not torch.equal(snap[k], eager[1]["state"][k])]
    assert len(moved) > 20                     # (a clipped step is still a step)
    for streams in (1, 2):
        restore_model(model, snap, opt)
        gs = GraphedStep(step, max_streams=streams).capture(warmup=0)      # (a capture executes nothing)
        bad = diff(eager, two_steps(gs))
        assert not bad, f"replay on {streams} stream(s) vs eager: {len(bad)} tensors differ, first: {bad[:8]}"
        gs.close()


def _run(mtype, keys):
    """One eager step, then (HipAdam only) one replay of the captured step from the same start, on a fresh model."""
    from nsdp_amd.graph_step import GraphedStep, capturable_adam
    from nsdp_amd.model import optimizer_factory
    cfg, model, train_fn, data = _setup(mtype)
    _, opt = optimizer_factory(dict(OPT, **keys), model.parameters())
    capturable_adam(opt)

    def step():
        return train_fn.tensor_step(model, opt, data, cfg)

    snap = snapshot_model(model)
    out = {"eager": step().detach().clone()}
    torch.cuda.synchronize()
    out["eager_state"] = snapshot_model(model)
    out["stats"] = opt.grad_stats() if hasattr(opt, "grad_stats") else None      # (None too: HipAdam built without the keys)
    if HIP_ADAM:
        restore_model(model, snap, opt)
        gs = GraphedStep(step, max_streams=2).capture(warmup=0)
        out["replayed"] = gs().detach().clone()
        torch.cuda.synchronize()
        out["replayed_state"] = snapshot_model(model)
        out["info"] = dict(gs.info)
        gs.close()
        gs.fn = None
    return out


@pytest.mark.parametrize("mtype", ["forward", "arbitrary"])
def test_a_bound_out_of_reach_is_the_step_of_a_config_without_the_key(mtype):
    runs = []
    for keys in ({}, {"clip_grad_norm": 1e30, "skip_nonfinite_steps": True}):
        gc.collect()
        runs.append(_run(mtype, keys))
    base, clipped = runs
    assert base["stats"] is None and clipped["stats"]["coef"] == 1.0 and clipped["stats"]["clipped"] == 0
    for key in ("eager", "replayed") if HIP_ADAM else ("eager",):
        assert torch.equal(base[key], clipped[key])
        a, b = base[key + "_state"], clipped[key + "_state"]
        assert a.keys() == b.keys() and all(torch.equal(a[k], b[k]) for k in a), key
    if HIP_ADAM:
        # one parameter group: one norm launch + the finalize; the update stays one node
        assert clipped["info"]["nodes"] == base["info"]["nodes"] + 2, (clipped["info"], base["info"])
        assert clipped["info"]["kernels"] == base["info"]["kernels"] + 2


@pytest.mark.skipif(not HIP_ADAM, reason="NSDP_HIP_ADAM=0: the host-side clip reads the norm and cannot be captured")
def test_the_data_parallel_form_of_the_replayed_step_clips_like_the_eager_loop():
    """GraphedTrainOnBatch(reducer=): the optimizer step is a captured graph of its OWN behind the exchange, and every gradient a
    view into the reducer's flat buffer (4-byte granular offsets: the scalar-load paths).  One rank, no process group -- the
    exchange is skipped, the graphs and the views are the data-parallel job's.  Losses step for step, the weights and the
    optimizer's statistics equal the plain eager loop's: the sum of squares does not depend on where a gradient lives."""
    if nondeterministic_knobs():
        pytest.skip("the step is not bit-reproducible under " + ", ".join(nondeterministic_knobs()))
    from helpers import model_cfg
    from nsdp_amd import train
    from nsdp_amd.graph_step import GraphedTrainOnBatch, capturable_adam
    from nsdp_amd.model import build_model, optimizer_factory
    from nsdp_amd.parallel import GradAllReducer
    cfg = model_cfg("forward", [256, 64, 16])
    cfg["training"] = dict(OPT, lr=5e-4, clip_grad_norm=1e-3, skip_nonfinite_steps=True)
    batches = [{k: v.to(DEV) for k, v in b.items()} for b in train.SyntheticLoader(5, 3, 2, n_surf=256, n_query=128)]
    seq = [batches[i % 3] for i in range(5)]
    runs = []
    for mode in ("eager", "two graphs", "three graphs"):
        train.seed_everything(31)
        model, train_fn, _, _ = build_model(cfg, device=DEV)
        model.train()
        _, opt = optimizer_factory(cfg["training"], model.parameters())
        capturable_adam(opt)
        fn = train_fn
        if mode != "eager":
            fn = GraphedTrainOnBatch(train_fn, reducer=GradAllReducer(model, 1), overlap=(mode == "three graphs"))
        losses = [fn(model, opt, b, cfg) for b in seq]
        torch.cuda.synchronize()
        if mode != "eager":
            assert fn.replays == len(seq) - 1 and fn._update is not None and (fn._tail is not None) == (mode == "three graphs")
            assert fn._update.info["kernels"] == 3                       # norm, finalize, update: the whole captured optimizer step
            assert any(p.grad.data_ptr() % 16 for p in model.parameters())      # (some views ARE misaligned)
        runs.append((losses, snapshot_model(model), opt.clip_state()))
        del fn
        gc.collect()
    (l0, w0, s0) = runs[0]
    assert s0["steps"] == 5 and s0["clipped"] == 5 and s0["coef"] < 1.0
    for losses, weights, stats in runs[1:]:
        assert losses == l0
        assert stats == s0
        assert all(torch.equal(weights[k], w0[k]) for k in w0)
