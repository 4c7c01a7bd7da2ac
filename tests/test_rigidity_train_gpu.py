"""Training with ``config["training"]["rigidity"]`` (nsdp_amd/rigidity.py wired into the step functions), at the tiny
configuration of the train-step tests (tests/helpers.py: 128 query points per shape), for the forward and the arbitrary model
types and under ``loss: l2`` and ``loss: chamfer``: the step's loss as the sum of its two terms bit for bit, its parameter
gradients against the regulariser composed from existing operations on the same indices, the replayed step against the eager
one bit for bit, the untouched step of a config without the key, and validation."""
import pytest
import torch

from helpers import build_product, fixture_setup, nondeterministic_knobs, restore_model, run_forward, snapshot_model, to_dev

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")

CASES = [("forward", "l2", 4, 1.0), ("forward", "chamfer", 8, 0.5), ("arbitrary", "l2", 8, 2.0), ("arbitrary", "chamfer", 16, 1.0)]


def _setup(mtype, training=None):
    _, cfg, seed, data = fixture_setup("tiny_" + mtype, mtype)
    if training is not None:
        cfg = dict(cfg, training=training)
    model, train_fn, _ = build_product(cfg, seed, DEV)
    model.train()
    return cfg, model, train_fn, to_dev(data, DEV)


def _grads(model):
    return {k: p.grad.detach().clone() for k, p in model.named_parameters() if p.grad is not None}


def _assert_gradients_close(got, want):
    """The tolerance the train-step tests give gradient norms and samples (tests/test_model_gpu.py: 3e-3 relative + 2e-5 on the
    norm; samples 5e-3 relative + 1e-4 of the norm + 1.5e-5 + 3e-3 of the largest sample), here on every entry -- as copied in
    tests/test_chamfer_train_gpu.py."""
    assert got.keys() == want.keys()
    for k in want:
        gn, mine = float(want[k].double().norm()), float(got[k].double().norm())
        assert abs(mine - gn) <= 3e-3 * gn + 2e-5, (k, mine, gn)
        atol = 1e-4 * gn + 1.5e-5 + 3e-3 * float(want[k].abs().max())
        assert bool(((got[k] - want[k]).abs() <= 5e-3 * want[k].abs() + atol).all()), k


@pytest.mark.parametrize("mtype,loss_name,k,weight", CASES)
def test_step_loss_is_the_sum_and_its_gradients_equal_the_composed_regulariser(mtype, loss_name, k, weight):
    from nsdp_amd import chamfer, rigidity
    cfg, model, train_fn, data = _setup(mtype, {"loss": loss_name, "rigidity": {"weight": weight, "k": k}})
    src, tgt = data["space_samples_src"], data["space_samples_tgt"]
    assert k + 1 < src.shape[1]
    model.zero_grad(set_to_none=True)
    loss = train_fn.loss_fn(model, data, cfg)
    loss.backward()
    got = _grads(model)
    # the two terms evaluated separately on the same train-mode prediction (batch statistics: the same prediction again)
    model.zero_grad(set_to_none=True)
    pred = run_forward(model, cfg, data)
    with torch.no_grad():
        data_term = chamfer.training_loss(cfg)(pred.detach(), tgt)
        reg = rigidity.local_rigidity_loss(pred.detach(), src, k=k, weight=weight)
        assert float(reg) > 0 and torch.equal(loss.detach(), data_term + reg)
    # autograd through the composed regulariser on the same indices
    idx = rigidity.neighbour_sets(src, k)
    partner = chamfer.training_loss(cfg)(pred, tgt) + rigidity.composed_loss(pred, src, idx, weight)
    partner.backward()
    torch.cuda.synchronize()
    loss, partner = loss.item(), partner.item()
    assert abs(loss - partner) <= 2e-5 * max(1.0, abs(loss)), (loss, partner)
    assert len(got) > 20
    _assert_gradients_close(got, _grads(model))


@pytest.mark.parametrize("mtype,loss_name,k", [("forward", "l2", 4), ("arbitrary", "chamfer", 16)])
def test_replayed_step_is_bit_equal_to_the_eager_step(mtype, loss_name, k, monkeypatch):
    """The regularised step under the race detector of tests/test_graph_exec_gpu.py: captured (the self-search, the list build --
    the one-workgroup entry at k = 4, 512 entries, the many-workgroup entry at k = 16 -- and the rigidity kernels are nodes of
    the graph) and replayed on 1 and 2 streams, it reproduces the eager step's loss, every gradient, weight and BatchNorm buffer
    bit for bit, for two consecutive steps."""
    if nondeterministic_knobs():
        pytest.skip("the step is not bit-reproducible under " + ", ".join(nondeterministic_knobs()))
    from nsdp_amd import hip_linear
    from nsdp_amd.graph_step import GraphedStep, capturable_adam
    from nsdp_amd.model import optimizer_factory
    if hip_linear._OVERLAP_WGRAD == "auto":      # (eager and captured steps take the weight-gradient stream alike)
        monkeypatch.setattr(hip_linear, "_OVERLAP_WGRAD", True)
    cfg, model, train_fn, data = _setup(mtype, {"loss": loss_name, "rigidity": {"weight": 1.0, "k": k}})
    _, opt = optimizer_factory({"optimizer": "Adam", "lr": 5e-5}, model.parameters())
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
            out.append({"loss": loss.detach().clone(), "grads": _grads(model), "state": snapshot_model(model)})
        return out

    def diff(a, b):
        bad = []
        for i, (x, y) in enumerate(zip(a, b)):
            if not torch.equal(x["loss"], y["loss"]):
                bad.append(f"step {i} loss {float(x['loss'])!r} vs {float(y['loss'])!r}")
            assert x["grads"].keys() == y["grads"].keys()
            bad += [f"step {i} grad {k}" for k in x["grads"] if not torch.equal(x["grads"][k], y["grads"][k])]
            bad += [f"step {i} state {k}" for k in x["state"] if not torch.equal(x["state"][k], y["state"][k])]
        return bad

    eager = two_steps(step)
    assert float(eager[0]["loss"]) > 0
    again = diff(eager, two_steps(step))
    assert not again, f"the eager regularised step is not deterministic: {len(again)} tensors differ, first {again[:6]}"
    for streams in (1, 2):
        restore_model(model, snap, opt)
        gs = GraphedStep(step, max_streams=streams).capture(warmup=0)      # (a capture executes nothing)
        bad = diff(eager, two_steps(gs))
        assert not bad, f"replay on {streams} stream(s) vs eager: {len(bad)} tensors differ, first: {bad[:8]}"
        gs.close()


def _plain_run(mtype, training):
    """One eager step and one replay of the captured step of a fresh model: ``training`` = "written out" for today's step spelled
    out with ``chamfer.training_loss`` alone, else the ``training`` section (or None: no such section) handed to the step
    function.  Nothing of the model outlives the call (a captured step rebuilds the weight packs of every live model)."""
    from nsdp_amd import chamfer
    from nsdp_amd.graph_step import GraphedStep, capturable_adam
    from nsdp_amd.model import optimizer_factory
    cfg, model, train_fn, data = _setup(mtype, training if isinstance(training, dict) else None)
    _, opt = optimizer_factory({"optimizer": "Adam", "lr": 5e-5}, model.parameters())
    capturable_adam(opt)

    def written_out():
        opt.zero_grad()
        loss = chamfer.training_loss(cfg)(run_forward(model, cfg, data), data["space_samples_tgt"])
        loss.backward()
        opt.step()
        return loss

    step = written_out if training == "written out" else (lambda: train_fn.tensor_step(model, opt, data, cfg))
    snap = snapshot_model(model)
    eager = step().detach().clone()
    torch.cuda.synchronize()
    grads = _grads(model)
    restore_model(model, snap, opt)
    gs = GraphedStep(step, max_streams=2).capture(warmup=0)
    replayed = gs().detach().clone()
    torch.cuda.synchronize()
    out = {"info": dict(gs.info), "eager": eager, "replayed": replayed, "grads": grads, "replayed_grads": _grads(model)}
    gs.close()
    gs.fn = None
    return out


@pytest.mark.parametrize("mtype", ["forward", "arbitrary"])
def test_a_config_without_the_key_is_todays_step(mtype, monkeypatch):
    """No ``training.rigidity`` (and ``None``): the step is today's -- the same bits and, captured, the same number of graph
    nodes as the step written out without the regulariser, compared in this process, with every rigidity entry patched to
    raise."""
    import gc
    from nsdp_amd import rigidity

    def never(*args, **kwargs):
        raise AssertionError("a step without training.rigidity came near the rigidity loss")

    for name in ("local_rigidity_loss", "neighbour_sets", "forward_raw", "backward_raw"):
        monkeypatch.setattr(rigidity, name, never)
    runs = []
    for training in ("written out", None, {"rigidity": None}, {"loss": "l2"}):
        gc.collect()
        runs.append(_plain_run(mtype, training))
        print(training, runs[-1]["info"])
    base = runs[0]
    for run in runs[1:]:
        assert run["info"]["nodes"] == base["info"]["nodes"] and run["info"]["kernels"] == base["info"]["kernels"], (run["info"], base["info"])
        assert torch.equal(run["eager"], base["eager"]) and torch.equal(run["replayed"], base["replayed"])
        for key in ("grads", "replayed_grads"):
            assert run[key].keys() == base[key].keys()
            assert all(torch.equal(run[key][k], base[key][k]) for k in base[key]), key


@pytest.mark.parametrize("mtype,loss_name", [("forward", "chamfer"), ("arbitrary", "l2")])
def test_validation_reports_the_sum(mtype, loss_name):
    from nsdp_amd import chamfer, rigidity
    from nsdp_amd.model.deformation_networks import validate_on_batch_with_cano
    from nsdp_amd.model.flow_arbitrary import validate_on_batch_with_arbitrary
    validate = validate_on_batch_with_arbitrary if mtype == "arbitrary" else validate_on_batch_with_cano
    cfg, model, _, data = _setup(mtype, {"loss": loss_name})
    model.eval()
    with torch.no_grad():
        pred = run_forward(model, cfg, data)
        data_term = chamfer.training_loss(cfg)(pred, data["space_samples_tgt"])
        reg = rigidity.local_rigidity_loss(pred, data["space_samples_src"], k=6, weight=0.75)
    with_key = dict(cfg, training={"loss": loss_name, "rigidity": {"weight": 0.75, "k": 6}})
    got = validate(model, data, with_key)
    assert float(reg) > 0 and got == float(data_term + reg)
    assert validate(model, data, cfg) == float(data_term) != got
