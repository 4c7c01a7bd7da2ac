"""Packed ("ragged") dense inference on the GPU (nsdp_amd.ragged): meshes of different vertex counts decoded in one call get,
row for row, the bits the rectangular calls give them -- the kNN and both fused decoder kernels against their per-shape twins,
the step functions against the same batch padded to [B, max, 3], the per-shape oracle, one captured graph replayed for
different mixes of sizes, the refusals and the ``python -m nsdp_amd.infer --vertex-counts`` command."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from helpers import build_product, l2_err, model_cfg, nondeterministic_knobs, to_dev
from nsdp_amd import hip_decoder, pointnet2_utils as pu, synth
from nsdp_amd.ragged import RaggedPoints, RaggedTestOnBatch
from oracle import tdnet_ref

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = ("surface_samples_tgt_pred", "verts_tgt_pred")
COUNTS = (3001, 0, 1, 15, 16, 17, 255, 256, 257)      # an empty shape, both tile sizes (16, 256) +- 1
TOL_L2 = 1e-4                                         # tests/test_model_gpu.py: the suite's bar against the oracle
SENTINEL = -7.5


def _skip_variants():
    from nsdp_amd import precision
    from nsdp_amd.model import deformation_networks as dn
    knobs = nondeterministic_knobs()
    if not hip_decoder.ENABLED:
        knobs.append("NSDP_FUSED_DECODER=0")      # (refused by the ragged decode: there is no layered ragged path)
    if precision.is_bf16():
        knobs.append("NSDP_STORAGE=bf16")         # (the rectangular twin runs the layered bf16 decoder: other arithmetic)
    if not dn.ENCODE_ONCE:
        knobs.append("NSDP_ENCODE_ONCE=0")
    if knobs:
        pytest.skip("bit equality of ragged and rectangular decodes does not apply under " + ", ".join(knobs))


def _first_difference(a, b):
    rows = (a != b).reshape(a.shape[0], -1).any(-1).nonzero().flatten()
    return f"{rows.numel()} rows differ, first: {rows[:8].tolist()}"


def _clouds(counts, seed, capacity=None):
    pts = [torch.from_numpy(synth.uniform(seed, f"ragged_{b}", (n, 3), -0.5, 0.5)).to(DEV) for b, n in enumerate(counts)]
    return pts, RaggedPoints.from_list(pts, capacity=capacity)


def _setup(mtype, batch, ns, seed):
    cfg = model_cfg(mtype, [min(ns, 2048), 500 if ns >= 2048 else 64, 100 if ns >= 2048 else 16])
    model, _, state = build_product(cfg, seed, DEV)
    model.eval()
    data = synth.make_batch(seed, batch, ns, 4)
    dd = to_dev(data, DEV)
    dd.pop("space_samples_src"), dd.pop("space_samples_tgt")
    dd["surface_samples_src"] = dd["surface_samples_inputs"][:, :, :3].contiguous()
    return cfg, model, dd, state, data


def _step_fn(mtype):
    from nsdp_amd.model.deformation_networks import test_on_batch_with_cano
    from nsdp_amd.model.flow_arbitrary import test_on_batch_with_arbitrary
    return test_on_batch_with_arbitrary if mtype == "arbitrary" else test_on_batch_with_cano


# ---- kernels against their rectangular twins ----------------------------------------------------------------------------

@pytest.mark.parametrize("m,k", [(100, 7), (16, 7)])
def test_knn_ragged_equals_knn_per_shape(m, k):
    pts, r = _clouds(COUNTS, 71)
    src = torch.from_numpy(synth.uniform(72, "anchors", (len(COUNTS), m, 3), -0.5, 0.5)).to(DEV)
    idx, d2 = pu.knn_ragged(r.packed, r.offsets, src, k, return_dist=True)
    assert idx.shape == (r.capacity, k) and idx.dtype == torch.int32 and d2.shape == (r.capacity, k)
    lo = 0
    for b, n in enumerate(COUNTS):
        if n:
            wi, wd = pu.knn(pts[b][None].contiguous(), src[b:b + 1].contiguous(), k, return_dist=True)
            assert torch.equal(idx[lo:lo + n], wi[0]), (b, n, _first_difference(idx[lo:lo + n], wi[0]))
            assert torch.equal(d2[lo:lo + n].view(torch.int32), wd[0].view(torch.int32)), (b, n, _first_difference(d2[lo:lo + n], wd[0]))
        lo += n
    only = pu.knn_ragged(r.packed, r.offsets, src, k)
    assert torch.equal(only, idx)


def _encoding(model, dd):
    with torch.no_grad():
        return model.encode(dd["surface_samples_inputs"])


@pytest.mark.parametrize("mode", ["f32", "bf16"])
def test_decoder_forward_ragged_equals_decoder_forward_per_shape(mode):
    _skip_variants()
    cfg, model, dd, _, _ = _setup("forward", len(COUNTS), 256, 73)
    pts, r = _clouds(COUNTS, 74)
    enc = _encoding(model, dd)
    with torch.no_grad(), hip_decoder.mode(mode):
        out = hip_decoder.decoder_forward_ragged(model.decoder, r, enc)
        assert isinstance(out, RaggedPoints) and out.packed.shape == (r.capacity, 3) and out.offsets is r.offsets
        got = out.split()
        for b, n in enumerate(COUNTS):
            if not n:
                assert got[b].shape == (0, 3)
                continue
            one = {k: v[b:b + 1].contiguous() for k, v in enc.items() if torch.is_tensor(v)}
            want = hip_decoder.decoder_forward(model.decoder, pts[b][None].contiguous(), one)[0]
            assert torch.equal(got[b], want), (mode, b, n, _first_difference(got[b], want))
        # the model-level call is the same call
        via_model = model.decode(r, enc)
        assert isinstance(via_model, RaggedPoints) and torch.equal(via_model.packed, out.packed)
    if mode == "bf16":      # (the two operand types are different kernels: their results must differ somewhere)
        with torch.no_grad():
            f32 = hip_decoder.decoder_forward_ragged(model.decoder, r, enc)
        assert not torch.equal(f32.packed, out.packed)


@pytest.mark.parametrize("mode", ["f32", "bf16"])
def test_rows_beyond_the_total_are_never_written(mode):
    _skip_variants()
    cfg, model, dd, _, _ = _setup("forward", len(COUNTS), 256, 75)
    total = sum(COUNTS)
    cap = total + 1000
    pts, r = _clouds(COUNTS, 76, capacity=cap)
    _, tight = _clouds(COUNTS, 76)
    enc = _encoding(model, dd)
    idx = torch.full((cap, 7), 12345, dtype=torch.int32, device=DEV)
    d2 = torch.full((cap, 7), SENTINEL, device=DEV)
    pu.knn_ragged(r.packed, r.offsets, enc["anchors"].contiguous().float(), 7, idx_out=idx, dist_out=d2)
    assert bool((idx[total:] == 12345).all()) and bool((d2[total:] == SENTINEL).all())
    assert bool((idx[:total] != 12345).all())
    out = torch.full((cap, 3), SENTINEL, device=DEV)
    with torch.no_grad(), hip_decoder.mode(mode):
        got = hip_decoder.decoder_forward_ragged(model.decoder, r, enc, out=out)
        want = hip_decoder.decoder_forward_ragged(model.decoder, tight, enc)
    assert got.packed is out
    assert bool((out[total:] == SENTINEL).all()), "padding rows were written"
    assert torch.equal(out[:total], want.packed), _first_difference(out[:total], want.packed)
    assert bool((out[:total] != SENTINEL).any(-1).all()), "a real row was not written"


# ---- step level: ragged batch against the same batch padded -------------------------------------------------------------

def _ragged_equals_padded(mtype, ns, counts, seed):
    cfg, model, dd, _, _ = _setup(mtype, len(counts), ns, seed)
    nmax = max(counts)
    padded = torch.from_numpy(synth.uniform(seed, "verts", (len(counts), nmax, 3), -0.5, 0.5)).to(DEV)
    step = _step_fn(mtype)
    pdd = dict(dd)
    pdd["verts_src"] = padded
    _, want = step(model, pdd, cfg)
    rdd = dict(dd)
    rdd["verts_src"] = RaggedPoints.from_list([padded[b, :n] for b, n in enumerate(counts)])
    _, got = step(model, rdd, cfg)
    assert isinstance(got["verts_tgt_pred"], RaggedPoints)
    assert torch.equal(got["surface_samples_tgt_pred"], want["surface_samples_tgt_pred"]), \
        (mtype, _first_difference(got["surface_samples_tgt_pred"].flatten(0, 1), want["surface_samples_tgt_pred"].flatten(0, 1)))
    rows = got["verts_tgt_pred"].split()
    for b, n in enumerate(counts):
        assert rows[b].shape == (n, 3)
        assert torch.equal(rows[b], want["verts_tgt_pred"][b, :n]), (mtype, b, n, _first_difference(rows[b], want["verts_tgt_pred"][b, :n]))


@pytest.mark.parametrize("mtype", ["forward", "arbitrary"])
def test_step_on_ragged_batch_equals_padded_batch_tiny(mtype):
    _skip_variants()
    _ragged_equals_padded(mtype, 256, COUNTS, 77)


@pytest.mark.parametrize("mtype", ["forward", "arbitrary"])
def test_step_on_ragged_batch_equals_padded_batch_full_size(mtype):
    """B = 4, NS = 2048, the issue's mixed config-5 sizes: 278 160 rows against 400 000 padded."""
    _skip_variants()
    _ragged_equals_padded(mtype, 2048, (100000, 61234, 35007, 81919), 78)


def test_ragged_loss_is_the_mean_of_the_per_shape_losses():
    _skip_variants()
    counts = (300, 0, 17, 1000)
    cfg, model, dd, _, _ = _setup("forward", len(counts), 256, 79)
    pts, r = _clouds(counts, 80)
    tgt = [p + 0.01 for p in pts]
    step = _step_fn("forward")
    rdd = dict(dd, verts_src=r, verts_tgt=RaggedPoints.from_list(tgt))
    loss, got = step(model, rdd, cfg, compute_loss=True)
    per = []
    for b, n in enumerate(counts):
        if n:
            one = {k: v[b:b + 1].contiguous() for k, v in dd.items()}
            one.update(verts_src=pts[b][None].contiguous(), verts_tgt=tgt[b][None].contiguous())
            per.append(step(model, one, cfg, compute_loss=True)[0])
    assert abs(loss - float(np.mean(per))) <= 1e-6 * max(1.0, abs(loss)), (loss, per)


# ---- the oracle ---------------------------------------------------------------------------------------------------------

def test_ragged_rows_match_the_oracle_per_shape():
    """Tiny forward model, eval-mode BatchNorm (a shape does not see its batch): per shape the oracle's model_forward at batch 1
    against that shape's ragged rows."""
    counts = (3001, 17, 1, 640)
    cfg, model, dd, state, data = _setup("forward", len(counts), 256, 81)
    pts, r = _clouds(counts, 82)
    if not hip_decoder.fused_for_inference():
        pytest.skip("the ragged decode is refused without the fused decoder")
    _, got = _step_fn("forward")(model, dict(dd, verts_src=r), cfg)
    rows = got["verts_tgt_pred"].split()
    sd = tdnet_ref.to_torch_state(state)
    for b, n in enumerate(counts):
        with torch.no_grad():
            ref = tdnet_ref.model_forward(sd, cfg["model"], {"surface_samples_inputs": torch.from_numpy(data["surface_samples_inputs"][b:b + 1]),
                                                            "q": pts[b][None].cpu()}, queries_key="q").numpy()
        err = l2_err(rows[b][None].cpu().numpy(), ref)
        print(f"shape {b} ({n} vertices): l2 error against the oracle {err:.3e}")
        assert err <= TOL_L2, (b, n, err)


# ---- one captured graph, any mix of sizes -------------------------------------------------------------------------------

@pytest.mark.parametrize("mtype", ["forward", "arbitrary"])
def test_one_captured_graph_replays_every_mix_of_sizes(mtype):
    _skip_variants()
    cfg, model, dd, _, _ = _setup(mtype, 3, 256, 83)
    step_fn = _step_fn(mtype)
    eager = RaggedTestOnBatch(step_fn, 4000)
    graphed = RaggedTestOnBatch(step_fn, 4000, graph=True)
    sets = [(1000, 2000, 1000), (7, 0, 3001), (1, 1, 1), (1000, 2000, 1000)]
    try:
        outs = []
        for i, counts in enumerate(sets):
            pts, _ = _clouds(counts, 84 + (i % 3))
            _, e = eager(model, dict(dd, verts_src=list(pts)), cfg)
            _, g = graphed(model, dict(dd, verts_src=list(pts)), cfg)
            assert isinstance(g["verts_tgt_pred"], RaggedPoints) and g["verts_tgt_pred"].packed.shape == (sum(counts), 3)
            assert g["verts_tgt_pred"].counts == counts
            assert torch.equal(g["verts_tgt_pred"].packed, e["verts_tgt_pred"].packed), \
                (mtype, counts, _first_difference(g["verts_tgt_pred"].packed, e["verts_tgt_pred"].packed))
            assert torch.equal(g["surface_samples_tgt_pred"], e["surface_samples_tgt_pred"]), (mtype, counts)
            outs.append(g["verts_tgt_pred"].packed)
        assert graphed.replays == 4 and graphed.eager_calls == 0
        assert eager.replays == 0 and eager.eager_calls == 4
        assert torch.equal(outs[0], outs[3]) and outs[0].data_ptr() != outs[3].data_ptr()
        # beyond the capacity: one eager call, still correct
        counts = (3000, 2000, 1000)
        pts, _ = _clouds(counts, 90)
        _, e = eager(model, dict(dd, verts_src=list(pts)), cfg)
        _, g = graphed(model, dict(dd, verts_src=list(pts)), cfg)
        assert graphed.replays == 4 and graphed.eager_calls == 1
        assert torch.equal(g["verts_tgt_pred"].packed, e["verts_tgt_pred"].packed)
        # ... and the graph still serves the next batch that fits
        pts, _ = _clouds(sets[0], 84)
        _, g = graphed(model, dict(dd, verts_src=list(pts)), cfg)
        assert graphed.replays == 5 and torch.equal(g["verts_tgt_pred"].packed, outs[0])
    finally:
        graphed.close()


# ---- refusals -----------------------------------------------------------------------------------------------------------

def test_refusals_name_their_reason():
    from nsdp_amd.query_shard import QueryShards, query_sharded
    _skip_variants()
    counts = (100, 17)
    cfg, model, dd, _, _ = _setup("forward", len(counts), 256, 91)
    pts, r = _clouds(counts, 92)
    enc = _encoding(model, dd)
    # autograd enabled: the rectangular call would take the layered path; the ragged one has none
    with torch.enable_grad():
        with pytest.raises(RuntimeError, match="autograd"):
            model.decode(r, enc)
        with pytest.raises(RuntimeError, match="autograd"):
            model(r, dd["surface_samples_inputs"])
    # a captured replay of a model in training mode
    step = RaggedTestOnBatch(_step_fn("forward"), 1000, graph=True)
    model.train()
    try:
        with pytest.raises(ValueError, match=r"eval\(\)"):
            step(model, dict(dd, verts_src=list(pts)), cfg)
    finally:
        model.eval()
        step.close()
    # the fused decoder switched off
    was = hip_decoder.ENABLED
    hip_decoder.ENABLED = False
    try:
        with torch.no_grad(), pytest.raises(RuntimeError, match="NSDP_FUSED_DECODER=0"):
            model.decode(r, enc)
    finally:
        hip_decoder.ENABLED = was
    # splitting a ragged set over ranks
    with pytest.raises(NotImplementedError, match="ragged"):
        query_sharded(_step_fn("forward"), QueryShards(0, 1))(model, dict(dd, verts_src=r), cfg)
    with pytest.raises(NotImplementedError, match="ragged"):
        query_sharded(_step_fn("forward"), QueryShards(0, 1), graph=True)(model, dict(dd, verts_src=r), cfg)
    # a set whose batch is not the encoding's
    _, three = _clouds((5, 6, 7), 93)
    with torch.no_grad(), pytest.raises(RuntimeError, match="3 shapes"):
        model.decode(three, enc)


# ---- the command --------------------------------------------------------------------------------------------------------

def _infer(tmp_path, name, *flags):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "LOCAL_WORLD_SIZE",
                                                             "MASTER_ADDR", "MASTER_PORT")}
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    out = tmp_path / name
    p = subprocess.run([sys.executable, "-m", "nsdp_amd.infer", str(tmp_path / "forward.yaml"), "--surface", "256",
                        "--steps", "2", "--warmup", "1", "--out", str(out), *flags],
                       capture_output=True, text=True, timeout=600, cwd=ROOT, env=env)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, p.stdout[-2000:]
    return json.loads(lines[0]), out


@pytest.mark.timeout(1300)
def test_infer_vertex_counts_equals_the_padded_run(tmp_path):
    _skip_variants()
    import yaml
    from nsdp_amd.config import default_config
    cfg = default_config("forward")
    cfg["model"]["encoder_kwargs"]["npoints_per_layer"] = [256, 64, 16]
    (tmp_path / "forward.yaml").write_text(yaml.safe_dump(cfg))
    counts = (1001, 17, 640)
    rag, rdir = _infer(tmp_path, "ragged", "--vertex-counts", ",".join(map(str, counts)), "--graph", "--reps", "2")
    pad, pdir = _infer(tmp_path, "padded", "--batch", "3", "--queries", "1001")
    assert rag["ragged"] is True and rag["vertex_counts"] == list(counts) and rag["total"] == sum(counts)
    assert rag["capacity"] == sum(counts) and rag["batch"] == 3
    assert rag["equal_to_padded"] is True
    assert rag["replays"] == 1 + 2 and rag["eager_calls"] == 0, rag          # (--warmup 1 --steps 2: all of them replayed)
    for k in ("ms_per_call", "ms_padded", "ms_per_shape_loop"):
        assert rag[k] > 0, k
    offs = np.load(rdir / "verts_offsets.npy")
    assert offs.tolist() == [0, 1001, 1018, 1658]
    verts = np.load(rdir / "verts_tgt_pred.npy")
    want = np.load(pdir / "verts_tgt_pred.npy")
    assert verts.shape == (sum(counts), 3) and want.shape == (3, 1001, 3)
    for b, n in enumerate(counts):
        assert np.array_equal(verts[offs[b]:offs[b + 1]].view(np.int32), want[b, :n].view(np.int32)), b
    assert np.array_equal(np.load(rdir / "surface_samples_tgt_pred.npy").view(np.int32),
                          np.load(pdir / "surface_samples_tgt_pred.npy").view(np.int32))
    # more than one GPU: a message, not a run
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    p = subprocess.run([sys.executable, "-m", "nsdp_amd.infer", str(tmp_path / "forward.yaml"), "--vertex-counts", "5,6", "--gpus", "2"],
                       capture_output=True, text=True, timeout=120, cwd=ROOT, env=env)
    assert p.returncode != 0 and "one GPU" in p.stderr
