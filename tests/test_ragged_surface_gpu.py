"""Ragged SURFACE clouds on the GPU (nsdp_amd.ragged): shapes of different sample counts encoded in one call.  The two
packed-source geometry kernels against their rectangular twins (exact), the encoder and the step functions against the per-shape
oracle at batch 1 (the suite's bar), the wiring of the two-network step, the refusals and the ``--surface-counts`` command."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from helpers import build_product, l2_err, model_cfg, to_dev
from nsdp_amd import hip_decoder, pointnet2_utils as pu, precision, synth
from nsdp_amd.model import ops
from nsdp_amd.ragged import RaggedPoints, RaggedTestOnBatch
from oracle import tdnet_ref
from test_geometry_gpu import _cloud

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL_L2 = 1e-4                                         # tests/test_model_gpu.py: the suite's bar against the oracle
SENTINEL = -7.5
FPS_COUNTS = (64, 65, 127, 128, 129, 511, 512, 513, 700, 2048, 2049, 3000)      # n == nsamples, every change of the tie rule's
FPS_SAMPLES = 64                                                                # block size, the 512 / 2048 template boundaries
KNN_COUNTS = (10, 11, 255, 256, 257, 1023, 1024, 1025, 3001)      # n == k, the 256-query workgroup +- 1, the 1024-point tile +- 1
SURF_COUNTS = (256, 64, 65, 300, 513, 700)
VERT_COUNTS = (3001, 17, 1, 640, 16, 257)


def _skip_refused_variants():
    """The library variants under which the ragged surface path is refused by design (tests/test_ragged_gpu.py skips likewise)."""
    knobs = []
    if not hip_decoder.ENABLED:
        knobs.append("NSDP_FUSED_DECODER=0")
    if precision.is_bf16():
        knobs.append("NSDP_STORAGE=bf16")
    if knobs:
        pytest.skip("ragged surface clouds are refused under " + ", ".join(knobs))


def _first_difference(a, b):
    rows = (a != b).reshape(a.shape[0], -1).any(-1).nonzero().flatten()
    return f"{rows.numel()} rows differ, first: {rows[:8].tolist()}"


def _clouds(counts, seed, capacity=None, kind="uniform"):
    if kind == "uniform":
        pts = [torch.from_numpy(synth.uniform(seed, f"surf_{b}", (n, 3), -0.5, 0.5)).to(DEV) for b, n in enumerate(counts)]
    else:      # the generators of tests/test_geometry_gpu.py: exact distance ties
        pts = [torch.from_numpy(_cloud(seed + b, 1, n, kind)[0]).to(DEV) for b, n in enumerate(counts)]
    return pts, RaggedPoints.from_list(pts, capacity=capacity)


# ---- kernels against their rectangular twins ----------------------------------------------------------------------------

def _fps_equals_per_shape(pts, r, counts, n_maxes):
    want = [pu.furthest_point_sample(p[None].contiguous(), FPS_SAMPLES)[0] for p in pts]      # (once, shared by every n_max)
    offs = r.offsets.tolist()
    for n_max in n_maxes:
        got = pu.furthest_point_sample_ragged(r.packed, r.offsets, FPS_SAMPLES, n_max)
        assert got.shape == (len(counts), FPS_SAMPLES) and got.dtype == torch.int32
        for b, n in enumerate(counts):
            local = got[b] - offs[b]
            assert torch.equal(local, want[b]), (n_max, b, n, (local != want[b]).nonzero().flatten()[:8].tolist())


def test_fps_ragged_equals_fps_per_shape_for_every_n_max():
    """One call samples twelve clouds; each shape's indices minus its offset are those of the rectangular call on that shape
    alone, whichever kernel form n_max selects (3000: 512 threads, 4096: the same form at its LDS limit, 9000: global scratch)."""
    pts, r = _clouds(FPS_COUNTS, 101)
    _fps_equals_per_shape(pts, r, FPS_COUNTS, (3000, 4096, 9000))


@pytest.mark.parametrize("kind", ["grid", "dupes"])
def test_fps_ragged_ties_follow_each_shapes_own_block_size(kind):
    counts = (64, 100, 129, 512, 700, 2049, 4096)
    pts, r = _clouds(counts, 103, kind=kind)
    _fps_equals_per_shape(pts, r, counts, (4096,))


def _knn_equals_per_shape(idx, d2, queries, pts, offs, k, what):
    for b, c in enumerate(pts):
        wi, wd = pu.knn(queries[b][None].contiguous(), c[None].contiguous(), k, return_dist=True)
        gi = idx[b] - offs[b]
        assert torch.equal(gi, wi[0]), (what, k, b, c.shape[0], _first_difference(gi, wi[0]))
        assert torch.equal(d2[b].view(torch.int32), wd[0].view(torch.int32)), (what, k, b, _first_difference(d2[b], wd[0]))


@pytest.mark.parametrize("k", [10, 20])      # (k <= 16: four lanes per query with deferred insertion; above: one lane per query)
def test_knn_self_search_equals_knn_per_shape(k):
    counts = KNN_COUNTS if k == 10 else tuple(n for n in KNN_COUNTS if n >= k)
    pts, r = _clouds(counts, 105)
    idx, d2 = pu.knn_ragged_source(r.packed, r.packed, r.offsets, k, max(counts), query_offsets=r.offsets, return_dist=True)
    assert idx.shape == (r.capacity, k) and idx.dtype == torch.int32 and d2.shape == (r.capacity, k)
    offs = r.offsets.tolist()
    _knn_equals_per_shape([idx[offs[b]:offs[b + 1]] for b in range(len(counts))], [d2[offs[b]:offs[b + 1]] for b in range(len(counts))],
                          pts, pts, offs, k, "self-search")
    only = pu.knn_ragged_source(r.packed, r.packed, r.offsets, k, max(counts), query_offsets=r.offsets)
    assert torch.equal(only, idx)


@pytest.mark.parametrize("k,kind", [(16, "uniform"), (20, "uniform"), (16, "grid")])
def test_knn_rectangular_queries_against_packed_sources_equals_knn_per_shape(k, kind):
    counts = tuple(n for n in KNN_COUNTS if n >= k)
    pts, r = _clouds(counts, 105, kind=kind)
    q = torch.from_numpy(synth.uniform(106, "queries", (len(counts), 64, 3), -0.5, 0.5)).to(DEV)
    if kind == "grid":      # (queries ON lattice points: ties at every distance)
        q = torch.stack([c[torch.arange(64, device=DEV) % c.shape[0]] for c in pts]).contiguous()
    idx, d2 = pu.knn_ragged_source(q, r.packed, r.offsets, k, max(counts), return_dist=True)
    assert idx.shape == (len(counts), 64, k) and d2.shape == (len(counts), 64, k)
    _knn_equals_per_shape(idx, d2, q, pts, r.offsets.tolist(), k, "rectangular queries")


def test_rows_beyond_the_total_are_never_written_and_every_real_row_is():
    total = sum(KNN_COUNTS)
    cap = total + 1000
    pts, r = _clouds(KNN_COUNTS, 105, capacity=cap)
    _, tight = _clouds(KNN_COUNTS, 105)
    idx = torch.full((cap, 10), 12345678, dtype=torch.int32, device=DEV)
    d2 = torch.full((cap, 10), SENTINEL, device=DEV)
    pu.knn_ragged_source(r.packed, r.packed, r.offsets, 10, max(KNN_COUNTS), query_offsets=r.offsets, idx_out=idx, dist_out=d2)
    assert bool((idx[total:] == 12345678).all()) and bool((d2[total:] == SENTINEL).all()), "padding rows were written"
    assert bool((idx[:total] != 12345678).all()) and bool((d2[:total] != SENTINEL).all()), "a real row was not written"
    wi, wd = pu.knn_ragged_source(tight.packed, tight.packed, tight.offsets, 10, max(KNN_COUNTS), query_offsets=tight.offsets,
                                  return_dist=True)
    assert torch.equal(idx[:total], wi) and torch.equal(d2[:total], wd)
    # the sampler reads nothing beyond the total either: the same indices from the padded buffer
    a = pu.furthest_point_sample_ragged(r.packed, r.offsets, 10, max(KNN_COUNTS))
    b = pu.furthest_point_sample_ragged(tight.packed, tight.offsets, 10, max(KNN_COUNTS))
    assert torch.equal(a, b) and int(a.max()) < total


# ---- encoder and steps against the oracle -------------------------------------------------------------------------------

def _setup(mtype, npl, counts, seed):
    cfg = model_cfg(mtype, list(npl))
    model, _, state = build_product(cfg, seed, DEV)
    model.eval()
    data = synth.make_batch(seed, len(counts), max(counts), 4)
    inputs = torch.from_numpy(np.ascontiguousarray(data["surface_samples_inputs"])).to(DEV)
    surf = RaggedPoints.from_rows([inputs[b, :n] for b, n in enumerate(counts)])
    dd = {"surface_samples_inputs": surf, "surface_samples_src": surf.columns(0, 3)}
    return cfg, model, dd, tdnet_ref.to_torch_state(state), data


def _step_fn(mtype):
    from nsdp_amd.model.deformation_networks import test_on_batch_with_cano
    from nsdp_amd.model.flow_arbitrary import test_on_batch_with_arbitrary
    return test_on_batch_with_arbitrary if mtype == "arbitrary" else test_on_batch_with_cano


def _oracle(sd, cfg, data, b, n, queries, tape=None):
    """The oracle on shape b alone (its first n surface samples) at batch 1."""
    with torch.no_grad():
        return tdnet_ref.model_forward(sd, cfg["model"], {"surface_samples_inputs": torch.from_numpy(data["surface_samples_inputs"][b:b + 1, :n]),
                                                          "q": queries[None].cpu()}, queries_key="q", tape=tape).numpy()[0]


def _rows_against_oracle(got, cfg, sd, data, counts, verts, shapes=None):
    surf_rows = got["surface_samples_tgt_pred"].split()
    vert_rows = got["verts_tgt_pred"].split() if isinstance(got["verts_tgt_pred"], RaggedPoints) else list(got["verts_tgt_pred"])
    src = torch.from_numpy(data["surface_samples_inputs"][:, :, 0:3])
    for b in (range(len(counts)) if shapes is None else shapes):
        n, nv = counts[b], verts[b].shape[0]
        assert surf_rows[b].shape == (n, 3) and vert_rows[b].shape == (nv, 3)
        # (one oracle pass per shape: the decoder treats query points independently)
        ref = _oracle(sd, cfg, data, b, n, torch.cat([verts[b].cpu(), src[b, :n]]))
        ev = l2_err(vert_rows[b][None].cpu().numpy(), ref[None, :nv])
        es = l2_err(surf_rows[b][None].cpu().numpy(), ref[None, nv:])
        print(f"{cfg['model']['type']} shape {b} ({n} surface samples, {nv} vertices): l2 error against the oracle, vertices {ev:.3e}, "
              f"surface samples {es:.3e}")
        assert ev <= TOL_L2 and es <= TOL_L2, (b, n, nv, ev, es)


@pytest.mark.parametrize("mtype", ["forward", "backward"])
def test_ragged_surface_step_matches_the_oracle_per_shape(mtype):
    _skip_refused_variants()
    cfg, model, dd, sd, data = _setup(mtype, (256, 64, 16), SURF_COUNTS, 111)
    verts, rv = _clouds(VERT_COUNTS, 112)
    _, got = _step_fn(mtype)(model, dict(dd, verts_src=rv), cfg)
    assert isinstance(got["surface_samples_tgt_pred"], RaggedPoints) and isinstance(got["verts_tgt_pred"], RaggedPoints)
    assert got["surface_samples_tgt_pred"].counts == SURF_COUNTS and got["verts_tgt_pred"].counts == VERT_COUNTS
    _rows_against_oracle(got, cfg, sd, data, SURF_COUNTS, verts)


def test_ragged_surface_beside_rectangular_vertices_matches_the_oracle():
    _skip_refused_variants()
    cfg, model, dd, sd, data = _setup("forward", (256, 64, 16), SURF_COUNTS, 113)
    verts = torch.from_numpy(synth.uniform(114, "verts", (len(SURF_COUNTS), 1000, 3), -0.5, 0.5)).to(DEV)
    _, got = _step_fn("forward")(model, dict(dd, verts_src=verts), cfg)
    assert isinstance(got["surface_samples_tgt_pred"], RaggedPoints) and got["verts_tgt_pred"].shape == verts.shape
    _rows_against_oracle(got, cfg, sd, data, SURF_COUNTS, list(verts))


@pytest.mark.parametrize("mtype", ["forward", "backward"])
def test_ragged_encode_anchors_equal_the_batch_one_encode(mtype):
    """The anchors are gathered coordinates (exact geometry all the way down): bit-equal to each shape's own batch-1 call (the
    features pass the dense layers at another row count: they are held to the oracle, not to bit equality)."""
    _skip_refused_variants()
    cfg, model, dd, _, _ = _setup(mtype, (256, 64, 16), SURF_COUNTS, 115)
    with torch.no_grad():
        enc = model.encode(dd["surface_samples_inputs"])
        assert enc["anchors"].shape == (len(SURF_COUNTS), 16, 3) and enc["z"].shape[0] == len(SURF_COUNTS)
        for b, rows in enumerate(dd["surface_samples_inputs"].split()):
            one = model.encode(rows[None].contiguous())
            assert torch.equal(enc["anchors"][b], one["anchors"][0]), (b, _first_difference(enc["anchors"][b], one["anchors"][0]))
    # a set built from device offsets alone: the counts are read back once
    bare = RaggedPoints(dd["surface_samples_inputs"].packed, dd["surface_samples_inputs"].offsets)
    with torch.no_grad():
        again = model.encode(bare)
    assert torch.equal(again["anchors"], enc["anchors"]) and bare._counts == SURF_COUNTS


def test_full_size_ragged_surface_geometry_is_exact_and_predictions_match_the_oracle():
    """[2048, 500, 100], clouds of 2048 to 5000 samples: the level-0 index sets against the rectangular kernels per shape, and
    the smallest and the largest shape's predictions on 3000 vertices against the oracle."""
    _skip_refused_variants()
    counts = (2048, 5000, 1234, 3500)
    cfg, model, dd, sd, data = _setup("forward", (2048, 500, 100), counts, 117)
    surf = dd["surface_samples_inputs"]
    coords = surf.columns(0, 3).packed
    enc = model.encoder
    npoints, ks, _ = enc._pyramid_args()
    begin_idx, levels, join = ops.geometry_pyramid_ragged(coords, surf.offsets, max(counts), enc.transformer_begin.k, npoints, ks)
    join()
    offs, n1 = surf.offsets.tolist(), npoints[0]
    lv = levels[0]
    for b, c in enumerate(surf.columns(0, 3).split()):
        c1 = c[None].contiguous()
        fps = pu.furthest_point_sample(c1, n1)
        assert torch.equal(lv["fps_idx"].view(len(counts), n1)[b] - offs[b], fps[0]), ("fps", b)
        centres = pu.gather_rows(c1, fps)
        assert torch.equal(lv["new_xyz"].view(len(counts), n1, 3)[b], centres[0]), ("centres", b)
        sa = pu.knn(centres, c1, ks[0][0])
        assert torch.equal(lv["sa_idx"].view(len(counts), n1, -1)[b] - offs[b], sa[0]), ("sa_idx", b, _first_difference(lv["sa_idx"].view(len(counts), n1, -1)[b] - offs[b], sa[0]))
        assert torch.equal(lv["blk_idx"][b], pu.knn(centres, centres, ks[0][1])[0]), ("blk_idx", b)
        own = pu.knn(c1, c1, enc.transformer_begin.k)
        assert torch.equal(begin_idx[0, offs[b]:offs[b + 1]] - offs[b], own[0]), ("begin_idx", b)
    verts = [torch.from_numpy(synth.uniform(118, f"v{b}", (3000, 3), -0.5, 0.5)).to(DEV) for b in range(len(counts))]
    _, got = _step_fn("forward")(model, dict(dd, verts_src=RaggedPoints.from_list(verts)), cfg)
    _rows_against_oracle(got, cfg, sd, data, counts, verts, shapes=(2, 1))


# ---- the two-network step -----------------------------------------------------------------------------------------------

def test_arbitrary_step_on_ragged_surfaces_is_the_hand_composed_sequence():
    """Network 2 samples the points network 1 predicts, so an end-to-end bar would measure the composition; both networks are
    held to the oracle as 'backward' / 'forward' models above, and this holds the wiring: bit for bit the sequence composed by
    hand from the two networks' ragged calls."""
    _skip_refused_variants()
    cfg, model, dd, _, _ = _setup("arbitrary", (256, 64, 16), SURF_COUNTS, 119)
    _, rv = _clouds(VERT_COUNTS, 120)
    _, got = _step_fn("arbitrary")(model, dict(dd, verts_src=rv), cfg)
    surf = dd["surface_samples_inputs"]
    src, tgt, mask = surf.columns(0, 3), surf.columns(3, 6), surf.columns(6, 7)
    net1, net2 = model.model_canonicalize, model.model_deform
    with torch.no_grad(), hip_decoder.canonicalize_mode():
        enc1 = net1.encode(src)
        surf2cano, verts2cano = net1.decode(src, enc1), net1.decode(rv, enc1)
    with torch.no_grad():
        deform_in = model.deform_input(surf2cano, tgt, mask)
        assert isinstance(deform_in, RaggedPoints) and deform_in.packed.shape == (surf.capacity, 7) and deform_in.offsets is surf.offsets
        enc2 = net2.encode(deform_in)
        want_surf, want_verts = net2.decode(surf2cano, enc2), net2.decode(verts2cano, enc2)
    assert isinstance(got["surface_samples_tgt_pred"], RaggedPoints) and isinstance(got["verts_tgt_pred"], RaggedPoints)
    assert torch.equal(got["surface_samples_tgt_pred"].packed, want_surf.packed), _first_difference(got["surface_samples_tgt_pred"].packed, want_surf.packed)
    assert torch.equal(got["verts_tgt_pred"].packed, want_verts.packed), _first_difference(got["verts_tgt_pred"].packed, want_verts.packed)
    assert bool(torch.isfinite(want_verts.packed).all())
    # the model's forward is the same composition
    with torch.no_grad():
        fwd = model(rv, src, tgt, mask)
    assert torch.equal(fwd.packed, want_verts.packed)


# ---- the wrapper, the refusals ------------------------------------------------------------------------------------------

def test_ragged_step_wrapper_runs_ragged_surfaces_eagerly():
    _skip_refused_variants()
    cfg, model, dd, _, _ = _setup("forward", (256, 64, 16), (300, 64, 513), 121)
    verts, _ = _clouds((1001, 17, 640), 122)
    step = RaggedTestOnBatch(_step_fn("forward"), 4000, graph=True)
    try:
        _, got = step(model, dict(dd, verts_src=list(verts)), cfg)
        assert step.eager_calls == 1 and step.replays == 0
        _, want = _step_fn("forward")(model, dict(dd, verts_src=RaggedPoints.from_list(verts)), cfg)
        assert torch.equal(got["verts_tgt_pred"].packed, want["verts_tgt_pred"].packed)
        assert torch.equal(got["surface_samples_tgt_pred"].packed, want["surface_samples_tgt_pred"].packed)
    finally:
        step.close()


def test_refusals_name_their_reason():
    from nsdp_amd.query_shard import QueryShards, query_sharded
    _skip_refused_variants()
    cfg, model, dd, _, _ = _setup("forward", (256, 64, 16), (300, 64), 123)
    surf = dd["surface_samples_inputs"]
    _, rv = _clouds((100, 17), 124)
    with torch.enable_grad(), pytest.raises(ValueError, match="autograd"):
        model.encode(surf)
    with torch.enable_grad(), pytest.raises(ValueError, match="autograd"):
        model(rv, surf)
    model.train()
    try:
        with torch.no_grad(), pytest.raises(ValueError, match="training mode"):
            model.encode(surf)
    finally:
        model.eval()
    # everything the ragged decoder refuses: it decodes the surface samples
    was = hip_decoder.ENABLED
    hip_decoder.ENABLED = False
    try:
        with torch.no_grad(), pytest.raises(ValueError, match="NSDP_FUSED_DECODER=0"):
            model.encode(surf)
    finally:
        hip_decoder.ENABLED = was
    with precision.storage(torch.bfloat16), torch.no_grad(), pytest.raises(ValueError, match="bf16 storage"):
        model.encode(surf)
    with torch.no_grad():
        with pytest.raises(ValueError, match="geometry="):
            model.encode(surf, geometry={"encoder": {}})
        with pytest.raises(ValueError, match="PipelinedGeometry"):
            model.geometry(rv.padded(), surf)
        with pytest.raises(ValueError, match="geometry="):
            model.encoder(surf, geometry={"levels": []})
    for graph in (False, True):
        with pytest.raises(NotImplementedError, match="surface"):
            query_sharded(_step_fn("forward"), QueryShards(0, 1), graph=graph)(model, dict(dd, verts_src=rv.padded()), cfg)
    # validation on the host, each naming the shape and the number
    inputs = surf.split()
    with torch.no_grad():
        with pytest.raises(ValueError, match=r"shape 1 has 63 samples, fewer than the 64 points"):
            model.encode(RaggedPoints.from_rows([inputs[0], inputs[1][:63]]))
        with pytest.raises(ValueError, match=r"shape 1 is empty"):
            model.encode(RaggedPoints.from_rows([inputs[0], inputs[1][:0], inputs[1]]))
    small, _, _ = build_product(model_cfg("forward", [256, 8, 4]), 123, DEV)
    k = small.encoder.transformer_begin.k
    with torch.no_grad(), pytest.raises(ValueError, match=rf"shape 0 has {k - 1} samples, fewer than the {k} neighbours"):
        small.eval().encode(RaggedPoints.from_rows([inputs[0][:k - 1], inputs[0]]))


# ---- the command --------------------------------------------------------------------------------------------------------

@pytest.mark.timeout(900)
def test_infer_surface_counts(tmp_path):
    _skip_refused_variants()
    import yaml
    from nsdp_amd.config import default_config
    cfg = default_config("forward")
    cfg["model"]["encoder_kwargs"]["npoints_per_layer"] = [256, 64, 16]
    (tmp_path / "forward.yaml").write_text(yaml.safe_dump(cfg))
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "LOCAL_WORLD_SIZE",
                                                             "MASTER_ADDR", "MASTER_PORT")}
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    scounts, vcounts = (300, 64, 513), (1001, 17, 640)
    out = tmp_path / "ragged"
    cmd = [sys.executable, "-m", "nsdp_amd.infer", str(tmp_path / "forward.yaml"), "--surface-counts", ",".join(map(str, scounts)),
           "--vertex-counts", ",".join(map(str, vcounts))]
    p = subprocess.run(cmd + ["--steps", "2", "--warmup", "1", "--reps", "2", "--out", str(out)],
                       capture_output=True, text=True, timeout=600, cwd=ROOT, env=env)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, p.stdout[-2000:]
    line = json.loads(lines[0])
    assert line["ragged_surface"] is True and line["surface_counts"] == list(scounts) and line["vertex_counts"] == list(vcounts)
    assert line["batch"] == 3 and line["levels"] == [64, 64, 16]                      # (capped at the smallest cloud)
    assert line["ms_per_call"] > 0 and line["ms_per_shape_loop"] > 0 and len(line["ms_per_shape_loop_reps"]) == 2
    print("l2_vs_per_shape_loop", line["l2_vs_per_shape_loop"])
    assert np.isfinite(line["l2_vs_per_shape_loop"]) and line["l2_vs_per_shape_loop"] >= 0      # (reported, not held to a bar)
    assert np.load(out / "surface_offsets.npy").tolist() == [0, 300, 364, 877]
    assert np.load(out / "verts_offsets.npy").tolist() == [0, 1001, 1018, 1658]
    surf, verts = np.load(out / "surface_samples_tgt_pred.npy"), np.load(out / "verts_tgt_pred.npy")
    assert surf.shape == (sum(scounts), 3) and verts.shape == (sum(vcounts), 3)
    assert np.isfinite(surf).all() and np.isfinite(verts).all()
    # more than one GPU: a message, not a run
    p = subprocess.run(cmd + ["--gpus", "2"], capture_output=True, text=True, timeout=120, cwd=ROOT, env=env)
    assert p.returncode != 0 and "one GPU" in p.stderr
