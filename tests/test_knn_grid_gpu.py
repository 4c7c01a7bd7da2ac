"""GPU: the k-nearest-neighbour search through a cell grid (include/nsdp_search.h, csrc/knn_grid.hip) gives the indices AND the
distance bits of the exhaustive scan (nsdp_knn / nsdp_knn_ragged_source on the same inputs, taken through
``knn_grid_mode("0")``) -- on surfaces, volumes, lattices full of exact ties and duplicates, degenerate clouds, far outliers,
queries outside the box, shapes shorter than k, packed sets, through the dispatch, through the model and replayed from a graph.
The grid entries are called explicitly, so these small shapes run them."""
import numpy as np
import pytest
import torch

from helpers import build_product, model_cfg
from nsdp_amd import _lib, hip_decoder, pointnet2_utils as pu, precision, synth
from nsdp_amd.ragged import RaggedPoints
from oracle import pointnet2_ref as ref
from poison_arena import _Recorder

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)


def _sphere(rng, n, radius=0.5, centre=(0.0, 0.0, 0.0)):
    v = rng.standard_normal((n, 3))
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    return (v * radius + np.asarray(centre)).astype(np.float32)


def _family(name):
    """One cloud (m, 3) fp32 of the named family, the same on every call."""
    rng = np.random.default_rng(sum(map(ord, name)))
    if name == "sphere":
        return _sphere(rng, 3001)
    if name == "cube":
        return rng.uniform(-0.5, 0.5, (5000, 3)).astype(np.float32)
    if name == "lattice":          # multiples of 1/8 on a 12^3 lattice: exact ties, duplicates, points on cell faces
        return (rng.integers(0, 12, (4000, 3)) / 8.0).astype(np.float32)
    if name == "identical":
        return np.tile(np.array([[0.25, -0.5, 0.125]], np.float32), (300, 1))
    if name == "collinear":
        t = rng.uniform(-1.0, 1.0, (2000, 1))
        return (t * np.array([[0.3, -0.7, 0.2]]) + np.array([[0.1, 0.2, 0.3]])).astype(np.float32)
    if name == "coplanar":
        uv = rng.uniform(-0.5, 0.5, (3000, 2))
        return np.stack([uv[:, 0], uv[:, 1], np.full(3000, 0.125)], 1).astype(np.float32)
    if name == "outlier":          # two tiny clusters 3 apart and one point far away: its shells cross the whole grid
        return np.concatenate([_sphere(rng, 1500, 0.025), _sphere(rng, 1500, 0.025, (3.0, 0.0, 0.0)),
                               np.array([[40.0, -40.0, 40.0]], np.float32)])
    if name == "seventeen":
        return rng.uniform(-0.5, 0.5, (17, 3)).astype(np.float32)
    if name == "one":
        return np.array([[0.5, 0.25, -1.0]], np.float32)
    raise KeyError(name)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _scan(query, source, k):
    with pu.knn_grid_mode("0"):
        return pu.knn(query, source, k, return_dist=True)


def _same(got, want):
    """Indices and distance BITS."""
    np.testing.assert_array_equal(got[0].cpu().numpy(), want[0].cpu().numpy())
    np.testing.assert_array_equal(got[1].cpu().numpy().view(np.int32), want[1].cpu().numpy().view(np.int32))


@pytest.mark.parametrize("name,k", [("sphere", 16), ("cube", 10), ("lattice", 16), ("identical", 16), ("collinear", 16),
                                    ("coplanar", 16), ("outlier", 16), ("seventeen", 16), ("one", 1)])
def test_self_search_equals_the_scan(name, k):
    cloud = _family(name)
    xyz = _dev(cloud[None])
    got = pu.knn_grid(xyz, xyz, k, return_dist=True)
    stats = pu.knn_grid_stats()
    _same(got, _scan(xyz, xyz, k))
    assert stats["queries"] == cloud.shape[0] and stats["tests"] >= cloud.shape[0] * k and stats["cells"] >= 1
    if name == "outlier":
        # the clusters fall into single cells (1500 tests each); the outlier alone is finished by the plain scan
        assert stats["scanned"] == 1 and stats["tests"] <= 3000 * 1500 + 2 * 3001
    if name == "sphere":           # ... and one case against the oracle itself
        want_idx, want_d = ref.knn(cloud[None], cloud[None], k, return_dist=True)
        np.testing.assert_array_equal(got[0].cpu().numpy(), want_idx)
        np.testing.assert_array_equal(got[1].cpu().numpy().view(np.int32), want_d.view(np.int32))


def test_queries_outside_the_box():
    rng = np.random.default_rng(10)
    source = _dev(_sphere(rng, 3000)[None])
    query = _dev((rng.standard_normal((1, 100, 3)) * 2.0).astype(np.float32))
    _same(pu.knn_grid(query, source, 7, return_dist=True), _scan(query, source, 7))


def test_three_families_in_one_call():
    clouds = np.stack([_family("sphere")[:3000], _family("lattice")[:3000], _family("coplanar")[:3000]])
    xyz = _dev(clouds)
    _same(pu.knn_grid(xyz, xyz, 16, return_dist=True), _scan(xyz, xyz, 16))
    query = _dev(np.stack([_family("cube")[:333], _family("lattice")[3000:3333], _family("collinear")[:333]]))
    got = pu.knn_grid(query, xyz, 16)                                      # (and without the distances)
    np.testing.assert_array_equal(got.cpu().numpy(), _scan(query, xyz, 16)[0].cpu().numpy())


COUNTS, SLACK = (1200, 16, 17, 3000, 1), 50


def _packed_set():
    rng = np.random.default_rng(23)
    parts = [_sphere(rng, 1200), rng.uniform(-1, 1, (16, 3)).astype(np.float32), _family("seventeen"), _family("coplanar"),
             _family("one"), rng.uniform(-1, 1, (SLACK, 3)).astype(np.float32)]
    return _dev(np.concatenate(parts)), _dev(np.array([0] + list(np.cumsum(COUNTS)), np.int32))


@pytest.mark.parametrize("queries", ["packed", "rectangular"])
def test_packed_source_equals_the_scan_and_leaves_the_slack_alone(queries):
    """Two shapes are shorter than k = 16 (the sentinels: the shape's first row, FLT_MAX); rows beyond the total keep their fill."""
    xyz, off = _packed_set()
    total, k, n_max = sum(COUNTS), 16, max(COUNTS)
    if queries == "packed":
        q, qoff, lead = xyz, off, (xyz.shape[0],)
    else:
        q = _dev(np.random.default_rng(24).uniform(-0.7, 0.7, (len(COUNTS), 64, 3)).astype(np.float32))
        qoff, lead = None, (len(COUNTS), 64)
    bufs = [(torch.full(lead + (k,), -7, dtype=torch.int32, device=DEV), torch.full(lead + (k,), -1.0, device=DEV)) for _ in range(2)]
    got = pu.knn_grid_ragged_source(q, xyz, off, k, n_max, query_offsets=qoff, idx_out=bufs[0][0], dist_out=bufs[0][1])
    stats = pu.knn_grid_stats()
    with pu.knn_grid_mode("0"):
        want = pu.knn_ragged_source(q, xyz, off, k, n_max, query_offsets=qoff, idx_out=bufs[1][0], dist_out=bufs[1][1])
    _same(got, want)
    assert stats["queries"] == (total if queries == "packed" else len(COUNTS) * 64)
    if queries == "packed":
        assert bool((got[0][total:] == -7).all()) and bool((got[1][total:] == -1.0).all())
        first = int(off[1])                                               # the 16-row shape has 16 neighbours, the 1-row shape one
        assert bool((got[0][sum(COUNTS[:4])] == sum(COUNTS[:4])).all()) and float(got[1][sum(COUNTS[:4]), 1]) == np.finfo(np.float32).max
        assert sorted(got[0][first].tolist()) == list(range(first, first + 16))


def test_the_grid_prunes_a_surface():
    """A condition, not a measurement: on a uniform surface the search must stay far below the scan's tests and never take
    its plain-scan finish."""
    n, k = 20000, 16
    xyz = _dev(_sphere(np.random.default_rng(77), n)[None])
    got = pu.knn_grid(xyz, xyz, k, return_dist=True)
    stats = pu.knn_grid_stats()
    print("knn_grid stats on the 20 000-point sphere:", stats)
    assert stats["queries"] == n
    assert stats["tests"] <= n * 20000 // 8
    assert stats["scanned"] == 0
    _same(got, _scan(xyz, xyz, k))


def test_dispatch_by_mode():
    xyz = _dev(_sphere(np.random.default_rng(5), 9000)[None])
    res = {}
    for mode in ("1", "0", "force"):
        with pu.knn_grid_mode(mode):
            res[mode] = pu.knn(xyz, xyz, 16, return_dist=True)
    _same(res["1"], res["0"])
    _same(res["force"], res["0"])
    small = xyz[:, :600].contiguous()
    pu.knn_grid_stats()                                                   # (forgets the searches above)
    with pu.knn_grid_mode("0"):
        off = pu.knn(small, small, 16)
        assert pu.knn_grid_stats() is None
    with pu.knn_grid_mode("1"):
        pu.knn(small, small, 16)
        assert pu.knn_grid_stats() is None                                # below KNN_GRID_MIN_POINTS: the scan
    with pu.knn_grid_mode("force"):
        on = pu.knn(small, small, 16)
        stats = pu.knn_grid_stats()
    assert stats is not None and stats["queries"] == 600
    assert torch.equal(on, off)


def test_captured_call_follows_the_clouds_contents():
    """One call in a graph over static buffers: the workspace is initialised by nodes of the graph, so every replay is right."""
    rng = np.random.default_rng(31)
    clouds = [_dev(_sphere(rng, 1500)[None]), _dev(rng.uniform(-1, 1, (1, 1500, 3)).astype(np.float32)),
              _dev((rng.integers(0, 9, (1, 1500, 3)) / 4.0).astype(np.float32))]
    static = clouds[0].clone()
    ws = torch.empty(16 << 20, dtype=torch.uint8, device=DEV)
    pu.knn_grid(static, static, 16, return_dist=True, workspace=ws)       # (warm-up outside the capture)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        idx, d2 = pu.knn_grid(static, static, 16, return_dist=True, workspace=ws)
    for cloud in clouds[1:]:
        static.copy_(cloud)
        graph.replay()
        torch.cuda.synchronize()
        _same((idx.clone(), d2.clone()), _scan(cloud, cloud, 16))


# ---------------------------------------------------------------------------------------------------------------- the model
def _skip_refused_variants():
    """The library variants under which the ragged surface path is refused by design (tests/test_ragged_surface_gpu.py)."""
    knobs = []
    if not hip_decoder.ENABLED:
        knobs.append("NSDP_FUSED_DECODER=0")
    if precision.is_bf16():
        knobs.append("NSDP_STORAGE=bf16")
    if knobs:
        pytest.skip("ragged surface clouds are refused under " + ", ".join(knobs))


def _predict(model, dd, cfg, mode, monkeypatch):
    from nsdp_amd.model.deformation_networks import test_on_batch_with_cano
    real, called = _lib.lib(), set()
    monkeypatch.setattr(_lib, "_lib", _Recorder(real, called))
    with pu.knn_grid_mode(mode):
        _, got = test_on_batch_with_cano(model, dd, cfg)
    monkeypatch.setattr(_lib, "_lib", real)
    torch.cuda.synchronize()
    return got, called


def _packed(t):
    return t.packed if isinstance(t, RaggedPoints) else t


def _tiny_model(surface, verts):
    cfg = model_cfg("forward", [256, 64, 16])
    model, _, _ = build_product(cfg, 141, DEV)
    model.eval()
    inputs = _dev(synth.make_batch(141, 2, surface, 4)["surface_samples_inputs"])
    return cfg, model, inputs, _dev(synth.uniform(142, "verts", (2, verts, 3), -0.5, 0.5))


def test_model_predictions_are_bit_identical_under_force_and_off(monkeypatch):
    cfg, model, inputs, verts = _tiny_model(9000, 2000)
    one = {"surface_samples_inputs": inputs[:1].contiguous(), "surface_samples_src": inputs[:1, :, 0:3].contiguous(),
           "verts_src": verts[:1].contiguous()}
    (on, reached), (off, without) = _predict(model, one, cfg, "force", monkeypatch), _predict(model, one, cfg, "0", monkeypatch)
    assert "nsdp_knn_grid" in reached
    assert "nsdp_knn" in without and not {"nsdp_knn_grid", "nsdp_knn_grid_ragged_source"} & without
    for key in ("verts_tgt_pred", "surface_samples_tgt_pred"):
        assert bool(torch.isfinite(on[key]).all()) and torch.equal(on[key], off[key]), key


def test_ragged_surface_step_is_bit_identical_under_force_and_off(monkeypatch):
    _skip_refused_variants()
    cfg, model, inputs, verts = _tiny_model(2600, 64)
    surf = RaggedPoints.from_rows([inputs[0, :2600], inputs[1, :1100]])
    rag = {"surface_samples_inputs": surf, "surface_samples_src": surf.columns(0, 3),
           "verts_src": RaggedPoints.from_list([verts[0], verts[1, :17].contiguous()])}
    (on, reached), (off, without) = _predict(model, rag, cfg, "force", monkeypatch), _predict(model, rag, cfg, "0", monkeypatch)
    assert "nsdp_knn_grid_ragged_source" in reached
    assert "nsdp_knn_ragged_source" in without and "nsdp_knn_grid_ragged_source" not in without
    for key in ("verts_tgt_pred", "surface_samples_tgt_pred"):
        assert bool(torch.isfinite(_packed(on[key])).all()) and torch.equal(_packed(on[key]), _packed(off[key])), key
