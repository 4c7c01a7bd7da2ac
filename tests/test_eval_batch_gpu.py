"""GPU: evaluation metrics for a whole batch of meshes in one call (nsdp_amd.eval_metric.*_batch, include/nsdp_eval.h).

Kernels: nsdp_nn_dist2 / nsdp_nn_dist2_ragged hold the distance bits and the indices of the k = 1 searches they replace
(pointnet2_utils.knn / knn_ragged_source), nsdp_segment_mean_f32 holds float32(the float64 mean) within one ulp and gives a
shape the same bits whatever surrounds it.  Interface: l2 / fnc / cd per shape against the float64 oracle at the bars of the
single-mesh test (tests/test_eval_harness_gpu.py), and the same bits for a mesh alone, in a ragged batch and in a rectangular
one.  Sizes of the search: 1023 / 1024 / 1025 sit on both sides of the kernel's queries per workgroup (1024) and of its LDS
tile (1024 source rows); a split source is cut in whole LDS tiles, and the 30 000-query cases cut 24 575 / 24 576 / 24 577 rows
into parts of three tiles (3072 rows) on a 256-CU device, with a part of one row and empty parts behind it."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from nsdp_amd import eval_metric, pointnet2_utils as pu
from nsdp_amd.ragged import RaggedPoints, offsets_of
from oracle import eval_metric_ref

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLT_MAX = float(np.finfo(np.float32).max)
SIZES = [1, 3, 255, 256, 257, 1023, 1024, 1025, 2049, 4099]


def _gen(seed):
    return torch.Generator(device=DEV).manual_seed(seed)


def _clouds(kind, B, n, m, seed):
    g = _gen(seed)
    if kind == "uniform":
        return torch.rand(B, n, 3, device=DEV, generator=g) - 0.5, torch.rand(B, m, 3, device=DEV, generator=g) - 0.5
    if kind == "repeated":          # every source point occurs about four times: the smallest index must win
        base = torch.rand(B, m // 4 + 1, 3, device=DEV, generator=g) - 0.5
        pick = torch.randint(0, m // 4 + 1, (B, m), device=DEV, generator=g)
        return torch.rand(B, n, 3, device=DEV, generator=g) - 0.5, torch.gather(base, 1, pick[:, :, None].expand(B, m, 3)).contiguous()
    if kind == "lattice":           # a 5 x 5 x 5 lattice: many exact ties between DIFFERENT points as well
        return (torch.randint(0, 5, (B, n, 3), device=DEV, generator=g).float() / 4,
                torch.randint(0, 5, (B, m, 3), device=DEV, generator=g).float() / 4)
    assert kind == "self"           # query = source (rows i mod m): distance zero at the row itself
    s = torch.rand(B, m, 3, device=DEV, generator=g) - 0.5
    return s[:, torch.arange(n, device=DEV) % m].contiguous(), s


def _check_rect(q, s, what):
    widx, wd2 = pu.knn(q, s, 1, return_dist=True)
    d2_only = pu.nn_dist2(q, s)
    d2, idx = pu.nn_dist2(q, s, return_index=True)
    assert torch.equal(d2_only.view(torch.int32), wd2[:, :, 0].view(torch.int32)), f"{what}: distance bits (no index)"
    assert torch.equal(d2.view(torch.int32), wd2[:, :, 0].view(torch.int32)), f"{what}: distance bits (with index)"
    assert torch.equal(idx, widx[:, :, 0]), f"{what}: indices"


@pytest.mark.parametrize("kind", ["uniform", "repeated", "lattice", "self"])
@pytest.mark.parametrize("B", [1, 3])
def test_nn_dist2_has_the_bits_and_indices_of_knn_k1(B, kind):
    for n in SIZES:
        for m in SIZES:
            q, s = _clouds(kind, B, n, m, 1000 * n + m)
            _check_rect(q, s, f"{kind} B={B} n={n} m={m}")


@pytest.mark.parametrize("m", [24575, 24576, 24577])
def test_nn_dist2_split_source_on_both_sides_of_a_part(m):
    q, s = _clouds("uniform", 3, 30000, m, m)
    _check_rect(q, s, f"split m={m}")
    q, s = _clouds("lattice", 1, 30000, m, m + 1)
    _check_rect(q, s, f"split lattice m={m}")


def _packed(counts, cap, seed, lattice=False):
    g = _gen(seed)
    rows = torch.randint(0, 5, (cap, 3), device=DEV, generator=g).float() / 4 if lattice else torch.rand(cap, 3, device=DEV, generator=g) - 0.5
    return rows, offsets_of(counts, DEV)


@pytest.mark.parametrize("lattice", [False, True])
def test_nn_dist2_ragged_equals_knn_ragged_source_k1(lattice):
    qc, sc = [3001, 0, 1, 257], [17, 1025, 5, 300]
    qtot, qcap, scap = sum(qc), sum(qc) + 700, sum(sc) + 90
    q, qoff = _packed(qc, qcap, 1, lattice)
    s, soff = _packed(sc, scap, 2, lattice)
    marker_d, marker_i = -7.0, -12345

    def outs():
        return (torch.full((qcap,), marker_d, device=DEV), torch.full((qcap,), marker_i, dtype=torch.int32, device=DEV))

    wd, wi = torch.full((qcap, 1), marker_d, device=DEV), torch.full((qcap, 1), marker_i, dtype=torch.int32, device=DEV)
    pu.knn_ragged_source(q, s, soff, 1, max(sc), query_offsets=qoff, idx_out=wi, dist_out=wd)
    d_only, _ = outs()
    assert pu.nn_dist2_ragged(q, qoff, s, soff, dist_out=d_only) is d_only
    d, i = outs()
    pu.nn_dist2_ragged(q, qoff, s, soff, dist_out=d, idx_out=i)
    for got in (d_only, d):
        assert torch.equal(got.view(torch.int32), wd[:, 0].view(torch.int32))          # element for element, padding included
    assert torch.equal(i, wi[:, 0])
    assert bool((d_only[qtot:] == marker_d).all()) and bool((d[qtot:] == marker_d).all()) and bool((i[qtot:] == marker_i).all())
    assert bool((d[:qtot] >= 0).all()) and bool((i[:qtot] >= 0).all()) and bool((i[:qtot] < sum(sc)).all())


@pytest.mark.parametrize("sc,scap,empty,want_idx", [([40, 0, 7], 60, 1, 40), ([40, 0], 40, 1, 39), ([0, 9], 9, 0, 0)])
def test_nn_dist2_ragged_shape_without_source_rows(sc, scap, empty, want_idx):
    qc = [5, 300, 2][:len(sc)]
    q, qoff = _packed(qc, sum(qc) + 3, 3)
    s, soff = _packed(sc, scap, 4)
    lo, hi = sum(qc[:empty]), sum(qc[:empty + 1])
    d_only = pu.nn_dist2_ragged(q, qoff, s, soff)
    d, i = pu.nn_dist2_ragged(q, qoff, s, soff, return_index=True)
    for got in (d_only, d):
        assert bool((got[lo:hi] == FLT_MAX).all())
    assert bool((i[lo:hi] == want_idx).all())
    rest = [r for r in range(sum(qc)) if not lo <= r < hi]
    assert bool((d[rest] < 3.0).all()) and torch.equal(d_only[rest], d[rest])


# ---- the per-shape mean ----------------------------------------------------------------------------------------------------

COUNTS = [1, 0, 63, 64, 65, 1023, 1025, 30000]


def _values(transform, seed=11):
    g = torch.Generator().manual_seed(seed)
    if transform:
        return [torch.rand(c, generator=g) - 0.1 for c in COUNTS]          # (some negative: clamped to zero before the root)
    return [torch.randn(c, generator=g) for c in COUNTS]


def _mean_of(parts, transform, cap_extra=0):
    vals = torch.cat(parts + [torch.full((cap_extra,), float("nan"))]).to(DEV)
    return pu.segment_mean(vals, offsets_of([len(p) for p in parts], DEV), sqrt=bool(transform))


@pytest.mark.parametrize("transform", [0, 1])
def test_segment_mean_is_the_float64_mean_within_one_ulp(transform):
    parts = _values(transform)
    got = _mean_of(parts, transform, cap_extra=37).cpu().numpy()
    for b, p in enumerate(parts):
        v = p.numpy()
        if transform:
            v = np.sqrt(np.maximum(v, np.float32(0)))                     # (fp32, correctly rounded: the kernel's sqrtf)
        if len(v) == 0:
            assert np.isnan(got[b])
            continue
        want = np.float32(v.astype(np.float64).mean())
        np.testing.assert_allclose(got[b], want, rtol=1.2e-7, atol=0, err_msg=f"count {len(v)}")


@pytest.mark.parametrize("transform", [0, 1])
def test_segment_mean_of_a_shape_does_not_depend_on_the_other_shapes(transform):
    parts = _values(transform)
    full = _mean_of(parts, transform).view(torch.int32)
    again = _mean_of(parts, transform).view(torch.int32)
    assert torch.equal(full, again)
    flipped = _mean_of(parts[::-1], transform).view(torch.int32)
    assert torch.equal(flipped, full.flip(0))
    for b, p in enumerate(parts):
        alone = _mean_of([p], transform).view(torch.int32)
        assert torch.equal(alone, full[b:b + 1]), f"count {len(p)}"


# ---- the interface ----------------------------------------------------------------------------------------------------------

def _mesh(seed, V, F):
    g = np.random.RandomState(seed)
    verts = g.rand(V, 3).astype(np.float32)
    faces = np.argsort(g.rand(F, V), axis=1)[:, :3].astype(np.int32)      # three distinct vertices: no degenerate face
    pred = verts + np.float32(0.01) * g.randn(V, 3).astype(np.float32)
    return pred, verts, faces


def _ragged_dict(meshes):
    return {"verts_tgt_pred": RaggedPoints.from_list([torch.from_numpy(m[0]).to(DEV) for m in meshes]),
            "verts_tgt": RaggedPoints.from_list([torch.from_numpy(m[1]).to(DEV) for m in meshes]),
            "faces": RaggedPoints.from_rows([torch.from_numpy(m[2]).to(DEV) for m in meshes])}


def _rect_dict(meshes):
    return {"verts_tgt_pred": torch.stack([torch.from_numpy(m[0]) for m in meshes]).to(DEV),
            "verts_tgt": torch.stack([torch.from_numpy(m[1]) for m in meshes]).to(DEV),
            "faces": torch.stack([torch.from_numpy(m[2]) for m in meshes]).to(DEV)}


@pytest.fixture(scope="module")
def meshes():
    return [_mesh(0, 500, 900), _mesh(1, 37, 40), _mesh(2, 1200, 2000), _mesh(3, 500, 900)]


@pytest.fixture(scope="module")
def ragged_run(meshes):
    """The three meshes of different sizes as one ragged batch, with explicit draws; computed once."""
    dd = _ragged_dict(meshes[:3])
    samples = eval_metric.sample_surface_batch(dd["verts_tgt_pred"], dd["faces"], 2000, _gen(5))
    return dd, samples, eval_metric.compute_evaluation_metrics_batch(dd, pointcloud_size=2000, samples=samples)


def test_metrics_batch_against_the_float64_oracle(meshes, ragged_run):
    dd, (face_idx, bary), got = ragged_run
    assert all(got[k].shape == (3,) and got[k].dtype == torch.float32 and got[k].is_cuda for k in ("l2", "fnc", "cd"))
    pts_p = eval_metric.sample_points(dd["verts_tgt_pred"], dd["faces"], face_idx, bary).double().cpu().numpy()
    pts_g = eval_metric.sample_points(dd["verts_tgt"], dd["faces"], face_idx, bary).double().cpu().numpy()
    l2, fnc, cd = (got[k].tolist() for k in ("l2", "fnc", "cd"))
    for b, (pred, verts, faces) in enumerate(meshes[:3]):
        p64, v64, f = pred.astype(np.float64), verts.astype(np.float64), faces.astype(np.int64)
        assert abs(l2[b] - eval_metric_ref.compute_dist_square(p64, v64)) < 1e-8
        want = eval_metric_ref.normal_consistency(eval_metric_ref.face_normals(p64, f), eval_metric_ref.face_normals(v64, f))
        assert abs(fnc[b] - want) < 1e-5
        want = eval_metric_ref.chamfer_distance(pts_p[b], pts_g[b])
        assert abs(cd[b] - want) <= 2e-6 * want
        # the sampled points lie on the faces they name
        tri = v64[f[face_idx[b].cpu().numpy()]]
        np.testing.assert_allclose(pts_g[b], (bary[b].double().cpu().numpy()[:, :, None] * tri).sum(1), atol=1e-6)


def test_a_mesh_gets_the_same_bits_alone_ragged_and_rectangular(meshes, ragged_run):
    _, (face_idx, bary), got = ragged_run
    for b in range(3):
        one = eval_metric.compute_evaluation_metrics_batch(_ragged_dict(meshes[b:b + 1]), samples=(face_idx[b:b + 1], bary[b:b + 1]))
        rect1 = eval_metric.compute_evaluation_metrics_batch(_rect_dict(meshes[b:b + 1]), samples=(face_idx[b:b + 1], bary[b:b + 1]))
        for k in ("l2", "fnc", "cd"):
            assert torch.equal(one[k], got[k][b:b + 1]), (k, b)
            assert torch.equal(rect1[k], got[k][b:b + 1]), (k, b)
    pair = [meshes[0], meshes[3]]                                         # equal sizes: a rectangular batch as well
    samples = eval_metric.sample_surface_batch(*(_rect_dict(pair)[k] for k in ("verts_tgt_pred", "faces")), 2000, _gen(6))
    rect = eval_metric.compute_evaluation_metrics_batch(_rect_dict(pair), samples=samples)
    rag = eval_metric.compute_evaluation_metrics_batch(_ragged_dict(pair), samples=samples)
    for k in ("l2", "fnc", "cd"):
        assert torch.equal(rect[k], rag[k]), k
        for b in range(2):
            alone = eval_metric.compute_evaluation_metrics_batch(_rect_dict(pair[b:b + 1]), samples=(samples[0][b:b + 1], samples[1][b:b + 1]))
            assert torch.equal(alone[k], rect[k][b:b + 1]), (k, b)
    # mesh 0 with the draws of the first run: the batch it sits in does not matter
    again = eval_metric.compute_evaluation_metrics_batch(_rect_dict(pair), samples=(face_idx[[0, 0]], bary[[0, 0]]))
    assert all(torch.equal(again[k][0:1], got[k][0:1]) for k in ("l2", "fnc", "cd"))


def test_metrics_batch_draws_its_own_samples_under_a_generator(meshes):
    dd = _ragged_dict(meshes[:3])
    a = eval_metric.compute_evaluation_metrics_batch(dd, pointcloud_size=2000, generator=_gen(9))
    b = eval_metric.compute_evaluation_metrics_batch(dd, pointcloud_size=2000, generator=_gen(9))
    assert all(torch.equal(a[k], b[k]) for k in a)
    cd = a["cd"].tolist()
    assert all(0.0 < c < 0.05 for c in cd)                                # sampled surfaces 1 cm apart


def test_chamfer_distance_batch_at_evaluation_size_against_the_kd_tree():
    g = _gen(21)
    a, b = torch.rand(2, 30000, 3, device=DEV, generator=g) - 0.5, torch.rand(2, 30000, 3, device=DEV, generator=g) - 0.5
    got = eval_metric.chamfer_distance_batch(a, b).tolist()
    rag = eval_metric.chamfer_distance_batch(RaggedPoints.from_list(list(a)), RaggedPoints.from_list(list(b)))
    assert torch.equal(rag, eval_metric.chamfer_distance_batch(a, b))
    for s in range(2):
        want = eval_metric_ref.chamfer_distance(a[s].double().cpu().numpy(), b[s].double().cpu().numpy())
        np.testing.assert_allclose(got[s], want, rtol=2e-6)
    single = eval_metric.chamfer_distance(a[0], b[0])                      # the one-mesh function is close, not bit-equal
    np.testing.assert_allclose(float(single), got[0], rtol=2e-6)


def test_nn_distance2_batch_layouts():
    g = _gen(22)
    q, s = torch.rand(3, 700, 3, device=DEV, generator=g), torch.rand(3, 1500, 3, device=DEV, generator=g)
    d2, idx = eval_metric.nn_distance2_batch(q, s, return_index=True)
    assert d2.shape == (3, 700) and idx.shape == (3, 700) and idx.dtype == torch.int32
    picked = torch.gather(s, 1, idx.long()[:, :, None].expand(3, 700, 3))
    assert torch.allclose((q - picked).pow(2).sum(-1), d2, rtol=1e-5, atol=0)
    rq, rs = RaggedPoints.from_list([q[0], q[1, :5], q[2]], capacity=1500), RaggedPoints.from_list([s[0], s[1], s[2, :9]])
    rd2, ridx = eval_metric.nn_distance2_batch(rq, rs, return_index=True)
    assert isinstance(rd2, RaggedPoints) and rd2.offsets is rq.offsets and rd2.packed.shape == (1500, 1)
    parts, iparts = rd2.split(), ridx.split()
    assert torch.equal(parts[0][:, 0], d2[0]) and torch.equal(iparts[0][:, 0], idx[0])
    assert torch.equal(parts[1][:, 0], d2[1, :5]) and torch.equal(iparts[1][:, 0] - 1500, idx[1, :5])
    assert torch.equal(eval_metric.nn_distance2_batch(rq, rs).split()[2], parts[2])


def test_sample_surface_batch_ranges_reproducibility_and_area_weighting(meshes):
    dd = _ragged_dict(meshes[:3])
    fi, bary = eval_metric.sample_surface_batch(dd["verts_tgt_pred"], dd["faces"], 4000, _gen(31))
    fi2, bary2 = eval_metric.sample_surface_batch(dd["verts_tgt_pred"], dd["faces"], 4000, _gen(31))
    assert torch.equal(fi, fi2) and torch.equal(bary, bary2)
    assert fi.shape == (3, 4000) and bary.shape == (3, 4000, 3)
    for b, F in enumerate((900, 40, 2000)):
        assert int(fi[b].min()) >= 0 and int(fi[b].max()) < F
        assert int(fi[b].max()) > F // 2                                   # (and the whole range is in use)
    assert bool((bary >= 0).all()) and torch.allclose(bary.sum(-1), torch.ones(3, 4000, device=DEV), atol=1e-6)
    # two triangles of areas 1.5 and 0.5 (and the same mesh again with the faces swapped, as a second shape)
    verts = torch.tensor([[0, 0, 0], [3, 0, 0], [0, 1, 0], [0, 0, 1], [1, 0, 1], [0, 1, 1]], dtype=torch.float32, device=DEV)
    faces = torch.tensor([[0, 1, 2], [3, 4, 5]], dtype=torch.int32, device=DEV)
    fi, _ = eval_metric.sample_surface_batch(torch.stack([verts, verts]), torch.stack([faces, faces.flip(0)]), 20000, _gen(32))
    share0, share1 = float((fi[0] == 0).float().mean()), float((fi[1] == 1).float().mean())
    assert abs(share0 - 0.75) <= 0.02 and abs(share1 - 0.75) <= 0.02      # six standard deviations of the binomial


def test_infer_command_reports_batch_metrics(tmp_path):
    import yaml
    from nsdp_amd.config import default_config
    cfg = default_config("forward")
    cfg["model"]["encoder_kwargs"]["npoints_per_layer"] = [256, 64, 16]
    (tmp_path / "forward.yaml").write_text(yaml.safe_dump(cfg))
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "LOCAL_WORLD_SIZE",
                                                             "MASTER_ADDR", "MASTER_PORT")}
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    p = subprocess.run([sys.executable, "-m", "nsdp_amd.infer", str(tmp_path / "forward.yaml"), "--surface", "256", "--steps", "2",
                        "--warmup", "1", "--reps", "1", "--vertex-counts", "300,500", "--metrics", "2000"],
                       capture_output=True, text=True, timeout=600, cwd=ROOT, env=env)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, p.stdout[-2000:]
    line = json.loads(lines[0])
    assert line["metrics_points"] == 2000 and set(line["metrics"]) == {"l2", "fnc", "cd"}
    for k in ("l2", "fnc", "cd"):
        assert len(line["metrics"][k]) == 2 and all(np.isfinite(v) for v in line["metrics"][k]), line["metrics"]
    assert line["metrics_ms_batch"] > 0 and line["metrics_ms_per_mesh_loop"] > 0
    assert 0 <= line["metrics_l2_fnc_max_abs_diff"] <= 1e-5


def test_metrics_batch_refuses_mismatched_layouts(meshes):
    rag, rect = _ragged_dict(meshes[:1]), _rect_dict(meshes[:1])
    with pytest.raises(RuntimeError, match="mismatched layouts"):
        eval_metric.compute_evaluation_metrics_batch({**rag, "verts_tgt": rect["verts_tgt"]}, samples=None)
    with pytest.raises(RuntimeError, match="mismatched layouts"):
        eval_metric.compute_evaluation_metrics_batch({**rag, "faces": rect["faces"]}, pointcloud_size=10)
    other = _ragged_dict([meshes[0], meshes[1]])
    with pytest.raises(RuntimeError, match="mismatched layouts"):         # one mesh of predictions, two of targets
        eval_metric.compute_evaluation_metrics_batch({**rag, "verts_tgt": other["verts_tgt"]}, pointcloud_size=10)
    same_rows = RaggedPoints.from_list([torch.zeros(100, 3, device=DEV), torch.zeros(400, 3, device=DEV)])
    pair = _ragged_dict([meshes[0]])                                       # 500 rows as (100, 400) against (500,)
    with pytest.raises(RuntimeError, match="mismatched layouts"):
        eval_metric.chamfer_distance_batch(pair["verts_tgt"], same_rows)
    with pytest.raises(RuntimeError, match="float32"):
        eval_metric.compute_evaluation_metrics_batch({**rect, "verts_tgt_pred": rect["verts_tgt_pred"].double()}, pointcloud_size=10)
