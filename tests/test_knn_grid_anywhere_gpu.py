"""GPU: the cell-grid search (include/nsdp_search.h, csrc/knn_grid.hip) away from centred surfaces -- clouds far from the
origin, boxes a few ulps wide, a cloud that fills its volume, a clustered surface, and queries that end in the wave-cooperative
exhaustive finish.  Expected results are always the scan's on the same inputs (``knn_grid_mode("0")``), compared on indices and
distance BITS; the stats words say whether the search pruned (tests) and how many queries took the finish (scanned)."""
import numpy as np
import pytest
import torch

from nsdp_amd import pointnet2_utils as pu
from nsdp_amd.ragged import RaggedPoints
from test_knn_grid_gpu import _dev, _family, _same, _scan, _sphere

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)


def _self_search(cloud, k):
    """(result, stats) of the grid's self-search of one cloud (m, 3), held against the scan."""
    xyz = _dev(cloud[None])
    got = pu.knn_grid(xyz, xyz, k, return_dist=True)
    stats = pu.knn_grid_stats()
    _same(got, _scan(xyz, xyz, k))
    assert stats["queries"] == cloud.shape[0]
    return got, stats


def test_translated_sphere_prunes_like_the_centred_one():
    """Coordinates on multiples of 2^-8 and a translate whose ulp is 2^-8: the translate is exact, every coordinate difference is
    the centred cloud's, and the stop rule works on differences against the box's corner.  (With a slack that follows the largest
    coordinate, 2^-18 * 32768.5 = 0.125 against five cells = 0.070, every bound is 0 and all 20 000 queries take the finish.)"""
    n, k = 20000, 16
    centred = (np.round(_sphere(np.random.default_rng(77), n) * 256.0) / 256.0).astype(np.float32)
    moved = centred + np.array([32768.0, -32768.0, 32768.0], np.float32)
    assert moved.dtype == np.float32 and np.array_equal((moved.astype(np.float64) - [32768.0, -32768.0, 32768.0]), centred.astype(np.float64))
    _, at_home = _self_search(centred, k)
    _, away = _self_search(moved, k)
    print("knn_grid stats, quantised 20 000-point sphere: centred", at_home, "translated", away)
    assert away["scanned"] == 0
    assert away["tests"] <= 1.05 * at_home["tests"]


SMALL = {"sphere": np.array([2000.0, -1500.0, 900.0], np.float32), "lattice": np.array([1024.0, 1024.0, 1024.0], np.float32)}


@pytest.mark.parametrize("name", sorted(SMALL))
def test_translated_small_clouds(name):
    """Rectangular, and as two shapes of one packed set: the translated shape beside the centred one.  (1024 + i / 8 is exact.)"""
    centred, k = _family(name), 16
    moved = centred + SMALL[name]
    _self_search(moved, k)
    r = RaggedPoints.from_list([_dev(moved), _dev(centred[:2500])])
    n_max = moved.shape[0]
    got = pu.knn_grid_ragged_source(r.packed, r.packed, r.offsets, k, n_max, query_offsets=r.offsets, return_dist=True)
    with pu.knn_grid_mode("0"):
        want = pu.knn_ragged_source(r.packed, r.packed, r.offsets, k, n_max, query_offsets=r.offsets, return_dist=True)
    _same(got, want)


def test_box_of_a_few_ulps():
    """{0, 1, 2, 3} * 2^-7 per axis around 65536, where 2^-7 is the ulp: 64 distinct points, duplicates and exact ties only."""
    rng = np.random.default_rng(65536)
    cloud = (rng.integers(0, 4, (2000, 3)) * 2.0 ** -7 + np.array([65536.0, -65536.0, 65536.0])).astype(np.float32)
    assert len(np.unique(cloud, axis=0)) == 64
    _self_search(cloud, 16)


def test_volume_is_pruned():
    """A uniform cube at the surface's G: 0.06 points per cell, k = 32.  A fixed four shells held k points for 0.2 % of these
    queries; shells under the work budget need five to nine, about 90 tests and 360 rows per query."""
    n, k = 20000, 32
    cloud = np.random.default_rng(1).uniform(-0.5, 0.5, (n, 3)).astype(np.float32)
    _, stats = _self_search(cloud, k)
    print("knn_grid stats, 20 000-point uniform cube, k = 32:", stats)
    assert stats["scanned"] <= 200
    assert stats["tests"] <= n * n // 8


def test_clustered_surface_keeps_its_sparse_part_in_the_shells():
    """1 000 points over the sphere and about 10 000 on its cap z > 0.4975: the sparse part's queries (9 % of all) need up to ten
    shells.  At most 2 % of the queries may take the finish."""
    rng = np.random.default_rng(4975)
    sparse = _sphere(rng, 1000)
    dense = _sphere(rng, 4_000_000)
    dense = dense[dense[:, 2] > 0.4975]
    assert 9000 <= dense.shape[0] <= 11000
    cloud = np.concatenate([sparse, dense])
    _, stats = _self_search(cloud, 16)
    print("knn_grid stats, clustered surface of", cloud.shape[0], "points:", stats)
    assert stats["scanned"] <= 0.02 * cloud.shape[0]


# ---------------------------------------------------------------------------------------------------------------- the finish
# Queries 50 standard deviations wide around a cloud of extent 1: each lies farther outside the box than the box is wide on some
# axis (all three within 1.5 of the centre has probability 1e-5), gets no budget for shells and, its cell clamped into a grid
# of 28 cells per axis, cannot cover the grid with shell 0: every one of them takes the finish.
def _far(seed, shape):
    return (np.random.default_rng(seed).standard_normal(shape) * 50.0).astype(np.float32)


@pytest.fixture(scope="module")
def sphere3000():
    return _dev(_sphere(np.random.default_rng(10), 3000)[None])


@pytest.mark.parametrize("k", [1, 7, 16, 32])
@pytest.mark.parametrize("n", [1, 45, 46, 63, 64, 65, 130])
def test_far_queries_take_the_cooperative_finish(sphere3000, n, k):
    """Partial waves, one full wave, a second wave with a single live lane; every list length the kernel is compiled for.  Up to
    45 needy lanes in a wave (kCrowd) the queries are broadcast, from 46 the rows: 1 and 45 take the first form, 46, 63 and 64
    the second, 65 and 130 both, one wave each (k = 32 has the second form alone)."""
    query = _dev(_far(1000 * n + k, (1, n, 3)))
    got = pu.knn_grid(query, sphere3000, k, return_dist=True)
    stats = pu.knn_grid_stats()
    _same(got, _scan(query, sphere3000, k))
    assert stats["queries"] == n and stats["scanned"] == n
    assert stats["tests"] >= n * 3000


def test_finish_beside_lanes_that_proved():
    """Every other lane far outside, the others on the surface: the lanes that stopped in their shells take part in the finish of
    their neighbours and keep their own lists."""
    rng = np.random.default_rng(11)
    source = _sphere(rng, 3000)
    query = (source[:130] * 1.001).astype(np.float32)
    query[::2] = _far(12, (65, 3))
    q, s = _dev(query[None]), _dev(source[None])
    got = pu.knn_grid(q, s, 16, return_dist=True)
    stats = pu.knn_grid_stats()
    _same(got, _scan(q, s, 16))
    assert stats["scanned"] == 65


def test_finish_over_a_lattice_of_ties():
    """Exact ties among the candidates of one step and across steps: the insertion order (distance, index) decides, as in the scan."""
    source = _dev(_family("lattice")[None])
    query = _dev(np.round(_far(13, (1, 65, 3))))          # (integer coordinates: whole planes of the lattice at one distance)
    got = pu.knn_grid(query, source, 16, return_dist=True)
    stats = pu.knn_grid_stats()
    _same(got, _scan(query, source, 16))
    assert stats["scanned"] == 65


def test_finish_in_a_shape_shorter_than_k():
    """A packed source whose second shape has 5 rows, k = 16: the finish leaves the shape's first row and FLT_MAX in the empty
    slots, as the scan does."""
    rng = np.random.default_rng(14)
    counts, k, n = (3000, 5), 16, 65
    xyz = _dev(np.concatenate([_sphere(rng, 3000), rng.uniform(-0.5, 0.5, (5, 3)).astype(np.float32)]))
    off = _dev(np.array([0, 3000, 3005], np.int32))
    query = _dev(_far(15, (2, n, 3)))
    got = pu.knn_grid_ragged_source(query, xyz, off, k, max(counts), return_dist=True)
    stats = pu.knn_grid_stats()
    with pu.knn_grid_mode("0"):
        want = pu.knn_ragged_source(query, xyz, off, k, max(counts), return_dist=True)
    _same(got, want)
    assert stats["scanned"] == 2 * n
    assert bool((got[0][1, :, 5:] == 3000).all()) and bool((got[1][1, :, 5:] == np.finfo(np.float32).max).all())


def test_outlier_alone_takes_the_finish():
    """One needy lane in a wave whose other lanes proved long ago (the existing `outlier` family, here far from the origin)."""
    cloud = _family("outlier") + np.array([500.0, 0.0, -500.0], np.float32)
    _, stats = _self_search(cloud, 16)
    assert stats["scanned"] == 1 and stats["tests"] <= 3000 * 1500 + 2 * 3001


def test_captured_translated_call_follows_the_clouds_contents():
    """One call in a graph over static buffers, far from the origin; the contents change between replays."""
    rng = np.random.default_rng(32)
    shift = np.array([2000.0, -1500.0, 900.0], np.float32)
    clouds = [_dev((_sphere(rng, 1500) + shift)[None]), _dev((rng.uniform(-1, 1, (1, 1500, 3)) + shift).astype(np.float32)),
              _dev((rng.integers(0, 9, (1, 1500, 3)) / 4.0 + 1024.0).astype(np.float32)),
              _dev(np.concatenate([_sphere(rng, 1499, 0.05) + shift, -shift[None]])[None])]      # (one row far away: a finish)
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
