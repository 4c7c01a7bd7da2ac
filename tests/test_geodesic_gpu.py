"""GPU: geodesic distances (nsdp_amd/geodesic.py, include/nsdp_geodesic.h) against the numpy emulation of tests/geodesic_ref.py,
every comparison byte for byte: the edge table, and the fixed point from one triangle to meshes that straddle the block size
K = geodesic.BLOCK, a strip about 2 K hops long across more than four blocks (in the identity order, under a shuffle, one
round per call), poles of valence 3000 (lists beyond a lane and a wave), unreached components, zero-length edges, several seeds
with start values, a limit that falls exactly on a reachable distance, a packed batch with an empty shape and padding rows,
poses of one topology and a batch over shared faces.  NSDP_GEODESIC_NO_LOCAL and reorder=False give the same bytes; seeds of
NaN, negative values and -0 count as +inf; two runs give equal bits."""
import numpy as np
import pytest
import torch

import geodesic_ref as gr
import mesh_normals_ref as mr
from nsdp_amd import geodesic as g
from nsdp_amd import synth
from nsdp_amd.ragged import RaggedPoints

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
K = g.BLOCK
f32 = np.float32
INF = float("inf")


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _bits(x):
    x = x.packed if isinstance(x, RaggedPoints) else x
    x = x.detach().cpu().numpy() if torch.is_tensor(x) else np.asarray(x)
    return np.ascontiguousarray(x, dtype=f32).reshape(-1).view(np.uint32)


def _same(got, want):
    return np.array_equal(_bits(got), np.ascontiguousarray(want, dtype=f32).reshape(-1).view(np.uint32))


def _run(v, f, seeds=None, start=None, limit=INF, reorder=True, **kw):
    plan = g.GeodesicPlan(_t(f), _t(v), reorder=reorder)
    return g.geodesic_distances(_t(v), plan, None if seeds is None else _t(np.asarray(seeds, np.int64)),
                                None if start is None else _t(np.asarray(start, f32)), limit, **kw)


@pytest.fixture(scope="module")
def strip():
    """A strip of 4 K + 3 vertices, the fixed point from its first vertex, and a fixed shuffle of it."""
    v, f = gr.strip(4 * K + 3)
    D, hops = gr.geodesic(v, f, [0], return_hops=True)
    assert hops.max() >= 2 * K
    perm = np.random.default_rng(11).permutation(len(v))            # new row k holds old row perm[k]
    rank = np.empty(len(v), np.int64)
    rank[perm] = np.arange(len(v))
    return dict(v=v, f=f, D=D, perm=perm, rank=rank)


def test_block_size_is_the_librarys():
    from nsdp_amd import _lib
    assert _lib.lib().nsdp_mesh_geodesic_block() == K and K >= 64


def test_edge_table_bytes():
    v, f = gr.sphere_with(300)
    poses = np.stack([v, (v * f32(1.7))[:, [2, 0, 1]]])
    plan = g.GeodesicPlan(_t(f), _t(poses), reorder=False)
    nbr, length = g.edge_lengths(_t(poses), plan)
    lo, le, want_nbr, want_len = gr.edge_table(poses, f, [0, len(f)], [0, len(v)])
    assert np.array_equal(plan.list_offsets.cpu().numpy(), lo) and np.array_equal(plan.list_entries.cpu().numpy(), le)
    assert np.array_equal(nbr.cpu().numpy(), want_nbr) and _same(length, want_len) and tuple(length.shape) == (2, 6 * len(f))


def test_one_triangle():
    v = f32([[0, 0, 0], [3, 0, 0], [0, 4, 0]])
    f = np.int32([[0, 1, 2]])
    got, stats = _run(v, f, [1], return_stats=True)
    assert _same(got, [3, 0, 5]) and _same(got, gr.geodesic(v, f, [1])) and stats["rounds"] >= 1 and stats["calls"] >= 1


@pytest.mark.parametrize("V", [K - 1, K, K + 1, 3 * K + 5])
def test_meshes_that_straddle_the_block(V):
    v, f = gr.sphere_with(V, seed=V)
    want = gr.geodesic(v, f, [V // 3])
    assert np.isfinite(want).all()
    for reorder in (True, False):
        assert _same(_run(v, f, [V // 3], reorder=reorder), want), reorder
    assert _same(_run(v, f, [V // 3], no_local=True), want)                      # NSDP_GEODESIC_NO_LOCAL: the same bytes


def test_strip_in_the_identity_order(strip):
    got, stats = _run(strip["v"], strip["f"], [0], reorder=False, return_stats=True)
    assert _same(got, strip["D"])
    assert stats["rounds"] <= 16, stats            # four blocks and a bit, each relaxed to convergence: a handful of rounds


def test_strip_under_a_fixed_shuffle(strip):
    s = strip
    got, stats = _run(s["v"][s["perm"]], s["rank"][s["f"]], [s["rank"][0]], reorder=False, return_stats=True)
    assert _same(got.cpu()[torch.from_numpy(s["rank"])], s["D"]) and stats["rounds"] <= len(s["v"]) + 1
    again = _run(s["v"][s["perm"]], s["rank"][s["f"]], [s["rank"][0]], reorder=True)      # the plan's Morton order mends it
    assert _same(again.cpu()[torch.from_numpy(s["rank"])], s["D"])


def test_strip_with_one_round_per_call(strip):
    got, stats = _run(strip["v"], strip["f"], [0], reorder=False, rounds_per_call=1, return_stats=True)
    assert _same(got, strip["D"]) and stats["calls"] == stats["rounds"] >= 4      # many continuation calls
    plain, pstats = _run(strip["v"], strip["f"], [0], reorder=False, rounds_per_call=64, no_local=True, return_stats=True)
    assert _same(plain, strip["D"]) and pstats["rounds"] > stats["rounds"]


def test_poles_of_valence_3000():
    v, f = synth.sphere_mesh(2, 3000)
    v = v.astype(f32)
    want = gr.geodesic(v, f, [17])
    assert np.isfinite(want).all()
    assert _same(_run(v, f, [17]), want) and _same(_run(v, f, [17], reorder=False, no_local=True), want)
    assert _same(_run(v, f, [6000]), gr.geodesic(v, f, [6000]))                  # from a pole: its list feeds everything


def test_unreached_components_are_inf():
    a, fa = mr.sphere(6, 9)
    b, fb = mr.sphere(5, 7)
    v = np.concatenate([a, b + 3, [[9, 9, 9]]]).astype(f32)                      # two spheres and an isolated vertex
    f = np.concatenate([fa, np.asarray(fb) + len(a)]).astype(np.int32)
    want = gr.geodesic(v, f, [2])
    got = _run(v, f, [2])
    assert _same(got, want) and np.isinf(want[len(a):]).all() and np.isfinite(want[:len(a)]).all()


def test_zero_length_edges_carry_zero_across():
    v, f = gr.sphere_with(200)
    v = v.copy()
    v[40:60] = v[40]                                                             # duplicated coordinates
    want = gr.geodesic(v, f, [41])
    assert (want == 0).sum() >= 2
    assert _same(_run(v, f, [41]), want)


def test_several_seeds_with_start_values_and_bad_ones():
    v, f = gr.sphere_with(K + 77)
    start = np.full(len(v), np.inf, f32)
    start[[5, K // 2, K + 50]] = [0.25, 0.0, 1.5]
    start[[6, 7, 8, 9]] = [np.nan, -1.0, -0.0, -np.inf]                          # count as +inf
    want = gr.geodesic(v, f, start=start)
    clean = start.copy()
    clean[[6, 7, 8, 9]] = np.inf
    assert _same(want, gr.geodesic(v, f, start=clean)) and want[8] > 0
    assert _same(_run(v, f, start=start), want)
    assert _same(_run(v, f, seeds=[5, -1, 10 ** 6], start=start), gr.geodesic(v, f, seeds=[5], start=start))


def test_limit_exactly_on_a_reachable_distance():
    v, f = gr.sphere_with(700)
    full = gr.geodesic(v, f, [0])
    order = np.sort(np.unique(full))
    lim = float(order[len(order) // 2])
    want = gr.geodesic(v, f, [0], limit=lim)
    assert _same(want, np.where(full <= lim, full, np.inf)) and (want == f32(lim)).any()      # equality kept, the next dropped
    got = _run(v, f, [0], limit=lim)
    assert _same(got, want)
    plan = g.GeodesicPlan(_t(f), _t(v))
    ball = g.geodesic_ball(_t(v), plan, _t(np.int64([0])), lim)
    assert ball.dtype == torch.uint8 and np.array_equal(ball.cpu().numpy(), (full <= lim).astype(np.uint8))
    assert _same(_run(v, f, [0], limit=0.0), np.where(full == 0, full, np.inf))


def test_packed_batch_with_an_empty_shape_and_padding_rows():
    (va, fa), (vc, fc) = gr.sphere_with(K + 30), gr.sphere_with(150)
    verts = RaggedPoints.from_list([_t(va), _t(np.zeros((0, 3), f32)), _t(vc)], capacity=len(va) + len(vc) + 9)
    faces = RaggedPoints.from_rows([_t(fa), _t(np.zeros((0, 3), np.int32)), _t(fc)], capacity=len(fa) + len(fc) + 5)
    verts.packed[len(va) + len(vc):] = float("nan")
    seeds = _t(np.int64([[3, 40], [0, -1], [-1, 149]]))
    want = np.concatenate([gr.geodesic(va, fa, [3, 40]), gr.geodesic(vc, fc, [149]), np.full(9, np.inf, f32)])
    for reorder in (True, False):
        plan = g.GeodesicPlan(faces, verts, reorder=reorder)
        got = g.geodesic_distances(verts, plan, seeds)
        assert isinstance(got, RaggedPoints) and tuple(got.packed.shape) == (verts.capacity, 1) and _same(got, want), reorder


def test_poses_of_one_topology_and_a_batch_over_shared_faces():
    v, f = gr.sphere_with(K + 5)
    poses = np.stack([v, (v * f32(0.5))[:, [1, 2, 0]], v + f32(0.01) * np.sin(v * f32(9)).astype(f32)])       # P = 3
    seeds = np.int64([[0], [K], [77]])
    want = np.stack([gr.geodesic(poses[p], f, seeds[p]) for p in range(3)])
    plan = g.GeodesicPlan(_t(f), _t(poses))
    got = g.geodesic_distances(_t(poses), plan, _t(seeds))
    assert tuple(got.shape) == (3, len(v)) and _same(got, want)
    one = g.geodesic_distances(_t(poses), plan, _t(np.int64([77])))              # one seed set for every pose
    assert _same(one[2], want[2])
    own = g.GeodesicPlan(_t(np.stack([f, f[::-1], f])), _t(poses))               # faces of their own: [B, F, 3] with [B, V, 3]
    assert own.topology.kind == "batched" and _same(g.geodesic_distances(_t(poses), own, _t(seeds)), want)


def test_two_runs_give_equal_bits():
    v, f = gr.sphere_with(2 * K + 1)
    a, b = _run(v, f, [1, 2 * K]), _run(v, f, [1, 2 * K])
    assert np.array_equal(_bits(a), _bits(b))


def test_wrapper_refusals_on_the_device():
    v, f = gr.sphere_with(50)
    plan = g.GeodesicPlan(_t(f), _t(v))
    with pytest.raises(g.GeodesicError, match="no seeds"):
        g.geodesic_distances(_t(v), plan)
    with pytest.raises(g.GeodesicError, match="NaN or negative"):
        g.geodesic_distances(_t(v), plan, _t(np.int64([0])), limit=-1.0)
    with pytest.raises(g.GeodesicError, match="rounds_per_call"):
        g.geodesic_distances(_t(v), plan, _t(np.int64([0])), rounds_per_call=0)
