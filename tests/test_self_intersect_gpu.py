"""GPU: nsdp_mesh_self_intersections against the numpy emulation of its header (tests/self_intersect_ref.py), byte for byte on
every output: the inputs of the table, block edges in a packed batch, several poses, the three forms that must agree (culled,
unculled, shuffled under face_ids), rows nobody owns, degenerate faces, the work guard, and one mid-size case in which the
culling by block boxes has something to skip.  On the four clear inputs the kernel's hits are the EXACT verdicts too."""
import numpy as np
import pytest
import torch

import self_intersect_ref as sr
from nsdp_amd.ragged import RaggedPoints
from nsdp_amd.synth import sphere_mesh

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
KEYS = ("cand", "hits", "partner", "pairs", "skipped")


def run(verts, faces, fo, vo, ids=None, budget=0, cull=True):
    """The raw entry on numpy operands; verts (vcap, 3) or (P, vcap, 3) -> dict of numpy arrays with a leading P."""
    from nsdp_amd import self_intersect as si
    v = torch.from_numpy(np.ascontiguousarray(verts, np.float32).reshape(-1, verts.shape[-2], 3)).to(DEV)
    t = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a, np.int32)).to(DEV)
    out = si.mesh_self_intersections(v, t(vo), t(faces), t(fo), t(ids), budget=budget, cull=cull)
    return {k: o.cpu().numpy() for k, o in zip(KEYS, out)}


def same(got, want, pose=0):
    for k in KEYS:
        assert got[k].dtype == want[k].dtype and np.array_equal(got[k][pose], want[k]), (k, pose, got[k][pose], want[k])


def soup(n, seed):
    rng = np.random.default_rng(seed)
    v = (rng.uniform(-1, 1, (n, 1, 3)) + rng.normal(0, 0.25, (n, 3, 3))).reshape(-1, 3).astype(np.float32)
    return v, np.arange(3 * n).reshape(n, 3).astype(np.int32)


@pytest.mark.parametrize("name", list(sr.inputs()))
def test_every_input_of_the_table(name):
    from nsdp_amd import self_intersect as si
    v, f = sr.inputs()[name]
    verts, faces, fo, vo = sr.pack([(v, f)])
    want = sr.self_intersections(verts, faces, fo, vo)
    got = run(verts, faces, fo, vo)
    same(got, want)
    assert np.array_equal(run(verts, faces, fo, vo)["partner"], got["partner"])                   # two runs, the same bytes
    r = sr.solved(name)
    assert want["pairs"][0] == r["hit"].sum() and np.array_equal(want["hits"], r["hits"])
    if name in sr.CLEAR_INPUTS:                                                                   # every pair clear: the truth
        verdict, clear, _ = sr.exact(name)
        assert clear.all()
        truth = np.bincount(np.concatenate([r["I"][verdict], r["J"][verdict]]), minlength=len(f))
        assert np.array_equal(got["hits"][0], truth) and got["pairs"][0, 0] == verdict.sum()
    if name in ("sphere", "sphere_twice"):
        assert got["pairs"][0, 0] == 0 and not got["hits"].any() and (got["partner"] == -1).all()
    # the wrapper: a plan reorders the faces along a Morton curve and reports under the caller's rows
    tv, tf = torch.from_numpy(v).to(DEV), torch.from_numpy(f).to(DEV)
    plan = si.SelfIntersectionPlan(tf, tv)
    assert plan.face_ids is not None and sorted(plan.face_ids.tolist()) == list(range(len(f)))
    res = si.self_intersections(tv, plan, budget=0)
    assert res.hits.shape == (len(f),) and res.pairs.shape == () and res.pairs.dtype == torch.int64
    for k in ("cand", "hits", "partner"):
        assert np.array_equal(getattr(res, k).cpu().numpy(), want[k]), k
    assert int(res.pairs) == want["pairs"][0] and int(res.skipped) == 0 and int(res.faces_hit) == (want["hits"] > 0).sum()


def test_packed_batch_with_block_edges_an_empty_mesh_and_a_partial_last_block():
    from nsdp_amd import self_intersect as si
    meshes = []
    for k, n in enumerate((0, 1, 63, 64, 65, 129)):
        v, f = soup(max(n, 1), 10 + k)
        meshes.append((v, f[:n]))
    meshes.insert(3, sr.inputs()["spheres"])
    verts, faces, fo, vo = sr.pack(meshes, vpad=7, fpad=70)
    want = sr.self_intersections(verts, faces, fo, vo)
    assert want["pairs"][3] == 53 and (want["pairs"][[2, 4, 5, 6]] > 0).all() and want["pairs"][0] == want["pairs"][1] == 0
    for cull in (True, False):
        same(run(verts, faces, fo, vo, cull=cull), want)
    # the ragged layout of the wrapper: partner local to its mesh, faces_hit per mesh
    rv = RaggedPoints(torch.from_numpy(verts).to(DEV), torch.from_numpy(vo).to(DEV))
    rf = RaggedPoints(torch.from_numpy(faces).to(DEV), torch.from_numpy(fo).to(DEV))
    res = si.self_intersections(rv, si.SelfIntersectionPlan(rf, rv), budget=0)
    assert np.array_equal(res.hits.cpu().numpy(), want["hits"]) and np.array_equal(res.pairs.cpu().numpy(), want["pairs"])
    first = np.repeat(fo[:-1], np.diff(fo))
    local = np.where(want["partner"][:fo[-1]] >= 0, want["partner"][:fo[-1]] - first, -1)
    assert np.array_equal(res.partner.cpu().numpy()[:fo[-1]], local)
    hit = [(want["hits"][fo[b]:fo[b + 1]] > 0).sum() for b in range(len(meshes))]
    assert res.faces_hit.cpu().tolist() == hit


def test_three_poses_of_one_topology():
    from nsdp_amd import self_intersect as si
    v, f = sphere_mesh(6, 8)
    rng = np.random.default_rng(1)
    vj = v + rng.normal(0, 0.01, v.shape)
    poses = np.stack([np.concatenate([vj, v + shift]) for shift in ([2.0, 0.0, 0.0], [0.81, 0.0, 0.0], [0.31, 0.07, 0.05])]).astype(np.float32)
    faces = np.concatenate([f, f + len(v)]).astype(np.int32)
    _, _, fo, vo = sr.pack([(poses[0], faces)])
    got = run(poses, faces, fo, vo)
    want = [sr.self_intersections(p, faces, fo, vo) for p in poses]
    for p in range(3):
        same(got, want[p], p)
    assert want[0]["pairs"][0] == 0 and want[2]["pairs"][0] > 20
    tv, tf = torch.from_numpy(poses).to(DEV), torch.from_numpy(faces).to(DEV)
    res = si.self_intersections(tv, si.SelfIntersectionPlan(tf, tv), budget=0)           # (the plan's order is pose 0's)
    assert res.hits.shape == (3, len(faces)) and res.pairs.tolist() == [int(w["pairs"][0]) for w in want]
    assert np.array_equal(res.partner.cpu().numpy(), np.stack([w["partner"] for w in want]))
    # faces of their own per mesh: [B, F, 3] with [B, V, 3]
    res = si.self_intersections(tv, si.SelfIntersectionPlan(tf[None].expand(3, -1, -1).contiguous(), tv), budget=0)
    assert res.hits.shape == (3, len(faces)) and res.pairs.shape == (3,) and res.pairs.tolist() == [int(w["pairs"][0]) for w in want]


def test_culled_unculled_and_shuffled_agree_and_partner_is_the_smallest_original_row():
    v, f = sr.inputs()["spheres"]
    verts, faces, fo, vo = sr.pack([(v, f)], vpad=2, fpad=9)
    want = sr.self_intersections(verts, faces, fo, vo)
    perm = np.random.default_rng(8).permutation(len(f))
    shuffled, ids = faces.copy(), np.arange(len(faces), dtype=np.int32)
    shuffled[:len(f)], ids[:len(f)] = f[perm], perm
    ids[len(f):] = -12345                                                                 # (rows nobody owns: never read)
    assert all(np.array_equal(sr.self_intersections(verts, shuffled, fo, vo, face_ids=ids)[k], want[k]) for k in KEYS)
    for got in (run(verts, faces, fo, vo), run(verts, faces, fo, vo, cull=False), run(verts, shuffled, fo, vo, ids=ids),
                run(verts, shuffled, fo, vo, ids=ids, cull=False)):
        same(got, want)
    r = sr.solved("spheres")
    for q in np.flatnonzero(want["hits"] > 0):
        mates = np.concatenate([r["J"][r["hit"] & (r["I"] == q)], r["I"][r["hit"] & (r["J"] == q)]])
        assert want["partner"][q] == mates.min() and want["hits"][q] == len(mates)


def test_stale_offsets_and_wild_indices():
    v, f = sr.inputs()["soup"]
    verts, faces, fo, vo = sr.pack([(v[:90], f[:30]), (v, f)], vpad=5, fpad=40)
    verts[vo[-1]:] = np.nan                                                               # rows nobody owns
    faces[fo[-1]:] = np.array([-1, 1 << 30, -(1 << 31)], np.int32)
    faces[3] = [-7, 1 << 29, 5]                                                           # an owned face with indices outside its mesh: clamped
    same(run(verts, faces, fo, vo), sr.self_intersections(verts, faces, fo, vo))
    for bad_fo, bad_vo in ((np.array([0, 30, 10 ** 9], np.int32), vo), (np.array([-5, 30, 20], np.int32), vo),
                           (fo, np.array([0, 90, 10 ** 9], np.int32)), (fo, np.array([0, 0, 450], np.int32))):
        clean = np.nan_to_num(verts)                                                      # (stale offsets may own the padding rows)
        tame = faces.copy()
        tame[fo[-1]:] = 0
        same(run(clean, tame, bad_fo, bad_vo), sr.self_intersections(clean, tame, bad_fo, bad_vo))


def test_zero_area_and_repeated_corner_faces():
    v, f = sr.inputs()["soup"]
    f = f.copy()
    f[:20, 2] = f[:20, 1]                                                                 # a repeated corner (by index)
    v = v.copy()
    v[f[20:40, 2]] = v[f[20:40, 0]]                                                       # ... by coordinates
    v[f[40:60, 2]] = (v[f[40:60, 0]] + v[f[40:60, 1]]) * np.float32(0.5)                  # collinear within rounding
    v[f[60:70]] = v[f[60:70, :1]]                                                         # a point
    verts, faces, fo, vo = sr.pack([(v, f)])
    want = sr.self_intersections(verts, faces, fo, vo)
    same(run(verts, faces, fo, vo), want)
    assert want["pairs"][0] > 0 and (want["hits"][60:70] == 0).all()


def test_the_work_guard():
    v, f = sr.inputs()["soup"]
    verts, faces, fo, vo = sr.pack([(v, f), sr.inputs()["spheres"]], fpad=3)
    free = sr.self_intersections(verts, faces, fo, vo)
    budget = 6
    over = free["cand"] > budget
    assert 0 < over[:120].sum() < 120
    want = sr.self_intersections(verts, faces, fo, vo, budget=budget)
    for cull in (True, False):
        got = run(verts, faces, fo, vo, budget=budget, cull=cull)
        same(got, want)
        assert np.array_equal(got["hits"][0] == -1, over) and np.array_equal(got["cand"][0], free["cand"])
        assert got["skipped"][0].tolist() == [over[:120].sum(), over[120:].sum()]
    r = sr.mesh_result(v[f])
    keep = r["hit"] & ~over[r["I"]] & ~over[r["J"]]
    assert want["pairs"][0] == keep.sum() < r["hit"].sum()
    same(run(verts, faces, fo, vo, budget=0), free)                                       # budget = 0: the unguarded emulation
    same(run(verts, faces, fo, vo, budget=10 ** 6), free)                                 # ... and a budget nobody exceeds, in two passes


@pytest.fixture(scope="module")
def midsize():
    v, f = sphere_mesh(20, 40)
    rng = np.random.default_rng(2)
    verts = np.concatenate([v, v + np.array([0.31, 0.07, 0.05]) + rng.normal(0, 0.002, v.shape)]).astype(np.float32)
    faces = np.concatenate([f, f + len(v)]).astype(np.int32)
    packed = sr.pack([(verts, faces)])
    return packed, sr.self_intersections(*packed)


def test_mid_size_where_block_culling_skips(midsize):
    from nsdp_amd import self_intersect as si
    (verts, faces, fo, vo), want = midsize
    assert len(faces) == 3200 and want["pairs"][0] > 100
    same(run(verts, faces, fo, vo), want)
    same(run(verts, faces, fo, vo, cull=False), want)
    tv, tf = torch.from_numpy(verts).to(DEV), torch.from_numpy(faces).to(DEV)
    plan = si.SelfIntersectionPlan(tf, tv)
    for budget in (0, None):                                                              # (the default budget skips nothing here)
        res = si.self_intersections(tv, plan, budget=budget)
        assert all(np.array_equal(getattr(res, k).cpu().numpy(), want[k]) for k in ("cand", "hits", "partner"))
        assert int(res.pairs) == want["pairs"][0] and int(res.skipped) == 0


def test_capturable_and_refusals(midsize):
    from nsdp_amd import self_intersect as si
    (verts, faces, _, _), want = midsize
    tv, tf = torch.from_numpy(verts).to(DEV), torch.from_numpy(faces).to(DEV)
    plan = si.SelfIntersectionPlan(tf, tv)
    si.self_intersections(tv, plan)                                                       # (warm: the library is loaded)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        res = si.self_intersections(tv, plan)
    g.replay()
    torch.cuda.synchronize()
    assert np.array_equal(res.hits.cpu().numpy(), want["hits"]) and int(res.pairs) == want["pairs"][0]
    with pytest.raises(si.SelfIntersectError, match="GPU tensor"):
        si.self_intersections(tv.cpu(), plan)
    with pytest.raises(si.SelfIntersectError, match="budget"):
        si.self_intersections(tv, plan, budget=-1)
    with pytest.raises(si.SelfIntersectError, match="outside"):
        si.SelfIntersectionPlan(tf + 5000, tv)
