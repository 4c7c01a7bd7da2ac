"""GPU: nsdp_mesh_ray_cast (include/nsdp_raycast.h) against its numpy emulation (tests/ray_cast_ref.py) BYTE FOR BYTE -- t,
face, bary, count -- at the smallest shapes that can go wrong: a partial wave, a partial last block, three blocks (several parts
meet in the atomics), a packed batch with an empty mesh and a mesh without vertices, stale indices and offsets, the tie set,
every form (culled, NO_CULL, with and without count_out) on a Morton-ordered sphere, the three Python layouts and a replayed
capture."""
import numpy as np
import pytest
import torch

import ray_cast_ref as rr

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
f32 = np.float32


def _dev(a, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(a if dtype is None else np.asarray(a).astype(dtype))).to(DEV)


def _entry(o, d, roff, v, voff, f, foff, cull, count=True, bary=True):
    from nsdp_amd import ray_cast as rc
    t, face, b, c = rc.mesh_ray_cast(_dev(o, f32), _dev(d, f32), _dev(roff, np.int32), _dev(v, f32), _dev(voff, np.int32),
                                     _dev(f, np.int32), _dev(foff, np.int32), return_bary=bary, count=count, cull=cull)
    torch.cuda.synchronize()
    return (t.cpu().numpy(), face.cpu().numpy(), None if b is None else b.cpu().numpy(), None if c is None else c.cpu().numpy())


def _same(got, want, live, what=""):
    """Bytes: fp32 compared as their bit patterns."""
    t, face, bary, count = got
    wt, wf, wb, wc = want
    assert np.array_equal(t[:live].view(np.uint32), wt[:live].view(np.uint32)), what
    assert np.array_equal(face[:live], wf[:live]), what
    if bary is not None:
        assert np.array_equal(bary[:live].view(np.uint32), wb[:live].view(np.uint32)), what
    if count is not None:
        assert np.array_equal(count[:live], wc[:live]), what


def _soup(F, n, seed):
    """F random faces around the origin of coordinates (a few degenerate ones) over V vertices, n rays from a shell around
    them aimed at random points inside -- most rays cross several faces."""
    rng = np.random.default_rng(seed)
    V = max(3, F // 2 + 2)
    v = rng.normal(0, 1, (V, 3)).astype(f32)
    f = rng.integers(0, V, (F, 3))
    o = rng.normal(0, 1, (n, 3))
    o = (3 * o / np.linalg.norm(o, axis=1, keepdims=True)).astype(f32)
    d = (rng.normal(0, 0.5, (n, 3)).astype(f32) - o).astype(f32)
    return v, f, o, d


@pytest.mark.parametrize("n", [1, 63, 64, 65, 200])
@pytest.mark.parametrize("F", [1, 63, 64, 65, 129])
def test_entry_equals_emulation(F, n):
    v, f, o, d = _soup(F, n, 7 * F + n)
    if F == 1:
        v[:3] = f32([[-4, -4, 0.5], [4, -4, 0.25], [0, 4, -0.5]])          # one large face that most rays cross
        f[0] = (0, 1, 2)
    args = (o, d, [0, n], v, [0, len(v)], f, [0, F])
    want = rr.ray_cast(*args)
    assert (want[3] > 0).sum() > 0
    for cull in (True, False):
        _same(_entry(*args, cull=cull), want, n, (F, n, cull))
        _same(_entry(*args, cull=cull, count=False, bary=False), want, n, (F, n, cull, "first hit"))


def _packed_batch():
    """B = 3: a soup of 129 faces with 70 rays, an EMPTY mesh (vertices, no faces) with 5 rays in the middle, and a mesh
    WITHOUT VERTICES with 66 rays -- its 12 face rows are a cube's, whose 8 vertices lie behind the last vertex offset (so new
    offsets can hand them over); the capacities end in rows of NaN / -1."""
    v0, f0, o0, d0 = _soup(129, 70, 5)
    vc, fc = rr.cube()
    rng = np.random.default_rng(9)
    oc = rng.uniform(-1.5, 1.5, (66, 3)).astype(f32)
    dc = rng.normal(0, 1, (66, 3)).astype(f32)
    o = np.concatenate([o0, o0[:5], oc, np.full((4, 3), np.nan, f32)])
    d = np.concatenate([d0, d0[:5], dc, np.full((4, 3), np.nan, f32)])
    v = np.concatenate([v0, v0[:4], vc, np.full((3, 3), np.nan, f32)])
    f = np.concatenate([f0, fc, np.full((5, 3), -1)])
    V0 = len(v0)
    return o, d, [0, 70, 75, 141], v, [0, V0, V0 + 4, V0 + 4], f, [0, 129, 129, 141]


def test_packed_batch_with_an_empty_mesh_and_a_mesh_without_vertices():
    args = _packed_batch()
    want = rr.ray_cast(*args)
    assert (want[1][70:141] == -1).all() and (want[3][70:141] == 0).all() and (want[3][:70] > 0).sum() > 20
    for cull in (True, False):
        _same(_entry(*args, cull=cull), want, 141, cull)
    # the third mesh with its vertices: packed face rows from 129 on
    args = args[:4] + ([0, args[4][1], args[4][2], args[4][2] + 8],) + args[5:]
    want = rr.ray_cast(*args)
    assert (want[3][75:141] > 0).sum() > 20 and ((want[1][75:141] == -1) | (want[1][75:141] >= 129)).all()
    for cull in (True, False):
        _same(_entry(*args, cull=cull), want, 141, cull)


def test_stale_indices_and_offsets_give_the_emulations_clamps():
    g = np.random.default_rng(3)
    qcap, vcap, fcap = 300, 50, 200
    o = g.normal(0, 2, (qcap, 3)).astype(f32)
    d = (-o + g.normal(0, 0.5, (qcap, 3))).astype(f32)
    v = g.normal(0, 1, (vcap, 3)).astype(f32)
    f = g.integers(-(1 << 31), (1 << 31) - 1, (fcap, 3))
    f[::3] = g.integers(-5, 60, (len(f[::3]), 3))                           # some inside, some just outside their mesh
    roff, voff, foff = [-5, 130, 100, 1 << 30], [0, 20, 20, 1 << 30], [7, 90, 150, -1]
    want = rr.ray_cast(o, d, roff, v, voff, f, foff)
    assert (want[3][:130] > 0).sum() > 10 and (want[1][130:] == -1).all()
    for cull in (True, False):
        _same(_entry(o, d, roff, v, voff, f, foff, cull=cull), want, 300, cull)


@pytest.mark.parametrize("name", ["cube", "sphere"])
def test_tie_set(name):
    """The WHOLE tie set of tests/test_ray_cast_ref_cpu.py -- every vertex and edge midpoint, every axis, diagonal and random
    direction, and the rays from the centre -- through both forms."""
    v, f = rr.cube() if name == "cube" else rr.uv_sphere(grid=4096)
    oo, do, oi, di = rr.tie_set(v, f)
    o, d = np.concatenate([oo, oi]), np.concatenate([do, di])
    args = (o, d, [0, len(o)], v, [0, len(v)], f, [0, len(f)])
    want = rr.ray_cast(*args)
    assert len(oo) == {"cube": 624, "sphere": 10416}[name] and len(oi) == {"cube": 26, "sphere": 434}[name]
    assert (want[3][:len(oo)] % 2 == 0).all() and (want[3][len(oo):] == 1).all()
    for cull in (True, False):
        _same(_entry(*args, cull=cull), want, len(o), (name, cull))


@pytest.fixture(scope="module")
def sphere_case():
    """A Morton-ordered sphere of 4992 faces, 2000 random rays (origins inside and outside) and 200 from far outside its box."""
    from nsdp_amd import ray_cast as rc
    v, f = rr.sphere()
    rng = np.random.default_rng(21)
    o = rng.uniform(-1.5, 1.5, (2000, 3)).astype(f32)
    d = rng.normal(0, 1, (2000, 3)).astype(f32)
    far = rng.normal(0, 1, (200, 3))
    far = (50 * far / np.linalg.norm(far, axis=1, keepdims=True)).astype(f32)
    o, d = np.concatenate([o, far]), np.concatenate([d, (rng.uniform(-1.2, 1.2, (200, 3)).astype(f32) - far).astype(f32)])
    plan = rc.RayCastPlan(_dev(f), _dev(v))
    assert plan.reordered and plan.open_edges == 0
    fm = plan.faces.cpu().numpy()
    want = rr.ray_cast(o, d, [0, len(o)], v, [0, len(v)], fm, [0, len(fm)])
    return v, f, fm, o, d, plan, want


def test_every_form_gives_the_same_bytes_on_a_morton_ordered_sphere(sphere_case):
    v, f, fm, o, d, plan, want = sphere_case
    args = (o, d, [0, len(o)], v, [0, len(v)], fm, [0, len(fm)])
    assert (want[3] % 2 == 0).sum() + (want[3] % 2 == 1).sum() == len(o) and 100 < (want[3] == 1).sum() and (want[3] == 2).sum() > 100
    for cull in (True, False):
        for count in (True, False):
            _same(_entry(*args, cull=cull, count=count, bary=count), want, len(o), (cull, count))


def test_python_layouts_agree_with_single_mesh_calls(sphere_case):
    from nsdp_amd import ray_cast as rc
    from nsdp_amd.ragged import RaggedPoints
    v, f, fm, o, d, plan, want = sphere_case
    o, d = o[:300], d[:300]
    # one mesh, the caller's face numbering: the reported face is the emulation's on the caller's own order wherever t is untied
    one = rc.cast_rays(_dev(o), _dev(d), _dev(v), plan)
    ref = rr.cast(o, d, v, f)
    assert np.array_equal(one.t.cpu().numpy().view(np.uint32), ref[0].view(np.uint32))
    assert np.array_equal(one.crossings.cpu().numpy(), ref[3]) and np.array_equal(one.hit.cpu().numpy(), ref[1] >= 0)
    tri = v[f]
    got_face, got_bary = one.face.cpu().numpy(), one.bary.cpu().numpy()
    hit = got_face >= 0
    point = (tri[got_face[hit]] * got_bary[hit][:, :, None]).sum(1)
    assert np.abs(point - (o[hit] + ref[0][hit][:, None] * d[hit])).max() < 1e-4
    # poses over shared faces: [2, V, 3] with rays [2, n, 3]; faces of their own [2, F, 3]; packed
    v2 = np.stack([v, v * f32(0.5) + f32(0.25)])
    o2, d2 = np.stack([o, o]), np.stack([d, d[::-1]])
    singles = [rc.cast_rays(_dev(o2[k]), _dev(d2[k]), _dev(v2[k]), plan) for k in range(2)]
    shared = rc.cast_rays(_dev(o2), _dev(d2), _dev(v2), plan)
    own_plan = rc.RayCastPlan(_dev(np.stack([f, f[::-1]])), _dev(v2), reorder=False)
    own = rc.cast_rays(_dev(o2), _dev(d2), _dev(v2), own_plan)
    rag_plan = rc.RayCastPlan(RaggedPoints.from_list([_dev(f), _dev(f[:2000])]), RaggedPoints.from_list([_dev(v2[0]), _dev(v2[1])]))
    ro = RaggedPoints.from_list([_dev(o2[0]), _dev(o2[1][:100])], capacity=450)
    rd = RaggedPoints.from_list([_dev(d2[0]), _dev(d2[1][:100])], capacity=450)
    rag = rc.cast_rays(ro, rd, RaggedPoints.from_list([_dev(v2[0]), _dev(v2[1])]), rag_plan)
    part = rr.cast(o2[1][:100], d2[1][:100], v2[1], f[:2000])
    for k in range(2):
        for name in ("t", "crossings", "hit"):
            assert torch.equal(getattr(shared, name)[k], getattr(singles[k], name)), (k, name)
            assert torch.equal(getattr(own, name)[k], getattr(singles[k], name)), (k, name)
        assert torch.equal(shared.face[k], singles[k].face) and torch.equal(shared.bary[k], singles[k].bary)
    flip = torch.where(own.face[1] >= 0, len(f) - 1 - own.face[1], own.face[1])            # the second mesh's faces are reversed
    untied = singles[1].crossings <= 1
    assert torch.equal(flip[untied], singles[1].face[untied])
    assert torch.equal(rag.t.packed[:300, 0], singles[0].t) and torch.equal(rag.face.packed[:300, 0], singles[0].face)
    assert np.array_equal(rag.t.packed[300:400, 0].cpu().numpy().view(np.uint32), part[0].view(np.uint32))
    assert np.array_equal(rag.crossings.packed[300:400, 0].cpu().numpy(), part[3])
    with pytest.raises(rc.RayCastError, match="mismatched layouts"):
        rc.cast_rays(ro, rd, _dev(v), plan)
    with pytest.raises(rc.RayCastError, match="dtype"):
        rc.cast_rays(_dev(o).double(), _dev(d).double(), _dev(v), plan)
    with pytest.raises(rc.RayCastError, match="CPU tensors"):
        rc.cast_rays(torch.from_numpy(o), torch.from_numpy(d), _dev(v), plan)
    with pytest.raises(rc.RayCastError, match="shape"):
        rc.cast_rays(_dev(o), _dev(d[:10]), _dev(v), plan)
    with pytest.raises(rc.RayCastError, match="outside"):
        rc.RayCastPlan(_dev(f) + 50000, _dev(v))
    assert rc.RayCastPlan(_dev(f[:-1]), _dev(v)).open_edges == 3 and rc.RayCastPlan(_dev(f).long(), _dev(v)).faces.dtype == torch.int32


def test_replayed_capture_with_changed_offsets_equals_the_eager_call():
    from nsdp_amd import ray_cast as rc
    args = list(_packed_batch())
    o, d, roff, v, voff, f, foff = [_dev(a, t) for a, t in zip(args, (f32, f32, np.int32, f32, np.int32, np.int32, np.int32))]
    rc.mesh_ray_cast(o, d, roff, v, voff, f, foff, cull=True)                  # (warm: the library is loaded)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        res = rc.mesh_ray_cast(o, d, roff, v, voff, f, foff, cull=True)
    g.replay()
    torch.cuda.synchronize()
    _same([x.cpu().numpy() for x in res], rr.ray_cast(*args), 141)
    # other offsets in the same tensors: the first mesh loses faces and rays, the third gets its vertices and the middle's rays
    new = ([0, 60, 60, 138], [0, args[4][1], args[4][2], args[4][2] + 8], [0, 100, 129, 141])
    for t, n in zip((roff, voff, foff), new):
        t.copy_(_dev(n, np.int32))
    g.replay()
    torch.cuda.synchronize()
    want = rr.ray_cast(args[0], args[1], new[0], args[3], new[1], args[5], new[2])
    assert (want[3][60:138] > 0).sum() > 20
    _same([x.cpu().numpy() for x in res], want, 138)
    eager = rc.mesh_ray_cast(o, d, roff, v, voff, f, foff, cull=True)
    torch.cuda.synchronize()
    _same([x.cpu().numpy() for x in eager], want, 138)


def test_reordered_rays_give_the_same_bytes_in_the_given_order(sphere_case):
    """The wrapper's ray reordering (what a large culled call does by itself) changes which rays share a wave, nothing else."""
    from nsdp_amd import ray_cast as rc
    from nsdp_amd.ragged import RaggedPoints
    v, f, fm, o, d, plan, want = sphere_case
    for count in (True, False):
        plain = rc.cast_rays(_dev(o), _dev(d), _dev(v), plan, count=count, cull=False, reorder=False)
        sorted_ = rc.cast_rays(_dev(o), _dev(d), _dev(v), plan, count=count, cull=True, reorder=True)
        assert torch.equal(plain.t.view(torch.int32), sorted_.t.view(torch.int32)) and torch.equal(plain.face, sorted_.face)
        assert torch.equal(plain.bary.view(torch.int32), sorted_.bary.view(torch.int32))
        assert (plain.crossings is None) == (not count) and (not count or torch.equal(plain.crossings, sorted_.crossings))
    assert np.array_equal(plain.t.cpu().numpy().view(np.uint32), want[0].view(np.uint32))
    perm = rc._ray_order(_dev(o), _dev(d), _dev(np.int32([0, len(o)])), _dev(v), _dev(np.int32([0, len(v)])))
    assert sorted(perm.tolist()) == list(range(len(o))) and perm.tolist() != list(range(len(o)))
    vs, fs = rr.uv_sphere()
    rv = RaggedPoints.from_list([_dev(v), _dev(vs)])
    rplan = rc.RayCastPlan(RaggedPoints.from_list([_dev(f), _dev(fs)]), rv)
    ro = RaggedPoints.from_list([_dev(o[:700]), _dev(o[700:1000])], capacity=1100)
    rd = RaggedPoints.from_list([_dev(d[:700]), _dev(d[700:1000])], capacity=1100)
    a, b = rc.cast_rays(ro, rd, rv, rplan, cull=True, reorder=True), rc.cast_rays(ro, rd, rv, rplan, cull=False, reorder=False)
    for name in ("t", "face", "bary", "crossings"):
        assert torch.equal(getattr(a, name).packed[:1000], getattr(b, name).packed[:1000]), name
    assert (b.crossings.packed[700:1000] > 0).sum() > 20
    assert rc._dispatch(1, 1 << 15, 1 << 14, None, None) == (True, True) and rc._dispatch(1, 1 << 14, 1 << 14, None, None) == (False, False)
    assert rc._dispatch(1, 100, 100, True, None) == (True, False)


def test_captured_cast_rays_with_reordering_and_a_plan_without_host_reads():
    """``cast_rays`` itself under capture in the form a large call takes (culled, rays reordered): the replay gives the eager
    bytes.  And a plan built with ``validate=False`` -- what evaluate builds per batch -- synchronises nowhere, its open edges
    included; the count is read back only where ``open_edges`` is asked for."""
    from nsdp_amd import ray_cast as rc
    v, f = rr.uv_sphere()
    rng = np.random.default_rng(31)
    o, d = rng.uniform(-1.5, 1.5, (500, 3)).astype(f32), rng.normal(0, 1, (500, 3)).astype(f32)
    from nsdp_amd.ragged import RaggedPoints
    to, td, tv, tf = _dev(o), _dev(d), _dev(v), _dev(f[:-3])
    vc, fc = rr.cube()
    # the packed layout evaluate uses (its offsets are on the device already: nothing is uploaded either); torch raises at every
    # synchronising call it knows of while the mode is "error"
    rv, rf = RaggedPoints.from_list([tv, _dev(vc)]), RaggedPoints.from_list([tf, _dev(fc)])
    ro, rd = RaggedPoints.from_list([to, to[:100]]), RaggedPoints.from_list([td, td[:100]])
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        packed_plan = rc.RayCastPlan(rf, rv, validate=False)
        packed = rc.cast_rays(ro, rd, rv, packed_plan, cull=True, reorder=True)
        inside = rc.contains(ro, rv, packed_plan)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert packed_plan.open_edges_per_mesh.tolist() == [rr.open_edges(f[:-3]), 0] and packed_plan.open_edges == rr.open_edges(f[:-3]) > 0
    assert inside.packed.dtype == torch.bool
    plan = rc.RayCastPlan(tf, tv, validate=False)
    eager = rc.cast_rays(to, td, tv, plan, cull=True, reorder=True)
    assert torch.equal(packed.t.packed[:500, 0], eager.t) and torch.equal(packed.crossings.packed[:500, 0], eager.crossings)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        hits = rc.cast_rays(to, td, tv, plan, cull=True, reorder=True)
    g.replay()
    torch.cuda.synchronize()
    want = rr.cast(o, d, v, f[:-3])
    for got in (eager, hits):
        assert np.array_equal(got.t.cpu().numpy().view(np.uint32), want[0].view(np.uint32))
        assert np.array_equal(got.crossings.cpu().numpy(), want[3]) and np.array_equal(got.face.cpu().numpy(), want[1])
    to.copy_(_dev(o[::-1].copy()))
    td.copy_(_dev(d[::-1].copy()))
    g.replay()
    torch.cuda.synchronize()
    assert np.array_equal(hits.t.cpu().numpy().view(np.uint32), want[0][::-1].view(np.uint32))
    assert np.array_equal(hits.crossings.cpu().numpy(), want[3][::-1])
