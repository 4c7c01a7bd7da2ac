"""nsdp_mesh_closest and what is built on it against the fp64 yardstick of tests/surface_ref.py.

The envelope (include/nsdp_surface.h): |dist2 - exact| <= E * 2^-24 * R2 to first order, E = 17, R2 the largest
squared distance from the query to the face's corners; the tests allow E + 1 (one unit for second order) and leave no query
out.  Two faces are involved where fp32 cannot separate them: the kernel's dist2 lies above the exact minimum by at most the
envelope of the fp64 winner and below it by at most the envelope of its own face, so the unit is the larger of the two R2.

Worst observed shares of E + 1 are printed by the envelope test (pytest -s) and recorded in DESIGN.md 4k."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import surface_ref
from surface_ref import E, U

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
FLT_MAX = float(np.finfo(np.float32).max)
_ci, _vp = ctypes.c_int, ctypes.c_void_p


def _t(x, dtype=None):
    return torch.as_tensor(np.ascontiguousarray(x), dtype=dtype).to(DEV)


def _raw(q, qoff, v, voff, f, foff, cull, bary=True, fill=-7.0, bound=True):
    """nsdp_mesh_closest on packed CPU operands, outputs prefilled with `fill` so that rows the call leaves alone show."""
    from nsdp_amd import _lib
    L = _lib.lib()
    tq, tv, tf = _t(q, torch.float32).reshape(-1, 3), _t(v, torch.float32).reshape(-1, 3), _t(f, torch.int32).reshape(-1, 3)
    tqo, tvo, tfo = _t(qoff, torch.int32), _t(voff, torch.int32), _t(foff, torch.int32)
    B, qcap, vcap, fcap = tqo.numel() - 1, tq.shape[0], tv.shape[0], tf.shape[0]
    L.nsdp_mesh_closest_workspace_bytes.restype = ctypes.c_size_t
    need = int(L.nsdp_mesh_closest_workspace_bytes(_ci(B), _ci(qcap), _ci(fcap)))
    assert need == 8 * qcap + 24 * (fcap // 64 + B + 1)
    ws = torch.full((need // 4,), float("nan"), device=DEV)
    d2 = torch.full((qcap,), fill, device=DEV)
    face = torch.full((qcap,), int(fill), dtype=torch.int32, device=DEV)
    bo = torch.full((qcap, 3), fill, device=DEV) if bary else None
    _lib.check(L.nsdp_mesh_closest(_vp(tq.data_ptr()), _vp(tqo.data_ptr()), _vp(tv.data_ptr()), _vp(tvo.data_ptr()), _vp(tf.data_ptr()),
                                   _vp(tfo.data_ptr()), _ci(B), _ci(qcap), _ci(vcap), _ci(fcap), _ci((0 if cull else 1) | (0 if bound else 2)), _vp(ws.data_ptr()),
                                   _vp(d2.data_ptr()), _vp(face.data_ptr()), _vp(bo.data_ptr() if bary else 0), _lib.stream_ptr()),
               "nsdp_mesh_closest")
    torch.cuda.synchronize()
    return d2.cpu().numpy(), face.cpu().numpy(), (bo.cpu().numpy() if bary else None)


def _one(q, v, f, **kw):
    """closest_on_mesh on one mesh (numpy in, numpy out)."""
    from nsdp_amd import surface_distance
    d2, face, bary = surface_distance.closest_on_mesh(_t(q, torch.float32)[None], _t(v, torch.float32)[None], _t(f, torch.int64)[None], **kw)
    return d2[0].cpu().numpy(), face[0].cpu().numpy(), (None if bary is None else bary[0].cpu().numpy())


def _check(q, v, f, d2, face, bary=None, ref=None):
    """One mesh: the kernel's (d2, face, bary) against fp64 -- every query.  -> the worst share of the allowed envelope."""
    q, v = np.asarray(q, dtype=np.float32), np.asarray(v, dtype=np.float32)
    best, bface, _ = ref if ref is not None else surface_ref.brute(q, v, f)
    assert not np.isnan(d2).any() and (face >= 0).all() and (face < len(f)).all()
    unit = U * np.maximum(surface_ref.corner_r2(q, v, f, face), surface_ref.corner_r2(q, v, f, bface))
    allowed = (E + 1) * unit
    err = np.abs(d2.astype(np.float64) - best)
    assert (err <= allowed).all(), (int(np.argmax(err - allowed)), float((err / unit).max()))
    own, _ = surface_ref.to_face(q, v, f, face)          # the fp64 distance to the face the kernel chose: within the envelope
    assert (own - best <= allowed).all(), float(((own - best) / unit).max())      # of the minimum (the index is not compared)
    def worst(e):
        return float(np.divide(e, allowed, out=np.zeros_like(e), where=allowed > 0).max()) if len(e) else 0.0

    share = worst(err)
    if bary is not None:
        assert (bary >= 0).all() and not np.isnan(bary).any()
        assert (np.abs(bary.astype(np.float64).sum(-1) - 1.0) <= 4 * U).all()
        # (the weights are homogeneous: fp32 weights sum to 1 only within rounding, and (sum - 1) times a coordinate of 2000 is no
        # error of the closest point -- the point is named by the weights over their sum)
        w = bary.astype(np.float64) / bary.astype(np.float64).sum(-1, keepdims=True)
        point = (w[:, :, None] * v.astype(np.float64)[np.asarray(f)[face]]).sum(1)
        named = ((point - q.astype(np.float64)) ** 2).sum(-1)
        assert (np.abs(named - best) <= allowed).all(), float((np.abs(named - best) / unit).max())
        share = max(share, worst(np.abs(named - best)))
    return share


# ------------------------------------------------------------------------------------------------------------ one triangle
@pytest.mark.parametrize("flip", [False, True])
def test_one_triangle_every_region(flip):
    """Above and below the interior, beyond each edge and each corner, in the plane, on an edge, at a corner; both orientations."""
    a, b, c = surface_ref.TRI_A, surface_ref.TRI_B, surface_ref.TRI_C
    v = np.array([a, c, b] if flip else [a, b, c], dtype=np.float32)
    q = np.array([r[0] for r in surface_ref.REGIONS], dtype=np.float32)
    for cull in (True, False):
        d2, face, bary = _one(q, v, np.array([[0, 1, 2]]), cull=cull)
        assert (face == 0).all()
        for i, (_, want, wb) in enumerate(surface_ref.REGIONS):
            wb = (wb[0], wb[2], wb[1]) if flip else wb
            assert d2[i] == np.float32(want), (i, d2[i])                 # (small integers and halves: exact in fp32)
            assert np.abs(bary[i] - np.array(wb)).max() <= 2 * U, (i, bary[i])


@pytest.mark.parametrize("flip", [False, True])
def test_a_query_that_is_bitwise_a_corner_gets_exactly_zero(flip):
    rng = np.random.default_rng(5)
    v = (rng.standard_normal((30, 3)) * 3 + np.array([2000.0, -1500.0, 900.0])).astype(np.float32)
    f = np.stack([rng.permutation(30)[:3] for _ in range(70)])
    if flip:
        f = f[:, [0, 2, 1]]
    q = v[f.reshape(-1)]                                                  # every corner of every face
    for cull in (True, False):
        d2, face, bary = _one(q, v, f, cull=cull)
        assert (d2 == 0.0).all() and not np.signbit(d2).any()
        named = (bary[:, :, None] * v[f[face]]).sum(1)
        assert np.abs(named - q).max() <= 4 * U * 2600.0


# --------------------------------------------------------------------------------------------------- block and wave edges
@pytest.mark.parametrize("F", [1, 63, 64, 65, 129])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_block_and_wave_edges(F, n):
    """B = 3 packed: a mesh of F faces with n queries, a mesh without faces (FLT_MAX, -1, 0), a mesh whose shape has no
    queries; capacity rows beyond the last offset stay untouched."""
    rng = np.random.default_rng(1000 * F + n)
    V = max(3, F // 2 + 2)
    v0, v2 = rng.standard_normal((V, 3)).astype(np.float32), rng.standard_normal((7, 3)).astype(np.float32)
    f0, f2 = rng.integers(0, V, (F, 3)), rng.integers(0, 7, (F + 3, 3))
    q0, q1 = (rng.standard_normal((n, 3)) * 1.5).astype(np.float32), rng.standard_normal((5, 3)).astype(np.float32)
    pad = 9
    q = np.concatenate((q0, q1, np.full((pad, 3), 1e30, dtype=np.float32)))
    v = np.concatenate((v0, rng.standard_normal((4, 3)).astype(np.float32), v2, np.zeros((pad, 3), dtype=np.float32)))
    f = np.concatenate((f0, f2, np.full((pad, 3), 10 ** 6)))
    qoff, voff, foff = [0, n, n + 5, n + 5], [0, V, V + 4, V + 11], [0, F, F, 2 * F + 3]
    got = {cull: _raw(q, qoff, v, voff, f, foff, cull) for cull in (True, False)}
    for cull in (True, False):
        d2, face, bary = got[cull]
        _check(q0, v0, f0, d2[:n], face[:n], bary[:n])
        assert (d2[n:n + 5] == np.float32(FLT_MAX)).all() and (face[n:n + 5] == -1).all() and (bary[n:n + 5] == 0).all()
        assert (d2[n + 5:] == -7.0).all() and (face[n + 5:] == -7).all() and (bary[n + 5:] == -7.0).all()
    for a, b in zip(got[True], got[False]):
        assert np.array_equal(a.view(np.int32), b.view(np.int32))
    for a, b in zip(got[True], _raw(q, qoff, v, voff, f, foff, True, bound=False)):      # (culling without the bound pass)
        assert np.array_equal(a.view(np.int32), b.view(np.int32))
    d2, face, bary = _raw(q, qoff, v, voff, f, foff, True, bary=False)
    assert np.array_equal(d2.view(np.int32), got[True][0].view(np.int32)) and np.array_equal(face, got[True][1]) and bary is None


# ------------------------------------------------------------------------------------------------------------- the envelope
@functools.lru_cache(maxsize=None)
def _sphere_case(kind):
    """The 1280-face icosphere as it is, translated by (2000, -1500, 900) or scaled by 1e-3, with 640 queries inside, near, on
    and outside it, and its fp64 answers (computed once, on the fp32 values the kernel sees)."""
    v, f = surface_ref.icosphere(3)
    q = surface_ref.sphere_queries(640, 11, radii=(0.5, 0.9, 0.999, 1.0, 1.001, 1.1, 3.0, 100.0))
    q[:64] = v[:64]                                                       # (and queries that are vertices)
    if kind == "translated":
        shift = np.array([2000.0, -1500.0, 900.0])
        v, q = (v.astype(np.float64) + shift).astype(np.float32), (q.astype(np.float64) + shift).astype(np.float32)
    elif kind == "scaled":
        v, q = (v * np.float32(1e-3)).astype(np.float32), (q * np.float32(1e-3)).astype(np.float32)
    return q, v, f, surface_ref.brute(q, v, f)


@pytest.mark.parametrize("kind", ["plain", "translated", "scaled"])
def test_envelope(kind):
    q, v, f, ref = _sphere_case(kind)
    d2, face, bary = _one(q, v, f)
    share = _check(q, v, f, d2, face, bary, ref)
    print(f"\nenvelope, {kind}: worst share of (E + 1) = {share:.4f}  ({share * (E + 1):.3f} units of 2^-24 R2)")
    assert (d2[:64] == 0).all()


def test_degenerate_faces():
    """Two and three equal corners and collinear corners mixed into a mesh, and a mesh of nothing else: no NaN, and the fp64
    segment and point distances within the envelope."""
    v, f = surface_ref.icosphere(1)
    a, b = np.array([1.5, 0.2, 0.1], dtype=np.float32), np.array([2.5, 0.9, -0.4], dtype=np.float32)
    mid = ((a + b) / np.float32(2)).astype(np.float32)
    third = (a + (b - a) * np.float32(1 / 3)).astype(np.float32)          # (collinear up to its own rounding)
    lone = np.array([-2.0, -2.0, 0.5], dtype=np.float32)
    k = len(v)
    v = np.concatenate((v, np.stack((a, b, mid, third, lone))))
    extra = np.array([[k, k, k + 1], [k, k + 1, k + 1], [k + 1, k, k + 1], [k, k + 2, k + 1], [k + 3, k + 1, k], [k + 4, k + 4, k + 4],
                      [k + 2, k + 2, k + 2]])
    rng = np.random.default_rng(2)
    f = np.concatenate((f, extra))[rng.permutation(len(f) + len(extra))]
    t = rng.uniform(-0.3, 1.3, (150, 1)).astype(np.float32)
    near_segment = a + t * (b - a) + (rng.standard_normal((150, 3)) * 0.1).astype(np.float32)
    q = np.concatenate((near_segment, lone + (rng.standard_normal((50, 3)) * 0.2).astype(np.float32), surface_ref.sphere_queries(100, 4),
                        np.stack((a, b, mid, lone))))
    for cull in (True, False):
        d2, face, bary = _one(q, v, f, cull=cull)
        _check(q, v, f, d2, face, bary)
    assert (d2[-4:] == 0).all()
    # the degenerate faces alone: the closed-form fp64 distance to the segment [a, b]
    only = extra[:5]
    d2, face, bary = _one(near_segment, v, only)
    _check(near_segment, v, only, d2, face, bary)
    P = a.astype(np.float64) - near_segment.astype(np.float64)
    _, seg = surface_ref._seg(P, np.broadcast_to(b.astype(np.float64) - a.astype(np.float64), P.shape))
    r2 = np.maximum((P * P).sum(-1), ((b.astype(np.float64) - near_segment) ** 2).sum(-1))
    assert (np.abs(d2 - seg) <= (E + 1) * U * r2).all()


# ------------------------------------------------------------------------------------------------------ culling is invisible
def _cull_inputs():
    v, f = surface_ref.icosphere(3)
    rng = np.random.default_rng(8)
    q = surface_ref.sphere_queries(640, 12, radii=(0.2, 0.95, 1.0, 1.0, 1.05, 2.0, 100.0, 100.0))
    yield "icosphere", q, v, f
    yield "shuffled faces", q, v, f[rng.permutation(len(f))]
    big = np.array([[-3, -3, -3], [3, -3, -3], [0, 3, -3], [0, 0, 3]], dtype=np.float32)      # a few triangles spanning the whole box
    k = len(v)
    fb = np.concatenate((f[:700], [[k, k + 1, k + 2], [k, k + 1, k + 3]], f[700:], [[k + 1, k + 2, k + 3], [k, k + 2, k + 3]]))
    yield "big among small", np.concatenate((q, (rng.standard_normal((128, 3)) * 2).astype(np.float32))), np.concatenate((v, big)), fb
    yield "shuffled queries", q[rng.permutation(len(q))], v, f


@pytest.mark.parametrize("reorder", [False, True])
def test_culling_is_invisible(reorder):
    """The culled and the plain scan: equal dist2, face and bary bits -- what protects the bound pass and the margin.  With the
    wrapper's reordering (compared after mapping the face back) the dist2 bits still equal those of the given order; where the
    reordering changes which face wins a tie the face is checked through fp64."""
    from nsdp_amd import surface_distance
    for name, q, v, f in _cull_inputs():
        for morton in (False, True):
            if morton:      # queries in Morton order as given
                order = surface_distance._morton_order(_t(q, torch.float32), _t([0, len(q)], torch.int32)).cpu().numpy()
                q = q[order]
            on, off = _one(q, v, f, cull=True, reorder=reorder), _one(q, v, f, cull=False, reorder=reorder)
            for a, b in zip(on, off):
                assert np.array_equal(a.view(np.int32), b.view(np.int32)), (name, morton)
            assert (on[1] >= 0).all()
            for a, b in zip(on, _one(q, v, f, cull=True, reorder=reorder, bound=False)):      # (and without the bound pass)
                assert np.array_equal(a.view(np.int32), b.view(np.int32)), (name, morton)
            if reorder:
                plain = _one(q, v, f, cull=False, reorder=False)
                assert np.array_equal(on[0].view(np.int32), plain[0].view(np.int32)), (name, morton)
                moved = on[1] != plain[1]
                if moved.any():      # a tie in the computed dist2: both faces within the envelope of each other in fp64
                    mine, _ = surface_ref.to_face(q[moved], v, f, on[1][moved])
                    theirs, _ = surface_ref.to_face(q[moved], v, f, plain[1][moved])
                    unit = U * np.maximum(surface_ref.corner_r2(q[moved], v, f, on[1][moved]),
                                          surface_ref.corner_r2(q[moved], v, f, plain[1][moved]))
                    assert (np.abs(mine - theirs) <= 2 * (E + 1) * unit).all(), (name, morton)


# --------------------------------------------------------------------------------------------------- layouts and determinism
def test_layouts_and_determinism():
    """A mesh gets the same bits alone, in a rectangular batch and in a ragged one; two runs give the same bits."""
    from nsdp_amd import surface_distance
    from nsdp_amd.ragged import RaggedPoints
    v, f = surface_ref.icosphere(2)
    q = surface_ref.sphere_queries(300, 21)
    v1, q1 = (v * np.float32(1.3) + np.float32(0.2)).astype(np.float32), surface_ref.sphere_queries(300, 22)
    v2, f2 = surface_ref.icosphere(1)
    q2 = surface_ref.sphere_queries(77, 23)
    tq, tv, tf = _t(q), _t(v), _t(f)
    for reorder in (False, True):
        alone = surface_distance.closest_on_mesh(tq[None], tv[None], tf[None], reorder=reorder)
        again = surface_distance.closest_on_mesh(tq[None], tv[None], tf[None], reorder=reorder)
        rect = surface_distance.closest_on_mesh(torch.stack((_t(q1), tq)), torch.stack((_t(v1), tv)), torch.stack((tf, tf)), reorder=reorder)
        rag = surface_distance.closest_on_mesh(RaggedPoints.from_list([_t(q2), tq, _t(q1)]), RaggedPoints.from_list([_t(v2), tv, _t(v1)]),
                                               RaggedPoints.from_rows([_t(f2).int(), tf.int(), tf.int()]), reorder=reorder)
        for k in range(3):
            assert torch.equal(alone[k], again[k])
            assert torch.equal(alone[k][0], rect[k][1])
            assert torch.equal(alone[k][0].reshape(300, -1), rag[k].split()[1])
        assert alone[1].dtype == torch.int32 and int(alone[1].min()) >= 0 and int(alone[1].max()) < len(f)
        _check(q, v, f, alone[0][0].cpu().numpy(), alone[1][0].cpu().numpy(), alone[2][0].cpu().numpy())
        _check(q2, v2, f2, *(rag[k].split()[0].cpu().numpy().reshape(77, -1).squeeze(-1) if k < 2 else rag[k].split()[0].cpu().numpy()
                             for k in range(3)))
    none = surface_distance.closest_on_mesh(tq[None], tv[None], tf[None], return_bary=False)
    assert none[2] is None and torch.equal(none[0], alone[0])


# ------------------------------------------------------------------------------------------------------------------ metric
def test_scan_metrics_batch():
    """p2s against the fp64 mean within the envelope's mean plus segment_mean's one ulp; s2p equal to segment_mean of nn_dist2 on
    the same samples, bit for bit; cd_surface half their sum.  Two meshes of different sizes, scans with their own counts."""
    from nsdp_amd import eval_metric, pointnet2_utils
    from nsdp_amd.ragged import RaggedPoints
    (va, fa), (vb, fb) = surface_ref.icosphere(1), surface_ref.icosphere(2)
    vb = (vb * np.float32(0.8)).astype(np.float32)
    rng = np.random.default_rng(31)
    scans = [(surface_ref.sphere_queries(300, 32, radii=(0.97, 1.0, 1.03)) + rng.standard_normal((300, 3)).astype(np.float32) * 0.01),
             (surface_ref.sphere_queries(500, 33, radii=(0.78, 0.8, 0.82)))]
    scans = [s.astype(np.float32) for s in scans]
    pred = RaggedPoints.from_list([_t(va), _t(vb)])
    faces = RaggedPoints.from_rows([_t(fa).int(), _t(fb).int()])
    scan = RaggedPoints.from_list([_t(s) for s in scans])
    gen = torch.Generator(device=DEV).manual_seed(3)
    samples = eval_metric.sample_surface_batch(pred, faces, 400, gen)
    m = eval_metric.scan_metrics_batch(pred, faces, scan, samples=samples)
    assert set(m) == {"p2s", "s2p", "cd_surface"} and all(t.shape == (2,) and t.dtype == torch.float32 and t.is_cuda for t in m.values())
    from nsdp_amd import surface_distance
    d2 = surface_distance.closest_on_mesh(scan, pred, faces, return_bary=False)[0].split()
    fc = surface_distance.closest_on_mesh(scan, pred, faces, return_bary=False)[1].split()
    for b, (s, v, f) in enumerate(((scans[0], va, fa), (scans[1], vb, fb))):
        best, bface, _ = surface_ref.brute(s, v, f)
        got2, gface = d2[b].cpu().numpy().reshape(-1).astype(np.float64), fc[b].cpu().numpy().reshape(-1)
        env = (E + 1) * U * np.maximum(surface_ref.corner_r2(s, v, f, gface), surface_ref.corner_r2(s, v, f, bface))
        assert (np.abs(got2 - best) <= env).all()
        # |sqrt a - sqrt b| = |a - b| / (sqrt a + sqrt b); sqrtf adds half an ulp of the root; the double mean rounds once
        root = np.sqrt(got2) + np.sqrt(best)
        per_point = np.where(root > 0, env / np.where(root > 0, root, 1.0), 0.0) + U * np.sqrt(got2)
        want = np.sqrt(best).mean()
        assert abs(float(m["p2s"][b]) - want) <= per_point.mean() + 2 * U * want, (b, float(m["p2s"][b]), want)
    pts = eval_metric.sample_points(pred, faces, *samples).contiguous()
    off = torch.arange(3, device=DEV, dtype=torch.int32) * 400
    back = pointnet2_utils.nn_dist2_ragged(pts.reshape(-1, 3), off, scan.packed, scan.offsets)
    assert torch.equal(m["s2p"], pointnet2_utils.segment_mean(back, off, sqrt=True))
    assert torch.equal(m["cd_surface"], 0.5 * (m["p2s"] + m["s2p"]))
    # rectangular: the second mesh twice, each scan of 300 points -- the bits of the packed call, and nn_dist2 itself for s2p
    tv, tf, ts = torch.stack((_t(vb), _t(vb))), torch.stack((_t(fb), _t(fb))), torch.stack((_t(scans[1][:300]), _t(scans[0])))
    rsamples = (samples[0][1:].expand(2, -1).contiguous(), samples[1][1:].expand(2, -1, -1).contiguous())
    r = eval_metric.scan_metrics_batch(tv, tf, ts, samples=rsamples)
    rr = eval_metric.scan_metrics_batch(RaggedPoints.from_list([_t(vb), _t(vb)]), RaggedPoints.from_rows([_t(fb).int(), _t(fb).int()]),
                                        RaggedPoints.from_list([_t(scans[1][:300]), _t(scans[0])]), samples=rsamples)
    for k in m:
        assert torch.equal(r[k], rr[k]), k
    rp = eval_metric.sample_points(tv, tf, *rsamples).contiguous()
    assert torch.equal(r["s2p"], pointnet2_utils.segment_mean(pointnet2_utils.nn_dist2(rp, ts).reshape(-1), off, sqrt=True))
    # drawn inside: the same generator state gives the same figures
    g1, g2 = torch.Generator(device=DEV).manual_seed(9), torch.Generator(device=DEV).manual_seed(9)
    one, two = (eval_metric.scan_metrics_batch(pred, faces, scan, pointcloud_size=256, generator=g) for g in (g1, g2))
    assert all(torch.equal(one[k], two[k]) for k in one) and torch.equal(one["p2s"], m["p2s"])


# ----------------------------------------------------------------------------------------------------------- fitting recipe
def _closest64(p, a, b, c):
    """surface_ref.closest in torch fp64 (autograd): p [n, 1, 3] against corners [1, F, 3] -> dist2 [n, F]."""
    A, B, C = a - p, b - p, c - p
    ab, ac, bc = B - A, C - A, C - B

    def seg(P, e):
        ee, tn = (e * e).sum(-1), -(P * e).sum(-1)
        t = torch.where(ee > 0, (tn / torch.where(ee > 0, ee, torch.ones_like(ee))).clamp(0.0, 1.0), torch.zeros_like(ee))
        X = P + t[..., None] * e
        return (X * X).sum(-1)

    best = torch.minimum(torch.minimum(seg(A, ab), seg(A, ac)), seg(B, bc))
    g11, g12, g22, r1, r2 = (ab * ab).sum(-1), (ab * ac).sum(-1), (ac * ac).sum(-1), -(A * ab).sum(-1), -(A * ac).sum(-1)
    det, v, w = g11 * g22 - g12 * g12, g22 * r1 - g12 * r2, g11 * r2 - g12 * r1
    inside = (det > 1e-24 * g11 * g22) & (v > 0) & (w > 0) & (v + w < det)
    safe = torch.where(inside, det, torch.ones_like(det))
    X = A + (v / safe)[..., None] * ab + (w / safe)[..., None] * ac
    return torch.where(inside, torch.minimum((X * X).sum(-1), best), best)


GAP = 1e-3      # kept queries: the fp64 squared distance to the second-best face exceeds the best by more than this


def test_point_to_surface_loss_gradients():
    """d loss / d points and d loss / d verts against fp64 autograd of the brute-force minimum, B = 2.  The queries sit 0.05
    outside the interior of a face (every barycentric weight >= 0.2) of a convex mesh, so the best face leads the second best
    by more than GAP in fp64 -- asserted for all of them -- and the closest point is an interior one.

    Tolerance, to first order, per query with R the largest distance to the winning face's corners, l its shortest edge, M the
    largest coordinate magnitude among p and the corners, d = |p - c|: the kernel's closest point is off by at most 16 U R inside
    the face's plane (the errors of t, b1, b2: 3 U |P||e| / ee and the like, times |e|) -- each weight by 16 U R / l;
    torch's c = (b0 v0 + b1 v1) + b2 v2 adds 5 U M per component and p - c one more U d.  So with s = 2 / (B n) the scale of the mean,
      |g_p - exact| <= s (16 U R + 5 U M + U d) + 3 U |g_p|        (the square's derivative and the two mean divisions)
      |g_v[k] - exact| <= sum over the queries of vertex k of s (b_k (16 U R + 5 U M + U d) + (16 U R / l) d) + 4 U sum |terms|
    (the sum over a vertex's queries is an fp32 accumulation of a handful of terms)."""
    from nsdp_amd import surface_distance
    rng = np.random.default_rng(41)
    v, f = surface_ref.icosphere(1)
    B, n = 2, 96
    verts = np.stack((v, (v * np.float32(1.2) + rng.standard_normal(v.shape).astype(np.float32) * np.float32(0.02)).astype(np.float32)))
    pts = np.empty((B, n, 3), dtype=np.float32)
    for b in range(B):
        face = rng.integers(0, len(f), n)
        w = rng.dirichlet((1, 1, 1), n) * 0.4 + 0.2
        tri = verts[b].astype(np.float64)[f[face]]
        on = (w[:, :, None] * tri).sum(1)
        normal = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
        normal /= np.linalg.norm(normal, axis=1, keepdims=True)
        normal *= np.sign((normal * on).sum(-1, keepdims=True))           # outward: beyond a convex mesh the other faces are farther
        pts[b] = (on + normal * 0.05).astype(np.float32)
    p32, v32 = _t(pts).requires_grad_(True), _t(verts).requires_grad_(True)
    faces = _t(np.stack((f, f)))
    loss, per_shape = surface_distance.point_to_surface_loss(p32, v32, faces)
    loss.backward()
    p64 = torch.tensor(pts, dtype=torch.float64, requires_grad=True)
    v64 = torch.tensor(verts, dtype=torch.float64, requires_grad=True)
    fl = torch.tensor(f)
    terms, tol_terms, s = [], [], 2.0 / (B * n)
    tol_p, tol_v = np.zeros((B, n, 3)), np.zeros((B,) + v.shape)
    for b in range(B):
        every = _closest64(p64[b][:, None, :], v64[b][fl[:, 0]][None], v64[b][fl[:, 1]][None], v64[b][fl[:, 2]][None])
        two = torch.topk(every.detach(), 2, dim=1, largest=False).values
        assert bool((two[:, 1] - two[:, 0] > GAP).all()), float((two[:, 1] - two[:, 0]).min())
        terms.append(every.min(dim=1).values.mean())
        win = every.detach().argmin(dim=1).numpy()
        d64, bary = surface_ref.to_face(pts[b], verts[b], f, win)
        assert bary.min() > 0.1                                            # (interior closest points, as constructed)
        tri = verts[b].astype(np.float64)[f[win]]
        R = np.sqrt(surface_ref.corner_r2(pts[b], verts[b], f, win))
        l = np.sqrt(np.minimum(np.minimum(((tri[:, 1] - tri[:, 0]) ** 2).sum(-1), ((tri[:, 2] - tri[:, 0]) ** 2).sum(-1)),
                               ((tri[:, 2] - tri[:, 1]) ** 2).sum(-1)))
        M = np.maximum(np.abs(tri).max(axis=(1, 2)), np.abs(pts[b]).max(axis=1))
        d = np.sqrt(d64)
        point = U * (16 * R + 5 * M + d)
        tol_p[b] = (s * point + 3 * U * s * d)[:, None]
        tol_terms.append(float((2 * d * point + 4 * U * d64).mean() + 2 * U * d64.mean()))      # (|p - c|^2 recomputed, then its mean)
        for k in range(3):
            term = s * (bary[:, k] * point + 16 * U * R / l * d) + 4 * U * s * bary[:, k] * d
            np.add.at(tol_v[b], f[win][:, k], term[:, None])
    want = torch.stack(terms).mean()
    want.backward()
    assert abs(float(loss.detach()) - float(want.detach())) <= np.mean(tol_terms) + 2 * U * float(want.detach())
    for b in range(B):
        assert abs(float(per_shape[b].detach()) - float(terms[b].detach())) <= tol_terms[b], b
    gp, gv = p32.grad.cpu().double().numpy(), v32.grad.cpu().double().numpy()
    ep, ev = np.abs(gp - p64.grad.numpy()), np.abs(gv - v64.grad.numpy())
    print(f"\nfitting recipe: worst share of the tolerance, points {float((ep / tol_p).max()):.4f}, "
          f"verts {float((ev[tol_v > 0] / tol_v[tol_v > 0]).max()):.4f}")
    assert (ep <= tol_p).all(), float((ep / tol_p).max())
    assert (ev <= tol_v).all(), float((ev[tol_v > 0] / tol_v[tol_v > 0]).max())      # (a vertex no query reaches: exactly 0 on both sides)


# ------------------------------------------------------------------------------------------------------------ label transfer
def test_label_transfer_end_to_end():
    """Two painted regions of the icosphere's vertices carried to a 500-point cloud sampled on it: every point's label equals
    that of its fp64-nearest corner of its fp64-closest face, except where fp64 itself ties at the resolution the search can
    hold: the two largest fp64 weights closer than TIE.  A point of the cloud lies on its face up to fp32 rounding, so a
    neighbouring face within the envelope may win; the closest point then moves by at most sqrt((E + 1) U) R (the envelope is
    one of squared distance) and a weight by that over the shortest edge l: TIE = 2 sqrt((E + 1) U) max(R / l)."""
    from nsdp_amd import eval_metric, surface_distance
    v, f = surface_ref.icosphere(3)
    labels = np.where(v[:, 0] > 0.3, 1, np.where(v[:, 0] < -0.3, 2, 0)).astype(np.uint8)
    tv, tf = _t(v)[None], _t(f)[None]
    gen = torch.Generator(device=DEV).manual_seed(17)
    cloud = eval_metric.sample_points(tv, tf, *eval_metric.sample_surface_batch(tv, tf, 500, gen)).contiguous()
    _, face, bary = surface_distance.closest_on_mesh(cloud, tv, tf)
    got = surface_distance.transfer_vertex_labels(_t(labels)[None], tf, face, bary)
    assert got.shape == (1, 500) and got.dtype == torch.uint8
    q = cloud[0].cpu().numpy()
    best, bface, _ = surface_ref.brute(q, v, f)
    _, b64 = surface_ref.to_face(q, v, f, bface)
    tri = v.astype(np.float64)[f]
    edges = np.sqrt(np.stack([((tri[:, i] - tri[:, j]) ** 2).sum(-1) for i, j in ((0, 1), (0, 2), (1, 2))]))
    tie = 2 * np.sqrt((E + 1) * U) * float(edges.max() / edges.min())      # (a query on the surface: R is at most the longest edge)
    top = np.sort(b64, axis=1)
    clear = top[:, 2] - top[:, 1] > tie
    want = labels[f[bface, b64.argmax(axis=1)]]
    assert clear.sum() >= 450
    assert np.array_equal(got[0].cpu().numpy()[clear], want[clear])
    assert set(got[0].cpu().tolist()) == {0, 1, 2}


# --------------------------------------------------------------------------------------------------------- the infer command
def test_infer_command_prints_scan_metrics(tmp_path):
    """python -m nsdp_amd.infer CONFIG --vertex-counts ... --metrics --scan-points N: the three figures per mesh."""
    import json
    import os
    import subprocess
    import sys
    import yaml
    from nsdp_amd.config import default_config
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cfg = default_config("forward")
    cfg["model"]["encoder_kwargs"]["npoints_per_layer"] = [256, 64, 16]
    (tmp_path / "forward.yaml").write_text(yaml.safe_dump(cfg))
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "LOCAL_WORLD_SIZE",
                                                             "MASTER_ADDR", "MASTER_PORT")}
    env["PYTHONPATH"] = root + os.pathsep + env.get("PYTHONPATH", "")
    p = subprocess.run([sys.executable, "-m", "nsdp_amd.infer", str(tmp_path / "forward.yaml"), "--surface", "256", "--steps", "1",
                        "--warmup", "1", "--reps", "1", "--vertex-counts", "300,500", "--metrics", "1000", "--scan-points", "700"],
                       capture_output=True, text=True, timeout=600, cwd=root, env=env)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, p.stdout[-2000:]
    line = json.loads(lines[0])
    assert line["scan_points"] == 700 and set(line["scan_metrics"]) == {"p2s", "s2p", "cd_surface"}
    for k, v in line["scan_metrics"].items():
        assert len(v) == 2 and all(np.isfinite(x) and x >= 0 for x in v), line["scan_metrics"]
    for b in range(2):
        assert line["scan_metrics"]["cd_surface"][b] == pytest.approx(0.5 * (line["scan_metrics"]["p2s"][b] + line["scan_metrics"]["s2p"][b]), rel=1e-6)
    assert p.stderr.count("scan metrics, mesh") == 2
