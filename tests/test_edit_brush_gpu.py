"""Editing sessions' ``labels_from_brush`` (nsdp_amd/edit.py, ``faces=``): a click becomes a handle -- ``pick`` -> brush ->
``set_handles`` -> ``pose`` on an EditSession and a RaggedEditSession equals, bit for bit, the same pose with labels built in numpy
from the reference distances (tests/geodesic_ref.py); earlier strokes win where they overlap, a stroke whose vertex is -1 labels
nothing, a separate cloud's labels are ``transfer_vertex_labels`` of the vertex labels, a session without faces refuses by name,
and drags and poses of a session that never brushed keep their bits."""
import numpy as np
import pytest
import torch

import geodesic_ref as gr
from helpers import build_product, model_cfg
from nsdp_amd.edit import EditSession, Motion, RaggedEditSession
from nsdp_amd.ragged import RaggedPoints
from nsdp_amd.surface_distance import closest_on_mesh, transfer_vertex_labels
from test_edit_normals_gpu import _skip_variants
from test_edit_pick_gpu import KEYS, SPHERES, T0, _bits, _cloud, _mesh, _rays

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
f32 = np.float32
RADII = (0.3, 0.45, 0.2)


@pytest.fixture(scope="module")
def model():
    _skip_variants()
    return build_product(model_cfg("arbitrary", [256, 64, 16]), 71, DEV)[0].eval()


def _labels_ref(v, f, strokes):
    """strokes: (seed vertices, radius) per stroke for ONE mesh -> uint8 labels, earlier strokes winning."""
    labels = np.zeros(len(v), np.uint8)
    for i in reversed(range(len(strokes))):
        seeds, radius = strokes[i]
        seeds = [s for s in np.atleast_1d(seeds) if s >= 0]
        if seeds:
            labels[gr.geodesic(v, f, seeds, limit=radius) <= f32(radius)] = i + 1
    return labels


def _motions(count):
    return [Motion.translate((0.05, -0.1, 0.02))] + [Motion.identity()] * (count - 1)


def _posed_equal(a, b):
    for k in KEYS:
        assert torch.equal(_bits(a[k]), _bits(b[k])), k


def test_brush_on_a_rectangular_session(model):
    v, f = _mesh(*SPHERES[0])
    verts = np.stack([v, (v * f32(0.9))[:, [1, 2, 0]]])
    o, d = zip(*[_rays(verts[b], f, 4, 3 + b) for b in range(2)])                 # four rays per shape, the last two miss
    to, td = torch.from_numpy(np.stack(o)).to(DEV), torch.from_numpy(np.stack(d)).to(DEV)
    with torch.no_grad():
        tv, tf = torch.from_numpy(verts).to(DEV), torch.from_numpy(f).to(DEV)
        quiet = EditSession(model, tv, faces=tf)                                  # never brushes
        s = EditSession(model, tv, faces=tf)
        before = s.drag("head", T0)
        picked = s.pick(to, td)["vertex"]                                         # [B, 4]
        hit = picked.cpu().numpy()
        assert (hit[:, :2] >= 0).all() and (hit[:, 2:] == -1).all() and s.brush_plan is None
        radius1 = torch.tensor([RADII[1], 0.1], device=DEV)                       # per shape
        strokes = [(picked[:, 0], RADII[0]), (picked[:, :3], radius1), (picked[:, 3], 0.5)]
        labels, count = s.labels_from_brush(strokes)
        assert count == 3 and labels.dtype == torch.uint8 and tuple(labels.shape) == (2, len(v)) and s.brush_plan is not None
        want = np.stack([_labels_ref(verts[b], f, [(hit[b, 0], RADII[0]), (hit[b, :3], float(radius1[b])), (hit[b, 3], 0.5)])
                         for b in range(2)])
        assert np.array_equal(labels.cpu().numpy(), want)
        assert (want == 1).any() and (want[0] == 2).any() and not (want == 3).any()      # earlier strokes win; -1 labels nothing
        for b in range(2):
            alone = _labels_ref(verts[b], f, [(hit[b, :3], float(radius1[b]))])
            assert ((alone == 1) & (want[b] == 1)).any()                          # the overlap went to the earlier stroke
        s.set_handles(labels, count)
        posed = s.pose(_motions(count))
        other = EditSession(model, tv, faces=tf)
        other.set_handles(torch.from_numpy(want).to(DEV), 3)
        _posed_equal(posed, other.pose(_motions(3)))
        assert not torch.equal(_bits(posed[KEYS[0]]), _bits(tv))
        # measured on a posed vertex set of the same topology
        moved = before["verts_tgt_pred"]
        got, _ = s.labels_from_brush(strokes[:1], pose_verts=moved)
        mv = moved.cpu().numpy()
        assert np.array_equal(got.cpu().numpy(), np.stack([_labels_ref(mv[b], f, [(hit[b, 0], RADII[0])]) for b in range(2)]))
        # a session that never brushed gives the same drags and poses
        _posed_equal(before, s.drag("head", T0))
        _posed_equal(before, quiet.drag("head", T0))
        quiet.set_handles(labels, count)
        _posed_equal(posed, quiet.pose(_motions(count)))
        for x in (s, other, quiet):
            x.close()
        assert s.brush_plan is None
        bare = EditSession(model, tv)
        with pytest.raises(ValueError, match=r"refused: labels_from_brush\(\) without faces"):
            bare.labels_from_brush(strokes)
        bare.close()


def test_brush_with_a_separate_cloud(model):
    v, f = _mesh(*SPHERES[1])
    verts = np.stack([v, (v * f32(0.8))[:, [2, 0, 1]]])
    with torch.no_grad():
        tv, tf = torch.from_numpy(verts).to(DEV), torch.from_numpy(f).to(DEV)
        surface = torch.from_numpy(np.stack([_cloud(verts[b], 300, 40 + b) for b in range(2)])).to(DEV)
        s = EditSession(model, tv, surface, faces=tf)
        seeds = torch.tensor([[5], [60]], device=DEV)
        strokes = [(seeds, 0.35), (torch.tensor([100, 20], device=DEV), 0.3)]
        vlabels, count = s.labels_from_brush(strokes, verts=True)
        labels, count2 = s.labels_from_brush(strokes)
        assert count == count2 == 2 and tuple(vlabels.shape) == (2, len(v)) and tuple(labels.shape) == (2, 300)
        want = np.stack([_labels_ref(verts[b], f, [([5, 60][b], 0.35), ([100, 20][b], 0.3)]) for b in range(2)])
        assert np.array_equal(vlabels.cpu().numpy(), want) and (want == 1).any() and (want == 2).any()
        faces = tf[None].expand(2, -1, -1).contiguous()
        _, face, bary = closest_on_mesh(surface, tv, faces)
        assert torch.equal(labels, transfer_vertex_labels(vlabels, faces, face, bary)) and (labels > 0).any()
        s.set_handles(labels, count, vlabels)
        out = s.pose(_motions(count))
        assert out["verts_tgt_pred"].shape == tv.shape
        s.close()


def test_brush_on_a_packed_session(model):
    meshes = [_mesh(*rs) for rs in SPHERES]
    verts = RaggedPoints.from_list([torch.from_numpy(v).to(DEV) for v, _ in meshes])
    faces = RaggedPoints.from_rows([torch.from_numpy(f).to(DEV) for _, f in meshes])
    counts = (2, 1, 2)
    rays = [_rays(v, f, n + 2, 11 + i) for i, ((v, f), n) in enumerate(zip(meshes, counts))]      # (the last two of each miss)
    ro = RaggedPoints.from_list([torch.from_numpy(o).to(DEV) for o, _ in rays])
    rd = RaggedPoints.from_list([torch.from_numpy(d).to(DEV) for _, d in rays])
    with torch.no_grad():
        quiet = RaggedEditSession(model, verts, faces=faces)
        s = RaggedEditSession(model, verts, faces=faces)
        before = s.drag("head", T0)
        picked = s.pick(ro, rd)["vertex"]                                        # RaggedPoints [rays, 1] over the rays' offsets
        hits = [p[:, 0].cpu().numpy() for p in picked.split()]
        radius = torch.tensor([0.3, 0.5, 0.25], device=DEV)
        first = torch.tensor([[int(h[0])] for h in hits], device=DEV)
        strokes = [(first, 0.2), (picked, radius), (torch.full((3,), -1, device=DEV), 0.4)]
        labels, count = s.labels_from_brush(strokes)
        assert count == 3 and tuple(labels.shape) == (verts.capacity,) and labels.dtype == torch.uint8
        want = np.concatenate([_labels_ref(v, f, [(hits[i][0], 0.2), (hits[i], float(radius[i])), (-1, 0.4)])
                               for i, (v, f) in enumerate(meshes)])
        assert np.array_equal(labels.cpu().numpy(), want) and (want == 1).any() and (want == 2).any() and not (want == 3).any()
        s.set_handles(labels, count)
        posed = s.pose(_motions(count))
        other = RaggedEditSession(model, verts, faces=faces)
        other.set_handles(torch.from_numpy(want).to(DEV), 3)
        _posed_equal(posed, other.pose(_motions(3)))
        _posed_equal(before, s.drag("head", T0))
        _posed_equal(before, quiet.drag("head", T0))
        for x in (s, other, quiet):
            x.close()
        bare = RaggedEditSession(model, verts)
        with pytest.raises(ValueError, match=r"refused: labels_from_brush\(\) without faces"):
            bare.labels_from_brush(strokes)
        bare.close()


def test_brush_on_a_packed_session_with_a_separate_cloud(model):
    meshes = [_mesh(*rs) for rs in SPHERES]
    verts = RaggedPoints.from_list([torch.from_numpy(v).to(DEV) for v, _ in meshes])
    faces = RaggedPoints.from_rows([torch.from_numpy(f).to(DEV) for _, f in meshes])
    with torch.no_grad():
        clouds = [torch.from_numpy(_cloud(v, 280 + 20 * i, 50 + i)).to(DEV) for i, (v, _) in enumerate(meshes)]
        s = RaggedEditSession(model, verts, RaggedPoints.from_list(clouds), faces=faces)
        strokes = [(torch.tensor([[3], [9], [40]], device=DEV), 0.4)]
        vlabels, _ = s.labels_from_brush(strokes, verts=True)
        labels, count = s.labels_from_brush(strokes)
        assert count == 1 and tuple(labels.shape) == (sum(c.shape[0] for c in clouds),)
        q0 = v0 = 0
        for i, (v, f) in enumerate(meshes):
            tv, tf = torch.from_numpy(v).to(DEV), torch.from_numpy(f).to(DEV)
            vl = vlabels[v0:v0 + len(v)]
            assert np.array_equal(vl.cpu().numpy(), _labels_ref(v, f, [([3, 9, 40][i], 0.4)]))
            _, face, bary = closest_on_mesh(clouds[i][None], tv[None], tf[None])
            want = transfer_vertex_labels(vl, tf, face[0], bary[0])
            assert torch.equal(labels[q0:q0 + clouds[i].shape[0]], want) and (want > 0).any()
            q0, v0 = q0 + clouds[i].shape[0], v0 + len(v)
        s.set_handles(labels, count, vlabels)
        s.pose(_motions(count))
        s.close()
