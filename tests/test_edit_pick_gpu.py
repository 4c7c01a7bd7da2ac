"""Editing sessions' ``pick`` (nsdp_amd/edit.py, ``faces=``): a click as a ray against the source mesh and against a drag's
prediction, on an EditSession and a RaggedEditSession, eager and with captured drags -- ``t``, ``face``, ``bary`` are the numpy
emulation's bytes (tests/ray_cast_ref.py), ``vertex`` is the hit face's corner of the largest weight and ``label`` its handle
label after ``set_handles``; a drag returns the same bits before and after a pick.  Without faces the call is refused by name."""
import numpy as np
import pytest
import torch

import mesh_normals_ref as mr
import ray_cast_ref as rr
from helpers import build_product, model_cfg
from nsdp_amd.edit import EditSession, RaggedEditSession
from nsdp_amd.ragged import RaggedPoints
from test_edit_normals_gpu import _skip_variants

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
KEYS = ("verts_tgt_pred", "surface_samples_tgt_pred")
T0 = (-0.15, -0.2, -0.2)
SPHERES = ((8, 14), (9, 16), (7, 12))                # rings, segments: 114, 146 and 86 vertices
f32 = np.float32


@pytest.fixture(scope="module")
def model():
    _skip_variants()
    return build_product(model_cfg("arbitrary", [256, 64, 16]), 71, DEV)[0].eval()


def _mesh(rings, segments):
    v, f = mr.sphere(rings, segments)
    return v.astype(f32), np.ascontiguousarray(f, np.int32)


def _rays(v, f, n, seed):
    """n rays from a shell around the mesh (outside the ball that holds it), each aimed at the centroid of one of its faces --
    so it meets that face or one in front of it -- and the last two turned round: they miss."""
    rng = np.random.default_rng(seed)
    c, r = v.mean(0), np.abs(v - v.mean(0)).max()
    o = rng.normal(0, 1, (n, 3))
    o = (c + 3 * r * o / np.linalg.norm(o, axis=1, keepdims=True)).astype(f32)
    d = (v[f[rng.integers(0, len(f), n)]].mean(1).astype(f32) - o).astype(f32)
    d[-2:] = -d[-2:]
    return o, d


def _cloud(v, n, seed):
    """A separate surface cloud: n points of the mesh's vertices (with repeats), moved a little."""
    rng = np.random.default_rng(seed)
    return (v[rng.integers(0, len(v), n)] + rng.normal(0, 0.01, (n, 3))).astype(f32)


def _label(s, separate):
    """Labels from the rule: over the cloud, and with a separate cloud over the vertices too (``vert_labels``, which is what a
    pick then reports) -> the vertices' labels on the host."""
    labels, count = s.labels_from_parts(["head", "tail"])
    if not separate:
        s.set_handles(labels, count)
        return s._labels.cpu().numpy()
    vlabels, vcount = s.labels_from_parts(["head", "tail"], verts=True)
    assert vcount == count and vlabels.shape != labels.shape
    s.set_handles(labels, count, vlabels)
    assert s._vert_labelled and (s._vlabels > 0).any()
    return s._vlabels.cpu().numpy()


def _bits(t):
    t = t.packed if isinstance(t, RaggedPoints) else t
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def _expected(o, d, v, f, labels):
    t, face, bary, _, _, _ = rr.cast(o, d, v, f)
    vertex = np.where(face >= 0, f[np.maximum(face, 0), np.argmax(bary, axis=1)], -1)
    label = np.where(vertex >= 0, labels[np.maximum(vertex, 0)], 0)
    return t, face, bary, vertex, label


def _check(got, want, what):
    t, face, bary, vertex, label = [x.cpu().numpy() for x in got]
    assert np.array_equal(t.view(np.uint32), want[0].view(np.uint32)), what
    assert np.array_equal(face, want[1]) and np.array_equal(bary.view(np.uint32), want[2].view(np.uint32)), what
    assert np.array_equal(vertex, want[3]) and np.array_equal(label, want[4]), what
    assert (face[-2:] == -1).all() and (vertex[-2:] == -1).all() and (label[-2:] == 0).all() and (face[:-2] >= 0).all()


@pytest.mark.parametrize("graph,separate", [(False, False), (True, False), (True, True)])
def test_pick_on_a_rectangular_session(model, graph, separate):
    v, f = _mesh(*SPHERES[0])
    verts = np.stack([v, (v * f32(0.9))[:, [1, 2, 0]]])
    o, d = zip(*[_rays(verts[b], f, 40, 3 + b) for b in range(2)])
    to, td = torch.from_numpy(np.stack(o)).to(DEV), torch.from_numpy(np.stack(d)).to(DEV)
    with torch.no_grad():
        surface = torch.from_numpy(np.stack([_cloud(verts[b], 300, 40 + b) for b in range(2)])).to(DEV) if separate else None
        s = EditSession(model, torch.from_numpy(verts).to(DEV), surface, graph=graph, faces=torch.from_numpy(f).to(DEV))
        assert s.pick_plan is None and s.pick(to, td)["label"] is None          # (no labels yet; the plan is made by the first pick)
        labels = _label(s, separate)
        assert labels.shape == (2, len(v)) and (labels > 0).any()
        before = s.drag("head", T0)
        moved = before["verts_tgt_pred"].cpu().numpy()
        assert not np.array_equal(moved, verts)
        po, pd = zip(*[_rays(moved[b], f, 40, 5 + b) for b in range(2)])      # (the prediction is another mesh: rays of its own)
        src = s.pick(to, td)
        pred = s.pick(torch.from_numpy(np.stack(po)).to(DEV), torch.from_numpy(np.stack(pd)).to(DEV), before["verts_tgt_pred"])
        after = s.drag("head", T0)
        for k in KEYS:
            assert torch.equal(_bits(before[k]), _bits(after[k])), (k, "a pick changes no drag")
        if graph:
            assert s.eager_calls == 0 and s.replays >= 1
        for b in range(2):
            _check([src[k][b] for k in ("t", "face", "bary", "vertex", "label")], _expected(o[b], d[b], verts[b], f, labels[b]), ("source", b))
            _check([pred[k][b] for k in ("t", "face", "bary", "vertex", "label")], _expected(po[b], pd[b], moved[b], f, labels[b]), ("prediction", b))
        s.close()
        assert s.pick_plan is None
        bare = EditSession(model, torch.from_numpy(verts).to(DEV))
        with pytest.raises(ValueError, match=r"refused: pick\(\) without faces"):
            bare.pick(to, td)
        bare.close()


@pytest.mark.parametrize("separate", [False, True])
def test_pick_on_a_packed_session(model, separate):
    meshes = [_mesh(*rs) for rs in SPHERES]
    counts = (30, 70, 5)
    rays = [_rays(v, f, n, 11 + i) for i, ((v, f), n) in enumerate(zip(meshes, counts))]
    verts = RaggedPoints.from_list([torch.from_numpy(v).to(DEV) for v, _ in meshes])
    faces = RaggedPoints.from_rows([torch.from_numpy(f).to(DEV) for _, f in meshes])
    ro = RaggedPoints.from_list([torch.from_numpy(o).to(DEV) for o, _ in rays], capacity=120)
    rd = RaggedPoints.from_list([torch.from_numpy(d).to(DEV) for _, d in rays], capacity=120)
    with torch.no_grad():
        surface = RaggedPoints.from_list([torch.from_numpy(_cloud(v, 280 + 20 * i, 50 + i)).to(DEV) for i, (v, _) in enumerate(meshes)]) \
            if separate else None
        s = RaggedEditSession(model, verts, surface, faces=faces)
        labels = _label(s, separate)
        assert labels.shape == (verts.capacity,)
        before = s.drag("head", T0)
        moved = before["verts_tgt_pred"].packed.cpu().numpy()
        starts = np.cumsum([0] + [len(v) for v, _ in meshes])
        prays = [_rays(moved[starts[i]:starts[i + 1]], f, n, 21 + i) for i, ((_, f), n) in enumerate(zip(meshes, counts))]
        po = RaggedPoints.from_list([torch.from_numpy(o).to(DEV) for o, _ in prays], capacity=120)
        pd = RaggedPoints.from_list([torch.from_numpy(d).to(DEV) for _, d in prays], capacity=120)
        src, pred = s.pick(ro, rd), s.pick(po, pd, before["verts_tgt_pred"])
        after = s.drag("head", T0)
        for k in KEYS:
            assert torch.equal(_bits(before[k]), _bits(after[k])), (k, "a pick changes no drag")
        q0 = 0
        for i, (v, f) in enumerate(meshes):
            rows, vr = slice(q0, q0 + counts[i]), slice(starts[i], starts[i + 1])
            for got, (o, d), pose, what in ((src, rays[i], v, "source"), (pred, prays[i], moved[vr], "prediction")):
                part = [got[k].packed[rows] for k in ("t", "face", "bary", "vertex", "label")]
                part = [p[:, 0] if p.shape[1] == 1 else p for p in part]
                _check(part, _expected(o, d, pose, f, labels[vr]), (what, i))
            q0 += counts[i]
        s.close()
