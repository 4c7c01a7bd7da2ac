"""Editing sessions with self-intersections (nsdp_amd/edit.py, ``faces=`` and ``self_intersections=True``) on small sphere-pair
meshes -- two spheres through each other, so the deformed mesh has hits: for drag and track on an EditSession and for pose on a
RaggedEditSession, eager and replayed, ``faces_tgt_hits`` / ``tgt_self_intersections`` / ``tgt_self_skipped`` equal a direct
``self_intersections`` of the predictions the same call returns, the predictions are bit-equal to the same call without the
flag, replay equals eager, and the flag has a graph of its own.  Without faces the flag is refused by name."""
import numpy as np
import pytest
import torch

import mesh_normals_ref as mr
from helpers import build_product, model_cfg
from nsdp_amd.edit import EditSession, Motion, RaggedEditSession
from nsdp_amd.ragged import RaggedPoints
from test_edit_normals_gpu import _skip_variants

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
KEYS = ("verts_tgt_pred", "surface_samples_tgt_pred")
FIELDS = ("faces_tgt_hits", "tgt_self_intersections", "tgt_self_skipped")
T0, T1 = (-0.15, -0.2, -0.2), (0.1, 0.15, -0.1)
PAIRS = ((8, 14), (9, 16), (7, 12))                  # rings, segments of each sphere of a pair: 228, 292 and 172 vertices


@pytest.fixture(scope="module")
def model():
    _skip_variants()
    return build_product(model_cfg("arbitrary", [256, 64, 16]), 71, DEV)[0].eval()


def _pair(rings, segments):
    v, f = mr.sphere(rings, segments)
    v2 = (v * np.float32(0.8) + np.float32([0.21, 0.05, 0.03])).astype(np.float32)
    verts, faces = np.concatenate([v, v2]), np.concatenate([f, f + len(v)]).astype(np.int32)
    return torch.from_numpy(verts).to(DEV), torch.from_numpy(faces).to(DEV)


def _bits(t):
    t = t.packed if isinstance(t, RaggedPoints) else t
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def _open(kind, model, graph, with_faces=True):
    if kind == "rect":
        v, f = _pair(*PAIRS[0])
        verts = torch.stack([v, (v * 0.9)[:, [1, 2, 0]]]).contiguous()
        return EditSession(model, verts, graph=graph, faces=f if with_faces else None)
    meshes = [_pair(*rs) for rs in PAIRS]
    verts, faces = RaggedPoints.from_list([v for v, _ in meshes]), RaggedPoints.from_rows([f for _, f in meshes])
    return RaggedEditSession(model, verts, graph=graph, faces=faces if with_faces else None)


def _call(session, call, translation, flag):
    kw = {"self_intersections": True} if flag else {}
    if call == "drag":
        return session.drag("head", translation, **kw)
    if session._labels is None:
        session.set_handles(*session.labels_from_parts(["head", "tail"]))
    pose = lambda scale: [Motion.rotate((0, 0, 1), 20 * scale).then(Motion.translate(np.asarray(translation) * scale)),
                          Motion.identity(), Motion.identity()]
    if call == "pose":
        return session.pose(motions=pose(1.0), **kw)
    return session.track(motions=[pose((t + 1) / 3) for t in range(3)], **kw)


@pytest.mark.parametrize("kind,call", [("rect", "drag"), ("rect", "track"), ("ragged", "pose")])
def test_self_intersections_ride_along_and_change_no_prediction(model, kind, call):
    from nsdp_amd.self_intersect import self_intersections
    with torch.no_grad():
        eager, replayed = _open(kind, model, False), _open(kind, model, True)
        assert eager.selfint_plan is None                                   # (made by the first call that asks)
        for translation in (T0, T1, T0):                                    # (graph: capture, replay, replay)
            out, plain = _call(eager, call, translation, True), _call(eager, call, translation, False)
            rep, rep_plain = _call(replayed, call, translation, True), _call(replayed, call, translation, False)
            assert not any(k in plain or k in rep_plain for k in FIELDS)
            pred = out["verts_tgt_pred"]
            direct = self_intersections(pred.packed if kind == "ragged" else pred, eager.selfint_plan)
            assert torch.equal(out["faces_tgt_hits"], direct.hits) and torch.equal(out["tgt_self_intersections"], direct.pairs)
            assert torch.equal(out["tgt_self_skipped"], direct.skipped)
            pairs = out["tgt_self_intersections"]
            assert pairs.dtype == torch.int64 and tuple(pairs.shape) == ((3, 2) if call == "track" else (2,) if kind == "rect" else (3,))
            assert bool((pairs > 0).all()) and int(out["tgt_self_skipped"].sum()) == 0
            if call == "track":
                assert tuple(out["faces_tgt_hits"].shape) == (3, 2, eager.faces.shape[0])
            for k in KEYS:
                assert torch.equal(_bits(out[k]), _bits(plain[k])), (translation, k, "the flag changes no prediction")
                assert torch.equal(_bits(rep[k]), _bits(rep_plain[k])), (translation, k, "... replayed")
            for k in FIELDS:
                assert torch.equal(rep[k], out[k]), (translation, k, "replay equals eager")
        assert replayed.eager_calls == 0 and sum(1 for k in replayed._steps if k[-1] == "self_intersections") == 1
        assert sum(1 for k in replayed._steps if k[-1] != "self_intersections") == 1
        both = _call(eager, call, T1, True) if call != "drag" else eager.drag("head", T1, normals=True, self_intersections=True)
        assert all(k in both for k in FIELDS)
        bare = _open(kind, model, False, with_faces=False)
        with pytest.raises(ValueError, match=r"refused: " + call + r"\(self_intersections=True\) without faces"):
            _call(bare, call, T0, True)
        for s in (eager, replayed, bare):
            s.close()
        assert eager.selfint_plan is None
