"""Editing sessions with vertex normals (nsdp_amd/edit.py, ``faces=`` and ``normals=True``): for drag, pose and track on an
EditSession and for drag and pose on a RaggedEditSession, eager and replayed, ``verts_tgt_normals`` is bit-equal to
``vertex_normals`` of the predictions the same call returns, the predictions are bit-equal to the same call without normals and
to a session opened without faces, and the second replay equals the first.  ``verts_src_normals`` carries the emulation's bits
(tests/mesh_normals_ref.py).  ``normals=True`` without faces is refused by name."""
import numpy as np
import pytest
import torch

import mesh_normals_ref as mr
from helpers import build_product, model_cfg, nondeterministic_knobs
from nsdp_amd.edit import EditSession, Motion, RaggedEditSession
from nsdp_amd.ragged import RaggedPoints

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
KEYS = ("verts_tgt_pred", "surface_samples_tgt_pred")
T0, T1 = (-0.15, -0.2, -0.2), (0.1, 0.15, -0.1)
SPHERES = ((14, 22), (16, 30), (13, 20))             # 310, 482 and 262 vertices


def _skip_variants():
    from nsdp_amd import hip_decoder, precision
    from nsdp_amd.model import deformation_networks as dn
    knobs = nondeterministic_knobs()
    if not hip_decoder.ENABLED:
        knobs.append("NSDP_FUSED_DECODER=0")      # (refused by the session)
    if precision.is_bf16():
        knobs.append("NSDP_STORAGE=bf16")         # (refused by the session)
    if not dn.ENCODE_ONCE:
        knobs.append("NSDP_ENCODE_ONCE=0")        # (refused by the session)
    if knobs:
        pytest.skip("the session does not apply under " + ", ".join(knobs))


@pytest.fixture(scope="module")
def model():
    _skip_variants()
    return build_product(model_cfg("arbitrary", [256, 64, 16]), 71, DEV)[0].eval()


def _mesh(rings, segments):
    v, f = mr.sphere(rings, segments)
    return torch.from_numpy(v).to(DEV), torch.from_numpy(f).to(DEV)


def _bits(t):
    return (t.packed if isinstance(t, RaggedPoints) else t).view(torch.int32)


def _same(a, b):
    return a is b if a is None or b is None else torch.equal(_bits(a), _bits(b))


def _open(kind, model, graph, with_faces):
    if kind == "rect":
        v, f = _mesh(*SPHERES[0])
        verts = torch.stack([v, (v * 0.9)[:, [1, 2, 0]]]).contiguous()      # (the second shape: scaled and turned, the same winding)
        return EditSession(model, verts, graph=graph, faces=f if with_faces else None), verts
    meshes = [_mesh(*rs) for rs in SPHERES]
    verts = RaggedPoints.from_list([v for v, _ in meshes])
    faces = RaggedPoints.from_rows([f for _, f in meshes])
    return RaggedEditSession(model, verts, graph=graph, faces=faces if with_faces else None), verts


def _call(session, call, translation, normals):
    if call == "drag":
        return session.drag("head", translation, normals=normals)
    if session._labels is None:
        session.set_handles(*session.labels_from_parts(["head", "tail"]))
    pose = lambda scale: [Motion.rotate((0, 0, 1), 20 * scale).then(Motion.translate(np.asarray(translation) * scale)),
                          Motion.identity(), Motion.identity()]
    if call == "pose":
        return session.pose(motions=pose(1.0), normals=normals)
    return session.track(motions=[pose((t + 1) / 3) for t in range(3)], normals=normals)


@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])
@pytest.mark.parametrize("kind,call", [("rect", "drag"), ("rect", "pose"), ("rect", "track"), ("ragged", "drag"), ("ragged", "pose")])
def test_normals_ride_along_and_change_no_prediction(model, kind, call, graph):
    from nsdp_amd.mesh_normals import vertex_normals
    with torch.no_grad():
        session, verts = _open(kind, model, graph, True)
        bare, _ = _open(kind, model, graph, False)
        assert bare.topology is None and bare.verts_src_normals is None
        assert _same(session.verts_src_normals, vertex_normals(verts, session.topology))
        for translation in (T0, T1, T0):                                    # (graph: capture, replay, replay)
            out = _call(session, call, translation, True)
            again = _call(session, call, translation, True)
            plain = _call(session, call, translation, False)
            none = _call(bare, call, translation, False)
            assert "verts_tgt_normals" not in plain and "verts_tgt_normals" not in none
            normals, pred = out["verts_tgt_normals"], out["verts_tgt_pred"]
            assert type(normals) is type(pred) and _bits(normals).shape == _bits(pred).shape
            if call == "track":
                assert tuple(normals.shape) == (3, 2, verts.shape[1], 3)
            assert _same(normals, vertex_normals(pred, session.topology)), (translation, "normals of the predictions")
            length = _bits(normals).view(torch.float32).double().pow(2).sum(dim=-1).sqrt()
            live = length[:verts.total] if kind == "ragged" else length
            assert bool(((live - 1).abs() <= 1e-6).all())
            for k in KEYS:
                assert _same(out[k], plain[k]), (translation, k, "normals=False")
                assert _same(out[k], none[k]), (translation, k, "no faces")
                assert _same(out[k], again[k]), (translation, k, "second call")
            assert _same(normals, again["verts_tgt_normals"])
        if graph:
            assert session.eager_calls == 0 and sum(1 for k in session._steps if k[-1] == "normals") == 1
        with pytest.raises(ValueError, match=r"refused: " + call + r"\(normals=True\) without faces"):
            _call(bare, call, T0, True)
        session.close()
        bare.close()
        assert session.topology is None and session.verts_src_normals is None


def test_source_normals_are_the_emulations_and_faces_per_shape(model):
    from nsdp_amd.mesh_normals import MeshNormalsError, vertex_normals
    with torch.no_grad():
        session, verts = _open("rect", model, False, True)
        v, f = mr.sphere(*SPHERES[0])
        want = mr.vertex_normals(*mr.pack([(v, f)]))["normals"]
        assert np.array_equal(session.verts_src_normals[0].cpu().numpy().view(np.uint32), want.view(np.uint32))
        tf = torch.from_numpy(f).to(DEV)
        own = EditSession(model, verts, faces=torch.stack([tf, tf]).long())      # [B, F, 3], int64
        assert _same(own.verts_src_normals, session.verts_src_normals)
        a, b = own.drag("tail", T1, normals=True), session.drag("tail", T1, normals=True)
        assert _same(a["verts_tgt_normals"], b["verts_tgt_normals"]) and _same(a["verts_tgt_pred"], b["verts_tgt_pred"])
        assert _same(a["verts_tgt_normals"], vertex_normals(a["verts_tgt_pred"], own.topology))
        bad = tf.clone()
        bad[5, 2] = verts.shape[1]
        with pytest.raises(MeshNormalsError, match="face row 5 of shape 0 names the vertices"):
            EditSession(model, verts, faces=bad)
        session.close()
        own.close()
