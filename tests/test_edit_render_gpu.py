"""Editing sessions with previews (nsdp_amd/edit.py, ``faces=`` and ``render=RenderSpec(...)``): for drag, pose and track on an
EditSession and for drag and pose on a RaggedEditSession, eager and replayed over two different drags, ``tgt_depth`` /
``tgt_face_image`` / ``tgt_dropped`` are bit-equal to a direct ``rasterize`` of the vertices the same call returns and
``tgt_image`` to its ``shade``; the predictions and ``verts_tgt`` are bit-equal to the same call without ``render`` and to a
session opened without faces; the replay equals the eager session.  ``render=`` without faces is refused by name;
``session.render`` draws the source mesh; the command line writes a PNG of the requested size."""
import json
import os
import struct
import subprocess
import sys
import zlib

import numpy as np
import pytest
import torch

from nsdp_amd.edit import RenderSpec
from nsdp_amd.ragged import RaggedPoints
from test_edit_normals_gpu import T0, T1, _bits, _open, _same, model      # noqa: F401  (the sessions of the normals' tests)

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = ("verts_tgt_pred", "surface_samples_tgt_pred", "verts_tgt")
H, W = 40, 56


DIRECTIONS = ((0.4, 0.3, -1.0), (0.0, -0.2, 1.0))


def _cameras(pred, lead=()):
    """Two views of every mesh, fitted to that mesh's own vertices in ``pred`` ([B, V, 3] or a RaggedPoints: the procedural
    weights put a prediction nowhere near its source) -> float32 [B, 2, 4, 4] on the GPU, repeated over ``lead``."""
    from nsdp_amd.rasterize import Camera
    meshes = pred.split() if isinstance(pred, RaggedPoints) else list(pred)
    cams = torch.from_numpy(np.stack([[Camera.fit(m, d, W, H).matrix for d in DIRECTIONS] for m in meshes])).to(DEV)
    return cams.expand(lead + tuple(cams.shape)).contiguous()


def _call(session, call, translation, render):
    from nsdp_amd.edit import Motion
    if call == "drag":
        return session.drag("head", translation, render=render)
    if session._labels is None:
        session.set_handles(*session.labels_from_parts(["head", "tail"]))
    pose = lambda scale: [Motion.rotate((0, 0, 1), 20 * scale).then(Motion.translate(np.asarray(translation) * scale)),
                          Motion.identity(), Motion.identity()]
    if call == "pose":
        return session.pose(motions=pose(1.0), render=render)
    return session.track(motions=[pose((t + 1) / 3) for t in range(3)], render=render)


@pytest.mark.parametrize("kind,call", [("rect", "drag"), ("rect", "pose"), ("rect", "track"), ("ragged", "drag"), ("ragged", "pose")])
def test_previews_ride_along_and_change_no_prediction(model, kind, call):      # noqa: F811
    from nsdp_amd.rasterize import rasterize, shade
    with torch.no_grad():
        eager, verts = _open(kind, model, False, True)
        replay, _ = _open(kind, model, True, True)
        bare, _ = _open(kind, model, False, False)
        shapes = 3 if kind == "ragged" else 2
        lead = (3, shapes) if call == "track" else (shapes,)
        first = _call(bare, call, T0, None)["verts_tgt_pred"]
        cams = _cameras(first[0] if call == "track" else first, (3,) if call == "track" else ())
        views = {s: RenderSpec(cams, H, W, shade=True, count=(kind == "ragged")) for s in (eager, replay)}
        for translation in (T0, T1, T0):                                    # (graph: capture, replay, replay)
            out = _call(eager, call, translation, views[eager])
            again = _call(replay, call, translation, views[replay])
            plain = _call(eager, call, translation, None)
            none = _call(bare, call, translation, None)
            assert "tgt_depth" not in plain and "tgt_image" not in plain and "tgt_depth" not in none
            for k in KEYS:
                assert _same(out[k], plain[k]), (translation, k, "render=None")
                assert _same(out[k], none[k]), (translation, k, "no faces")
                assert _same(out[k], again[k]), (translation, k, "replayed")
            pred = out["verts_tgt_pred"]
            v = pred.packed if isinstance(pred, RaggedPoints) else pred
            r = rasterize(v, eager.render_plan, views[eager].tensor, H, W, count=(kind == "ragged"))
            assert tuple(out["tgt_depth"].shape) == lead + (2, H, W) and tuple(out["tgt_image"].shape) == lead + (2, H, W, 3)
            assert out["tgt_image"].dtype == torch.uint8 and tuple(out["tgt_dropped"].shape) == lead + (2,)
            assert torch.equal(_bits(out["tgt_depth"]), _bits(r.depth)) and torch.equal(out["tgt_face_image"], r.face)
            assert torch.equal(out["tgt_dropped"], r.dropped) and int(r.dropped.sum()) == 0
            assert torch.equal(out["tgt_image"], shade(r, v, eager.render_plan))
            if kind == "ragged":
                assert torch.equal(out["tgt_count_image"], r.count) and int(r.count.max()) >= 2
            covered = (out["tgt_face_image"] >= 0).flatten(-2).sum(dim=-1)
            assert int(covered.min()) >= 1 and float(covered.float().mean()) > 40      # every view of every mesh shows it
            for k in ("tgt_depth", "tgt_face_image", "tgt_dropped", "tgt_image"):
                assert torch.equal(_bits(out[k]) if out[k].dtype == torch.float32 else out[k],
                                   _bits(again[k]) if again[k].dtype == torch.float32 else again[k]), (translation, k, "replayed")
        assert replay.eager_calls == 0 and sum(1 for k in replay._steps if "render" in k) == 1
        with pytest.raises(ValueError, match=r"refused: " + call + r"\(render=\.\.\.\) without faces"):
            _call(bare, call, T0, RenderSpec(cams, H, W))
        with pytest.raises(ValueError, match="RenderSpec"):
            _call(eager, call, T0, (H, W))
        for s in (eager, replay, bare):
            s.close()
        assert eager.render_plan is None


def test_render_draws_the_source_mesh_or_given_vertices(model):      # noqa: F811
    from nsdp_amd.rasterize import Camera, rasterize
    with torch.no_grad():
        session, verts = _open("rect", model, False, True)
        views = [Camera.look_at((1.0, 0.6, -1.5), (0, 0, 0), (0, 1, 0), 35, W, H), Camera.orthographic((0, 0, 3), (0, 0, 0), (0, 1, 0), 1.2, W, H)]
        got = session.render(views, H, W)
        spec = RenderSpec(views, H, W)
        r = rasterize(verts, session.render_plan, session._render_wanted("render", spec).tensor, H, W)
        assert torch.equal(_bits(got["tgt_depth"]), _bits(r.depth)) and torch.equal(got["tgt_face_image"], r.face)
        assert tuple(got["tgt_image"].shape) == (2, 2, H, W, 3) and "tgt_count_image" not in got
        assert int((got["tgt_face_image"] >= 0).flatten(-2).sum(dim=-1).min()) > H * W // 12      # the source spheres fill the views
        moved = session.drag("head", T0)["verts_tgt_pred"]
        cams = _cameras(moved)
        other = session.render(cams, H, W, verts=moved, shade=False, count=True)
        assert "tgt_image" not in other and int((other["tgt_face_image"] >= 0).sum()) > 80
        assert torch.equal(other["tgt_count_image"], rasterize(moved, session.render_plan, cams, H, W, count=True).count)
        session.close()


def _decode(path):
    raw = open(path, "rb").read()
    assert raw[:8] == b"\x89PNG\r\n\x1a\n"
    w, h, depth, colour = struct.unpack(">IIBB", raw[16:26])
    n = struct.unpack(">I", raw[33:37])[0]
    assert raw[37:41] == b"IDAT" and (depth, colour) == (8, 2)
    rows = np.frombuffer(zlib.decompress(raw[41:41 + n]), np.uint8).reshape(h, 1 + 3 * w)
    return rows[:, 1:].reshape(h, w, 3)


def test_command_line_writes_a_png_of_the_requested_size(tmp_path, model):      # noqa: F811
    import yaml
    from helpers import model_cfg
    with open(tmp_path / "arbitrary.yaml", "w") as f:
        yaml.safe_dump(model_cfg("arbitrary", [256, 64, 16]), f)
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    png = tmp_path / "view.png"
    p = subprocess.run([sys.executable, "-m", "nsdp_amd.edit", str(tmp_path / "arbitrary.yaml"), "--vertices", "300", "--drags", "2",
                        "--warmup", "1", "--graph", "--render", str(png), "--render-size", "48"],
                       capture_output=True, text=True, timeout=600, cwd=ROOT, env=env)
    assert p.returncode == 0, p.stderr[-3000:]
    line = json.loads([l for l in p.stdout.splitlines() if l.startswith("{")][-1])
    assert line["render"] == str(png) and line["render_size"] == 48 and line["render_dropped"] == 0 and line["render_covered"] > 48 * 48 // 50
    assert line["ms_per_drag_render"] > 0 and line["graph"] is True
    image = _decode(str(png))
    assert image.shape == (48, 48, 3) and image[0, 0].tolist() == [255, 255, 255] and len(np.unique(image.reshape(-1, 3), axis=0)) > 3
