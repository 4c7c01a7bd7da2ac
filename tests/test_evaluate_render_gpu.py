"""GPU: nsdp_amd.evaluate with ``test.vert_pred_color`` and ``test.render: {views: K, size: S}`` on the tree of three identities
of tests/test_evaluate_iou_gpu.py, 9 pairs in batches of 4.  The deformed meshes carry colours equal to
``to_uint8(error_colors(vertex_errors(pred, tgt)))`` of the vertices the same run wrote, every other mesh file keeps its bytes;
K PNGs of S x S per pair, equal to a direct rasterise-and-shade of the written meshes under cameras fitted to the written
target; the rows gain ``dropped``; without the keys the folder listing and the metric rows are what they were.

The runs go through ``_near_target`` (the prediction is the target shrunk and shifted): errors of a few hundredths, so the
colours run through the map instead of saturating at red."""
import json
import os
import struct
import zlib

import numpy as np
import pytest
import torch

from helpers import build_product, model_cfg
from nsdp_amd import evaluate, meshio, meshstore, synth
from test_evaluate_iou_gpu import _near_target, _pair
from test_evaluate_normals_gpu import _files, _skip_variants

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
SEED, BATCH, CLOUD, VIEWS, SIZE = 6, 4, 2000, 2, 40
SPLIT = "test_unseen_motions"


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    _skip_variants()
    from nsdp_amd.model.deformation_networks import test_on_batch_with_cano
    test_fn = _near_target(test_on_batch_with_cano)
    root = tmp_path_factory.mktemp("evaluate_render")
    meshes = {"duo": _pair(6, 8), "ball": synth.sphere_mesh(5, 8), "big": synth.sphere_mesh(6, 10)}
    tree = synth.write_mesh_dataset_tree(str(root / "tree"), meshes, ["walk", "jump", "turn"], 3, seed=9)
    cfg = model_cfg("forward", [256, 64, 16])
    cfg["data"] = dict(tree)
    cfg["test"] = {"iden_split": "identity_seen", "motion_split": SPLIT, "num_sampled_pairs": -1, "batch_size": BATCH,
                   "generate_mesh": True, "generate_pointcloud": False, "mesh_folder": "meshes", "mesh_format": "ply",
                   "pointcloud_size": CLOUD}
    model, _, _ = build_product(cfg, 72, DEV)
    model.eval()
    store = meshstore.MeshStore(cfg, "identity_seen", SPLIT, device=DEV)
    out = {"store": store, "model": model}
    for name, keys in (("plain", {}), ("render", {"vert_pred_color": True, "render": {"views": VIEWS, "size": SIZE}})):
        config = dict(cfg, test=dict(cfg["test"], **keys))
        out[name] = {"exp": str(root / name), "rows": evaluate.evaluate(model, test_fn, store, config, str(root / name), BATCH, SEED,
                                                                        log=lambda *_: None)}
    return out


def _ply(path):
    """(verts fp32 (V, 3), colours uint8 (V, 3) or None) of a binary .ply as write_mesh writes it."""
    raw = open(path, "rb").read()
    head, body = raw.split(b"end_header\n", 1)
    n = int(head.split(b"element vertex ")[1].split()[0])
    props = [l.split()[1:] for l in head.decode().split("\n") if l.startswith("property ") and " list " not in l]
    dt = np.dtype([(name, {"float": "<f4", "uchar": "u1"}[kind]) for kind, name in props])
    rec = np.frombuffer(body[:dt.itemsize * n], dtype=dt)
    return np.stack([rec[a] for a in "xyz"], axis=1), (np.stack([rec[a] for a in ("red", "green", "blue")], axis=1) if "red" in dt.names else None)


def _png(path):
    raw = open(path, "rb").read()
    assert raw[:8] == b"\x89PNG\r\n\x1a\n" and raw[37:41] == b"IDAT"
    w, h, depth, colour = struct.unpack(">IIBB", raw[16:26])
    n = struct.unpack(">I", raw[33:37])[0]
    assert (depth, colour) == (8, 2)
    return np.frombuffer(zlib.decompress(raw[41:41 + n]), np.uint8).reshape(h, 1 + 3 * w)[:, 1:].reshape(h, w, 3)


def test_without_the_keys_the_listing_and_the_rows_are_what_they_were(runs):
    plain, render = _files(runs["plain"]["exp"]), _files(runs["render"]["exp"])
    assert not any(k.endswith(".png") for k in plain) and len(plain) > 2 + 3 * 9
    extra = sorted(set(render) - set(plain))
    assert sorted(set(plain) - set(render)) == [] and len(extra) == 9 * VIEWS and all(k.endswith(".png") for k in extra)
    changed = sorted(k for k in plain if plain[k] != render[k])
    assert len(changed) == 9 + 2 and all(os.sep + "deformed" + os.sep in k or k in (SPLIT + ".txt", SPLIT + ".json") for k in changed)
    assert not any(b"property uchar red" in v[:400] for k, v in plain.items() if os.sep + "deformed" + os.sep in k)
    for r, p in zip(runs["render"]["rows"], runs["plain"]["rows"]):
        assert sorted(p) == ["cd", "fnc", "index", "l2", "loss", "pair_info"] and sorted(set(r) - set(p)) == ["dropped"]
        assert all(r[k] == p[k] for k in p) and r["dropped"] == 0
    old = open(os.path.join(runs["plain"]["exp"], SPLIT + ".txt")).read().splitlines()
    new = open(os.path.join(runs["render"]["exp"], SPLIT + ".txt")).read().splitlines()
    assert len(old) == len(new) == 10 and new[9] == old[9] and all(n == o + "  dropped 0" for n, o in zip(new[:9], old[:9]))
    with open(os.path.join(runs["render"]["exp"], SPLIT + ".json")) as f:
        assert json.load(f)["pairs"] == json.loads(json.dumps(runs["render"]["rows"]))


def test_colours_and_views_are_the_direct_calls_on_the_written_meshes(runs):
    from nsdp_amd import rasterize as rz
    store, rows = runs["store"], runs["render"]["rows"]
    folder = os.path.join(runs["render"]["exp"], SPLIT, "meshes")
    colours_seen = set()
    for r in rows:
        names = evaluate.export_names(store.pairs[r["index"]], "ply")
        (vp, colours), (vt, none) = _ply(os.path.join(folder, names["deformed"])), _ply(os.path.join(folder, names["target"]))
        _, f = meshio.read_mesh(os.path.join(folder, names["deformed"]))
        tp, tt = torch.from_numpy(vp.copy()).to(DEV), torch.from_numpy(vt.copy()).to(DEV)
        want = rz.error_colors(rz.vertex_errors(tp, tt))
        assert colours is not None and colours.dtype == np.uint8 and np.array_equal(colours, rz.to_uint8(want).cpu().numpy())
        colours_seen.update(map(tuple, colours.tolist()))
        lo, hi = vt.min(axis=0), vt.max(axis=0)                             # (fp32 on both sides: the bounding box the run read back)
        cams = [rz.Camera.fit_box(lo, hi, evaluate.VIEW_DIRECTIONS[k], SIZE, SIZE) for k in range(VIEWS)]
        plan = rz.RasterPlan(torch.from_numpy(np.ascontiguousarray(f, np.int32)).to(DEV), tp)
        image = rz.shade(rz.rasterize(tp, plan, cams, SIZE, SIZE), tp, plan, colors=want).cpu().numpy()
        stem = os.path.splitext(os.path.basename(names["deformed"]))[0]
        for k in range(VIEWS):
            got = _png(os.path.join(runs["render"]["exp"], SPLIT, "renders", f"{stem}_view{k}.png"))
            assert got.shape == (SIZE, SIZE, 3) and (got != 255).any(axis=-1).sum() > SIZE * SIZE // 10
            # (the run shades inside a packed batch, this call one mesh alone: the same vertices, faces and cameras -- the
            # rasteriser's bytes do not depend on the batch; normals and colours are per-vertex functions of the mesh)
            assert np.array_equal(got, image[k]), (r["index"], k, int((got != image[k]).sum()))
    assert len(colours_seen) > 50                                           # the map is walked, not one saturated colour


def test_render_key_is_refused_by_name(runs, tmp_path):
    from nsdp_amd.model.deformation_networks import test_on_batch_with_cano
    for bad in ({"views": 0}, {"views": 7}, {"size": 5000}, {"views": True}, 3):
        with pytest.raises(evaluate.EvaluateError, match="test.render"):
            evaluate.evaluate(runs["model"], test_on_batch_with_cano, runs["store"], {"test": {"render": bad}}, str(tmp_path), BATCH, SEED)
    assert "test.vert_pred_color" in evaluate.__doc__ and "no near-plane clipping" in evaluate.__doc__
