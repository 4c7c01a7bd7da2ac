"""GPU: nsdp_amd.evaluate with ``test.volume_iou: N`` on a tree of three identities -- a sphere pair, a sphere, and a sphere
with two faces missing (an OPEN topology) -- 9 pairs in batches of 4.  ``iou`` of every pair equals a direct call on the meshes
the same run wrote, with the batch's own draws (``evaluate.iou_generator``); the l2 / fnc / cd columns and every mesh file keep
their bytes; the batches that hold the open mesh get the WARNING line that names its pairs; without the key two runs write the
same bytes, file for file, with no ``iou`` anywhere (that the no-key path is the parent's is pinned by tests/test_evaluate_gpu.py's
values, not here).

The network has procedural weights, and what it predicts lies far from its target: every iou would be 0.  ``evaluate`` takes
the step function as an argument, so the runs here go through ``_near_target``: the network's step with ``verts_tgt_pred``
replaced by the target shrunk and shifted -- a prediction that overlaps its target, so the column holds values strictly
between 0 and 1 that differ from pair to pair."""
import json
import os

import numpy as np
import pytest
import torch

from helpers import build_product, model_cfg
from nsdp_amd import evaluate, meshio, meshstore, synth
from test_evaluate_normals_gpu import _files, _skip_variants

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
SEED, BATCH, CLOUD, N = 6, 4, 2000, 3000
SPLIT = "test_unseen_motions"


def _pair(rings, segments):
    v, f = synth.sphere_mesh(rings, segments)
    return np.concatenate([v, v * 0.8 + np.array([0.21, 0.05, 0.03])]), np.concatenate([f, f + len(v)]).astype(np.int32)


def _near_target(step):
    def test_fn(model, data_dict, config, compute_loss=False):
        loss, out = step(model, data_dict, config, compute_loss=compute_loss)
        out = dict(out)
        tgt = out["verts_tgt"]
        out["verts_tgt_pred"] = tgt.like((tgt.packed * 0.85 + torch.tensor([0.05, -0.03, 0.02], device=tgt.packed.device)).contiguous())
        return loss, out
    return test_fn


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    _skip_variants()
    from nsdp_amd.model.deformation_networks import test_on_batch_with_cano
    test_fn = _near_target(test_on_batch_with_cano)
    root = tmp_path_factory.mktemp("evaluate_iou")
    ball = synth.sphere_mesh(6, 10)
    meshes = {"duo": _pair(6, 8), "ball": synth.sphere_mesh(5, 8), "holed": (ball[0], ball[1][:-2])}
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
    for name, keys in (("plain", {}), ("again", {}), ("iou", {"volume_iou": N})):
        config = dict(cfg, test=dict(cfg["test"], **keys))
        out[name] = {"exp": str(root / name), "rows": evaluate.evaluate(model, test_fn, store, config, str(root / name), BATCH, SEED,
                                                                        log=lambda *_: None)}
    return out


def test_without_the_key_two_runs_write_the_same_bytes_and_no_iou(runs):
    a, b = _files(runs["plain"]["exp"]), _files(runs["again"]["exp"])
    assert sorted(a) == sorted(b) and len(a) > 2 + 3 * 9
    assert all(a[k] == b[k] for k in a), [k for k in a if a[k] != b[k]]
    assert b"iou" not in a[SPLIT + ".txt"] and b"iou" not in a[SPLIT + ".json"] and b"WARNING" not in a[SPLIT + ".txt"]
    for r in runs["plain"]["rows"]:
        assert sorted(r) == ["cd", "fnc", "index", "l2", "loss", "pair_info"]
    with open(os.path.join(runs["plain"]["exp"], SPLIT + ".json")) as f:
        assert sorted(json.load(f)["means"]) == ["cd", "fnc", "l2"]


def _direct(pred_path, target_path, u):
    """The IoU of two written meshes from the draws ``u`` [N, 3] of their pair."""
    (vp, f), (vt, _) = meshio.read_mesh(pred_path), meshio.read_mesh(target_path)
    return _direct_arrays(vp, vt, f, u)


def _direct_arrays(vp, vt, f, u):
    """The IoU of two poses of one mesh from the draws ``u`` [N, 3]: the operations of ``ray_cast.iou_samples``, one mesh."""
    from nsdp_amd.ray_cast import RayCastPlan, contains
    tp, tt = torch.from_numpy(vp.astype(np.float32)).to(DEV), torch.from_numpy(vt.astype(np.float32)).to(DEV)
    plan = RayCastPlan(torch.from_numpy(np.ascontiguousarray(f, np.int32)).to(DEV), tp)
    lo, hi = torch.minimum(tp.amin(dim=0), tt.amin(dim=0)), torch.maximum(tp.amax(dim=0), tt.amax(dim=0))
    pts = lo + u * (hi - lo)
    a, b = contains(pts, tp, plan), contains(pts, tt, plan)
    both, union = int((a & b).sum()), int((a | b).sum())
    return (both / union if union else 0.0), plan.open_edges


def test_iou_column_is_the_direct_call_on_the_written_meshes(runs):
    store, plain, rows = runs["store"], runs["plain"]["rows"], runs["iou"]["rows"]
    folder = os.path.join(runs["iou"]["exp"], SPLIT, "meshes")
    before, after = _files(os.path.join(runs["plain"]["exp"], SPLIT, "meshes")), _files(folder)
    assert sorted(before) == sorted(after) and all(before[k] == after[k] for k in before)      # every mesh file: the same bytes
    assert [r["index"] for r in rows] == list(range(9))
    open_pairs = []
    for r, p in zip(rows, plain):
        assert all(r[k] == p[k] for k in ("loss", "l2", "fnc", "cd")) and sorted(set(r) - set(p)) == ["iou"]
        step, b, size = r["index"] // BATCH, r["index"] % BATCH, min(BATCH, 9 - r["index"] // BATCH * BATCH)
        u = torch.rand((size, N, 3), generator=evaluate.iou_generator(DEV, SEED, step), device=DEV)[b]
        names = evaluate.export_names(store.pairs[r["index"]], "ply")
        iou, open_edges = _direct(os.path.join(folder, names["deformed"]), os.path.join(folder, names["target"]), u)
        print(r["index"], store.pairs[r["index"]][4], "iou", r["iou"], "open edges", open_edges)
        assert isinstance(r["iou"], float) and r["iou"] == iou and 0.0 < iou < 1.0
        assert (open_edges > 0) == ("holed" in str(store.pairs[r["index"]][6]))
        if open_edges:
            open_pairs.append(r["index"])
    assert len(open_pairs) == 3 and len({r["iou"] for r in rows}) >= 5      # (values of their own, not one constant)
    with open(os.path.join(runs["iou"]["exp"], SPLIT + ".json")) as f:
        saved = json.load(f)
    assert saved["pairs"] == json.loads(json.dumps(rows)) and saved["means"]["iou"] == np.mean([r["iou"] for r in rows])
    assert "iou" not in saved["left_out"]
    text = open(os.path.join(runs["iou"]["exp"], SPLIT + ".txt")).read().splitlines()
    old = open(os.path.join(runs["plain"]["exp"], SPLIT + ".txt")).read().splitlines()
    warnings = [line for line in text if line.startswith("WARNING")]
    text = [line for line in text if not line.startswith("WARNING")]
    assert len(text) == 11 and text[9] == old[9] and text[10].endswith("iou {:.6e}".format(saved["means"]["iou"]))
    for r, new, line in zip(rows, text[:9], old[:9]):
        assert new.startswith(line) and new.endswith("  iou {:.6e}".format(r["iou"]))
    # one WARNING line per batch that holds an open mesh, naming exactly its pairs
    named = []
    for line in warnings:
        assert "open edges" in line
        named += json.loads(line[line.index("["):line.index("]") + 1])
    assert named == open_pairs and 1 <= len(warnings) <= 3


def test_volume_iou_key_is_a_count_not_a_flag(runs, tmp_path):
    from nsdp_amd.model.deformation_networks import test_on_batch_with_cano
    for bad in (True, -5, 2.5, "many"):
        with pytest.raises(evaluate.EvaluateError, match="test.volume_iou"):
            evaluate.evaluate(runs["model"], test_on_batch_with_cano, runs["store"], {"test": {"volume_iou": bad}}, str(tmp_path), BATCH, SEED)


def test_batch_volume_iou_on_overlapping_meshes():
    """What evaluate calls per batch, on poses that overlap: every shape's iou is the direct single-mesh call with the batch's
    own draws, and lies strictly between 0 and 1; the open edges stay per mesh."""
    from nsdp_amd.ragged import RaggedPoints
    ball, duo = synth.sphere_mesh(6, 10), _pair(6, 8)
    meshes = [(ball[0].astype(np.float32), ball[1]), (duo[0].astype(np.float32), duo[1]), (ball[0].astype(np.float32), ball[1][:-2])]
    shift = np.float32([0.15, -0.1, 0.05])
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)      # noqa: E731
    pred = RaggedPoints.from_list([dev(v) for v, _ in meshes])
    target = RaggedPoints.from_list([dev((v * np.float32(0.9) + shift).astype(np.float32)) for v, _ in meshes])
    faces = RaggedPoints.from_rows([dev(np.ascontiguousarray(f, np.int32)) for _, f in meshes])
    got = evaluate.batch_volume_iou(faces, pred, target, N, SEED, 2)
    assert got["iou_open"].tolist() == [0.0, 0.0, 4.0] and got["iou"].dtype == torch.float64
    u = torch.rand((3, N, 3), generator=evaluate.iou_generator(DEV, SEED, 2), device=DEV)
    for b, (v, f) in enumerate(meshes):
        iou, _ = _direct_arrays(v, (v * np.float32(0.9) + shift).astype(np.float32), f, u[b])
        print(b, "iou", float(got["iou"][b]), iou)
        assert float(got["iou"][b]) == iou and 0.05 < iou < 1.0
