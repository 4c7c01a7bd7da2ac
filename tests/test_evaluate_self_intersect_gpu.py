"""GPU: nsdp_amd.evaluate with ``test.self_intersections`` on a tree of three identities -- two sphere pairs that pass through
each other (so the TARGET meshes intersect by construction: ``si_gt > 0``) and one clean sphere -- 9 pairs in batches of 4.
``si``, ``si_faces`` and ``si_gt`` of every pair equal a direct ``self_intersections`` of the meshes the same run wrote; the
l2 / fnc / cd columns and every mesh file keep their bytes; without the key the run takes the code path it took before the key
existed: the same bytes as a second run, file for file, no ``si`` anywhere, the rows' old keys alone
(tests/test_evaluate_gpu.py pins that path's values)."""
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
SEED, BATCH, CLOUD = 6, 4, 2000
SPLIT = "test_unseen_motions"


def _pair(rings, segments):
    v, f = synth.sphere_mesh(rings, segments)
    return np.concatenate([v, v * 0.8 + np.array([0.21, 0.05, 0.03])]), np.concatenate([f, f + len(v)]).astype(np.int32)


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    _skip_variants()
    from nsdp_amd.model.deformation_networks import test_on_batch_with_cano as test_fn
    root = tmp_path_factory.mktemp("evaluate_si")
    meshes = {"duo": _pair(6, 8), "ball": synth.sphere_mesh(5, 8), "twin": _pair(7, 10)}
    tree = synth.write_mesh_dataset_tree(str(root / "tree"), meshes, ["walk", "jump", "turn"], 3, seed=9)
    cfg = model_cfg("forward", [256, 64, 16])
    cfg["data"] = dict(tree)
    cfg["test"] = {"iden_split": "identity_seen", "motion_split": SPLIT, "num_sampled_pairs": -1, "batch_size": BATCH,
                   "generate_mesh": True, "generate_pointcloud": False, "mesh_folder": "meshes", "mesh_format": "ply",
                   "pointcloud_size": CLOUD}
    model, _, _ = build_product(cfg, 72, DEV)
    model.eval()
    store = meshstore.MeshStore(cfg, "identity_seen", SPLIT, device=DEV)
    out = {"store": store}
    for name, keys in (("plain", {}), ("again", {}), ("si", {"self_intersections": True})):
        config = dict(cfg, test=dict(cfg["test"], **keys))
        out[name] = {"exp": str(root / name), "rows": evaluate.evaluate(model, test_fn, store, config, str(root / name), BATCH, SEED,
                                                                        log=lambda *_: None)}
    return out


def test_without_the_key_every_file_is_the_same_bytes(runs):
    a, b = _files(runs["plain"]["exp"]), _files(runs["again"]["exp"])
    assert sorted(a) == sorted(b) and len(a) > 2 + 3 * 9
    assert all(a[k] == b[k] for k in a), [k for k in a if a[k] != b[k]]
    assert b" si " not in a[SPLIT + ".txt"] and b"si_gt" not in a[SPLIT + ".txt"] and b'"si' not in a[SPLIT + ".json"]
    for r in runs["plain"]["rows"]:
        assert sorted(r) == ["cd", "fnc", "index", "l2", "loss", "pair_info"]
    with open(os.path.join(runs["plain"]["exp"], SPLIT + ".json")) as f:
        assert sorted(json.load(f)["means"]) == ["cd", "fnc", "l2"]


def _direct(path):
    from nsdp_amd.self_intersect import SelfIntersectionPlan, self_intersections
    v, f = meshio.read_mesh(path)
    tv, tf = torch.from_numpy(v.astype(np.float32)).to(DEV), torch.from_numpy(np.ascontiguousarray(f, np.int32)).to(DEV)
    r = self_intersections(tv, SelfIntersectionPlan(tf, tv))
    assert int(r.skipped) == 0
    return int(r.pairs), int(r.faces_hit) / len(f)


def test_si_columns_are_the_direct_call_on_the_written_meshes(runs):
    store, plain, rows = runs["store"], runs["plain"]["rows"], runs["si"]["rows"]
    folder = os.path.join(runs["si"]["exp"], SPLIT, "meshes")
    before, after = _files(os.path.join(runs["plain"]["exp"], SPLIT, "meshes")), _files(folder)
    assert sorted(before) == sorted(after) and all(before[k] == after[k] for k in before)      # every mesh file: the same bytes
    assert [r["index"] for r in rows] == list(range(9))
    for r, p in zip(rows, plain):
        assert all(r[k] == p[k] for k in ("loss", "l2", "fnc", "cd")) and sorted(set(r) - set(p)) == ["si", "si_faces", "si_gt"]
        names = evaluate.export_names(store.pairs[r["index"]], "ply")
        si, share = _direct(os.path.join(folder, names["deformed"]))
        si_gt, _ = _direct(os.path.join(folder, names["target"]))
        print(r["index"], store.pairs[r["index"]][4], "si", r["si"], "si_faces", r["si_faces"], "si_gt", r["si_gt"])
        assert isinstance(r["si"], int) and isinstance(r["si_gt"], int)
        assert (r["si"], r["si_gt"]) == (si, si_gt) and r["si_faces"] == share and 0.0 <= share <= 1.0
        assert (si_gt > 0) == ("ball" not in str(store.pairs[r["index"]][6]))                     # the pairs intersect, the sphere does not
    assert sum(r["si_gt"] > 0 for r in rows) >= 3
    with open(os.path.join(runs["si"]["exp"], SPLIT + ".json")) as f:
        saved = json.load(f)
    assert saved["pairs"] == json.loads(json.dumps(rows)) and all(k in saved["means"] for k in ("si", "si_faces", "si_gt"))
    assert saved["means"]["si_gt"] == np.mean([r["si_gt"] for r in rows]) and "si" not in saved["left_out"]
    text = open(os.path.join(runs["si"]["exp"], SPLIT + ".txt")).read().splitlines()
    old = open(os.path.join(runs["plain"]["exp"], SPLIT + ".txt")).read().splitlines()
    assert len(text) == 11 and text[9] == old[9] and " si_gt " in text[10]                        # the old closing line, then the si means
    for r, new, line in zip(rows, text[:9], old[:9]):
        assert new.startswith(line) and new.endswith("si {:d}  si_faces {:.6e}  si_gt {:d}".format(r["si"], r["si_faces"], r["si_gt"]))
