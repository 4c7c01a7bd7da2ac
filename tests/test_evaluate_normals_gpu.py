"""GPU: nsdp_amd.evaluate with ``test.export_normals`` and ``test.vertex_normal_consistency`` on the three-topology tree of
tests/test_evaluate_gpu.py (4, 18 and 121 vertices, 9 pairs, batches of 4).  Without the keys two runs of the same command write
the same bytes, file for file (tests/test_evaluate_gpu.py pins those values); with them the l2 / fnc / cd columns keep their
values, the written source, deformed and target meshes carry the normals ``vertex_normals`` gives their own vertices, and ``vnc``
is the composition's: the fp32 dots of those normals, their mean taken in double by torch -- to 1e-12 -- and lies in [0, 1].
The user-handle loop (``tosca``) writes its source, deformed and target meshes with normals the same way.

With the prediction replaced by the target every dot is |n|^2: |n| is within 1e-6 of 1 (the bound of
tests/test_mesh_normals_cpu.py), so |n|^2 within 2e-6 + 1e-12, and the fp32 dot adds three roundings, under 4 * 2^-24 relative:
|vnc - 1| <= 2.3e-6 for every pair whose vertices all have a normal.  The grid of the fixture carries one vertex that no
face names (vertex 120 of 121): it has no normal, its dot is 0, and the grid's pairs are held to 120 / 121 within the same
relative bound -- a vertex without a normal counts as a miss, it is not left out of the mean."""
import json
import os

import numpy as np
import pytest
import torch

import mesh_sample_ref as ms
from helpers import build_product, model_cfg, nondeterministic_knobs
from nsdp_amd import evaluate, meshio, meshstore, synth

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
SEED, BATCH, CLOUD = 6, 4, 2000
SPLIT = "test_unseen_motions"


def _skip_variants():
    from nsdp_amd import hip_decoder, precision
    from nsdp_amd.model import deformation_networks as dn
    knobs = nondeterministic_knobs()
    if not hip_decoder.ENABLED:
        knobs.append("NSDP_FUSED_DECODER=0")      # (the layered decoder has no ragged form)
    if precision.is_bf16():
        knobs.append("NSDP_STORAGE=bf16")
    if not dn.ENCODE_ONCE:
        knobs.append("NSDP_ENCODE_ONCE=0")
    if knobs:
        pytest.skip("packed whole-mesh evaluation does not apply under " + ", ".join(knobs))


def _files(root):
    out = {}
    for d, _, names in os.walk(root):
        for n in names:
            with open(os.path.join(d, n), "rb") as f:
                out[os.path.relpath(os.path.join(d, n), root)] = f.read()
    return out


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """The split evaluated four times: twice as today, once with both keys, once with the target in place of the prediction."""
    _skip_variants()
    from nsdp_amd.model.deformation_networks import test_on_batch_with_cano as test_fn
    root = tmp_path_factory.mktemp("evaluate_normals")
    meshes = {"tet": ms.tetrahedron(), "oct": ms.octahedron(), "grid": ms.grid()}
    tree = synth.write_mesh_dataset_tree(str(root / "tree"), meshes, ["walk", "jump", "turn"], 3, seed=9)
    cfg = model_cfg("forward", [256, 64, 16])
    cfg["data"] = dict(tree)
    cfg["test"] = {"iden_split": "identity_seen", "motion_split": SPLIT, "num_sampled_pairs": -1, "batch_size": BATCH,
                   "generate_mesh": True, "generate_pointcloud": False, "mesh_folder": "meshes", "mesh_format": "ply",
                   "pointcloud_size": CLOUD}
    model, _, _ = build_product(cfg, 72, DEV)
    model.eval()
    store = meshstore.MeshStore(cfg, "identity_seen", SPLIT, device=DEV)

    def target_for_prediction(model, data_dict, config, compute_loss=False):
        loss, out = test_fn(model, data_dict, config, compute_loss=compute_loss)
        out["verts_tgt_pred"] = out["verts_tgt"].like(out["verts_tgt"].packed.clone())
        return loss, out

    out = {"store": store}
    for name, keys, fn in (("plain", {}, test_fn), ("again", {}, test_fn),
                           ("normals", {"export_normals": True, "vertex_normal_consistency": True}, test_fn),
                           ("target", {"vertex_normal_consistency": True, "generate_mesh": False}, target_for_prediction)):
        config = dict(cfg, test=dict(cfg["test"], **keys))
        out[name] = {"exp": str(root / name), "rows": evaluate.evaluate(model, fn, store, config, str(root / name), BATCH, SEED,
                                                                        log=lambda *_: None)}
    return out


def test_without_the_keys_every_file_is_the_same_bytes(runs):
    a, b = _files(runs["plain"]["exp"]), _files(runs["again"]["exp"])
    assert sorted(a) == sorted(b) and len(a) > 2 + 3 * 9                                 # the .txt, the .json; deformed, target and handle per pair, shared sources
    assert all(a[k] == b[k] for k in a), [k for k in a if a[k] != b[k]]
    assert b"vnc" not in a[SPLIT + ".txt"] and b"vnc" not in a[SPLIT + ".json"]
    assert not any(b"property float nx" in v[:400] for k, v in a.items() if k.endswith(".ply"))
    for r in runs["plain"]["rows"]:
        assert sorted(r) == ["cd", "fnc", "index", "l2", "loss", "pair_info"]


def _ply(path):
    """(verts fp32 (V, 3), normals fp32 (V, 3) or None) of a binary .ply as write_mesh writes it."""
    raw = open(path, "rb").read()
    head, body = raw.split(b"end_header\n", 1)
    n = int(head.split(b"element vertex ")[1].split()[0])
    props = [l.split()[1:] for l in head.decode().split("\n") if l.startswith("property ") and " list " not in l]
    dt = np.dtype([(name, {"float": "<f4", "uchar": "u1"}[kind]) for kind, name in props])
    rec = np.frombuffer(body[:dt.itemsize * n], dtype=dt)
    xyz = np.stack([rec[a] for a in "xyz"], axis=1)
    return xyz, (np.stack([rec[a] for a in ("nx", "ny", "nz")], axis=1) if "nx" in dt.names else None), [name for _, name in props]


def _device_normals(verts, faces):
    from nsdp_amd.mesh_normals import MeshTopology, vertex_normals
    tv = torch.from_numpy(np.ascontiguousarray(verts)).to(DEV)
    return vertex_normals(tv, MeshTopology(torch.from_numpy(np.ascontiguousarray(faces)).to(DEV), tv))


def test_exported_normals_are_those_of_the_written_vertices_and_vnc_is_the_composition(runs):
    store = runs["store"]
    plain, rows = runs["plain"]["rows"], runs["normals"]["rows"]
    folder = os.path.join(runs["normals"]["exp"], SPLIT, "meshes")
    before = _files(os.path.join(runs["plain"]["exp"], SPLIT, "meshes"))
    assert [r["index"] for r in rows] == list(range(9))
    for r, p in zip(rows, plain):
        assert all(r[k] == p[k] for k in ("loss", "l2", "fnc", "cd")) and sorted(set(r) - set(p)) == ["vnc"]      # the old columns keep their values
        names = evaluate.export_names(store.pairs[r["index"]], "ply")
        got = {}
        for part in ("source", "deformed", "target"):
            v, f = meshio.read_mesh(os.path.join(folder, names[part]))
            xyz, normals, props = _ply(os.path.join(folder, names[part]))
            assert props[:6] == ["x", "y", "z", "nx", "ny", "nz"] and np.array_equal(xyz.astype(np.float64), v)
            v0, f0 = meshio.read_mesh(os.path.join(runs["plain"]["exp"], SPLIT, "meshes", names[part]))
            assert np.array_equal(v, v0) and np.array_equal(f, f0)                       # the same mesh as without the key
            got[part] = _device_normals(xyz, f)
            assert np.array_equal(got[part].cpu().numpy().view(np.uint32), normals.view(np.uint32)), (r["index"], part)
        for part in ("canonical", "handle"):                                            # written as before
            assert open(os.path.join(folder, names[part]), "rb").read() == before[names[part]]
        a, b = got["deformed"], got["target"]
        dots = ((a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2]).abs()
        want = float(dots.double().mean())
        print(r["index"], "vnc", r["vnc"], "composition", want, "difference", r["vnc"] - want)
        assert 0.0 <= r["vnc"] <= 1.0 and abs(r["vnc"] - want) <= 1e-12, (r["index"], r["vnc"], want)
    with open(os.path.join(runs["normals"]["exp"], SPLIT + ".json")) as f:
        saved = json.load(f)
    assert saved["pairs"] == json.loads(json.dumps(rows)) and "vnc" in saved["means"] and "vnc" in saved["left_out"]
    text = open(os.path.join(runs["normals"]["exp"], SPLIT + ".txt")).read().splitlines()
    assert len(text) == 10 and all("vnc {:.6e}".format(r["vnc"]) in line for r, line in zip(rows, text)) and " vnc " in text[-1]
    old = open(os.path.join(runs["plain"]["exp"], SPLIT + ".txt")).read().splitlines()
    assert all(new.startswith(line) for new, line in zip(text[:9], old[:9]))            # the pair lines: the old text, then vnc


def test_vnc_of_the_target_against_itself_is_one(runs):
    rows = runs["target"]["rows"]
    assert len(rows) == 9 and not os.path.isdir(os.path.join(runs["target"]["exp"], SPLIT))
    store, whole = runs["store"], 0
    for r in rows:
        verts, faces = store.mesh(int(store.pair_frames[r["index"], 2]))
        named = np.unique(faces.cpu().numpy())
        have = len(named) / verts.shape[0]                                             # the vertices some face names
        whole += have == 1.0
        print(r["index"], "vertices with a face", have, "vnc - that", r["vnc"] - have)
        assert abs(r["vnc"] - have) <= 2.3e-6 * have and r["l2"] == 0.0, (r["index"], r["vnc"], have)
    assert whole >= 6                                                                  # the tetrahedron's and the octahedron's pairs: exactly 1


def test_user_handle_export_carries_normals(tmp_path):
    _skip_variants()
    meshes = {"a": synth.sphere_mesh(15, 20), "b": synth.sphere_mesh(16, 16)}      # 302 and 258 vertices
    cfg = model_cfg("arbitrary", [256, 64, 16])
    cfg["data"] = synth.write_handle_mesh_tree(str(tmp_path / "tree"), meshes, data_type="tosca")
    cfg["test"] = {"iden_split": None, "motion_split": "test", "num_sampled_pairs": -1, "generate_mesh": True,
                   "generate_pointcloud": False, "mesh_folder": "meshes", "mesh_format": "ply"}
    model, _, _ = build_product(cfg, 71, DEV)
    model.eval()
    store = meshstore.HandleMeshStore(cfg, None, "test", device=DEV)
    for name, keys in (("plain", {}), ("normals", {"export_normals": True})):
        rows = evaluate.evaluate(model, None, store, dict(cfg, test=dict(cfg["test"], **keys)), str(tmp_path / name), 2, SEED,
                                 log=lambda *_: None)
        assert [r["index"] for r in rows] == [0, 1]
    drag = "drag_head_x-0.15y-0.20z-0.20_ratio0.10"
    before = _files(os.path.join(str(tmp_path / "plain"), drag, "meshes"))
    folder = os.path.join(str(tmp_path / "normals"), drag, "meshes")
    for info in store.pairs:
        names = evaluate.export_names(info, "ply")
        for part in ("source", "deformed", "target"):
            v, f = meshio.read_mesh(os.path.join(folder, names[part]))
            xyz, normals, props = _ply(os.path.join(folder, names[part]))
            v0, f0 = meshio.read_mesh(os.path.join(str(tmp_path / "plain"), drag, "meshes", names[part]))
            assert props[:6] == ["x", "y", "z", "nx", "ny", "nz"] and np.array_equal(v, v0) and np.array_equal(f, f0)
            assert np.array_equal(_device_normals(xyz, f).cpu().numpy().view(np.uint32), normals.view(np.uint32)), (info[1], part)
            assert (np.abs(np.sqrt((normals.astype(np.float64) ** 2).sum(axis=1)) - 1) <= 1e-6).all()
        assert open(os.path.join(folder, names["handle"]), "rb").read() == before[names["handle"]]
