"""GPU: nsdp_amd.evaluate, the reference's test.py loop over packed batches from the mesh store.  On the three-topology tree of
tests/test_mesh_store_gpu.py (4, 18 and 121 vertices) with the tiny forward model, the ``test_unseen_motions`` split (9 pairs) and
batch 4 -- batches of (4, 4, 4, 18), (18, 18, 121, 121) and (121) vertices -- every per-pair value equals, bit for bit, a
composition from pieces that existed before the evaluation loop: ``store.mesh`` slices packed by ``RaggedPoints.from_list``, the
same ``assemble`` batch, the step function, ``compute_evaluation_metrics_batch`` with the same surface draws.  The files hold
those values; the written meshes read back to the predictions.  With an ``arbitrary`` model on a user-handle tree the exported
meshes are ``RaggedEditSession.drag``'s."""
import json
import os

import numpy as np
import pytest
import torch

import mesh_sample_ref as mr
from helpers import build_product, model_cfg, nondeterministic_knobs
from nsdp_amd import evaluate, meshio, meshstore, synth
from nsdp_amd.eval_metric import compute_evaluation_metrics_batch
from nsdp_amd.ragged import RaggedPoints, offsets_of

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
SEED, BATCH, CLOUD = 6, 4, 2000


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


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    """One ``evaluate`` over the split, with mesh export, and everything the tests compare it with."""
    _skip_variants()
    from nsdp_amd.model.deformation_networks import test_on_batch_with_cano as test_fn
    root = tmp_path_factory.mktemp("evaluate")
    meshes = {"tet": mr.tetrahedron(), "oct": mr.octahedron(), "grid": mr.grid()}
    tree = synth.write_mesh_dataset_tree(str(root / "tree"), meshes, ["walk", "jump", "turn"], 3, seed=9)
    cfg = model_cfg("forward", [256, 64, 16])
    cfg["data"] = dict(tree)
    cfg["test"] = {"iden_split": "identity_seen", "motion_split": "test_unseen_motions", "num_sampled_pairs": -1, "batch_size": BATCH,
                   "generate_mesh": True, "generate_pointcloud": False, "mesh_folder": "meshes", "mesh_format": "ply",
                   "pointcloud_size": CLOUD}
    model, _, _ = build_product(cfg, 72, DEV)
    model.eval()
    store = meshstore.MeshStore(cfg, "identity_seen", "test_unseen_motions", device=DEV)
    exp, lines = str(root / "run"), []
    rows = evaluate.evaluate(model, test_fn, store, cfg, exp, BATCH, SEED, log=lines.append)
    return {"cfg": cfg, "model": model, "test_fn": test_fn, "store": store, "exp": exp, "lines": lines, "rows": rows}


def _composed(run):
    """The per-pair values and predictions from the earlier pieces, batch by batch."""
    store, cfg = run["store"], run["cfg"]
    rows, preds = [], []
    for step, lo in enumerate(range(0, len(store), BATCH)):
        picks = list(range(lo, min(lo + BATCH, len(store))))
        host = np.ascontiguousarray(store.pair_frames[picks].T)
        dd = store.assemble(torch.from_numpy(host).to(DEV), SEED, 0, step)
        cano, src, tgt = ([store.mesh(int(k)) for k in host[c]] for c in range(3))
        dd["verts_src"] = RaggedPoints.from_list([v for v, _ in src])
        dd["verts_tgt"] = RaggedPoints.from_list([v for v, _ in tgt])
        fcounts = [int(f.shape[0]) for _, f in cano]
        faces = RaggedPoints(torch.cat([f for _, f in cano]), offsets_of(fcounts, DEV), fcounts)
        loss, out = run["test_fn"](run["model"], dd, cfg, compute_loss=True)
        samples = evaluate.metric_samples(out["verts_tgt_pred"], faces, CLOUD, SEED, step)
        m = compute_evaluation_metrics_batch({"verts_tgt_pred": out["verts_tgt_pred"], "verts_tgt": dd["verts_tgt"], "faces": faces},
                                             samples=samples)
        m = {k: v.tolist() for k, v in m.items()}
        rows += [{"index": p, "loss": float(loss), "l2": m["l2"][b], "fnc": m["fnc"][b], "cd": m["cd"][b]} for b, p in enumerate(picks)]
        preds += [p.cpu().numpy() for p in out["verts_tgt_pred"].split()]
    return rows, preds


def test_per_pair_values_equal_the_composition_and_the_files_hold_them(run):
    store, rows = run["store"], run["rows"]
    assert len(store) == 9 and [r["index"] for r in rows] == list(range(9))
    want, _ = _composed(run)
    for got, ref in zip(rows, want):
        for k in ("loss", "l2", "fnc", "cd"):
            print(got["index"], k, got[k], ref[k])
            assert got[k] == ref[k] and np.isfinite(got[k]), (got["index"], k, got[k], ref[k])
        assert tuple(got["pair_info"]) == store.pairs[got["index"]]
    assert len({r["loss"] for r in rows}) == 3                                           # one loss per batch
    with open(os.path.join(run["exp"], "test_unseen_motions.json")) as f:
        saved = json.load(f)
    assert saved["pairs"] == json.loads(json.dumps(rows))                                # every value, unfiltered
    means, left_out = evaluate.filtered_means(rows)
    assert saved["left_out"] == left_out and all(saved["means"][k] == means[k] or np.isnan(means[k]) for k in means)
    with open(os.path.join(run["exp"], "test_unseen_motions.txt")) as f:
        text = f.read().splitlines()
    assert text == run["lines"] and len(text) == 10 and text[-1].startswith("mean over 9 pairs")
    for r, line in zip(rows, text):
        assert line.startswith("pair {:5d} ".format(r["index"])) and all("{} {:.6e}".format(k, r[k]) in line for k in ("l2", "fnc", "cd"))
    assert "left out: " + ", ".join("{} {}".format(k, left_out[k]) for k in ("l2", "fnc", "cd")) in text[-1]


def _ply_colors(path):
    raw = open(path, "rb").read()
    head, body = raw.split(b"end_header\n", 1)
    assert b"property uchar red" in head
    n = int(head.split(b"element vertex ")[1].split()[0])
    rec = np.frombuffer(body[:15 * n], dtype=np.dtype([("p", "<f4", (3,)), ("c", "u1", (3,))]))
    return rec["c"]


def test_exported_meshes_read_back(run):
    store = run["store"]
    _, preds = _composed(run)
    folder = os.path.join(run["exp"], "test_unseen_motions", "meshes")
    with_handle_faces = 0
    for p, info in enumerate(store.pairs):
        names = {k: os.path.join(folder, v) for k, v in evaluate.export_names(info, "ply").items()}
        c, s, t = (store.mesh(int(k)) for k in store.pair_frames[p])
        faces = c[1].cpu().numpy()
        for part, verts in (("deformed", preds[p]), ("source", s[0].cpu().numpy()), ("canonical", c[0].cpu().numpy()),
                            ("target", t[0].cpu().numpy())):
            v, f = meshio.read_mesh(names[part])
            assert np.array_equal(v.astype(np.float32).view(np.uint32), verts.view(np.uint32)) and np.array_equal(f, faces), (p, part)
        assert b"property uchar red" not in open(names["deformed"], "rb").read(400)      # written uncoloured
        host = np.ascontiguousarray(store.pair_frames[[p]].T)
        h = store.whole_meshes(torch.from_numpy(host).to(DEV), host)["cano_handle_vert_idx"].reshape(-1).cpu().numpy()
        for part, colour in (("source", (255, 0, 0)), ("canonical", (255, 0, 0)), ("target", (0, 0, 255))):
            col = _ply_colors(names[part])
            assert np.array_equal(col[h], np.tile(np.array(colour, np.uint8), (int(h.sum()), 1))), (p, part)
            assert np.array_equal(col[~h], np.full((int((~h).sum()), 3), 191, np.uint8)), (p, part)
        keep = faces[h[faces].all(axis=1)]
        assert os.path.isfile(names["handle"])
        if len(keep):                                                                    # (a file without faces is not read back)
            v, f = meshio.read_mesh(names["handle"])
            assert np.array_equal(f, keep) and np.array_equal(v.astype(np.float32), t[0].cpu().numpy()), p
            with_handle_faces += len(keep) < len(faces)
    assert with_handle_faces >= 1                                                        # some, and not all, of a mesh's faces


def test_user_handle_meshes_are_the_sessions_drags(tmp_path):
    _skip_variants()
    from nsdp_amd.edit import HandleSpec, RaggedEditSession
    meshes = {"a": synth.sphere_mesh(15, 20), "b": synth.sphere_mesh(16, 16), "c": synth.sphere_mesh(20, 20)}      # 302, 258, 402 vertices
    tree = synth.write_handle_mesh_tree(str(tmp_path / "tree"), meshes, data_type="tosca")
    cfg = model_cfg("arbitrary", [256, 64, 16])
    cfg["data"] = tree
    cfg["test"] = {"iden_split": None, "motion_split": "test", "num_sampled_pairs": -1, "generate_mesh": True,
                   "generate_pointcloud": False, "mesh_folder": "meshes", "mesh_format": "ply"}
    model, _, _ = build_product(cfg, 71, DEV)
    model.eval()
    store = meshstore.HandleMeshStore(cfg, None, "test", device=DEV)
    assert [i[1] for i in store.pairs] == ["a", "b", "c"] and len(store.frames) == 3
    host = np.ascontiguousarray(store.pair_frames[[0, 1, 2]].T)
    whole = store.whole_meshes(torch.from_numpy(host).to(DEV), host)
    assert torch.equal(whole["verts_cano"].packed, whole["verts_src"].packed) and whole["verts_src"].counts == (302, 258, 402)
    rows = evaluate.evaluate(model, None, store, cfg, str(tmp_path / "run"), 2, SEED, log=lambda *_: None)
    assert [r["index"] for r in rows] == [0, 1, 2] and all(sorted(r) == ["index", "pair_info"] for r in rows)      # no metrics
    folder = os.path.join(str(tmp_path / "run"), "drag_head_x-0.15y-0.20z-0.20_ratio0.10", "meshes")
    assert sorted(os.listdir(folder)) == ["deformed", "handle", "source", "target"]
    spec = HandleSpec.from_config(cfg["data"])
    for picks in ([0, 1], [2]):
        verts = RaggedPoints.from_list([store.mesh(int(store.pair_frames[p, 1]))[0] for p in picks])
        with torch.no_grad(), RaggedEditSession(model, verts, partial_range=spec.partial_range, cliptail=spec.cliptail) as session:
            out = session.drag(spec)
        for b, p in enumerate(picks):
            names = {k: os.path.join(folder, v) for k, v in evaluate.export_names(store.pairs[p], "ply").items()}
            faces = store.mesh(int(store.pair_frames[p, 0]))[1].cpu().numpy()
            for part, want in (("deformed", out["verts_tgt_pred"]), ("target", out["verts_tgt"]), ("source", verts)):
                v, f = meshio.read_mesh(names[part])
                w = want.split()[b].cpu().numpy()
                assert np.array_equal(v.astype(np.float32).view(np.uint32), w.view(np.uint32)) and np.array_equal(f, faces), (p, part)
            h = out["cano_handle_vert_idx"].split()[b].reshape(-1).cpu().numpy()
            assert 0 < h.sum() < len(h)
            v, f = meshio.read_mesh(names["handle"])
            assert np.array_equal(f, faces[h[faces].all(axis=1)]) and 0 < len(f) < len(faces), p
            moved = out["verts_tgt"].split()[b] != verts.split()[b]
            assert moved.any() and not moved.all()                                        # the drag moved the head alone
