"""CPU: whole meshes of a batch and the evaluation loop without a device (include/nsdp_meshwhole.h, nsdp_amd/meshstore.py,
nsdp_amd/evaluate.py).  The boundary of the header: declared there and nowhere else, exported at ABI version 24, built EXACT, bad
arguments come back as a status before anything is launched; the emulation's own truncation rule; the user-handle store's pair
rule; the export's file names and the drag's folder name; the mean filter; the point-cloud refusal."""
import ctypes
import json
import os

import numpy as np
import pytest

import mesh_whole_ref as wr
from nsdp_amd import _lib, build as nsdp_build, datastore, evaluate, meshstore, synth

ENTRY_POINTS = ["nsdp_mesh_batch_whole"]
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


# ------------------------------------------------------------------------------------------------------------------ boundary
@pytest.fixture(scope="module")
def so():
    if not os.path.exists(_lib.SO_PATH):
        nsdp_build.build()
    lib = ctypes.CDLL(_lib.SO_PATH)
    lib.nsdp_last_error.restype = ctypes.c_char_p
    return lib


def test_header_declares_and_library_exports_the_entry(so):
    assert _lib.declared_symbols("nsdp_meshwhole.h") == sorted(ENTRY_POINTS)
    for other in (None, "nsdp_batch.h", "nsdp_meshbatch.h"):
        assert not set(ENTRY_POINTS) & set(_lib.declared_symbols(other)), other
    for name in ENTRY_POINTS:
        assert hasattr(so, name), name
    assert so.nsdp_abi_version() >= 24
    assert "nsdp_meshwhole.h" in open(nsdp_build.__file__).read() and nsdp_build.PER_FILE["mesh_whole.hip"] == nsdp_build.EXACT


def test_bad_arguments_return_status_and_launch_nothing(so):
    one, odd = ctypes.c_void_p(16), ctypes.c_void_p(18)       # (non-null pointers the library must not touch: nothing may be launched)
    ll, f = ctypes.c_longlong, ctypes.c_float

    def whole(**kw):
        a = dict(verts=one, vert_rows=10, faces=one, face_rows=10, table=one, frames=2, topos=one, n_topos=1, ids=one, B=2, vcap=8,
                 fcap=8, partial_range=0.1, voff=one, foff=one, verts_out=one, handle=one, inputs=one, faces_out=one)
        a.update(kw)
        return so.nsdp_mesh_batch_whole(a["verts"], ll(a["vert_rows"]), a["faces"], ll(a["face_rows"]), a["table"], a["frames"],
                                        a["topos"], a["n_topos"], a["ids"], a["B"], a["vcap"], a["fcap"], f(a["partial_range"]),
                                        a["voff"], a["foff"], a["verts_out"], a["handle"], a["inputs"], a["faces_out"], None)

    eight, twenty = ctypes.c_void_p(24), ctypes.c_void_p(20)
    for kw, word in ((dict(B=-2), "B=-2"), (dict(B=65536), "B=65536"), (dict(vcap=0), "vcap=0"), (dict(vcap=1 << 27), "vcap=134217728"),
                     (dict(fcap=0), "fcap=0"), (dict(fcap=-3), "fcap=-3"), (dict(fcap=1 << 27), "fcap=134217728"),
                     (dict(frames=0), "n_frames=0"), (dict(n_topos=0), "n_topos=0"), (dict(vert_rows=0), "vert_rows=0"),
                     (dict(face_rows=-4), "face_rows=-4"), (dict(partial_range=float("nan")), "partial_range"),
                     (dict(partial_range=float("inf")), "partial_range"),
                     (dict(verts=None), "null"), (dict(faces=None), "null"), (dict(table=None), "null"), (dict(topos=None), "null"),
                     (dict(ids=None), "null"), (dict(voff=None), "null"), (dict(foff=None), "null"), (dict(verts_out=None), "null"),
                     (dict(handle=None), "null"), (dict(inputs=None), "null"), (dict(faces_out=None), "null"),
                     (dict(verts=odd), "16-byte"), (dict(faces=eight), "16-byte"), (dict(table=twenty), "8-byte"),
                     (dict(topos=twenty), "8-byte"), (dict(ids=odd), "4-byte"), (dict(voff=odd), "4-byte"), (dict(foff=odd), "4-byte"),
                     (dict(verts_out=odd), "4-byte"), (dict(inputs=odd), "4-byte"), (dict(faces_out=odd), "4-byte"),
                     (dict(frames=0, table=None, ids=None), "n_frames=0"),          # sizes are judged before pointers
                     (dict(partial_range=float("nan"), verts=None), "partial_range"),      # values before pointers
                     (dict(verts=odd, faces_out=None), "null")):                     # pointers before alignment
        assert whole(**kw) == -1 and word.encode() in so.nsdp_last_error() and b"mesh_batch_whole" in so.nsdp_last_error(), kw
    assert whole(B=0, table=None, ids=None, verts=None, voff=None) == 0
    assert whole(handle=ctypes.c_void_p(17), verts=None) == -1                     # (a byte output needs no alignment: the null is named)
    assert b"null" in so.nsdp_last_error()


# ------------------------------------------------------------------------------------------------------------------ emulation
def test_emulation_truncates_as_the_header_says():
    g = np.random.RandomState(0)
    verts = [g.rand(v, 3).astype(np.float32) for v in (5, 5, 3, 3)]
    faces = [g.randint(0, 5, size=(4, 3)).astype(np.int32), g.randint(0, 3, size=(2, 3)).astype(np.int32)]
    arrays = meshstore.pack(verts, [0, 0, 1, 1], faces, [])
    ids = np.array([[0, 2, 0], [1, 3, 1], [1, 3, 0]], dtype=np.int32)
    assert wr.counts(arrays, ids) == [(5, 4), (3, 2), (5, 4)]
    full = wr.whole(arrays, ids, 13, 10, 0.1)
    assert full["vert_offsets"].tolist() == [0, 5, 8, 13] and full["face_offsets"].tolist() == [0, 4, 6, 10]
    assert np.array_equal(full["verts"][0, :5], verts[0]) and np.array_equal(full["verts"][1, 5:8], verts[3])
    assert np.array_equal(full["faces"][:4], faces[0]) and np.array_equal(full["faces"][4:6], faces[1])
    assert np.array_equal(full["inputs"][:, :3], full["verts"][1]) and np.array_equal(full["inputs"][:, 6], full["handle"].astype(np.float32))
    assert np.array_equal(full["inputs"][:, 3:6], full["verts"][2] * full["handle"][:, None].astype(np.float32))
    cut = wr.whole(arrays, ids, 7, 5, 0.1)
    assert cut["vert_offsets"].tolist() == [0, 5, 7, 7] and cut["face_offsets"].tolist() == [0, 4, 5, 5]
    assert all(np.array_equal(cut[k][..., :7, :] if k == "verts" else cut[k][:7], full[k][..., :7, :] if k == "verts" else full[k][:7])
               for k in ("verts", "inputs"))
    padded = wr.whole(arrays, ids, 20, 12, 0.1)
    assert not padded["verts"][:, 13:].any() and not padded["inputs"][13:].any() and not padded["handle"][13:].any()
    assert not padded["faces"][10:].any()


# ------------------------------------------------------------------------------------------------------------------ the stores
def _handle_tree(root, kind="tosca"):
    sphere = synth.sphere_mesh(3, 4)
    return synth.write_handle_mesh_tree(str(root), {"cat0": sphere, "dog1": sphere, "wolf2": synth.sphere_mesh(2, 5)}, data_type=kind)


@pytest.mark.parametrize("kind", ["tosca", "dogrec"])
def test_handle_store_forms_one_pair_per_listed_directory(tmp_path, kind):
    data = _handle_tree(tmp_path, kind)
    with open(os.path.join(data["split_dir"], kind, "test.lst"), "a") as f:
        f.write("not_there\n")                                          # a listed name without a directory gives no pair
    store = meshstore.HandleMeshStore({"data": data}, None, "test", pairs_only=True)
    assert store.pairs == [(i, n, "0000", i, n, "0000", n, "0000") for i, n in enumerate(("cat0", "dog1", "wolf2"))]
    assert len(store) == 3 and store.sample_indices(0) == [0, 1, 2]
    assert issubclass(meshstore.HandleMeshStore, datastore.PairStore) and issubclass(meshstore.HandleMeshStore, meshstore.MeshFrames)
    assert meshstore.MeshStore not in meshstore.HandleMeshStore.__mro__
    # the kinds are learnt by this class alone: the other stores keep refusing them, and this one the flow kinds
    for other in (meshstore.MeshStore, datastore.SampleStore):
        with pytest.raises(datastore.DataStoreError, match=kind):
            other({"data": data}, None, "test", pairs_only=True)
    with pytest.raises(meshstore.MeshStoreError, match="unknown data type 'deform4d' \\(tosca and dogrec are read\\)"):
        meshstore.HandleMeshStore({"data": dict(data, type="deform4d")}, None, "test", pairs_only=True)
    with pytest.raises(_lib.NsdpHipError, match="needs a GPU"):             # everything on the host passed: only the device is missing
        meshstore.HandleMeshStore({"data": data}, None, "test", device="cpu", byte_budget=1 << 30)
    with pytest.raises(ValueError, match="neither 'tosca' nor 'dogrec'"):
        synth.write_handle_mesh_tree(str(tmp_path / "x"), {}, data_type="deform4d")
    with pytest.raises(ValueError):
        synth.write_dataset_tree(str(tmp_path / "y"), ["a"], ["m"], 1, 4, 4, data_type=kind)      # (keeps refusing these kinds)


def test_whole_meshes_needs_counts_or_capacities():
    store = meshstore.MeshStore.__new__(meshstore.MeshStore)
    with pytest.raises(meshstore.MeshStoreError, match="capacity and face_capacity must be given"):
        store.whole_meshes(np.zeros((3, 2), np.int32))
    store.frame_table_host = np.array([[0, 5 | (1 << 32), -1, 0, 0, 0], [5, 3, -1, 0, 0, 0]], dtype=np.int64)
    store.topo_table_host = np.array([[0, 2], [2, 7]], dtype=np.int64)
    assert store.mesh_counts(np.array([[0, 1, 0], [1, 1, 1], [0, 0, 0]])) == ([5, 3, 5], [7, 2, 7])
    with pytest.raises(meshstore.MeshStoreError, match="13 vertices / 16 faces do not fit the capacities 12 / 16"):
        store.whole_meshes(np.zeros((3, 3), np.int32), np.array([[0, 1, 0], [1, 1, 1], [0, 0, 0]]), capacity=12, face_capacity=16)


# ------------------------------------------------------------------------------------------------------------------ evaluate
def test_export_file_names_follow_the_reference():
    info = (2, "cat_walk", "0000", 5, "cat_jump", "0003", "cat_jump", "0007")
    assert evaluate.export_names(info, "ply") == {
        "source": os.path.join("source", "cat_jump_0003.ply"), "canonical": os.path.join("canonical", "cat_walk_0000.ply"),
        "deformed": os.path.join("deformed", "cat_jump_0003_to_cat_jump_0007.ply"),
        "target": os.path.join("target", "cat_jump_0003_to_cat_jump_0007.ply"),
        "handle": os.path.join("handle", "cat_jump_0003_to_cat_jump_0007.ply")}
    assert evaluate.export_names(info, "obj")["source"].endswith("cat_jump_0003.obj")


def test_drag_folder_names_of_the_reference_configs():
    with open(os.path.join(GOLDEN, "userhandle_configs.json")) as f:
        configs = json.load(f)
    want = {"head": "drag_head_x-0.15y-0.20z-0.20_ratio0.10", "tail": "drag_tail_x-0.15y0.15z-0.15_ratio0.10",
            "frontleftfoot": "drag_frontleftfoot_x0.15y-0.20z0.20_ratio0.10",
            "behindrightfoot": "drag_behindrightfoot_x-0.15y-0.20z0.20_ratio0.10"}
    assert sorted(configs) == sorted(f"{kind}/{part}" for kind in ("dogrec", "tosca") for part in want)
    for name, data in configs.items():
        assert evaluate.drag_folder_name(data) == want[name.split("/")[1]], name
    clipped = json.loads(json.dumps(configs["tosca/tail"]))
    clipped["userhandle"]["cliptail"], clipped["partial_range"] = True, 0.25
    clipped["userhandle"]["head"] = True                                   # the first part that is set names the drag
    assert evaluate.drag_folder_name(clipped) == "drag_head_x-0.15y0.15z-0.15_ratio0.25_cliptail"


def test_means_leave_out_values_above_one_and_count_them():
    rows = [{"l2": 0.5, "fnc": 0.9, "cd": 0.25}, {"l2": 1.0, "fnc": 1.5, "cd": 2.0}, {"l2": 3.0, "fnc": 0.7, "cd": float("nan")}]
    means, left_out = evaluate.filtered_means(rows)
    assert means["l2"] == 0.75 and means["fnc"] == pytest.approx(0.8) and means["cd"] == 0.25       # 1.0 itself enters
    assert left_out == {"l2": 1, "fnc": 1, "cd": 2}
    means, left_out = evaluate.filtered_means([{"l2": 2.0, "fnc": 2.0, "cd": 2.0}])
    assert all(np.isnan(v) for v in means.values()) and left_out == {"l2": 1, "fnc": 1, "cd": 1}


def test_pointcloud_export_is_refused_by_name(tmp_path):
    config = {"test": {"generate_pointcloud": True, "generate_mesh": False}}
    with pytest.raises(evaluate.EvaluateError, match="generate_pointcloud"):
        evaluate.evaluate(None, None, None, config, str(tmp_path / "run"), 1, 0)
    assert not (tmp_path / "run").exists()
    import yaml
    cfg = tmp_path / "c.yaml"
    cfg.write_text(yaml.safe_dump(dict(config, experiment={"out_dir": str(tmp_path), "name": "run"})))
    with pytest.raises(SystemExit) as e:
        evaluate.main([str(cfg)])
    assert "generate_pointcloud" in str(e.value) and not (tmp_path / "run").exists()
    evaluate.refuse_pointclouds({"test": {"generate_pointcloud": False}})
