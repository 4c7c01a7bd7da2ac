"""CPU: the data store's host side -- pair lists and reshuffled lists against the reference's (tests/golden/dataset_tree.npz),
the numpy emulation of nsdp_subset_draw (a bijection, a function of its key, uniform within derived bounds), every refusal by
name, the trainer's flags, and the boundary of include/nsdp_batch.h: declared, exported at ABI version 22, bad arguments come
back as a status with a message and launch nothing."""
import ctypes
import os

import numpy as np
import pytest

import datastore_tree as dt
import subset_ref as sr
from nsdp_amd import _lib, build as nsdp_build, datastore, synth, train

ENTRY_POINTS = ["nsdp_batch_assemble", "nsdp_subset_draw"]


# ------------------------------------------------------------------------------------------------------------------ pair lists
@pytest.fixture(scope="module")
def trees(tmp_path_factory):
    root = str(tmp_path_factory.mktemp("trees"))
    return {kind: dt.rebuild(kind, root) for kind in ("deform4d", "deformtransfer")}


@pytest.mark.parametrize("name", sorted(dt.cases("pairs")))
def test_pair_lists_equal_the_references(trees, name):
    z, cfg = dt.golden(), dt.cases("pairs")[name]
    config = {"data": dt.case_data(trees[cfg["tree"]], cfg)}
    split, sampled = cfg["motion_split"], cfg["num_sampled_pairs"]
    train_split = split[:5] == "train"
    store = datastore.SampleStore(config, "identity_seen", split, pairs_only=True)
    assert dt.pair_rows(store.sample_pairs(0)) == z[f"pairs/{name}/loaded"].tolist()
    assert len(store) == len(z[f"pairs/{name}/loaded"]) > 0
    # one more random_shuffle_samples: a train split's next epoch here; for the others the function itself
    again = store.sample_indices(1) if train_split else store.order_after(1)
    assert dt.pair_rows([store.pairs[i] for i in again]) == z[f"pairs/{name}/reshuffled"].tolist()
    few = datastore.SampleStore(config, "identity_seen", split, num_sampled_pairs=sampled, pairs_only=True)
    assert dt.pair_rows(few.sample_pairs(0)) == z[f"pairs/{name}/loaded_sampled"].tolist() and len(few) == min(sampled, len(few.pairs))
    again = few.sample_indices(1) if train_split else few.order_after(2)[:sampled]
    assert dt.pair_rows([few.pairs[i] for i in again]) == z[f"pairs/{name}/reshuffled_sampled"].tolist()
    if not train_split:                # a sampled evaluation split is shuffled once and stays
        assert few.sample_indices(3) == few.sample_indices(0)


def test_cases_cover_the_rules():
    names = set(dt.cases("pairs"))
    for kind in ("deform4d", "deformtransfer"):
        for mode in ("arbitrary", "canonical"):
            assert {f"{kind}/{mode}/train_seen", f"{kind}/{mode}/test_unseen_motions"} <= names
    z = dt.golden()
    sources = {tuple(r[4:6]) for r in z["pairs/deformtransfer/arbitrary/test_unseen_motions/loaded"].tolist()}
    assert sources == {("cat-run", "0003"), ("horse-run", "0005"), ("dog-run", "0001")}       # the per-animal source frame
    frames = {r[7] for r in z["pairs/deform4d/arbitrary/train_seen/loaded"].tolist()}
    assert frames == {"0000", "0002", "0004"}                                                   # the interval filter


def test_epoch_permutation_is_a_function_of_seed_and_epoch():
    a = datastore.epoch_permutation(5, 2, 40)
    assert np.array_equal(a, datastore.epoch_permutation(5, 2, 40)) and sorted(a.tolist()) == list(range(40))
    assert not np.array_equal(a, datastore.epoch_permutation(5, 3, 40)) and not np.array_equal(a, datastore.epoch_permutation(6, 2, 40))


# ------------------------------------------------------------------------------------------------------------------ the draw
def test_emulation_is_a_bijection_for_every_small_n():
    for n in range(1, 301):
        rows = sr.draw(np.full(2, n), n, seed=11, epoch=1, step=n, which=sr.SURFACE)
        assert rows.dtype == np.int32 and np.array_equal(np.sort(rows, axis=1), np.tile(np.arange(n), (2, 1))), n
    rows = sr.draw([1 << 20], 1 << 20, 3, 0, 0, sr.SPACE)                       # the largest frame: a full permutation
    assert np.array_equal(np.sort(rows[0]), np.arange(1 << 20))


def test_emulation_is_a_function_of_its_key_alone():
    base = dict(seed=(7 << 32) | 9, epoch=4, step=6, which=sr.SURFACE)
    a = sr.draw([1000, 1000], 200, **base)
    assert np.array_equal(a, sr.draw([1000, 1000], 200, **base))
    assert np.array_equal(a[:, :50], sr.draw([1000, 1000], 50, **base))          # row j does not depend on n_keep
    assert np.array_equal(a[1], sr.draw([1000], 200, b0=1, **base)[0])           # nor on the rest of the batch
    assert not np.array_equal(a[0], a[1])                                         # b
    for change in (dict(which=sr.SPACE), dict(step=7), dict(epoch=5), dict(seed=(7 << 32) | 10), dict(seed=(8 << 32) | 9)):
        assert not np.array_equal(a, sr.draw([1000, 1000], 200, **dict(base, **change))), change


@pytest.mark.parametrize("n_full,n_keep", [(64, 16), (65, 16), (1000, 250)])
def test_emulation_is_uniform_within_six_sigma(n_full, n_keep):
    rows = sr.draw(np.full(4096, n_full), n_keep, seed=2024, epoch=0, step=0, which=sr.SURFACE)
    assert not sr.uniformity_violations(rows, n_full, n_keep)


# ------------------------------------------------------------------------------------------------------------------ refusals
def _tree(tmp_path, **kw):
    spec = dict(identities=["ant", "bee"], motions=["walk", "jump"], frames=3, n_surface=20, n_space=12, dtype=np.float16)
    spec.update(kw)
    return {"data": synth.write_dataset_tree(str(tmp_path), **spec)}


def _store(config, **kw):
    return datastore.SampleStore(config, "identity_seen", "train_seen", device="cpu", byte_budget=kw.pop("byte_budget", 1 << 30), **kw)


def test_refusals_carry_their_names(tmp_path):
    config = _tree(tmp_path / "ok")
    config["data"].update(num_surf_samples=16, num_space_samples=8)
    for kind in ("tosca", "dogrec"):
        with pytest.raises(datastore.DataStoreError, match=kind):
            _store({"data": dict(config["data"], type=kind)})
    with pytest.raises(datastore.DataStoreError, match="load_mesh"):
        _store(config, load_mesh=True)
    with pytest.raises(datastore.DataStoreError, match="partial_shape_ratio"):
        _store({"data": dict(config["data"], partial_shape_ratio=0.8)})
    with pytest.raises(datastore.DataStoreError, match="num_surf_samples = 21"):
        _store({"data": dict(config["data"], num_surf_samples=21)})
    with pytest.raises(datastore.DataStoreError, match=r"byte budget of 1000 bytes") as e:
        _store(config, byte_budget=1000)
    assert "6 frames need" in str(e.value)
    with pytest.raises(datastore.DataStoreError, match="missing split list"):
        datastore.SampleStore(config, "identity_seen", "train_nowhere", device="cpu", byte_budget=1 << 30)
    with pytest.raises(datastore.DataStoreError, match="missing dataset_dir"):
        _store({"data": dict(config["data"], dataset_dir=str(tmp_path / "nowhere"))})
    with pytest.raises(_lib.NsdpHipError, match="GPU"):            # everything in order: the store itself needs a device
        _store(config)
    # files: a missing file, a missing key
    broken = _tree(tmp_path / "missing_file")
    os.remove(os.path.join(broken["data"]["dataset_dir"], "bee_walk", "0001", "flow.npz"))
    with pytest.raises(datastore.DataStoreError, match=r"missing file .*bee_walk.0001.flow\.npz"):
        _store(broken)
    broken = _tree(tmp_path / "missing_key")
    path = os.path.join(broken["data"]["dataset_dir"], "ant_walk", "0002", "surface_points.npz")
    np.savez(path, points=np.load(path)["points"])
    with pytest.raises(datastore.DataStoreError, match="no array 'normals'"):
        _store(broken)
    # counts: the frames of a pair differ in surface count; space counts neither all above the request nor all equal
    broken = _tree(tmp_path / "surface_counts")
    path = os.path.join(broken["data"]["dataset_dir"], "ant_walk", "0001", "surface_points.npz")
    z = np.load(path)
    np.savez(path, points=z["points"][:-1], normals=z["normals"][:-1])
    with pytest.raises(datastore.DataStoreError, match="differ in surface count"):
        _store({"data": dict(broken["data"], num_surf_samples=8)})
    mixed = _tree(tmp_path / "space_counts", n_space=[12, 6])
    with pytest.raises(datastore.DataStoreError, match="neither all above num_space_samples = 8 nor all equal"):
        _store({"data": dict(mixed["data"], num_surf_samples=8, num_space_samples=8)})


def test_dataset_and_synthetic_together_are_an_error(tmp_path):
    with pytest.raises(SystemExit) as e:
        train.main([str(tmp_path / "config.yaml"), str(tmp_path / "run"), "--dataset", "--synthetic", "4"])
    assert "--dataset" in str(e.value) and "--synthetic 4" in str(e.value)
    assert not (tmp_path / "run").exists()


def test_written_tree_follows_both_namings(tmp_path):
    for kind, sep in (("deform4d", "_"), ("deformtransfer", "-")):
        data = synth.write_dataset_tree(str(tmp_path / kind), ["ant", "bee"], ["walk", "jump"], 2, [10, 12], 6, np.float32, data_type=kind)
        assert sorted(os.listdir(data["dataset_dir"])) == sorted(f"{i}{sep}{m}" for i in ("ant", "bee") for m in ("walk", "jump"))
        frame = os.path.join(data["dataset_dir"], f"bee{sep}jump", "0001")
        assert sorted(os.listdir(frame)) == ["flow.npz", "orig_to_gaps.txt", "surface_points.npz"]
        z = np.load(os.path.join(frame, "surface_points.npz"))
        assert z["points"].shape == z["normals"].shape == (12, 3) and z["points"].dtype == np.float32
        assert np.array_equal(np.loadtxt(os.path.join(frame, "orig_to_gaps.txt")).reshape(4, 4), np.eye(4))
        assert sorted(os.listdir(os.path.join(data["split_dir"], kind))) == ["identity_seen.lst", "test_unseen_motions.lst", "train_seen.lst"]
        store = datastore.SampleStore({"data": data}, "identity_seen", "train_seen", pairs_only=True)
        assert len(store) == 2 * 2                     # two identities x one training motion x two frames
    with pytest.raises(ValueError, match="neither"):
        synth.write_dataset_tree(str(tmp_path / "x"), ["a"], ["m"], 1, 4, 4, data_type="tosca")


# ------------------------------------------------------------------------------------------------------------------ boundary
@pytest.fixture(scope="module")
def so():
    if not os.path.exists(_lib.SO_PATH):
        nsdp_build.build()
    lib = ctypes.CDLL(_lib.SO_PATH)
    lib.nsdp_last_error.restype = ctypes.c_char_p
    return lib


def test_header_declares_and_library_exports_the_entries(so):
    # (nsdp_hip.h keeps its own table of entries, which the poisoned-arena accounting walks: the later headers are asked by name)
    assert _lib.declared_symbols("nsdp_batch.h") == sorted(ENTRY_POINTS)
    assert not set(ENTRY_POINTS) & set(_lib.declared_symbols())
    for name in ENTRY_POINTS:
        assert hasattr(so, name), name
    assert so.nsdp_abi_version() >= 22
    assert "nsdp_batch.h" in open(nsdp_build.__file__).read() and nsdp_build.PER_FILE["batch_assemble.hip"] == nsdp_build.EXACT


def test_bad_arguments_return_status_and_launch_nothing(so):
    one = ctypes.c_void_p(16)          # (a non-null, aligned pointer the library must not touch: nothing may be launched)
    odd = ctypes.c_void_p(18)
    u64, u32, ll, f = ctypes.c_uint64, ctypes.c_uint32, ctypes.c_longlong, ctypes.c_float

    def draw(n_full=one, B=2, n_keep=4, which=0, out=one):
        return so.nsdp_subset_draw(n_full, B, n_keep, u64(1), u32(0), u32(0), which, out, None)

    for kw, word in ((dict(B=-1), "B=-1"), (dict(B=65536), "B=65536"), (dict(n_keep=-3), "n_keep=-3"),
                     (dict(n_keep=(1 << 20) + 1), "n_keep=1048577"), (dict(B=4096, n_keep=1 << 20), "too large"),
                     (dict(which=2), "which=2"), (dict(n_full=None), "null"), (dict(out=None), "null"), (dict(out=odd), "aligned"),
                     (dict(B=-1, n_full=None, out=None), "B=-1")):          # sizes are judged before pointers
        assert draw(**kw) == -1 and word.encode() in so.nsdp_last_error() and b"subset_draw" in so.nsdp_last_error(), kw
    assert draw(B=0, n_full=None, out=None) == 0 and draw(n_keep=0, n_full=None, out=None) == 0

    def assemble(**kw):
        a = dict(surface=one, surface_rows=10, space=one, space_rows=10, table=one, frames=2, ids=one, B=2, surf_idx=one, n=4, space_idx=one,
                 m=4, partial_range=0.1, noise=None, level=0.0, surface_out=one, handle=one, inputs=one, space_out=one)
        a.update(kw)
        return so.nsdp_batch_assemble(a["surface"], ll(a["surface_rows"]), 1, a["space"], ll(a["space_rows"]), 1, a["table"], a["frames"],
                                      a["ids"], a["B"], a["surf_idx"], a["n"], a["space_idx"], a["m"], f(a["partial_range"]), a["noise"],
                                      f(a["level"]), a["surface_out"], a["handle"], a["inputs"], a["space_out"], None)

    for kw, word in ((dict(B=-2), "B=-2"), (dict(B=65536), "B=65536"), (dict(n=-1), "n=-1"), (dict(m=-1), "m=-1"),
                     (dict(n=(1 << 20) + 1), "n=1048577"), (dict(m=(1 << 20) + 1), "m=1048577"), (dict(B=1024, n=1 << 17), "too large"),
                     (dict(frames=0), "n_frames=0"), (dict(surface_rows=0), "surface_rows=0"), (dict(space_rows=-4), "space_rows=-4"),
                     (dict(partial_range=float("nan")), "partial_range"), (dict(level=float("inf")), "noise_level"),
                     (dict(table=None), "null"), (dict(ids=None), "null"), (dict(surface=None), "null"), (dict(surf_idx=None), "null"),
                     (dict(surface_out=None), "null"), (dict(handle=None), "null"), (dict(inputs=None), "null"), (dict(space=None), "null"),
                     (dict(space_out=None), "null"), (dict(surface=odd), "16-byte"), (dict(space=ctypes.c_void_p(24)), "16-byte"),
                     (dict(table=ctypes.c_void_p(20)), "8-byte"), (dict(noise=odd), "4-byte"), (dict(space_idx=odd), "4-byte"),
                     (dict(frames=0, table=None, ids=None), "n_frames=0")):
        assert assemble(**kw) == -1 and word.encode() in so.nsdp_last_error() and b"batch_assemble" in so.nsdp_last_error(), kw
    assert assemble(B=0, table=None, ids=None) == 0
    assert assemble(n=0, m=0, table=None, ids=None, surface=None, space=None) == 0
