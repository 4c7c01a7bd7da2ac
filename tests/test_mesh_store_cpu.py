"""CPU: the mesh data path without a device (nsdp_amd/meshstore.py, include/nsdp_meshbatch.h).  The area thresholds; the sampling
RULE's statistics, checked on its numpy emulation alone (tests/mesh_sample_ref.py -- the GPU tests pin the kernel to that
emulation bit for bit, so nothing statistical runs on the GPU); the store's pair rules, normalisation and refusals; the trainer's
flags; and the boundary of the header: declared, exported at ABI version 23, bad arguments come back as a status."""
import ctypes
import os

import numpy as np
import pytest

import mesh_sample_ref as mr
from nsdp_amd import _lib, build as nsdp_build, datastore, meshio, meshstore, synth, train

ENTRY_POINTS = ["nsdp_mesh_batch_sample"]


# ------------------------------------------------------------------------------------------------------------------ thresholds
def _areas(verts, faces):
    v = verts.astype(np.float32).astype(np.float64)
    return np.linalg.norm(np.cross(v[faces[:, 1]] - v[faces[:, 0]], v[faces[:, 2]] - v[faces[:, 0]]), axis=1)


@pytest.mark.parametrize("zero_area", [(17, 199), (0, 1, 198, 199), ()])
def test_thresholds_are_monotone_end_at_2_31_and_repeat_exactly_at_zero_area_faces(zero_area):
    verts, faces = mr.grid(zero_area=zero_area)
    T = meshstore.area_thresholds(verts.astype(np.float32), faces)
    assert T.dtype == np.uint32 and T.shape == (200,)
    t = T.astype(np.int64)
    assert np.all(np.diff(t) >= 0) and t[-1] == 1 << 31
    equal_to_previous = np.concatenate([[t[0] == 0], np.diff(t) == 0])
    assert sorted(np.nonzero(equal_to_previous)[0].tolist()) == sorted(zero_area)           # (a trailing zero-area face too)
    area = _areas(verts, faces)
    assert np.array_equal(area == 0, equal_to_previous)
    # the definition, restated: floor(cdf / total * 2^31), 2^31 from the last face of positive area on
    cdf = np.cumsum(area)
    want = np.floor(cdf / cdf[-1] * 2.0 ** 31)
    want[np.nonzero(area > 0)[0][-1]:] = 2.0 ** 31
    assert np.array_equal(t, want.astype(np.int64))
    # the first face with T[f] > r, at both ends of the draw's range
    assert mr.search(T, np.array([0, (1 << 31) - 1], dtype=np.uint32)).tolist() == [int(np.nonzero(area > 0)[0][0]), int(np.nonzero(area > 0)[0][-1])]
    with pytest.raises(ValueError, match="not positive"):
        meshstore.area_thresholds(np.zeros((3, 3), np.float32), np.array([[0, 1, 2]], np.int32))


def test_search_is_the_first_threshold_above_the_draw():
    g = np.random.RandomState(0)
    for F in (1, 2, 3, 4, 5, 31, 32, 33, 200):
        T = np.sort(g.randint(0, 1 << 31, size=F).astype(np.uint32))
        T[F // 2:F // 2 + 2] = T[F // 2]                                               # equal neighbours
        T[-1] = 1 << 31
        r = np.concatenate([g.randint(0, 1 << 31, size=500), T[:-1], T[:-1] - (T[:-1] > 0), [0, (1 << 31) - 1]]).astype(np.uint32)
        assert np.array_equal(mr.search(T, r), np.searchsorted(T, r, side="right")), F


# ------------------------------------------------------------------------------------------------------------------ statistics
@pytest.fixture(scope="module")
def drawn():
    """64 samples x 4096 rows on the 200-face grid with two zero-area faces: faces and integer weights of every row."""
    verts, faces = mr.grid()
    T = meshstore.area_thresholds(verts.astype(np.float32), faces)
    f, iw, iu, iv = [], [], [], []
    for b in range(64):
        w = mr.words(1234, 0, 7, b, mr.MESH_SURFACE, np.arange(4096))
        f.append(mr.search(T, w[0] >> np.uint32(1)))
        a, u, v = mr.weights(w)
        iw.append(a), iu.append(u), iv.append(v)
    return _areas(verts, faces), np.concatenate(f), np.concatenate(iw), np.concatenate(iu), np.concatenate(iv)


def test_faces_are_drawn_by_area(drawn):
    area, f, *_ = drawn
    N = f.shape[0]
    counts = np.bincount(f, minlength=200)
    assert counts[area == 0].sum() == 0 and (area == 0).sum() == 2                       # a zero-area face is never drawn
    expected = N * area / area.sum()
    keep = expected >= 5
    chi2 = float((((counts - expected) ** 2)[keep] / expected[keep]).sum())
    dof = int(keep.sum()) - 1
    print(f"chi2 = {chi2:.1f} for {dof} degrees of freedom, bound {dof + 6 * np.sqrt(2 * dof):.1f}")
    assert dof >= 150 and chi2 < dof + 6.0 * np.sqrt(2.0 * dof)


def test_weights_are_exact_and_uniform_on_the_triangle(drawn):
    _, _, iw, iu, iv = drawn
    N = iw.shape[0]
    assert iw.min() >= 0 and iu.min() >= 0 and iv.min() >= 0 and np.all(iw + iu + iv == mr.ONE24)
    w0, u, v = mr.as_weight(iw), mr.as_weight(iu), mr.as_weight(iv)
    for x, i in ((w0, iw), (u, iu), (v, iv)):
        assert x.dtype == np.float32 and np.array_equal(x.astype(np.float64) * 2.0 ** 24, i)      # exact in fp32
    assert np.all((w0 + u) + v == np.float32(1)) and np.all((1 - u) - v == w0)             # fp32 sums, no rounding anywhere
    sigma = np.sqrt(1.0 / 18.0 / N)
    for name, x in (("w0", w0), ("u", u), ("v", v)):
        z = abs(float(x.astype(np.float64).mean()) - 1.0 / 3.0) / sigma
        print(f"mean of {name}: {z:.2f} sigma from 1/3")
        assert z < 6.0
    half = mr.ONE24 // 2
    parts = [iw > half, iu > half, iv > half]
    parts.append(~(parts[0] | parts[1] | parts[2]))
    for k, part in enumerate(parts):                                                       # the four midpoint sub-triangles
        z = abs(int(part.sum()) - N / 4.0) / np.sqrt(N * 0.25 * 0.75)
        print(f"sub-triangle {k}: {z:.2f} sigma from a quarter")
        assert z < 6.0


def test_the_two_draws_and_the_row_subsets_use_different_streams():
    j = np.arange(64)
    seen = [mr.words(5, 1, 2, 0, which, j)[0].tolist() for which in (0, 1, mr.MESH_SURFACE, mr.MESH_SPACE)]
    assert all(seen[a] != seen[b] for a in range(4) for b in range(a))
    assert (meshstore.MESH_SURFACE, meshstore.MESH_SPACE) == (mr.MESH_SURFACE, mr.MESH_SPACE) == (2, 3)
    assert (datastore.SURFACE, datastore.SPACE) == (0, 1)


def test_emulated_samples_lie_on_their_triangles():
    """The emulation end to end on the host arrays: surface rows inside the vertex box, normals of unit length, space rows
    within sigma of the surface, halves split at m // 2."""
    verts, faces = mr.grid()
    frames = [mr.deform(verts, k).astype(np.float32) for k in range(3)]
    arrays = meshstore.pack(frames, [0, 0, 0], [faces], [0])
    ids = np.array([[0], [1], [2]], dtype=np.int32)
    out = mr.sample(arrays, ids, 500, 7, 9, 0, 3, 0.1, 0.1, 0.02)
    for c, name in enumerate(("cano", "src", "tgt")):
        p, nrm = out[f"surface_samples_{name}"][0], out[f"surface_normals_{name}"][0]
        assert np.all(p >= frames[c].min(axis=0) - 1e-6) and np.all(p <= frames[c].max(axis=0) + 1e-6)
        np.testing.assert_allclose(np.linalg.norm(nrm.astype(np.float64), axis=1), 1.0, atol=1e-6)
    assert np.array_equal(out["surface_samples_inputs"][0, :, :3], out["surface_samples_src"][0])
    m_out = mr.sample(arrays, ids, 7, 7, 9, 0, 3, 0.1, 0.1, 0.02)
    surf = mr.sample(arrays, ids, 0, 0, 9, 0, 3, 0.1, 0.1, 0.02)
    assert surf["space_samples_cano"].shape == (1, 0, 3) and m_out["space_samples_cano"].shape == (1, 7, 3)
    zero = mr.sample(arrays, ids, 0, 7, 9, 0, 3, 0.1, 0.0, 0.0)["space_samples_tgt"][0]      # sigma = 0: the points on the surface
    d = np.linalg.norm(m_out["space_samples_tgt"][0].astype(np.float64) - zero, axis=1)
    assert np.all(d[:3] <= 0.1 + 1e-6) and np.all(d[3:] <= 0.02 + 1e-6) and d[:3].max() > 0.02      # 7 // 2 = 3 rows of sigma1


# ------------------------------------------------------------------------------------------------------------------ the store
def _meshes():
    return {"tet": mr.tetrahedron(), "oct": mr.octahedron(), "grid": mr.grid()}


def _tree(root, **kw):
    spec = dict(motions=["walk", "jump", "turn"], frames=3, seed=4)
    spec.update(kw)
    return synth.write_mesh_dataset_tree(str(root), _meshes(), **spec)


def _store(data, **kw):
    args = dict(device="cpu", byte_budget=1 << 30)
    args.update(kw)
    return meshstore.MeshStore({"data": data}, "identity_seen", "train_seen", **args)


def test_pair_rules_are_the_sample_stores(tmp_path):
    for kind in ("deform4d", "deformtransfer"):
        data = _tree(tmp_path / kind, data_type=kind)
        for split, sampled in (("train_seen", -1), ("train_seen", 5), ("test_unseen_motions", -1), ("test_unseen_motions", 4)):
            a = meshstore.MeshStore({"data": data}, "identity_seen", split, num_sampled_pairs=sampled, pairs_only=True)
            b = datastore.SampleStore({"data": data}, "identity_seen", split, num_sampled_pairs=sampled, pairs_only=True)
            assert a.pairs == b.pairs and len(a) == len(b) and len(a) > 0
            assert all(a.sample_indices(e) == b.sample_indices(e) for e in range(3))
    assert meshstore.form_pairs is datastore.form_pairs and issubclass(meshstore.MeshLoader, datastore.StoreLoader)
    assert meshstore.MeshLoader.epoch_samples is datastore.StoreLoader.epoch_samples      # (imported, not copied)
    assert meshstore.MeshLoader.shard is datastore.StoreLoader.shard
    # one store core: both stores derive from it, neither from the other, and what they share is the same function objects
    assert issubclass(meshstore.MeshStore, datastore.PairStore) and issubclass(datastore.SampleStore, datastore.PairStore)
    assert datastore.SampleStore not in meshstore.MeshStore.__mro__
    for name in ("sample_indices", "order_after", "frame_bbox"):
        assert getattr(meshstore.MeshStore, name) is getattr(datastore.SampleStore, name) is getattr(datastore.PairStore, name), name
    assert meshstore.MeshLoader._batches is datastore.StoreLoader._batches


def test_vertices_are_normalised_in_float64_and_rounded_once(tmp_path):
    o2w = np.array([[0.7, 0.1, -0.2, 0.05], [-0.1, 0.9, 0.3, -0.02], [0.2, -0.3, 0.8, 0.01], [0, 0, 0, 1]])
    data = _tree(tmp_path / "orig", mesh_file="mesh.obj", orig2world=o2w)
    d = os.path.join(data["dataset_dir"], "grid_jump", "0002")
    raw, faces = meshio.read_mesh(os.path.join(d, "mesh.obj"))
    m = np.loadtxt(os.path.join(d, "orig_to_gaps.txt")).reshape(4, 4).astype(np.float32).astype(np.float64)
    want = (m[:3, :3] @ raw.T + m[:3, 3:4]).T.astype(np.float32)
    got, got_faces = meshstore.read_frame(data, d)
    assert got.dtype == np.float32 and np.array_equal(got, want) and np.array_equal(got_faces, faces)
    assert not np.array_equal(got, (m.astype(np.float32)[:3, :3] @ raw.astype(np.float32).T + m.astype(np.float32)[:3, 3:4]).T)
    fixed, _ = meshstore.read_frame(dict(data, fix_coord_system=True), d)
    assert np.array_equal(fixed, np.stack([want[:, 0], -want[:, 2], want[:, 1]], axis=1))
    # "norm" in the file's name: the vertices are taken as they are
    normed = _tree(tmp_path / "norm", mesh_file="mesh_norm.ply", orig2world=o2w)
    d = os.path.join(normed["dataset_dir"], "grid_jump", "0002")
    assert np.array_equal(meshstore.read_frame(normed, d)[0], meshio.read_mesh(os.path.join(d, "mesh_norm.ply"))[0].astype(np.float32))


def test_every_refusal_is_raised_by_name(tmp_path, monkeypatch):
    data = _tree(tmp_path / "good")
    with pytest.raises(_lib.NsdpHipError, match="needs a GPU"):             # everything on the host passed: only the device is missing
        _store(data)
    with pytest.raises(meshstore.MeshStoreError, match="more than the byte budget of 1000 bytes"):
        _store(data, byte_budget=1000)
    for kind in ("tosca", "dogrec"):
        with pytest.raises(meshstore.MeshStoreError, match=kind):
            _store(dict(data, type=kind))
    with pytest.raises(meshstore.MeshStoreError, match="load_mesh"):
        _store(data, load_mesh=True)
    with pytest.raises(meshstore.MeshStoreError, match="partial"):
        _store(dict(data, partial_shape_ratio=0.5))
    assert issubclass(meshstore.MeshStoreError, datastore.DataStoreError)
    # a missing mesh file
    broken = _tree(tmp_path / "missing")
    gone = os.path.join(broken["dataset_dir"], "oct_jump", "0001", "mesh_norm.ply")
    os.remove(gone)
    with pytest.raises(meshstore.MeshStoreError, match="missing mesh file .*oct_jump.0001.mesh_norm.ply"):
        _store(broken)
    # a topology mismatch inside a pair: both directories are named
    broken = _tree(tmp_path / "topology")
    path = os.path.join(broken["dataset_dir"], "tet_jump", "0002", "mesh_norm.ply")
    verts, faces = meshio.read_mesh(path)
    meshio.write_mesh(path, verts.astype(np.float32), faces[:, [1, 2, 0]])
    with pytest.raises(meshstore.MeshStoreError, match="differ in topology") as e:
        _store(broken)
    assert os.path.join("tet_walk", "0000") in str(e.value) and os.path.join("tet_jump", "0002") in str(e.value)
    # a canonical frame of zero total area
    broken = _tree(tmp_path / "flat")
    for motion in ("walk", "jump", "turn"):
        for f in range(3):
            path = os.path.join(broken["dataset_dir"], f"tet_{motion}", "%04d" % f, "mesh_norm.ply")
            verts, faces = meshio.read_mesh(path)
            meshio.write_mesh(path, np.outer(np.arange(4), [1.0, 2.0, 3.0]).astype(np.float32), faces)      # collinear vertices
    with pytest.raises(meshstore.MeshStoreError, match="zero total area") as e:
        _store(broken)
    assert os.path.join("tet_walk", "0000") in str(e.value)
    # the per-frame limit (lowered here: a frame of 2^21 + 1 vertices is 25 MB of text)
    monkeypatch.setattr(meshstore, "MAX_ELEMS", 100)
    with pytest.raises(meshstore.MeshStoreError, match="121 vertices / 200 faces, more than the 100 a frame may hold"):
        _store(data)
    assert mr.MAX_ELEMS == 1 << 21


def test_thresholds_are_computed_once_and_operands_must_share_a_device(monkeypatch):
    import torch
    verts, faces = mr.grid()
    frames = [mr.deform(verts, k).astype(np.float32) for k in range(2)]
    plain = meshstore.pack(frames, [0, 0], [faces], [0])
    calls = []
    real = meshstore.area_thresholds
    monkeypatch.setattr(meshstore, "area_thresholds", lambda *a: calls.append(1) or real(*a))
    given = meshstore.pack(frames, [0, 0], [faces], [0], {0: real(frames[0], faces)})
    assert not calls and all(np.array_equal(plain[k], given[k]) for k in plain)          # taken as they are, not computed again
    meshstore.pack(frames, [0, 0], [faces], [0, 1], {0: real(frames[0], faces)})
    assert len(calls) == 1                                                                # only the frame that came without
    t = {k: torch.from_numpy(v.view(np.int32) if v.dtype == np.uint32 else v) for k, v in plain.items()}
    ids = torch.zeros((3, 1), dtype=torch.int32)
    args = lambda **kw: [dict(t, **kw)[k] for k in ("vert_arena", "face_arena", "thr_arena", "frame_table", "topo_table")]
    with pytest.raises(_lib.NsdpHipError, match="GPU tensor"):                            # no fallback for CPU tensors
        meshstore.mesh_batch_sample(*args(), ids, 4, 4, 1, 0, 0, 0.1, 0.1, 0.02)
    for name in ("vert_arena", "face_arena", "thr_arena", "frame_table", "topo_table"):
        with pytest.raises(_lib.NsdpHipError, match=f"{name} lives on meta, frame_ids on cpu"):
            meshstore.mesh_batch_sample(*args(**{name: t[name].to("meta")}), ids, 4, 4, 1, 0, 0, 0.1, 0.1, 0.02)
    with pytest.raises(_lib.NsdpHipError, match="noise lives on meta"):
        meshstore.mesh_batch_sample(*args(), ids, 4, 4, 1, 0, 0, 0.1, 0.1, 0.02, torch.zeros((1, 4, 3), device="meta"), 0.02)


def test_mesh_dataset_excludes_the_other_sources(tmp_path):
    for other, word in ((["--dataset"], "--dataset"), (["--synthetic", "4"], "--synthetic 4")):
        with pytest.raises(SystemExit) as e:
            train.main([str(tmp_path / "config.yaml"), str(tmp_path / "run"), "--mesh-dataset"] + other)
        assert "--mesh-dataset" in str(e.value) and word in str(e.value)
    assert not (tmp_path / "run").exists() and callable(train.mesh_dataset_loaders)


# ------------------------------------------------------------------------------------------------------------------ boundary
@pytest.fixture(scope="module")
def so():
    if not os.path.exists(_lib.SO_PATH):
        nsdp_build.build()
    lib = ctypes.CDLL(_lib.SO_PATH)
    lib.nsdp_last_error.restype = ctypes.c_char_p
    return lib


def test_header_declares_and_library_exports_the_entries(so):
    assert _lib.declared_symbols("nsdp_meshbatch.h") == sorted(ENTRY_POINTS)
    assert not set(ENTRY_POINTS) & set(_lib.declared_symbols()) and not set(ENTRY_POINTS) & set(_lib.declared_symbols("nsdp_batch.h"))
    for name in ENTRY_POINTS:
        assert hasattr(so, name), name
    assert so.nsdp_abi_version() >= 23
    assert "nsdp_meshbatch.h" in open(nsdp_build.__file__).read() and nsdp_build.PER_FILE["mesh_sample.hip"] == nsdp_build.EXACT
    header = open(os.path.join(os.path.dirname(_lib.HEADER_PATH), "nsdp_meshbatch.h")).read()
    assert "#define NSDP_DRAW_MESH_SURFACE 2" in header and "#define NSDP_DRAW_MESH_SPACE 3" in header
    assert "#define NSDP_MESH_MAX_ELEMS (1 << 21)" in header


def test_bad_arguments_return_status_and_launch_nothing(so):
    one, odd = ctypes.c_void_p(16), ctypes.c_void_p(18)       # (non-null pointers the library must not touch: nothing may be launched)
    u64, u32, ll, f = ctypes.c_uint64, ctypes.c_uint32, ctypes.c_longlong, ctypes.c_float

    def sample(**kw):
        a = dict(verts=one, vert_rows=10, faces=one, face_rows=10, thr=one, thr_rows=10, table=one, frames=2, topos=one, n_topos=1,
                 ids=one, B=2, n=4, m=4, partial_range=0.1, sigma1=0.1, sigma2=0.02, noise=None, level=0.0, surface_out=one,
                 handle=one, inputs=one, space_out=one)
        a.update(kw)
        return so.nsdp_mesh_batch_sample(a["verts"], ll(a["vert_rows"]), a["faces"], ll(a["face_rows"]), a["thr"], ll(a["thr_rows"]),
                                         a["table"], a["frames"], a["topos"], a["n_topos"], a["ids"], a["B"], a["n"], a["m"], u64(1),
                                         u32(0), u32(0), f(a["partial_range"]), f(a["sigma1"]), f(a["sigma2"]), a["noise"], f(a["level"]),
                                         a["surface_out"], a["handle"], a["inputs"], a["space_out"], None)

    for kw, word in ((dict(B=-2), "B=-2"), (dict(B=65536), "B=65536"), (dict(n=-1), "n=-1"), (dict(m=-1), "m=-1"),
                     (dict(n=(1 << 20) + 1), "n=1048577"), (dict(m=(1 << 20) + 1), "m=1048577"), (dict(B=1024, n=1 << 17), "too large"),
                     (dict(frames=0), "n_frames=0"), (dict(n_topos=0), "n_topos=0"), (dict(vert_rows=0), "vert_rows=0"),
                     (dict(face_rows=-4), "face_rows=-4"), (dict(thr_rows=0), "thr_rows=0"), (dict(partial_range=float("nan")), "partial_range"),
                     (dict(level=float("inf")), "noise_level"), (dict(sigma1=float("nan")), "sigma"), (dict(sigma2=float("-inf")), "sigma"),
                     (dict(verts=None), "null"), (dict(faces=None), "null"), (dict(thr=None), "null"), (dict(table=None), "null"),
                     (dict(topos=None), "null"), (dict(ids=None), "null"), (dict(surface_out=None), "null"), (dict(handle=None), "null"),
                     (dict(inputs=None), "null"), (dict(space_out=None), "null"), (dict(verts=odd), "16-byte"),
                     (dict(faces=ctypes.c_void_p(24)), "16-byte"), (dict(table=ctypes.c_void_p(20)), "8-byte"),
                     (dict(topos=ctypes.c_void_p(20)), "8-byte"), (dict(noise=odd), "4-byte"), (dict(thr=odd), "4-byte"),
                     (dict(frames=0, table=None, ids=None), "n_frames=0")):          # sizes are judged before pointers
        assert sample(**kw) == -1 and word.encode() in so.nsdp_last_error() and b"mesh_batch_sample" in so.nsdp_last_error(), kw
    assert sample(B=0, table=None, ids=None, verts=None) == 0
    assert sample(n=0, m=0, table=None, ids=None, verts=None, faces=None, thr=None) == 0
