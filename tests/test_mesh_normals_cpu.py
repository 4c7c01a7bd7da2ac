"""CPU: vertex normals without a device (include/nsdp_meshnormals.h, nsdp_amd/mesh_normals.py, tests/mesh_normals_ref.py).  The
boundary of the header: declared there and nowhere else, exported at ABI version 26, built EXACT, bad arguments come back as a
status before anything is launched.  The emulation the GPU tests hold the kernels to is itself held to an fp64 evaluation of the
same fp32 positions, to unit length, and to the geometry (outward on spheres and on a counter-clockwise tetrahedron).  The
wrapper's host-side refusals and the writer's round trip with normals.

The fp64 bound, derived and not fitted.  A term of a vertex's sum is one component of a face's cross product, u v - w x with
u, v, w, x edge components.  With d = 2^-24: each edge component carries one rounding, (1 + d) relative; each product one more,
so a product is exact up to (1 + d)^3; the difference rounds once, and both products enter it, so the face's component is off by
at most ((1 + d)^4 - 1) (|u v| + |w x|) = ((1 + d)^4 - 1) M_q; the sum's order then puts depth(T) additions on a term's way,
each a factor (1 + d) on everything below it.  Together (1 + d)^k - 1 <= gamma_k = k d / (1 - k d) with k = depth(T) + 4,
relative to the sum of the M_q of the vertex's faces (Higham, Accuracy and Stability of Numerical Algorithms, lemma 3.1)."""
import ctypes
import os

import numpy as np
import pytest
import torch

import mesh_normals_ref as mr
from list_order_ref import depth
from nsdp_amd import _lib, build as nsdp_build, meshio

ENTRY_POINTS = ["nsdp_mesh_corner_lists", "nsdp_mesh_corner_lists_workspace_bytes", "nsdp_mesh_vertex_normals"]
SPHERES = [(2, 1100), (3, 40), (6, 12)]


# ------------------------------------------------------------------------------------------------------------------ boundary
@pytest.fixture(scope="module")
def so():
    if not os.path.exists(_lib.SO_PATH):
        nsdp_build.build()
    lib = ctypes.CDLL(_lib.SO_PATH)
    lib.nsdp_last_error.restype = ctypes.c_char_p
    lib.nsdp_mesh_corner_lists_workspace_bytes.restype = ctypes.c_size_t
    lib.nsdp_knn_invert_wide_workspace_bytes.restype = ctypes.c_size_t
    return lib


def test_header_declares_and_library_exports_the_entries(so):
    assert _lib.declared_symbols("nsdp_meshnormals.h") == sorted(ENTRY_POINTS)
    for other in (None, "nsdp_batch.h", "nsdp_meshbatch.h", "nsdp_meshwhole.h", "nsdp_scatter.h", "nsdp_optim.h"):
        assert not set(ENTRY_POINTS) & set(_lib.declared_symbols(other)), other
    for name in ENTRY_POINTS:
        assert hasattr(so, name), name
    assert so.nsdp_abi_version() >= 26
    assert "nsdp_meshnormals.h" in open(nsdp_build.__file__).read() and nsdp_build.PER_FILE["mesh_normals.hip"] == nsdp_build.EXACT


def test_workspace_query(so):
    ws = so.nsdp_mesh_corner_lists_workspace_bytes
    assert ws(1, 100, 200) == 2400 + so.nsdp_knn_invert_wide_workspace_bytes(1, 600, 100) and ws(1, 100, 200) % 16 == 0
    assert ws(3, 1 << 20, (1 << 25) // 3) > 0                                       # the limits themselves are taken
    for B, vcap, fcap in ((0, 10, 10), (65536, 10, 10), (1, 0, 10), (1, (1 << 20) + 1, 10), (1, 10, 0), (1, 10, (1 << 25) // 3 + 1)):
        assert ws(B, vcap, fcap) == 0, (B, vcap, fcap)


def test_bad_arguments_return_status_and_launch_nothing(so):
    one, odd, eight = ctypes.c_void_p(16), ctypes.c_void_p(18), ctypes.c_void_p(24)      # (non-null pointers nothing may touch)

    def lists(**kw):
        a = dict(faces=one, foff=one, voff=one, B=2, vcap=8, fcap=8, ws=one, loff=one, lent=one)
        a.update(kw)
        return so.nsdp_mesh_corner_lists(a["faces"], a["foff"], a["voff"], a["B"], a["vcap"], a["fcap"], a["ws"], a["loff"], a["lent"], None)

    def normals(**kw):
        a = dict(verts=one, P=1, faces=one, foff=one, voff=one, B=2, vcap=8, fcap=8, loff=one, lent=one, fn=one, sums=one, out=one)
        a.update(kw)
        return so.nsdp_mesh_vertex_normals(a["verts"], a["P"], a["faces"], a["foff"], a["voff"], a["B"], a["vcap"], a["fcap"], a["loff"],
                                           a["lent"], a["fn"], a["sums"], a["out"], None)

    sizes = ((dict(B=0), "B=0"), (dict(B=65536), "B=65536"), (dict(vcap=0), "vcap=0"), (dict(vcap=(1 << 20) + 1), "vcap=1048577"),
             (dict(fcap=0), "fcap=0"), (dict(fcap=-3), "fcap=-3"), (dict(fcap=(1 << 25) // 3 + 1), "fcap=11184811"),
             (dict(vcap=0, faces=None), "vcap=0"))                                       # sizes are judged before pointers
    for kw, word in sizes + ((dict(faces=None), "null"), (dict(foff=None), "null"), (dict(voff=None), "null"), (dict(ws=None), "null"),
                             (dict(loff=None), "null"), (dict(lent=None), "null"), (dict(ws=eight), "16-byte"),
                             (dict(faces=odd), "4-byte"), (dict(foff=odd), "4-byte"), (dict(voff=odd), "4-byte"),
                             (dict(loff=odd), "4-byte"), (dict(lent=odd), "4-byte"),
                             (dict(ws=eight, lent=None), "null")):                       # pointers before alignment
        assert lists(**kw) == -1 and word.encode() in so.nsdp_last_error() and b"mesh_corner_lists" in so.nsdp_last_error(), kw
    for kw, word in sizes + ((dict(P=0), "P=0"), (dict(P=65536), "P=65536"), (dict(P=0, B=0), "P=0"),
                             (dict(verts=None), "null"), (dict(faces=None), "null"), (dict(foff=None), "null"),
                             (dict(voff=None), "null"), (dict(loff=None), "null"), (dict(lent=None), "null"), (dict(fn=None), "null"),
                             (dict(out=None), "null"), (dict(verts=odd), "4-byte"), (dict(faces=odd), "4-byte"),
                             (dict(loff=odd), "4-byte"), (dict(fn=odd), "4-byte"), (dict(sums=odd), "4-byte"), (dict(out=odd), "4-byte"),
                             (dict(sums=odd, out=None), "null")):
        assert normals(**kw) == -1 and word.encode() in so.nsdp_last_error() and b"mesh_vertex_normals" in so.nsdp_last_error(), kw


# ------------------------------------------------------------------------------------------------------------------ emulation
@pytest.fixture(scope="module")
def evaluated():
    """name -> (packed operands, the fp32 emulation, the fp64 evaluation), once for every test below."""
    out = {}
    meshes = dict({f"sphere{r}x{s}": ([mr.sphere(r, s)], None, None) for r, s in SPHERES}, **mr.cases())
    for name, (shapes, vcap, fcap) in meshes.items():
        verts, faces, fo, vo = mr.pack(shapes, vcap, fcap)
        out[name] = ((verts, faces, fo, vo), mr.vertex_normals(verts, faces, fo, vo), mr.reference64(verts, faces, fo, vo))
    return out


def test_emulated_lists_are_the_stable_sort(evaluated):
    (verts, faces, fo, vo), got, _ = evaluated["packed"]
    offsets, entries = got["list_offsets"], got["list_entries"]
    assert offsets[0] == 0 and offsets[-1] == 3 * fo[-1] and not entries[offsets[-1]:].any() and len(entries) == 3 * 420
    assert not np.diff(offsets)[vo[-1]:].any()                                           # rows nobody owns: empty lists
    for b in range(4):
        local = faces[fo[b]:fo[b + 1]]
        for i in (0, vo[b + 1] - vo[b] - 1):
            want = 3 * fo[b] + np.flatnonzero(local.reshape(-1) == i)
            r = vo[b] + i
            assert np.array_equal(entries[offsets[r]:offsets[r + 1]], want), (b, i)
    lengths = {n: int(np.diff(evaluated[n][1]["list_offsets"]).max()) for n in ("lane", "wave", "workgroup")}
    assert lengths == {"lane": 12, "wave": 40, "workgroup": 1100}                        # one form of the sum each (32 / 1024)


def test_emulation_against_fp64(evaluated):
    d = 2.0 ** -24
    for name, (_, got, (s64, mags, lengths)) in evaluated.items():
        k = depth(torch.from_numpy(lengths)).numpy().astype(np.float64) + 4
        gamma = k * d / (1 - k * d)
        err = np.abs(got["sums"].astype(np.float64) - s64)
        assert (err <= gamma[:, None] * mags).all(), (name, float((err / np.maximum(gamma[:, None] * mags, 1e-300)).max()))
    assert float(np.abs(evaluated["workgroup"][1]["sums"]).max()) > 0


def test_unit_length_and_zero_normals(evaluated):
    for name, (_, got, _) in evaluated.items():
        s, n = got["sums"], got["normals"]
        m = np.abs(s).max(axis=1)
        has = np.isfinite(m) & (m > 0)
        length = np.sqrt((n.astype(np.float64) ** 2).sum(axis=1))
        assert (np.abs(length[has] - 1) <= 1e-6).all(), name
        assert not n[~has].any() and not np.signbit(n[~has]).any(), name
    assert not evaluated["cancelling"][1]["sums"].any() and not evaluated["cancelling"][1]["normals"].any()      # s = 0 exactly
    assert not evaluated["isolated"][1]["normals"][4].any() and evaluated["isolated"][1]["normals"][:4].any(axis=1).all()
    bad = mr.unit(np.array([[np.inf, 1, 1], [np.nan, 0, 0], [1e38, -np.inf, 0], [0, 0, 0], [3, 0, -4]], np.float32))
    assert not bad[:4].any() and np.array_equal(bad[4], np.array([0.6, 0, -0.8], np.float32))


def test_sphere_normals_point_outward(evaluated):
    for r, s in SPHERES:
        (verts, _, _, _), got, _ = evaluated[f"sphere{r}x{s}"]
        cos = (got["normals"].astype(np.float64) * verts).sum(axis=1) / np.sqrt((verts.astype(np.float64) ** 2).sum(axis=1))
        assert cos.min() > 0.99, (r, s, cos.min())


def test_tetrahedron_is_counter_clockwise(evaluated):
    (verts, faces, _, _), got, _ = evaluated["tetrahedron"]
    centre = verts.astype(np.float64).mean(axis=0)
    assert ((got["normals"] * (verts - centre)).sum(axis=1) > 0).all()
    mid = verts[faces].astype(np.float64).mean(axis=1)
    assert ((got["face_normals"] * (mid - centre)).sum(axis=1) > 0).all()


def test_power_of_two_scaling_keeps_the_bits():
    """The GPU test's mesh for this: no intermediate of the 2^-40 run is subnormal (so the build's denormal mode has no say),
    and the emulation itself keeps every bit."""
    verts, faces, fo, vo = mr.pack([mr.sphere(4, 11)])
    edge, rest = mr.smallest_intermediate(verts, faces, fo, vo)
    assert edge * 2.0 ** -40 >= 2.0 ** -126 and rest * 2.0 ** -80 >= 2.0 ** -126
    base = mr.vertex_normals(verts, faces, fo, vo)["normals"]
    assert base.any(axis=1).all()
    for scale in (2.0 ** -40, 2.0 ** 40):
        assert np.array_equal(mr.vertex_normals(verts * np.float32(scale), faces, fo, vo)["normals"].view(np.uint32), base.view(np.uint32))


# ------------------------------------------------------------------------------------------------------------------ wrapper
def test_host_side_refusals():
    from nsdp_amd import mesh_normals as mn
    from nsdp_amd.ragged import RaggedPoints
    faces, verts = torch.zeros((4, 3), dtype=torch.int32), torch.zeros((5, 3))
    with pytest.raises(mn.MeshNormalsError, match="faces must be a GPU tensor"):
        mn.MeshTopology(faces, verts)
    with pytest.raises(mn.MeshNormalsError, match=r"faces \(4, 2\) with vertices \(5, 3\)"):
        mn.MeshTopology(torch.zeros((4, 2), dtype=torch.int32), verts)
    with pytest.raises(mn.MeshNormalsError, match=r"faces \(2, 4, 3\) with vertices \(3, 5, 3\)"):
        mn.MeshTopology(torch.zeros((2, 4, 3), dtype=torch.int32), torch.zeros((3, 5, 3)))
    with pytest.raises(mn.MeshNormalsError, match="a RaggedPoints each"):
        mn.MeshTopology(faces, RaggedPoints(verts, torch.tensor([0, 5], dtype=torch.int32)))
    with pytest.raises(mn.MeshNormalsError, match="must be a MeshTopology"):
        mn.vertex_normals(verts, faces)
    with pytest.raises(mn.MeshNormalsError, match="1048577 vertex rows outside"):
        mn._sizes(1, (1 << 20) + 1, 10)
    with pytest.raises(mn.MeshNormalsError, match="at most 2\\^25 corners"):
        mn._sizes(1, 10, (1 << 25) // 3 + 1)
    with pytest.raises(mn.MeshNormalsError, match="65536 shapes"):
        mn._sizes(65536, 10, 10)
    with pytest.raises(mn.MeshNormalsError, match="verts must be a GPU tensor"):
        mn.mesh_vertex_normals(torch.zeros((1, 5, 3)), faces, None, None, None, None)
    with pytest.raises(mn.MeshNormalsError, match="faces must be a GPU tensor"):
        mn.mesh_corner_lists(faces, None, None, 5)


# ------------------------------------------------------------------------------------------------------------------ export
@pytest.mark.parametrize("ext", [".ply", ".obj"])
@pytest.mark.parametrize("real", [np.float32, np.float64])
def test_write_mesh_round_trip_with_normals(tmp_path, ext, real):
    verts, faces = mr.tetrahedron()
    normals = mr.vertex_normals(*mr.pack([(verts, faces)]))["normals"]
    verts = verts.astype(real)
    path = str(tmp_path / ("tet" + ext))
    meshio.write_mesh(path, verts, faces, normals=normals)
    v, f = meshio.read_mesh(path)
    assert np.array_equal(v.astype(real), verts) and np.array_equal(f, faces)      # (the text form holds the digits that read back to the type)
    if ext == ".ply":
        raw = open(path, "rb").read()
        head = raw[:raw.index(b"end_header")].decode().split("\n")
        kind = "float" if real == np.float32 else "double"
        assert head[3:9] == [f"property {kind} {a}" for a in ("x", "y", "z", "nx", "ny", "nz")]
        body = np.frombuffer(raw, dtype=np.dtype([(a, "<f4" if real == np.float32 else "<f8") for a in ("x", "y", "z", "nx", "ny", "nz")]),
                             count=4, offset=raw.index(b"end_header") + len(b"end_header\n"))
        assert np.array_equal(np.stack([body["nx"], body["ny"], body["nz"]], axis=1), normals.astype(real))
    else:
        lines = open(path).read().split("\n")
        assert sum(l.startswith("v ") for l in lines) == 4 and sum(l.startswith("vn ") for l in lines) == 4
        assert lines[8] == "f 1//1 2//2 3//3"
        back = np.array([l.split()[1:] for l in lines if l.startswith("vn ")], dtype=np.float64)
        assert np.array_equal(back.astype(np.float32), normals)
    plain = str(tmp_path / ("plain" + ext))
    meshio.write_mesh(plain, verts, faces)
    meshio.write_mesh(str(tmp_path / ("none" + ext)), verts, faces, normals=None)
    assert open(plain, "rb").read() == open(str(tmp_path / ("none" + ext)), "rb").read() and b"nx" not in open(plain, "rb").read()
    with pytest.raises(meshio.MeshError, match="normals must be float"):
        meshio.write_mesh(path, verts, faces, normals=normals[:3])
    meshio.write_mesh(path, verts, faces, colors=np.full((4, 3), 7, np.uint8), normals=normals)      # both at once still read back
    v, f = meshio.read_mesh(path)
    assert np.array_equal(f, faces) and np.array_equal(v.astype(real), verts)


# ------------------------------------------------------------------------------------------------------------------ the tool
def test_edit_tool_takes_normals_and_sizes_its_sphere():
    from nsdp_amd import edit
    args = edit.build_parser().parse_args(["c", "--vertices", "5000", "--normals", "--graph"])
    assert args.normals and not edit.build_parser().parse_args(["c"]).normals
    for n in (8, 300, 5000, 100000):
        v, f = edit.sphere_for(n)
        assert 0.9 * n - 2 <= v.shape[0] <= n and v.dtype == np.float32 and f.shape[0] == 2 * (v.shape[0] - 2) and f.max() == v.shape[0] - 1
    with pytest.raises(SystemExit, match="at least 8 vertices"):
        edit.sphere_for(7)
    with pytest.raises(SystemExit, match="--normals times drags by rule"):
        edit.main(["c", "--handles", "head", "--normals"])
