"""CPU: the rasteriser without a device (include/nsdp_raster.h, tests/raster_ref.py).  The emulation the GPU tests hold the
kernel to is itself held to rational arithmetic: its coverage IS the exact coverage of the snapped corners by the centre
displaced by (e, e^2), on random, degenerate and tied faces, and its depth lies within the derived envelope of the exact
perspective-correct value; closed meshes under cameras that put pixel centres bitwise on vertices and along edges cover every
pixel an even number of times; the boundary of the header: declared there and nowhere else, exported at ABI version 30, built
EXACT; the bad-argument table through tools/raster_host_check.cpp, a stand-alone host program, with no GPU; the error colours
against the fixture recorded from the reference's scalar rule; the PNG writer against zlib.

The envelope, derived and not fitted.  With u = 2^-53: iw = fl(1 / W) and t = fl(e iw) carry two roundings (e
is exact); every term of the numerator (ta Za + tb Zb) + tc Zc carries those two, its product's and at most two sums' (5 u), s =
(ta + tb) + tc the two and at most two sums' per term (4 u) -- all t > 0 or 0, so s does not cancel and |numerator*| <= s*
max|Z|; the quotient rounds once more: 10 u max|Z| to first order, 11 u with every second-order term; fp32(.) adds 2^-24 |d|."""
import ctypes
import os
import struct
import subprocess
import zlib
from fractions import Fraction

import numpy as np
import pytest

import raster_ref as ra
from nsdp_amd import _lib, build as nsdp_build

ENTRY_POINTS = ["nsdp_mesh_rasterize", "nsdp_mesh_rasterize_workspace_bytes"]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
# exactly zero edge functions at pixel centres the emulation meets on the tie set, per (mesh, camera)
TIES = {("cube", "ortho"): 9636, ("cube", "pinhole"): 1012, ("sphere", "ortho"): 3984}


@pytest.fixture(scope="module")
def so():
    if not os.path.exists(_lib.SO_PATH):
        nsdp_build.build()
    lib = ctypes.CDLL(_lib.SO_PATH)
    lib.nsdp_last_error.restype = ctypes.c_char_p
    lib.nsdp_mesh_rasterize_workspace_bytes.restype = ctypes.c_size_t
    return lib


# ------------------------------------------------------------------------------------------------------------------ the rule
def _faces(kind, rng, n):
    """n faces (n, 3, 3) fp32 in front of the pinhole of `_camera`: random, or degenerate / tied in the way named."""
    tri = rng.uniform(-1, 1, (n, 3, 3)).astype(f32)
    if kind == "two_equal":
        tri[:, 2] = tri[:, 1]
    elif kind == "three_equal":
        tri[:, 1] = tri[:, 0]
        tri[:, 2] = tri[:, 0]
    elif kind in ("collinear", "on_centres", "edge_through_centre"):
        # vertices bitwise on pixel centres of the orthographic camera: px = 4 x + 4.5 is a centre where 4 x is an integer
        tri = (np.round(tri * 4) / 4).astype(f32)
        if kind == "collinear":
            tri[:, 2, :2] = (tri[:, 0, :2] + tri[:, 1, :2]) * f32(0.5)
        elif kind == "edge_through_centre":
            tri[:, 1, :2] = -tri[:, 0, :2]                # the edge a b passes through the centre of pixel (4, 4)
    return tri


def _camera(kind):
    return ra.pinhole(12.0, 4.25, 3.75, 3.0) if kind == "random" else ra.ortho(4.0, 4.5, 4.5, 2.0)


@pytest.mark.parametrize("kind", ["random", "two_equal", "three_equal", "collinear", "on_centres", "edge_through_centre"])
def test_emulation_equals_rational_arithmetic(kind):
    rng = np.random.default_rng(17)
    n, H, W = 40, 9, 9
    tri, M = _faces(kind, rng, n), _camera(kind)
    covered = ties = fronts = 0
    for i in range(n):
        both = ra.image(tri[i], [[0, 1, 2]], M, H, W)
        front = ra.image(tri[i], [[0, 1, 2]], M, H, W, front=True)
        c = ra.corners(tri[i], M)
        assert c["ok"].all() and both["dropped"] == 0
        P = [(c["sx"][k], c["sy"][k], c["Z"][k], c["W"][k]) for k in range(3)]
        ties += both["ties"]
        for y in range(H):
            for x in range(W):
                inside, side, dstar, zmax = ra.exact_pixel(P[0], P[1], P[2], 256 * x + 128, 256 * y + 128)
                assert bool(both["count"][y, x]) == inside, (kind, i, y, x)
                assert bool(front["count"][y, x]) == (inside and side > 0), (kind, i, y, x)
                if not inside:
                    assert both["face"][y, x] == -1 and both["depth"][y, x] == ra.FLT_MAX and (both["bary"][y, x] == 0).all()
                    continue
                covered += 1
                fronts += int(front["count"][y, x])
                d = Fraction(float(both["depth"][y, x]))
                assert abs(d - dstar) <= ra.d_bound(dstar, zmax), (kind, i, y, x, float(d), float(dstar))
                bary = both["bary"][y, x].astype(np.float64)
                assert (bary >= 0).all() and abs(bary.sum() - 1) <= 4 * 2.0 ** -24
    print(kind, "covered", covered, "front", fronts, "ties", ties)
    if kind in ("two_equal", "three_equal", "collinear"):
        assert covered == 0                                             # zero snapped area: never covered, not dropped
    else:
        assert covered > 100 and 0 < fronts < covered
    if kind in ("collinear", "on_centres", "edge_through_centre"):
        assert ties >= n


def test_edge_sign_is_antisymmetric_and_zero_only_for_equal_points():
    rng = np.random.default_rng(2)
    p = (np.round(rng.normal(0, 2, (60, 2))) * 256 + 128).astype(np.int64)      # on pixel centres: many exact ties
    p[:6] = 128
    I, J = [a.reshape(-1) for a in np.meshgrid(np.arange(60), np.arange(60), indexing="ij")]
    for cx, cy in ((128, 128), (384, -128)):
        E, s = ra.edge(p[I, 0], p[I, 1], p[J, 0], p[J, 1], np.int64(cx), np.int64(cy))
        _, back = ra.edge(p[J, 0], p[J, 1], p[I, 0], p[I, 1], np.int64(cx), np.int64(cy))
        assert np.array_equal(s, -back)
        same = (p[I] == p[J]).all(1)
        assert (s[same] == 0).all() and (s[~same] != 0).all()
        assert (E == 0).sum() > 300                                       # the tie-break was at work


def _tie_case(name, cam):
    v, f = ra.cube() if name == "cube" else ra.uv_sphere(grid=4096)
    if cam == "ortho":                # vertices and axis-aligned edges bitwise on pixel centres
        M, H, W = (ra.ortho(8, 16.5, 16.5, 4), 33, 33) if name == "cube" else (ra.ortho(16, 24.5, 24.5, 2), 49, 49)
    else:                             # W = 2 and 4 at the cube's corners: +-8 and +-4 pixels off the principal point, on centres
        M, H, W = ra.pinhole(16, 16.5, 16.5, 3), 33, 33
    return v, f, M, H, W


@pytest.mark.parametrize("name,cam", sorted(TIES))
def test_closed_meshes_cover_every_pixel_an_even_number_of_times(name, cam):
    v, f, M, H, W = _tie_case(name, cam)
    assert ra.open_edges(f) == 0
    r = ra.image(v, f, M, H, W)
    print(name, cam, "ties", r["ties"], "counts", np.unique(r["count"], return_counts=True))
    assert r["dropped"] == 0 and (r["count"] % 2 == 0).all() and np.isin(r["count"], (0, 2)).all()
    assert (r["count"] == 2).sum() > H * W // 5
    assert ((r["face"] >= 0) == (r["count"] > 0)).all()
    front = ra.image(v, f, M, H, W, front=True)
    assert np.array_equal(front["count"] * 2, r["count"])                 # one facing each way, ties included
    assert np.array_equal(front["depth"], r["depth"])                     # the near one faces the viewer
    apart = r["second"] != r["depth"]                                     # (on the silhouette both have one depth: the smaller row wins)
    assert np.array_equal(front["face"][apart], r["face"][apart]) and apart.sum() > 0.8 * (r["count"] > 0).sum()
    assert r["ties"] == TIES[(name, cam)]


def test_smallest_row_wins_among_equal_depths_and_rows_are_packed():
    v, f = ra.cube()
    M = ra.ortho(8, 16.5, 16.5, 4)
    one, two = ra.image(v, f, M, 33, 33), ra.image(v, np.concatenate([f, f]), M, 33, 33, row0=100)
    assert np.array_equal(two["count"], 2 * one["count"]) and np.array_equal(two["depth"], one["depth"])
    assert np.array_equal(two["face"][one["face"] >= 0], one["face"][one["face"] >= 0] + 100)
    assert np.array_equal(two["second"][one["face"] >= 0], one["depth"][one["face"] >= 0])      # the twin is the runner-up


def test_dropped_faces_cover_nothing_and_are_counted():
    v, f = ra.cube()
    r = ra.image(v, f, ra.pinhole(16, 16.5, 16.5, 0.5), 33, 33)          # the eye inside the cube: W = -0.5 on the near corners
    assert r["dropped"] == 10 and r["count"].max() == 1 and (r["count"] == 1).sum() > 100 and (r["depth"][r["face"] >= 0] == f32(1.5)).all()
    big = ra.image(v * f32(3e4), f, ra.ortho(8, 16.5, 16.5, 4), 33, 33)   # |sx| = 256 * 240 000 > 2^24
    assert big["dropped"] == 12 and (big["face"] == -1).all()
    nan = v.copy()
    nan[0, 1] = np.nan
    assert ra.image(nan, f, ra.ortho(8, 16.5, 16.5, 4), 33, 33)["dropped"] == int((f == 0).any(axis=1).sum())


def test_packed_emulation_clamps():
    v, f = ra.cube()
    verts = np.concatenate([v, v + f32(0.25), np.full((2, 3), np.nan, f32)])
    faces = np.concatenate([f, f, f, np.full((3, 3), -1)])                 # the second mesh has faces but no vertices
    cams = np.stack([ra.ortho(8, 16.5, 16.5, 4)] * 4)
    r = ra.rasterize(verts, [0, 8, 8, 16], faces, [0, 12, 24, 36], cams, [0, 1, 2, 7], 33, 33)
    assert (r["face"][1] == -1).all() and r["dropped"].tolist() == [0, 0, 0, 0]
    assert (r["face"][0][r["face"][0] >= 0] < 12).all() and (r["face"][2][r["face"][2] >= 0] >= 24).all()
    assert np.array_equal(r["face"][3], r["face"][2])                      # image_shape is clamped into 0 .. B-1


def test_cross_check_case_leaves_few_pixels_undecided():
    """The mesh of the GPU cross-check with the ray cast: the emulation alone leaves at most 2 % of the covered pixels out of the
    face comparison (a runner-up within 2^-20 relative of the winner), and the case does meet exact ties."""
    v, f, M, H, W = ra.cross_check_case()
    r = ra.image(v, f, M, H, W)
    covered = r["face"] >= 0
    close = covered & ~(np.abs(r["second"].astype(np.float64) - r["depth"]) > 2.0 ** -20 * np.abs(r["depth"]))
    print("covered", covered.sum(), "left out", close.sum(), "ties", r["ties"])
    assert covered.sum() > 700 and close.sum() <= 0.02 * covered.sum() and r["ties"] > 1000 and r["dropped"] == 0


# ------------------------------------------------------------------------------------------------------------------ boundary
def test_envelope_is_the_headers_and_the_designs():
    header = open(os.path.join(ROOT, "include", "nsdp_raster.h")).read()
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert ra.D_REL == Fraction(1, 2 ** 24) and ra.D_ABS == Fraction(11, 2 ** 53)
    for text in (header, design):
        assert "|depth - d*| <= 2^-24 |d*| + 11 * 2^-53 max(|Za|, |Zb|, |Zc|)" in text
        assert "NO NEAR-PLANE CLIPPING" in text


def test_header_declares_and_library_exports_the_entries(so):
    assert _lib.declared_symbols("nsdp_raster.h") == sorted(ENTRY_POINTS)
    for other in (None, "nsdp_batch.h", "nsdp_meshbatch.h", "nsdp_meshwhole.h", "nsdp_scatter.h", "nsdp_optim.h", "nsdp_meshnormals.h",
                  "nsdp_surface.h", "nsdp_selfintersect.h", "nsdp_raycast.h", "nsdp_geodesic.h"):
        assert not set(ENTRY_POINTS) & set(_lib.declared_symbols(other)), other
    for name in ENTRY_POINTS:
        assert hasattr(so, name), name
    assert so.nsdp_abi_version() >= 30
    assert "nsdp_raster.h" in open(nsdp_build.__file__).read() and nsdp_build.PER_FILE["rasterize.hip"] == nsdp_build.EXACT
    assert 'declared_symbols("nsdp_raster.h")' in open(os.path.join(ROOT, "__graft_entry__.py")).read()
    assert os.path.samefile(_lib.RASTER_HEADER_PATH, os.path.join(ROOT, "include", "nsdp_raster.h"))


def test_kernel_uses_the_shared_blocks_header():
    text = open(os.path.join(ROOT, "nsdp_amd", "csrc", "rasterize.hip")).read()
    assert '#include "mesh_blocks.h"' in text and "struct Mesh" not in text and "Mesh mesh_of" not in text
    assert "atomic" not in text.replace("no atomics", "").replace("No atomics", "").replace("no\n// atomics", "")


def test_workspace_query(so):
    size = so.nsdp_mesh_rasterize_workspace_bytes
    for B, I, fcap in ((1, 1, 1), (3, 5, 129), (2, 3, 12), (4, 4, 800000), (1, 65535, 1 << 20), (65535, 65535, 65535)):
        assert size(B, I, fcap) == 20 * I * (fcap // 64 + B + 1), (B, I, fcap)
    for B, I, fcap in ((0, 1, 1), (65536, 1, 1), (-1, 1, 1), (1, 0, 1), (1, 65536, 1), (1, 1, 0), (1, 1, (1 << 20) + 1), (2, 1, (2 << 20) + 1)):
        assert size(B, I, fcap) == 0, (B, I, fcap)


def test_bad_argument_table_and_refusal_order_through_the_stand_alone_host_program(so, tmp_path):
    """tools/raster_host_check.cpp, linked against the built library: sizes before flags before pointers before the alignment;
    no GPU is touched, nothing is launched."""
    exe = str(tmp_path / "raster_host_check")
    libdir = os.path.dirname(_lib.SO_PATH)
    subprocess.check_call([nsdp_build.HIPCC, "-x", "c++", "-std=c++17", os.path.join(ROOT, "tools", "raster_host_check.cpp"),
                           "-L" + libdir, "-lnsdp_hip", "-Wl,-rpath," + libdir, "-o", exe])
    done = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert done.returncode == 0 and done.stdout.strip() == "ok", done.stderr


# ------------------------------------------------------------------------------------------------------------------ python
def test_error_colors_equal_the_recorded_reference_rule():
    import torch
    from nsdp_amd import rasterize as rz
    g = np.load(os.path.join(ROOT, "tests", "golden", "error_colors.npz"))
    err = torch.from_numpy(g["err"])
    for got, want in ((rz.error_colors(err, vmax=float(g["vmax"])), g["colors"]), (rz.error_colors(err, use_max=True), g["colors_use_max"])):
        assert got.dtype == torch.float32 and tuple(got.shape) == (len(err), 3)
        assert np.abs(got.numpy().astype(np.float64) - want).max() <= 2.0 ** -22
        x = want.astype(np.float64) * 255
        assert (np.abs(x - np.floor(x) - 0.5) > 1e-3).all()                # no fixture colour sits on a rounding boundary
        assert np.array_equal(rz.to_uint8(got).numpy(), np.round(x).astype(np.uint8))
    assert (g["err"] < 0).any() and (g["err"] > 0.2).any() and len(np.unique(g["colors"], axis=0)) > 40
    assert rz.error_colors(torch.zeros(2, 5)).shape == (2, 5, 3)


def _decode_png(path):
    raw = open(path, "rb").read()
    assert raw[:8] == b"\x89PNG\r\n\x1a\n"
    pos, chunks = 8, []
    while pos < len(raw):
        n, kind = struct.unpack(">I4s", raw[pos:pos + 8])
        data = raw[pos + 8:pos + 8 + n]
        assert struct.unpack(">I", raw[pos + 8 + n:pos + 12 + n])[0] == zlib.crc32(kind + data) & 0xFFFFFFFF
        chunks.append((kind, data))
        pos += 12 + n
    assert [k for k, _ in chunks] == [b"IHDR", b"IDAT", b"IEND"]
    w, h, depth, colour, comp, filt, lace = struct.unpack(">IIBBBBB", chunks[0][1])
    assert (depth, comp, filt, lace) == (8, 0, 0, 0) and colour in (0, 2)
    c = 3 if colour == 2 else 1
    rows = np.frombuffer(zlib.decompress(chunks[1][1]), np.uint8).reshape(h, 1 + w * c)
    assert (rows[:, 0] == 0).all()                                         # filter 0 on every row
    return rows[:, 1:].reshape((h, w, 3) if c == 3 else (h, w))


def test_write_png_round_trips_through_zlib(tmp_path):
    import torch
    from nsdp_amd import rasterize as rz
    rng = np.random.default_rng(3)
    for shape in ((5, 7, 3), (1, 1, 3), (33, 17)):
        img = rng.integers(0, 256, shape).astype(np.uint8)
        path = str(tmp_path / ("x".join(map(str, shape)) + ".png"))
        rz.write_png(path, torch.from_numpy(img) if len(shape) == 3 else img)
        assert np.array_equal(_decode_png(path), img)
    for bad in (np.zeros((4, 4, 4), np.uint8), np.zeros((4, 4), np.float32), np.zeros((0, 4), np.uint8)):
        with pytest.raises(rz.RasterError, match="write_png"):
            rz.write_png(str(tmp_path / "bad.png"), bad)


def test_cameras_put_the_target_in_the_middle_and_depth_is_metric():
    from nsdp_amd.rasterize import Camera, RasterError
    eye, target = np.array([3.0, 2.0, -4.0]), np.array([0.25, -0.5, 0.5])
    for cam in (Camera.look_at(eye, target, (0, 1, 0), 40, 64, 48), Camera.orthographic(eye, target, (0, 1, 0), 3.0, 64, 48)):
        assert cam.matrix.dtype == np.float32 and cam.matrix.shape == (4, 4)
        X, Y, Z, W = cam.matrix.astype(np.float64) @ np.append(target, 1.0)
        assert abs(X / W - 32) < 1e-4 and abs(Y / W - 24) < 1e-4 and abs(Z - np.linalg.norm(target - eye)) < 1e-5
        X2, Y2, _, W2 = cam.matrix.astype(np.float64) @ np.append(target + [0, 0.1, 0], 1.0)
        assert Y2 / W2 < Y / W                                             # up in the world is up in the image: rows run down
    # an outward (counter-clockwise) face seen from outside keeps all three edge signs +1: front_only keeps the near side
    v, f = ra.cube()
    cam = Camera.look_at((3, 2, -4), (0, 0, 0), (0, 1, 0), 40, 48, 32)
    front, both = ra.image(v, f, cam.matrix, 32, 48, front=True), ra.image(v, f, cam.matrix, 32, 48)
    assert np.array_equal(front["depth"], both["depth"]) and front["count"].max() == 1 and both["count"].max() == 2
    with pytest.raises(RasterError, match="parallel"):
        Camera.look_at((0, 0, 0), (0, 1, 0), (0, 2, 0), 40, 8, 8)
    with pytest.raises(RasterError, match="fov_deg"):
        Camera.look_at((0, 0, 0), (0, 0, 1), (0, 1, 0), 180, 8, 8)


def test_wrapper_refuses_by_name_without_a_device():
    import torch
    from nsdp_amd import rasterize as rz
    with pytest.raises(rz.RasterError, match="GPU tensor"):
        rz.RasterPlan(torch.zeros(4, 3, dtype=torch.int32), torch.zeros(5, 3))
    with pytest.raises(rz.RasterError, match="RasterPlan"):
        rz.rasterize(torch.zeros(5, 3), object(), torch.zeros(1, 4, 4), 8, 8)
    with pytest.raises(rz.RasterError, match="GPU tensor"):
        rz.mesh_rasterize(torch.zeros(5, 3), None, None, None, None, None, 8, 8)
    assert "NO NEAR-PLANE CLIPPING" in rz.__doc__ and "no near-plane clipping" in rz.rasterize.__doc__


def test_edit_tool_and_evaluate_take_the_keys():
    from nsdp_amd import edit, evaluate
    args = edit.build_parser().parse_args(["c", "--vertices", "300", "--render", "o.png", "--render-size", "64", "--graph"])
    assert args.render == "o.png" and args.render_size == 64 and edit.build_parser().parse_args(["c"]).render is None
    with pytest.raises(SystemExit, match="--render goes with drags by rule"):
        edit.main(["c", "--handles", "head", "--render", "o.png"])
    with pytest.raises(SystemExit, match="--render goes with --vertices"):
        edit.main(["c", "--vertex-counts", "100,200", "--render", "o.png"])
    with pytest.raises(SystemExit, match="--render-size wants 1 .. 4096"):
        edit.main(["c", "--render", "o.png", "--render-size", "0"])
    spec = edit.RenderSpec(None, 8, 9)
    assert (spec.height, spec.width, spec.shade, spec.count, spec.tensor) == (8, 9, True, False, None)
    assert evaluate.render_settings({}) == (0, 0) and evaluate.render_settings({"render": {"views": 3, "size": 128}}) == (3, 128)
    assert len(evaluate.VIEW_DIRECTIONS) == 6 and "test.render" in evaluate.__doc__
    with pytest.raises(evaluate.EvaluateError, match="test.render"):
        evaluate.render_settings({"render": {"views": 7}})
