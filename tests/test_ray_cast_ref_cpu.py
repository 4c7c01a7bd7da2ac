"""CPU: the ray cast without a device (include/nsdp_raycast.h, tests/ray_cast_ref.py).  The emulation the GPU tests hold the
kernel to is itself held to rational arithmetic: its coverage IS the exact coverage of the fp32 sheared corners by the generic
point (e, e^2), on random, degenerate and tied faces, and its t lies within the derived envelope of the exact quotient; the tie
set (a cube and a UV sphere, rays aimed bitwise at vertices, edge midpoints and the centre) crosses an even number of faces from
outside and exactly one from the centre; the boundary of the header: declared there and nowhere else, exported at ABI version
28, built EXACT; the bad-argument table and the refusal order through tools/raycast_host_check.cpp, a stand-alone host
program, with no GPU.

The envelope, derived and not fitted.  With u = 2^-53: U, V, W are exact products and ONE rounded difference
each; every term of T = (U za + V zb) + W zc carries that rounding, its product's and at most two sums' (4 u), det = (U + V) + W
at most three per term (3 u) -- and on a covered face U, V, W have one sign, so det does not cancel and |T*| <= |det*| max|z|;
the quotient rounds once more: |T / det - t*| <= 8 u max|z| = 2^-50 max|z| to first order; fp32(.) adds 2^-24 |t|."""
import ctypes
import os
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import ray_cast_ref as rr
from nsdp_amd import _lib, build as nsdp_build

ENTRY_POINTS = ["nsdp_mesh_ray_cast", "nsdp_mesh_ray_cast_workspace_bytes"]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
# exactly tied edge functions (equal fp64 products) of the emulation over the tie set: (outside, centre) per mesh
TIES = {"cube": (6052, 288), "sphere": (127862, 6176)}


@pytest.fixture(scope="module")
def so():
    if not os.path.exists(_lib.SO_PATH):
        nsdp_build.build()
    lib = ctypes.CDLL(_lib.SO_PATH)
    lib.nsdp_last_error.restype = ctypes.c_char_p
    lib.nsdp_mesh_ray_cast_workspace_bytes.restype = ctypes.c_size_t
    return lib


# ------------------------------------------------------------------------------------------------------------------ the rule
def _faces(kind, rng, n):
    """n faces (n, 3, 3) fp32 around the origin of coordinates: random, or degenerate / tied in the way named."""
    tri = rng.normal(0, 1, (n, 3, 3)).astype(f32)
    if kind == "two_equal":
        tri[:, 2] = tri[:, 1]
    elif kind == "three_equal":
        tri[:, 1] = tri[:, 0]
        tri[:, 2] = tri[:, 0]
    elif kind == "collinear":                     # on a binary grid, so that the midpoint is exactly on the segment
        tri = np.round(tri * 64).astype(f32) / f32(64)
        tri[:, 2] = (tri[:, 0] + tri[:, 1]) * f32(0.5)
    elif kind == "edge_on":                       # the face contains the ray's direction (0, 0, 1): it projects to a segment
        tri = np.round(tri * 64).astype(f32) / f32(64)
        tri[:, 1, :2] = tri[:, 0, :2]
        tri[:, 2, :2] = tri[:, 0, :2] * f32(2)
    elif kind == "through_vertex":                # a corner exactly on the ray
        tri = np.round(tri * 64).astype(f32) / f32(64)
        tri[:, 0, :2] = 0
    elif kind == "through_edge":                  # an edge exactly through the ray: b = -2 a in the projection
        tri = np.round(tri * 64).astype(f32) / f32(64)
        tri[:, 1, :2] = tri[:, 0, :2] * f32(-2)
    return tri


@pytest.mark.parametrize("kind", ["random", "two_equal", "three_equal", "collinear", "edge_on", "through_vertex", "through_edge"])
def test_emulation_equals_rational_arithmetic(kind):
    rng = np.random.default_rng(11)
    n = 400
    tri = _faces(kind, rng, n)
    exact_dir = kind != "random"
    o = np.zeros((n, 3), f32) if exact_dir else rng.normal(0, 0.3, (n, 3)).astype(f32)
    d = np.tile(f32([0, 0, 1]), (n, 1)) if exact_dir else rng.normal(0, 1, (n, 3)).astype(f32)
    fr = rr.frame(o, d)
    r = rr.face_tests(fr, tri[:, None, 0], tri[:, None, 1], tri[:, None, 2])
    (ax, ay, az), (bx, by, bz), (cx, cy, cz) = r["xyz"]
    covered, hits, decided = 0, 0, 0
    for i in range(n):
        inside, tstar, zmax = rr.exact_face(((ax[i, 0], ay[i, 0], az[i, 0]), (bx[i, 0], by[i, 0], bz[i, 0]), (cx[i, 0], cy[i, 0], cz[i, 0])))
        assert bool(r["covered"][i, 0]) == inside, (kind, i)
        if not inside:
            assert not r["hit"][i, 0]
            continue
        covered += 1
        assert tstar is not None                                        # (a covered face has det != 0)
        if abs(tstar) > rr.T_ABS * zmax:                                # beyond the fp64 part of the envelope the sign is decided
            decided += 1
            assert bool(r["hit"][i, 0]) == (tstar > 0), (kind, i)
        if r["hit"][i, 0]:
            hits += 1
            t = Fraction(float(r["t"][i, 0]))
            assert abs(t - tstar) <= rr.t_bound(tstar, zmax), (kind, i, float(t), float(tstar))
            bary = r["bary"][i, 0].astype(np.float64)
            assert (bary >= 0).all() and abs(bary.sum() - 1) <= 4 * 2.0 ** -24
    print(kind, "covered", covered, "hit", hits, "decided", decided, "ties", r["ties"])
    if kind in ("two_equal", "three_equal", "collinear", "edge_on"):
        assert covered == 0                                             # zero projected area: never covered
    else:
        assert covered > 30 and hits > 10
    if kind in ("through_vertex", "through_edge", "edge_on", "three_equal"):
        assert r["ties"] >= n


def test_edge_sign_is_antisymmetric_on_all_pairs():
    rng = np.random.default_rng(2)
    p = np.round(rng.normal(0, 1, (60, 2)) * 4).astype(f32) / f32(4)      # a coarse grid: many exact ties, repeated points, zeros
    p[:6] = 0
    p[6:12, 0] = 0
    p[12:18] = p[18:24] * f32(2)
    I, J = [a.reshape(-1) for a in np.meshgrid(np.arange(60), np.arange(60), indexing="ij")]
    s, l, r = rr.edge_sign(p[I, 0], p[I, 1], p[J, 0], p[J, 1])
    back, _, _ = rr.edge_sign(p[J, 0], p[J, 1], p[I, 0], p[I, 1])
    assert np.array_equal(s, -back)
    same = (p[I] == p[J]).all(1)
    assert (s[same] == 0).all() and (s[~same] != 0).all()                 # 0 only for equal points
    assert (l == r).sum() > 500                                           # the tie-break was at work


@pytest.fixture(scope="module")
def tie_results():
    out = {}
    for name, (v, f) in {"cube": rr.cube(), "sphere": rr.uv_sphere(grid=4096)}.items():
        oo, do, oi, di = rr.tie_set(v, f)
        out[name] = (v, f, oo, do, rr.cast(oo, do, v, f), rr.cast(oi, di, v, f))
    return out


@pytest.mark.parametrize("name", ["cube", "sphere"])
def test_tie_set_counts(tie_results, name):
    v, f, oo, do, outside, centre = tie_results[name]
    assert rr.open_edges(f) == 0 and len(f) == {"cube": 12, "sphere": 216}[name]
    if name == "cube":
        assert rr.is_convex(v, f)
    t, face, bary, count, covered, ties = outside
    print(name, "outside rays", len(oo), "ties", ties, "counts", np.unique(count, return_counts=True))
    assert (covered % 2 == 0).all()                                       # closed mesh: exact parity for every ray
    assert np.isin(count, (0, 2)).all() and (count == 2).sum() > len(oo) // 2
    assert ((face >= 0) == (count > 0)).all() and (t[count > 0] > 0).all() and (t[count == 0] == rr.FLT_MAX).all()
    tc, fc, bc, cc, covc, tiesc = centre
    assert (cc == 1).all() and (covc == 2).all() and (fc >= 0).all()
    assert (ties, tiesc) == TIES[name]


def test_tie_set_holds_ten_thousand_tied_edge_functions(tie_results):
    total = sum(tie_results[n][4][5] + tie_results[n][5][5] for n in tie_results)
    assert total == sum(a + b for a, b in TIES.values()) == 140378 and total >= 10000
    assert sum(len(tie_results[n][2]) for n in tie_results) == 11040       # rays from outside


def test_cube_ray_through_a_corner_leaves_once(tie_results):
    v, f = rr.cube()
    t, face, bary, count, covered, _ = rr.cast(np.zeros((1, 3), f32), f32([[1, 1, 1]]), v, f)
    assert count[0] == 1 and covered[0] == 2 and t[0] == 1 and face[0] >= 0
    assert np.array_equal(np.sort(bary[0]), f32([0, 0, 1]))


def test_zero_direction_misses_everything():
    v, f = rr.cube()
    o = f32([[0, 0, 0], [0.25, 0.5, -0.125], [3, 0, 0]])
    t, face, bary, count, covered, ties = rr.cast(o, np.zeros((3, 3), f32), v, f)
    assert (count == 0).all() and (face == -1).all() and (t == rr.FLT_MAX).all() and (bary == 0).all() and ties == 0
    t, face, bary, count, _, _ = rr.cast(o, np.tile(f32([0, 0, 2]), (3, 1)), v, f)
    assert count.tolist() == [1, 1, 0] and t[0] == f32(0.5) and t[1] == f32(0.5625)      # t is in units of d


def test_smallest_row_wins_among_equal_t():
    """The cube's top face is two triangles; a ray through their shared diagonal is covered by exactly one of them, and two
    copies of the mesh give equal t bits: the smaller row is reported."""
    v, f = rr.cube()
    t, face, bary, count, _, _ = rr.cast(f32([[0, 0, 0]]), f32([[0, 0, 1]]), v, np.concatenate([f, f]))
    assert count[0] == 2 and face[0] < 12 and t[0] == 1
    t2, face2, _, count2, _, _ = rr.cast(f32([[0, 0, 0]]), f32([[0, 0, 1]]), v, np.concatenate([f, f]), row0=100)
    assert face2[0] == face[0] + 100


def test_packed_emulation_clamps():
    v, f = rr.cube()
    verts = np.concatenate([v, np.zeros((0, 3), f32), v + f32(4), np.full((2, 3), np.nan, f32)])
    faces = np.concatenate([f, f, f, np.full((3, 3), -1)])                 # the second mesh has faces but no vertices
    o = np.zeros((7, 3), f32)
    o[3:5] = 4
    d = np.tile(f32([0, 0, 1]), (7, 1))
    t, face, bary, count = rr.ray_cast(o, d, [0, 2, 3, 5], verts, [0, 8, 8, 16], faces, [0, 12, 24, 36])
    assert count[:5].tolist() == [1, 1, 0, 1, 1] and face[2] == -1 and (face[3:5] >= 24).all() and (face[:2] < 12).all()
    assert np.isnan(t[5:]).all() and (face[5:] == -9).all() and (count[5:] == -9).all()      # rows beyond the last offset: not written


# ------------------------------------------------------------------------------------------------------------------ boundary
def test_envelopes_are_the_headers_and_the_designs():
    header = open(os.path.join(ROOT, "include", "nsdp_raycast.h")).read()
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert rr.T_REL == Fraction(1, 2 ** 24) and rr.T_ABS == Fraction(1, 2 ** 50) and (rr.SHEAR_XY, rr.SHEAR_Z) == (6, 3)
    for text in (header, design):
        assert "|t - t*| <= 2^-24 |t*| + 2^-50 max(|za|, |zb|, |zc|)" in text
        assert "6 * 2^-24 * R" in text and "3 * 2^-24 * |z*|" in text


def test_header_declares_and_library_exports_the_entries(so):
    assert _lib.declared_symbols("nsdp_raycast.h") == sorted(ENTRY_POINTS)
    for other in (None, "nsdp_batch.h", "nsdp_meshbatch.h", "nsdp_meshwhole.h", "nsdp_scatter.h", "nsdp_optim.h", "nsdp_meshnormals.h",
                  "nsdp_surface.h", "nsdp_selfintersect.h"):
        assert not set(ENTRY_POINTS) & set(_lib.declared_symbols(other)), other
    for name in ENTRY_POINTS:
        assert hasattr(so, name), name
    assert so.nsdp_abi_version() >= 28
    assert "nsdp_raycast.h" in open(nsdp_build.__file__).read() and nsdp_build.PER_FILE["ray_cast.hip"] == nsdp_build.EXACT
    assert 'declared_symbols("nsdp_raycast.h")' in open(os.path.join(ROOT, "__graft_entry__.py")).read()


def test_shared_blocks_header_is_used_by_both_scans():
    """One definition of the blocks, their boxes and the clamps: surface_distance.hip and ray_cast.hip include it, neither
    keeps a copy."""
    csrc = os.path.join(ROOT, "nsdp_amd", "csrc")
    shared = open(os.path.join(csrc, "mesh_blocks.h")).read()
    for name in ("boxes_kernel", "mesh_of", "struct Mesh", "corner(", "wave_min", "wave_max"):
        assert name in shared, name
    for src in ("surface_distance.hip", "ray_cast.hip"):
        text = open(os.path.join(csrc, src)).read()
        assert '#include "mesh_blocks.h"' in text
        assert "void boxes_kernel" not in text and "struct Mesh" not in text and "Mesh mesh_of" not in text, src


def test_workspace_query(so):
    size = so.nsdp_mesh_ray_cast_workspace_bytes
    for B, qcap, fcap in ((1, 1, 1), (3, 1, 129), (2, 10, 12), (4, 400000, 800000), (1, 1 << 20, 1 << 20), (65535, 65535, 65535)):
        assert size(B, qcap, fcap) == 12 * qcap + 24 * (fcap // 64 + B + 1), (B, qcap, fcap)
    for B, qcap, fcap in ((0, 1, 1), (65536, 1, 1), (-1, 1, 1), (1, 0, 1), (1, 1, 0), (1, (1 << 20) + 1, 1), (1, 1, (1 << 20) + 1),
                          (2, 1, (2 << 20) + 1)):
        assert size(B, qcap, fcap) == 0, (B, qcap, fcap)


def test_bad_argument_table_and_refusal_order_through_the_stand_alone_host_program(so, tmp_path):
    """tools/raycast_host_check.cpp, linked against the built library: sizes before flags before pointers before the
    alignment; no GPU is touched, nothing is launched."""
    exe = str(tmp_path / "raycast_host_check")
    libdir = os.path.dirname(_lib.SO_PATH)
    subprocess.check_call([nsdp_build.HIPCC, "-x", "c++", "-std=c++17", os.path.join(ROOT, "tools", "raycast_host_check.cpp"),
                           "-L" + libdir, "-lnsdp_hip", "-Wl,-rpath," + libdir, "-o", exe])
    done = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert done.returncode == 0 and done.stdout.strip() == "ok", done.stderr


# ------------------------------------------------------------------------------------------------------------------ python
def test_wrapper_refuses_by_name_without_a_device(monkeypatch):
    import torch
    from nsdp_amd import ray_cast as rc
    with pytest.raises(rc.RayCastError, match="GPU tensor"):
        rc.RayCastPlan(torch.zeros(4, 3, dtype=torch.int32), torch.zeros(5, 3))
    with pytest.raises(rc.RayCastError, match="RayCastPlan"):
        rc.cast_rays(torch.zeros(5, 3), torch.zeros(5, 3), torch.zeros(5, 3), object())
    with pytest.raises(rc.RayCastError, match="GPU tensor"):
        rc.mesh_ray_cast(torch.zeros(5, 3), torch.zeros(5, 3), None, torch.zeros(5, 3), None, torch.zeros(4, 3, dtype=torch.int32), None)
    monkeypatch.setenv("NSDP_RAYCAST_CULL", "0")
    assert rc._cull_default() is False
    monkeypatch.setenv("NSDP_RAYCAST_CULL", "1")
    assert rc._cull_default() is True
    monkeypatch.setenv("NSDP_RAYCAST_CULL", "2")
    with pytest.raises(rc.RayCastError, match="NSDP_RAYCAST_CULL"):
        rc._cull_default()
    monkeypatch.delenv("NSDP_RAYCAST_CULL")
    assert rc._cull_default() is None and rc.AUTO_MIN_TESTS & (rc.AUTO_MIN_TESTS - 1) == 0
    assert "NSDP_RAYCAST_CULL" in open(os.path.join(ROOT, "docs", "KNOBS.md")).read()


def test_edit_tool_takes_the_flag():
    from nsdp_amd import edit
    args = edit.build_parser().parse_args(["c", "--vertices", "5000", "--pick", "0,0,2,0,0,-1", "--graph"])
    assert edit.pick_from_args(args) == [0.0, 0.0, 2.0, 0.0, 0.0, -1.0] and edit.pick_from_args(edit.build_parser().parse_args(["c"])) is None
    with pytest.raises(SystemExit, match="--pick wants six numbers"):
        edit.main(["c", "--pick", "0,0,2"])
    with pytest.raises(SystemExit, match="--pick goes with drags by rule"):
        edit.main(["c", "--handles", "head", "--pick", "0,0,2,0,0,-1"])
    with pytest.raises(SystemExit, match="--pick goes with --vertices"):
        edit.main(["c", "--vertex-counts", "100,200", "--pick", "0,0,2,0,0,-1"])


def test_evaluate_refuses_a_negative_sample_count_and_seeds_by_step():
    from nsdp_amd import evaluate
    assert "test.volume_iou" in evaluate.__doc__
    a, b = evaluate.iou_generator("cpu", 6, 0), evaluate.iou_generator("cpu", 6, 1)
    assert a.initial_seed() != b.initial_seed() and a.initial_seed() == evaluate.iou_generator("cpu", 6, 0).initial_seed()
