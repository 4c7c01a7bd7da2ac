"""CPU: geodesic distances without a device (include/nsdp_geodesic.h, tests/geodesic_ref.py).  The emulation the GPU tests hold
the kernels to is held to itself: the heap Dijkstra satisfies the fixed-point equation at every vertex; a block-local schedule in
numpy -- the kernel's shape -- reaches the same bits at two block sizes and on a shuffled numbering; renumbering the vertices
keeps the bits; on an integer grid the distances along the seed's row and column are exactly the integers; and the fp32
distances lie within the derived envelope of an fp64 Dijkstra over fp64 lengths of the same coordinates.

The envelope, derived and not fitted: an edge length carries at most 3.5 half-ulps to first order (a difference,
a square, two sums, a root: the difference and the square count twice under the root's halving, the root once); every further
sum of a path adds one, the first sum (with a start value of 0) is exact: (H + 2.5) 2^-24 relative for a path of H hops, and
|d - d*| <= (H + 4) 2^-24 d* leaves the second order, H the larger hop count of the two shortest-path trees.

The boundary of the header: declared there and nowhere else, exported at ABI version 29, built EXACT; the bad-argument table and
the refusal order through ctypes and through tools/geodesic_host_check.cpp, a stand-alone host program, with no GPU."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import geodesic_ref as gr
import mesh_normals_ref as mr
from nsdp_amd import _lib, build as nsdp_build

ENTRY_POINTS = ["nsdp_mesh_edge_lengths", "nsdp_mesh_edge_table_entries", "nsdp_mesh_geodesic_block", "nsdp_mesh_geodesic_relax"]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
_ci, _vp, _cf = ctypes.c_int, ctypes.c_void_p, ctypes.c_float


@pytest.fixture(scope="module")
def so():
    if not os.path.exists(_lib.SO_PATH):
        nsdp_build.build()
    lib = ctypes.CDLL(_lib.SO_PATH)
    lib.nsdp_last_error.restype = ctypes.c_char_p
    lib.nsdp_mesh_edge_table_entries.restype = ctypes.c_size_t
    return lib


@pytest.fixture(scope="module")
def sphere():
    """A sphere of 1202 vertices with its table, and the fixed point from one seed."""
    v, f = mr.sphere(30, 40)
    v, f = v.astype(f32), np.asarray(f, np.int64)
    lo, _, nbr, length = gr.edge_table(v, f, [0, len(f)], [0, len(v)])
    start = np.full(len(v), np.inf, f32)
    start[7] = 0
    D, hops = gr.dijkstra(lo, nbr, length[0], start)
    return dict(v=v, f=f, lo=lo, nbr=nbr, length=length[0], start=start, D=D, hops=hops)


def _same(a, b):
    return np.array_equal(np.asarray(a, f32).view(np.uint32), np.asarray(b, f32).view(np.uint32))


# ------------------------------------------------------------------------------------------------------------------ the rule
def test_edge_table_is_symmetric_and_lists_every_edge_of_its_row(sphere):
    s = sphere
    own = gr._owners(s["lo"])
    assert own.size == 6 * len(s["f"]) and s["length"].dtype == f32
    edges = {}
    for a, u, w in zip(own, s["nbr"], s["length"]):
        edges.setdefault((int(a), int(u)), set()).add(f32(w).view(np.uint32).item())
    for (a, u), ws in edges.items():
        assert len(ws) == 1 and edges[(u, a)] == ws          # one length per edge, the same bits from both ends
    tri = s["f"][0]
    assert all((int(tri[i]), int(tri[j])) in edges for i in range(3) for j in range(3) if i != j)


def test_dijkstra_satisfies_the_fixed_point_equation(sphere):
    s = sphere
    assert np.isfinite(s["D"]).all() and s["D"][7] == 0 and s["hops"].max() >= 15
    assert gr.fixed_point_violations(s["lo"], s["nbr"], s["length"], s["start"], s["D"]).size == 0
    worse = s["D"].copy()
    worse[100] = np.nextafter(worse[100], f32(np.inf))
    assert 100 in gr.fixed_point_violations(s["lo"], s["nbr"], s["length"], s["start"], worse)
    # with a limit: pruned candidates, equality kept
    lim = np.sort(s["D"])[300]
    Dl, _ = gr.dijkstra(s["lo"], s["nbr"], s["length"], s["start"], lim)
    assert _same(Dl, np.where(s["D"] <= lim, s["D"], np.inf)) and np.isfinite(Dl).sum() >= 301
    assert gr.fixed_point_violations(s["lo"], s["nbr"], s["length"], s["start"], Dl, lim).size == 0


@pytest.mark.parametrize("block", [64, 256])
def test_block_local_schedule_reaches_the_same_bits(sphere, block):
    s = sphere
    D, rounds = gr.block_local(s["lo"], s["nbr"], s["length"], s["start"], block)
    assert _same(D, s["D"]) and 2 <= rounds <= s["hops"].max() + 1
    plain, plain_rounds = gr.block_local(s["lo"], s["nbr"], s["length"], s["start"], 1)
    assert _same(plain, s["D"]) and plain_rounds >= rounds


def test_renumbering_keeps_the_bits_under_either_schedule(sphere):
    s = sphere
    V = len(s["v"])
    perm = np.random.default_rng(5).permutation(V)               # new row k holds old row perm[k]
    rank = np.empty(V, np.int64)
    rank[perm] = np.arange(V)
    lo, _, nbr, length = gr.edge_table(s["v"][perm], rank[s["f"]], [0, len(s["f"])], [0, V])
    D, _ = gr.dijkstra(lo, nbr, length[0], s["start"][perm])
    assert _same(D[rank], s["D"])
    Db, _ = gr.block_local(lo, nbr, length[0], s["start"][perm], 256)
    assert _same(Db[rank], s["D"])


def test_integer_grid_distances_are_the_integers():
    v, f = gr.grid(23, 17)
    seed = 5 * 23 + 9                                            # (x, y) = (9, 5)
    D, hops = gr.geodesic(v, f, [seed], return_hops=True)
    grid = D.reshape(17, 23)
    assert _same(grid[5], np.abs(np.arange(23) - 9)) and _same(grid[:, 9], np.abs(np.arange(17) - 5))
    assert grid[6, 10] == np.sqrt(f32(2)) and hops.reshape(17, 23)[6, 10] == 1      # along the diagonal
    assert grid[4, 10] == 2                                                          # against it: two unit edges


@pytest.mark.parametrize("mesh", ["sphere", "strip"])
def test_envelope_against_fp64(mesh):
    if mesh == "sphere":
        v, f = mr.sphere(40, 80)
    else:
        v, f = gr.strip(515)
    v, f = np.asarray(v, f32), np.asarray(f, np.int64)
    lo, _, nbr, length = gr.edge_table(v, f, [0, len(f)], [0, len(v)])
    _, _, nbr64, length64 = gr.edge_table(v, f, [0, len(f)], [0, len(v)], dtype=np.float64)
    assert np.array_equal(nbr, nbr64) and length64.dtype == np.float64
    start = np.full(len(v), np.inf, f32)
    start[0] = 0
    D, hops = gr.dijkstra(lo, nbr, length[0], start)
    D64, hops64 = gr.dijkstra(lo, nbr, length64[0], start.astype(np.float64), dtype=np.float64)
    H = np.maximum(hops, hops64)
    assert np.isfinite(D64).all() and H.max() >= (40 if mesh == "sphere" else 250)
    bound = (H + 4) * 2.0 ** -24 * D64
    err = np.abs(D.astype(np.float64) - D64)
    print(f"{mesh}: worst |d - d*| / d* = {np.max(err[1:] / D64[1:]):.3g} against {np.max(bound[1:] / D64[1:]):.3g} at H <= {H.max()}")
    assert (err <= bound).all()


def test_sanitising_takes_negatives_nan_and_minus_zero_as_inf():
    x = f32([0.0, -0.0, 1.5, -1.0, np.nan, np.inf, 3.0, 1e-45])
    assert _same(gr.sanitise(x), f32([0, np.inf, 1.5, np.inf, np.inf, np.inf, 3.0, 1e-45]))
    assert _same(gr.sanitise(x, 1.5), f32([0, np.inf, 1.5, np.inf, np.inf, np.inf, np.inf, 1e-45]))


# ------------------------------------------------------------------------------------------------------------------ boundary
def test_header_declares_and_library_exports_the_entries(so):
    assert _lib.declared_symbols("nsdp_geodesic.h") == sorted(ENTRY_POINTS)
    for other in (None, "nsdp_batch.h", "nsdp_meshbatch.h", "nsdp_meshwhole.h", "nsdp_scatter.h", "nsdp_optim.h", "nsdp_meshnormals.h",
                  "nsdp_surface.h", "nsdp_selfintersect.h", "nsdp_raycast.h"):
        assert not set(ENTRY_POINTS) & set(_lib.declared_symbols(other)), other
    for name in ENTRY_POINTS:
        assert hasattr(so, name), name
    assert so.nsdp_abi_version() >= 29
    assert "nsdp_geodesic.h" in open(nsdp_build.__file__).read() and nsdp_build.PER_FILE["geodesic.hip"] == nsdp_build.EXACT
    assert 'declared_symbols("nsdp_geodesic.h")' in open(os.path.join(ROOT, "__graft_entry__.py")).read()
    from nsdp_amd import geodesic
    header = open(os.path.join(ROOT, "include", "nsdp_geodesic.h")).read()
    assert so.nsdp_mesh_geodesic_block() == geodesic.BLOCK and f"#define NSDP_GEODESIC_BLOCK {geodesic.BLOCK}\n" in header
    assert f"#define NSDP_GEODESIC_NO_LOCAL {geodesic.NO_LOCAL} " in header
    assert f"#define NSDP_GEODESIC_MAX_ROUNDS {geodesic.MAX_ROUNDS}\n" in header


def test_corner_text_is_shared_with_the_normals():
    """One definition of a corner's row: mesh_normals.hip and geodesic.hip include it, neither keeps a copy."""
    csrc = os.path.join(ROOT, "nsdp_amd", "csrc")
    assert "corner_rows_of" in open(os.path.join(csrc, "mesh_corners.h")).read()
    for src in ("mesh_normals.hip", "geodesic.hip"):
        text = open(os.path.join(csrc, src)).read()
        assert '#include "mesh_corners.h"' in text and "struct Mesh {" not in text, src


def test_size_query(so):
    size = so.nsdp_mesh_edge_table_entries
    for B, vcap, fcap in ((1, 1, 1), (3, 7, 129), (65535, 1 << 20, (1 << 25) // 3)):
        assert size(B, vcap, fcap) == 6 * fcap
    for B, vcap, fcap in ((0, 1, 1), (65536, 1, 1), (1, 0, 1), (1, (1 << 20) + 1, 1), (1, 1, 0), (1, 1, (1 << 25) // 3 + 1), (-1, 1, 1)):
        assert size(B, vcap, fcap) == 0


def _relax(so, B=2, vcap=8, fcap=12, P=2, limit=1.5, rounds=3, flags=0, ptrs=(16,) * 6):
    loff, nbr, length, voff, dist, changed = (_vp(p) for p in ptrs)
    rc = so.nsdp_mesh_geodesic_relax(loff, nbr, length, voff, _ci(B), _ci(vcap), _ci(fcap), _ci(P), _cf(limit), _ci(rounds), _ci(flags),
                                     dist, changed, _vp(0))
    return rc, so.nsdp_last_error().decode()


def _lengths(so, P=2, B=2, vcap=8, fcap=12, ptrs=(16,) * 8):
    verts, faces, foff, voff, loff, lent, nbr, length = (_vp(p) for p in ptrs)
    rc = so.nsdp_mesh_edge_lengths(verts, _ci(P), faces, foff, voff, _ci(B), _ci(vcap), _ci(fcap), loff, lent, nbr, length, _vp(0))
    return rc, so.nsdp_last_error().decode()


SIZES = [(dict(P=0), "P=0"), (dict(P=65536), "P=65536"), (dict(B=0), "B=0"), (dict(B=65536), "B=65536"), (dict(vcap=0), "vcap=0"),
         (dict(vcap=(1 << 20) + 1), "vcap=1048577"), (dict(fcap=0), "fcap=0"), (dict(fcap=(1 << 25) // 3 + 1), "fcap=11184811")]


@pytest.mark.parametrize("kw,word", SIZES)
def test_every_size_limit_is_refused_by_name_before_anything_else(so, kw, word):
    rc, msg = _lengths(so, ptrs=(0,) * 8, **kw)
    assert rc == -1 and word in msg and "mesh_edge_lengths" in msg, msg
    rc, msg = _relax(so, limit=float("nan"), rounds=0, flags=6, ptrs=(0,) * 6, **kw)
    assert rc == -1 and word in msg and "mesh_geodesic_relax" in msg, msg


def test_values_are_refused_by_name_before_pointers(so):
    for limit in (float("nan"), -1.0, -0.0, float("-inf")):
        rc, msg = _relax(so, limit=limit, ptrs=(0,) * 6)
        assert rc == -1 and "limit=" in msg and "NaN or negative" in msg, (limit, msg)
    for rounds in (0, -3, 1025):
        rc, msg = _relax(so, rounds=rounds, ptrs=(0,) * 6)
        assert rc == -1 and f"rounds={rounds} " in msg, msg
    for flags in (2, 4, 3, -1):
        rc, msg = _relax(so, flags=flags, ptrs=(0,) * 6)
        assert rc == -1 and f"flags={flags} " in msg, msg
    for kw in (dict(limit=float("inf")), dict(limit=0.0), dict(rounds=1), dict(rounds=1024), dict(flags=1)):
        rc, msg = _relax(so, ptrs=(0,) * 6, **kw)
        assert rc == -1 and "null" in msg, (kw, msg)            # taken: the next thing judged is the pointers


def test_null_and_misaligned_pointers(so):
    for i in range(6):
        rc, msg = _relax(so, ptrs=tuple(0 if k == i else 16 for k in range(6)))
        assert rc == -1 and "null" in msg, (i, msg)
    for i in range(8):
        if i == 6:                                               # nbr may be null: that call would be taken, and launched
            continue
        rc, msg = _lengths(so, ptrs=tuple(0 if k == i else 16 for k in range(8)))
        assert rc == -1 and "null" in msg, (i, msg)
    rc, msg = _lengths(so, ptrs=(16, 16, 16, 16, 16, 16, 0, 20))      # a null nbr is no refusal: the next thing judged is named
    assert rc == -1 and "aligned" in msg, msg
    for i, odd in ((0, 18), (1, 20), (2, 20), (3, 18), (4, 18), (5, 17)):      # nbr and len are pairs: 8-byte
        rc, msg = _relax(so, ptrs=tuple(odd if k == i else 16 for k in range(6)))
        assert rc == -1 and "aligned" in msg, (i, msg)
        rc, msg = _relax(so, ptrs=tuple(odd if k == i else (0 if k == (i + 1) % 6 else 16) for k in range(6)))
        assert rc == -1 and "null" in msg, (i, msg)              # pointers before the alignment
    for i, odd in ((0, 18), (1, 18), (2, 18), (3, 18), (4, 18), (5, 18), (6, 20), (7, 20)):
        rc, msg = _lengths(so, ptrs=tuple(odd if k == i else 16 for k in range(8)))
        assert rc == -1 and "aligned" in msg, (i, msg)


def test_bad_argument_table_through_the_stand_alone_host_program(so, tmp_path):
    """tools/geodesic_host_check.cpp, linked against the built library: sizes before values before pointers before the
    alignment; no GPU is touched, nothing is launched."""
    exe = str(tmp_path / "geodesic_host_check")
    libdir = os.path.dirname(_lib.SO_PATH)
    subprocess.check_call([nsdp_build.HIPCC, "-x", "c++", "-std=c++17", os.path.join(ROOT, "tools", "geodesic_host_check.cpp"),
                           "-L" + libdir, "-lnsdp_hip", "-Wl,-rpath," + libdir, "-o", exe])
    done = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert done.returncode == 0 and done.stdout.strip() == "ok", done.stderr


# ------------------------------------------------------------------------------------------------------------------ python
def test_wrapper_refuses_by_name_without_a_device(monkeypatch):
    import torch
    from nsdp_amd import geodesic as g
    with pytest.raises(g.GeodesicError, match="GPU tensor"):
        g.GeodesicPlan(torch.zeros(4, 3, dtype=torch.int32), torch.zeros(5, 3))
    with pytest.raises(g.GeodesicError, match="GeodesicPlan"):
        g.geodesic_distances(torch.zeros(5, 3), object(), torch.zeros(1, dtype=torch.int64))
    with pytest.raises(g.GeodesicError, match="GPU tensor"):
        g.mesh_edge_lengths(torch.zeros(1, 5, 3), None, None, None, None, None)
    monkeypatch.delenv("NSDP_GEODESIC_ROUNDS", raising=False)
    assert g._rounds_default() == g.DEFAULT_ROUNDS and 1 <= g.DEFAULT_ROUNDS <= g.MAX_ROUNDS
    monkeypatch.setenv("NSDP_GEODESIC_ROUNDS", "3")
    assert g._rounds_default() == 3
    for bad in ("0", "1025", "many"):
        monkeypatch.setenv("NSDP_GEODESIC_ROUNDS", bad)
        with pytest.raises(g.GeodesicError, match="NSDP_GEODESIC_ROUNDS"):
            g._rounds_default()


def test_knob_is_documented_and_in_the_matrix():
    assert "NSDP_GEODESIC_ROUNDS" in open(os.path.join(ROOT, "docs", "KNOBS.md")).read()
    assert "NSDP_GEODESIC_ROUNDS" in open(os.path.join(ROOT, "tools", "knob_matrix.sh")).read()


def test_edit_tool_takes_the_flag():
    from nsdp_amd import edit
    args = edit.build_parser().parse_args(["c", "--vertices", "5000", "--brush", "0,0,2,0,0,-1,0.1", "--brush", "0,2,0,0,-1,0,0.2"])
    assert edit.brushes_from_args(args) == [[0.0, 0.0, 2.0, 0.0, 0.0, -1.0, 0.1], [0.0, 2.0, 0.0, 0.0, -1.0, 0.0, 0.2]]
    assert edit.brushes_from_args(edit.build_parser().parse_args(["c"])) is None
    with pytest.raises(SystemExit, match="--brush wants seven numbers"):
        edit.main(["c", "--brush", "0,0,2"])
    with pytest.raises(SystemExit, match="--brush goes with --vertices"):
        edit.main(["c", "--vertex-counts", "100,200", "--brush", "0,0,2,0,0,-1,0.1"])
