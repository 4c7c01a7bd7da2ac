"""The launching entry of include/nsdp_surface.h inside the poisoned arena of tests/poison_arena.py, as
tests/test_rigidity_arena_gpu.py holds those of include/nsdp_rigidity.h: every operand between guards, the workspace exactly the
bytes the size query declares and poisoned on entry, outputs poisoned until the kernels write them, no byte changed outside
them, no output row of a live query left unwritten -- and nothing read that nobody wrote: the poison is NaN (and -1 as a face or
an offset), and the results are compared with the fp64 yardstick.  COVERAGE plays the part of the other files' table for this
header."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import surface_ref
from poison_arena import PoisonArena
from surface_ref import E, U

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "nsdp_surface.h")

COVERAGE = {"nsdp_mesh_closest": "test_entry_inside_the_arena"}
HOST_ONLY = {"nsdp_mesh_closest_workspace_bytes"}
_SEEN: set = set()

_ci, _vp = ctypes.c_int, ctypes.c_void_p
FLT_MAX = np.float32(np.finfo(np.float32).max)


def _p(t):
    return _vp(0) if t is None else _vp(t.data_ptr())


def _batch(n, F, seed):
    """Three shapes packed, capacities beyond the last offsets: a mesh of F faces with n queries, a mesh without faces with 3
    queries, a mesh of 70 faces with 66 queries."""
    rng = np.random.default_rng(seed)
    V = max(3, F // 2 + 2)
    meshes = [(rng.standard_normal((V, 3)).astype(np.float32), rng.integers(0, V, (F, 3))),
              (rng.standard_normal((4, 3)).astype(np.float32), np.zeros((0, 3), dtype=np.int64)),
              (rng.standard_normal((40, 3)).astype(np.float32) + 3, rng.integers(0, 40, (70, 3)))]
    queries = [(rng.standard_normal((k, 3)) * 1.5).astype(np.float32) for k in (n, 3, 66)]
    queries[2] += 3
    pad = 5

    def pack(rows, dtype, fill):
        off = np.cumsum([0] + [len(r) for r in rows])
        return torch.tensor(np.concatenate(list(rows) + [np.full((pad, 3), fill)]).astype(dtype)), torch.tensor(off, dtype=torch.int32)

    return meshes, queries, pack(queries, np.float32, np.nan), pack([m[0] for m in meshes], np.float32, np.nan), \
        pack([m[1] for m in meshes], np.int32, -1)


@pytest.mark.parametrize("cull", [True, False])
@pytest.mark.parametrize("with_bary", [True, False])
@pytest.mark.parametrize("n,F", [(1, 1), (65, 63), (257, 129)])
def test_entry_inside_the_arena(n, F, with_bary, cull):
    from nsdp_amd import _lib
    L = _lib.lib()
    meshes, queries, (q, qoff), (v, voff), (f, foff) = _batch(n, F, 13 * n + F)
    B, qcap, vcap, fcap = 3, int(q.shape[0]), int(v.shape[0]), int(f.shape[0])
    live = int(qoff[-1])
    a = PoisonArena(DEV, 16 << 20)
    tq, tqo, tv, tvo = a.input("query", q), a.input("query_offsets", qoff), a.input("verts", v), a.input("vert_offsets", voff)
    tf, tfo = a.input("faces", f), a.input("face_offsets", foff)
    size = L.nsdp_mesh_closest_workspace_bytes
    size.restype = ctypes.c_size_t
    need = int(size(_ci(B), _ci(qcap), _ci(fcap)))
    assert need == 8 * qcap + 24 * (fcap // 64 + B + 1)
    ws = a.workspace("workspace", need)
    d2, face = a.output("dist2_out", (qcap,), rows=live), a.output("face_out", (qcap,), torch.int32, rows=live)
    bary = a.output("bary_out", (qcap, 3), rows=live) if with_bary else None
    with a.routed():
        _lib.check(_lib.lib().nsdp_mesh_closest(_p(tq), _p(tqo), _p(tv), _p(tvo), _p(tf), _p(tfo), _ci(B), _ci(qcap), _ci(vcap), _ci(fcap),
                                                _ci(0 if cull else 1), _p(ws), _p(d2), _p(face), _p(bary), _lib.stream_ptr()),
                   "nsdp_mesh_closest")
    _SEEN.update(a.called)
    # every live row written (face -1 of the mesh without faces is the poison pattern too: those rows are compared below), the
    # key of every live query in the workspace as well
    has_faces = torch.ones(live, dtype=torch.bool)
    has_faces[n:n + 3] = False
    rows = has_faces.nonzero().reshape(-1).to(DEV)
    a.check(written=[d2[:live], ws[:2 * live].view(torch.int64)] + ([bary[:live]] if with_bary else []))
    assert int((face[rows] == -1).sum()) == 0
    lo = first = 0
    for (mv, mf), mq in zip(meshes, queries):
        k = len(mq)
        gd, gf = d2[lo:lo + k].cpu().numpy(), face[lo:lo + k].cpu().numpy()
        if len(mf) == 0:
            assert (gd == FLT_MAX).all() and (gf == -1).all() and (not with_bary or bool((bary[lo:lo + k] == 0).all()))
        else:
            best, bface, _ = surface_ref.brute(mq, mv, mf)
            local = gf - first
            assert (local >= 0).all() and (local < len(mf)).all()
            unit = U * np.maximum(surface_ref.corner_r2(mq, mv, mf, local), surface_ref.corner_r2(mq, mv, mf, bface))
            assert (np.abs(gd.astype(np.float64) - best) <= (E + 1) * unit).all()      # (a NaN -- poison that was read -- fails this)
            if with_bary:
                gb = bary[lo:lo + k].cpu().numpy().astype(np.float64)
                assert (gb >= 0).all() and (np.abs(gb.sum(-1) - 1) <= 4 * U).all()
        lo, first = lo + k, first + len(mf)


def test_stale_offsets_and_indices_stay_inside_the_operands():
    """Offsets and vertex indices outside their ranges (a poisoned or stale tensor) are clamped before they form an address:
    wrong numbers, but nothing outside the operands is read into a fault or written."""
    from nsdp_amd import _lib
    g = torch.Generator().manual_seed(3)
    lo, hi = -(1 << 31), (1 << 31) - 1
    B, qcap, vcap, fcap = 3, 300, 50, 200
    q, v = torch.randn(qcap, 3, generator=g), torch.randn(vcap, 3, generator=g)
    f = torch.randint(lo, hi, (fcap, 3), generator=g, dtype=torch.int64).int()
    qoff = torch.tensor([-5, 130, 100, 1 << 30], dtype=torch.int32)           # clamped: [0, 130, 130, 300]
    voff = torch.tensor([0, 20, 20, 1 << 30], dtype=torch.int32)              # (the second mesh has no vertices: no faces either)
    foff = torch.tensor([7, 90, 150, -1], dtype=torch.int32)                  # clamped: [7, 90, 150, 150]
    for cull in (True, False):
        a = PoisonArena(DEV, 16 << 20)
        tq, tqo, tv, tvo = a.input("query", q), a.input("query_offsets", qoff), a.input("verts", v), a.input("vert_offsets", voff)
        tf, tfo = a.input("faces", f), a.input("face_offsets", foff)
        ws = a.workspace("workspace", 8 * qcap + 24 * (fcap // 64 + B + 1))
        d2, face, bary = a.output("dist2_out", (qcap,)), a.output("face_out", (qcap,), torch.int32), a.output("bary_out", (qcap, 3))
        with a.routed():
            _lib.check(_lib.lib().nsdp_mesh_closest(_p(tq), _p(tqo), _p(tv), _p(tvo), _p(tf), _p(tfo), _ci(B), _ci(qcap), _ci(vcap),
                                                    _ci(fcap), _ci(0 if cull else 1), _p(ws), _p(d2), _p(face), _p(bary),
                                                    _lib.stream_ptr()), "nsdp_mesh_closest")
        _SEEN.update(a.called)
        a.check(written=[d2, bary])
        assert bool(torch.isfinite(d2).all()) and bool(torch.isfinite(bary).all())
        assert bool(((face[:130] >= 7) & (face[:130] < 90)).all())            # the first mesh's faces, as clamped
        assert bool((face[130:] == -1).all()) and bool((d2[130:] == float(FLT_MAX)).all())      # the third shape's mesh: no faces


def test_wrapper_allocates_inside_the_arena():
    """closest_on_mesh with the wrapper's own allocations (workspace, outputs, the reordered copies' scatter targets) routed
    through the arena: all get guards too."""
    from nsdp_amd import surface_distance
    v, f = surface_ref.icosphere(1)
    q = surface_ref.sphere_queries(130, 7)
    for reorder in (False, True):
        a = PoisonArena(DEV, 16 << 20)
        tq, tv = a.input("query", torch.tensor(q)[None]), a.input("verts", torch.tensor(v)[None])
        tf = a.input("faces", torch.tensor(f)[None])
        with a.routed(surface_distance):
            d2, face, bary = surface_distance.closest_on_mesh(tq, tv, tf, reorder=reorder)
        _SEEN.update(a.called)
        assert "nsdp_mesh_closest" in a.called
        a.check()
        best, bface, _ = surface_ref.brute(q, v, f)
        gf = face[0].cpu().numpy()
        unit = U * np.maximum(surface_ref.corner_r2(q, v, f, gf), surface_ref.corner_r2(q, v, f, bface))
        assert (np.abs(d2[0].cpu().numpy().astype(np.float64) - best) <= (E + 1) * unit).all()
        assert bool(torch.isfinite(bary).all())


def test_every_launching_entry_of_the_header_is_called_inside_the_arena():
    """Last in the file: the table against the header, and against what the recording proxy saw in the tests above."""
    with open(HEADER) as fh:
        text = re.sub(r"/\*.*?\*/", "", fh.read(), flags=re.S)
    declared = set(re.findall(r"\b(nsdp_[a-z0-9_]+)\s*\(", text))
    assert declared == set(COVERAGE) | HOST_ONLY, sorted(declared ^ (set(COVERAGE) | HOST_ONLY))
    for entry, test in COVERAGE.items():
        assert callable(globals().get(test)), f"{entry}: no test function {test}"
    if _SEEN:                                                             # (run alone, this test has nothing to compare)
        assert set(COVERAGE) <= _SEEN, sorted(set(COVERAGE) - _SEEN)
