"""The launching entry of include/nsdp_raycast.h inside the poisoned arena of tests/poison_arena.py, as
tests/test_surface_distance_arena_gpu.py holds that of include/nsdp_surface.h: every operand between guards, the workspace
exactly the bytes the size query declares and poisoned on entry, outputs poisoned until the kernels write them, no byte changed
outside them, no output row of a live ray left unwritten, rows beyond the last ray offset untouched -- and nothing read that
nobody wrote: the poison is NaN (and -1 as a face or an offset), and the results are compared with the emulation byte for byte.
Both forms, bary_out / count_out NULL and non-NULL.  COVERAGE plays the part of the other files' table for this header."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import ray_cast_ref as rr
from poison_arena import PoisonArena

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "nsdp_raycast.h")

COVERAGE = {"nsdp_mesh_ray_cast": "test_entry_inside_the_arena"}
HOST_ONLY = {"nsdp_mesh_ray_cast_workspace_bytes"}
_SEEN: set = set()

_ci, _vp = ctypes.c_int, ctypes.c_void_p
f32 = np.float32


def _p(t):
    return _vp(0) if t is None else _vp(t.data_ptr())


def _batch(n, F, seed):
    """Three shapes packed, capacities beyond the last offsets: a mesh of F faces with n rays, a mesh without faces with 3 rays,
    a cube with 66 rays."""
    rng = np.random.default_rng(seed)
    V = max(3, F // 2 + 2)
    vc, fc = rr.cube()
    meshes = [(rng.standard_normal((V, 3)).astype(f32), rng.integers(0, V, (F, 3))),
              (rng.standard_normal((4, 3)).astype(f32), np.zeros((0, 3), dtype=np.int64)), (vc + f32(3), fc)]
    origins = [(rng.standard_normal((k, 3)) * 1.5).astype(f32) for k in (n, 3, 66)]
    origins[2] += 3
    dirs = [rng.standard_normal((k, 3)).astype(f32) for k in (n, 3, 66)]
    if F == 1:
        meshes[0][0][:3] = f32([[-9, -9, 0.5], [9, -9, 0.25], [0, 9, -0.5]])
        meshes[0][1][0] = (0, 1, 2)
    pad = 5

    def pack(rows, dtype, fill):
        off = np.cumsum([0] + [len(r) for r in rows])
        return np.concatenate(list(rows) + [np.full((pad, 3), fill)]).astype(dtype), off.astype(np.int32)

    return pack(origins, f32, np.nan), pack(dirs, f32, np.nan), pack([m[0] for m in meshes], f32, np.nan), \
        pack([m[1] for m in meshes], np.int32, -1)


@pytest.mark.parametrize("cull", [True, False])
@pytest.mark.parametrize("with_bary,with_count", [(True, True), (False, False), (True, False), (False, True)])
@pytest.mark.parametrize("n,F", [(1, 1), (65, 63), (257, 129)])
def test_entry_inside_the_arena(n, F, with_bary, with_count, cull):
    from nsdp_amd import _lib
    L = _lib.lib()
    (o, roff), (d, _), (v, voff), (f, foff) = _batch(n, F, 13 * n + F)
    B, qcap, vcap, fcap = 3, len(o), len(v), len(f)
    live = int(roff[-1])
    want = rr.ray_cast(o, d, roff, v, voff, f, foff)
    assert (want[3][:live] > 0).sum() > 0
    a = PoisonArena(DEV, 16 << 20)
    to, td, tro = a.input("origins", torch.tensor(o)), a.input("dirs", torch.tensor(d)), a.input("ray_offsets", torch.tensor(roff))
    tv, tvo = a.input("verts", torch.tensor(v)), a.input("vert_offsets", torch.tensor(voff))
    tf, tfo = a.input("faces", torch.tensor(f)), a.input("face_offsets", torch.tensor(foff))
    size = L.nsdp_mesh_ray_cast_workspace_bytes
    size.restype = ctypes.c_size_t
    need = int(size(_ci(B), _ci(qcap), _ci(fcap)))
    assert need == 12 * qcap + 24 * (fcap // 64 + B + 1)
    ws = a.workspace("workspace", need)
    t, face = a.output("t_out", (qcap,), rows=live), a.output("face_out", (qcap,), torch.int32, rows=live)
    bary = a.output("bary_out", (qcap, 3), rows=live) if with_bary else None
    count = a.output("count_out", (qcap,), torch.int32, rows=live) if with_count else None
    with a.routed():
        _lib.check(_lib.lib().nsdp_mesh_ray_cast(_p(to), _p(td), _p(tro), _p(tv), _p(tvo), _p(tf), _p(tfo), _ci(B), _ci(qcap), _ci(vcap),
                                                 _ci(fcap), _ci(0 if cull else 1), _p(ws), _p(t), _p(face), _p(bary), _p(count),
                                                 _lib.stream_ptr()), "nsdp_mesh_ray_cast")
    _SEEN.update(a.called)
    # every live row written (a face of -1 and a count of -1 are the poison pattern too: those rows are compared below), the key
    # of every live ray in the workspace as well
    a.check(written=[t[:live], ws[:2 * live].view(torch.int64)] + ([bary[:live]] if with_bary else []))
    got = (t.cpu().numpy(), face.cpu().numpy(), bary.cpu().numpy() if with_bary else None, count.cpu().numpy() if with_count else None)
    assert np.array_equal(got[0][:live].view(np.uint32), want[0][:live].view(np.uint32))      # (a NaN -- poison that was read -- fails this)
    assert np.array_equal(got[1][:live], want[1][:live])
    if with_bary:
        assert np.array_equal(got[2][:live].view(np.uint32), want[2][:live].view(np.uint32))
    if with_count:
        assert np.array_equal(got[3][:live], want[3][:live]) and (got[3][:live] >= 0).all()


def test_stale_offsets_and_indices_stay_inside_the_operands():
    """Offsets and vertex indices outside their ranges (a poisoned or stale tensor) are clamped before they form an address:
    wrong numbers, but nothing outside the operands is read into a fault or written."""
    from nsdp_amd import _lib
    g = torch.Generator().manual_seed(3)
    lo, hi = -(1 << 31), (1 << 31) - 1
    B, qcap, vcap, fcap = 3, 300, 50, 200
    o, d, v = torch.randn(qcap, 3, generator=g) * 2, torch.randn(qcap, 3, generator=g), torch.randn(vcap, 3, generator=g)
    f = torch.randint(lo, hi, (fcap, 3), generator=g, dtype=torch.int64).int()
    roff = torch.tensor([-5, 130, 100, 1 << 30], dtype=torch.int32)           # clamped: [0, 130, 130, 300]
    voff = torch.tensor([0, 20, 20, 1 << 30], dtype=torch.int32)              # (the second mesh has no vertices: no faces either)
    foff = torch.tensor([7, 90, 150, -1], dtype=torch.int32)                  # clamped: [7, 90, 150, 150]
    want = rr.ray_cast(o.numpy(), d.numpy(), roff.numpy(), v.numpy(), voff.numpy(), f.numpy(), foff.numpy())
    for cull in (True, False):
        a = PoisonArena(DEV, 16 << 20)
        to, td, tro = a.input("origins", o), a.input("dirs", d), a.input("ray_offsets", roff)
        tv, tvo, tf, tfo = a.input("verts", v), a.input("vert_offsets", voff), a.input("faces", f), a.input("face_offsets", foff)
        ws = a.workspace("workspace", 12 * qcap + 24 * (fcap // 64 + B + 1))
        t, face = a.output("t_out", (qcap,)), a.output("face_out", (qcap,), torch.int32)
        bary, count = a.output("bary_out", (qcap, 3)), a.output("count_out", (qcap,), torch.int32)
        with a.routed():
            _lib.check(_lib.lib().nsdp_mesh_ray_cast(_p(to), _p(td), _p(tro), _p(tv), _p(tvo), _p(tf), _p(tfo), _ci(B), _ci(qcap),
                                                     _ci(vcap), _ci(fcap), _ci(0 if cull else 1), _p(ws), _p(t), _p(face), _p(bary),
                                                     _p(count), _lib.stream_ptr()), "nsdp_mesh_ray_cast")
        _SEEN.update(a.called)
        a.check(written=[t, bary])
        assert bool(torch.isfinite(t).all()) and bool(torch.isfinite(bary).all())
        assert bool(((face[:130] == -1) | ((face[:130] >= 7) & (face[:130] < 90))).all())      # the first mesh's faces, as clamped
        assert bool((face[130:] == -1).all()) and bool((count[130:] == 0).all())                # the third shape's mesh: no faces
        assert np.array_equal(face.cpu().numpy(), want[1]) and np.array_equal(count.cpu().numpy(), want[3])


def test_wrapper_allocates_inside_the_arena():
    """cast_rays with the wrapper's own allocations (workspace, outputs, the face renumbering) routed through the arena: all get
    guards too."""
    from nsdp_amd import ray_cast
    v, f = rr.uv_sphere()
    rng = np.random.default_rng(7)
    o, d = rng.uniform(-1.5, 1.5, (130, 3)).astype(f32), rng.standard_normal((130, 3)).astype(f32)
    for reorder in (False, True):
        plan = ray_cast.RayCastPlan(torch.tensor(f).to(DEV), torch.tensor(v).to(DEV), reorder=reorder)
        a = PoisonArena(DEV, 16 << 20)
        to, td, tv = a.input("origins", torch.tensor(o)), a.input("dirs", torch.tensor(d)), a.input("verts", torch.tensor(v))
        with a.routed(ray_cast):
            hits = ray_cast.cast_rays(to, td, tv, plan)
        _SEEN.update(a.called)
        assert "nsdp_mesh_ray_cast" in a.called
        a.check()
        want = rr.cast(o, d, v, f)
        assert np.array_equal(hits.t.cpu().numpy().view(np.uint32), want[0].view(np.uint32))
        assert np.array_equal(hits.crossings.cpu().numpy(), want[3]) and np.array_equal(hits.face.cpu().numpy(), want[1])


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
