"""The launching entry of include/nsdp_raster.h inside the poisoned arena of tests/poison_arena.py, as
tests/test_ray_cast_arena_gpu.py holds that of include/nsdp_raycast.h: every operand between guards, the workspace exactly the
bytes the size query declares and poisoned on entry, every output poisoned until the kernels write it, no byte changed outside
them, every element of every image written, nothing beyond I * H * W touched -- and nothing read that nobody wrote: the poison
is NaN (and -1 as a face, an offset or a mesh), and the results are compared with the emulation byte for byte.  Both forms,
bary_out / count_out NULL and non-NULL.  COVERAGE plays the part of the other files' table for this header."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import raster_ref as ra
from poison_arena import PoisonArena
from test_raster_gpu import _scene

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "nsdp_raster.h")

COVERAGE = {"nsdp_mesh_rasterize": "test_entry_inside_the_arena"}
HOST_ONLY = {"nsdp_mesh_rasterize_workspace_bytes"}
_SEEN: set = set()

_ci, _vp = ctypes.c_int, ctypes.c_void_p


def _p(t):
    return _vp(0) if t is None else _vp(t.data_ptr())


def _launch(a, scene, H, W, flags, with_bary, with_count):
    from nsdp_amd import _lib
    L = _lib.lib()
    verts, voff, faces, foff, cams, shape = scene
    B, I, vcap, fcap = len(voff) - 1, len(cams), len(verts), len(faces)
    tv, tvo = a.input("verts", torch.tensor(verts)), a.input("vert_offsets", torch.tensor(voff))
    tf, tfo = a.input("faces", torch.tensor(faces)), a.input("face_offsets", torch.tensor(foff))
    tc, ts = a.input("cams", torch.tensor(cams)), a.input("image_shape", torch.tensor(shape))
    size = L.nsdp_mesh_rasterize_workspace_bytes
    size.restype = ctypes.c_size_t
    need = int(size(_ci(B), _ci(I), _ci(fcap)))
    assert need == 20 * I * (fcap // 64 + B + 1)
    ws = a.workspace("workspace", need)
    depth, face = a.output("depth_out", (I, H, W)), a.output("face_out", (I, H, W), torch.int32)
    bary = a.output("bary_out", (I, H, W, 3)) if with_bary else None
    count = a.output("count_out", (I, H, W), torch.int32) if with_count else None
    dropped = a.output("dropped_out", (I,), torch.int32)
    with a.routed():
        _lib.check(_lib.lib().nsdp_mesh_rasterize(_p(tv), _p(tvo), _p(tf), _p(tfo), _p(tc), _p(ts), _ci(B), _ci(I), _ci(vcap), _ci(fcap),
                                                  _ci(H), _ci(W), _ci(flags), _p(ws), _p(depth), _p(face), _p(bary), _p(count),
                                                  _p(dropped), _lib.stream_ptr()), "nsdp_mesh_rasterize")
    _SEEN.update(a.called)
    return depth, face, bary, count, dropped


@pytest.mark.parametrize("with_bary,with_count", [(True, True), (False, False), (True, False), (False, True)])
@pytest.mark.parametrize("H,W,F", [(1, 1, 1), (33, 17, 65), (64, 48, 129)])
def test_entry_inside_the_arena(H, W, F, with_bary, with_count):
    scene = _scene(F, H, W, 11 * F + W)
    flags = ra.FRONT_ONLY if (with_bary and not with_count) else 0
    want = ra.rasterize(*scene, H, W, flags)
    a = PoisonArena(DEV, 16 << 20)
    depth, face, bary, count, dropped = _launch(a, scene, H, W, flags, with_bary, with_count)
    # every element written (a face of -1 and a count of -1 are the poison pattern too: those are compared below)
    a.check(written=[depth] + ([bary] if with_bary else []))
    assert np.array_equal(depth.cpu().numpy().view(np.uint32), want["depth"].view(np.uint32))      # (a NaN -- poison that was read -- fails this)
    assert np.array_equal(face.cpu().numpy(), want["face"]) and np.array_equal(dropped.cpu().numpy(), want["dropped"])
    if with_bary:
        assert np.array_equal(bary.cpu().numpy().view(np.uint32), want["bary"].view(np.uint32))
    if with_count:
        assert np.array_equal(count.cpu().numpy(), want["count"]) and bool((count >= 0).all())


def test_stale_offsets_indices_and_meshes_stay_inside_the_operands():
    """Offsets, vertex indices and image_shape entries outside their ranges (a poisoned or stale tensor) are clamped before they
    form an address: wrong numbers, but nothing outside the operands is read into a fault or written."""
    g = torch.Generator().manual_seed(3)
    lo, hi = -(1 << 31), (1 << 31) - 1
    B, I, vcap, fcap, H, W = 3, 4, 50, 200, 33, 17
    v = (torch.rand(vcap, 3, generator=g) * 2 - 1).numpy()
    f = torch.randint(-10, 40, (fcap, 3), generator=g, dtype=torch.int64)         # half of them outside the mesh's 20 vertices
    f[::7] = torch.randint(lo, hi, (len(f[::7]), 3), generator=g, dtype=torch.int64)      # and some anywhere in int32
    f = f.int().numpy()
    voff = np.array([0, 20, 20, 1 << 30], np.int32)              # (the second mesh has no vertices: no faces either)
    foff = np.array([7, 90, 150, -1], np.int32)                  # clamped: [7, 90, 150, 150]
    cams = np.stack([ra.pinhole(12, W / 2, H / 2, 3).reshape(16)] * I)
    shape = np.array([-5, 1, 1 << 30, 0], np.int32)              # clamped: [0, 1, 2, 0]
    scene = (v, voff, f, foff, cams, shape)
    want = ra.rasterize(*scene, H, W, 0)
    a = PoisonArena(DEV, 16 << 20)
    depth, face, bary, count, dropped = _launch(a, scene, H, W, 0, True, True)
    a.check(written=[depth, bary])
    assert bool(torch.isfinite(depth).all()) and bool(torch.isfinite(bary).all())
    fn = face.cpu().numpy()
    assert ((fn[0] == -1) | ((fn[0] >= 7) & (fn[0] < 90))).all() and (fn[0] >= 0).any()        # the first mesh's faces, as clamped
    assert (fn[1] == -1).all() and (fn[2] == -1).all() and np.array_equal(fn[3], fn[0])
    assert np.array_equal(fn, want["face"]) and np.array_equal(count.cpu().numpy(), want["count"])
    assert np.array_equal(depth.cpu().numpy().view(np.uint32), want["depth"].view(np.uint32))


def test_wrapper_allocates_inside_the_arena():
    """rasterize with the wrapper's own allocations (workspace, outputs, the face renumbering) routed through the arena: all get
    guards too."""
    from nsdp_amd import rasterize
    v, f = ra.uv_sphere()
    H, W = 33, 40
    cam = rasterize.Camera.look_at((2.5, 1.5, -3), (0, 0, 0), (0, 1, 0), 35, W, H)
    want = ra.image(v, f, cam.matrix, H, W)
    for reorder in (False, True):
        plan = rasterize.RasterPlan(torch.tensor(f).to(DEV), torch.tensor(v).to(DEV), reorder=reorder)
        a = PoisonArena(DEV, 16 << 20)
        tv, tc = a.input("verts", torch.tensor(v)), a.input("cams", torch.tensor(cam.matrix).reshape(1, 4, 4))
        with a.routed(rasterize):
            r = rasterize.rasterize(tv, plan, tc, H, W, count=True)
        _SEEN.update(a.called)
        assert "nsdp_mesh_rasterize" in a.called
        a.check()
        assert np.array_equal(r.depth[0].cpu().numpy().view(np.uint32), want["depth"].view(np.uint32))
        assert np.array_equal(r.count[0].cpu().numpy(), want["count"])
        apart = want["second"] != want["depth"]
        assert np.array_equal(r.face[0].cpu().numpy()[apart], want["face"][apart])


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
