"""Both launching entries of include/nsdp_geodesic.h inside the poisoned arena of tests/poison_arena.py, as
tests/test_ray_cast_arena_gpu.py holds that of include/nsdp_raycast.h: every operand between guards, outputs poisoned until the
kernels write them and written whole -- nbr, len, changed_out, and EVERY row of dist, those beyond the totals too --, no byte
changed outside them, and nothing read that nobody wrote: the poison is NaN (and -1 as a face, a row or an offset), and the
results are compared with the emulation byte for byte.  Stale nbr rows and offsets (-1, beyond the capacity) stay inside the
operands and the call returns.  COVERAGE plays the part of the other files' table for this header."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import geodesic_ref as gr
from poison_arena import PoisonArena

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "nsdp_geodesic.h")

COVERAGE = {"nsdp_mesh_edge_lengths": "test_entries_inside_the_arena", "nsdp_mesh_geodesic_relax": "test_entries_inside_the_arena"}
HOST_ONLY = {"nsdp_mesh_edge_table_entries", "nsdp_mesh_geodesic_block"}
_SEEN: set = set()

_ci, _vp, _cf = ctypes.c_int, ctypes.c_void_p, ctypes.c_float
f32 = np.float32
INF_BITS = 0x7F800000


def _p(t):
    return _vp(0) if t is None else _vp(t.data_ptr())


def _K():
    from nsdp_amd import geodesic
    return geodesic.BLOCK


def _mesh(V, F, seed):
    rng = np.random.default_rng(seed)
    v = rng.standard_normal((V, 3)).astype(f32)
    f = rng.integers(0, V, (F, 3)).astype(np.int32)
    if F >= 1 and V >= 3:
        f[0] = (0, 1, 2)
    return v, f


def _batch(case):
    """(verts (vcap, 3), vert offsets, faces (fcap, 3), face offsets, B): one mesh tight in its rows, or three shapes packed
    (the middle one empty) with capacity rows beyond the totals: NaN vertices, faces of -1."""
    K = _K()
    if case == "triangle":
        meshes, pad = [_mesh(3, 1, 1)], 0
    elif case == "block":
        meshes, pad = [_mesh(K + 1, 2 * K - 3, 2)], 0
    else:
        meshes, pad = [_mesh(K // 2 + 3, K + 1, 3), (np.zeros((0, 3), f32), np.zeros((0, 3), np.int32)), _mesh(70, 131, 4)], 6
    v = np.concatenate([m[0] for m in meshes] + [np.full((pad, 3), np.nan, f32)])
    f = np.concatenate([m[1] for m in meshes] + [np.full((pad, 3), -1, np.int32)])
    voff = np.cumsum([0] + [len(m[0]) for m in meshes]).astype(np.int32)
    foff = np.cumsum([0] + [len(m[1]) for m in meshes]).astype(np.int32)
    return v, voff, f, foff, len(meshes)


@pytest.mark.parametrize("flags", [0, 1])
@pytest.mark.parametrize("with_nbr", [True, False])
@pytest.mark.parametrize("case", ["triangle", "block", "packed"])
def test_entries_inside_the_arena(case, with_nbr, flags):
    from nsdp_amd import _lib
    L = _lib.lib()
    v, voff, f, foff, B = _batch(case)
    P, vcap, fcap, live = 2, len(v), len(f), int(voff[-1])
    poses = np.stack([v, (v * f32(1.5))[:, [1, 2, 0]]])
    lo, le, want_nbr, want_len = gr.edge_table(poses, f, foff, voff)
    a = PoisonArena(DEV, 32 << 20)
    tv, tf = a.input("verts", torch.tensor(poses)), a.input("faces", torch.tensor(f))
    tfo, tvo = a.input("face_offsets", torch.tensor(foff)), a.input("vert_offsets", torch.tensor(voff))
    tlo, tle = a.input("list_offsets", torch.tensor(lo)), a.input("list_entries", torch.tensor(le))
    nbr = a.output("nbr", (6 * fcap,), torch.int32) if with_nbr else None
    length = a.output("len", (P, 6 * fcap))
    with a.routed():
        _lib.check(_lib.lib().nsdp_mesh_edge_lengths(_p(tv), _ci(P), _p(tf), _p(tfo), _p(tvo), _ci(B), _ci(vcap), _ci(fcap), _p(tlo),
                                                     _p(tle), _p(nbr), _p(length), _lib.stream_ptr()), "nsdp_mesh_edge_lengths")
    _SEEN.update(a.called)
    a.check(written=[length] + ([nbr] if with_nbr else []))
    assert np.array_equal(length.cpu().numpy().view(np.uint32), want_len.view(np.uint32))      # (a NaN -- poison that was read -- fails this)
    if with_nbr:
        assert np.array_equal(nbr.cpu().numpy(), want_nbr)

    # the relaxation over the table just written (the emulation's neighbours where nbr was not asked for)
    start = np.full((P, vcap), np.nan, f32)                                   # NaN: poison as a start value is +inf
    start[:, [1, (live // 2 + 1) % live]] = [0.0, 0.125]
    start[0, 0], start[1, 0] = -1.0, -0.0
    want = np.stack([gr.dijkstra(lo, want_nbr, want_len[p], start[p], 2.5, live)[0] for p in range(P)])
    b = PoisonArena(DEV, 32 << 20)
    rlo, rnbr = b.input("list_offsets", torch.tensor(lo)), b.input("nbr", torch.tensor(want_nbr))
    rlen, rvo = b.input("len", torch.tensor(want_len)), b.input("vert_offsets", torch.tensor(voff))
    dist = b.accum("dist", torch.tensor(start))
    changed = b.output("changed_out", (1,), torch.int32)
    lowered = None
    for _ in range(vcap // 32 + 2):
        with b.routed():
            _lib.check(_lib.lib().nsdp_mesh_geodesic_relax(_p(rlo), _p(rnbr), _p(rlen), _p(rvo), _ci(B), _ci(vcap), _ci(fcap), _ci(P),
                                                           _cf(2.5), _ci(32), _ci(flags), _p(dist), _p(changed), _lib.stream_ptr()),
                       "nsdp_mesh_geodesic_relax")
        _SEEN.update(b.called)
        b.check(written=[dist, changed])                                       # every row of dist, those beyond the totals too
        lowered = int(changed.item())
        assert lowered >= 0
        if lowered == 0:
            break
    assert lowered == 0
    got = dist.cpu().numpy()
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert (got[:, live:].view(np.uint32) == INF_BITS).all() and (want[0] <= 2.5).sum() >= 2


def test_stale_tables_stay_inside_the_operands():
    """nbr rows and list offsets outside their ranges (a poisoned or stale table) are clamped before they form an address:
    wrong numbers, but nothing outside the operands is read into a fault or written, and the call returns."""
    from nsdp_amd import _lib
    K = _K()
    g = torch.Generator().manual_seed(3)
    lo_i, hi_i = -(1 << 31), (1 << 31) - 1
    B, vcap, fcap, P = 2, K + 40, 500, 2
    nbr = torch.randint(lo_i, hi_i, (6 * fcap,), generator=g, dtype=torch.int64).int()
    nbr[::5], nbr[1::7], nbr[2::11] = -1, vcap, vcap + 5
    nbr[3::4] = torch.randint(0, vcap, (len(nbr[3::4]),), generator=g).int()
    lo = torch.randint(-50, 3 * fcap + 50, (vcap + 1,), generator=g, dtype=torch.int64).int()
    lo[::9], lo[1::13] = -1, 1 << 30
    length = torch.rand((P, 6 * fcap), generator=g)
    length[:, ::17] = float("nan")
    length[:, 1::19] = -1.0
    voff = torch.tensor([-3, 700, 1 << 30], dtype=torch.int32)                # clamped: [0, 700, vcap]
    start = torch.full((P, vcap), float("inf"))
    start[:, ::50] = 0.0
    for flags in (0, 1):
        a = PoisonArena(DEV, 16 << 20)
        tlo, tn, tl, tvo = a.input("list_offsets", lo), a.input("nbr", nbr), a.input("len", length), a.input("vert_offsets", voff)
        dist, changed = a.accum("dist", start), a.output("changed_out", (1,), torch.int32)
        with a.routed():
            _lib.check(_lib.lib().nsdp_mesh_geodesic_relax(_p(tlo), _p(tn), _p(tl), _p(tvo), _ci(B), _ci(vcap), _ci(fcap), _ci(P),
                                                           _cf(float("inf")), _ci(3), _ci(flags), _p(dist), _p(changed),
                                                           _lib.stream_ptr()), "nsdp_mesh_geodesic_relax")
        _SEEN.update(a.called)
        a.check(written=[dist, changed])
        bits = dist.cpu().numpy().view(np.uint32)
        assert (bits <= INF_BITS).all() and 0 <= int(changed.item()) <= P * vcap      # non-negative or +inf: never a NaN, never a sign
        assert (bits[:, ::50] == 0).all()


def test_wrapper_allocates_inside_the_arena():
    """geodesic_distances with the wrapper's own allocations (the table, the start array, the counter) routed through the
    arena: all get guards too."""
    from nsdp_amd import geodesic
    v, f = gr.sphere_with(_K() + 9)
    want = gr.geodesic(v, f, [4])
    for reorder in (False, True):
        plan = geodesic.GeodesicPlan(torch.tensor(f).to(DEV), torch.tensor(v).to(DEV), reorder=reorder)
        a = PoisonArena(DEV, 32 << 20)
        tv = a.input("verts", torch.tensor(v))
        with a.routed(geodesic):
            got = geodesic.geodesic_distances(tv, plan, torch.tensor([4], device=DEV))
        _SEEN.update(a.called)
        assert {"nsdp_mesh_edge_lengths", "nsdp_mesh_geodesic_relax"} <= a.called
        a.check()
        assert np.array_equal(got.cpu().numpy().view(np.uint32), want.view(np.uint32))


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
