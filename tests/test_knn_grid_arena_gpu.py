"""The launching entries of include/nsdp_search.h inside the poisoned arena of tests/poison_arena.py, as
tests/test_fps_cluster_arena_gpu.py holds the entries of include/nsdp_sampling.h: every operand between 256 KiB guards, the
workspace exactly the bytes the size query declares and poisoned on entry (the call initialises it itself), idx_out / dist_out
poisoned until the kernel writes them, no byte changed outside the three, and the results those of the oracle.  COVERAGE plays the
part of the other file's table for this header: the last test holds it against the header and against what the recording proxy
saw.  (Non-finite coordinates and corrupt offsets are held by construction -- csrc/knn_grid.hip clamps every cell coordinate as
a float and every offset and slot as ragged.h does -- not by a run.)"""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from nsdp_amd import synth
from oracle import pointnet2_ref as ref
from poison_arena import PoisonArena

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "nsdp_search.h")
FLT_MAX = np.finfo(np.float32).max

COVERAGE = {      # the entries that launch; the size query and the stats read are host-side
    "nsdp_knn_grid": "test_grid",
    "nsdp_knn_grid_ragged_source": "test_grid_ragged_source",
}
HOST_ONLY = {"nsdp_knn_grid_workspace_bytes", "nsdp_knn_grid_stats"}
_SEEN: set = set()


def _call(a, name, *args):
    """One C-ABI call through the arena's recording proxy: tensors as device pointers, None as NULL, int -> int."""
    from nsdp_amd import _lib, pointnet2_utils
    conv = [ctypes.c_void_p(v.data_ptr()) if isinstance(v, torch.Tensor) else ctypes.c_void_p(0) if v is None else ctypes.c_int(int(v))
            for v in args]
    with a.routed(pointnet2_utils):
        _lib.check(getattr(_lib.lib(), name)(*conv, _lib.stream_ptr()), name)
    _SEEN.update(a.called)


def _workspace(a, B, queries, rows, m_max):
    from nsdp_amd import _lib
    fn = _lib.lib().nsdp_knn_grid_workspace_bytes
    fn.restype = ctypes.c_size_t
    need = int(fn(ctypes.c_int(B), ctypes.c_int(queries), ctypes.c_int(rows), ctypes.c_int(m_max)))
    assert need > 0
    return a.workspace("workspace", need)


def _stats(ws):
    from nsdp_amd import _lib
    out = (ctypes.c_int64 * 4)()
    assert _lib.lib().nsdp_knn_grid_stats(ctypes.c_void_p(ws.data_ptr()), _lib.stream_ptr(), out) == 0
    return list(out)


def _bits(t):
    return t.cpu().numpy().view(np.int32)


@pytest.mark.parametrize("B,n,m,k,own", [(2, 513, 513, 16, True), (1, 77, 1025, 7, False)])
def test_grid(B, n, m, k, own):
    source = synth.uniform(n + m, "arena_source", (B, m, 3), -0.5, 0.5)
    query = source if own else synth.uniform(n + m + 1, "arena_query", (B, n, 3), -0.7, 0.7)
    a = PoisonArena(DEV, 16 << 20)
    tsrc = a.input("source", torch.from_numpy(source))
    tq = tsrc if own else a.input("query", torch.from_numpy(query))      # (the self-search: one operand, taken in cell order)
    ws = _workspace(a, B, B * n, B * m, m)
    idx, d2 = a.output("idx", (B, n, k), torch.int32), a.output("dist", (B, n, k), torch.float32)
    _call(a, "nsdp_knn_grid", tq, tsrc, B, n, m, k, ws, idx, d2)
    a.check(written=[idx, d2])
    assert _stats(ws)[0] == B * n
    want_idx, want_d = ref.knn(query, source, k, return_dist=True)
    np.testing.assert_array_equal(idx.cpu().numpy(), want_idx)
    np.testing.assert_array_equal(_bits(d2), want_d.view(np.int32))


@pytest.mark.parametrize("queries", ["packed", "rectangular"])
def test_grid_ragged_source(queries):
    counts, k, n = [300, 0, 700], 16, 40
    B, total = len(counts), sum(counts)
    cap = total + 50
    xyz = synth.uniform(79, "arena_packed", (cap, 3), -0.5, 0.5)
    a = PoisonArena(DEV, 16 << 20)
    txyz = a.input("xyz", torch.from_numpy(xyz))
    toff = a.input("offsets", torch.tensor([0] + list(np.cumsum(counts)), dtype=torch.int32))
    if queries == "packed":
        q, tq, tqoff, rows = None, txyz, toff, cap
        idx, d2 = a.output("idx", (cap, k), torch.int32, rows=total), a.output("dist", (cap, k), torch.float32, rows=total)
    else:
        q = synth.uniform(80, "arena_rect", (B, n, 3), -0.7, 0.7)
        tq, tqoff, rows = a.input("query", torch.from_numpy(q)), None, B * n
        idx, d2 = a.output("idx", (B, n, k), torch.int32), a.output("dist", (B, n, k), torch.float32)
    ws = _workspace(a, B, rows, cap, max(counts))
    _call(a, "nsdp_knn_grid_ragged_source", tq, tqoff, txyz, toff, B, 0 if queries == "packed" else n, cap if queries == "packed" else 0,
          cap, max(counts), k, ws, idx, d2)
    a.check(written=[idx[:total], d2[:total]] if queries == "packed" else [idx, d2])
    got_idx, got_d, lo = idx.cpu().numpy(), d2.cpu().numpy(), 0
    for b, cnt in enumerate(counts):
        rows_q = xyz[None, lo:lo + cnt] if queries == "packed" else q[b:b + 1]
        mine = (got_idx[lo:lo + cnt], got_d[lo:lo + cnt]) if queries == "packed" else (got_idx[b], got_d[b])
        if cnt:
            want_idx, want_d = ref.knn(rows_q, xyz[None, lo:lo + cnt], k, return_dist=True)
            np.testing.assert_array_equal(mine[0] - lo, want_idx[0])
            np.testing.assert_array_equal(mine[1].view(np.int32), want_d[0].view(np.int32))
        elif queries == "rectangular":      # (a shape without rows: its clamped first row and FLT_MAX in every slot)
            assert (mine[0] == min(lo, cap - 1)).all() and (mine[1] == FLT_MAX).all()
        lo += cnt


def test_wrappers_allocate_nothing_but_the_declared_outputs():
    """The Python bindings routed through the arena: the outputs and the workspace (their only allocations) get guards too."""
    from nsdp_amd import pointnet2_utils as pu
    xyz = synth.uniform(81, "arena_wrapped", (1, 1000, 3), -0.5, 0.5)
    a = PoisonArena(DEV, 16 << 20)
    txyz = a.input("xyz", torch.from_numpy(xyz))
    toff = a.input("offsets", torch.tensor([0, 600, 1000], dtype=torch.int32))
    with a.routed(pu), pu.knn_grid_mode("force"):
        rect_idx, rect_d = pu.knn(txyz, txyz, 16, return_dist=True)                     # (through the dispatch)
        assert pu.knn_grid_stats()["queries"] == 1000
        rag_idx, rag_d = pu.knn_ragged_source(txyz[0], txyz[0], toff, 10, 600, query_offsets=toff, return_dist=True)
        assert pu.knn_grid_stats()["queries"] == 1000
    _SEEN.update(a.called)
    a.check(written=[rect_idx, rect_d, rag_idx, rag_d])
    want_idx, want_d = ref.knn(xyz, xyz, 16, return_dist=True)
    np.testing.assert_array_equal(rect_idx.cpu().numpy(), want_idx)
    np.testing.assert_array_equal(_bits(rect_d), want_d.view(np.int32))
    for lo, hi in ((0, 600), (600, 1000)):
        want_idx, want_d = ref.knn(xyz[:, lo:hi], xyz[:, lo:hi], 10, return_dist=True)
        np.testing.assert_array_equal(rag_idx[lo:hi].cpu().numpy() - lo, want_idx[0])
        np.testing.assert_array_equal(_bits(rag_d[lo:hi]), want_d[0].view(np.int32))


def test_every_launching_entry_of_the_header_is_called_inside_the_arena():
    """Last in the file: the table against the header, and against what the recording proxy saw in the tests above."""
    with open(HEADER) as f:
        text = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    declared = set(re.findall(r"\b(nsdp_[a-z0-9_]+)\s*\(", text))
    assert declared == set(COVERAGE) | HOST_ONLY, sorted(declared ^ (set(COVERAGE) | HOST_ONLY))
    for entry, test in COVERAGE.items():
        assert callable(globals().get(test)), f"{entry}: no test function {test}"
    if _SEEN:                                                             # (run alone, this test has nothing to compare)
        assert set(COVERAGE) <= _SEEN, sorted(set(COVERAGE) - _SEEN)
