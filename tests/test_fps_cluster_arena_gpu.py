"""The launching entries of include/nsdp_sampling.h inside the poisoned arena of tests/poison_arena.py, as
tests/test_eval_batch_arena_gpu.py holds the entries of include/nsdp_eval.h: every operand between 256 KiB guards, the
workspace exactly the bytes the size query declares and poisoned on entry (the call initialises it itself), idx_out -1 until the
kernel writes it, no byte changed outside the two, and the indices those of the oracle.  COVERAGE plays the part of the other
file's table for this header: the last test holds it against the header and against what the recording proxy saw."""
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
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "nsdp_sampling.h")

COVERAGE = {      # the entries that launch; the size queries and the status read are host-side
    "nsdp_furthest_point_sampling_cluster": "test_cluster",
    "nsdp_furthest_point_sampling_cluster_ragged": "test_cluster_ragged",
}
HOST_ONLY = {"nsdp_fps_cluster_groups", "nsdp_fps_cluster_workspace_bytes", "nsdp_fps_cluster_status"}
_SEEN: set = set()


def _call(a, name, *args):
    """One C-ABI call through the arena's recording proxy: tensors as device pointers, int -> int."""
    from nsdp_amd import _lib, pointnet2_utils
    conv = [ctypes.c_void_p(v.data_ptr()) if isinstance(v, torch.Tensor) else ctypes.c_int(int(v)) for v in args]
    with a.routed(pointnet2_utils):
        _lib.check(getattr(_lib.lib(), name)(*conv, _lib.stream_ptr()), name)
    _SEEN.update(a.called)


def _workspace(a, B, n_max, m, G):
    from nsdp_amd import _lib
    fn = _lib.lib().nsdp_fps_cluster_workspace_bytes
    fn.restype = ctypes.c_size_t
    need = int(fn(ctypes.c_int(B), ctypes.c_int(n_max), ctypes.c_int(m), ctypes.c_int(G)))
    assert need > 0
    return a.workspace("workspace", need)


def _status(ws):
    from nsdp_amd import _lib
    return int(_lib.lib().nsdp_fps_cluster_status(ctypes.c_void_p(ws.data_ptr()), _lib.stream_ptr()))


@pytest.mark.parametrize("B,N,m,G", [(2, 513, 77, 3), (1, 8193, 16, 2)])
def test_cluster(B, N, m, G):
    xyz = synth.uniform(N + m, "arena_cloud", (B, N, 3), -0.5, 0.5)
    a = PoisonArena(DEV, 16 << 20)
    txyz = a.input("xyz", torch.from_numpy(xyz))
    ws, idx = _workspace(a, B, N, m, G), a.output("idx", (B, m), torch.int32)
    _call(a, "nsdp_furthest_point_sampling_cluster", txyz, B, N, m, G, ws, idx)
    a.check(written=[idx])
    assert _status(ws) == 0
    np.testing.assert_array_equal(idx.cpu().numpy(), ref.furthest_point_sampling(xyz, m))


def test_cluster_ragged():
    counts, m, G = [300, 0, 700], 40, 2
    cap = sum(counts) + 50
    xyz = synth.uniform(77, "arena_packed", (cap, 3), -0.5, 0.5)
    a = PoisonArena(DEV, 16 << 20)
    txyz = a.input("xyz", torch.from_numpy(xyz))
    toff = a.input("offsets", torch.tensor([0] + list(np.cumsum(counts)), dtype=torch.int32))
    ws, idx = _workspace(a, len(counts), max(counts), m, G), a.output("idx", (len(counts), m), torch.int32)
    _call(a, "nsdp_furthest_point_sampling_cluster_ragged", txyz, toff, len(counts), cap, max(counts), m, G, ws, idx)
    a.check(written=[idx])
    assert _status(ws) == 0
    got, lo = idx.cpu().numpy(), 0
    for b, n in enumerate(counts):
        if n:
            np.testing.assert_array_equal(got[b] - lo, ref.furthest_point_sampling(xyz[None, lo:lo + n], m)[0])
        else:
            assert (got[b] == min(lo, cap - 1)).all()      # (an empty shape: its clamped first row in every slot)
        lo += n


def test_wrappers_allocate_nothing_but_the_declared_outputs():
    """The Python bindings routed through the arena: idx and the workspace (their only allocations) get guards too."""
    from nsdp_amd import pointnet2_utils as pu
    xyz = synth.uniform(78, "arena_wrapped", (1, 9000, 3), -0.5, 0.5)
    a = PoisonArena(DEV, 16 << 20)
    txyz = a.input("xyz", torch.from_numpy(xyz))
    toff = a.input("offsets", torch.tensor([0, 8500, 9000], dtype=torch.int32))
    with a.routed(pu), pu.fps_cluster(True):
        rect = pu.furthest_point_sample(txyz, 24)
        assert pu.fps_cluster_status() == 0
        rag = pu.furthest_point_sample_ragged(txyz[0], toff, 24, 8500)
        assert pu.fps_cluster_status() == 0
    _SEEN.update(a.called)
    a.check(written=[rect, rag])
    np.testing.assert_array_equal(rect.cpu().numpy(), ref.furthest_point_sampling(xyz, 24))
    np.testing.assert_array_equal(rag[0].cpu().numpy(), ref.furthest_point_sampling(xyz[:, :8500], 24)[0])
    np.testing.assert_array_equal(rag[1].cpu().numpy() - 8500, ref.furthest_point_sampling(xyz[:, 8500:], 24)[0])


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
