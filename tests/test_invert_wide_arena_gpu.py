"""The launching entry of include/nsdp_scatter.h inside the poisoned arena of tests/poison_arena.py, as
tests/test_knn_grid_arena_gpu.py holds the entries of include/nsdp_search.h: the index tensor between guards, the workspace
exactly the bytes the size query declares and poisoned on entry (the call initialises it itself), offsets / entries poisoned
until the kernels write them, no byte changed outside the three, and the lists those of the stable sort.  One call carries
indices outside [0, N): they are clamped before they form an address, so nothing outside changes and the lists stay complete.
COVERAGE plays the part of the other file's table for this header."""
import ctypes
import os
import re

import pytest
import torch

from poison_arena import PoisonArena

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "nsdp_scatter.h")

COVERAGE = {"nsdp_knn_invert_wide": "test_invert_wide"}      # the entry that launches; the size query is host-side
HOST_ONLY = {"nsdp_knn_invert_wide_workspace_bytes"}
_SEEN: set = set()


def _call(a, tidx, B, E, N):
    from nsdp_amd import _lib, hip_attention
    fn = _lib.lib().nsdp_knn_invert_wide_workspace_bytes
    fn.restype = ctypes.c_size_t
    need = int(fn(ctypes.c_int(B), ctypes.c_int(E), ctypes.c_int(N)))
    assert need > 0
    ws = a.workspace("workspace", need)
    off, ent = a.output("offsets", (B, N + 1), torch.int32), a.output("entries", (B, E), torch.int32)
    with a.routed(hip_attention):
        _lib.check(_lib.lib().nsdp_knn_invert_wide(ctypes.c_void_p(tidx.data_ptr()), ctypes.c_int(B), ctypes.c_int(E), ctypes.c_int(N),
                                                   ctypes.c_void_p(ws.data_ptr()), ctypes.c_void_p(off.data_ptr()),
                                                   ctypes.c_void_p(ent.data_ptr()), _lib.stream_ptr()), "nsdp_knn_invert_wide")
    _SEEN.update(a.called)
    a.check(written=[off, ent])
    return off.cpu(), ent.cpu()


def _truth(flat, N):
    ent = torch.sort(flat.long(), dim=1, stable=True).indices.int()
    off = torch.zeros(flat.shape[0], N + 1, dtype=torch.int64)
    for b in range(flat.shape[0]):
        off[b, 1:] = torch.cumsum(torch.bincount(flat[b].long(), minlength=N), 0)
    return off.int(), ent


@pytest.mark.parametrize("B,n,N,k", [(2, 300, 700, 16), (1, 1100, 33000, 3)])
def test_invert_wide(B, n, N, k):
    g = torch.Generator().manual_seed(n + N)
    idx = torch.randint(0, N, (B, n, k), generator=g, dtype=torch.int32)
    idx[:, :, 0] = 5
    a = PoisonArena(DEV, 16 << 20)
    tidx = a.input("idx", idx)
    off, ent = _call(a, tidx, B, n * k, N)
    want_off, want_ent = _truth(idx.reshape(B, -1), N)
    assert torch.equal(off, want_off) and torch.equal(ent, want_ent)


def test_invert_wide_clamps_indices_outside_the_sources():
    B, n, N, k = 2, 300, 700, 16
    g = torch.Generator().manual_seed(9)
    idx = torch.randint(0, N, (B, n, k), generator=g, dtype=torch.int32)
    flat = idx.reshape(B, -1)
    flat[0, 3] = flat[1, 1000] = flat[1, 4799] = -1
    flat[0, 0] = flat[0, 2222] = flat[1, 17] = N + 7
    flat[1, 18] = -(1 << 31)
    flat[0, 19] = (1 << 31) - 1
    a = PoisonArena(DEV, 16 << 20)
    tidx = a.input("idx", idx)
    off, ent = _call(a, tidx, B, n * k, N)
    assert bool((off[:, N] == n * k).all()) and bool((off[:, 0] == 0).all())
    want_off, want_ent = _truth(flat.clamp(0, N - 1), N)      # (an index outside counts for the nearest source)
    assert torch.equal(off, want_off) and torch.equal(ent, want_ent)


def test_wrapper_allocates_nothing_but_the_outputs_and_the_workspace():
    """hip_attention.inverse_lists routed through the arena: its three allocations get guards too."""
    from nsdp_amd import hip_attention as ha
    B, n, N, k = 1, 640, 9000, 16
    g = torch.Generator().manual_seed(4)
    idx = torch.randint(0, N, (B, n, k), generator=g, dtype=torch.int32)
    a = PoisonArena(DEV, 16 << 20)
    tidx = a.input("idx", idx)
    with a.routed(ha), ha.invert_wide_mode("1"):
        off, ent = ha.inverse_lists(tidx, N)
    _SEEN.update(a.called)
    assert "nsdp_knn_invert_wide" in a.called and "nsdp_knn_invert" not in a.called
    a.check(written=[off, ent])
    want_off, want_ent = _truth(idx.reshape(B, -1), N)
    assert torch.equal(off.cpu(), want_off) and torch.equal(ent.cpu(), want_ent)


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
