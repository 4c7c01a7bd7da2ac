"""The launching entries of include/nsdp_handles.h inside the poisoned arena of tests/poison_arena.py, as
tests/test_invert_wide_arena_gpu.py holds the entry of include/nsdp_scatter.h: inputs between guards, the workspace exactly the
bytes the size query declares and poisoned on entry (the call writes every word it reads), every declared output element
written, no byte changed outside -- and columns 0:3 of the [B, n, 7] rows, which the contract leaves alone, still poison.
COVERAGE plays the part of the other file's table for this header."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from poison_arena import PoisonArena

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "nsdp_handles.h")

COVERAGE = {"nsdp_handle_bounds": "test_bounds", "nsdp_handle_rows": "test_rows"}      # the entries that launch
HOST_ONLY = {"nsdp_handle_bounds_workspace_bytes"}
_SEEN: set = set()


def _cloud(B, n, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(B, n, 3, generator=g) - 0.5, torch.rand(B, n, 3, generator=g) - 0.5


def _bounds(a, tcano, B, n):
    from nsdp_amd import _lib, pointnet2_utils as pu
    fn = _lib.lib().nsdp_handle_bounds_workspace_bytes
    fn.restype = ctypes.c_size_t
    need = int(fn(ctypes.c_int(B), ctypes.c_int(n)))
    assert need > 0
    ws = a.workspace("workspace", need)
    out = a.output("bounds", (B, 6))
    with a.routed(pu):
        _lib.check(_lib.lib().nsdp_handle_bounds(ctypes.c_void_p(tcano.data_ptr()), ctypes.c_int(B), ctypes.c_int(n),
                                                 ctypes.c_void_p(ws.data_ptr()), ctypes.c_void_p(out.data_ptr()),
                                                 _lib.stream_ptr()), "nsdp_handle_bounds")
    _SEEN.update(a.called)
    a.check(written=[out, ws])      # (every word of the declared workspace is a partial some workgroup wrote)
    return out


@pytest.mark.parametrize("B,n", [(3, 1), (2, 4097), (1, 70000)])
def test_bounds(B, n):
    cano, _ = _cloud(B, n, n)
    a = PoisonArena(DEV, 16 << 20)
    out = _bounds(a, a.input("cano", cano), B, n)
    want = torch.cat([cano.amin(dim=1), cano.amax(dim=1)], dim=1)
    assert torch.equal(out.cpu(), want)


def test_bounds_wrapper_allocates_nothing_but_the_output_and_the_workspace():
    from nsdp_amd import pointnet2_utils as pu
    cano, _ = _cloud(2, 9000, 3)
    a = PoisonArena(DEV, 16 << 20)
    tcano = a.input("cano", cano)
    with a.routed(pu):
        out = pu.handle_bounds(tcano)
    _SEEN.update(a.called)
    assert "nsdp_handle_bounds" in a.called and len(a.regions) == 3      # cano, the workspace, the bounds
    a.check(written=[out, a.regions[1].tensor])
    assert torch.equal(out.cpu(), torch.cat([cano.amin(dim=1), cano.amax(dim=1)], dim=1))


@pytest.mark.parametrize("masks", [False, True])
@pytest.mark.parametrize("B,n", [(3, 1), (2, 1025)])
def test_rows(B, n, masks):
    from nsdp_amd import pointnet2_utils as pu
    from nsdp_amd.edit import pack_params
    cano, src = _cloud(B, n, 7 + n)
    a = PoisonArena(DEV, 16 << 20)
    tcano, tsrc = a.input("cano", cano), a.input("src", src)
    tb = a.input("bounds", torch.cat([cano.amin(dim=1), cano.amax(dim=1)], dim=1))
    words = pack_params(B, ["head", "tail", "frontleftfoot"][:B], (-0.15, -0.2, 0.2), 0.1, False)
    tp = a.input("params", torch.from_numpy(words))
    g = torch.Generator().manual_seed(n)
    hm = a.input("handle_mask", (torch.rand(B, n, generator=g) < 0.5).to(torch.uint8)) if masks else None
    mm = a.input("move_mask", (torch.rand(B, n, generator=g) < 0.5).to(torch.uint8)) if masks else None
    # rows: B + 1 shapes of which the call may touch the first B; tgt and the two flag outputs written whole
    rows = a.output("rows", (B + 1, n, 7), rows=B)
    tgt = a.output("tgt", (B, n, 3))
    ho, mo = a.output("handle_out", (B, n), torch.uint8), a.output("move_out", (B, n), torch.uint8)
    with a.routed(pu):
        pu.handle_rows(tcano, tsrc, tb, tp, rows[:B], hm, mm, tgt=tgt, handle_out=ho, move_out=mo)
    _SEEN.update(a.called)
    assert "nsdp_handle_rows" in a.called
    a.check(written=[rows[:B, :, 3:7], tgt])      # no stray write; every declared element written
    poison = torch.full((1,), -1, dtype=torch.int32, device=DEV)
    assert bool((rows[:B, :, 0:3].contiguous().view(torch.int32) == poison).all()), "columns 0:3 were written"
    assert bool((rows[B:].contiguous().view(torch.int32) == poison).all()), "rows behind the B shapes were written"
    assert bool((ho <= 1).all()) and bool((mo <= 1).all())      # (a flag byte still holding the poison would be 0xFF)
    if masks:
        assert torch.equal(ho, hm) and torch.equal(mo, mm)
    h, m = ho.cpu().float()[:, :, None], mo.cpu().float()[:, :, None]
    d = torch.from_numpy(words.view(np.float32)[:, 3:6].copy())[:, None, :]
    want_tgt = src + d * m
    assert torch.equal(tgt.cpu(), want_tgt)
    assert torch.equal(rows[:B, :, 3:7].cpu(), torch.cat([want_tgt * h, h], dim=-1))


def test_rows_without_the_optional_outputs():
    from nsdp_amd import pointnet2_utils as pu
    from nsdp_amd.edit import pack_params
    B, n = 2, 257
    cano, src = _cloud(B, n, 5)
    a = PoisonArena(DEV, 16 << 20)
    tcano, tsrc = a.input("cano", cano), a.input("src", src)
    tb = a.input("bounds", torch.cat([cano.amin(dim=1), cano.amax(dim=1)], dim=1))
    tp = a.input("params", torch.from_numpy(pack_params(B, "behindrightfoot", (0.1, 0.2, 0.3), 0.2, True)))
    rows = a.output("rows", (B, n, 7))
    with a.routed(pu):
        pu.handle_rows(tcano, tsrc, tb, tp, rows)
    _SEEN.update(a.called)
    a.check(written=[rows[:, :, 3:7]])


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
