"""The launching entries of include/nsdp_handles_ragged.h inside the poisoned arena of tests/poison_arena.py, as
tests/test_handles_arena_gpu.py holds the rectangular ones: inputs between guards, the workspace exactly the bytes the size query
declares and poisoned on entry (the call writes every word it reads), every declared output element of the B shapes written, no
byte changed outside -- the padding rows behind offsets[B] and columns 0:3 of the [cap, 7] rows, which the contract leaves
alone, still poison.  COVERAGE plays the part of the other file's table for this header."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from poison_arena import PoisonArena

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "nsdp_handles_ragged.h")

COVERAGE = {"nsdp_handle_bounds_ragged": "test_bounds", "nsdp_handle_rows_ragged": "test_rows"}      # the entries that launch
HOST_ONLY = {"nsdp_handle_bounds_ragged_workspace_bytes"}
_SEEN: set = set()
PAD = 37


def _cloud(counts, seed):
    g = torch.Generator().manual_seed(seed)
    cap = sum(counts) + PAD
    offsets = torch.tensor(np.concatenate([[0], np.cumsum(counts)]), dtype=torch.int32)
    return cap, offsets, torch.rand(cap, 3, generator=g) - 0.5, torch.rand(cap, 3, generator=g) - 0.5


def _want_bounds(cano, counts):
    out, lo = [], 0
    for n in counts:
        if n:
            out.append(torch.cat([cano[lo:lo + n].amin(dim=0), cano[lo:lo + n].amax(dim=0)]))
        else:      # the identities of the two reductions, by their bits
            out.append(torch.tensor([0x7FFFFFFF] * 3 + [-1] * 3, dtype=torch.int32).view(torch.float32))
        lo += n
    return torch.stack(out)


# `real`: every partial workgroup owns a row of its shape, so no word the call writes is an identity of the reductions.  The
# identity of the maximum (and, as a key, of the minimum) is the word 0xffffffff -- the arena's poison -- so where a shape is
# empty or shorter than its grid the test refills the workspace and the output with ANOTHER pattern before the call and asks
# that no word still holds it afterwards.
OTHER = 0x55555555


@pytest.mark.parametrize("counts,n_max,real", [((1, 1, 1), 1, True), ((70000,), 70000, True), ((600, 5000), 9000, True),
                                               ((4097, 0, 300), 4097, False), ((300, 5000), 9000, False)])
def test_bounds(counts, n_max, real):
    from nsdp_amd import _lib, pointnet2_utils as pu
    B = len(counts)
    cap, offsets, cano, _ = _cloud(counts, n_max)
    a = PoisonArena(DEV, 16 << 20)
    tcano, toff = a.input("cano", cano), a.input("offsets", offsets)
    fn = _lib.lib().nsdp_handle_bounds_ragged_workspace_bytes
    fn.restype = ctypes.c_size_t
    need = int(fn(ctypes.c_int(B), ctypes.c_int(cap), ctypes.c_int(n_max)))
    assert need == B * -(-n_max // 4096) * 6 * 4
    ws = a.workspace("workspace", need)
    out = a.output("bounds", (B, 6))
    if not real:
        ws.view(torch.int32).fill_(OTHER)
        out.view(torch.int32).fill_(OTHER)
    with a.routed(pu):
        _lib.check(_lib.lib().nsdp_handle_bounds_ragged(ctypes.c_void_p(tcano.data_ptr()), ctypes.c_void_p(toff.data_ptr()),
                                                        ctypes.c_int(B), ctypes.c_int(cap), ctypes.c_int(n_max),
                                                        ctypes.c_void_p(ws.data_ptr()), ctypes.c_void_p(out.data_ptr()),
                                                        _lib.stream_ptr()), "nsdp_handle_bounds_ragged")
    _SEEN.update(a.called)
    if real:
        a.check(written=[out, ws])      # (every word of the declared workspace is a partial some workgroup wrote)
    else:
        a.check()
        assert not bool((ws.view(torch.int32) == OTHER).any()) and not bool((out.view(torch.int32) == OTHER).any()), "never written"
    assert torch.equal(out.cpu().view(torch.int32), _want_bounds(cano, counts).view(torch.int32))


def test_bounds_wrapper_allocates_nothing_but_the_output_and_the_workspace():
    from nsdp_amd import pointnet2_utils as pu
    counts = (9000, 600)      # (every partial workgroup of the 3 per shape owns a row: no identity word, which is the poison's)
    cap, offsets, cano, _ = _cloud(counts, 3)
    a = PoisonArena(DEV, 16 << 20)
    tcano, toff = a.input("cano", cano), a.input("offsets", offsets)
    with a.routed(pu):
        out = pu.handle_bounds_ragged(tcano, toff, max(counts))
    _SEEN.update(a.called)
    assert "nsdp_handle_bounds_ragged" in a.called and len(a.regions) == 4      # cano, offsets, the workspace, the bounds
    a.check(written=[out, a.regions[2].tensor])
    assert torch.equal(out.cpu(), _want_bounds(cano, counts))


@pytest.mark.parametrize("masks", [False, True])
@pytest.mark.parametrize("counts", [(1, 1, 1), (257, 0, 1025), (63, 64, 65)])
def test_rows(counts, masks):
    from nsdp_amd import pointnet2_utils as pu
    from nsdp_amd.edit import pack_params
    B, total = len(counts), sum(counts)
    cap, offsets, cano, src = _cloud(counts, 7 + total)
    a = PoisonArena(DEV, 16 << 20)
    tcano, tsrc, toff = a.input("cano", cano), a.input("src", src), a.input("offsets", offsets)
    bounds = _want_bounds(cano, counts)
    tb = a.input("bounds", bounds)
    words = pack_params(B, ["head", "tail", "frontleftfoot"], [(-0.15, -0.2, 0.2), (0.1, 0.0, -0.3), (0.25, 0.5, -1.0)], 0.1, False)
    tp = a.input("params", torch.from_numpy(words))
    g = torch.Generator().manual_seed(total)
    hm = a.input("handle_mask", (torch.rand(cap, generator=g) < 0.5).to(torch.uint8)) if masks else None
    mm = a.input("move_mask", (torch.rand(cap, generator=g) < 0.5).to(torch.uint8)) if masks else None
    # of the cap rows the call may touch the first `total`: the rows of the B shapes
    rows = a.output("rows", (cap, 7), rows=total)
    tgt = a.output("tgt", (cap, 3), rows=total)
    ho, mo = a.output("handle_out", (cap,), torch.uint8, rows=total), a.output("move_out", (cap,), torch.uint8, rows=total)
    with a.routed(pu):
        pu.handle_rows_ragged(tcano, tsrc, toff, tb, tp, rows, hm, mm, tgt=tgt, handle_out=ho, move_out=mo)
    _SEEN.update(a.called)
    assert "nsdp_handle_rows_ragged" in a.called
    a.check(written=[rows[:total, 3:7], tgt[:total], ho[:total], mo[:total]])      # no stray write; every declared element written
    poison = torch.full((1,), -1, dtype=torch.int32, device=DEV)
    assert bool((rows[:, 0:3].contiguous().view(torch.int32) == poison).all()), "columns 0:3 were written"
    assert bool((rows[total:].contiguous().view(torch.int32) == poison).all()), "rows behind the B shapes were written"
    assert bool((ho[:total] <= 1).all()) and bool((mo[:total] <= 1).all())      # (a flag byte still holding the poison would be 0xFF)
    if masks:
        assert torch.equal(ho[:total], hm[:total]) and torch.equal(mo[:total], mm[:total])
    shape = torch.repeat_interleave(torch.arange(B), torch.tensor(counts))
    h, m = ho[:total].cpu().float()[:, None], mo[:total].cpu().float()[:, None]
    d = torch.from_numpy(words.view(np.float32)[:, 3:6].copy())[shape]
    want_tgt = src[:total] + d * m
    assert torch.equal(tgt[:total].cpu(), want_tgt)
    assert torch.equal(rows[:total, 3:7].cpu(), torch.cat([want_tgt * h, h], dim=-1))
    if not masks:      # the rule's handle, from the shape's own bounds
        lo, r = bounds[shape], float(np.float32(0.1))
        y, z = cano[:total, 1], cano[:total, 2]
        handle = (y < lo[:, 1] + r) | (y > lo[:, 4] - r) | (z < lo[:, 2] + r)
        assert torch.equal(ho[:total].cpu().bool(), handle)


def test_rows_without_the_optional_outputs():
    from nsdp_amd import pointnet2_utils as pu
    from nsdp_amd.edit import pack_params
    counts = (257, 130)
    total = sum(counts)
    cap, offsets, cano, src = _cloud(counts, 5)
    a = PoisonArena(DEV, 16 << 20)
    tcano, tsrc, toff = a.input("cano", cano), a.input("src", src), a.input("offsets", offsets)
    tb = a.input("bounds", _want_bounds(cano, counts))
    tp = a.input("params", torch.from_numpy(pack_params(2, "behindrightfoot", (0.1, 0.2, 0.3), 0.2, True)))
    rows = a.output("rows", (cap, 7), rows=total)
    with a.routed(pu):
        pu.handle_rows_ragged(tcano, tsrc, toff, tb, tp, rows)
    _SEEN.update(a.called)
    a.check(written=[rows[:total, 3:7]])


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
