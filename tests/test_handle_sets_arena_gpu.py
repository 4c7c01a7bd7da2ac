"""The two entries of include/nsdp_handle_sets.h inside the poisoned arena of tests/poison_arena.py, as
tests/test_handles_arena_gpu.py and tests/test_handles_ragged_arena_gpu.py hold the rule kernels: operands between guards in
0xFF-filled memory, every declared output element written, no byte changed outside -- columns 0:3 of the rows and the padding
rows behind offsets[B], which the contract leaves alone, still poison -- and nothing read that nobody wrote: the poison is NaN,
so a label above H that indexed the motion table (255 lands 12 KB behind a table of three motions, inside its guard) or a lane
that read a target it has no business with would show in the comparison with the reference, evaluated on the host from the
arena's inputs.  COVERAGE plays the part of the other files' table for this header."""
import os
import re

import numpy as np
import pytest
import torch

from poison_arena import PoisonArena

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "nsdp_handle_sets.h")

COVERAGE = {"nsdp_handle_set_rows": "test_rows", "nsdp_handle_set_rows_ragged": "test_rows_ragged"}      # both launch
_SEEN: set = set()
PAD = 37
H = 3


def _operands(B, n, T, seed):
    """src, labels (0..H, H + 1 and 255 all present), motions [T, B, H, 12], targets [T, B, n, 3] -- on the host."""
    g = torch.Generator().manual_seed(seed)
    src = torch.rand(B, n, 3, generator=g) - 0.5
    labels = torch.randint(0, H + 2, (B, n), generator=g).to(torch.uint8)
    labels.view(-1)[torch.randperm(B * n, generator=g)[:max(1, B * n // 8)]] = 255
    return src, labels, torch.rand(T, B, H, 12, generator=g) - 0.5, torch.rand(T, B, n, 3, generator=g) - 0.5


def _want(src, labels, motions, targets, form):
    from nsdp_amd.edit import reference_pose_dict
    T = motions.shape[0]
    dds = [reference_pose_dict(src, None, labels, H, motions=motions[t] if form == "motions" else None,
                               targets=targets[t] if form == "targets" else None) for t in range(T)]
    return (torch.stack([d["verts_tgt"] for d in dds]), torch.stack([d["surface_samples_inputs"][:, :, 3:7] for d in dds]),
            dds[0]["cano_handle_sample_idx"].to(torch.uint8))


def _same_bits(got, want):
    return torch.equal(got.cpu().contiguous().view(torch.int32), want.contiguous().view(torch.int32))


@pytest.mark.parametrize("form", ["motions", "targets"])
@pytest.mark.parametrize("B,n,T", [(1, 1, 1), (3, 257, 2), (2, 4097, 3)])
def test_rows(B, n, T, form):
    from nsdp_amd import pointnet2_utils as pu
    src, labels, motions, targets = _operands(B, n, T, 100 * n + T)
    if B * n >= 8:
        assert set(range(H + 2)) | {255} <= set(labels.unique().tolist())
    a = PoisonArena(DEV, 16 << 20)
    tsrc, tlab = a.input("src", src), a.input("labels", labels)
    kw = {form: a.input(form, motions if form == "motions" else targets)}      # (the other one is null: it has no memory to read)
    rows, tgt = a.output("rows", (T, B, n, 7)), a.output("tgt", (T, B, n, 3))
    ho = a.output("handle_out", (B, n), torch.uint8)
    with a.routed(pu):
        pu.handle_set_rows(tsrc, tlab, rows, tgt=tgt, handle_out=ho, **kw)
    _SEEN.update(a.called)
    assert "nsdp_handle_set_rows" in a.called
    a.check(written=[rows[..., 3:7], tgt, ho])      # no stray write; every declared element written
    poison = torch.full((1,), -1, dtype=torch.int32, device=DEV)
    assert bool((rows[..., 0:3].contiguous().view(torch.int32) == poison).all()), "columns 0:3 were written"
    want_tgt, want_cols, want_handle = _want(src, labels, motions, targets, form)
    assert torch.equal(ho.cpu(), want_handle)
    assert _same_bits(tgt, want_tgt) and _same_bits(rows[..., 3:7], want_cols)
    assert not bool(torch.isnan(tgt).any()), "a target made of memory nobody wrote"


@pytest.mark.parametrize("form", ["motions", "targets"])
@pytest.mark.parametrize("counts", [(1, 1, 1), (257, 0, 1025), (63, 64, 65)])
def test_rows_ragged(counts, form):
    from nsdp_amd import pointnet2_utils as pu
    B, total = len(counts), sum(counts)
    cap = total + PAD
    src, labels, motions, targets = _operands(1, cap, 1, 7 + total)
    src, labels, targets = src[0], labels[0], targets[0, 0]
    g = torch.Generator().manual_seed(total)
    motions = torch.rand(B, H, 12, generator=g) - 0.5
    offsets = torch.tensor(np.concatenate([[0], np.cumsum(counts)]), dtype=torch.int32)
    a = PoisonArena(DEV, 16 << 20)
    # of the cap rows of every operand the call may read and touch the first `total`: the inputs' padding rows are poison
    psrc, ptgts = src.clone(), targets.clone()
    psrc[total:], ptgts[total:] = float("nan"), float("nan")
    tsrc, tlab, toff = a.input("src", psrc), a.input("labels", labels), a.input("offsets", offsets)
    kw = {form: a.input(form, motions if form == "motions" else ptgts)}
    rows, tgt = a.output("rows", (cap, 7), rows=total), a.output("tgt", (cap, 3), rows=total)
    ho = a.output("handle_out", (cap,), torch.uint8, rows=total)
    with a.routed(pu):
        pu.handle_set_rows_ragged(tsrc, toff, tlab, rows, tgt=tgt, handle_out=ho, **kw)
    _SEEN.update(a.called)
    assert "nsdp_handle_set_rows_ragged" in a.called
    a.check(written=[rows[:total, 3:7], tgt[:total], ho[:total]])
    poison = torch.full((1,), -1, dtype=torch.int32, device=DEV)
    assert bool((rows[:, 0:3].contiguous().view(torch.int32) == poison).all()), "columns 0:3 were written"
    assert bool((rows[total:].contiguous().view(torch.int32) == poison).all()), "rows behind the B shapes were written"
    # the reference, shape by shape (each shape reads its own motion table)
    from nsdp_amd.edit import reference_pose_dict
    lo = 0
    for b, nb in enumerate(counts):
        if nb:
            dd = reference_pose_dict(src[None, lo:lo + nb], None, labels[None, lo:lo + nb], H,
                                     motions=motions[b:b + 1] if form == "motions" else None,
                                     targets=targets[None, lo:lo + nb] if form == "targets" else None)
            assert torch.equal(ho[lo:lo + nb].cpu(), dd["cano_handle_sample_idx"][0].to(torch.uint8)), b
            assert _same_bits(tgt[lo:lo + nb], dd["verts_tgt"][0]), b
            assert _same_bits(rows[lo:lo + nb, 3:7], dd["surface_samples_inputs"][0, :, 3:7]), b
        lo += nb
    assert not bool(torch.isnan(tgt[:total]).any())


@pytest.mark.parametrize("form", ["motions", "targets"])
def test_rows_without_the_optional_outputs(form):
    from nsdp_amd import pointnet2_utils as pu
    B, n, T = 2, 300, 2
    src, labels, motions, targets = _operands(B, n, T, 5)
    a = PoisonArena(DEV, 16 << 20)
    tsrc, tlab = a.input("src", src), a.input("labels", labels)
    kw = {form: a.input(form, motions if form == "motions" else targets)}
    rows = a.output("rows", (T, B, n, 7))
    with a.routed(pu):
        pu.handle_set_rows(tsrc, tlab, rows, **kw)
    _SEEN.update(a.called)
    a.check(written=[rows[..., 3:7]])
    assert _same_bits(rows[..., 3:7], _want(src, labels, motions, targets, form)[1])
    assert len(a.regions) == 4      # src, labels, the motions or targets, rows: the wrapper allocates nothing


def test_every_entry_of_the_header_is_called_inside_the_arena():
    """Last in the file: the table against the header, and against what the recording proxy saw in the tests above."""
    with open(HEADER) as f:
        text = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    declared = set(re.findall(r"\b(nsdp_[a-z0-9_]+)\s*\(", text))
    assert declared == set(COVERAGE), sorted(declared ^ set(COVERAGE))
    for entry, test in COVERAGE.items():
        assert callable(globals().get(test)), f"{entry}: no test function {test}"
    if _SEEN:                                                             # (run alone, this test has nothing to compare)
        assert set(COVERAGE) <= _SEEN, sorted(set(COVERAGE) - _SEEN)
