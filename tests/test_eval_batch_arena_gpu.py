"""The three entries of include/nsdp_eval.h inside the poisoned arena of tests/poison_arena.py, as
tests/test_poisoned_arena_gpu.py holds the entries of include/nsdp_hip.h: every operand between 256 KiB guards, outputs NaN /
-1 until the kernel writes them (the split search combines its partial minima IN the output: it must initialise it itself),
no byte changed outside the outputs, rows a packed set leaves alone still poisoned, and the results those of the k = 1
searches / the float64 mean.  COVERAGE plays the part of the other file's table for this header: the last test holds it
against the header and against what the recording proxy saw."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from poison_arena import PoisonArena

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "nsdp_eval.h")
FLT_MAX = float(np.finfo(np.float32).max)

COVERAGE = {
    "nsdp_nn_dist2": "test_nn_dist2",
    "nsdp_nn_dist2_ragged": "test_nn_dist2_ragged",
    "nsdp_segment_mean_f32": "test_segment_mean",
}
_SEEN: set = set()


def _call(a, name, *args):
    """One C-ABI call through the arena's recording proxy: tensors as device pointers, None as NULL, int -> int."""
    from nsdp_amd import _lib, pointnet2_utils
    conv = []
    for v in args:
        if v is None:
            conv.append(ctypes.c_void_p(0))
        elif isinstance(v, torch.Tensor):
            assert v.is_cuda and v.is_contiguous()
            conv.append(ctypes.c_void_p(v.data_ptr()))
        else:
            conv.append(ctypes.c_int(int(v)))
    with a.routed(pointnet2_utils):
        _lib.check(getattr(_lib.lib(), name)(*conv, _lib.stream_ptr()), name)
    _SEEN.update(a.called)


def _cloud(seed, *shape, lattice=False):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, 5, shape, generator=g).float() / 4 if lattice else torch.rand(*shape, generator=g) - 0.5


def _bits(t):
    return t.contiguous().view(torch.int32)


# (B, n, m): one workgroup; queries and LDS tile on both sides of 1024 with a source split in parts; a larger split
@pytest.mark.parametrize("B,n,m,lattice", [(1, 3, 1, False), (3, 1025, 1023, False), (2, 257, 4099, True), (1, 5000, 2049, False)])
def test_nn_dist2(B, n, m, lattice):
    from nsdp_amd import pointnet2_utils as pu
    q, s = _cloud(n, B, n, 3, lattice=lattice), _cloud(m + 7, B, m, 3, lattice=lattice)
    a = PoisonArena(DEV, 16 << 20)
    tq, ts = a.input("query", q), a.input("source", s)
    d_only = a.output("dist2.only", (B, n))
    _call(a, "nsdp_nn_dist2", tq, ts, B, n, m, d_only, None)
    d, idx = a.output("dist2", (B, n)), a.output("idx", (B, n), torch.int32)
    _call(a, "nsdp_nn_dist2", tq, ts, B, n, m, d, idx)
    a.check(written=[d_only, d, idx])
    widx, wd = pu.knn(q.to(DEV), s.to(DEV), 1, return_dist=True)
    assert bool(torch.isfinite(d).all())
    assert torch.equal(_bits(d_only), _bits(wd[:, :, 0])) and torch.equal(_bits(d), _bits(wd[:, :, 0])) and torch.equal(idx, widx[:, :, 0])


def _ragged_case(a, qoff, soff, qcap, scap, seed, want_q, want_s):
    """The packed search inside the arena with the given (possibly corrupt) offsets; `want_*`: the host's clamped counts, the
    shapes the kernels must have seen.  Returns nothing: asserts."""
    from nsdp_amd import pointnet2_utils as pu
    B = len(want_q)
    q, s = _cloud(seed, qcap, 3), _cloud(seed + 1, scap, 3)
    tq, ts = a.input("query", q), a.input("source", s)
    tqo, tso = a.input("query_offsets", torch.tensor(qoff, dtype=torch.int32)), a.input("source_offsets", torch.tensor(soff, dtype=torch.int32))
    first = min(max(qoff[0], 0), qcap)
    last = first + sum(want_q)
    # (rows: the arena lets the call touch the rows before `last` only)
    d_only = a.output("dist2.only", (qcap,), rows=last)
    _call(a, "nsdp_nn_dist2_ragged", tq, tqo, ts, tso, B, qcap, scap, d_only, None)
    d, idx = a.output("dist2", (qcap,), rows=last), a.output("idx", (qcap,), torch.int32, rows=last)
    _call(a, "nsdp_nn_dist2_ragged", tq, tqo, ts, tso, B, qcap, scap, d, idx)
    a.check(written=[d_only[first:last], d[first:last], idx[first:last]])
    assert bool(torch.isnan(d_only[last:]).all()) and bool(torch.isnan(d[last:]).all()) and bool((idx[last:] == -1).all())
    assert bool(torch.isnan(d_only[:first]).all()) and bool((idx[:first] == -1).all())
    qlo, slo = first, min(max(soff[0], 0), scap)
    qd, sd = q.to(DEV), s.to(DEV)
    for nq, ns in zip(want_q, want_s):
        rows = slice(qlo, qlo + nq)
        if nq and ns:
            widx, wd = pu.knn(qd[None, rows].contiguous(), sd[None, slo:slo + ns].contiguous(), 1, return_dist=True)
            assert torch.equal(_bits(d_only[rows]), _bits(wd[0, :, 0])) and torch.equal(_bits(d[rows]), _bits(wd[0, :, 0]))
            assert torch.equal(idx[rows] - slo, widx[0, :, 0])
        elif nq:
            assert bool((d_only[rows] == FLT_MAX).all()) and bool((d[rows] == FLT_MAX).all())
            assert bool((idx[rows] == min(slo, scap - 1)).all())
        qlo, slo = qlo + nq, slo + ns


def _clamped_counts(off, cap):
    prev, counts = min(max(off[0], 0), cap), []
    for o in off[1:]:
        o = min(max(o, prev), cap)
        counts.append(o - prev)
        prev = o
    return counts


def test_nn_dist2_ragged():
    qc, sc = [3001, 0, 1, 257], [17, 1025, 5, 300]
    qoff, soff = [0] + list(np.cumsum(qc)), [0] + list(np.cumsum(sc))
    _ragged_case(PoisonArena(DEV, 16 << 20), qoff, soff, sum(qc) + 700, sum(sc) + 90, 50, qc, sc)
    # a shape without source rows, the last one, in a source set without padding: the index clamps to scap - 1
    _ragged_case(PoisonArena(DEV, 16 << 20), [0, 300, 305], [0, 2100, 2100], 305, 2100, 52, [300, 5], [2100, 0])


def test_nn_dist2_ragged_corrupt_offsets_stay_inside_the_operands():
    """Offsets that run backwards and exceed the capacities by up to 3000 rows (36 KB, inside the 256 KiB guards: an unclamped
    access would land in a guard band and be reported, not fault): the kernels see the clamped shapes."""
    qcap, scap = 1500, 2300
    qoff, soff = [-5, 900, 400, 1200, qcap + 3000], [40, 1030, 2200, 1000, scap + 2999]
    assert _clamped_counts(qoff, qcap) == [900, 0, 300, 300] and _clamped_counts(soff, scap) == [990, 1170, 0, 100]
    _ragged_case(PoisonArena(DEV, 16 << 20), qoff, soff, qcap, scap, 54, _clamped_counts(qoff, qcap), _clamped_counts(soff, scap))


@pytest.mark.parametrize("transform", [0, 1])
def test_segment_mean(transform):
    counts = [1, 0, 63, 64, 65, 1023, 1025, 30000]
    g = torch.Generator().manual_seed(60 + transform)
    cap = sum(counts) + 100
    v = torch.rand(cap, generator=g) - (0.1 if transform else 0.5)
    a = PoisonArena(DEV, 16 << 20)
    tv, to = a.input("values", v), a.input("offsets", torch.tensor([0] + list(np.cumsum(counts)), dtype=torch.int32))
    out = a.output("out", (len(counts),))
    _call(a, "nsdp_segment_mean_f32", tv, to, len(counts), cap, transform, out)
    a.check(written=[out])
    got, lo = out.cpu().numpy(), 0
    for b, c in enumerate(counts):
        x = v[lo:lo + c].numpy()
        x = np.sqrt(np.maximum(x, np.float32(0))) if transform else x
        if c == 0:
            assert np.isnan(got[b])
        else:
            np.testing.assert_allclose(got[b], np.float32(x.astype(np.float64).mean()), rtol=1.2e-7, atol=0)
        lo += c
    # corrupt offsets: backwards and up to 3000 rows beyond the capacity -- the clamped shapes, nothing outside the operands
    off = [7, 3, 500, cap + 3000, cap + 1]
    cc = _clamped_counts(off, cap)
    a = PoisonArena(DEV, 16 << 20)
    tv, to = a.input("values", v), a.input("offsets", torch.tensor(off, dtype=torch.int32))
    out = a.output("out", (4,))
    _call(a, "nsdp_segment_mean_f32", tv, to, 4, cap, transform, out)
    a.check(written=[out])
    got, lo = out.cpu().numpy(), 7
    for b, c in enumerate(cc):
        x = v[lo:lo + c].numpy()
        x = np.sqrt(np.maximum(x, np.float32(0))) if transform else x
        if c == 0:
            assert np.isnan(got[b])
        else:
            np.testing.assert_allclose(got[b], np.float32(x.astype(np.float64).mean()), rtol=1.2e-7, atol=0)
        lo += c


def test_wrappers_allocate_nothing_but_the_declared_outputs():
    """The Python bindings routed through the arena: their outputs (the only allocations) get guards too."""
    from nsdp_amd import pointnet2_utils as pu
    from nsdp_amd.ragged import offsets_of
    a = PoisonArena(DEV, 16 << 20)
    q, s = a.input("q", _cloud(70, 2, 1300, 3)), a.input("s", _cloud(71, 2, 2500, 3))
    off = a.input("off", torch.tensor([0, 1300, 2600], dtype=torch.int32))
    soff = a.input("soff", torch.tensor([0, 2500, 5000], dtype=torch.int32))
    with a.routed(pu):
        d = pu.nn_dist2(q, s)
        d2, idx = pu.nn_dist2(q, s, return_index=True)
        rd = pu.nn_dist2_ragged(q.view(-1, 3), off, s.view(-1, 3), soff)
        mean = pu.segment_mean(rd, off, sqrt=True)
    _SEEN.update(a.called)
    a.check(written=[d, d2, idx, rd, mean])
    assert torch.equal(_bits(d), _bits(d2)) and torch.equal(_bits(rd.view(2, 1300)), _bits(d))
    assert torch.equal(idx, pu.knn(q, s, 1)[:, :, 0])
    assert torch.allclose(mean, d.sqrt().mean(1), rtol=1e-6)


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
