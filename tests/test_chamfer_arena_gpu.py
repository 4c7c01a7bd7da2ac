"""The launching entries of include/nsdp_chamfer.h inside the poisoned arena of tests/poison_arena.py, as
tests/test_invert_wide_arena_gpu.py holds the entry of include/nsdp_scatter.h: every operand between guards, the workspace
exactly the bytes the size query declares and poisoned on entry, outputs poisoned until the kernels write them, no byte changed
outside them, no output element left unwritten -- and nothing read that nobody wrote: the poison is NaN, and the results are
compared with the fp64 yardstick.  COVERAGE plays the part of the other files' table for this header."""
import ctypes
import os
import re

import pytest
import torch

import chamfer_ref
from chamfer_ref import U
from poison_arena import PoisonArena

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "nsdp_chamfer.h")

COVERAGE = {"nsdp_chamfer_forward": "test_entries_inside_the_arena", "nsdp_chamfer_backward": "test_entries_inside_the_arena"}
HOST_ONLY = {"nsdp_chamfer_forward_workspace_bytes"}
_SEEN: set = set()

_ci, _cf, _vp = ctypes.c_int, ctypes.c_float, ctypes.c_void_p


def _p(t):
    return _vp(0) if t is None else _vp(t.data_ptr())


def _clouds(B, n, m, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(B, n, 3, generator=g), torch.randn(B, m, 3, generator=g)


def _lists(idx, sources):
    """Ascending inverse lists on the CPU: offsets [B, sources + 1], entries [B, E] (the stable sort)."""
    B = idx.shape[0]
    ent = torch.sort(idx.long(), dim=1, stable=True).indices.int()
    off = torch.zeros(B, sources + 1, dtype=torch.int64)
    for b in range(B):
        off[b, 1:] = torch.cumsum(torch.bincount(idx[b].long(), minlength=sources), 0)
    return off.int(), ent


def _check_grad(name, got, want):
    grad, mass, lengths = want
    bound = chamfer_ref.envelope_c(lengths)[:, :, None] * U * mass
    assert bool(((got.double() - grad).abs() <= bound).all()), name      # (a NaN -- poison that was read -- fails this)


@pytest.mark.parametrize("B,n,m,w_pt,w_tp", [(1, 1, 63, 1.0, 1.0), (3, 63, 1, 1.0, 1.0), (1, 1, 1, 1.0, 1.0), (3, 64, 65, 0.5, 2.0),
                                              (1, 257, 1000, 1.0, 1.0), (3, 1000, 255, 1.0, 0.0), (1, 300, 8200, 1.0, 1.0)])
def test_entries_inside_the_arena(B, n, m, w_pt, w_tp):
    """nsdp_chamfer_forward, then nsdp_chamfer_backward for either operand on the forward's indices, all operands carved from
    the arena.  (1, 300, 8200): collapsed predictions, one list of 8200 entries for the workgroup form; w_tp = 0: the backward
    of the predictions runs without lists (NULL)."""
    from nsdp_amd import _lib
    L = _lib.lib()
    P, Q = _clouds(B, n, m, 7 * n + m)
    if m == 8200:
        P = torch.full((B, n, 3), 0.25)
    a = PoisonArena(DEV, 32 << 20)
    tp, tq = a.input("pred", P), a.input("target", Q)
    fn = L.nsdp_chamfer_forward_workspace_bytes
    fn.restype = ctypes.c_size_t
    need = int(fn(_ci(B)))
    assert need == 8 * B
    ws = a.workspace("workspace", need)
    d_pt, i_pt = a.output("dist2_pt", (B, n)), a.output("idx_pt", (B, n), torch.int32)
    d_tp, i_tp = a.output("dist2_tp", (B, m)), a.output("idx_tp", (B, m), torch.int32)
    terms, loss = a.output("terms", (B,)), a.output("loss", (1,))
    with a.routed():
        _lib.check(_lib.lib().nsdp_chamfer_forward(_p(tp), _p(tq), _ci(B), _ci(n), _ci(m), _cf(w_pt), _cf(w_tp), _p(ws), _p(d_pt),
                                                   _p(i_pt), _p(d_tp), _p(i_tp), _p(terms), _p(loss), _lib.stream_ptr()),
                   "nsdp_chamfer_forward")
    _SEEN.update(a.called)
    a.check(written=[d_pt, i_pt, d_tp, i_tp, terms, loss, ws.view(torch.int64)])
    L64, terms64 = chamfer_ref.loss64(P, Q, w_pt, w_tp)
    assert abs(float(loss) - float(L64)) <= 16 * U * float(L64)
    assert bool(((terms.cpu().double() - terms64).abs() <= 16 * U * terms64).all())
    assert bool(((ws.view(torch.float64).cpu() - terms64).abs() <= 16 * U * terms64).all())
    idx_pt, idx_tp = i_pt.cpu(), i_tp.cpu()
    chamfer_ref.assert_minimisers(P, Q, idx_pt, idx_tp)
    want = chamfer_ref.closed_form(P, Q, idx_pt, idx_tp, w_pt, w_tp, g=2.0)

    g = a.input("g", torch.tensor([2.0]))
    for name, x, y, ix, iy, nx, ny, wd, wl in (("dP", tp, tq, i_pt, idx_tp, n, m, w_pt, w_tp), ("dQ", tq, tp, i_tp, idx_pt, m, n, w_tp, w_pt)):
        off = ent = None
        if wl != 0.0:
            off, ent = _lists(iy, nx)
            off, ent = a.input(name + ".offsets", off), a.input(name + ".entries", ent)
        grad = a.output(name, (B, nx, 3))
        with a.routed():
            _lib.check(_lib.lib().nsdp_chamfer_backward(_p(x), _p(y), _p(ix), _p(off), _p(ent), _p(g), _ci(B), _ci(nx), _ci(ny),
                                                        _cf(wd), _cf(wl), _p(grad), _lib.stream_ptr()), "nsdp_chamfer_backward")
        _SEEN.update(a.called)
        a.check(written=[grad])
        _check_grad(name, grad.cpu(), want[name])


def test_stale_indices_stay_inside_the_operands():
    """Indices, offsets and entries outside their ranges (a poisoned or stale tensor) are clamped before they form an address:
    wrong numbers, but nothing outside the operands is read into a fault or written."""
    from nsdp_amd import _lib
    B, n, m = 2, 65, 300
    P, Q = _clouds(B, n, m, 5)
    g = torch.Generator().manual_seed(6)
    idx = torch.randint(-(1 << 31), (1 << 31) - 1, (B, n), generator=g, dtype=torch.int64).int()
    off = torch.randint(-(1 << 31), (1 << 31) - 1, (B, n + 1), generator=g, dtype=torch.int64).int()
    ent = torch.randint(-(1 << 31), (1 << 31) - 1, (B, m), generator=g, dtype=torch.int64).int()
    off[0] = torch.linspace(0, m, n + 1).int()      # (one shape with valid offsets of long lists over garbage entries)
    a = PoisonArena(DEV, 16 << 20)
    tp, tq, ti, to, te = a.input("self", P), a.input("other", Q), a.input("idx", idx), a.input("offsets", off), a.input("entries", ent)
    tg = a.input("g", torch.tensor([1.0]))
    grad = a.output("grad", (B, n, 3))
    with a.routed():
        _lib.check(_lib.lib().nsdp_chamfer_backward(_p(tp), _p(tq), _p(ti), _p(to), _p(te), _p(tg), _ci(B), _ci(n), _ci(m), _cf(1.0),
                                                    _cf(1.0), _p(grad), _lib.stream_ptr()), "nsdp_chamfer_backward")
    _SEEN.update(a.called)
    a.check(written=[grad])
    assert bool(torch.isfinite(grad).all())


@pytest.mark.parametrize("n,m", [(1, 1), (257, 1000), (300, 8200)])
def test_wrapper_allocates_inside_the_arena(n, m, monkeypatch):
    """chamfer_loss forward + backward with the wrapper's own allocations (workspace, outputs, kept indices, the lists of
    hip_attention.inverse_lists and their workspace, both gradients) routed through the arena: all get guards too."""
    from nsdp_amd import chamfer, hip_attention
    B = 2
    P, Q = _clouds(B, n, m, 9)
    if m == 8200:
        P = torch.full((B, n, 3), 0.25)
    a = PoisonArena(DEV, 48 << 20)
    tp, tq = a.input("pred", P).requires_grad_(True), a.input("target", Q).requires_grad_(True)
    made, real = [], chamfer.backward_operand      # (autograd may hand .grad a copy: the kernel's own outputs are what is checked)
    monkeypatch.setattr(chamfer, "backward_operand", lambda *args: made.append(real(*args)) or made[-1])
    with a.routed(chamfer, hip_attention):
        loss = chamfer.chamfer_loss(tp, tq)
        loss.backward()
    _SEEN.update(a.called)
    assert {"nsdp_chamfer_forward", "nsdp_chamfer_backward"} <= a.called
    if m == 8200:
        assert "nsdp_knn_invert_wide" in a.called
    assert len(made) == 2 and torch.equal(made[0], tp.grad) and torch.equal(made[1], tq.grad)
    a.check(written=made + [loss.detach().reshape(1)])
    idx = [t.cpu() for t in chamfer.forward_raw(tp.detach(), tq.detach())]
    want = chamfer_ref.closed_form(P, Q, idx[3], idx[5])
    _check_grad("dP", tp.grad.cpu(), want["dP"])
    _check_grad("dQ", tq.grad.cpu(), want["dQ"])


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
