"""The launching entries of include/nsdp_rigidity.h inside the poisoned arena of tests/poison_arena.py, as
tests/test_chamfer_arena_gpu.py holds those of include/nsdp_chamfer.h: every operand between guards, the workspace exactly the
bytes the size query declares and poisoned on entry, outputs poisoned until the kernels write them, no byte changed outside
them, no output element left unwritten -- and nothing read that nobody wrote: the poison is NaN, and the results are compared
with the fp64 yardstick.  COVERAGE plays the part of the other files' table for this header."""
import ctypes
import os
import re

import pytest
import torch

import rigidity_ref
from poison_arena import PoisonArena
from rigidity_ref import RESID_C, TERMS_C, U

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "nsdp_rigidity.h")

COVERAGE = {"nsdp_rigidity_forward": "test_entries_inside_the_arena", "nsdp_rigidity_backward": "test_entries_inside_the_arena"}
HOST_ONLY = {"nsdp_rigidity_forward_workspace_bytes"}
_SEEN: set = set()

_ci, _cf, _vp = ctypes.c_int, ctypes.c_float, ctypes.c_void_p


def _p(t):
    return _vp(0) if t is None else _vp(t.data_ptr())


def _operands(B, n, K, seed, hub=False):
    g = torch.Generator().manual_seed(seed)
    S = torch.randn(B, n, 3, generator=g)
    P = S + 0.3 * torch.randn(B, n, 3, generator=g)
    idx = torch.randint(0, n, (B, n, K), generator=g, dtype=torch.int64).int()
    if hub:                                              # (three quarters of the entries name row 1: a list beyond 1024)
        idx[:, :, 1:] = 1
    return P, S, idx


def _lists(idx, n):
    """Ascending inverse lists of idx [B, n, K] viewed as [B, n * K] on the CPU: offsets [B, n + 1], entries [B, n * K]."""
    B = idx.shape[0]
    flat = idx.reshape(B, -1).long()
    ent = torch.sort(flat, dim=1, stable=True).indices.int()
    off = torch.zeros(B, n + 1, dtype=torch.int64)
    for b in range(B):
        off[b, 1:] = torch.cumsum(torch.bincount(flat[b], minlength=n), 0)
    return off.int(), ent


def _check_grad(P, idx, resid, got, weight, g):
    grad, mass, lengths = rigidity_ref.closed_form(P, idx, resid, weight, g)
    bound = rigidity_ref.envelope_c(lengths, idx.shape[2])[:, :, None] * U * mass
    assert bool(((got.double() - grad).abs() <= bound).all())      # (a NaN -- poison that was read -- fails this)
    return lengths


@pytest.mark.parametrize("B,n,K,hub", [(1, 1, 1, False), (3, 63, 1, False), (1, 1, 32, False), (3, 64, 7, False), (2, 515, 4, True)])
def test_entries_inside_the_arena(B, n, K, hub):
    """nsdp_rigidity_forward, then nsdp_rigidity_backward on the forward's residuals, all operands carved from the arena.
    (2, 515, 4): row 1 is named by 1545 entries, the workgroup form."""
    from nsdp_amd import _lib
    L = _lib.lib()
    P, S, idx = _operands(B, n, K, 7 * n + K, hub)
    w = 0.5
    a = PoisonArena(DEV, 16 << 20)
    tp, ts, ti = a.input("pred", P), a.input("source", S), a.input("idx", idx)
    fn = L.nsdp_rigidity_forward_workspace_bytes
    fn.restype = ctypes.c_size_t
    need = int(fn(_ci(B)))
    assert need == 65 * 8 * B                            # (the per-shape terms in double, then 64 slice sums per shape)
    ws = a.workspace("workspace", need)
    resid, terms, loss = a.output("resid", (B, n, K)), a.output("terms", (B,)), a.output("loss", (1,))
    with a.routed():
        _lib.check(_lib.lib().nsdp_rigidity_forward(_p(tp), _p(ts), _p(ti), _ci(B), _ci(n), _ci(K), _cf(w), _p(ws), _p(resid),
                                                    _p(terms), _p(loss), _lib.stream_ptr()), "nsdp_rigidity_forward")
    _SEEN.update(a.called)
    a.check(written=[resid, terms, loss, ws.view(torch.int64)])
    r64, cur, rest = rigidity_ref.resid64(P, S, idx)
    r = resid.cpu()
    assert bool(((r.double() - r64).abs() <= RESID_C * U * (cur + rest)).all())
    L64, terms64 = rigidity_ref.from_resid(r, w)
    assert abs(float(loss) - float(L64)) <= TERMS_C * U * float(L64)
    assert bool(((terms.cpu().double() - terms64).abs() <= TERMS_C * U * terms64).all())
    assert bool(((ws.view(torch.float64)[:B].cpu() - terms64).abs() <= 2.0 ** -40 * terms64).all())      # (the unrounded doubles)

    off, ent = _lists(idx, n)
    to, te, tg = a.input("offsets", off), a.input("entries", ent), a.input("g", torch.tensor([2.0]))
    grad = a.output("grad", (B, n, 3))
    with a.routed():
        _lib.check(_lib.lib().nsdp_rigidity_backward(_p(tp), _p(ti), _p(resid), _p(to), _p(te), _p(tg), _ci(B), _ci(n), _ci(K), _cf(w),
                                                     _p(grad), _lib.stream_ptr()), "nsdp_rigidity_backward")
    _SEEN.update(a.called)
    a.check(written=[grad])
    lengths = _check_grad(P, idx, r, grad.cpu(), w, 2.0)
    if hub:
        assert int(lengths.max()) > rigidity_ref.WAVE_MAX


def test_stale_indices_stay_inside_the_operands():
    """Indices, offsets and entries outside their ranges (a poisoned or stale tensor) are clamped before they form an address:
    wrong numbers, but nothing outside the operands is read into a fault or written."""
    from nsdp_amd import _lib
    B, n, K = 2, 300, 4
    P, S, _ = _operands(B, n, K, 5)
    g = torch.Generator().manual_seed(6)
    lo, hi = -(1 << 31), (1 << 31) - 1
    idx = torch.randint(lo, hi, (B, n, K), generator=g, dtype=torch.int64).int()
    off = torch.randint(lo, hi, (B, n + 1), generator=g, dtype=torch.int64).int()
    ent = torch.randint(lo, hi, (B, n * K), generator=g, dtype=torch.int64).int()
    off[0] = torch.linspace(0, n * K, n + 1).int()      # (one shape with valid offsets over garbage entries)
    off[1, :3] = torch.tensor([0, 0, n * K])            # (and one list of every entry: the workgroup form over garbage)
    a = PoisonArena(DEV, 16 << 20)
    tp, ts, ti = a.input("pred", P), a.input("source", S), a.input("idx", idx)
    to, te, tg = a.input("offsets", off), a.input("entries", ent), a.input("g", torch.tensor([1.0]))
    ws = a.workspace("workspace", 65 * 8 * B)
    resid, terms, loss, grad = a.output("resid", (B, n, K)), a.output("terms", (B,)), a.output("loss", (1,)), a.output("grad", (B, n, 3))
    with a.routed():
        _lib.check(_lib.lib().nsdp_rigidity_forward(_p(tp), _p(ts), _p(ti), _ci(B), _ci(n), _ci(K), _cf(1.0), _p(ws), _p(resid),
                                                    _p(terms), _p(loss), _lib.stream_ptr()), "nsdp_rigidity_forward")
        _lib.check(_lib.lib().nsdp_rigidity_backward(_p(tp), _p(ti), _p(resid), _p(to), _p(te), _p(tg), _ci(B), _ci(n), _ci(K),
                                                     _cf(1.0), _p(grad), _lib.stream_ptr()), "nsdp_rigidity_backward")
    _SEEN.update(a.called)
    a.check(written=[resid, terms, loss, grad, ws.view(torch.int64)])
    assert bool(torch.isfinite(grad).all()) and bool(torch.isfinite(resid).all()) and bool(torch.isfinite(loss).all())


@pytest.mark.parametrize("n,K,hub", [(1, 1, False), (64, 7, False), (515, 4, True)])
def test_wrapper_allocates_inside_the_arena(n, K, hub, monkeypatch):
    """local_rigidity_loss forward + backward with the wrapper's own allocations (workspace, outputs, the kept residuals, the
    lists of hip_attention.inverse_lists and their workspace, the gradient) routed through the arena: all get guards too."""
    from nsdp_amd import hip_attention, rigidity
    B = 2
    P, S, idx = _operands(B, n, K, 9, hub)
    a = PoisonArena(DEV, 32 << 20)
    tp, ts, ti = a.input("pred", P).requires_grad_(True), a.input("source", S), a.input("idx", idx)
    made, real = [], rigidity.backward_raw      # (autograd may hand .grad a copy: the kernel's own output is what is checked)
    monkeypatch.setattr(rigidity, "backward_raw", lambda *args: made.append(real(*args)) or made[-1])
    with a.routed(rigidity, hip_attention):
        loss = rigidity.local_rigidity_loss(tp, ts, idx=ti, weight=0.5)
        loss.backward()
    _SEEN.update(a.called)
    assert {"nsdp_rigidity_forward", "nsdp_rigidity_backward"} <= a.called
    assert ("nsdp_knn_invert_wide" if n * K > 1024 else "nsdp_knn_invert") in a.called
    assert len(made) == 1 and torch.equal(made[0], tp.grad)
    a.check(written=made + [loss.detach().reshape(1)])
    resid = rigidity.forward_raw(tp.detach(), ts, ti, 0.5)[2].cpu()
    _check_grad(P, idx, resid, tp.grad.cpu(), 0.5, 1.0)


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
