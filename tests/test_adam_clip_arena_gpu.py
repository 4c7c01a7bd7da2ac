"""The launching entries of include/nsdp_optim.h inside the poisoned arena of tests/poison_arena.py, as
tests/test_rigidity_arena_gpu.py holds those of include/nsdp_rigidity.h: the tables, every gradient, parameter and moment between
guards (every other tensor a view 4 bytes into its operand), the partials buffer exactly the declared bytes and poisoned on
entry, the state's output fields poisoned until the finalize writes them -- no byte changed outside the operands, none left
unwritten, and nothing read that nobody wrote: the poison is NaN and the results are compared with tests/adam_clip_ref.py."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import adam_clip_ref as ref
from poison_arena import PoisonArena

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "nsdp_optim.h")

COVERAGE = {"nsdp_grad_sumsq_f32": "test_entries_inside_the_arena", "nsdp_grad_clip_finalize": "test_entries_inside_the_arena",
            "nsdp_adam_multi_clipped_f32": "test_entries_inside_the_arena"}
HOST_ONLY = {"nsdp_grad_sumsq_workspace_bytes"}
_SEEN: set = set()

_ci, _cd, _vp = ctypes.c_int, ctypes.c_double, ctypes.c_void_p
KW = dict(lr=5e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01)
STATE = np.dtype([("sumsq", "<f8"), ("norm", "<f4"), ("coef", "<f4"), ("apply", "<i4"), ("steps", "<i4"), ("clipped", "<i4"),
                  ("skipped", "<i4")])


def _p(t):
    return _vp(0) if t is None else _vp(t.data_ptr())


def _bits(t):
    return t.detach().contiguous().view(torch.int32)


class _Operand:
    """One fp32 tensor of the tables inside the arena; ``off`` = 1: a view one element into the operand."""

    def __init__(self, arena, name, values, off, accum):
        flat = torch.cat([torch.full((off,), 7.0), values.reshape(-1)])
        self.whole = (arena.accum if accum else arena.input)(name, flat)
        if accum and off:      # the element in front of the view is NOT the call's to write
            r = arena.regions[-1]
            arena.writable[r.start:r.start + 4 * off] = False
        self.view, self.off = self.whole[off:], off
        assert self.view.data_ptr() % 16 == 4 * off


def _tables(a, grads, values):
    ps, gs, ms, vs = [], [], [], []
    for i, (g, v) in enumerate(zip(grads, values)):
        off = i % 2
        ps.append(_Operand(a, f"param{i}", v, off, True))
        gs.append(_Operand(a, f"grad{i}", g, off, False))
        ms.append(_Operand(a, f"exp_avg{i}", torch.zeros_like(v), off, True))
        vs.append(_Operand(a, f"exp_avg_sq{i}", torch.zeros_like(v), off, True))
    steps = a.accum("steps", torch.zeros(len(values)))
    rows = [(p.view.data_ptr(), g.view.data_ptr(), m.view.data_ptr(), v.view.data_ptr(), steps[i:].data_ptr(), p.view.numel())
            for i, (p, g, m, v) in enumerate(zip(ps, gs, ms, vs))]
    chunks = [(i, c) for i, r in enumerate(rows) for c in range(-(-r[5] // ref.CHUNK))]
    descs = a.input("descs", torch.tensor(rows, dtype=torch.int64))
    table = a.input("chunks", torch.tensor(chunks, dtype=torch.int32))
    done = a.accum("done", torch.zeros(len(rows), dtype=torch.int32))
    return ps, gs, ms, vs, steps, descs, table, done, len(chunks)


def _state(a):
    raw = torch.full((8,), -1, dtype=torch.int32)      # the poison pattern in the fields the finalize must write ...
    raw[5:] = torch.tensor([3, 1, 2], dtype=torch.int32)      # ... and running counters with a history
    return a.accum("state", raw)


def _read_state(t):
    return t.cpu().numpy().view(STATE)[0]


@pytest.mark.parametrize("bad", [None, float("inf")])
def test_entries_inside_the_arena(bad):
    """nsdp_grad_sumsq_f32, nsdp_grad_clip_finalize, nsdp_adam_multi_clipped_f32 on operands carved from the arena.  ``bad``: an inf
    in the last element of the largest gradient and skip_nonfinite set -- the apply == 0 launch."""
    from nsdp_amd import _lib
    L = _lib.lib()
    assert int(L.nsdp_adam_chunk_elems()) == ref.CHUNK
    grads = ref.grads(7, 0)
    if bad is not None:
        grads[10].view(-1)[-1] = bad
    values = ref.params_agreeing_with(ref.params(3), grads)      # (weight decay against the CPU: nothing cancels in the first step)
    a = PoisonArena(DEV, 64 << 20)
    ps, gs, ms, vs, steps, descs, table, done, n_chunks = _tables(a, grads, values)
    fn = L.nsdp_grad_sumsq_workspace_bytes
    fn.restype = ctypes.c_size_t
    need = int(fn(_ci(n_chunks)))
    assert need == 8 * n_chunks and int(fn(_ci(0))) == 0 == int(fn(_ci(-3)))
    partials = a.workspace("partials", need)
    state = _state(a)
    kept = [(p.whole.clone(), m.whole.clone(), v.whole.clone()) for p, m, v in zip(ps, ms, vs)]

    with a.routed():
        _lib.check(_lib.lib().nsdp_grad_sumsq_f32(_p(descs), _p(table), _ci(n_chunks), _p(partials), _lib.stream_ptr()),
                   "nsdp_grad_sumsq_f32")
    _SEEN.update(a.called)
    a.check(written=[partials.view(torch.int64)])
    want = ref.partials(grads)
    got = partials.view(torch.float64).cpu().numpy()
    assert got.shape == want.shape and np.array_equal(got.view(np.int64), want.view(np.int64))      # (a read of poison: NaN)

    bound = 0.1 * float(np.sqrt(ref.ordered_sumsq(ref.grads(7, 0))))
    with a.routed():
        _lib.check(_lib.lib().nsdp_grad_clip_finalize(_p(partials), _ci(n_chunks), _cd(bound), _ci(1), _p(state), _lib.stream_ptr()),
                   "nsdp_grad_clip_finalize")
    _SEEN.update(a.called)
    a.check(written=[state[:5]])
    S = ref.ordered_sumsq(grads)
    norm, coef, apply = ref.rule(S, bound, skip_nonfinite=True)
    st = _read_state(state)
    assert st["sumsq"] == S and st["norm"] == np.float32(norm) and int(st["apply"]) == int(apply) == (0 if bad else 1)
    assert abs(float(st["coef"]) - float(coef)) <= float(np.spacing(coef))
    assert (int(st["steps"]), int(st["clipped"]), int(st["skipped"])) == ((4, 1, 3) if bad else (4, 2, 2))

    beta1, beta2 = KW["betas"]
    state_before = state.clone()
    with a.routed():
        _lib.check(_lib.lib().nsdp_adam_multi_clipped_f32(_p(descs), _p(table), _ci(n_chunks), _p(done), _vp(0), _cd(KW["lr"]),
                                                          _cd(beta1), _cd(beta2), _cd(KW["eps"]), _cd(KW["weight_decay"]), _ci(0),
                                                          _p(state), _lib.stream_ptr()), "nsdp_adam_multi_clipped_f32")
    _SEEN.update(a.called)
    a.check()
    assert int(done.abs().sum()) == 0
    assert torch.equal(state, state_before)                          # (read only here)
    for t in ps + ms + vs:
        assert t.off == 0 or float(t.whole[0]) == 7.0                # the element in front of a misaligned view
    if bad is not None:
        assert float(steps.abs().sum()) == 0.0
        for p, m, v, (p0, m0, v0) in zip(ps, ms, vs, kept):
            assert torch.equal(_bits(p.whole), _bits(p0)) and torch.equal(_bits(m.whole), _bits(m0)) and torch.equal(_bits(v.whole), _bits(v0))
        return
    assert torch.equal(steps.cpu(), torch.ones(len(values)))
    cpu, opt, _ = ref.run(values, [grads], max_norm=bound, **KW)
    for x, p, m, v in zip(cpu, ps, ms, vs):
        sa = opt.state[x]
        torch.testing.assert_close(m.view.cpu().view(x.shape), sa["exp_avg"], rtol=1e-6, atol=4e-7 * float(sa["exp_avg"].abs().max()))
        torch.testing.assert_close(v.view.cpu().view(x.shape), sa["exp_avg_sq"], rtol=1e-6, atol=4e-7 * float(sa["exp_avg_sq"].abs().max()))
        torch.testing.assert_close(p.view.cpu().view(x.shape), x.detach(), rtol=0, atol=6e-7)


def test_bad_arguments_are_refused_by_name_before_anything_is_launched():
    from nsdp_amd import _lib
    L = _lib.lib()
    buf = torch.zeros(16, dtype=torch.float64, device=DEV)
    for max_norm in (0.0, -1.0, float("nan")):
        assert L.nsdp_grad_clip_finalize(_p(buf), _ci(1), _cd(max_norm), _ci(0), _p(buf[8:]), _lib.stream_ptr()) != 0
        assert "max_norm" in L.nsdp_last_error().decode()
    assert L.nsdp_grad_clip_finalize(_p(buf), _ci(1), _cd(1.0), _ci(0), _vp(0), _lib.stream_ptr()) != 0
    assert "grad_clip_finalize" in L.nsdp_last_error().decode()
    assert L.nsdp_grad_sumsq_f32(_p(buf), _p(buf), _ci(1), _vp(0), _lib.stream_ptr()) != 0
    assert "grad_sumsq_f32" in L.nsdp_last_error().decode()
    assert L.nsdp_adam_multi_clipped_f32(_p(buf), _p(buf), _ci(1), _p(buf), _vp(0), _cd(1e-3), _cd(0.9), _cd(0.999), _cd(1e-8), _cd(0.0),
                                         _ci(0), _vp(0), _lib.stream_ptr()) != 0
    assert "adam_multi_clipped_f32" in L.nsdp_last_error().decode()
    assert L.nsdp_grad_sumsq_f32(_vp(0), _vp(0), _ci(0), _vp(0), _lib.stream_ptr()) == 0      # (nothing to do: nothing launched)
    torch.cuda.synchronize()
    assert float(buf.abs().sum()) == 0.0


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
