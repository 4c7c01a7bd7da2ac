"""The two batched weight-gradient reductions (nsdp_wgrad_bf16_reduce_batched: linear layout, eight chains;
nsdp_wgrad_bf16x3_reduce_batched: fragment layout, eight ranges of four chains) against the numpy emulation of their documented
orders (tests/wgrad_reduce_ref.py): bit-equal dW and db on hand-built descriptors over random workspaces -- fresh and accumulated
targets, with and without a bias gradient, at the partial counts and shapes where the code takes each of its branches.  The
one-call forms are tied to the same sums by test_linear_gpu.py (one call against partials + batched) and the arena tests."""
import ctypes

import numpy as np
import pytest
import torch

import wgrad_reduce_ref as ref

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def _mixed(gen, n):
    """n fp32 values over sixteen binades (reassociation changes the rounding of their sums)."""
    return torch.randn(n, generator=gen) * torch.exp2(torch.randint(-8, 9, (n,), generator=gen).float())


def _run(entry, Desc, cases, gen):
    """cases: (emulation, descriptor fields, workspace floats, N, K, accumulate, want_db).  One call of `entry` over all of them;
    every target must come out bit-equal to the emulation (a NULL db: nothing to compare)."""
    from nsdp_amd import _lib
    descs, held = [], []
    for emulate, fields, ws_floats, N, K, acc, want_db in cases:
        ws = _mixed(gen, ws_floats)
        dw0, db0 = _mixed(gen, N * K).reshape(N, K), _mixed(gen, N)
        dw, db = dw0.to(DEV), db0.to(DEV)
        ws_d = ws.to(DEV)
        d = Desc(ws=ws_d.data_ptr(), dW=dw.data_ptr(), db=db.data_ptr() if want_db else None, N=N, K=K, accumulate=acc, **fields)
        descs.append(d)
        held.append((ws_d, dw, db, emulate(ws.numpy(), dw0.numpy(), db0.numpy(), bool(acc), want_db), db0))
    arr = (Desc * len(descs))(*descs)
    _lib.check(entry(arr, len(descs), _lib.stream_ptr()), "batched reduce")
    torch.cuda.synchronize()
    for i, ((_, dw, db, (want_w, want_b), db0), case) in enumerate(zip(held, cases)):
        what = (i, case[1], case[3:])
        assert np.array_equal(dw.cpu().numpy().view(np.uint32), want_w.view(np.uint32)), what
        if want_b is None:      # db == NULL: the tensor that was not handed over is untouched
            want_b = db0.numpy()
        assert np.array_equal(db.cpu().numpy().view(np.uint32), want_b.view(np.uint32)), what


def _linear_case(S, N, K, acc, want_db):
    emulate = lambda ws, dw, db, a, wb: ref.linear_reduce(ws, S, N, K, dw, db, a, wb)
    return emulate, {"S": S}, S * (N * K + N), N, K, acc, want_db


def _fragment_case(S, nta, ktb, N, K, acc, want_db):
    parts = -(-K // (16 * ktb))
    emulate = lambda ws, dw, db, a, wb: ref.fragment_reduce(ws, S, nta, ktb, N, K, dw, db, a, wb)
    return emulate, {"S": S, "nta": nta, "ktb": ktb}, parts * S * ref.fragment_stride(nta, ktb), N, K, acc, want_db


@pytest.mark.parametrize("S", [1, 7, 8, 9, 20])
def test_linear_order_is_bit_equal_to_its_emulation(S):
    """N K + N = 66 / 1280 / 6: not a multiple of 256, a multiple, less than one workgroup."""
    from nsdp_amd import _lib, hip_linear
    cases = [_linear_case(S, N, K, acc, want_db) for (N, K) in ((6, 10), (256, 4), (3, 1)) for acc in (0, 1) for want_db in (True, False)]
    _run(_lib.lib().nsdp_wgrad_bf16_reduce_batched, hip_linear._ReduceDescB16, cases, torch.Generator().manual_seed(100 + S))


def test_linear_order_fifty_descriptors_of_different_sizes():
    """More than one launch of the host loop (48 descriptors each); small layers inside a grid sized by the largest one."""
    from nsdp_amd import _lib, hip_linear
    cases = [_linear_case(1 + i % 11, 1 + (7 * i) % 23, 1 + (5 * i) % 17, i % 2, i % 3 != 0) for i in range(50)]
    cases[13] = _linear_case(9, 64, 36, 1, True)      # (the largest of the first launch)
    _run(_lib.lib().nsdp_wgrad_bf16_reduce_batched, hip_linear._ReduceDescB16, cases, torch.Generator().manual_seed(150))


FRAGMENT_SHAPES = [(8, 8, 20, 24), (8, 13, 128, 200), (13, 13, 200, 200), (16, 8, 256, 256)]


@pytest.mark.parametrize("S", [1, 3, 8, 13, 37])
def test_fragment_order_is_bit_equal_to_its_emulation(S):
    """Below eight partials some of the eight ranges are empty; at 13 and 37 they have unequal lengths and their four chains
    remainders.  (20, 24): a partial 32-element block; (256, 256): two column parts, db from part 0.  All four shapes, fresh and
    accumulated, with and without db, in ONE call: mixed sizes under one grid."""
    from nsdp_amd import _lib, hip_linear
    cases = [_fragment_case(S, nta, ktb, N, K, acc, want_db) for i, (nta, ktb, N, K) in enumerate(FRAGMENT_SHAPES)
             for acc in (0, 1) for want_db in (True, False)]
    _run(_lib.lib().nsdp_wgrad_bf16x3_reduce_batched, hip_linear._ReduceDesc, cases, torch.Generator().manual_seed(200 + S))
