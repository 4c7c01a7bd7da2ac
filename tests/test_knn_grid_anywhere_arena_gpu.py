"""nsdp_knn_grid inside the poisoned arena of tests/poison_arena.py on the inputs tests/test_knn_grid_anywhere_gpu.py adds -- a
cloud far from the origin, a cloud that fills its volume, queries that all end in the wave-cooperative finish -- as
tests/test_knn_grid_arena_gpu.py holds the entry on centred clouds: every operand between guards, the workspace exactly the
declared bytes and poisoned on entry, idx_out / dist_out poisoned until the kernel writes them, no byte changed outside the
three, and the results those of the scan on the same inputs (a read of poison would change them)."""
import ctypes

import numpy as np
import pytest
import torch

from nsdp_amd import _lib, pointnet2_utils as pu
from poison_arena import PoisonArena
from test_knn_grid_gpu import _sphere

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def _grid_in_arena(query, source, k):
    """One rectangular call (query None: the self-search) -> the stats words; the arena and the scan's results are checked."""
    B, m = source.shape[:2]
    n = m if query is None else query.shape[1]
    a = PoisonArena(DEV, 32 << 20)
    tsrc = a.input("source", torch.from_numpy(source))
    tq = tsrc if query is None else a.input("query", torch.from_numpy(query))
    fn = _lib.lib().nsdp_knn_grid_workspace_bytes
    fn.restype = ctypes.c_size_t
    need = int(fn(ctypes.c_int(B), ctypes.c_int(B * n), ctypes.c_int(B * m), ctypes.c_int(m)))
    assert need > 0
    ws = a.workspace("workspace", need)
    idx, d2 = a.output("idx", (B, n, k), torch.int32), a.output("dist", (B, n, k), torch.float32)
    args = [ctypes.c_void_p(tq.data_ptr()), ctypes.c_void_p(tsrc.data_ptr()), ctypes.c_int(B), ctypes.c_int(n), ctypes.c_int(m),
            ctypes.c_int(k), ctypes.c_void_p(ws.data_ptr()), ctypes.c_void_p(idx.data_ptr()), ctypes.c_void_p(d2.data_ptr())]
    _lib.check(_lib.lib().nsdp_knn_grid(*args, _lib.stream_ptr()), "nsdp_knn_grid")
    a.check(written=[idx, d2])
    out = (ctypes.c_int64 * 4)()
    assert _lib.lib().nsdp_knn_grid_stats(ctypes.c_void_p(ws.data_ptr()), _lib.stream_ptr(), out) == 0
    s = torch.from_numpy(source).to(DEV)
    q = s if query is None else torch.from_numpy(query).to(DEV)
    with pu.knn_grid_mode("0"):
        want_idx, want_d = pu.knn(q, s, k, return_dist=True)
    np.testing.assert_array_equal(idx.cpu().numpy(), want_idx.cpu().numpy())
    np.testing.assert_array_equal(d2.cpu().numpy().view(np.int32), want_d.cpu().numpy().view(np.int32))
    assert out[0] == B * n
    return list(out)


def test_translated_cloud():
    cloud = _sphere(np.random.default_rng(41), 3001) + np.array([2000.0, -1500.0, 900.0], np.float32)
    assert _grid_in_arena(None, np.stack([cloud, cloud[::-1]]), 16)[2] == 0


def test_volume():
    cloud = np.random.default_rng(42).uniform(-0.5, 0.5, (1, 5000, 3)).astype(np.float32)
    _grid_in_arena(None, cloud, 32)


@pytest.mark.parametrize("n,k", [(130, 16), (65, 32), (1, 1)])
def test_all_finish(n, k):
    """Every query far outside the box: the whole wave reads the source rows, lanes without a query included."""
    rng = np.random.default_rng(43)
    source = _sphere(rng, 3000)[None]
    query = (rng.standard_normal((1, n, 3)) * 50.0).astype(np.float32)
    assert _grid_in_arena(query, source, k)[2] == n
