"""The entry of include/nsdp_meshbatch.h inside the poisoned arena of tests/poison_arena.py: every operand between 256 KiB guards,
outputs poisoned until the kernel writes them.  The tables are STALE: entries claim more vertices, faces and thresholds than the
arenas hold, first records lie before and beyond them, topology and frame ids point outside the tables, the face arena holds
vertex indices outside every frame and the thresholds of one frame are not even sorted.  As the header says, everything is
clamped as it is read, so the results are those of the clamped operands (tests/mesh_sample_ref.py applies the same clamps) -- no
stray write, no output element left unwritten, no read of memory nobody wrote (the poison is NaN)."""
import numpy as np
import pytest
import torch

import mesh_sample_ref as mr
from poison_arena import PoisonArena

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
COVERAGE = {"nsdp_mesh_batch_sample": "test_sample_inside_the_arena"}
_SEEN: set = set()


def _frame(first, count, topo, thr_first, box):
    e = np.zeros(6, dtype=np.int64)
    e[0], e[1], e[2] = first, (count & 0xFFFFFFFF) | (topo << 32), thr_first
    e[3:6] = np.asarray(box, dtype=np.float32).view(np.int64)
    return e


@pytest.mark.parametrize("with_noise,n,m", [(True, 300, 261), (False, 300, 0), (False, 0, 70)])
def test_sample_inside_the_arena(with_noise, n, m):
    from nsdp_amd import datastore, meshstore
    g = np.random.RandomState(11)
    V, FR, TR, B = 500, 400, 350, 5                 # more than one 256-lane block per part, neither a multiple of it
    verts = np.zeros((V, 4), np.float32)
    verts[:, :3] = g.rand(V, 3) - 0.5
    faces = np.zeros((FR, 4), np.int32)
    faces[:, :3] = g.randint(0, 120, size=(FR, 3))
    faces[::7, 0], faces[3::11, 1], faces[5::13, 2] = -3, 1 << 30, -(1 << 31)          # vertex indices outside every frame
    faces[:, 3] = g.randint(-9, 9, size=FR)                                              # (the padding is never used)
    thr = np.sort(g.randint(0, 1 << 31, size=TR).astype(np.uint32))
    thr[100:200] = g.randint(0, 1 << 31, size=100)                                       # stale: not sorted, no 2^31 at the end
    thr[99], thr[349] = 1 << 31, 1 << 31
    box = lambda: np.concatenate([-0.5 + 0.3 * g.rand(3), 0.5 - 0.3 * g.rand(3)]).astype(np.float32)
    frames = np.stack([
        _frame(0, 120, 0, 0, box()), _frame(120, 120, 0, -1, box()), _frame(240, 150, 1, 100, box()),
        _frame(390, 300, 1, 200, box()),                      # PARTIAL: 300 vertices from record 390 of 500, thresholds 200 + 150 = 350
        _frame(-7, 1 << 30, 9, 1 << 40, box()),               # corrupt throughout: topology 9 of 4
        _frame(1 << 40, -5, -2, -(1 << 40), box()),           # negative count and topology
        _frame(450, 50, 2, 340, box()),                       # topology 2 is PARTIAL, thresholds run off the arena
        _frame(10, 0, 3, 5, box())])                          # no vertices; topology 3 has no faces
    topos = np.array([[0, 100], [100, 150], [300, 200], [1 << 35, 0]], dtype=np.int64)      # [2]: 200 faces from record 300 of 400
    ids = np.array([[0, 3, 4, 6, 7], [1, 3, 44, 5, 2], [2, 0, -3, 7, 1 << 30]], dtype=np.int32)      # ids beyond the table too
    noise = g.randn(B, n, 3).astype(np.float32)
    arrays = {"vert_arena": verts, "face_arena": faces, "thr_arena": thr, "frame_table": frames, "topo_table": topos}
    a = PoisonArena(DEV, 16 << 20)
    t = {k: a.input(k, torch.from_numpy(v.view(np.int32) if v.dtype == np.uint32 else v)) for k, v in arrays.items()}
    t_ids = a.input("frame_ids", torch.from_numpy(ids))
    t_noise = a.input("noise", torch.from_numpy(noise)) if with_noise else None
    key = ((7 << 32) | 5, 3, 9)
    with a.routed(meshstore, datastore):      # (the outputs are datastore._batch_outputs', for both launches)
        out = meshstore.mesh_batch_sample(t["vert_arena"], t["face_arena"], t["thr_arena"], t["frame_table"], t["topo_table"], t_ids, n, m,
                                          *key, 0.1, 0.1, 0.02, t_noise, 0.02 if with_noise else 0.0)
    _SEEN.update(a.called)
    a.check(written=[v.view(torch.uint8) if v.dtype == torch.bool else v for v in out.values()])
    assert all(bool(torch.isfinite(v).all()) for v in out.values() if v.dtype == torch.float32)       # no poison was read
    ref = mr.sample(arrays, ids, n, m, *key, 0.1, 0.1, 0.02, noise if with_noise else None, 0.02 if with_noise else 0.0)
    assert sorted(out) == sorted(mr.KEYS)
    for k in mr.KEYS:
        got = out[k].cpu().numpy()
        assert got.shape == ref[k].shape and got.dtype == ref[k].dtype, k
        same = np.array_equal(got, ref[k]) if got.dtype == np.bool_ else np.array_equal(got.view(np.uint32), ref[k].view(np.uint32))
        assert same, k
    if n:
        assert 0 < ref["cano_handle_sample_idx"].mean() < 1


def test_coverage_names_the_headers_entries():
    """Last: the table above is the header's list of entries, and the recording proxy saw each of them inside the arena."""
    from nsdp_amd import _lib
    assert sorted(COVERAGE) == _lib.declared_symbols("nsdp_meshbatch.h")
    assert all(callable(globals().get(fn)) for fn in COVERAGE.values())
    assert set(COVERAGE) <= _SEEN, sorted(set(COVERAGE) - _SEEN)
