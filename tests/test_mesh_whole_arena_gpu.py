"""The entry of include/nsdp_meshwhole.h inside the poisoned arena of tests/poison_arena.py: every operand between 256 KiB guards,
outputs of exactly their declared size and poisoned until the kernels write them.  The tables are STALE, as in
tests/test_mesh_store_arena_gpu.py: entries claim more vertices and faces than the arenas hold, first records lie before and
beyond them, topology and frame ids point outside the tables and the face arena holds vertex indices outside every frame.  As the
header says, everything is clamped as it is read, so the results are those of the clamped operands (tests/mesh_whole_ref.py
applies the same clamps) -- no stray write, no output byte left unwritten (padding and truncated batches included), no read of
memory nobody wrote (the poison is NaN)."""
import numpy as np
import pytest
import torch

import mesh_whole_ref as wr
from poison_arena import PoisonArena

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
COVERAGE = {"nsdp_mesh_batch_whole": "test_whole_inside_the_arena"}
_SEEN: set = set()


def _frame(first, count, topo, box):
    e = np.zeros(6, dtype=np.int64)
    e[0], e[1], e[2] = first, (count & 0xFFFFFFFF) | (topo << 32), -1
    e[3:6] = np.asarray(box, dtype=np.float32).view(np.int64)
    return e


def _stale():
    g = np.random.RandomState(11)
    V, FR = 500, 400
    verts = np.zeros((V, 4), np.float32)
    verts[:, :3] = g.rand(V, 3) - 0.5
    faces = np.zeros((FR, 4), np.int32)
    faces[:, :3] = g.randint(0, 120, size=(FR, 3))
    faces[::7, 0], faces[3::11, 1], faces[5::13, 2] = -3, 1 << 30, -(1 << 31)          # vertex indices outside every frame
    faces[:, 3] = g.randint(-9, 9, size=FR)                                              # (the padding is never used)
    box = lambda: np.concatenate([-0.5 + 0.3 * g.rand(3), 0.5 - 0.3 * g.rand(3)]).astype(np.float32)
    frames = np.stack([
        _frame(0, 120, 0, box()), _frame(120, 120, 0, box()), _frame(240, 150, 1, box()),
        _frame(390, 300, 1, box()),                      # PARTIAL: 300 vertices from record 390 of 500
        _frame(-7, 1 << 30, 9, box()),                   # corrupt throughout: topology 9 of 4, a count beyond the arena
        _frame(1 << 40, -5, -2, box()),                  # negative count and topology
        _frame(450, 50, 2, box()),                       # topology 2 is PARTIAL
        _frame(10, 0, 3, box())])                        # no vertices; topology 3 has no faces
    topos = np.array([[0, 100], [100, 150], [300, 200], [1 << 35, 0]], dtype=np.int64)      # [2]: 200 faces from record 300 of 400
    ids = np.array([[0, 3, 4, 6, 7, 5, 2], [1, 3, 44, 5, 2, 0, 6], [2, 0, -3, 7, 1 << 30, 1, 4]], dtype=np.int32)      # ids beyond the table too
    return {"vert_arena": verts, "face_arena": faces, "frame_table": frames, "topo_table": topos}, ids


@pytest.mark.parametrize("vcap,fcap", [(None, None), (1300, 1000), (700, 260), (1, 1)])
def test_whole_inside_the_arena(vcap, fcap):
    from nsdp_amd import meshstore
    arrays, ids = _stale()
    counts = wr.counts(arrays, ids)
    assert counts == [(120, 100), (300, 150), (500, 0), (50, 200), (0, 0), (0, 100), (150, 150)]      # every clamp of the counts bites
    tv, tf = sum(v for v, _ in counts), sum(f for _, f in counts)
    vcap, fcap = (tv if vcap is None else vcap), (tf if fcap is None else fcap)                        # exact, padded, truncating
    a = PoisonArena(DEV, 16 << 20)
    t = {k: a.input(k, torch.from_numpy(v)) for k, v in arrays.items()}
    t_ids = a.input("frame_ids", torch.from_numpy(ids))
    with a.routed(meshstore):
        out = meshstore.mesh_batch_whole(t["vert_arena"], t["face_arena"], t["frame_table"], t["topo_table"], t_ids, vcap, fcap, 0.1)
    _SEEN.update(a.called)
    assert sorted(out) == sorted(wr.KEYS) and all(a._region_of(v)[0] is not None for v in out.values())
    # handle bytes and face words may legitimately be 0xFF.. only as poison: a written byte is 0 or 1, a written index >= 0
    a.check(written=list(out.values()))
    assert all(bool(torch.isfinite(v).all()) for v in out.values() if v.dtype == torch.float32)       # no poison was read
    ref = wr.whole(arrays, ids, vcap, fcap, 0.1)
    for k in wr.KEYS:
        got = out[k].cpu().numpy()
        assert got.shape == ref[k].shape and got.dtype == ref[k].dtype, k
        assert np.array_equal(got.view(np.uint32) if got.dtype == np.float32 else got, ref[k].view(np.uint32) if got.dtype == np.float32 else ref[k]), k
    if vcap >= tv:
        assert 0 < ref["handle"][:tv].mean() < 1 and ref["vert_offsets"][-1] == tv and ref["face_offsets"][-1] == tf


def test_coverage_names_the_headers_entries():
    """Last: the table above is the header's list of entries, and the recording proxy saw each of them inside the arena."""
    from nsdp_amd import _lib
    assert sorted(COVERAGE) == _lib.declared_symbols("nsdp_meshwhole.h")
    assert all(callable(globals().get(fn)) for fn in COVERAGE.values())
    assert set(COVERAGE) <= _SEEN, sorted(set(COVERAGE) - _SEEN)
