"""Both entries of include/nsdp_batch.h inside the poisoned arena of tests/poison_arena.py: every operand between 256 KiB guards,
outputs poisoned until the kernels write them.  The operand set ends on a PARTIAL last frame (its table entry claims more rows
than the arenas hold) and the frame ids, row indices and row counts carry out-of-range values: as the header says they are
clamped as they are read, so the results are those of the clamped operands -- no stray write, no output element left
unwritten, no read of memory nobody wrote (the poison is NaN in fp16 and fp32 alike)."""
import numpy as np
import pytest
import torch

import subset_ref as sr
from poison_arena import PoisonArena

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
COVERAGE = {"nsdp_subset_draw": "test_draw_inside_the_arena", "nsdp_batch_assemble": "test_assemble_inside_the_arena"}
_SEEN: set = set()


def test_draw_inside_the_arena():
    from nsdp_amd import datastore
    a = PoisonArena(DEV, 8 << 20)
    n_full = [7, 0, -5, 1 << 30, 300, 1]                      # as read: 7, 1, 1, 2^20, 300, 1
    seen = [7, 1, 1, 1 << 20, 300, 1]
    counts = a.input("n_full", torch.tensor(n_full, dtype=torch.int32))
    with a.routed(datastore):
        rows = datastore.subset_draw(counts, 300, seed=12, epoch=3, step=4, which=sr.SPACE)
    _SEEN.update(a.called)
    a.check(written=[rows])
    got = rows.cpu().numpy()
    assert np.array_equal(got, sr.draw(seen, 300, 12, 3, 4, sr.SPACE))
    for r, n in zip(got, seen):
        assert r.min() >= 0 and r.max() < n and len(np.unique(r)) == min(n, 300)


def _table(entries):
    """(first surface record, first space record, surface rows, space rows, bbox (6,)) per frame -> (F, 6) int64."""
    t = np.zeros((len(entries), 6), dtype=np.int64)
    for k, (s0, q0, sn, qn, box) in enumerate(entries):
        t[k, 0], t[k, 1] = s0, q0
        t[k, 2] = (sn & 0xFFFFFFFF) | (qn << 32)
        t[k, 3:6] = np.asarray(box, dtype=np.float32).view(np.int64)
    return t


def _clamped_reference(surface, space, entries, ids, surf_idx, space_idx, m, partial_range, noise, level):
    """The header's contract in numpy, clamps included.  surface (S, 6) / space (Q, 4) float32 (converted exactly)."""
    S, Q, F = len(surface), len(space), len(entries)
    B, n = surf_idx.shape
    clamp = lambda v, lo, hi: lo if v < lo else (hi if v > hi else v)
    out = {"surface": np.zeros((6, B, n, 3), np.float32), "handle": np.zeros((B, n), np.uint8),
           "inputs": np.zeros((B, n, 7), np.float32), "space": np.zeros((3, B, m, 3), np.float32)}
    for b in range(B):
        fr = []
        for c in range(3):
            s0, q0, sn, qn, box = entries[clamp(int(ids[c, b]), 0, F - 1)]
            sn, qn = clamp(sn, 0, S), clamp(qn, 0, Q)
            fr.append((clamp(s0, 0, S - sn), clamp(q0, 0, Q - qn), sn, qn, np.asarray(box, np.float32)))
        for j in range(n):
            rec = [surface[clamp(f[0] + clamp(int(surf_idx[b, j]), 0, max(f[2] - 1, 0)), 0, S - 1)] for f in fr]
            cano, src, tgt = (r[:3].copy() for r in rec)
            if noise is not None:
                src = src + np.float32(level) * noise[b, j]
            box = fr[0][4]
            pr = np.float32(partial_range)
            handle = bool(cano[1] < box[1] + pr) | bool(cano[1] > box[4] - pr) | bool(cano[2] < box[2] + pr)
            for c, r in enumerate((cano, src, tgt)):
                out["surface"][c, b, j] = r
                out["surface"][3 + c, b, j] = rec[c][3:]
            out["handle"][b, j] = handle
            out["inputs"][b, j] = np.concatenate([src, tgt * np.float32(handle), [np.float32(handle)]])
        for j in range(m):
            row = j if space_idx is None else int(space_idx[b, j])
            for c, f in enumerate(fr):
                out["space"][c, b, j] = space[clamp(f[1] + clamp(row, 0, max(f[3] - 1, 0)), 0, Q - 1)][:3]
    return out


@pytest.mark.parametrize("f16", [True, False])
@pytest.mark.parametrize("with_space_idx,with_noise", [(True, True), (False, False)])
def test_assemble_inside_the_arena(f16, with_space_idx, with_noise):
    from nsdp_amd import datastore
    g = np.random.RandomState(5)
    dtype = np.float16 if f16 else np.float32
    S, Q, B, n, m = 700, 500, 4, 300, 260          # more than one 256-lane block per part, neither a multiple of it
    surface = (g.rand(S, 6) - 0.5).astype(dtype)
    space = np.zeros((Q, 4), dtype)
    space[:, :3] = (g.rand(Q, 3) - 0.5).astype(dtype)
    box = lambda: np.concatenate([-0.5 + 0.2 * g.rand(3), 0.5 - 0.2 * g.rand(3)]).astype(np.float32)
    # three whole frames; the last entry is PARTIAL: it claims 300 + 300 rows from record 600 / 400, beyond both arenas; a fifth
    # entry is corrupt throughout (negative first record, counts beyond the arenas)
    entries = [(0, 0, 200, 150, box()), (200, 150, 250, 100, box()), (450, 250, 150, 150, box()), (600, 400, 300, 300, box()),
               (-7, 1 << 40, 1 << 30, 100000, box())]
    ids = np.array([[0, 3, 9, -2], [1, 3, 4, 2], [2, 4, 0, 3]], dtype=np.int32)                  # (3, B): ids beyond the table too
    surf_idx = g.randint(0, 150, size=(B, n)).astype(np.int32)
    surf_idx[:, ::17] = [[-1], [1 << 30], [-(1 << 31)], [100000]]
    space_idx = g.randint(0, 100, size=(B, m)).astype(np.int32)
    space_idx[:, ::13] = [[1 << 30], [-4], [99999], [-(1 << 31)]]
    noise = g.randn(B, n, 3).astype(np.float32)
    a = PoisonArena(DEV, 16 << 20)
    t_surface, t_space = a.input("surface_arena", torch.from_numpy(surface)), a.input("space_arena", torch.from_numpy(space))
    t_table = a.input("frame_table", torch.from_numpy(_table(entries)))
    t_ids, t_surf = a.input("frame_ids", torch.from_numpy(ids)), a.input("surf_idx", torch.from_numpy(surf_idx))
    t_sp = a.input("space_idx", torch.from_numpy(space_idx)) if with_space_idx else None
    t_noise = a.input("noise", torch.from_numpy(noise)) if with_noise else None
    with a.routed(datastore):
        out = datastore.batch_assemble(t_surface, t_space, t_table, t_ids, t_surf, t_sp, m, 0.1, t_noise, 0.02 if with_noise else 0.0)
    _SEEN.update(a.called)
    a.check(written=[v.view(torch.uint8) if v.dtype == torch.bool else v for v in out.values()])
    assert all(bool(torch.isfinite(v).all()) for v in out.values() if v.dtype == torch.float32)       # no poison was read
    ref = _clamped_reference(surface.astype(np.float32), space.astype(np.float32), entries, ids, surf_idx,
                             space_idx if with_space_idx else None, m, 0.1, noise if with_noise else None, 0.02)
    names = ["surface_samples_cano", "surface_samples_src", "surface_samples_tgt", "surface_normals_cano", "surface_normals_src",
             "surface_normals_tgt"]
    for c, name in enumerate(names):
        np.testing.assert_array_equal(out[name].cpu().numpy(), ref["surface"][c], err_msg=name)
    for c, name in enumerate(("space_samples_cano", "space_samples_src", "space_samples_tgt")):
        np.testing.assert_array_equal(out[name].cpu().numpy(), ref["space"][c], err_msg=name)
    np.testing.assert_array_equal(out["cano_handle_sample_idx"][..., 0].cpu().numpy(), ref["handle"].astype(bool))
    np.testing.assert_array_equal(out["surface_samples_inputs"].cpu().numpy(), ref["inputs"])
    assert 0 < ref["handle"].mean() < 1


def test_coverage_names_the_headers_entries():
    """Last: the table above is the header's list of entries, and the recording proxy saw each of them inside the arena."""
    from nsdp_amd import _lib
    assert sorted(COVERAGE) == _lib.declared_symbols("nsdp_batch.h")
    assert all(callable(globals().get(fn)) for fn in COVERAGE.values())
    assert set(COVERAGE) <= _SEEN, sorted(set(COVERAGE) - _SEEN)
