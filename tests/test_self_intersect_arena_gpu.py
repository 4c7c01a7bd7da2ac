"""The launching entry of include/nsdp_selfintersect.h inside the poisoned arena of tests/poison_arena.py, in the pattern of
tests/test_mesh_normals_arena_gpu.py: every operand between 256 KiB guards, the workspace exactly the bytes the size query
declares and poisoned on entry (the call initialises what it reads of it), every output poisoned until the kernels write it --
every element, rows nobody owns included -- and no byte changed outside them.  -1 is a VALUE of hits_out and partner_out and
also the arena's poison read as int32, so these two are refilled with a second pattern before the call and held to it.  The
rows nobody owns hold poison on the way IN as well: vertex rows behind the totals are NaN, face rows behind the totals name
vertices far outside everything, face_ids behind the totals are wild, and one mesh's faces carry stale indices.  The results
are the emulation's bytes all the same (tests/self_intersect_ref.py), so nothing nobody wrote was read and every index was
clamped before it formed an address."""
import ctypes

import numpy as np
import pytest
import torch

import self_intersect_ref as sr
from poison_arena import PoisonArena

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
COVERAGE = {"nsdp_mesh_self_intersections": "test_entry_inside_the_arena"}
HOST_ONLY = {"nsdp_mesh_self_intersections_workspace_bytes"}
SECOND = 0x5A5A5A5A
_SEEN: set = set()


def _soup(n, seed):
    rng = np.random.default_rng(seed)
    v = (rng.uniform(-1, 1, (n, 1, 3)) + rng.normal(0, 0.25, (n, 3, 3))).reshape(-1, 3).astype(np.float32)
    return v, np.arange(3 * n).reshape(n, 3).astype(np.int32)


def _case(name):
    spheres = sr.inputs()["spheres"]
    if name == "packed":
        return [_soup(65, 1), spheres, (np.zeros((3, 3), np.float32), np.zeros((0, 3), np.int32)), _soup(129, 2)], 5, 70
    if name == "stale":
        v, f = _soup(100, 3)
        f = f.copy()
        f[::7] += 1 << 20                                                  # stale indices: clamped into the mesh
        f[1::9] = -4
        return [(v, f), spheres], 3, 1
    if name == "triangle":
        return [_soup(1, 4)], 0, 0
    raise KeyError(name)


@pytest.mark.parametrize("name,poses,budget,ids,cull", [("packed", 1, 0, False, True), ("packed", 2, 5, True, True),
                                                        ("stale", 1, 7, True, False), ("triangle", 3, 0, False, True)])
def test_entry_inside_the_arena(name, poses, budget, ids, cull):
    from nsdp_amd import _lib
    meshes, vpad, fpad = _case(name)
    verts, faces, fo, vo = sr.pack(meshes, vpad=vpad, fpad=fpad)
    face_ids = None
    if ids:                                                                # every mesh's rows reversed under face_ids
        face_ids = np.arange(len(faces), dtype=np.int32)
        shuffled = faces.copy()
        for b in range(len(meshes)):
            face_ids[fo[b]:fo[b + 1]] = np.arange(fo[b], fo[b + 1])[::-1]
            shuffled[fo[b]:fo[b + 1]] = faces[fo[b]:fo[b + 1]][::-1]
        faces = shuffled
    stack = np.stack([verts * np.float32(1 + 0.5 * p) for p in range(poses)])
    want = [sr.self_intersections(stack[p], faces, fo, vo, face_ids=face_ids, budget=budget) for p in range(poses)]
    stack[:, vo[-1]:] = np.nan                                             # rows nobody owns: poison on the way in
    faces[fo[-1]:] = np.array([-1, 1 << 30, -(1 << 31)], np.int32)
    if ids:
        face_ids[fo[-1]:] = -(1 << 31)
    P, B, vcap, fcap = poses, len(fo) - 1, verts.shape[0], faces.shape[0]
    a = PoisonArena(DEV, 32 << 20)
    tv, tf = a.input("verts", torch.from_numpy(stack)), a.input("faces", torch.from_numpy(faces))
    tfo, tvo = a.input("face_offsets", torch.from_numpy(fo)), a.input("vert_offsets", torch.from_numpy(vo))
    tid = a.input("face_ids", torch.from_numpy(face_ids)) if ids else None
    with a.routed():
        L = _lib.lib()
        size = L.nsdp_mesh_self_intersections_workspace_bytes
        size.restype = ctypes.c_size_t
        need = int(size(P, B, fcap))
        assert need == 4 * P * (10 * fcap + 6 * (fcap // 64 + B + 1))
        ws = a.workspace("workspace", need)
        cand, hits, partner = (a.output(n, (P, fcap), torch.int32) for n in ("cand", "hits", "partner"))
        pairs, skipped = a.output("pairs", (P, B), torch.int64), a.output("skipped", (P, B), torch.int32)
        hits.fill_(SECOND), partner.fill_(SECOND)
        ptr = lambda t: ctypes.c_void_p(0 if t is None else t.data_ptr())
        rc = L.nsdp_mesh_self_intersections(ptr(tv), P, ptr(tvo), ptr(tf), ptr(tfo), ptr(tid), B, vcap, fcap, budget, 0 if cull else 1,
                                            ptr(ws), ptr(cand), ptr(hits), ptr(partner), ptr(pairs), ptr(skipped),
                                            _lib.stream_ptr())
        assert rc == 0, _lib.lib().nsdp_last_error()
    _SEEN.update(a.called)
    a.check(written=[cand, pairs, skipped])
    assert not bool((hits == SECOND).any()) and not bool((partner == SECOND).any())      # every element written
    for p in range(poses):
        for k, t in (("cand", cand), ("hits", hits), ("partner", partner), ("pairs", pairs), ("skipped", skipped)):
            assert np.array_equal(t[p].cpu().numpy(), want[p][k]), (k, p)
    assert sum(int(w["pairs"].sum()) for w in want) > 0 or name == "triangle"


def test_coverage_names_the_headers_entries():
    """Last: the table above is the header's list of launching entries, and the recording proxy saw each of them inside the arena."""
    from nsdp_amd import _lib
    assert sorted(set(COVERAGE) | HOST_ONLY) == _lib.declared_symbols("nsdp_selfintersect.h")
    assert all(callable(globals().get(fn)) for fn in COVERAGE.values())
    if _SEEN:                                                              # (run alone, this test has nothing to compare)
        assert set(COVERAGE) <= _SEEN, sorted(set(COVERAGE) - _SEEN)
