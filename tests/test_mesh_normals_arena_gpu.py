"""The launching entries of include/nsdp_meshnormals.h inside the poisoned arena of tests/poison_arena.py, as
tests/test_mesh_whole_arena_gpu.py holds the entry of include/nsdp_meshwhole.h: every operand between 256 KiB guards, the
workspace exactly the bytes the size query declares and poisoned on entry (the call initialises what it reads of it), the lists,
the face normals, the sums and the normals poisoned until the kernels write them -- every element of them, rows nobody owns
included -- and no byte changed outside them.  The rows nobody owns hold poison on the way IN as well: vertex rows behind the
totals are NaN, face rows behind the totals name vertices far outside everything, and one shape's faces carry stale indices.
The results are the emulation's bits all the same (tests/mesh_normals_ref.py), so nothing nobody wrote was read and every index
was clamped before it formed an address."""
import numpy as np
import pytest
import torch

import mesh_normals_ref as mr
from poison_arena import PoisonArena

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
COVERAGE = {"nsdp_mesh_corner_lists": "test_lists_and_normals_inside_the_arena",
            "nsdp_mesh_vertex_normals": "test_lists_and_normals_inside_the_arena"}
HOST_ONLY = {"nsdp_mesh_corner_lists_workspace_bytes"}
_SEEN: set = set()


def _bits(t):
    a = t.detach().cpu().numpy()
    return a.view(np.uint32) if a.dtype == np.float32 else a


@pytest.mark.parametrize("name,poses,want_sums", [("packed", 1, True), ("stale", 2, False), ("workgroup", 1, True), ("no_faces", 3, True),
                                                   ("triangle", 1, False)])
def test_lists_and_normals_inside_the_arena(name, poses, want_sums):
    from nsdp_amd import mesh_normals as mn
    shapes, vcap, fcap = mr.cases()[name]
    verts, faces, fo, vo = mr.pack(shapes, vcap, fcap)
    want = mr.vertex_normals(verts, faces, fo, vo)
    verts[vo[-1]:] = np.nan                                                # rows nobody owns: poison on the way in
    faces[fo[-1]:] = np.array([-1, 1 << 30, -(1 << 31)], np.int32)
    stack = np.stack([verts * np.float32(1 + p) for p in range(poses)])   # (a power of two or not: the first pose is the emulated one)
    a = PoisonArena(DEV, 32 << 20)
    tv, tf = a.input("verts", torch.from_numpy(stack)), a.input("faces", torch.from_numpy(faces))
    tfo, tvo = a.input("face_offsets", torch.from_numpy(fo)), a.input("vert_offsets", torch.from_numpy(vo))
    with a.routed(mn):
        loff, lent = mn.mesh_corner_lists(tf, tfo, tvo, verts.shape[0])
        normals, sums, fn = mn.mesh_vertex_normals(tv, tf, tfo, tvo, loff, lent, want_sums=want_sums)
    _SEEN.update(a.called)
    outs = [loff, lent, normals, fn] + ([sums] if want_sums else [])
    assert all(a._region_of(t)[0] is not None for t in outs) and (sums is None) == (not want_sums)
    workspace = [r for r in a.regions if r.kind == "routed"][0]
    assert workspace.nbytes == mn.lib().nsdp_mesh_corner_lists_workspace_bytes(len(fo) - 1, verts.shape[0], faces.shape[0])
    a.check(written=outs)
    assert all(bool(torch.isfinite(t).all()) for t in outs if t.dtype == torch.float32)       # no poison was read
    assert np.array_equal(_bits(loff), want["list_offsets"]) and np.array_equal(_bits(lent), want["list_entries"])
    assert np.array_equal(_bits(fn[0]), want["face_normals"].view(np.uint32))
    assert np.array_equal(_bits(normals[0]), want["normals"].view(np.uint32))
    if want_sums:
        assert np.array_equal(_bits(sums[0]), want["sums"].view(np.uint32))
    for p in range(1, poses):
        again = mr.vertex_normals(stack[p], faces, fo, vo)["normals"]
        assert np.array_equal(_bits(normals[p]), again.view(np.uint32)), p


def test_coverage_names_the_headers_entries():
    """Last: the table above is the header's list of launching entries, and the recording proxy saw each of them inside the arena."""
    from nsdp_amd import _lib
    assert sorted(set(COVERAGE) | HOST_ONLY) == _lib.declared_symbols("nsdp_meshnormals.h")
    assert all(callable(globals().get(fn)) for fn in COVERAGE.values())
    if _SEEN:                                                              # (run alone, this test has nothing to compare)
        assert set(COVERAGE) <= _SEEN, sorted(set(COVERAGE) - _SEEN)
