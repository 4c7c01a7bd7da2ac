"""GPU: nsdp_mesh_corner_lists and nsdp_mesh_vertex_normals (include/nsdp_meshnormals.h) against the numpy emulation of
tests/mesh_normals_ref.py, BIT for bit: the corner lists, the faces' cross products, the fixed-order sums and the unit normals.
The shapes are tests/mesh_normals_ref.cases(): one triangle, a tetrahedron, spheres whose poles take the lane, the wave and the
workgroup form of the sum, packed batches with capacities above the totals, a shape without faces, an isolated vertex, repeated
and stale indices, faces that cancel.  Then poses, power-of-two scalings, reruns, a captured replay, and the three layouts of
``MeshTopology``."""
import numpy as np
import pytest
import torch

import mesh_normals_ref as mr

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
KEYS = ("list_offsets", "list_entries", "face_normals", "sums", "normals")
CASES = sorted(mr.cases())


def _bits(a):
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _same(got, want, what=""):
    got, want = _bits(got), _bits(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    assert np.array_equal(got, want), (what, int((got != want).sum()), np.argwhere(got != want)[:4].tolist())


def _device(verts, faces, fo, vo):
    return tuple(torch.from_numpy(np.ascontiguousarray(a)).to(DEV) for a in (verts, faces, fo, vo))


def _run(verts, faces, fo, vo):
    """The two entries on packed numpy operands (verts (vcap, 3) or (P, vcap, 3)) -> dict of device tensors."""
    from nsdp_amd import mesh_normals as mn
    tv, tf, tfo, tvo = _device(verts, faces, fo, vo)
    loff, lent = mn.mesh_corner_lists(tf, tfo, tvo, tv.shape[-2])
    normals, sums, fn = mn.mesh_vertex_normals(tv.reshape(-1, tv.shape[-2], 3), tf, tfo, tvo, loff, lent, want_sums=True)
    return {"list_offsets": loff, "list_entries": lent, "face_normals": fn, "sums": sums, "normals": normals}


@pytest.fixture(scope="module")
def reference():
    """name -> (packed numpy operands, the emulation's arrays): computed once, never changed."""
    out = {}
    for name, (shapes, vcap, fcap) in mr.cases().items():
        packed = mr.pack(shapes, vcap, fcap)
        out[name] = (packed, mr.vertex_normals(*packed))
    return out


@pytest.mark.parametrize("name", CASES)
def test_bits_of_every_output(reference, name):
    packed, want = reference[name]
    got = _run(*packed)
    for k in KEYS:
        _same(got[k][0] if k in KEYS[2:] else got[k], want[k], (name, k))
    again = _run(*packed)                                                   # two runs: the same bits
    for k in KEYS:
        assert torch.equal(got[k].view(torch.int32), again[k].view(torch.int32)), (name, k)


def test_cases_are_what_they_claim(reference):
    longest = {n: int(np.diff(reference[n][1]["list_offsets"]).max()) for n in ("lane", "wave", "workgroup")}
    assert longest == {"lane": 12, "wave": 40, "workgroup": 1100}
    (verts, faces, fo, vo), want = reference["packed"]
    assert verts.shape[0] > vo[-1] and faces.shape[0] > fo[-1]                  # capacities above the totals:
    assert not want["normals"][vo[-1]:].any() and not want["face_normals"][fo[-1]:].any()      # dead rows are zeros,
    assert want["list_offsets"][-1] == 3 * fo[-1] and not want["list_entries"][3 * fo[-1]:].any()      # dead faces in no list
    assert not reference["cancelling"][1]["sums"].any() and reference["cancelling"][1]["face_normals"].any()
    (_, faces, fo, vo), _ = reference["stale"]
    local = faces[fo[1]:fo[2]]
    assert local.min() < 0 and local.max() >= vo[2] - vo[1]                     # indices beyond their shape


def test_poses_share_one_topology(reference):
    (verts, faces, fo, vo), _ = reference["packed"]
    g = np.random.RandomState(3)
    poses = np.stack([verts, verts + 0.01 * g.randn(*verts.shape).astype(np.float32), (verts * np.float32(1.5))[:, [2, 0, 1]]])
    together = _run(poses, faces, fo, vo)
    for p in range(3):
        alone = _run(poses[p], faces, fo, vo)
        for k in KEYS[2:]:
            assert torch.equal(together[k][p].view(torch.int32), alone[k][0].view(torch.int32)), (p, k)
        _same(alone["normals"][0], mr.vertex_normals(poses[p], faces, fo, vo)["normals"], p)


def test_power_of_two_scaling_keeps_the_normals_bits():
    verts, faces, fo, vo = mr.pack([mr.sphere(4, 11)])           # (tests/test_mesh_normals_cpu.py: no subnormal on the way)
    base = _run(verts, faces, fo, vo)["normals"]
    _same(base[0], mr.vertex_normals(verts, faces, fo, vo)["normals"])
    assert bool(base.abs().sum(dim=-1).gt(0).all())
    for scale in (2.0 ** -40, 2.0 ** 40):
        scaled = _run(verts * np.float32(scale), faces, fo, vo)["normals"]
        assert torch.equal(scaled.view(torch.int32), base.view(torch.int32)), scale


def test_captured_call_replays_the_eager_bits(reference):
    from nsdp_amd import mesh_normals as mn
    (verts, faces, fo, vo), want = reference["wave"]
    tv, tf, _, _ = _device(verts, faces, fo, vo)
    topo = mn.MeshTopology(tf, tv)
    eager = mn.vertex_normals(tv, topo)
    static = tv.clone()
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        mn.vertex_normals(static, topo)                                     # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(stream)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = mn.vertex_normals(static, topo)
    moved = tv[:, [1, 2, 0]].contiguous()
    for src in (tv, moved, tv):
        static.copy_(src)
        graph.replay()
        assert torch.equal(captured.view(torch.int32), mn.vertex_normals(src, topo).view(torch.int32))
    _same(eager, want["normals"])
    _same(captured, want["normals"])


def test_topology_layouts_agree_with_single_meshes(reference):
    from nsdp_amd import mesh_normals as mn
    from nsdp_amd.ragged import RaggedPoints
    (verts, faces, _, _), want = reference["lane"]
    tv, tf = torch.from_numpy(verts).to(DEV), torch.from_numpy(faces).to(DEV)
    single = mn.MeshTopology(tf.long(), tv)                                 # (int64 faces are converted once)
    g = torch.Generator().manual_seed(5)
    batch = torch.stack([tv, tv * 2.0, tv + 0.02 * torch.randn(tv.shape, generator=g).to(DEV)])
    singles = [mn.vertex_normals(b, single) for b in batch]
    _same(singles[0], want["normals"])
    # shared [F, 3] faces over [B, V, 3]: B poses
    shared = mn.MeshTopology(tf, batch)
    n, s, f = mn.vertex_normals(batch, shared, return_sums=True, return_face_normals=True)
    assert n.shape == batch.shape and s.shape == batch.shape and f.shape == (3,) + tuple(faces.shape)
    for b in range(3):
        assert torch.equal(n[b].view(torch.int32), singles[b].view(torch.int32)), b
    _same(s[0], want["sums"])
    _same(f[0], want["face_normals"])
    _same(mn.face_normals(tv, single), want["face_normals"])
    # faces [B, F, 3] of their own
    own = mn.MeshTopology(tf.expand(3, -1, -1).contiguous(), batch)
    assert torch.equal(mn.vertex_normals(batch, own).view(torch.int32), n.view(torch.int32))
    # packed
    tet_v, tet_f = (torch.from_numpy(a).to(DEV) for a in mr.tetrahedron())
    rv = RaggedPoints.from_list([tv, tet_v, tv * 2.0], capacity=170)
    rf = RaggedPoints.from_rows([tf, tet_f, tf], capacity=300)
    ragged = mn.MeshTopology(rf, rv)
    out = torch.full_like(rv.packed, float("nan"))
    rn = mn.vertex_normals(rv, ragged, out=out)
    assert isinstance(rn, RaggedPoints) and rn.packed.data_ptr() == out.data_ptr() and rn.offsets is rv.offsets
    parts = rn.split()
    assert torch.equal(parts[0].view(torch.int32), singles[0].view(torch.int32)) and torch.equal(parts[2].view(torch.int32), singles[1].view(torch.int32))
    _same(parts[1], mr.vertex_normals(*mr.pack([mr.tetrahedron()]))["normals"])
    assert not out[rv.total:].any()                                         # rows nobody owns: written, as zeros


def test_topology_refuses_a_face_index_outside_its_shape():
    from nsdp_amd import mesh_normals as mn
    from nsdp_amd.ragged import RaggedPoints
    tet_v, tet_f = (torch.from_numpy(a).to(DEV) for a in mr.tetrahedron())
    bad = tet_f.clone()
    bad[2, 1] = 4
    with pytest.raises(mn.MeshNormalsError, match=r"face row 2 of shape 0 names the vertices \[0, 4, 1\], outside \[0, 4\) \(1 such"):
        mn.MeshTopology(bad, tet_v)
    rv = RaggedPoints.from_list([tet_v, tet_v[:3]])
    with pytest.raises(mn.MeshNormalsError, match=r"face row 5 of shape 1 names the vertices \[0, 2, 3\], outside \[0, 3\)"):
        mn.MeshTopology(RaggedPoints.from_rows([tet_f, tet_f[:2]]), rv)     # local to the shape: 3 is inside the packed set
    topo = mn.MeshTopology(bad, tet_v, validate=False)                      # clamped, as the header says
    clamped = tet_f.clone()
    clamped[2, 1] = 3
    assert torch.equal(mn.vertex_normals(tet_v, topo).view(torch.int32), mn.vertex_normals(tet_v, mn.MeshTopology(clamped, tet_v)).view(torch.int32))
    with pytest.raises(mn.MeshNormalsError, match="must be float32"):
        mn.vertex_normals(tet_v.double(), topo)
    with pytest.raises(mn.MeshNormalsError, match="GPU tensor"):
        mn.vertex_normals(tet_v.cpu(), topo)
    with pytest.raises(mn.MeshNormalsError, match=r"verts \(5, 3\) against a topology over \[\.\.\., 4, 3\]"):
        mn.vertex_normals(torch.zeros((5, 3), device=DEV), topo)
