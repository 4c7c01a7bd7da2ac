"""GPU: whole meshes of a batch out of the mesh store (include/nsdp_meshwhole.h, MeshStore.whole_meshes).  The kernel against the
numpy emulation of its rule (tests/mesh_whole_ref.py) bit for bit on all six outputs, padding and truncation included, over frames
whose ends fall inside a wave, on a wave edge and beyond a workgroup; the store's call against ``store.mesh`` and the torch handle
rule on a tree from disk; ``inverse``; a captured call replayed for another batch."""
import numpy as np
import pytest
import torch

import mesh_sample_ref as mr
import mesh_whole_ref as wr
from nsdp_amd import dataset, meshstore, synth
from nsdp_amd.ragged import RaggedPoints

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
PARTIAL_RANGE = 0.1
VERTS = (0, 1, 4, 63, 64, 65, 257, 5000)      # shape ends inside a wave, on a wave edge, beyond a 256-lane workgroup
TOPO_OF = (0, 0, 1, 2, 2, 2, 2, 3)            # topologies of 0, 1, 200 and 9000 faces


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _assert_bit_equal(got, want, what=""):
    assert sorted(got) == sorted(wr.KEYS)
    for k in wr.KEYS:
        g = got[k].cpu().numpy()
        assert g.shape == want[k].shape and g.dtype == want[k].dtype, (what, k, g.shape, want[k].shape, g.dtype)
        assert np.array_equal(_bits(g), _bits(want[k])), (what, k, int((_bits(g) != _bits(want[k])).sum()))


@pytest.fixture(scope="module")
def frames():
    """24 frames: three (A, B, C) of each vertex count, all of one count over one topology.  The 200-face topology names vertices
    up to 256, so on the frames of 63 to 65 vertices its indices are clamped; the one-face topology names vertex 3 of 4."""
    g = np.random.RandomState(5)
    verts = [(g.rand(v, 3) - 0.5).astype(np.float32) for v in VERTS for _ in range(3)]
    verts[3 * 6][:3, 1] = [-0.6, 0.6, 0.0]                                  # (a box wide enough for both y bounds to decide)
    faces = [np.zeros((0, 3), np.int32), np.array([[0, 3, 2]], np.int32), g.randint(0, 257, size=(200, 3)).astype(np.int32),
             g.randint(0, 5000, size=(9000, 3)).astype(np.int32)]
    arrays = meshstore.pack(verts, [t for t in TOPO_OF for _ in range(3)], faces, [])
    dev = {k: torch.from_numpy(v.view(np.int32) if v.dtype == np.uint32 else v).to(DEV) for k, v in arrays.items()}
    return arrays, dev


def _launch(dev, ids, vcap, fcap, partial_range=PARTIAL_RANGE):
    return meshstore.mesh_batch_whole(dev["vert_arena"], dev["face_arena"], dev["frame_table"], dev["topo_table"],
                                      torch.from_numpy(ids).to(DEV), vcap, fcap, partial_range)


def _ids(B):
    f = lambda count, variant: 3 * VERTS.index(count) + variant
    if B == 1:
        return np.array([[f(257, 0)], [f(257, 1)], [f(257, 2)]], dtype=np.int32)
    # nine shapes: every count, the largest first, the 64-vertex frame twice (a repeated frame); shape 6 (65 vertices) reads a
    # SOURCE frame of 257 vertices and shape 7 (257) a source of 63 and a target of 1: the canonical count rules, the first
    # record is clamped so that the count fits the arena
    cano = [f(5000, 0), f(0, 0), f(1, 0), f(4, 0), f(63, 0), f(64, 0), f(65, 0), f(257, 0), f(64, 0)]
    src = [f(5000, 1), f(0, 1), f(1, 1), f(4, 1), f(63, 1), f(64, 1), f(257, 1), f(63, 1), f(64, 0)]
    tgt = [f(5000, 2), f(0, 2), f(1, 2), f(4, 2), f(63, 2), f(64, 2), f(65, 2), f(1, 2), f(64, 2)]
    return np.array([cano, src, tgt], dtype=np.int32)


@pytest.mark.parametrize("B", [1, 9])
def test_kernel_equals_the_emulation_bit_for_bit(frames, B):
    arrays, dev = frames
    ids = _ids(B)
    counts = wr.counts(arrays, ids)
    tv, tf = sum(v for v, _ in counts), sum(f for _, f in counts)
    assert (tv, tf) == ((257, 200) if B == 1 else (5000 + 1 + 4 + 63 + 64 + 65 + 257 + 64, 9000 + 1 + 5 * 200))
    for vcap, fcap in ((tv, tf), (tv + 77, tf + 77), (tv - 100, tf - 150), (130, 7), (1, 1)):      # exact, padded, three truncations
        got = _launch(dev, ids, vcap, fcap)
        want = wr.whole(arrays, ids, vcap, fcap, PARTIAL_RANGE)
        _assert_bit_equal(got, want, (B, vcap, fcap))
    want = wr.whole(arrays, ids, tv, tf, PARTIAL_RANGE)
    assert 0 < want["handle"].mean() < 1 and want["vert_offsets"][-1] == tv and want["face_offsets"][-1] == tf
    assert np.signbit(want["inputs"][:, 3:6][want["handle"] == 0]).any()                # -x * 0 = -0 is there to be matched
    if B == 9:
        assert want["faces"][9000:9001].tolist() == [[0, 3, 2]]                           # the one-face topology on 4 vertices
        rows = slice(int(want["face_offsets"][4]), int(want["face_offsets"][5]))            # 200 faces on 63 vertices: clamped
        assert want["faces"][rows].max() == 62 and arrays["face_arena"][1:201, :3].max() > 64


def test_the_handle_rule_decides_on_each_bound(frames):
    """One frame placed by hand with partial_range = 1/8 (exact in fp32): vertices ON a bound are no handles, the next float is."""
    lo, hi = np.float32(0.125), np.float32(0.875)
    v = np.array([[0, 0, 0], [0, 1, 1], [0.5, lo, 0.5], [0.5, np.nextafter(lo, np.float32(0)), 0.5], [0.5, hi, 0.5],
                  [0.5, np.nextafter(hi, np.float32(1)), 0.5], [0.5, 0.5, lo], [0.5, 0.5, np.nextafter(lo, np.float32(0))],
                  [0.5, 0.5, hi]], dtype=np.float32)
    arrays = meshstore.pack([v, -v], [0, 0], [np.array([[0, 1, 2]], np.int32)], [])
    dev = {k: torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).to(DEV) for k, a in arrays.items()}
    ids = np.array([[0], [0], [1]], dtype=np.int32)
    got = _launch(dev, ids, 9, 1, 0.125)
    _assert_bit_equal(got, wr.whole(arrays, ids, 9, 1, 0.125))
    assert got["handle"].tolist() == [1, 1, 0, 1, 0, 1, 0, 1, 0]
    assert torch.equal(got["verts"][0], got["verts"][1]) and torch.equal(got["verts"][2], -got["verts"][0])      # cano = src


# ------------------------------------------------------------------------------------------------------------------ the store
@pytest.fixture(scope="module")
def mesh_tree(tmp_path_factory):
    meshes = {"tet": mr.tetrahedron(), "oct": mr.octahedron(), "grid": mr.grid()}
    return synth.write_mesh_dataset_tree(str(tmp_path_factory.mktemp("whole")), meshes, ["walk", "jump", "turn"], 3, seed=9)


def test_whole_meshes_hold_the_stores_frames(mesh_tree):
    store = meshstore.MeshStore({"data": mesh_tree}, "identity_seen", "test_unseen_motions", device=DEV)
    picks = [0, 4, 8, 3, 4]                                                              # three topologies, a pair twice
    host = np.ascontiguousarray(store.pair_frames[picks].T)
    ids = torch.from_numpy(host).to(DEV)
    out = store.whole_meshes(ids, host)
    assert sorted(out) == ["cano_handle_vert_idx", "faces", "verts_cano", "verts_flow_inputs", "verts_src", "verts_tgt"]
    sets = [out[f"verts_{k}"] for k in ("cano", "src", "tgt")]
    counts = tuple(int(store.mesh(int(c))[0].shape[0]) for c in host[0])
    assert all(isinstance(s, RaggedPoints) and s.offsets is sets[0].offsets and s._counts == counts for s in sets)
    assert sets[0].capacity == sum(counts) and out["verts_flow_inputs"].packed.shape == (sum(counts), 7)
    assert out["faces"].packed.dtype == torch.int32 and out["faces"].capacity == sum(out["faces"]._counts)
    assert out["cano_handle_vert_idx"].shape == (sum(counts), 1) and out["cano_handle_vert_idx"].dtype == torch.bool
    pr = float(mesh_tree["partial_range"])
    for b in range(len(picks)):
        meshes = [store.mesh(int(host[c, b])) for c in range(3)]
        for c in range(3):
            assert torch.equal(sets[c].split()[b].view(torch.int32), meshes[c][0].view(torch.int32)), (b, c)
        assert torch.equal(out["faces"].split()[b], meshes[0][1]), b
        lo, hi = (torch.from_numpy(x.copy()).to(DEV) for x in store.frame_bbox(int(host[0, b])))
        mask = dataset.cano_sample_handle_mask(pr, meshes[0][0][None], lo[None], hi[None])[0].reshape(-1, 1)
        want = torch.cat([meshes[1][0], meshes[2][0] * mask.float(), mask.float()], dim=1)
        assert torch.equal(out["verts_flow_inputs"].split()[b].view(torch.int32), want.view(torch.int32)), b
        assert torch.equal(out["cano_handle_vert_idx"][sets[0].offsets[b]:sets[0].offsets[b + 1]], mask.bool()), b
    assert 0 < out["cano_handle_vert_idx"].float().mean() < 1
    # given capacities: padding behind the totals; below the totals: refused from the host table, before the launch
    padded = store.whole_meshes(ids, host, capacity=sum(counts) + 77, face_capacity=out["faces"].capacity + 5)
    assert torch.equal(padded["verts_tgt"].packed[:sum(counts)], sets[2].packed) and not padded["verts_tgt"].packed[sum(counts):].any()
    assert not padded["faces"].packed[out["faces"].capacity:].any()
    with pytest.raises(meshstore.MeshStoreError, match="do not fit the capacities"):
        store.whole_meshes(ids, host, capacity=sum(counts) - 1)
    # inverse swaps the source and the target plane
    inv = meshstore.MeshStore({"data": dict(mesh_tree, inverse=True)}, "identity_seen", "test_unseen_motions", device=DEV)
    swapped = inv.whole_meshes(ids, host)
    assert torch.equal(swapped["verts_src"].packed, sets[2].packed) and torch.equal(swapped["verts_tgt"].packed, sets[1].packed)
    assert torch.equal(swapped["verts_cano"].packed, sets[0].packed)
    assert torch.equal(swapped["verts_flow_inputs"].packed[:, :3], sets[2].packed)
    assert not torch.equal(sets[1].packed, sets[2].packed)


def test_eval_loader_walks_the_split_in_order(mesh_tree):
    store = meshstore.MeshStore({"data": mesh_tree}, "identity_seen", "test_unseen_motions", device=DEV)
    loader = store.eval_loader(4, seed=6)
    batches = list(loader)
    assert len(store) == 9 and len(loader) == 3 and [b["index"] for b in batches] == [[0, 1, 2, 3], [4, 5, 6, 7], [8]]
    assert [b["verts_src"].counts for b in batches] == [(4, 4, 4, 18), (18, 18, 121, 121), (121,)]
    for step, b in enumerate(batches):
        host = np.ascontiguousarray(store.pair_frames[b["index"]].T)
        ids = torch.from_numpy(host).to(DEV)
        want = dict(store.assemble(ids, 6, 0, step), **store.whole_meshes(ids, host))
        assert sorted(want) == sorted(k for k in b if k != "index")
        for k, v in want.items():
            g = b[k]
            if isinstance(v, RaggedPoints):
                assert g._counts == v._counts and torch.equal(g.offsets, v.offsets)
                g, v = g.packed, v.packed
            assert g.shape == v.shape and torch.equal(g.view(torch.uint8), v.view(torch.uint8)), (step, k)


def test_a_captured_call_replays_for_another_batch(mesh_tree):
    """No host counts: the capacities are given, nothing is read back, and the graph holds kernel nodes only -- the replay after
    ``frame_ids`` was overwritten on the device gives the new batch's bits (a smaller batch: padding behind it)."""
    store = meshstore.MeshStore({"data": mesh_tree}, "identity_seen", "test_unseen_motions", device=DEV)
    first, second = np.ascontiguousarray(store.pair_frames[[8, 7, 3]].T), np.ascontiguousarray(store.pair_frames[[0, 4, 6]].T)
    ids = torch.from_numpy(first).to(DEV)
    store.whole_meshes(ids, capacity=300, face_capacity=500)                             # (warm-up outside the capture)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = store.whole_meshes(ids, capacity=300, face_capacity=500)
    assert all(s._counts is None for s in out.values() if isinstance(s, RaggedPoints))
    arrays = {"vert_arena": store.vert_arena.cpu().numpy(), "face_arena": store.face_arena.cpu().numpy(),
              "frame_table": store.frame_table_host, "topo_table": store.topo_table_host}
    for host in (first, second):
        ids.copy_(torch.from_numpy(host).to(DEV))
        graph.replay()
        torch.cuda.synchronize()
        want = wr.whole(arrays, host, 300, 500, float(mesh_tree["partial_range"]))
        got = {"vert_offsets": out["verts_cano"].offsets, "face_offsets": out["faces"].offsets,
               "verts": torch.stack([out[f"verts_{k}"].packed for k in ("cano", "src", "tgt")]),
               "handle": out["cano_handle_vert_idx"].view(torch.uint8).reshape(-1), "inputs": out["verts_flow_inputs"].packed,
               "faces": out["faces"].packed}
        _assert_bit_equal(got, want, host.tolist())
    assert want["vert_offsets"].tolist() == [0, 4, 22, 143]
