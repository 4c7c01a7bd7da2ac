"""GPU: farthest-point sampling by a cluster of workgroups (include/nsdp_sampling.h, csrc/fps_cluster.hip) gives the indices
of the oracle -- bit for bit, ties included, no case excluded -- for every cluster size, with workgroups that own no point,
with more clouds than compute units, on a reused workspace, replayed from a graph, beside a loaded stream, over packed sets,
through the dispatch of pointnet2_utils and through the model.  Every case asserts that no wait gave up."""
import ctypes

import numpy as np
import pytest
import torch

from helpers import build_product, model_cfg
from nsdp_amd import _lib, hip_decoder, pointnet2_utils as pu, precision, synth
from nsdp_amd.ragged import RaggedPoints
from oracle import pointnet2_ref as ref
from poison_arena import _Recorder

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)


def _cloud(seed, b, n, kind="uniform"):
    """tests/test_geometry_gpu.py's generator (a copy: that file is not imported for one helper)."""
    xyz = synth.uniform(seed, f"cloud{kind}", (b, n, 3), -0.5, 0.5)
    if kind == "origin":       # many points inside the mag <= 1e-3 ball (skipped by the kernel)
        xyz[:, ::7] *= 0.03
    elif kind == "dupes":      # exact duplicates -> exact distance ties
        xyz[:, 1::2] = xyz[:, 0::2][:, : xyz[:, 1::2].shape[1]]
    elif kind == "grid":       # lattice: massive ties everywhere
        g = np.stack(np.meshgrid(*[np.arange(16)] * 3, indexing="ij"), -1).reshape(-1, 3)
        xyz = np.tile(((g[:n] - 7.5) / 16.0).astype(np.float32)[None], (b, 1, 1))
    elif kind == "allorigin":
        xyz = np.zeros((b, n, 3), np.float32)
    return np.ascontiguousarray(xyz, dtype=np.float32)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _workspace_bytes(B, n_max, m, G):
    fn = _lib.lib().nsdp_fps_cluster_workspace_bytes
    fn.restype = ctypes.c_size_t
    need = int(fn(ctypes.c_int(B), ctypes.c_int(n_max), ctypes.c_int(m), ctypes.c_int(G)))
    assert need > 0, (B, n_max, m, G)
    return need


def _status(ws, stream=None):
    raw = ctypes.c_void_p(stream.cuda_stream) if stream is not None else _lib.stream_ptr()
    return int(_lib.lib().nsdp_fps_cluster_status(ctypes.c_void_p(ws.data_ptr()), raw))


def _cluster(xyz, m, G, ws=None):
    """The rectangular C entry with an explicit cluster size on the current stream -> (idx, workspace)."""
    B, N, _ = xyz.shape
    if ws is None:
        ws = torch.empty(_workspace_bytes(B, N, m, G), dtype=torch.uint8, device=DEV)
    out = torch.full((B, m), -1, dtype=torch.int32, device=DEV)
    _lib.check(_lib.lib().nsdp_furthest_point_sampling_cluster(ctypes.c_void_p(xyz.data_ptr()), ctypes.c_int(B), ctypes.c_int(N),
                                                               ctypes.c_int(m), ctypes.c_int(G), ctypes.c_void_p(ws.data_ptr()),
                                                               ctypes.c_void_p(out.data_ptr()), _lib.stream_ptr()),
               "nsdp_furthest_point_sampling_cluster")
    return out, ws


# workgroups without a point; a slice boundary inside a wave; one workgroup; 8192 + 1 in two and in nine; uneven last slices
@pytest.mark.parametrize("N,m,G", [(1, 1, 2), (3, 3, 3), (5, 5, 8), (64, 16, 2), (513, 77, 3), (1000, 100, 4),
                                   (8192, 64, 1), (8193, 64, 2), (8193, 64, 9), (20000, 50, 3), (20000, 50, 7)])
def test_explicit_groups_match_the_oracle(N, m, G):
    B = 3 if N <= 1000 else 1
    xyz = _cloud(N * 7 + m, B, N)
    got, ws = _cluster(_dev(xyz), m, G)
    assert _status(ws) == 0
    np.testing.assert_array_equal(got.cpu().numpy(), ref.furthest_point_sampling(xyz, m))


@pytest.mark.parametrize("kind", ["origin", "dupes", "grid", "allorigin"])
@pytest.mark.parametrize("N,m,G", [(2048, 500, 5), (4096, 200, 3)])
def test_edge_clouds_match_the_oracle(kind, N, m, G):
    """Exact ties whose two points sit in different workgroups, points skipped by the mag <= 1e-3 rule, and a cloud without one
    valid point (every key negative: the reference keeps index 0)."""
    xyz = _cloud(11, 2, N, kind)
    got, ws = _cluster(_dev(xyz), m, G)
    assert _status(ws) == 0
    np.testing.assert_array_equal(got.cpu().numpy(), ref.furthest_point_sampling(xyz, m))


def test_more_clouds_than_compute_units():
    """40 clouds x 8 workgroups = 320 workgroups: more than the device has compute units, so the host splits the batch into
    consecutive launches (each of them wholly resident)."""
    B, N, m, G = 40, 600, 24, 8
    assert B * G > torch.cuda.get_device_properties(DEV).multi_processor_count
    xyz = _cloud(5, B, N)
    got, ws = _cluster(_dev(xyz), m, G)
    assert _status(ws) == 0
    np.testing.assert_array_equal(got.cpu().numpy(), ref.furthest_point_sampling(xyz, m))


def test_workspace_reuse_needs_no_cleaning():
    big, small = _cloud(21, 1, 20000), _cloud(22, 3, 513)
    ws = torch.zeros(max(_workspace_bytes(1, 20000, 50, 3), _workspace_bytes(3, 513, 77, 3)), dtype=torch.uint8, device=DEV)
    a, _ = _cluster(_dev(big), 50, 3, ws)
    assert _status(ws) == 0
    b, _ = _cluster(_dev(small), 77, 3, ws)
    assert _status(ws) == 0
    c, _ = _cluster(_dev(big[:, ::-1].copy()), 50, 3, ws)
    assert _status(ws) == 0
    np.testing.assert_array_equal(a.cpu().numpy(), ref.furthest_point_sampling(big, 50))
    np.testing.assert_array_equal(b.cpu().numpy(), ref.furthest_point_sampling(small, 77))
    np.testing.assert_array_equal(c.cpu().numpy(), ref.furthest_point_sampling(big[:, ::-1].copy(), 50))


def test_replayed_call_follows_the_clouds_contents():
    """pu.furthest_point_sample at 9000 points (two workgroups by default) captured once and replayed: the memset that
    initialises the workspace is a node of the graph, so every replay starts from fresh granules."""
    from nsdp_amd.graph_step import GraphedStep
    assert pu.fps_cluster_groups(9000) == 2
    clouds = [_cloud(30 + r, 1, 9000) for r in range(4)]
    static = _dev(clouds[0]).clone()
    assert pu.fps_cluster_status() == 0      # (forgets the calls of earlier tests: the capture's is then the only one on record)
    with pu.fps_cluster(True):      # (read when the call runs: the captured graph keeps the kernel it was captured with)
        gs = GraphedStep(lambda: pu.furthest_point_sample(static, 32)).capture(warmup=0)
    (ws, _), = pu._cluster_workspaces.values()      # the captured call's workspace: every replay's status word lands in it
    try:
        for r in (1, 2, 3):
            static.copy_(_dev(clouds[r]))
            got = gs().clone()
            torch.cuda.synchronize()
            assert _status(ws) == 0
            np.testing.assert_array_equal(got.cpu().numpy(), ref.furthest_point_sampling(clouds[r], 32))
    finally:
        gs.close()


def test_under_uneven_load_on_either_stream():
    """The hand-off while another stream keeps the compute units busy for a few hundred milliseconds: the cluster on a side
    stream beside matrix products on the main stream, then the roles swapped."""
    N, m, G = 20000, 50, 7
    xyz = _cloud(N * 7 + m, 1, N)
    want = ref.furthest_point_sampling(xyz, m)
    dxyz = _dev(xyz)
    a = torch.rand(8192, 8192, device=DEV)
    side = torch.cuda.Stream(device=DEV)
    torch.cuda.synchronize()
    for fps_on_side in (True, False):
        side.wait_stream(torch.cuda.current_stream())
        load, work = (torch.cuda.current_stream(), side) if fps_on_side else (side, torch.cuda.current_stream())
        with torch.cuda.stream(load):
            for _ in range(24):
                a @ a
        with torch.cuda.stream(work):
            got, ws = _cluster(dxyz, m, G)
            assert _status(ws, work) == 0
        torch.cuda.synchronize()
        np.testing.assert_array_equal(got.cpu().numpy(), want)


@pytest.mark.parametrize("counts", [[9000, 1, 300, 0, 8193], [20000, 12000]])
def test_ragged_equals_the_one_workgroup_entry_and_the_oracle(counts):
    m, n_max = 40, max(counts)
    pts = [_cloud(40 + b, 1, n)[0] for b, n in enumerate(counts)]
    r = RaggedPoints.from_list([_dev(p) for p in pts])
    with pu.fps_cluster(False):
        old = pu.furthest_point_sample_ragged(r.packed, r.offsets, m, n_max)
    assert pu.fps_cluster_groups(n_max) > 0
    with pu.fps_cluster(True):
        got = pu.furthest_point_sample_ragged(r.packed, r.offsets, m, n_max)
    assert pu.fps_cluster_status() == 0
    assert torch.equal(got, old), (got != old).nonzero()[:8].tolist()
    offs = r.offsets.tolist()
    for b, n in enumerate(counts):
        if n:
            np.testing.assert_array_equal((got[b] - offs[b]).cpu().numpy(), ref.furthest_point_sampling(pts[b][None], m)[0])


def test_dispatch_takes_the_cluster_with_the_knob_on_and_the_old_kernel_with_it_off(monkeypatch):
    xyz = _cloud(10000 * 7 + 40, 3, 10000)
    dxyz = _dev(xyz)
    real, seen = _lib.lib(), {}
    for on in (True, False):
        called = set()
        monkeypatch.setattr(_lib, "_lib", _Recorder(real, called))
        with pu.fps_cluster(on):
            seen[on] = (pu.furthest_point_sample(dxyz, 40), called)
        monkeypatch.setattr(_lib, "_lib", real)
    assert "nsdp_furthest_point_sampling_cluster" in seen[True][1] and "nsdp_furthest_point_sampling" not in seen[True][1]
    assert "nsdp_furthest_point_sampling" in seen[False][1] and "nsdp_furthest_point_sampling_cluster" not in seen[False][1]
    assert pu.fps_cluster_status() == 0
    assert torch.equal(seen[True][0], seen[False][0])
    np.testing.assert_array_equal(seen[True][0].cpu().numpy(), ref.furthest_point_sampling(xyz, 40))
    # at and below 8192 points the dispatch is untouched
    called = set()
    monkeypatch.setattr(_lib, "_lib", _Recorder(real, called))
    pu.furthest_point_sample(dxyz[:, :8192].contiguous(), 8)
    monkeypatch.setattr(_lib, "_lib", real)
    assert "nsdp_furthest_point_sampling" in called and "nsdp_furthest_point_sampling_cluster" not in called


def _skip_refused_variants():
    """The library variants under which the ragged surface path is refused by design (tests/test_ragged_surface_gpu.py)."""
    knobs = []
    if not hip_decoder.ENABLED:
        knobs.append("NSDP_FUSED_DECODER=0")
    if precision.is_bf16():
        knobs.append("NSDP_STORAGE=bf16")
    if knobs:
        pytest.skip("ragged surface clouds are refused under " + ", ".join(knobs))


def _predict(model, dd, cfg, on, monkeypatch):
    """One step under the knob -> (predictions, the entries of the library it reached)."""
    from nsdp_amd.model.deformation_networks import test_on_batch_with_cano
    real, called = _lib.lib(), set()
    monkeypatch.setattr(_lib, "_lib", _Recorder(real, called))
    with pu.fps_cluster(on):
        _, got = test_on_batch_with_cano(model, dd, cfg)
    monkeypatch.setattr(_lib, "_lib", real)
    torch.cuda.synchronize()
    return got, called


def _packed(t):
    return t.packed if isinstance(t, RaggedPoints) else t


def _tiny_model():
    """The tiny configuration of the ragged-surface tests, with two 9000-sample surfaces and 64 vertices each."""
    cfg = model_cfg("forward", [256, 64, 16])
    model, _, _ = build_product(cfg, 131, DEV)
    model.eval()
    inputs = _dev(synth.make_batch(131, 2, 9000, 4)["surface_samples_inputs"])
    return cfg, model, inputs, _dev(synth.uniform(132, "verts", (2, 64, 3), -0.5, 0.5))


def test_model_predictions_at_batch_one_are_bit_identical_with_the_knob_on_and_off(monkeypatch):
    cfg, model, inputs, verts = _tiny_model()
    one = {"surface_samples_inputs": inputs[:1].contiguous(), "surface_samples_src": inputs[:1, :, 0:3].contiguous(),
           "verts_src": verts[:1].contiguous()}
    (on, reached), (off, without) = _predict(model, one, cfg, True, monkeypatch), _predict(model, one, cfg, False, monkeypatch)
    assert pu.fps_cluster_status() == 0
    assert "nsdp_furthest_point_sampling_cluster" in reached and "nsdp_furthest_point_sampling_cluster" not in without
    assert "nsdp_furthest_point_sampling" in without
    for key in ("verts_tgt_pred", "surface_samples_tgt_pred"):
        assert bool(torch.isfinite(on[key]).all()) and torch.equal(on[key], off[key]), key


def test_ragged_surface_step_is_bit_identical_with_the_knob_on_and_off(monkeypatch):
    _skip_refused_variants()
    cfg, model, inputs, verts = _tiny_model()
    surf = RaggedPoints.from_rows([inputs[0, :9000], inputs[1, :700]])
    rag = {"surface_samples_inputs": surf, "surface_samples_src": surf.columns(0, 3),
           "verts_src": RaggedPoints.from_list([verts[0], verts[1, :17].contiguous()])}
    (on, reached), (off, without) = _predict(model, rag, cfg, True, monkeypatch), _predict(model, rag, cfg, False, monkeypatch)
    assert pu.fps_cluster_status() == 0
    assert "nsdp_furthest_point_sampling_cluster_ragged" in reached and "nsdp_furthest_point_sampling_cluster_ragged" not in without
    assert "nsdp_furthest_point_sampling_ragged" in without
    for key in ("verts_tgt_pred", "surface_samples_tgt_pred"):
        assert bool(torch.isfinite(_packed(on[key])).all()) and torch.equal(_packed(on[key]), _packed(off[key])), key
