"""CPU: the boundary of the batch evaluation metrics -- include/nsdp_eval.h declares the three entries and the built library
exports them at ABI version 11, bad arguments come back as a status with a message, the Python functions refuse what they
cannot take with the reason, and the sampling helpers (torch only) run on CPU tensors."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from nsdp_amd import _lib, build as nsdp_build, eval_metric
from nsdp_amd.ragged import RaggedPoints

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "nsdp_eval.h")
ENTRY_POINTS = ["nsdp_nn_dist2", "nsdp_nn_dist2_ragged", "nsdp_segment_mean_f32"]


@pytest.fixture(scope="module")
def so():
    if not os.path.exists(_lib.SO_PATH):
        nsdp_build.build()
    lib = ctypes.CDLL(_lib.SO_PATH)
    lib.nsdp_last_error.restype = ctypes.c_char_p
    return lib


def test_header_declares_and_library_exports_the_entries(so):
    with open(HEADER) as f:
        text = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(nsdp_[a-z0-9_]+)\s*\(", text)))
    assert declared == sorted(ENTRY_POINTS)
    for name in ENTRY_POINTS:
        assert hasattr(so, name), name
    assert so.nsdp_abi_version() >= 11
    assert not set(ENTRY_POINTS) & set(_lib.declared_symbols())          # (nsdp_hip.h keeps its own table of entries)
    assert os.path.basename(HEADER) in open(nsdp_build.__file__).read() and "eval_metric.hip" in nsdp_build.PER_FILE
    assert nsdp_build.PER_FILE["eval_metric.hip"] == nsdp_build.EXACT


def test_bad_arguments_return_status(so):
    one = ctypes.c_void_p(16)      # (a non-null pointer the library must not touch before it has checked the sizes)
    nn, rag, mean = so.nsdp_nn_dist2, so.nsdp_nn_dist2_ragged, so.nsdp_segment_mean_f32
    # (query, source, B, n, m, dist2_out, idx_out, stream)
    assert nn(None, None, 2, 4, 4, None, None, None) == -1 and b"null" in so.nsdp_last_error()
    assert nn(one, one, 2, 4, 0, one, None, None) == -1 and b"m=0" in so.nsdp_last_error()
    assert nn(one, one, 70000, 4, 4, one, None, None) == -1 and b"batch" in so.nsdp_last_error()
    assert nn(None, None, 0, 4, 4, None, None, None) == 0 and nn(None, None, 2, 0, 0, None, None, None) == 0
    # (query, query_offsets, source, source_offsets, B, qcap, scap, dist2_out, idx_out, stream)
    assert rag(one, None, one, one, 2, 8, 8, one, None, None) == -1 and b"null" in so.nsdp_last_error()
    assert rag(one, one, one, one, 2, 8, 0, one, None, None) == -1 and b"scap" in so.nsdp_last_error()
    assert rag(one, one, one, one, 70000, 8, 8, one, None, None) == -1 and b"batch" in so.nsdp_last_error()
    assert rag(None, None, None, None, 2, 0, 8, None, None, None) == 0 and rag(None, None, None, None, 0, 8, 8, None, None, None) == 0
    # (values, offsets, B, cap, transform, out, stream)
    assert mean(one, one, 2, 8, 0, None, None) == -1 and b"null" in so.nsdp_last_error()
    assert mean(one, one, 2, 8, 2, one, None) == -1 and b"transform" in so.nsdp_last_error()
    assert mean(one, one, 2, -1, 0, one, None) == -1 and b"capacity" in so.nsdp_last_error()
    assert mean(None, one, 2, 8, 0, one, None) == -1 and b"null" in so.nsdp_last_error()      # (values may be NULL only for cap = 0)
    assert mean(None, None, 0, 8, 0, None, None) == 0


def _mesh(seed, V, F):
    g = np.random.RandomState(seed)
    verts = torch.from_numpy(g.rand(V, 3).astype(np.float32))
    faces = torch.from_numpy(np.argsort(g.rand(F, V), axis=1)[:, :3].astype(np.int32))
    return verts, faces


def test_refusals_carry_their_reasons():
    v, f = _mesh(0, 20, 30)
    rect = {"verts_tgt_pred": v[None], "verts_tgt": v[None], "faces": f[None]}
    with pytest.raises(RuntimeError, match="GPU tensor"):                 # CPU tensors: there is no fallback
        eval_metric.compute_evaluation_metrics_batch(rect, pointcloud_size=10)
    with pytest.raises(RuntimeError, match="GPU tensor"):
        eval_metric.chamfer_distance_batch(v[None], v[None])
    with pytest.raises(RuntimeError, match="GPU tensor"):
        eval_metric.nn_distance2_batch(RaggedPoints.from_list([v]), RaggedPoints.from_list([v]))
    with pytest.raises(RuntimeError, match="float32"):
        eval_metric.chamfer_distance_batch(v[None].double(), v[None].double())
    with pytest.raises(RuntimeError, match=r"\[B, n, 3\]"):
        eval_metric.chamfer_distance_batch(v, v)
    with pytest.raises(TypeError, match="RaggedPoints"):
        eval_metric.nn_distance2_batch([v], [v])
    with pytest.raises(RuntimeError, match="mismatched layouts"):         # one packed, one rectangular
        eval_metric.sample_points(RaggedPoints.from_list([v]), f[None], torch.zeros(1, 4, dtype=torch.int64), torch.ones(1, 4, 3) / 3)
    with pytest.raises(RuntimeError, match="mismatched layouts"):         # two meshes of vertices, one of faces
        eval_metric.sample_surface_batch(torch.stack([v, v]), f[None], 4)
    with pytest.raises(RuntimeError, match="int32 / int64"):
        eval_metric.sample_surface_batch(v[None], f[None].float(), 4)
    with pytest.raises(RuntimeError, match=r"bary \[B, count, 3\]"):
        eval_metric.sample_points(v[None], f[None], torch.zeros(1, 4, dtype=torch.int64), torch.ones(1, 5, 3))


def test_sampling_helpers_on_cpu_tensors_in_both_layouts():
    (v0, f0), (v1, f1) = _mesh(1, 50, 80), _mesh(2, 9, 12)
    verts, faces = RaggedPoints.from_list([v0, v1], capacity=70), RaggedPoints.from_rows([f0, f1], capacity=100)
    g = torch.Generator().manual_seed(3)
    fi, bary = eval_metric.sample_surface_batch(verts, faces, 500, g)
    assert fi.shape == (2, 500) and fi.dtype == torch.int64 and bary.shape == (2, 500, 3)
    assert int(fi.min()) >= 0 and int(fi[0].max()) < 80 and int(fi[1].max()) < 12
    assert bool((bary >= 0).all()) and torch.allclose(bary.sum(-1), torch.ones(2, 500), atol=1e-6)
    fi2, bary2 = eval_metric.sample_surface_batch(verts, faces, 500, torch.Generator().manual_seed(3))
    assert torch.equal(fi, fi2) and torch.equal(bary, bary2)
    pts = eval_metric.sample_points(verts, faces, fi, bary)
    assert pts.shape == (2, 500, 3)
    for b, (v, f) in enumerate(((v0, f0), (v1, f1))):
        tri = v.double()[f.long()[fi[b]]]                                  # [count, 3 corners, 3]
        want = (bary[b].double()[:, :, None] * tri).sum(1)
        assert torch.allclose(pts[b].double(), want, atol=1e-6)
        # each mesh alone, rectangular, with the same draws: the same points, bit for bit
        alone = eval_metric.sample_points(v[None], f[None], fi[b:b + 1], bary[b:b + 1])
        assert torch.equal(alone[0], pts[b])
    # area weighting: a large and a small triangle, 3 : 1
    v = torch.tensor([[0, 0, 0], [3, 0, 0], [0, 1, 0], [0, 0, 1], [1, 0, 1], [0, 1, 1]], dtype=torch.float32)
    f = torch.tensor([[0, 1, 2], [3, 4, 5]], dtype=torch.int32)
    fi, _ = eval_metric.sample_surface_batch(v[None], f[None], 20000, torch.Generator().manual_seed(4))
    assert abs(float((fi == 0).float().mean()) - 0.75) <= 0.02
