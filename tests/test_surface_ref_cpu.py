"""tests/surface_ref.py against hand-computed answers, and what of the point-to-mesh distance can be held without a GPU: the
header and the exported entries, the bad-argument table, the workspace query, ``transfer_vertex_labels`` and the refusals of
``closest_on_mesh`` by name."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import surface_ref
from nsdp_amd import _lib
from nsdp_amd import build as nsdp_build
from nsdp_amd import surface_distance
from nsdp_amd.ragged import RaggedPoints

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "nsdp_surface.h")
ENTRY_POINTS = ["nsdp_mesh_closest", "nsdp_mesh_closest_workspace_bytes"]

A, B, C, REGIONS = surface_ref.TRI_A, surface_ref.TRI_B, surface_ref.TRI_C, surface_ref.REGIONS


@pytest.mark.parametrize("flip", [False, True])
def test_every_region_of_one_triangle(flip):
    b, c = (C, B) if flip else (B, C)
    for q, d2, bary in REGIONS:
        got, gb = surface_ref.closest(np.array(q), np.array(A), np.array(b), np.array(c))
        want = (bary[0], bary[2], bary[1]) if flip else bary
        assert abs(float(got) - d2) <= 1e-14, (q, got)
        assert np.abs(gb - np.array(want)).max() <= 1e-14, (q, gb)


def test_segment_and_point_shaped_faces():
    q = np.array([[1.0, 1.0, 0.0], [3.0, 0.0, 4.0], [-1.0, 0.0, 0.0]])
    a, b = np.array([0.0, 0.0, 0.0]), np.array([2.0, 0.0, 0.0])
    for tri in ((a, a, b), (a, b, b), (a, b, a), (a, (a + b) / 2, b), (b, a, (a + b) / 2)):      # two equal corners; collinear corners
        d, bary = surface_ref.closest(q, *tri)
        assert np.abs(d - np.array([1.0, 17.0, 1.0])).max() <= 1e-14
        assert np.abs(bary.sum(-1) - 1.0).max() <= 1e-15 and bary.min() >= 0.0
    d, bary = surface_ref.closest(q, b, b, b)                                                     # a point
    assert np.abs(d - np.array([2.0, 17.0, 9.0])).max() <= 1e-14 and not np.isnan(bary).any()


def test_brute_force_over_a_mesh():
    verts, faces = surface_ref.icosphere(1)
    assert verts.shape == (42, 3) and faces.shape == (80, 3) and verts.dtype == np.float32
    assert surface_ref.icosphere(3)[1].shape == (1280, 3)
    q = surface_ref.sphere_queries(40, 3)
    d, face, every = surface_ref.brute(q, verts, faces)
    assert every.shape == (40, 80) and np.array_equal(d, every.min(axis=1))
    one, bary = surface_ref.to_face(q, verts, faces, face)
    assert np.array_equal(one, d)
    point = (bary[:, :, None] * verts.astype(np.float64)[faces[face]]).sum(1)
    assert np.abs(((point - q) ** 2).sum(-1) - d).max() <= 1e-14
    # far outside a convex mesh the closest point is the support point's neighbourhood: the distance is about |q| - 1
    far = (q / np.linalg.norm(q, axis=1, keepdims=True) * 100).astype(np.float32)
    assert np.abs(np.sqrt(surface_ref.brute(far, verts, faces)[0]) - 99.0).max() < 0.1
    assert surface_ref.brute(q, verts, faces[:0])[1].tolist() == [-1] * 40
    assert surface_ref.corner_r2(q, verts, faces, face).min() >= d.min()


# ------------------------------------------------------------------------------------------------------------- the boundary
@pytest.fixture(scope="module")
def so():
    if not os.path.exists(_lib.SO_PATH):
        nsdp_build.build()
    lib = ctypes.CDLL(_lib.SO_PATH)
    lib.nsdp_last_error.restype = ctypes.c_char_p
    lib.nsdp_mesh_closest_workspace_bytes.restype = ctypes.c_size_t
    return lib


def test_header_declares_and_library_exports_the_entries(so):
    with open(HEADER) as f:
        raw = f.read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    declared = sorted(set(re.findall(r"\b(nsdp_[a-z0-9_]+)\s*\(", text)))
    assert declared == ENTRY_POINTS
    for name in ENTRY_POINTS:
        assert hasattr(so, name), name
    assert so.nsdp_abi_version() >= 21
    assert not set(ENTRY_POINTS) & set(_lib.declared_symbols())          # (nsdp_hip.h keeps its own table of entries)
    assert os.path.basename(HEADER) in open(nsdp_build.__file__).read()
    assert nsdp_build.PER_FILE["surface_distance.hip"] == nsdp_build.EXACT
    assert f"<= {int(surface_ref.E)} * 2^-24 * R2" in raw                 # (the envelope the tests hold the kernel to is the header's)


def test_workspace_query_answers_what_the_header_says(so):
    size = so.nsdp_mesh_closest_workspace_bytes
    for B, qcap, fcap in ((1, 1, 1), (3, 257, 129), (2, 10, 12), (4, 400000, 800000), (1, 1 << 20, 1 << 20), (65535, 65535, 65535)):
        assert size(B, qcap, fcap) == 8 * qcap + 24 * (fcap // 64 + B + 1), (B, qcap, fcap)
    for B, qcap, fcap in ((0, 1, 1), (-1, 1, 1), (65536, 1, 1), (1, 0, 1), (1, 1, 0), (1, (1 << 20) + 1, 1), (1, 1, (1 << 20) + 1),
                          (2, (2 << 20) + 1, 1)):
        assert size(B, qcap, fcap) == 0, (B, qcap, fcap)


def test_bad_arguments_return_status_before_any_launch(so):
    one = ctypes.c_void_p(16)      # (a non-null pointer the library must not touch)

    def call(B=2, qcap=10, vcap=8, fcap=12, flags=0, ptr=one, ws=one, out=one):
        return so.nsdp_mesh_closest(ptr, ptr, ptr, ptr, ptr, ptr, B, qcap, vcap, fcap, flags, ws, out, out, None, None)

    for kw, word in (({"B": 0}, b"B=0"), ({"B": 65536}, b"B=65536"), ({"qcap": 0}, b"qcap=0"), ({"qcap": -4}, b"qcap=-4"),
                     ({"B": 1, "qcap": (1 << 20) + 1}, b"qcap=1048577"), ({"vcap": 0}, b"vcap=0"),
                     ({"B": 1, "vcap": (1 << 20) + 1}, b"vcap=1048577"), ({"fcap": 0}, b"fcap=0"),
                     ({"B": 1, "fcap": (1 << 20) + 1}, b"fcap=1048577"), ({"flags": 4}, b"flags=4"), ({"flags": -1}, b"flags=-1"),
                     ({"ptr": None}, b"null"), ({"ws": None}, b"null"), ({"out": None}, b"null"),
                     ({"ws": ctypes.c_void_p(20)}, b"aligned")):
        assert call(**kw) == -1, kw
        assert word in so.nsdp_last_error() and b"mesh_closest" in so.nsdp_last_error(), (kw, so.nsdp_last_error())
    assert call(fcap=0, ptr=None, ws=None, out=None) == -1 and b"fcap=0" in so.nsdp_last_error()      # sizes before pointers
    assert call(B=1, qcap=1 << 20, vcap=1 << 20, fcap=1 << 20, ptr=None) == -1 and b"null" in so.nsdp_last_error()


# ------------------------------------------------------------------------------------------------------------- label transfer
def test_transfer_vertex_labels_on_hand_made_face_and_bary():
    faces = torch.tensor([[0, 1, 2], [2, 1, 3], [3, 4, 0]])
    labels = torch.tensor([0, 1, 2, 1, 0], dtype=torch.uint8)
    face = torch.tensor([0, 0, 1, 1, 2, 2, -1, 1], dtype=torch.int32)
    bary = torch.tensor([[0.6, 0.3, 0.1], [0.2, 0.3, 0.5], [0.5, 0.5, 0.0], [0.25, 0.25, 0.5], [0.0, 1.0, 0.0], [1 / 3, 1 / 3, 1 / 3],
                         [0.0, 0.0, 0.0], [0.0, 0.5, 0.5]])
    #       corner:  0 -> v0      2 -> v2      tie: first -> v2   2 -> v3     1 -> v4      tie: first -> v3   no face   tie 1, 2: -> v1
    want = [0, 2, 2, 1, 0, 1, 0, 1]
    got = surface_distance.transfer_vertex_labels(labels, faces, face, bary)
    assert got.dtype == torch.uint8 and got.tolist() == want
    batch = surface_distance.transfer_vertex_labels(torch.stack((labels, 2 - labels)), torch.stack((faces, faces)),
                                                    torch.stack((face, face)), torch.stack((bary, bary)))
    assert batch.shape == (2, 8) and batch[0].tolist() == want
    assert batch[1].tolist() == [2 - w if f >= 0 else 0 for w, f in zip(want, face.tolist())]
    with pytest.raises(_lib.NsdpHipError, match="transfer_vertex_labels: "):
        surface_distance.transfer_vertex_labels(labels, faces, face, bary[:, :2])


# ------------------------------------------------------------------------------------------------------------- the refusals
def test_refusals_are_named():
    q, v = torch.zeros(2, 5, 3), torch.zeros(2, 4, 3)
    f = torch.zeros(2, 6, 3, dtype=torch.int32)
    refusal = surface_distance.refusal
    assert "CPU tensors: query is on the CPU" in refusal(q, v, f)
    with pytest.raises(_lib.NsdpHipError, match="closest_on_mesh: CPU tensors: query is on the CPU"):
        surface_distance.closest_on_mesh(q, v, f)
    with pytest.raises(_lib.NsdpHipError, match="closest_on_mesh: CPU tensors"):
        surface_distance.point_to_surface_loss(q, v, f)
    assert "CPU tensors" in refusal(q, v, f.long())                                   # (int64 faces are taken)
    assert "dtype: query must be torch.float32, got torch.float64" in refusal(q.double(), v, f)
    assert "dtype: verts must be torch.float32, got torch.bfloat16" in refusal(q, v.bfloat16(), f)
    assert "dtype: faces must be torch.int32 or torch.int64" in refusal(q, v, f.float())
    assert "shape: query must be [B, rows, 3], got (2, 5, 2)" in refusal(q[:, :, :2], v, f)
    assert "shape: faces must be [B, rows, 3], got (2, 6)" in refusal(q, v, f[:, :, 0])
    assert "mismatched batches: query holds 2 shapes, verts holds 3 shapes, faces holds 2 shapes" in refusal(q, torch.zeros(3, 4, 3), f)
    rq, rv = RaggedPoints.from_list([q[0], q[1, :2]]), RaggedPoints.from_list([v[0], v[1]])
    rf = RaggedPoints.from_rows([f[0], f[1, :1]])
    assert "mismatched layouts: query is packed, verts is rectangular, faces is rectangular" in refusal(rq, v, f)
    assert "mismatched layouts" in refusal(q, v, rf)
    assert "CPU tensors" in refusal(rq, rv, rf)
    assert "mismatched batches" in refusal(rq, RaggedPoints.from_list([v[0]]), rf)
    assert "limits: B = 0 shapes" in refusal(q[:0], v[:0], f[:0])
    assert "limits: query holds 0 rows per shape" in refusal(q[:, :0], v, f)
    assert "limits: faces holds 0 rows per shape" in refusal(q, v, f[:, :0])
    big = torch.empty((1, surface_distance.MAX_ROWS + 1, 3), device="meta")
    assert "limits: query holds 1048577 rows in a shape" in refusal(big, v[:1], f[:1])
    assert "limits: verts holds 1048577 rows in a shape" in refusal(q[:1], big, f[:1])
    assert "limits: B = 65536 shapes" in refusal(torch.empty((65536, 1, 3), device="meta"), torch.empty((65536, 1, 3), device="meta"),
                                                 torch.empty((65536, 1, 3), dtype=torch.int32, device="meta"))
    assert "must be a torch.Tensor" in refusal(q.numpy(), v, f)


def test_cull_knob(monkeypatch):
    monkeypatch.delenv("NSDP_SURFACE_CULL", raising=False)
    assert surface_distance._cull_default() is None                      # (by size)
    assert surface_distance._large(4, 400000, 800000) and not surface_distance._large(8, 34000, 67588)
    monkeypatch.setenv("NSDP_SURFACE_CULL", "0")
    assert surface_distance._cull_default() is False
    monkeypatch.setenv("NSDP_SURFACE_CULL", "1")
    assert surface_distance._cull_default() is True
    monkeypatch.setenv("NSDP_SURFACE_CULL", "yes")
    with pytest.raises(_lib.NsdpHipError, match="NSDP_SURFACE_CULL"):
        surface_distance._cull_default()
    assert "NSDP_SURFACE_CULL" in open(os.path.join(os.path.dirname(HEADER), "..", "docs", "KNOBS.md")).read()
