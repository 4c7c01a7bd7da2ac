"""CPU: the boundary of the workgroup-cluster sampler -- include/nsdp_sampling.h declares the five entries and the built library
exports them at ABI version 12, bad arguments come back as a status with a message, the size queries answer as the header
says, the wrappers refuse CPU tensors and the FPS_CLUSTER knob parses and restores."""
import ctypes
import os
import re

import pytest
import torch

from nsdp_amd import _lib, build as nsdp_build, pointnet2_utils as pu

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "nsdp_sampling.h")
ENTRY_POINTS = ["nsdp_fps_cluster_groups", "nsdp_fps_cluster_status", "nsdp_fps_cluster_workspace_bytes",
                "nsdp_furthest_point_sampling_cluster", "nsdp_furthest_point_sampling_cluster_ragged"]


@pytest.fixture(scope="module")
def so():
    if not os.path.exists(_lib.SO_PATH):
        nsdp_build.build()
    lib = ctypes.CDLL(_lib.SO_PATH)
    lib.nsdp_last_error.restype = ctypes.c_char_p
    lib.nsdp_fps_cluster_workspace_bytes.restype = ctypes.c_size_t
    return lib


def test_header_declares_and_library_exports_the_entries(so):
    with open(HEADER) as f:
        text = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(nsdp_[a-z0-9_]+)\s*\(", text)))
    assert declared == sorted(ENTRY_POINTS)
    for name in ENTRY_POINTS:
        assert hasattr(so, name), name
    assert so.nsdp_abi_version() >= 12
    assert not set(ENTRY_POINTS) & set(_lib.declared_symbols())          # (nsdp_hip.h keeps its own table of entries)
    assert os.path.basename(HEADER) in open(nsdp_build.__file__).read()
    assert nsdp_build.PER_FILE["fps_cluster.hip"] == nsdp_build.EXACT == nsdp_build.PER_FILE["fps.hip"]


def test_bad_arguments_return_status(so):
    one = ctypes.c_void_p(16)      # (a non-null pointer the library must not touch before it has checked the sizes)
    rect, rag = so.nsdp_furthest_point_sampling_cluster, so.nsdp_furthest_point_sampling_cluster_ragged
    # (xyz, B, N, nsamples, groups, workspace, idx_out, stream)
    assert rect(None, 1, 9000, 4, 0, one, one, None) == -1 and b"null" in so.nsdp_last_error()
    assert rect(one, 1, 9000, 4, 0, None, one, None) == -1 and b"null" in so.nsdp_last_error()
    assert rect(one, 1, 9000, 4, 0, one, None, None) == -1 and b"null" in so.nsdp_last_error()
    assert rect(one, 1, 0, 4, 2, one, one, None) == -1 and b"positive" in so.nsdp_last_error()
    assert rect(one, 1, 9000, 4, 1, one, one, None) == -1 and b"too small" in so.nsdp_last_error()
    assert rect(one, 1, 8193, 4, 33, one, one, None) == -1 and b"groups" in so.nsdp_last_error()
    assert rect(one, 1, 8193, 4, -1, one, one, None) == -1 and b"groups" in so.nsdp_last_error()
    assert rect(one, 1, 8192, 4, 0, one, one, None) == -1 and b"default" in so.nsdp_last_error()
    assert rect(one, 1, 262145, 4, 0, one, one, None) == -1 and b"default" in so.nsdp_last_error()
    assert rect(one, 1, 262145, 4, 32, one, one, None) == -1 and b"too small" in so.nsdp_last_error()
    assert rect(None, 0, 9000, 4, 0, None, None, None) == 0 and rect(None, 1, 9000, 0, 0, None, None, None) == 0
    # (xyz_packed, offsets, B, cap, n_max, nsamples, groups, workspace, idx_out, stream)
    assert rag(one, None, 2, 20000, 9000, 4, 0, one, one, None) == -1 and b"null" in so.nsdp_last_error()
    assert rag(one, one, 2, 20000, 9000, 4, 0, None, one, None) == -1 and b"null" in so.nsdp_last_error()
    assert rag(one, one, 2, 20000, 9000, 0, 0, one, one, None) == -1 and b"nsamples" in so.nsdp_last_error()
    assert rag(one, one, 2, 0, 9000, 4, 0, one, one, None) == -1 and b"cap" in so.nsdp_last_error()
    assert rag(one, one, 2, 20000, 9000, 4, 1, one, one, None) == -1 and b"too small" in so.nsdp_last_error()
    assert rag(one, one, 2, 20000, 9000, 4, 33, one, one, None) == -1 and b"groups" in so.nsdp_last_error()
    assert rag(one, one, 2, 20000, 700, 4, 0, one, one, None) == -1 and b"default" in so.nsdp_last_error()
    assert rag(one, one, 70000, 20000, 9000, 4, 0, one, one, None) == -1 and b"batch" in so.nsdp_last_error()
    assert rag(None, None, 0, 20000, 9000, 4, 0, None, None, None) == 0
    assert so.nsdp_fps_cluster_status(None, None) == -1 and b"null" in so.nsdp_last_error()


def test_default_groups(so):
    assert so.nsdp_fps_cluster_groups(8192) == 0 and so.nsdp_fps_cluster_groups(1) == 0 and so.nsdp_fps_cluster_groups(0) == 0
    assert so.nsdp_fps_cluster_groups(8193) == 2 and so.nsdp_fps_cluster_groups(16384) == 2 and so.nsdp_fps_cluster_groups(16385) == 3
    assert so.nsdp_fps_cluster_groups(100000) == 13
    assert so.nsdp_fps_cluster_groups(262144) == 32 and so.nsdp_fps_cluster_groups(262145) == 0


def test_workspace_bytes_is_monotone_in_each_argument(so):
    ws = so.nsdp_fps_cluster_workspace_bytes
    base = ws(2, 20000, 50, 0)
    assert base >= 2 * 50 * 3 * 8 + 4 and base % 16 == 0                  # (a granule per workgroup and step, and the status word)
    assert [ws(b, 20000, 50, 0) for b in (1, 2, 3, 40)] == sorted(ws(b, 20000, 50, 0) for b in (1, 2, 3, 40))
    assert ws(1, 20000, 50, 0) < ws(2, 20000, 50, 0) < ws(40, 20000, 50, 0)
    sizes = [ws(2, n, 50, 0) for n in (8193, 16384, 16385, 100000, 262144)]
    assert sizes == sorted(sizes) and sizes[0] < sizes[-1] and sizes[0] == sizes[1] < sizes[2]
    assert ws(2, 20000, 1, 0) < ws(2, 20000, 50, 0) < ws(2, 20000, 500, 0)
    assert ws(2, 20000, 50, 3) < ws(2, 20000, 50, 7) < ws(2, 20000, 50, 32) and ws(2, 20000, 50, 3) == base
    assert ws(2, 5, 5, 8) == ws(2, 8192, 5, 8) == ws(2, 8 * 8192, 5, 8) > 0                   # (an explicit cluster: any N it can hold)
    # what the entries refuse needs no bytes
    assert ws(2, 8192, 50, 0) == 0 and ws(2, 262145, 50, 0) == 0 and ws(2, 20000, 50, 2) == 0 and ws(2, 20000, 50, 33) == 0
    assert ws(0, 20000, 50, 0) == 0 and ws(2, 20000, 0, 0) == 0


def test_wrappers_refuse_cpu_tensors():
    xyz = torch.rand(1, 9000, 3)
    with pytest.raises(RuntimeError, match="GPU tensor"):
        pu.furthest_point_sample_cluster(xyz, 8)
    with pytest.raises(RuntimeError, match="GPU tensor"):
        pu.furthest_point_sample_cluster(xyz[:, :100].contiguous(), 8, groups=2)
    with pytest.raises(RuntimeError, match="GPU tensor"):
        pu.furthest_point_sample(xyz, 8)
    with pytest.raises(RuntimeError, match="GPU tensor"):
        pu.furthest_point_sample_ragged(xyz[0], torch.tensor([0, 9000], dtype=torch.int32), 8, 9000)
    with pytest.raises(RuntimeError, match="GPU tensor"):
        pu.fps_cluster_status(torch.zeros(16, dtype=torch.uint8))


def test_knob_parsing_and_context_manager():
    assert pu._switch(None, True) is True and pu._switch(None, False) is False and pu._switch("", True) is True
    for off in ("0", "off", "OFF", "false", "no", " 0 "):
        assert pu._switch(off, True) is False, off
    for on in ("1", "on", "true", "yes", "2"):
        assert pu._switch(on, False) is True, on
    before = pu.FPS_CLUSTER
    with pu.fps_cluster(False):
        assert pu.FPS_CLUSTER is False
        with pu.fps_cluster(True):
            assert pu.FPS_CLUSTER is True
        assert pu.FPS_CLUSTER is False
    assert pu.FPS_CLUSTER is before
    with pytest.raises(KeyError):
        with pu.fps_cluster(not before):
            assert pu.FPS_CLUSTER is (not before)
            raise KeyError("inside")
    assert pu.FPS_CLUSTER is before
    assert pu.FPS_CLUSTER_MIN_POINTS >= 8193
