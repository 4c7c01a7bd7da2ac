"""CPU: the boundary of the cell-grid search -- include/nsdp_search.h declares the four entries and the built library exports
them at ABI version 13, bad arguments come back as a status with a message, the size query answers as the header says, the
wrappers refuse CPU tensors and the NSDP_KNN_GRID knob parses and restores."""
import ctypes
import os
import re

import pytest
import torch

from nsdp_amd import _lib, build as nsdp_build, pointnet2_utils as pu

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "nsdp_search.h")
ENTRY_POINTS = ["nsdp_knn_grid", "nsdp_knn_grid_ragged_source", "nsdp_knn_grid_stats", "nsdp_knn_grid_workspace_bytes"]


@pytest.fixture(scope="module")
def so():
    if not os.path.exists(_lib.SO_PATH):
        nsdp_build.build()
    lib = ctypes.CDLL(_lib.SO_PATH)
    lib.nsdp_last_error.restype = ctypes.c_char_p
    lib.nsdp_knn_grid_workspace_bytes.restype = ctypes.c_size_t
    return lib


def test_header_declares_and_library_exports_the_entries(so):
    with open(HEADER) as f:
        text = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(nsdp_[a-z0-9_]+)\s*\(", text)))
    assert declared == sorted(ENTRY_POINTS)
    for name in ENTRY_POINTS:
        assert hasattr(so, name), name
    assert so.nsdp_abi_version() >= 13
    assert not set(ENTRY_POINTS) & set(_lib.declared_symbols())          # (nsdp_hip.h keeps its own table of entries)
    assert os.path.basename(HEADER) in open(nsdp_build.__file__).read()
    assert nsdp_build.PER_FILE["knn_grid.hip"] == nsdp_build.EXACT == nsdp_build.PER_FILE["knn.hip"]


def test_bad_arguments_return_status(so):
    one = ctypes.c_void_p(16)      # (a non-null pointer the library must not touch before it has checked the sizes)
    rect, rag = so.nsdp_knn_grid, so.nsdp_knn_grid_ragged_source
    # (query, source, B, n, m, k, workspace, idx_out, dist_out, stream)
    assert rect(None, one, 1, 100, 100, 4, one, one, None, None) == -1 and b"null" in so.nsdp_last_error()
    assert rect(one, None, 1, 100, 100, 4, one, one, None, None) == -1 and b"null" in so.nsdp_last_error()
    assert rect(one, one, 1, 100, 100, 4, None, one, None, None) == -1 and b"null" in so.nsdp_last_error()
    assert rect(one, one, 1, 100, 100, 4, one, None, None, None) == -1 and b"null" in so.nsdp_last_error()
    assert rect(one, one, 1, 100, 3, 4, one, one, None, None) == -1 and b"exceeds" in so.nsdp_last_error()
    assert rect(one, one, 1, 100, 100, 33, one, one, None, None) == -1 and b"k=33" in so.nsdp_last_error()
    assert rect(one, one, 1, 100, 1048577, 4, one, one, None, None) == -1 and b"limit" in so.nsdp_last_error()
    assert rect(one, one, 65536, 100, 100, 4, one, one, None, None) == -1 and b"batch" in so.nsdp_last_error()
    assert rect(one, one, 60000, 100, 1000000, 4, one, one, None, None) == -1 and b"too large" in so.nsdp_last_error()
    assert rect(None, None, 0, 100, 100, 4, None, None, None, None) == 0
    assert rect(None, None, 1, 0, 100, 4, None, None, None, None) == 0
    assert rect(None, None, 1, 100, 100, 0, None, None, None, None) == 0
    # (query, query_offsets, source, offsets, B, n, qcap, cap, n_max, k, workspace, idx_out, dist_out, stream)
    assert rag(None, one, one, one, 2, 0, 500, 500, 300, 4, one, one, None, None) == -1 and b"null" in so.nsdp_last_error()
    assert rag(one, one, one, None, 2, 0, 500, 500, 300, 4, one, one, None, None) == -1 and b"null" in so.nsdp_last_error()
    assert rag(one, one, one, one, 2, 0, 500, 500, 300, 4, None, one, None, None) == -1 and b"null" in so.nsdp_last_error()
    assert rag(one, one, one, one, 2, 0, 500, 500, 300, 4, one, None, None, None) == -1 and b"null" in so.nsdp_last_error()
    assert rag(one, one, one, one, 2, 0, 500, 0, 300, 4, one, one, None, None) == -1 and b"cap" in so.nsdp_last_error()
    assert rag(one, one, one, one, 2, 0, 500, 500, 0, 4, one, one, None, None) == -1 and b"n_max" in so.nsdp_last_error()
    assert rag(one, one, one, one, 2, 0, 500, 500, 3, 4, one, one, None, None) == -1 and b"exceeds" in so.nsdp_last_error()
    assert rag(one, one, one, one, 2, 0, 500, 500, 300, 33, one, one, None, None) == -1 and b"k=33" in so.nsdp_last_error()
    assert rag(one, one, one, one, 2, 0, 500, 2000000, 1048577, 4, one, one, None, None) == -1 and b"limit" in so.nsdp_last_error()
    assert rag(one, one, one, one, 65536, 0, 500, 500, 300, 4, one, one, None, None) == -1 and b"batch" in so.nsdp_last_error()
    assert rag(None, None, None, None, 0, 0, 500, 500, 300, 4, None, None, None, None) == 0
    assert rag(None, None, None, None, 2, 0, 0, 500, 300, 4, None, None, None, None) == 0          # (packed queries without rows)
    assert rag(None, None, None, None, 2, 0, 0, 500, 300, 4, None, None, None, None) == 0
    out = (ctypes.c_int64 * 4)(7, 7, 7, 7)
    assert so.nsdp_knn_grid_stats(None, None, out) == -1 and b"null" in so.nsdp_last_error()
    assert so.nsdp_knn_grid_stats(one, None, None) == -1 and b"null" in so.nsdp_last_error()
    assert list(out) == [7, 7, 7, 7]


def test_workspace_bytes_is_monotone_in_each_argument(so):
    ws = so.nsdp_knn_grid_workspace_bytes
    base = ws(2, 20000, 20000, 10000)
    # (the sorted copy of the source, 16 bytes a row, and at least one cell per shape)
    assert base >= 20000 * 16 + 2 * 12 and base % 16 == 0
    for vary in (lambda v: ws(v, 200000, 200000, 10000), lambda v: ws(2, v, 200000, 10000), lambda v: ws(2, 200000, v, 10000),
                 lambda v: ws(2, 200000, 200000, v)):
        sizes = [vary(v) for v in (1, 2, 3, 16, 17, 1000, 5000, 8193, 40000, 65535)]
        assert all(s > 0 for s in sizes) and sizes == sorted(sizes) and sizes[0] < sizes[-1], sizes
    big = [ws(1, 1 << 20, 1 << 20, m) for m in (65535, 65536, 65537, 200000, 1 << 20)]
    assert big == sorted(big) and big[1] == big[-1]                       # (the grid stops growing at 128 cells per axis)
    assert ws(1, 1, 1, 1) > 0                                            # m = k = 1 is served
    # what the entries refuse, and empty work, need no bytes
    assert ws(0, 100, 100, 100) == 0 and ws(-1, 100, 100, 100) == 0 and ws(65536, 100, 100, 100) == 0
    assert ws(1, 0, 100, 100) == 0 and ws(1, 100, 0, 100) == 0 and ws(1, 100, 100, 0) == 0
    assert ws(1, 100, 2000000, (1 << 20) + 1) == 0 and ws(1, 100, 1 << 20, 1 << 20) > 0


def test_wrappers_refuse_cpu_tensors():
    xyz = torch.rand(1, 100, 3)
    off = torch.tensor([0, 100], dtype=torch.int32)
    with pytest.raises(RuntimeError, match="GPU tensor"):
        pu.knn_grid(xyz, xyz, 4)
    with pytest.raises(RuntimeError, match="GPU tensor"):
        pu.knn_grid_ragged_source(xyz, xyz[0], off, 4, 100)
    with pytest.raises(RuntimeError, match="GPU tensor"):
        pu.knn_grid_ragged_source(xyz[0], xyz[0], off, 4, 100, query_offsets=off)
    with pytest.raises(RuntimeError, match="GPU tensor"):
        pu.knn_grid_stats(torch.zeros(64, dtype=torch.uint8))
    with pu.knn_grid_mode("force"):      # the dispatch hands a CPU tensor to the scan wrapper, which refuses it as before
        with pytest.raises(RuntimeError, match="GPU tensor"):
            pu.knn(xyz, xyz, 4)


def test_knob_parsing_and_context_manager():
    assert pu._grid_mode(None) == "1" and pu._grid_mode("") == "1" and pu._grid_mode("  ") == "1"
    for off in ("0", "off", "OFF", "false", "no", " 0 "):
        assert pu._grid_mode(off) == "0", off
    for on in ("1", "on", "true", "yes", "2"):
        assert pu._grid_mode(on) == "1", on
    for force in ("force", "FORCE", " Force "):
        assert pu._grid_mode(force) == "force", force
    assert pu.KNN_GRID in pu.KNN_GRID_MODES
    before = pu.KNN_GRID
    with pu.knn_grid_mode("0"):
        assert pu.KNN_GRID == "0"
        with pu.knn_grid_mode("force"):
            assert pu.KNN_GRID == "force"
            with pu.knn_grid_mode(True):
                assert pu.KNN_GRID == "1"
            assert pu.KNN_GRID == "force"
        assert pu.KNN_GRID == "0"
    assert pu.KNN_GRID == before
    other = "0" if before != "0" else "force"
    with pytest.raises(KeyError):
        with pu.knn_grid_mode(other):
            assert pu.KNN_GRID == other
            raise KeyError("inside")
    assert pu.KNN_GRID == before
    with pytest.raises(ValueError):
        with pu.knn_grid_mode("sometimes"):
            pass
    assert pu.KNN_GRID == before


def test_thresholds_leave_the_training_shapes_to_the_scan():
    assert pu.KNN_GRID_MIN_POINTS >= 8193
    probe = torch.empty(0)

    class _Gpu:      # (the dispatch asks a tensor only whether it lives on a GPU)
        is_cuda = True

    with pu.knn_grid_mode("1"):
        assert not pu._use_grid(_Gpu, 32, 2048, 2048, 16) and not pu._use_grid(_Gpu, 1, 8192, 8192, 16)
        assert pu._use_grid(_Gpu, 1, 100000, 100000, 16) and pu._use_grid(_Gpu, 1, 500, 100000, 16)      # (measured wins)
        assert not pu._use_grid(_Gpu, 1, 100, 100000, 16)                 # few queries: below KNN_GRID_MIN_TESTS
        assert not pu._use_grid(_Gpu, 1, 100000, pu.KNN_GRID_MIN_POINTS - 1, 16)
        assert not pu._use_grid(probe, 1, 100000, 100000, 16)             # a CPU tensor goes on to the scan wrapper's refusal
        assert not pu._use_grid(_Gpu, 1, 100000, 100000, 33) and not pu._use_grid(_Gpu, 1, 100000, (1 << 20) + 1, 16)
    with pu.knn_grid_mode("0"):
        assert not pu._use_grid(_Gpu, 1, 100000, 100000, 16)
    with pu.knn_grid_mode("force"):
        assert pu._use_grid(_Gpu, 1, 5, 5, 1) and pu._use_grid(_Gpu, 32, 2048, 2048, 16)
        assert not pu._use_grid(_Gpu, 1, 100, 100, 33) and not pu._use_grid(_Gpu, 1, 100, 3, 4)
