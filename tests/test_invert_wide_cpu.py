"""CPU: the boundary of the many-workgroup inverse-list build -- include/nsdp_scatter.h declares the two entries and the built
library exports them at ABI version 14, outside nsdp_hip.h's table; the size query answers 0 for what the entry refuses, bad
arguments come back as a status with a message, and the NSDP_INVERT_WIDE knob parses, restores and steers the dispatch."""
import ctypes
import os
import re

import pytest
import torch

from nsdp_amd import _lib, build as nsdp_build, hip_attention as ha

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "nsdp_scatter.h")
SOURCE = os.path.join(ROOT, "nsdp_amd", "csrc", "invert_wide.hip")
ENTRY_POINTS = ["nsdp_knn_invert_wide", "nsdp_knn_invert_wide_workspace_bytes"]


@pytest.fixture(scope="module")
def so():
    if not os.path.exists(_lib.SO_PATH):
        nsdp_build.build()
    lib = ctypes.CDLL(_lib.SO_PATH)
    lib.nsdp_last_error.restype = ctypes.c_char_p
    lib.nsdp_knn_invert_wide_workspace_bytes.restype = ctypes.c_size_t
    return lib


def test_header_declares_and_library_exports_the_entries(so):
    with open(HEADER) as f:
        text = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(nsdp_[a-z0-9_]+)\s*\(", text)))
    assert declared == sorted(ENTRY_POINTS)
    for name in ENTRY_POINTS:
        assert hasattr(so, name), name
    assert so.nsdp_abi_version() >= 14
    assert not set(ENTRY_POINTS) & set(_lib.declared_symbols())          # (nsdp_hip.h keeps its own table of entries)
    assert os.path.basename(HEADER) in open(nsdp_build.__file__).read()
    assert nsdp_build.PER_FILE["invert_wide.hip"] == nsdp_build.EXACT


def test_workspace_bytes_refuses_what_the_entry_refuses(so):
    ws = so.nsdp_knn_invert_wide_workspace_bytes
    assert ws(1, 16, 0) == 0 and ws(1, 16, -3) == 0 and ws(1, 16, (1 << 20) + 1) == 0
    assert ws(1, 0, 100) == 0 and ws(1, (1 << 25) + 1, 100) == 0
    assert ws(0, 16, 100) == 0 and ws(65536, 16, 100) == 0
    assert ws(1, 1, 1) > 0 and ws(65535, 1, 1) > 0
    # the counters of every source, a slot of every entry, and index products in 64 bits (these sizes pass 2^32 bytes)
    assert ws(2, 300 * 16, 700) >= 2 * 4 * (700 + 300 * 16)
    assert ws(1, 1 << 25, 1 << 20) >= 4 * ((1 << 25) + (1 << 20))
    assert ws(64, 1 << 25, 1 << 20) >= 64 * 4 * ((1 << 25) + (1 << 20)) > 1 << 32
    for vary in (lambda v: ws(v, 4000, 1000), lambda v: ws(2, v, 1000), lambda v: ws(2, 4000, v)):
        sizes = [vary(v) for v in (1, 2, 3, 17, 1000, 1024, 1025, 1026, 5000, 65535)]
        assert all(s > 0 for s in sizes) and sizes == sorted(sizes) and sizes[0] < sizes[-1], sizes


def test_bad_arguments_return_status(so):
    one = ctypes.c_void_p(16)      # (a non-null pointer the library must not touch before it has checked the sizes)
    fn = so.nsdp_knn_invert_wide
    # (idx, B, E, N, workspace, offsets, entries, stream)
    assert fn(None, 1, 16, 4, one, one, one, None) == -1 and b"null" in so.nsdp_last_error()
    assert fn(one, 1, 16, 4, None, one, one, None) == -1 and b"null" in so.nsdp_last_error()
    assert fn(one, 1, 16, 4, one, None, one, None) == -1 and b"null" in so.nsdp_last_error()
    assert fn(one, 1, 16, 4, one, one, None, None) == -1 and b"null" in so.nsdp_last_error()
    assert fn(one, 1, 16, 0, one, one, one, None) == -1 and b"N=0" in so.nsdp_last_error()
    assert fn(one, 1, 16, (1 << 20) + 1, one, one, one, None) == -1 and b"N=1048577" in so.nsdp_last_error()
    assert fn(one, 1, 0, 4, one, one, one, None) == -1 and b"E=0" in so.nsdp_last_error()
    assert fn(one, 1, (1 << 25) + 1, 4, one, one, one, None) == -1 and b"E=33554433" in so.nsdp_last_error()
    assert fn(one, 0, 16, 4, one, one, one, None) == -1 and b"batch" in so.nsdp_last_error()
    assert fn(one, 65536, 16, 4, one, one, one, None) == -1 and b"batch" in so.nsdp_last_error()
    assert fn(one, 1, 16, 4, ctypes.c_void_p(18), one, one, None) == -1 and b"aligned" in so.nsdp_last_error()


def test_knob_parsing_and_context_manager():
    assert ha._wide_mode(None) == "1" and ha._wide_mode("") == "1" and ha._wide_mode("  ") == "1"
    for off in ("0", "off", "OFF", "false", "no", " 0 "):
        assert ha._wide_mode(off) == "0", off
    for on in ("1", "on", "true", "yes", "2"):
        assert ha._wide_mode(on) == "1", on
    for force in ("force", "FORCE", " Force "):
        assert ha._wide_mode(force) == "force", force
    assert ha.INVERT_WIDE in ha.INVERT_WIDE_MODES
    before = ha.INVERT_WIDE
    with ha.invert_wide_mode("0"):
        assert ha.INVERT_WIDE == "0"
        with ha.invert_wide_mode("force"):
            assert ha.INVERT_WIDE == "force"
            with ha.invert_wide_mode(True):
                assert ha.INVERT_WIDE == "1"
            assert ha.INVERT_WIDE == "force"
        assert ha.INVERT_WIDE == "0"
    assert ha.INVERT_WIDE == before
    other = "0" if before != "0" else "force"
    with pytest.raises(KeyError):
        with ha.invert_wide_mode(other):
            assert ha.INVERT_WIDE == other
            raise KeyError("inside")
    assert ha.INVERT_WIDE == before
    with pytest.raises(ValueError):
        with ha.invert_wide_mode("sometimes"):
            pass
    assert ha.INVERT_WIDE == before


def test_dispatch_keeps_the_training_shapes_on_the_old_entry():
    f32 = torch.float32
    with ha.invert_wide_mode("1"):
        assert not ha._use_wide(32, 2048 * 16, 2048) and not ha._use_wide(1, 8192 * 16, 8192)
        assert ha._use_wide(1, 8193 * 16, 8193) and ha._use_wide(2, 2100 * 16, 32769) and ha._use_wide(1, 1 << 25, 1 << 20)
        assert not ha._use_wide(1, 16, (1 << 20) + 1) and not ha._use_wide(1, (1 << 25) + 1, 9000)
        assert ha._use_inverse(f32, False, 9000, 9000, 32) and ha._use_inverse(f32, False, 1 << 20, 1 << 20, 32)
        assert not ha._use_inverse(f32, False, 9000, (1 << 20) + 1, 32) and not ha._use_inverse(f32, True, 9000, 9000, 32)
        assert ha.max_list_sources() == 1 << 20
    with ha.invert_wide_mode("0"):
        assert not ha._use_wide(1, 8193 * 16, 8193) and not ha._use_inverse(f32, False, 9000, 9000, 32)
        assert ha._use_inverse(f32, False, 8192, 8192, 32) and ha.max_list_sources() == 8192
        assert not ha.lists_serve(1, 100, 8193) and ha.lists_serve(1, 100, 8192)
    with ha.invert_wide_mode("1"):
        # what the wide entry does not accept keeps the atomic kernels: E above 2^25 over more than 8192 sources, B above 65535
        assert ha._use_inverse(f32, False, 1 << 20, 1 << 20, 32, 32) and not ha._use_inverse(f32, False, 1 << 20, 1 << 20, 32, 33)
        assert not ha._use_inverse(f32, False, 3_000_000, 40000, 32, 16) and ha._use_inverse(f32, False, 2_000_000, 40000, 32, 16)
        assert ha._use_inverse(f32, False, 3_000_000, 8192, 32, 16)            # (the one-workgroup entry has no bound on E)
        assert ha.lists_serve(1, 1 << 25, 40000) and not ha.lists_serve(1, (1 << 25) + 1, 40000)
        assert ha.lists_serve(65535, 100, 9000) and not ha.lists_serve(65536, 100, 9000) and not ha.lists_serve(1, 100, 0)
        assert ha.lists_serve(1, (1 << 25) + 1, 8192) and ha.lists_serve(70000, 100, 8192)
    with ha.invert_wide_mode("force"):
        assert ha._use_wide(1, 5, 1) and ha._use_wide(32, 2048 * 16, 2048) and not ha._use_wide(1, 16, (1 << 20) + 1)
        assert ha._use_inverse(f32, False, 9000, 9000, 32)


def test_python_constants_mirror_the_kernel_file():
    text = open(SOURCE).read()
    assert f"kScanTile = {ha.INVERT_WIDE_TILE};" in text
    assert "kMaxSources = 1 << 20;" in text and ha.INVERT_WIDE_MAX_SOURCES == 1 << 20
    assert "kMaxEntries = 1 << 25;" in text and ha.INVERT_WIDE_MAX_ENTRIES == 1 << 25


def test_train_cli_takes_the_cloud_sizes(monkeypatch):
    """``python -m nsdp_amd.train --surface N --queries N`` reach the procedural loader under the names nsdp_amd.infer uses."""
    from nsdp_amd import train
    seen = []

    class _Stop(Exception):
        pass

    class _Loader:
        def __init__(self, seed, n_batches, batch, n_surf=2048, n_query=8192):
            seen.append((batch, n_surf, n_query))
            if len(seen) == 2:
                raise _Stop

    monkeypatch.setattr(train, "SyntheticLoader", _Loader)
    monkeypatch.setattr(train, "build_model", lambda *a, **k: (torch.nn.Linear(1, 1), None, None, None))
    monkeypatch.setattr(train, "optimizer_factory", lambda *a, **k: (None, None))
    import tempfile
    import yaml
    with tempfile.TemporaryDirectory() as tmp:
        cfg = os.path.join(tmp, "c.yaml")
        with open(cfg, "w") as f:
            yaml.safe_dump({"model": {"type": "forward"}, "training": {"epochs": 1}}, f)
        with pytest.raises(_Stop):
            train.main([cfg, os.path.join(tmp, "exp"), "--surface", "25000", "--queries", "300", "--batch", "1"])
        assert seen == [(1, 25000, 300), (1, 25000, 300)]
        seen.clear()
        with pytest.raises(_Stop):
            train.main([cfg, os.path.join(tmp, "exp")])
        assert seen == [(8, 2048, 8192), (8, 2048, 8192)]


def test_scatter_add_rows_gate_follows_the_builds(monkeypatch):
    """index_points' backward takes the lists exactly where a build serves the shape; anything else keeps the atomic kernel."""
    from nsdp_amd import pointnet2_utils as pu
    seen = []
    monkeypatch.setattr(ha, "lists_serve", lambda B, E, N: (seen.append((B, E, N)), False)[1])
    monkeypatch.setattr(pu, "lib", lambda: (_ for _ in ()).throw(RuntimeError("atomic kernel")))
    with pytest.raises(RuntimeError, match="atomic kernel|GPU tensor"):
        pu.scatter_add_rows(torch.zeros(2, 50, 4), torch.zeros(2, 50, dtype=torch.int32), 9000)
    assert seen == [(2, 50, 9000)]
