"""Drop-in for the reference's ``pointnet2_ops_lib/pointnet2_ops/pointnet2_utils.py`` on MI355X.

Same public names, argument order, tensor layouts, dtypes and differentiability as the reference
(pointnet2_utils.py:34-379): ``furthest_point_sample``, ``gather_operation``, ``three_nn``,
``three_interpolate``, ``grouping_operation``, ``ball_query`` and the ``QueryAndGroup`` / ``GroupAll``
modules -- so a call site such as model/encoder/blocks.py:283 works unchanged.  The native side is
libnsdp_hip.so (hand-written HIP for gfx950) behind the C ABI of include/nsdp_hip.h instead of the
pybind11 module ``pointnet2_ops._ext`` (_ext-src/src/bindings.cpp:6-19).

Error behaviour mirrors the reference's CHECK_* macros (_ext-src/include/utils.h:5-25): non-contiguous,
wrong-dtype or CPU tensors raise ``RuntimeError`` (NsdpHipError is a RuntimeError).
"""
from __future__ import annotations

import contextlib
import ctypes
import os

import torch
import torch.nn as nn
from torch.autograd import Function

from . import _lib
from ._lib import check, fptr, iptr, lib, on_device, optptr, stream_ptr

_c_int = ctypes.c_int


# ------------------------------------------------------------------------------------------------
# thin functional layer over the C ABI (one function per entry point of include/nsdp_hip.h)
# ------------------------------------------------------------------------------------------------
def _switch(value, default: bool) -> bool:
    """An on/off knob from its environment text: unset or empty -> the default, "0" / "off" / "false" / "no" -> off, else on."""
    if value is None or not value.strip():
        return default
    return value.strip().lower() not in ("0", "off", "false", "no")


# Clouds of more than FPS_CLUSTER_MIN_POINTS - 1 points (and at most 262 144) are sampled by a cluster of workgroups
# (include/nsdp_sampling.h, csrc/fps_cluster.hip) instead of the one-workgroup large-cloud kernel of nsdp_furthest_point_sampling;
# the indices are the same.  NSDP_FPS_CLUSTER=0 / ``with fps_cluster(False):`` keeps the old kernel (the A/B partner).  Read when
# a call runs, so a captured graph keeps the kernel it was captured with.
FPS_CLUSTER = _switch(os.environ.get("NSDP_FPS_CLUSTER"), True)
FPS_CLUSTER_MIN_POINTS = 8193       # the lower end of the default range (profiles/fps_cluster.txt)
# The workspace of the latest cluster call on each (device, stream): what fps_cluster_status() reads when it is given none.  One
# entry per stream, replaced by that stream's next call and dropped by the check, so nothing accumulates.
_cluster_workspaces: dict = {}


@contextlib.contextmanager
def fps_cluster(on: bool):
    """``with pointnet2_utils.fps_cluster(False): ...`` -- the large-cloud sampling kernel inside the block, restored after it."""
    global FPS_CLUSTER
    prev, FPS_CLUSTER = FPS_CLUSTER, bool(on)
    try:
        yield
    finally:
        FPS_CLUSTER = prev


def fps_cluster_groups(n_max: int) -> int:
    """Workgroups per cloud the cluster entries take by default: 0 where they do not serve (n_max <= 8192 or > 262 144)."""
    return int(lib().nsdp_fps_cluster_groups(_c_int(int(n_max))))


def _use_cluster(n_max: int) -> bool:
    return FPS_CLUSTER and n_max >= FPS_CLUSTER_MIN_POINTS and fps_cluster_groups(n_max) != 0


def _cluster_workspace(B, n_max, npoint, groups, device, workspace):
    fn = lib().nsdp_fps_cluster_workspace_bytes
    fn.restype = ctypes.c_size_t
    need = int(fn(_c_int(B), _c_int(n_max), _c_int(int(npoint)), _c_int(int(groups))))
    if need == 0 and B > 0 and int(npoint) > 0:
        raise _lib.NsdpHipError(f"fps_cluster: no cluster of groups={int(groups)} for {n_max} points (1..32 workgroups of 8192 points; "
                                "default only above 8192 points)")
    if workspace is None:
        workspace = torch.empty((need,), dtype=torch.uint8, device=device)
    elif not (workspace.is_cuda and workspace.is_contiguous() and workspace.numel() * workspace.element_size() >= need):
        raise _lib.NsdpHipError(f"fps_cluster: the workspace must be a contiguous GPU tensor of at least {need} bytes")
    stream = stream_ptr()
    _cluster_workspaces[(workspace.device.index, stream.value)] = (workspace, stream)
    return workspace


def furthest_point_sample_cluster(xyz: torch.Tensor, npoint: int, groups: int = 0, workspace=None) -> torch.Tensor:
    """``furthest_point_sample`` by ``groups`` workgroups per cloud (include/nsdp_sampling.h; 0: ceil(N / 8192), for N above
    8192): xyz (B,N,3) -> (B,npoint) int32, the same indices.  ``workspace``: a buffer of the caller's, else allocated here."""
    with on_device(xyz):
        B, N, C = xyz.shape
        if C != 3:
            raise _lib.NsdpHipError("xyz must be (B, N, 3)")
        out = torch.empty((B, int(npoint)), dtype=torch.int32, device=xyz.device)
        ws = _cluster_workspace(B, N, npoint, groups, xyz.device, workspace)
        check(lib().nsdp_furthest_point_sampling_cluster(fptr(xyz, "xyz"), _c_int(B), _c_int(N), _c_int(int(npoint)),
                                                         _c_int(int(groups)), optptr(ws), iptr(out), stream_ptr()),
              "nsdp_furthest_point_sampling_cluster")
    return out


def fps_cluster_status(workspace=None) -> int:
    """0, or the negative status (NSDP_ETIMEOUT) if a wait between the workgroups of a cloud gave up: the indices of that call
    are in range and wrong.  With a ``workspace``: the call that last used it, after synchronising the current stream.  Without:
    the latest cluster call of EVERY stream that made one since the last check (the side stream of the geometry pyramid and
    the streams of a captured step included), each after synchronising its own stream; the record is dropped.  Not inside a
    capture.  The kernels cannot hang or fault on a wait that runs out, so nothing reads this word unasked: a caller that runs
    cluster calls of several streams at the same time checks it where it synchronises anyway (nsdp_amd.infer does)."""
    if workspace is not None:
        with on_device(workspace):
            return int(lib().nsdp_fps_cluster_status(optptr(workspace), stream_ptr()))
    worst = 0
    while _cluster_workspaces:
        _, (ws, stream) = _cluster_workspaces.popitem()
        with on_device(ws):
            worst = worst or int(lib().nsdp_fps_cluster_status(optptr(ws), stream))
    return worst


def check_fps_cluster() -> None:
    """``fps_cluster_status()`` as an error: raises if a cluster call since the last check gave up a wait."""
    rc = fps_cluster_status()
    if rc:
        raise _lib.NsdpHipError("farthest-point sampling by a workgroup cluster gave up a wait between workgroups (status "
                                f"{rc}): its indices are wrong.  Cluster calls of several streams held the device at the same time; "
                                "NSDP_FPS_CLUSTER=0 takes the one-workgroup kernel")


# Exact k-nearest-neighbour search through a uniform cell grid (include/nsdp_search.h, csrc/knn_grid.hip): the indices and the
# distance bits of the exhaustive scan (nsdp_knn / nsdp_knn_ragged_source) without its n x m distance tests.  NSDP_KNN_GRID:
# "1" (default) = the grid where the source bound (m, n_max) is at least KNN_GRID_MIN_POINTS and queries x source rows per
# shape at least KNN_GRID_MIN_TESTS, "0" = the scan everywhere (the A/B partner), "force" = the grid wherever its entries accept
# the arguments.  Read when a call runs, so a captured graph keeps the kernels it was captured with.
KNN_GRID_MODES = ("0", "1", "force")


def _grid_mode(value, default: str = "1") -> str:
    """NSDP_KNN_GRID's text -> "0" / "1" / "force": "force" by name, everything else as the on/off switch ``_switch`` parses."""
    if value is not None and str(value).strip().lower() == "force":
        return "force"
    return "1" if _switch(None if value is None else str(value), default != "0") else "0"


KNN_GRID = _grid_mode(os.environ.get("NSDP_KNN_GRID"))
KNN_GRID_MIN_POINTS = 25000         # the smallest measured source bound from which the grid wins (profiles/knn_grid.txt)
KNN_GRID_MIN_TESTS = 12_500_000     # ... and the smallest queries x source rows per shape: 500 centres x 25 000 points
KNN_GRID_MAX_K, KNN_GRID_MAX_POINTS = 32, 1 << 20      # the limits of the entries
# The workspace of the latest grid search on each (device, stream): what knn_grid_stats() reads when it is given none.  One entry
# per stream, replaced by that stream's next search and dropped by the read, so nothing accumulates -- but the entry keeps that
# one workspace allocated (up to 25 MB per shape at 128 cells per axis) until then: forget_knn_grid_stats() drops all of them.
_grid_workspaces: dict = {}


@contextlib.contextmanager
def knn_grid_mode(mode):
    """``with pointnet2_utils.knn_grid_mode("0"): ...`` -- "0" / "1" / "force" (or False / True) inside the block, the previous
    mode restored after it."""
    global KNN_GRID
    mode = {True: "1", False: "0"}.get(mode, mode)
    if mode not in KNN_GRID_MODES:
        raise ValueError(f"knn_grid_mode: one of {KNN_GRID_MODES}, got {mode!r}")
    prev, KNN_GRID = KNN_GRID, mode
    try:
        yield
    finally:
        KNN_GRID = prev


def _grid_accepts(B: int, m: int, k: int) -> bool:
    return 1 <= int(k) <= min(KNN_GRID_MAX_K, m) and m <= KNN_GRID_MAX_POINTS and 1 <= B <= 65535


def _use_grid(t: torch.Tensor, B: int, n: int, m: int, k: int) -> bool:
    """The dispatch of ``knn`` / ``knn_ragged_source``: n queries against (at most) m source rows per shape."""
    if KNN_GRID == "0" or not t.is_cuda or n <= 0 or not _grid_accepts(B, m, k):
        return False
    return KNN_GRID == "force" or (m >= KNN_GRID_MIN_POINTS and n * m >= KNN_GRID_MIN_TESTS)


def _grid_workspace(B, queries, source_rows, m_max, device, workspace):
    fn = lib().nsdp_knn_grid_workspace_bytes
    fn.restype = ctypes.c_size_t
    need = int(fn(_c_int(B), _c_int(queries), _c_int(source_rows), _c_int(m_max)))
    if workspace is None:
        workspace = torch.empty((need,), dtype=torch.uint8, device=device)
    elif not (workspace.is_cuda and workspace.is_contiguous() and workspace.numel() * workspace.element_size() >= need):
        raise _lib.NsdpHipError(f"knn_grid: the workspace must be a contiguous GPU tensor of at least {need} bytes")
    # (not during a capture: a workspace from the graph's private pool would stay pinned for counters that cannot be read there)
    if need and not torch.cuda.is_current_stream_capturing():
        stream = stream_ptr()
        _grid_workspaces[(workspace.device.index, stream.value)] = workspace
    return workspace


def knn_grid(query: torch.Tensor, source: torch.Tensor, k: int, return_dist: bool = False, workspace=None):
    """``knn`` through the cell grid (include/nsdp_search.h), at any size its entries accept: query (B,n,3), source (B,m,3) ->
    idx (B,n,k) int32 (and dist2), the bits of ``knn``.  ``workspace``: a buffer of the caller's, else allocated here."""
    with on_device(query):
        if query.dim() != 3 or query.shape[2] != 3 or source.dim() != 3 or source.shape[2] != 3 or source.shape[0] != query.shape[0]:
            raise _lib.NsdpHipError(f"knn_grid: query (B,n,3) and source (B,m,3), got {tuple(query.shape)}, {tuple(source.shape)}")
        B, n, m = int(query.shape[0]), int(query.shape[1]), int(source.shape[1])
        idx = torch.empty((B, n, int(k)), dtype=torch.int32, device=query.device)
        d2 = torch.empty((B, n, int(k)), dtype=torch.float32, device=query.device) if return_dist else None
        ws = _grid_workspace(B, B * n, B * m, m, query.device, workspace)
        check(lib().nsdp_knn_grid(fptr(query, "query"), fptr(source, "source"), _c_int(B), _c_int(n), _c_int(m), _c_int(int(k)),
                                  optptr(ws), iptr(idx), optptr(d2), stream_ptr()), "nsdp_knn_grid")
    return (idx, d2) if return_dist else idx


def forget_knn_grid_stats() -> None:
    """Drops the remembered workspaces of ``knn_grid_stats()`` (their memory goes back to the allocator)."""
    _grid_workspaces.clear()


def knn_grid_stats(workspace=None):
    """What the grid search that last used ``workspace`` did, after synchronising the current stream: a dict of ``queries``,
    ``tests`` (distance tests), ``scanned`` (queries finished by the plain scan) and ``cells`` (cells allocated).  Without a
    workspace: the latest search on the current stream, whose record is dropped -- None if there has been none since the last
    read.  Not inside a capture."""
    if workspace is None:
        if not torch.cuda.is_available():
            return None
        workspace = _grid_workspaces.pop((torch.cuda.current_device(), stream_ptr().value), None)
        if workspace is None:
            return None
    with on_device(workspace):
        out = (ctypes.c_int64 * 4)()
        check(lib().nsdp_knn_grid_stats(optptr(workspace), stream_ptr(), out), "nsdp_knn_grid_stats")
    return {"queries": int(out[0]), "tests": int(out[1]), "scanned": int(out[2]), "cells": int(out[3])}


def _fps(xyz: torch.Tensor, npoint: int) -> torch.Tensor:
    B, N, C = xyz.shape
    if C != 3:
        raise _lib.NsdpHipError("xyz must be (B, N, 3)")
    if N > 8192 and xyz.is_cuda and _use_cluster(N):
        return furthest_point_sample_cluster(xyz, npoint)
    out = torch.empty((B, int(npoint)), dtype=torch.int32, device=xyz.device)
    tmp = torch.empty((B, N), dtype=torch.float32, device=xyz.device) if N > 8192 else None
    with on_device(xyz):
        check(lib().nsdp_furthest_point_sampling(fptr(xyz, "xyz"), _c_int(B), _c_int(N), _c_int(int(npoint)),
                                                 optptr(tmp), iptr(out), stream_ptr()),
              "nsdp_furthest_point_sampling")
    return out


def knn(query: torch.Tensor, source: torch.Tensor, k: int, return_dist: bool = False):
    """``square_distance(query, source).argsort()[:, :, :k]`` without the n x m matrix.
    query (B,n,3), source (B,m,3) -> idx (B,n,k) int32 ascending by (distance, index)."""
    B, n, _ = query.shape
    m = source.shape[1]
    if _use_grid(query, int(B), int(n), int(m), k):      # large clouds: the cell grid, the same bits
        return knn_grid(query, source, k, return_dist)
    idx = torch.empty((B, n, int(k)), dtype=torch.int32, device=query.device)
    d2 = torch.empty((B, n, int(k)), dtype=torch.float32, device=query.device) if return_dist else None
    with on_device(query):
        check(lib().nsdp_knn(fptr(query, "query"), fptr(source, "source"), _c_int(B), _c_int(n), _c_int(m),
                             _c_int(int(k)), iptr(idx), optptr(d2), stream_ptr()), "nsdp_knn")
    return (idx, d2) if return_dist else idx


def knn_ragged(query: torch.Tensor, offsets: torch.Tensor, source: torch.Tensor, k: int, return_dist: bool = False,
               idx_out=None, dist_out=None):
    """``knn`` over a packed query set (nsdp_amd.ragged): query (cap,3), offsets (B+1) int32 on the device, source (B,m,3) ->
    idx (cap,k) int32 (and dist2 (cap,k)); row r of shape b is searched in source[b].  Rows at or beyond offsets[B] are not
    written (``idx_out`` / ``dist_out``: buffers of the caller's, e.g. the static ones of a captured graph).  The host never
    reads ``offsets``.  One lane per query (the decoder's case: few source points); the bits of ``knn`` on each shape alone."""
    with on_device(query):
        if query.dim() != 2 or query.shape[1] != 3 or source.dim() != 3 or source.shape[2] != 3:
            raise _lib.NsdpHipError(f"knn_ragged: query (cap,3) and source (B,m,3), got {tuple(query.shape)}, {tuple(source.shape)}")
        cap, (B, m) = query.shape[0], source.shape[:2]
        if offsets.numel() != B + 1:
            raise _lib.NsdpHipError(f"knn_ragged: {B} shapes need {B + 1} offsets, got {offsets.numel()}")
        idx = torch.empty((cap, int(k)), dtype=torch.int32, device=query.device) if idx_out is None else idx_out
        d2 = dist_out if dist_out is not None else (
            torch.empty((cap, int(k)), dtype=torch.float32, device=query.device) if return_dist else None)
        if tuple(idx.shape) != (cap, int(k)) or (d2 is not None and tuple(d2.shape) != (cap, int(k))):
            raise _lib.NsdpHipError(f"knn_ragged: output buffers must be ({cap},{int(k)})")
        check(lib().nsdp_knn_ragged(fptr(query, "query"), iptr(offsets, "offsets"), fptr(source, "source"), _c_int(B),
                                    _c_int(cap), _c_int(m), _c_int(int(k)), iptr(idx, "idx_out"),
                                    optptr(None) if d2 is None else fptr(d2, "dist_out"), stream_ptr()), "nsdp_knn_ragged")
    return (idx, d2) if (return_dist or dist_out is not None) else idx


def _packed_source(what, xyz, offsets, n_max):
    """The checks the two packed-source calls share (shapes only: the host never reads ``offsets``) -> (cap, B, n_max)."""
    if xyz.dim() != 2 or xyz.shape[1] != 3:
        raise _lib.NsdpHipError(f"{what}: the packed cloud must be (cap,3), got {tuple(xyz.shape)}")
    if offsets.dim() != 1 or offsets.numel() < 2:
        raise _lib.NsdpHipError(f"{what}: offsets must be (B+1) int32 with B >= 1, got {tuple(offsets.shape)}")
    cap = int(xyz.shape[0])
    if cap <= 0 or int(n_max) <= 0:
        raise _lib.NsdpHipError(f"{what}: an empty packed cloud (cap={cap}, n_max={int(n_max)})")
    return cap, int(offsets.numel()) - 1, min(int(n_max), cap)


def furthest_point_sample_ragged(xyz: torch.Tensor, offsets: torch.Tensor, npoint: int, n_max: int, idx_out=None, groups: int = 0,
                                 workspace=None):
    """``furthest_point_sample`` over a packed batch of clouds of different sizes (nsdp_amd.ragged): xyz (cap,3), offsets (B+1)
    int32 on the device, ``n_max`` = an upper bound of any shape's row count (it sizes the workgroup; the kernel clamps to it)
    -> idx (B,npoint) int32 of PACKED rows (offsets[b] + the index within shape b).  Minus its offset, a shape's row is the
    result of ``furthest_point_sample`` on that shape alone, ties included, whatever ``n_max`` is.  The host never reads
    ``offsets``; ``idx_out``: a buffer of the caller's.  With ``n_max`` above 8192 (and the FPS_CLUSTER knob on), or with an
    explicit ``groups`` (1..32, ``n_max <= groups * 8192``), every shape is sampled by a cluster of workgroups
    (include/nsdp_sampling.h; ``workspace``: a buffer of the caller's for it): the same indices."""
    with on_device(xyz):
        cap, B, n_max = _packed_source("furthest_point_sample_ragged", xyz, offsets, n_max)
        out = torch.empty((B, int(npoint)), dtype=torch.int32, device=xyz.device) if idx_out is None else idx_out
        if tuple(out.shape) != (B, int(npoint)):
            raise _lib.NsdpHipError(f"furthest_point_sample_ragged: idx_out must be ({B},{int(npoint)})")
        if groups or (n_max > 8192 and _use_cluster(n_max)):
            ws = _cluster_workspace(B, n_max, npoint, groups, xyz.device, workspace)
            check(lib().nsdp_furthest_point_sampling_cluster_ragged(fptr(xyz, "xyz"), iptr(offsets, "offsets"), _c_int(B), _c_int(cap),
                                                                    _c_int(n_max), _c_int(int(npoint)), _c_int(int(groups)),
                                                                    optptr(ws), iptr(out, "idx_out"), stream_ptr()),
                  "nsdp_furthest_point_sampling_cluster_ragged")
            return out
        tmp = torch.empty((cap,), dtype=torch.float32, device=xyz.device) if n_max > 8192 else None
        check(lib().nsdp_furthest_point_sampling_ragged(fptr(xyz, "xyz"), iptr(offsets, "offsets"), _c_int(B), _c_int(cap),
                                                        _c_int(n_max), _c_int(int(npoint)), optptr(tmp), iptr(out, "idx_out"),
                                                        stream_ptr()), "nsdp_furthest_point_sampling_ragged")
    return out


def _knn_ragged_source(grid, query, source, offsets, k, n_max, query_offsets, return_dist, idx_out, dist_out, workspace=None):
    """The body of ``knn_ragged_source`` / ``knn_grid_ragged_source``.  grid: None = by the dispatch, True = the grid entry."""
    what = "knn_grid_ragged_source" if grid else "knn_ragged_source"
    with on_device(query):
        cap, B, n_max = _packed_source(what, source, offsets, n_max)
        if query_offsets is None:
            if query.dim() != 3 or query.shape[2] != 3 or query.shape[0] != B:
                raise _lib.NsdpHipError(f"{what}: rectangular queries must be ({B},n,3), got {tuple(query.shape)}")
            n, qcap, lead = int(query.shape[1]), 0, (B, int(query.shape[1]))
        else:
            if query.dim() != 2 or query.shape[1] != 3 or query_offsets.numel() != B + 1:
                raise _lib.NsdpHipError(f"{what}: packed queries must be (qcap,3) with {B + 1} offsets, got "
                                        f"{tuple(query.shape)}, {query_offsets.numel()}")
            n, qcap, lead = 0, int(query.shape[0]), (int(query.shape[0]),)
        want = lead + (int(k),)
        idx = torch.empty(want, dtype=torch.int32, device=query.device) if idx_out is None else idx_out
        d2 = dist_out if dist_out is not None else (
            torch.empty(want, dtype=torch.float32, device=query.device) if return_dist else None)
        if tuple(idx.shape) != want or (d2 is not None and tuple(d2.shape) != want):
            raise _lib.NsdpHipError(f"{what}: output buffers must be {want}")
        qptr = optptr(None) if query_offsets is None else iptr(query_offsets, "query_offsets")
        dptr = optptr(None) if d2 is None else fptr(d2, "dist_out")
        # (a shape of a packed query set has at most n_max rows when it is the source itself, and at most qcap otherwise)
        per_shape = n if query_offsets is None else min(qcap, n_max if query_offsets is offsets else qcap)
        if grid or (grid is None and _use_grid(query, B, per_shape, n_max, k)):
            ws = _grid_workspace(B, qcap if query_offsets is not None else B * n, cap, n_max, query.device, workspace)
            check(lib().nsdp_knn_grid_ragged_source(fptr(query, "query"), qptr, fptr(source, "source"), iptr(offsets, "offsets"),
                                                    _c_int(B), _c_int(n), _c_int(qcap), _c_int(cap), _c_int(n_max), _c_int(int(k)),
                                                    optptr(ws), iptr(idx, "idx_out"), dptr, stream_ptr()),
                  "nsdp_knn_grid_ragged_source")
        else:
            check(lib().nsdp_knn_ragged_source(fptr(query, "query"), qptr, fptr(source, "source"), iptr(offsets, "offsets"), _c_int(B),
                                               _c_int(n), _c_int(qcap), _c_int(cap), _c_int(n_max), _c_int(int(k)),
                                               iptr(idx, "idx_out"), dptr, stream_ptr()), "nsdp_knn_ragged_source")
    return (idx, d2) if (return_dist or dist_out is not None) else idx


def knn_ragged_source(query: torch.Tensor, source: torch.Tensor, offsets: torch.Tensor, k: int, n_max: int, query_offsets=None,
                      return_dist: bool = False, idx_out=None, dist_out=None):
    """``knn`` against a packed source set: source (cap,3), offsets (B+1) int32 on the device, ``n_max`` as above.  The queries
    are rectangular (B,n,3) -> idx (B,n,k), or packed themselves, (qcap,3) with ``query_offsets`` (B+1) -> idx (qcap,k); the
    self-search of a packed cloud is ``knn_ragged_source(xyz, xyz, offsets, k, n_max, query_offsets=offsets)``.  The indices
    are PACKED rows of ``source``; minus the shape's offset they, and the distance bits, are those of ``knn`` on that shape
    alone.  Rows of a packed query set at or beyond query_offsets[B] are not written (``idx_out`` / ``dist_out``: buffers of
    the caller's).  The host never reads either offsets tensor.  Large clouds go through the cell grid (KNN_GRID above): the
    same bits."""
    return _knn_ragged_source(None, query, source, offsets, k, n_max, query_offsets, return_dist, idx_out, dist_out)


def knn_grid_ragged_source(query: torch.Tensor, source: torch.Tensor, offsets: torch.Tensor, k: int, n_max: int, query_offsets=None,
                           return_dist: bool = False, idx_out=None, dist_out=None, workspace=None):
    """``knn_ragged_source`` through the cell grid (include/nsdp_search.h), at any size its entries accept: the same arguments
    and the same bits.  ``workspace``: a buffer of the caller's, else allocated here."""
    return _knn_ragged_source(True, query, source, offsets, k, n_max, query_offsets, return_dist, idx_out, dist_out, workspace)

def nn_dist2(query: torch.Tensor, source: torch.Tensor, return_index: bool = False):
    """The squared distance of every query point to its nearest source point (include/nsdp_eval.h): query (B,n,3), source
    (B,m,3) -> dist2 (B,n) fp32 with the bits of ``knn(query, source, 1, return_dist=True)``, and with ``return_index`` that
    search's index (B,n) int32 as well.  Without the index the source range is split over workgroups (the metric's case)."""
    with on_device(query):
        if query.dim() != 3 or query.shape[2] != 3 or source.dim() != 3 or source.shape[2] != 3 or source.shape[0] != query.shape[0]:
            raise _lib.NsdpHipError(f"nn_dist2: query (B,n,3) and source (B,m,3), got {tuple(query.shape)}, {tuple(source.shape)}")
        B, n, m = int(query.shape[0]), int(query.shape[1]), int(source.shape[1])
        d2 = torch.empty((B, n), dtype=torch.float32, device=query.device)
        idx = torch.empty((B, n), dtype=torch.int32, device=query.device) if return_index else None
        check(lib().nsdp_nn_dist2(fptr(query, "query"), fptr(source, "source"), _c_int(B), _c_int(n), _c_int(m), fptr(d2, "dist2_out"),
                                  optptr(idx), stream_ptr()), "nsdp_nn_dist2")
    return (d2, idx) if return_index else d2


def nn_dist2_ragged(query: torch.Tensor, query_offsets: torch.Tensor, source: torch.Tensor, source_offsets: torch.Tensor,
                    return_index: bool = False, dist_out=None, idx_out=None):
    """``nn_dist2`` with both sets packed (nsdp_amd.ragged): query (qcap,3) + query_offsets (B+1), source (scap,3) +
    source_offsets (B+1), int32 offsets on the device -> dist2 (qcap) and, with ``return_index``, the PACKED source row (qcap)
    int32: element for element ``knn_ragged_source`` at k = 1.  Rows at or beyond query_offsets[B] are not written
    (``dist_out`` / ``idx_out``: buffers of the caller's); a shape without source rows gets FLT_MAX.  The host never reads
    either offsets tensor."""
    with on_device(query):
        if query.dim() != 2 or query.shape[1] != 3 or source.dim() != 2 or source.shape[1] != 3:
            raise _lib.NsdpHipError(f"nn_dist2_ragged: packed query (qcap,3) and source (scap,3), got {tuple(query.shape)}, "
                                    f"{tuple(source.shape)}")
        if query_offsets.dim() != 1 or query_offsets.numel() < 2 or source_offsets.shape != query_offsets.shape:
            raise _lib.NsdpHipError(f"nn_dist2_ragged: both offsets must be (B+1) int32 with B >= 1, got {tuple(query_offsets.shape)}, "
                                    f"{tuple(source_offsets.shape)}")
        B, qcap, scap = int(query_offsets.numel()) - 1, int(query.shape[0]), int(source.shape[0])
        d2 = torch.empty((qcap,), dtype=torch.float32, device=query.device) if dist_out is None else dist_out
        idx = idx_out if idx_out is not None else (
            torch.empty((qcap,), dtype=torch.int32, device=query.device) if return_index else None)
        if tuple(d2.shape) != (qcap,) or (idx is not None and tuple(idx.shape) != (qcap,)):
            raise _lib.NsdpHipError(f"nn_dist2_ragged: output buffers must be ({qcap},)")
        check(lib().nsdp_nn_dist2_ragged(fptr(query, "query"), iptr(query_offsets, "query_offsets"), fptr(source, "source"),
                                         iptr(source_offsets, "source_offsets"), _c_int(B), _c_int(qcap), _c_int(scap),
                                         fptr(d2, "dist_out"), optptr(None) if idx is None else iptr(idx, "idx_out"),
                                         stream_ptr()), "nsdp_nn_dist2_ragged")
    return (d2, idx) if (return_index or idx_out is not None) else d2


def segment_mean(values: torch.Tensor, offsets: torch.Tensor, sqrt: bool = False) -> torch.Tensor:
    """Per-shape mean of a packed column (include/nsdp_eval.h): values (cap) fp32, offsets (B+1) int32 on the device -> (B)
    fp32, the mean of v -- or of sqrt(max(v, 0)) with ``sqrt`` -- over each shape's rows, accumulated in double in a fixed
    order: the bits depend on that shape's rows alone.  NaN for a shape without rows.  No host synchronisation."""
    with on_device(values):
        if values.dim() != 1 or offsets.dim() != 1 or offsets.numel() < 2:
            raise _lib.NsdpHipError(f"segment_mean: values (cap) and offsets (B+1) with B >= 1, got {tuple(values.shape)}, "
                                    f"{tuple(offsets.shape)}")
        B = int(offsets.numel()) - 1
        out = torch.empty((B,), dtype=torch.float32, device=values.device)
        check(lib().nsdp_segment_mean_f32(fptr(values, "values"), iptr(offsets, "offsets"), _c_int(B), _c_int(int(values.shape[0])),
                                          _c_int(1 if sqrt else 0), fptr(out, "out"), stream_ptr()), "nsdp_segment_mean_f32")
    return out


def gather_rows(points: torch.Tensor, idx: torch.Tensor) -> torch.Tensor:
    """index_points for a 2-D index: points (B,N,C), idx (B,S) int32 -> (B,S,C)."""
    B, N, C = points.shape
    S = idx.shape[1]
    out = torch.empty((B, S, C), dtype=torch.float32, device=points.device)
    with on_device(points):
        check(lib().nsdp_gather_rows(fptr(points, "points"), iptr(idx, "idx"), _c_int(B), _c_int(N),
                                     _c_int(C), _c_int(S), fptr(out), stream_ptr()), "nsdp_gather_rows")
    return out


def rel_coords4(query: torch.Tensor, source: torch.Tensor, idx: torch.Tensor, sign: float = 1.0) -> torch.Tensor:
    """(sign * (query_i - source[idx_ij]), 0) as [B, n, k, 4] (nsdp_rel_coords4): no gradient."""
    B, n, _ = query.shape
    m, k = source.shape[1], idx.shape[2]
    out = torch.empty((B, n, k, 4), dtype=torch.float32, device=query.device)
    with on_device(query):
        check(lib().nsdp_rel_coords4(fptr(query, "query"), fptr(source, "source"), iptr(idx, "idx"), _c_int(B), _c_int(n),
                                     _c_int(m), _c_int(k), ctypes.c_float(sign), fptr(out), stream_ptr()), "nsdp_rel_coords4")
    return out


# index_points' backward: gather-reduce over inverse index lists (csrc/segment.hip: deterministic, every row read once at
# stream rate) instead of global fp32 atomics (1.0-1.25 TB/s) wherever the lists can be built -- they are cached on the index
# tensor, so an index set that is reused (two gathers of one kNN set, several steps over fixed geometry) builds them once.
# NSDP_SCATTER_ROWS=atomic keeps the atomic kernel (A/B knob).
_SCATTER_INVERSE = __import__("os").environ.get("NSDP_SCATTER_ROWS", "inverse") != "atomic"
_SCATTER_INVERSE_MIN_ROWS = 4096        # rows per launch below which one atomic launch beats invert + segment sum
# ... which is taken only with NSDP_SCATTER_DETERMINISTIC=0: by default a scatter goes through the lists at every size, so that a
# train step's result never depends on the order in which fp32 atomics retire (the replay-equals-eager tests hold every model to that)
_SCATTER_DETERMINISTIC = __import__("os").environ.get("NSDP_SCATTER_DETERMINISTIC", "1") != "0"


def scatter_add_rows(grad_out: torch.Tensor, idx: torch.Tensor, N: int) -> torch.Tensor:
    B, S, C = grad_out.shape
    # (average list length S / N <= 64: the list build sorts every list with one thread -- long lists, e.g. 57 344 gathers
    # of 100 anchors, cost more to build than the atomics cost)
    # Rows of any width: a width that is not a multiple of 4 -- the COORDINATE gradients of FlowArbitrary's second network,
    # whose input points are the first network's predictions (reference model/flow_arbitrary.py:19-27) -- is zero-padded to
    # float4 rows for the list kernel; through the atomic kernel those three-float rows made the whole step depend on the order
    # in which atomics retire (two eager runs of one FlowArbitrary step differed in 1589 of 1813 tensors).  _SCATTER_DETERMINISTIC
    # (default on) also takes the lists below the row count where one atomic launch is faster.
    # Above 8192 source points the lists come from the many-workgroup build, within its limits (hip_attention.lists_serve; the
    # knob INVERT_WIDE at "0" keeps the bound); what it does not accept keeps the atomic kernel.
    from . import hip_attention
    if (_SCATTER_INVERSE and 1 <= C <= 256 and S > 0 and hip_attention.lists_serve(B, S, int(N)) and S <= 64 * int(N)
            and (B * S >= _SCATTER_INVERSE_MIN_ROWS or _SCATTER_DETERMINISTIC)
            and grad_out.is_cuda and grad_out.dtype is torch.float32 and grad_out.is_contiguous()):
        if C % 4:
            padded = torch.nn.functional.pad(grad_out, (0, 4 - C % 4))
            return hip_attention.segment_sum(padded, idx, int(N), 1.0)[:, :, :C].contiguous()
        return hip_attention.segment_sum(grad_out, idx, int(N), 1.0)
    out = torch.empty((B, int(N), C), dtype=torch.float32, device=grad_out.device)
    with on_device(grad_out):
        check(lib().nsdp_scatter_add_rows(fptr(grad_out, "grad_out"), iptr(idx, "idx"), _c_int(B), _c_int(int(N)),
                                          _c_int(C), _c_int(S), fptr(out), stream_ptr()),
              "nsdp_scatter_add_rows")
    return out


# User-handle drags (include/nsdp_handles.h, csrc/handles.hip; the rule itself: csrc/handles_rule.h): the bounding box of a
# cloud, and the handle rule + dragged target + columns 3..6 of the deformation network's input rows, with the drag parameters in
# device memory (nsdp_amd.edit).
HANDLE_PARTS = ("head", "tail", "frontleftfoot", "frontrightfoot", "behindleftfoot", "behindrightfoot")      # NSDP_HANDLE_* order
HANDLE_PARAM_WORDS = 8
HANDLE_MAX_POINTS = 1 << 20


def _points3(what, t):
    if not torch.is_tensor(t) or t.dim() != 3 or t.shape[2] != 3:
        raise _lib.NsdpHipError(f"{what} must be (B, n, 3), got {tuple(t.shape) if torch.is_tensor(t) else type(t).__name__}")


def _bytes_ptr(t, name, shape):
    """A (B,n) mask or flag tensor of one-byte elements (uint8 or bool) as a pointer; None -> null."""
    if t is None:
        return ctypes.c_void_p(0)
    if not torch.is_tensor(t) or not t.is_cuda:
        raise _lib.NsdpHipError(f"{name} must be a GPU tensor (CPU not supported, no fallback)")
    if t.dtype not in (torch.uint8, torch.bool) or tuple(t.shape) != tuple(shape) or not t.is_contiguous():
        raise _lib.NsdpHipError(f"{name} must be a contiguous uint8 / bool tensor of shape {tuple(shape)}, got {t.dtype} "
                                f"{tuple(t.shape)}")
    return ctypes.c_void_p(t.data_ptr())


def _bounds_buffers(who, need, B, device, workspace, out, refused):
    """The workspace and the (B,6) output of a bounds entry (``who``): the caller's, checked, or allocated here.  ``need``: the
    entry's workspace bytes, 0 when it refuses the sizes -- then ``refused`` says which."""
    if need == 0:
        raise _lib.NsdpHipError(f"{who}: {refused}")
    if workspace is None:
        workspace = torch.empty((need // 4,), dtype=torch.int32, device=device)
    elif not (workspace.is_cuda and workspace.is_contiguous() and workspace.numel() * workspace.element_size() >= need):
        raise _lib.NsdpHipError(f"{who}: the workspace must be a contiguous GPU tensor of at least {need} bytes")
    bounds = torch.empty((B, 6), dtype=torch.float32, device=device) if out is None else out
    if tuple(bounds.shape) != (B, 6):
        raise _lib.NsdpHipError(f"{who}: out must be ({B}, 6), got {tuple(bounds.shape)}")
    return workspace, bounds


def handle_bounds(cano: torch.Tensor, workspace=None, out=None) -> torch.Tensor:
    """Per-shape bounding box (nsdp_handle_bounds): cano (B,n,3) fp32 -> (B,6) fp32, min xyz then max xyz, the exact extremes
    (-0.0 sorts below +0.0).  ``workspace``: a buffer of the caller's, else allocated here; ``out``: a (B,6) buffer."""
    with on_device(cano):
        _points3("cano", cano)
        B, n = int(cano.shape[0]), int(cano.shape[1])
        fn = lib().nsdp_handle_bounds_workspace_bytes
        fn.restype = ctypes.c_size_t
        need = int(fn(_c_int(B), _c_int(n)))
        workspace, bounds = _bounds_buffers("handle_bounds", need, B, cano.device, workspace, out,
                                            f"B={B} shapes of n={n} points outside 1..65535 x 1..{HANDLE_MAX_POINTS}")
        check(lib().nsdp_handle_bounds(fptr(cano, "cano"), _c_int(B), _c_int(n), optptr(workspace), fptr(bounds, "bounds"),
                                       stream_ptr()), "nsdp_handle_bounds")
    return bounds


def handle_rows(cano, src: torch.Tensor, bounds, params: torch.Tensor, rows: torch.Tensor, handle_mask=None, move_mask=None,
                tgt=None, handle_out=None, move_out=None) -> torch.Tensor:
    """One drag written into the deformation network's input rows (nsdp_handle_rows): columns 3..6 of ``rows`` (B,n,7) become
    [handle * tgt | handle] with tgt = src + d * move; columns 0..2 are never written.  ``params`` (B,8) int32 on the device:
    {part, cliptail, partial_range, dx, dy, dz, 0, 0} (the floats by their bits).  ``handle_mask`` / ``move_mask`` (B,n) uint8 or
    bool, together: they replace the rule (cano and bounds may then be None).  ``tgt`` (B,n,3), ``handle_out`` / ``move_out``
    (B,n) uint8: optional outputs, buffers of the caller's.  Returns ``rows``."""
    with on_device(src):
        _points3("src", src)
        B, n = int(src.shape[0]), int(src.shape[1])
        if cano is not None:
            _points3("cano", cano)
        if tuple(rows.shape) != (B, n, 7) or (cano is not None and cano.shape != src.shape) or (tgt is not None and tgt.shape != src.shape):
            raise _lib.NsdpHipError(f"handle_rows: src ({B},{n},3) goes with cano and tgt of that shape and rows ({B},{n},7), got "
                                    f"rows {tuple(rows.shape)}")
        if tuple(params.shape) != (B, HANDLE_PARAM_WORDS) or (bounds is not None and tuple(bounds.shape) != (B, 6)):
            raise _lib.NsdpHipError(f"handle_rows: params must be ({B}, {HANDLE_PARAM_WORDS}) int32 and bounds ({B}, 6)")
        check(lib().nsdp_handle_rows(optptr(None) if cano is None else fptr(cano, "cano"), fptr(src, "src"),
                                     optptr(None) if bounds is None else fptr(bounds, "bounds"), iptr(params, "params"),
                                     _bytes_ptr(handle_mask, "handle_mask", (B, n)), _bytes_ptr(move_mask, "move_mask", (B, n)),
                                     _c_int(B), _c_int(n), fptr(rows, "rows"),
                                     optptr(None) if tgt is None else fptr(tgt, "tgt"),
                                     _bytes_ptr(handle_out, "handle_out", (B, n)), _bytes_ptr(move_out, "move_out", (B, n)),
                                     stream_ptr()), "nsdp_handle_rows")
    return rows


# The same two entries over packed rows (include/nsdp_handles_ragged.h, csrc/handles_ragged.hip): B meshes of different sizes.
def _packed3(what, t, cap=None):
    if not torch.is_tensor(t) or t.dim() != 2 or t.shape[1] != 3 or (cap is not None and t.shape[0] != cap):
        raise _lib.NsdpHipError(f"{what} must be packed ({'cap' if cap is None else cap}, 3), got "
                                f"{tuple(t.shape) if torch.is_tensor(t) else type(t).__name__}")


def _offsets_batch(what, offsets):
    if not torch.is_tensor(offsets) or offsets.dim() != 1 or offsets.numel() < 2:
        raise _lib.NsdpHipError(f"{what}: offsets must be (B+1) int32 with B >= 1, got "
                                f"{tuple(offsets.shape) if torch.is_tensor(offsets) else type(offsets).__name__}")
    return int(offsets.numel()) - 1


def handle_bounds_ragged(cano: torch.Tensor, offsets: torch.Tensor, n_max: int, workspace=None, out=None) -> torch.Tensor:
    """``handle_bounds`` of every shape of a packed set (nsdp_handle_bounds_ragged): cano (cap,3) fp32, offsets (B+1) int32 on
    the device, ``n_max`` an upper bound of the largest shape -> (B,6) fp32, the bits ``handle_bounds`` gives on each shape
    alone; a shape without rows gets the reductions' identities (two NaN patterns, named in the header).  The host never reads
    the offsets.  ``workspace``: a buffer of the caller's, else allocated here; ``out``: a (B,6) buffer."""
    with on_device(cano):
        _packed3("cano", cano)
        B, cap, n_max = _offsets_batch("handle_bounds_ragged", offsets), int(cano.shape[0]), int(n_max)
        fn = lib().nsdp_handle_bounds_ragged_workspace_bytes
        fn.restype = ctypes.c_size_t
        need = int(fn(_c_int(B), _c_int(cap), _c_int(n_max)))
        workspace, bounds = _bounds_buffers("handle_bounds_ragged", need, B, cano.device, workspace, out,
                                            f"B={B} shapes in cap={cap} rows with n_max={n_max} outside 1..65535, 1.., "
                                            f"1..{HANDLE_MAX_POINTS}")
        check(lib().nsdp_handle_bounds_ragged(fptr(cano, "cano"), iptr(offsets, "offsets"), _c_int(B), _c_int(cap), _c_int(n_max),
                                              optptr(workspace), fptr(bounds, "bounds"), stream_ptr()), "nsdp_handle_bounds_ragged")
    return bounds


def handle_rows_ragged(cano, src: torch.Tensor, offsets: torch.Tensor, bounds, params: torch.Tensor, rows: torch.Tensor,
                       handle_mask=None, move_mask=None, tgt=None, handle_out=None, move_out=None) -> torch.Tensor:
    """``handle_rows`` over packed rows (nsdp_handle_rows_ragged): src (cap,3), offsets (B+1) int32 on the device, ``params``
    (B,8) one drag per shape, ``bounds`` (B,6); columns 3..6 of ``rows`` (cap,7) are written for the rows of the B shapes,
    columns 0..2 and the padding rows never.  ``handle_mask`` / ``move_mask`` (cap,) uint8 or bool, together: they replace the
    rule (cano and bounds may then be None).  ``tgt`` (cap,3), ``handle_out`` / ``move_out`` (cap,): optional outputs.  Returns
    ``rows``."""
    with on_device(src):
        _packed3("src", src)
        B, cap = _offsets_batch("handle_rows_ragged", offsets), int(src.shape[0])
        if cano is not None:
            _packed3("cano", cano, cap)
        if tgt is not None:
            _packed3("tgt", tgt, cap)
        if not torch.is_tensor(rows) or tuple(rows.shape) != (cap, 7):
            raise _lib.NsdpHipError(f"handle_rows_ragged: src ({cap},3) goes with rows ({cap},7), got "
                                    f"{tuple(rows.shape) if torch.is_tensor(rows) else type(rows).__name__}")
        if tuple(params.shape) != (B, HANDLE_PARAM_WORDS) or (bounds is not None and tuple(bounds.shape) != (B, 6)):
            raise _lib.NsdpHipError(f"handle_rows_ragged: params must be ({B}, {HANDLE_PARAM_WORDS}) int32 and bounds ({B}, 6)")
        check(lib().nsdp_handle_rows_ragged(optptr(None) if cano is None else fptr(cano, "cano"), fptr(src, "src"),
                                            iptr(offsets, "offsets"), optptr(None) if bounds is None else fptr(bounds, "bounds"),
                                            iptr(params, "params"), _bytes_ptr(handle_mask, "handle_mask", (cap,)),
                                            _bytes_ptr(move_mask, "move_mask", (cap,)), _c_int(B), _c_int(cap), fptr(rows, "rows"),
                                            optptr(None) if tgt is None else fptr(tgt, "tgt"),
                                            _bytes_ptr(handle_out, "handle_out", (cap,)), _bytes_ptr(move_out, "move_out", (cap,)),
                                            stream_ptr()), "nsdp_handle_rows_ragged")
    return rows


# Labelled handle sets (include/nsdp_handle_sets.h, csrc/handle_sets.hip): several handles per shape, each with a 3 x 4 motion of
# its own, or a target per point; T poses of one source per launch.
HANDLE_SET_MAX_HANDLES = 255
HANDLE_SET_MAX_POSE_SHAPES = 65535


def _one_of_motions_targets(who, motions, targets):
    if (motions is None) == (targets is None):
        raise _lib.NsdpHipError(f"{who}: exactly one of motions and targets (got {'neither' if motions is None else 'both'})")
    given = motions if targets is None else targets
    if not torch.is_tensor(given):
        raise _lib.NsdpHipError(f"{who}: {'motions' if targets is None else 'targets'} must be a torch.Tensor, got "
                                f"{type(given).__name__}")


def handle_set_rows(src: torch.Tensor, labels: torch.Tensor, rows: torch.Tensor, motions=None, targets=None, tgt=None,
                    handle_out=None) -> torch.Tensor:
    """T poses of a labelled handle set written into the deformation network's input rows (nsdp_handle_set_rows): src (B,n,3),
    ``labels`` (B,n) uint8 -- 0 a free point, 1..H a handle, above H a free point -- and exactly one of ``motions`` (T,B,H,12),
    a row-major [A | t] per (pose, shape, handle), and ``targets`` (T,B,n,3), a target per point (every non-zero label is then a
    handle).  Columns 3..6 of ``rows`` (T,B,n,7) become [handle * tgt | handle]; columns 0..2 are never written.  ``tgt``
    (T,B,n,3), ``handle_out`` (B,n) uint8: optional outputs, buffers of the caller's.  T and H are the motion tensor's.  Returns
    ``rows``."""
    with on_device(src):
        _points3("src", src)
        B, n = int(src.shape[0]), int(src.shape[1])
        _one_of_motions_targets("handle_set_rows", motions, targets)
        if motions is not None:
            if motions.dim() != 4 or motions.shape[1] != B or motions.shape[3] != 12:
                raise _lib.NsdpHipError(f"handle_set_rows: motions must be (T, {B}, H, 12), got {tuple(motions.shape)}")
            T, H = int(motions.shape[0]), int(motions.shape[2])
        else:
            if targets.dim() != 4 or tuple(targets.shape[1:]) != (B, n, 3):
                raise _lib.NsdpHipError(f"handle_set_rows: targets must be (T, {B}, {n}, 3), got {tuple(targets.shape)}")
            T, H = int(targets.shape[0]), 0
        if not torch.is_tensor(rows) or tuple(rows.shape) != (T, B, n, 7) or (tgt is not None and tuple(tgt.shape) != (T, B, n, 3)):
            raise _lib.NsdpHipError(f"handle_set_rows: {T} poses of src ({B},{n},3) go with rows ({T},{B},{n},7) and tgt "
                                    f"({T},{B},{n},3), got rows {tuple(rows.shape) if torch.is_tensor(rows) else type(rows).__name__}"
                                    + ("" if tgt is None else f", tgt {tuple(tgt.shape)}"))
        check(lib().nsdp_handle_set_rows(fptr(src, "src"), _labels_ptr(labels, (B, n)),
                                         optptr(None) if motions is None else fptr(motions, "motions"),
                                         optptr(None) if targets is None else fptr(targets, "targets"),
                                         _c_int(B), _c_int(n), _c_int(H), _c_int(T), fptr(rows, "rows"),
                                         optptr(None) if tgt is None else fptr(tgt, "tgt"),
                                         _bytes_ptr(handle_out, "handle_out", (B, n)), stream_ptr()), "nsdp_handle_set_rows")
    return rows


def handle_set_rows_ragged(src: torch.Tensor, offsets: torch.Tensor, labels: torch.Tensor, rows: torch.Tensor, motions=None,
                           targets=None, tgt=None, handle_out=None) -> torch.Tensor:
    """One pose of a labelled handle set over packed rows (nsdp_handle_set_rows_ragged): src (cap,3), offsets (B+1) int32 on
    the device, ``labels`` (cap,) uint8 and exactly one of ``motions`` (B,H,12) and ``targets`` (cap,3); columns 3..6 of ``rows``
    (cap,7) are written for the rows of the B shapes, columns 0..2 and the padding rows never.  ``tgt`` (cap,3), ``handle_out``
    (cap,): optional outputs.  Returns ``rows``."""
    with on_device(src):
        _packed3("src", src)
        B, cap = _offsets_batch("handle_set_rows_ragged", offsets), int(src.shape[0])
        _one_of_motions_targets("handle_set_rows_ragged", motions, targets)
        H = 0
        if motions is not None:
            if motions.dim() != 3 or motions.shape[0] != B or motions.shape[2] != 12:
                raise _lib.NsdpHipError(f"handle_set_rows_ragged: motions must be ({B}, H, 12), got {tuple(motions.shape)}")
            H = int(motions.shape[1])
        else:
            _packed3("targets", targets, cap)
        if tgt is not None:
            _packed3("tgt", tgt, cap)
        if not torch.is_tensor(rows) or tuple(rows.shape) != (cap, 7):
            raise _lib.NsdpHipError(f"handle_set_rows_ragged: src ({cap},3) goes with rows ({cap},7), got "
                                    f"{tuple(rows.shape) if torch.is_tensor(rows) else type(rows).__name__}")
        check(lib().nsdp_handle_set_rows_ragged(fptr(src, "src"), iptr(offsets, "offsets"), _labels_ptr(labels, (cap,)),
                                                optptr(None) if motions is None else fptr(motions, "motions"),
                                                optptr(None) if targets is None else fptr(targets, "targets"),
                                                _c_int(B), _c_int(cap), _c_int(H), fptr(rows, "rows"),
                                                optptr(None) if tgt is None else fptr(tgt, "tgt"),
                                                _bytes_ptr(handle_out, "handle_out", (cap,)), stream_ptr()),
              "nsdp_handle_set_rows_ragged")
    return rows


def _labels_ptr(labels, shape):
    """The label bytes of a handle set: uint8 only (a bool tensor would name one handle), required."""
    if not torch.is_tensor(labels) or not labels.is_cuda:
        raise _lib.NsdpHipError("labels must be a GPU tensor (CPU not supported, no fallback)")
    if labels.dtype is not torch.uint8 or tuple(labels.shape) != tuple(shape) or not labels.is_contiguous():
        raise _lib.NsdpHipError(f"labels must be a contiguous uint8 tensor of shape {tuple(shape)}, got {labels.dtype} "
                                f"{tuple(labels.shape)}")
    return ctypes.c_void_p(labels.data_ptr())


# ------------------------------------------------------------------------------------------------
# autograd Functions with the reference's names and signatures
# ------------------------------------------------------------------------------------------------
class FurthestPointSampling(Function):
    @staticmethod
    def forward(ctx, xyz, npoint):
        """xyz (B,N,3) float32 -> (B,npoint) int32 (pointnet2_utils.py:34-62)."""
        out = _fps(xyz, npoint)
        ctx.mark_non_differentiable(out)
        return out

    @staticmethod
    def backward(ctx, grad_out):
        return ()


furthest_point_sample = FurthestPointSampling.apply


def _scatter_cm(grad_out3, idx2, N, idx_obj=None):
    """grad (B,C,N) of a channel-major gather: grad_out3 (B,C,E), idx2 (B,E).  Through the inverse index lists (cached on the
    index tensor; csrc/segment.hip builds them) and the atomics-free LDS-staged kernel where a row of E floats fits LDS and
    the lists are short; None otherwise (the caller then uses the LDS-table / atomic entry point)."""
    B, C, E = grad_out3.shape
    L = lib()
    if not (_SCATTER_INVERSE and 0 < N <= 32768 and E <= 64 * N and L.nsdp_scatter_cm_lists_supported(_c_int(B), _c_int(C),
                                                                                                  _c_int(N), _c_int(E))):
        return None
    from . import hip_attention
    # (the cache of the lists lives on the index tensor OBJECT the caller holds across calls, not on a view of it)
    offsets, entries = hip_attention.inverse_lists(idx2 if idx_obj is None else idx_obj, N)
    grad = torch.empty((B, C, N), dtype=torch.float32, device=grad_out3.device)
    with on_device(grad_out3):
        check(L.nsdp_scatter_cm_lists(fptr(grad_out3, "grad_out"), iptr(offsets), iptr(entries), _c_int(B), _c_int(C), _c_int(N),
                                      _c_int(E), fptr(grad), stream_ptr()), "nsdp_scatter_cm_lists")
    return grad


class GatherOperation(Function):
    @staticmethod
    def forward(ctx, features, idx):
        """features (B,C,N), idx (B,npoint) int32 -> (B,C,npoint) (pointnet2_utils.py:68-101)."""
        ctx.save_for_backward(idx, features)
        B, C, N = features.shape
        M = idx.shape[1]
        out = torch.empty((B, C, M), dtype=torch.float32, device=features.device)
        with on_device(features):
            check(lib().nsdp_gather_points(fptr(features, "features"), iptr(idx, "idx"), _c_int(B), _c_int(C),
                                           _c_int(N), _c_int(M), fptr(out), stream_ptr()), "nsdp_gather_points")
        return out

    @staticmethod
    def backward(ctx, grad_out):
        idx, features = ctx.saved_tensors
        B, C, N = features.shape
        M = idx.shape[1]
        grad_out = grad_out.contiguous()
        grad = _scatter_cm(grad_out, idx, N)
        if grad is not None:
            return grad, None
        grad = torch.empty((B, C, N), dtype=torch.float32, device=grad_out.device)
        with on_device(grad_out):
            check(lib().nsdp_gather_points_grad(fptr(grad_out, "grad_out"), iptr(idx), _c_int(B), _c_int(C),
                                                _c_int(N), _c_int(M), fptr(grad), stream_ptr()),
                  "nsdp_gather_points_grad")
        return grad, None


gather_operation = GatherOperation.apply


class ThreeNN(Function):
    @staticmethod
    def forward(ctx, unknown, known):
        """unknown (B,n,3), known (B,m,3) -> dist (B,n,3) (sqrt of d2), idx (B,n,3) int32
        (pointnet2_utils.py:104-136)."""
        B, n, _ = unknown.shape
        m = known.shape[1]
        dist2 = torch.empty((B, n, 3), dtype=torch.float32, device=unknown.device)
        idx = torch.empty((B, n, 3), dtype=torch.int32, device=unknown.device)
        with on_device(unknown):
            check(lib().nsdp_three_nn(fptr(unknown, "unknown"), fptr(known, "known"), _c_int(B), _c_int(n),
                                      _c_int(m), fptr(dist2), iptr(idx), stream_ptr()), "nsdp_three_nn")
        dist = torch.sqrt(dist2)
        ctx.mark_non_differentiable(dist, idx)
        return dist, idx

    @staticmethod
    def backward(ctx, grad_dist, grad_idx):
        return ()


three_nn = ThreeNN.apply


class ThreeInterpolate(Function):
    @staticmethod
    def forward(ctx, features, idx, weight):
        """features (B,c,m), idx (B,n,3) int32, weight (B,n,3) -> (B,c,n) (pointnet2_utils.py:139-191)."""
        ctx.save_for_backward(idx, weight, features)
        B, c, m = features.shape
        n = idx.shape[1]
        out = torch.empty((B, c, n), dtype=torch.float32, device=features.device)
        with on_device(features):
            check(lib().nsdp_three_interpolate(fptr(features, "features"), iptr(idx, "idx"), fptr(weight, "weight"),
                                               _c_int(B), _c_int(c), _c_int(m), _c_int(n), fptr(out),
                                               stream_ptr()), "nsdp_three_interpolate")
        return out

    @staticmethod
    def backward(ctx, grad_out):
        idx, weight, features = ctx.saved_tensors
        B, c, m = features.shape
        n = idx.shape[1]
        grad_out = grad_out.contiguous()
        grad = torch.empty((B, c, m), dtype=torch.float32, device=grad_out.device)
        L = lib()
        if (_SCATTER_INVERSE and 3 * n <= 64 * m
                and L.nsdp_three_interpolate_grad_lists_supported(_c_int(B), _c_int(c), _c_int(n), _c_int(m))):
            # through the inverse lists of the 3-NN index map (cached on the index tensor): no atomics, deterministic
            from . import hip_attention
            offsets, entries = hip_attention.inverse_lists(idx, m)
            with on_device(grad_out):
                check(L.nsdp_three_interpolate_grad_lists(fptr(grad_out, "grad_out"), fptr(weight, "weight"), iptr(offsets),
                                                          iptr(entries), _c_int(B), _c_int(c), _c_int(n), _c_int(m), fptr(grad),
                                                          stream_ptr()), "nsdp_three_interpolate_grad_lists")
            return grad, torch.zeros_like(idx), torch.zeros_like(weight)
        with on_device(grad_out):
            check(lib().nsdp_three_interpolate_grad(fptr(grad_out, "grad_out"), iptr(idx), fptr(weight), _c_int(B),
                                                    _c_int(c), _c_int(n), _c_int(m), fptr(grad), stream_ptr()),
                  "nsdp_three_interpolate_grad")
        return grad, torch.zeros_like(idx), torch.zeros_like(weight)


three_interpolate = ThreeInterpolate.apply


class GroupingOperation(Function):
    @staticmethod
    def forward(ctx, features, idx):
        """features (B,C,N), idx (B,npoint,nsample) int32 -> (B,C,npoint,nsample)
        (pointnet2_utils.py:194-240)."""
        ctx.save_for_backward(idx, features)
        B, C, N = features.shape
        _, NP, NS = idx.shape
        out = torch.empty((B, C, NP, NS), dtype=torch.float32, device=features.device)
        with on_device(features):
            check(lib().nsdp_group_points(fptr(features, "features"), iptr(idx, "idx"), _c_int(B), _c_int(C),
                                          _c_int(N), _c_int(NP), _c_int(NS), fptr(out), stream_ptr()),
                  "nsdp_group_points")
        return out

    @staticmethod
    def backward(ctx, grad_out):
        idx, features = ctx.saved_tensors
        B, C, N = features.shape
        _, NP, NS = idx.shape
        grad_out = grad_out.contiguous()
        grad = _scatter_cm(grad_out.view(B, C, NP * NS), idx.view(B, NP * NS), N, idx_obj=idx)
        if grad is not None:
            return grad, torch.zeros_like(idx)
        grad = torch.empty((B, C, N), dtype=torch.float32, device=grad_out.device)
        with on_device(grad_out):
            check(lib().nsdp_group_points_grad(fptr(grad_out, "grad_out"), iptr(idx), _c_int(B), _c_int(C),
                                               _c_int(N), _c_int(NP), _c_int(NS), fptr(grad), stream_ptr()),
                  "nsdp_group_points_grad")
        return grad, torch.zeros_like(idx)


grouping_operation = GroupingOperation.apply


class BallQuery(Function):
    @staticmethod
    def forward(ctx, radius, nsample, xyz, new_xyz):
        """xyz (B,N,3), new_xyz (B,npoint,3) -> (B,npoint,nsample) int32 (pointnet2_utils.py:243-276)."""
        B, N, _ = xyz.shape
        M = new_xyz.shape[1]
        out = torch.empty((B, M, int(nsample)), dtype=torch.int32, device=xyz.device)
        with on_device(xyz):
            check(lib().nsdp_ball_query(fptr(new_xyz, "new_xyz"), fptr(xyz, "xyz"), _c_int(B), _c_int(N), _c_int(M),
                                        ctypes.c_float(float(radius)), _c_int(int(nsample)), iptr(out),
                                        stream_ptr()), "nsdp_ball_query")
        ctx.mark_non_differentiable(out)
        return out

    @staticmethod
    def backward(ctx, grad_out):
        return ()


ball_query = BallQuery.apply


def _with_xyz(local_xyz, feats, use_xyz):
    """Channel layout shared by both groupers: relative/absolute coordinates first, then the descriptors."""
    if feats is None:
        return local_xyz
    return torch.cat((local_xyz, feats), dim=1) if use_xyz else feats


class QueryAndGroup(nn.Module):
    """Ball query around each centre, then the members' coordinates (relative to the centre) and descriptors as one
    (B, 3 + C, npoint, nsample) tensor (same contract as pointnet2_utils.py:279-335)."""

    def __init__(self, radius, nsample, use_xyz=True):
        super().__init__()
        self.radius, self.nsample, self.use_xyz = radius, nsample, use_xyz

    def forward(self, xyz, new_xyz, features=None):
        if features is None and not self.use_xyz:
            raise AssertionError("QueryAndGroup: without descriptors the coordinates are the only features "
                                 "(use_xyz=False leaves nothing to return)")
        members = ball_query(self.radius, self.nsample, xyz, new_xyz)                  # (B, npoint, nsample) int32
        centres = new_xyz.permute(0, 2, 1)[:, :, :, None]                               # (B, 3, npoint, 1)
        local = grouping_operation(xyz.permute(0, 2, 1).contiguous(), members) - centres
        picked = grouping_operation(features, members) if features is not None else None
        return _with_xyz(local, picked, self.use_xyz)


class GroupAll(nn.Module):
    """One group holding every point: (B, 3 + C, 1, N); ``new_xyz`` is ignored (pointnet2_utils.py:338-379)."""

    def __init__(self, use_xyz=True):
        super().__init__()
        self.use_xyz = use_xyz

    def forward(self, xyz, new_xyz, features=None):
        everything = xyz.permute(0, 2, 1)[:, :, None, :]                                # (B, 3, 1, N), absolute
        return _with_xyz(everything, None if features is None else features[:, :, None, :], self.use_xyz)
