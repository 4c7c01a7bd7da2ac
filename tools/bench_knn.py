"""k-nearest-neighbour search of large clouds: the cell grid (include/nsdp_search.h) against the exhaustive scan of nsdp_hip.h,
in one process on one GPU.

    python tools/bench_knn.py [--reps 7] [--k 16] [--sizes 5000,8193,...] [--against other/libnsdp_hip.so]

Self-searches of sphere surfaces of N points (B = 1), the 500-centre search against the same clouds, one packed set and the
training shape 32 x 2048 (for information) are timed with HIP events in interleaved repetitions (scan, grid, scan, grid, ...)
after one untimed pass of each; each line gives both medians, each side's min-max, whether indices and distance bits are equal
and what the grid did (distance tests per query, queries finished by the plain scan).  The last line names the smallest N from
which the grid's median is below the scan's by more than the two min-max spreads together (KNN_GRID_MIN_POINTS) and whether the
500-centre searches win (KNN_GRID_MIN_TESTS).

Away from centred surfaces ("anywhere", ANYWHERE points each): the sphere translated by (2000, -1500, 900), a uniform cube, a
clustered surface (9 % of the points over the sphere, the rest on its cap z > 0.4975), 500 queries far outside the box and 500
on the sphere of radius 3 around the radius-0.5 cloud, which all end in the exhaustive finish.  Same interleaving, same "wins"
rule.

--against LIB loads a second build of the library (the A/B partner, e.g. the parent commit's) into the same process and times
ITS grid as a third member of every repetition (scan, grid, other, scan, ...): other_ms / other_min / other_max, what it did
(other_tests_per_query, other_scanned), and "not_slower": this build's median does not exceed the other's by more than the two
min-max spreads together.
"""
import argparse
import contextlib
import ctypes
import json
import math
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from nsdp_amd import _lib, pointnet2_utils as pu      # noqa: E402
from nsdp_amd.ragged import RaggedPoints              # noqa: E402

SIZES = (5000, 8193, 25000, 50000, 100000, 200000)
RAGGED = (25000, 9000, 40000, 12000)
CENTRES = 500
ANYWHERE = 100000
OTHER = None            # --against: the other build's handle


def _time(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), out


def _equal(want, got):
    return bool(torch.equal(want[0], got[0])) and bool(torch.equal(want[1].view(torch.int32), got[1].view(torch.int32)))


@contextlib.contextmanager
def _other_lib():
    """Inside the block the wrappers call the --against build.  This swaps the module's private handle, so it relies on two
    things: the wrappers fetch the handle through _lib.lib() at every call and cache none, and they pass every argument as an
    explicit ctypes value and set a restype other than int (nsdp_knn_grid_workspace_bytes) on the handle they have just
    fetched, so that nothing set on the first handle is missing on the second; nsdp_last_error's restype, which _lib sets once
    when it loads, is set again where OTHER is loaded.  A wrapper that declared argtypes at import would break this."""
    mine = _lib.lib()
    _lib._lib = OTHER
    try:
        yield
    finally:
        _lib._lib = mine


def _ab(scan, grid, reps):
    """Interleaved repetitions after one untimed pass of each -> (times of the scan, of the grid, equal, the grid's stats, and
    with --against the other build's times and stats)."""
    def other():
        with _other_lib():
            out = grid()
            return out, pu.knn_grid_stats()
    want, got = scan(), grid()
    stats = pu.knn_grid_stats()
    equal = _equal(want, got)
    t_scan, t_grid, t_other, other_stats = [], [], [], None
    if OTHER is not None:
        got, other_stats = other()
        equal = equal and _equal(want, got)
    for _ in range(reps):
        t_scan.append(_time(scan)[0])
        ms, got = _time(grid)
        t_grid.append(ms)
        equal = equal and _equal(want, got)
        if OTHER is not None:
            with _other_lib():
                ms, got = _time(grid)
            t_other.append(ms)
            equal = equal and _equal(want, got)
    return t_scan, t_grid, equal, stats, t_other, other_stats


def _line(what, t_scan, t_grid, equal, stats, t_other=(), other_stats=None):
    ms, mg = statistics.median(t_scan), statistics.median(t_grid)
    spread = (max(t_scan) - min(t_scan)) + (max(t_grid) - min(t_grid))
    rec = dict(what, scan_ms=round(ms, 4), scan_min=round(min(t_scan), 4), scan_max=round(max(t_scan), 4), grid_ms=round(mg, 4),
               grid_min=round(min(t_grid), 4), grid_max=round(max(t_grid), 4), speedup=round(ms / mg, 2), wins=bool(ms - mg > spread),
               equal=equal, tests_per_query=round(stats["tests"] / max(stats["queries"], 1), 1), scanned=stats["scanned"],
               cells=stats["cells"])
    if t_other:
        mo = statistics.median(t_other)
        both = (max(t_other) - min(t_other)) + (max(t_grid) - min(t_grid))
        rec.update(other_ms=round(mo, 4), other_min=round(min(t_other), 4), other_max=round(max(t_other), 4),
                   other_over_grid=round(mo / mg, 2), not_slower=bool(mg - mo <= both),
                   other_tests_per_query=round(other_stats["tests"] / max(other_stats["queries"], 1), 1),
                   other_scanned=other_stats["scanned"])
    print(json.dumps(rec), flush=True)
    return rec


def _sphere(n, g):
    v = torch.randn(n, 3, generator=g)
    return (0.5 * v / v.norm(dim=1, keepdim=True)).contiguous()


def _cap(n, g, z0=0.4975):
    """n points uniform over the cap z > z0 of the radius-0.5 sphere (a sphere's area is uniform in z)."""
    z = z0 + (0.5 - z0) * torch.rand(n, generator=g)
    phi = 2.0 * math.pi * torch.rand(n, generator=g)
    r = (0.25 - z * z).clamp_min(0.0).sqrt()
    return torch.stack([r * phi.cos(), r * phi.sin(), z], 1).contiguous()


def main():
    global OTHER
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--k", type=int, default=16)
    ap.add_argument("--sizes", type=lambda s: tuple(int(x) for x in s.split(",")), default=SIZES)
    ap.add_argument("--against", default=None, help="another build of libnsdp_hip.so: its grid is timed beside this one's")
    args = ap.parse_args()
    if args.against:
        OTHER = ctypes.CDLL(os.path.abspath(args.against))
        OTHER.nsdp_last_error.restype = ctypes.c_char_p
    dev = torch.device("cuda", 0)
    g = torch.Generator().manual_seed(0)
    k, selfs, centres = args.k, [], []

    def pair(q, s):
        def scan():
            with pu.knn_grid_mode("0"):
                return pu.knn(q, s, k, return_dist=True)
        return scan, (lambda: pu.knn_grid(q, s, k, return_dist=True))

    for N in args.sizes:
        xyz = _sphere(N, g)[None].to(dev)
        selfs.append(_line({"case": "self", "N": N, "k": k}, *_ab(*pair(xyz, xyz), args.reps)))
        q = xyz[:, torch.randperm(N, generator=g)[:CENTRES]].contiguous()
        centres.append(_line({"case": "centres", "n": CENTRES, "N": N, "k": k}, *_ab(*pair(q, xyz), args.reps)))
    r = RaggedPoints.from_list([_sphere(n, g).to(dev) for n in RAGGED])

    def scan_ragged():
        with pu.knn_grid_mode("0"):
            return pu.knn_ragged_source(r.packed, r.packed, r.offsets, k, max(RAGGED), query_offsets=r.offsets, return_dist=True)

    def grid_ragged():
        return pu.knn_grid_ragged_source(r.packed, r.packed, r.offsets, k, max(RAGGED), query_offsets=r.offsets, return_dist=True)
    packed = _line({"case": "packed self", "counts": list(RAGGED), "k": k}, *_ab(scan_ragged, grid_ragged, args.reps))
    train = torch.stack([_sphere(2048, g) for _ in range(32)]).to(dev)
    info = _line({"case": "training shape (information only)", "B": 32, "N": 2048, "k": k}, *_ab(*pair(train, train), args.reps))
    N, shift = ANYWHERE, torch.tensor([2000.0, -1500.0, 900.0])
    ball = _sphere(N, g)
    moved, cube = (ball + shift)[None].to(dev), (torch.rand(N, 3, generator=g) - 0.5)[None].to(dev)
    clustered = torch.cat([_sphere(N * 9 // 100, g), _cap(N - N * 9 // 100, g)])[None].to(dev)
    far, near = (50.0 * torch.randn(1, CENTRES, 3, generator=g)).to(dev), (6.0 * _sphere(CENTRES, g))[None].to(dev)
    ball = ball[None].to(dev)
    anywhere = [_line({"case": "anywhere: centred sphere (the partner of the next line)", "N": N, "k": k}, *_ab(*pair(ball, ball), args.reps)),
                _line({"case": "anywhere: sphere translated by (2000, -1500, 900)", "N": N, "k": k}, *_ab(*pair(moved, moved), args.reps)),
                _line({"case": "anywhere: uniform cube", "N": N, "k": k}, *_ab(*pair(cube, cube), args.reps)),
                _line({"case": "anywhere: clustered surface", "N": N, "k": k}, *_ab(*pair(clustered, clustered), args.reps)),
                _line({"case": "anywhere: queries far outside the box (all finish)", "n": CENTRES, "N": N, "k": k},
                      *_ab(*pair(far, ball), args.reps)),
                _line({"case": "anywhere: queries on the sphere of radius 3 (1.2 to 2.5 extents outside the box, no budget)",
                       "n": CENTRES, "N": N, "k": k}, *_ab(*pair(near, ball), args.reps))]
    same_time = abs(anywhere[1]["grid_ms"] - anywhere[0]["grid_ms"]) <= sum(x["grid_max"] - x["grid_min"] for x in anywhere[:2])
    ok = all(x["equal"] for x in selfs + centres + [packed, info] + anywhere)
    tail = [x["N"] for i, x in enumerate(selfs) if all(y["wins"] for y in selfs[i:])]
    print(json.dumps({"bits_equal": ok, "grid_wins_from_N": tail[0] if tail else None,
                      "centres_win_at": [x["N"] for x in centres if x["wins"]],
                      "translated_within_spreads_of_centred": bool(same_time)}), flush=True)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
