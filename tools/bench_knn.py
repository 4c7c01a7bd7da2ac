"""k-nearest-neighbour search of large clouds: the cell grid (include/nsdp_search.h) against the exhaustive scan of nsdp_hip.h,
in one process on one GPU.

    python tools/bench_knn.py [--reps 7] [--k 16] [--sizes 5000,8193,...]

Self-searches of sphere surfaces of N points (B = 1), the 500-centre search against the same clouds, one packed set and the
training shape 32 x 2048 (for information) are timed with HIP events in interleaved repetitions (scan, grid, scan, grid, ...)
after one untimed pass of each; each line gives both medians, each side's min-max, whether indices and distance bits are equal
and what the grid did (distance tests per query, queries finished by the plain scan).  The last line names the smallest N from
which the grid's median is below the scan's by more than the two min-max spreads together (KNN_GRID_MIN_POINTS) and whether the
500-centre searches win (KNN_GRID_MIN_TESTS).
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from nsdp_amd import pointnet2_utils as pu            # noqa: E402
from nsdp_amd.ragged import RaggedPoints              # noqa: E402

SIZES = (5000, 8193, 25000, 50000, 100000, 200000)
RAGGED = (25000, 9000, 40000, 12000)
CENTRES = 500


def _time(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), out


def _equal(want, got):
    return bool(torch.equal(want[0], got[0])) and bool(torch.equal(want[1].view(torch.int32), got[1].view(torch.int32)))


def _ab(scan, grid, reps):
    """Interleaved repetitions after one untimed pass of each -> (times of the scan, of the grid, equal, the grid's stats)."""
    want, got = scan(), grid()
    stats = pu.knn_grid_stats()
    equal = _equal(want, got)
    t_scan, t_grid = [], []
    for _ in range(reps):
        t_scan.append(_time(scan)[0])
        ms, got = _time(grid)
        t_grid.append(ms)
        equal = equal and _equal(want, got)
    return t_scan, t_grid, equal, stats


def _line(what, t_scan, t_grid, equal, stats):
    ms, mg = statistics.median(t_scan), statistics.median(t_grid)
    spread = (max(t_scan) - min(t_scan)) + (max(t_grid) - min(t_grid))
    rec = dict(what, scan_ms=round(ms, 4), scan_min=round(min(t_scan), 4), scan_max=round(max(t_scan), 4), grid_ms=round(mg, 4),
               grid_min=round(min(t_grid), 4), grid_max=round(max(t_grid), 4), speedup=round(ms / mg, 2), wins=bool(ms - mg > spread),
               equal=equal, tests_per_query=round(stats["tests"] / max(stats["queries"], 1), 1), scanned=stats["scanned"],
               cells=stats["cells"])
    print(json.dumps(rec), flush=True)
    return rec


def _sphere(n, g):
    v = torch.randn(n, 3, generator=g)
    return (0.5 * v / v.norm(dim=1, keepdim=True)).contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--k", type=int, default=16)
    ap.add_argument("--sizes", type=lambda s: tuple(int(x) for x in s.split(",")), default=SIZES)
    args = ap.parse_args()
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
    ok = all(x["equal"] for x in selfs + centres + [packed, info])
    tail = [x["N"] for i, x in enumerate(selfs) if all(y["wins"] for y in selfs[i:])]
    print(json.dumps({"bits_equal": ok, "grid_wins_from_N": tail[0] if tail else None,
                      "centres_win_at": [x["N"] for x in centres if x["wins"]]}), flush=True)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
