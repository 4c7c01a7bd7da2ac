"""Farthest-point sampling of large clouds: the workgroup cluster (include/nsdp_sampling.h) against the one-workgroup entry of
nsdp_hip.h, in one process on one GPU.

    python tools/bench_fps.py [--reps 7] [--samples 500]

For N in {8193, 12000, 25000, 50000, 100000, 200000} x B in {1, 4}, and one packed set, both entries are timed with HIP events
in interleaved repetitions (old, cluster, old, cluster, ...); each line gives both medians, each side's min-max, whether the
index sets are equal and the cluster's status word (0: no wait gave up).  The last line names the range of N over which the
cluster's median is below the old kernel's by more than the two min-max spreads together: the dispatch's default range.
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

SIZES = (8193, 12000, 25000, 50000, 100000, 200000)
RAGGED = (25000, 9000, 40000, 12000)


def _time(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), out


def _ab(old, new, reps):
    """Interleaved repetitions after one untimed pass of each -> (stats of old, stats of new, equal, status)."""
    want, got = old(), new()
    status = pu.fps_cluster_status()
    torch.cuda.synchronize()
    equal = bool(torch.equal(want, got))
    t_old, t_new = [], []
    for _ in range(reps):
        t_old.append(_time(old)[0])
        ms, got = _time(new)
        t_new.append(ms)
        equal = equal and bool(torch.equal(want, got))
        status = status or pu.fps_cluster_status()
    return t_old, t_new, equal, status


def _line(what, t_old, t_new, equal, status):
    mo, mn = statistics.median(t_old), statistics.median(t_new)
    spread = (max(t_old) - min(t_old)) + (max(t_new) - min(t_new))
    rec = dict(what, old_ms=round(mo, 4), old_min=round(min(t_old), 4), old_max=round(max(t_old), 4), cluster_ms=round(mn, 4),
               cluster_min=round(min(t_new), 4), cluster_max=round(max(t_new), 4), speedup=round(mo / mn, 2),
               wins=bool(mo - mn > spread), equal=equal, status=status)
    print(json.dumps(rec), flush=True)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--samples", type=int, default=500)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    g = torch.Generator().manual_seed(0)
    m, recs = args.samples, []
    for B in (1, 4):
        for N in SIZES:
            xyz = (torch.rand(B, N, 3, generator=g) - 0.5).to(dev)

            def old():
                with pu.fps_cluster(False):
                    return pu.furthest_point_sample(xyz, m)
            recs.append(_line({"B": B, "N": N, "m": m, "groups": pu.fps_cluster_groups(N)},
                              *_ab(old, lambda: pu.furthest_point_sample_cluster(xyz, m), args.reps)))
    r = RaggedPoints.from_list([(torch.rand(n, 3, generator=g) - 0.5).to(dev) for n in RAGGED])

    def old_ragged():
        with pu.fps_cluster(False):
            return pu.furthest_point_sample_ragged(r.packed, r.offsets, m, max(RAGGED))

    def new_ragged():
        with pu.fps_cluster(True):
            return pu.furthest_point_sample_ragged(r.packed, r.offsets, m, max(RAGGED), groups=pu.fps_cluster_groups(max(RAGGED)))
    _line({"ragged": list(RAGGED), "m": m, "groups": pu.fps_cluster_groups(max(RAGGED))}, *_ab(old_ragged, new_ragged, args.reps))
    ok = all(x["equal"] and x["status"] == 0 for x in recs)
    winning = sorted({x["N"] for x in recs if all(y["wins"] for y in recs if y["N"] == x["N"])})
    tail = [n for n in SIZES if all(k in winning for k in SIZES if k >= n)]
    print(json.dumps({"indices_equal_and_status_clean": ok, "cluster_wins_at": winning,
                      "default_range_starts_at": tail[0] if tail else None}), flush=True)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
