"""Inverse neighbour lists of large clouds: the many-workgroup build (include/nsdp_scatter.h) and the segment sums over it against
the fp32-atomic kernels that clouds above 8192 points took before, in one process on one GPU.

    python tools/bench_invert.py [--reps 7] [--k 16] [--d 120] [--sizes 8193,25000,...] [--batches 1,4] [--train] [--train-only]

For every B, N = n and each of three inputs -- the k-NN index set of a sphere surface, of a clustered surface (9 % of the points
over the sphere, the rest on its cap), and the all-duplicate cloud (every query's neighbours are rows 0 .. k-1: k lists of n
entries, the worst case of count, fill and the long lists) -- one JSON line with the medians and min-max in ms per pass, HIP
events around windows of several passes (`passes_per_window` backward passes, four times as many builds), interleaved
repetitions (build, lists, atomics, build, ...) after one untimed pass of each:

    build_ms        one list build (torch's allocations of offsets, entries and the workspace inside the window);
    bwd_lists_ms    the backward pass of ONE attention block -- `attn_pre` + `attn_post` with a value table and a residual, as
                    tests/test_invert_wide_gpu.py composes them, `torch.autograd.grad` of a weighted sum -- with the knob at 1:
                    everything the real backward runs, the dq pass over du and ONE build of the lists included (the cache on the
                    index tensor is dropped before every pass);
    bwd_atomic_ms   the same call with NSDP_INVERT_WIDE=0: what a cloud above 8192 points took before, d(vf) by the atomics
                    inside nsdp_attn_post_bwd and d(kf) by those inside nsdp_attn_pre_bwd;
    max_err         the largest difference of the two sets of gradients over (the largest magnitude + 1); `same_bits_twice`: the
                    gradients of two passes with lists are equal bit for bit.

Both sides share the same forward graph and the same elementwise glue; the windows hold enqueue from Python, as a step does.

Then `force` against the one-workgroup entry at N in {2048, 8192}, B in {1, 32}: old_ms / wide_ms per build (windows of 20
builds), and whether the lists are equal.  The last line sums up.

--train: end to end, `python -m nsdp_amd.train CONFIG DIR --surface 25000 --queries 25000 --batch 1` as child processes with the
knob at 1 and at 0, order alternated (1, 0, 0, 1), each at 2 and at 52 epochs of --synthetic 4 (no validation, no checkpoint):
wall seconds, and the difference over the 200 extra train steps as ms per step -- process start, model build and first-call
costs cancel.
"""
import argparse
import json
import math
import os
import statistics
import subprocess
import sys
import tempfile
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from nsdp_amd import hip_attention as ha, pointnet2_utils as pu      # noqa: E402
from nsdp_amd.config import default_config                           # noqa: E402

SIZES = (8193, 25000, 100000, 200000)
BATCHES = (1, 4)
BOUNDARY = ((1, 2048), (32, 2048), (1, 8192), (32, 8192))
BUILDS = 20                  # list builds per timed window of the boundary comparison
INNER = 5                    # backward passes per timed window (1 for the all-duplicate cloud, whose pass takes tens of ms)
SHORT, LONG = 2, 52          # epochs of the two end-to-end train runs per knob value: their difference is 200 steps


def _time(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), out


def _stats(ts):
    return round(statistics.median(ts), 4), round(min(ts), 4), round(max(ts), 4)


def _sphere(n, g):
    v = torch.randn(n, 3, generator=g)
    return (0.5 * v / v.norm(dim=1, keepdim=True)).contiguous()


def _cap(n, g, z0=0.4975):
    z = z0 + (0.5 - z0) * torch.rand(n, generator=g)
    phi = 2.0 * math.pi * torch.rand(n, generator=g)
    r = (0.25 - z * z).clamp_min(0.0).sqrt()
    return torch.stack([r * phi.cos(), r * phi.sin(), z], 1).contiguous()


def _fresh(idx):
    """The index tensor without its cached lists: every timed build is a build."""
    idx.__dict__.pop("_nsdp_inverse", None)
    return idx


def _build(idx, N, mode):
    with ha.invert_wide_mode(mode):
        return ha.inverse_lists(_fresh(idx), N)


def _block(B, n, N, k, d, dev):
    """The operands of one attention block (per-point queries, value table, residual), as tests/test_invert_wide_gpu.py runs it."""
    mk = lambda *s: torch.randn(*s, device=dev)      # (the device's generator, seeded in main: 6 GB a tensor at the largest size)
    t = dict(q=mk(B, n, d), kf=mk(B, N, d), vf=mk(B, N, d), pos=mk(B, n, k, d), res=mk(B, n, d))
    return {kk: v.requires_grad_(True) for kk, v in t.items()}, mk(B, n, d)


def _forward(t, w, idx, mode):
    with ha.invert_wide_mode(mode):
        u = ha.attn_pre(t["q"], t["kf"], t["pos"], idx, None)
        y = ha.attn_post(u * 0.5, t["vf"], t["pos"], idx, residual=t["res"])
        return (y * w).sum()


def _backward(loss, t, idx, mode, inner):
    """``inner`` backward passes of the block in one timed window.  With lists every pass builds them anew (the cache on the index
    tensor is dropped first): attn_post's backward builds, attn_pre's reuses -- one build per block, where the model shares one
    build between the two attentions of a set abstraction."""
    with ha.invert_wide_mode(mode):
        for _ in range(inner):
            _fresh(idx)
            grads = torch.autograd.grad(loss, list(t.values()), retain_graph=True)
    return grads


def _case(name, idx, N, d, reps, inner, dev):
    B, n, k = idx.shape
    wide = "1" if N > 8192 else "force"
    t, w = _block(B, n, N, k, d, dev)
    loss_l = loss_a = _forward(t, w, idx, wide)      # (one graph for both: the forward is the same kernels under either knob)
    first, second = _backward(loss_l, t, idx, wide, 1), _backward(loss_l, t, idx, wide, 1)
    atomic = _backward(loss_a, t, idx, "0", 1)
    for _ in range(inner):
        _build(idx, N, wide)
    same = all(bool(torch.equal(x, y)) for x, y in zip(first, second))
    err = max(float((x - y).abs().max()) / (float(y.abs().max()) + 1.0) for x, y in zip(first, atomic))
    del first, second, atomic
    tb, tl, ta = [], [], []
    for _ in range(reps):
        tb.append(_time(lambda: [_build(idx, N, wide) for _ in range(4 * inner)])[0] / (4 * inner))
        tl.append(_time(lambda: _backward(loss_l, t, idx, wide, inner))[0] / inner)
        ta.append(_time(lambda: _backward(loss_a, t, idx, "0", inner))[0] / inner)
    off, _ = _build(idx, N, wide)
    longest = int((off[:, 1:] - off[:, :-1]).max())
    rec = {"case": name, "B": B, "N": N, "k": k, "d": d, "longest_list": longest, "passes_per_window": inner}
    for key, ts in (("build", tb), ("bwd_lists", tl), ("bwd_atomic", ta)):
        rec[key + "_ms"], rec[key + "_min"], rec[key + "_max"] = _stats(ts)
    rec.update(atomic_over_lists=round(rec["bwd_atomic_ms"] / rec["bwd_lists_ms"], 2), same_bits_twice=same, max_err=float(f"{err:.3g}"))
    print(json.dumps(rec), flush=True)
    return rec


def _boundary(B, N, k, reps, g, dev):
    idx = pu.knn(*(2 * [torch.stack([_sphere(N, g) for _ in range(B)]).to(dev)]), k)
    old, new = _build(idx, N, "0"), _build(idx, N, "force")
    equal = bool(torch.equal(old[0], new[0])) and bool(torch.equal(old[1], new[1]))
    to, tw = [], []
    for _ in range(reps):
        to.append(_time(lambda: [_build(idx, N, "0") for _ in range(BUILDS)])[0] / BUILDS)
        tw.append(_time(lambda: [_build(idx, N, "force") for _ in range(BUILDS)])[0] / BUILDS)
    rec = {"case": "boundary: force against the one-workgroup entry", "B": B, "N": N, "k": k, "equal": equal}
    rec["old_ms"], rec["old_min"], rec["old_max"] = _stats(to)
    rec["wide_ms"], rec["wide_min"], rec["wide_max"] = _stats(tw)
    rec["wide_wins"] = bool(rec["old_ms"] - rec["wide_ms"] > (max(to) - min(to)) + (max(tw) - min(tw)))
    print(json.dumps(rec), flush=True)
    return rec


def _train(surface=25000, queries=25000, synthetic=4):
    import yaml
    out = []
    with tempfile.TemporaryDirectory() as tmp:
        cfg = os.path.join(tmp, "forward.yaml")
        with open(cfg, "w") as f:
            cfg_dict = dict(default_config("forward"), validation={"frequency": 10 ** 6})      # (no validation, no checkpoint)
            cfg_dict["training"]["save_frequency"] = 10 ** 6
            yaml.safe_dump(cfg_dict, f)
        for epochs, order in ((SHORT, ("1", "0")), (LONG, ("0", "1"))):
            for knob in order:
                env = dict(os.environ, NSDP_INVERT_WIDE=knob)
                cmd = [sys.executable, "-m", "nsdp_amd.train", cfg, os.path.join(tmp, f"exp_{knob}_{epochs}"), "--surface", str(surface),
                       "--queries", str(queries), "--batch", "1", "--synthetic", str(synthetic), "--epochs", str(epochs)]
                t0 = time.perf_counter()
                try:
                    p = subprocess.run(cmd, cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
                except subprocess.TimeoutExpired as e:      # (run() has killed the child; nothing more is started on the device)
                    print(json.dumps({"case": "train CLI", "NSDP_INVERT_WIDE": knob, "epochs": epochs, "rc": "timeout"}), flush=True)
                    print((e.stdout or "")[-4000:] if isinstance(e.stdout, str) else (e.stdout or b"").decode(errors="replace")[-4000:],
                          flush=True)
                    return out, False
                wall = time.perf_counter() - t0
                rec = {"case": "train CLI", "NSDP_INVERT_WIDE": knob, "surface": surface, "queries": queries, "batch": 1,
                       "epochs": epochs, "synthetic": synthetic, "rc": p.returncode, "wall_s": round(wall, 2),
                       "last_line": (p.stdout.strip().splitlines() or [""])[-1][:160]}
                print(json.dumps(rec), flush=True)
                out.append(rec)
                if p.returncode != 0:      # a Python exception (1: a HIP error arrives as one), a crash: nothing more is started
                    print("\n".join(p.stdout.strip().splitlines()[-40:]), flush=True)
                    return out, False
    for knob in ("1", "0"):
        runs = {r["epochs"]: r for r in out if r["NSDP_INVERT_WIDE"] == knob and r["rc"] == 0}
        if len(runs) == 2:
            steps = (LONG - SHORT) * synthetic
            print(json.dumps({"case": "train CLI, per step", "NSDP_INVERT_WIDE": knob,
                              "ms_per_train_step": round(1e3 * (runs[LONG]["wall_s"] - runs[SHORT]["wall_s"]) / steps, 2),
                              "steps": steps}), flush=True)
    return out, True


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--k", type=int, default=16)
    ap.add_argument("--d", type=int, default=default_config()["model"]["encoder_kwargs"]["d_reduced"])
    ap.add_argument("--sizes", type=lambda s: tuple(int(x) for x in s.split(",")), default=SIZES)
    ap.add_argument("--batches", type=lambda s: tuple(int(x) for x in s.split(",")), default=BATCHES)
    ap.add_argument("--train", action="store_true", help="also the end-to-end train runs (child processes)")
    ap.add_argument("--train-only", action="store_true")
    args = ap.parse_args()
    if args.train_only:
        return 0 if _train()[1] else 1
    dev = torch.device("cuda", 0)
    g = torch.Generator().manual_seed(0)
    torch.manual_seed(0)
    k, recs = args.k, []
    for N in args.sizes:
        for B in args.batches:
            sphere = torch.stack([_sphere(N, g) for _ in range(B)]).to(dev)
            clustered = torch.stack([torch.cat([_sphere(N * 9 // 100, g), _cap(N - N * 9 // 100, g)]) for _ in range(B)]).to(dev)
            dup = torch.arange(k, dtype=torch.int32, device=dev).repeat(B, N, 1).contiguous()
            for name, idx in (("sphere", pu.knn(sphere, sphere, k)), ("clustered", pu.knn(clustered, clustered, k)),
                              ("all-duplicate", dup)):
                recs.append(_case(name, idx, N, args.d, args.reps, 1 if name == "all-duplicate" else INNER, dev))
                torch.cuda.empty_cache()
    bounds = [_boundary(B, N, k, args.reps, g, dev) for B, N in BOUNDARY]
    ok = all(r["same_bits_twice"] for r in recs) and all(b["equal"] for b in bounds)
    print(json.dumps({"same_bits_twice_everywhere": ok,
                      "lists_slower_than_atomics_at": [(r["case"], r["B"], r["N"]) for r in recs if r["atomic_over_lists"] < 1.0],
                      "wide_wins_below_the_boundary_at": [(b["B"], b["N"]) for b in bounds if b["wide_wins"]]}), flush=True)
    if args.train:
        ok = _train()[1] and ok
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
