"""The local-rigidity training regulariser (nsdp_amd/rigidity.py) against its composition, in one process on one GPU.

    python tools/bench_rigidity.py [--reps 7] [--shapes 32x8192,4x100000] [--k 8] [--streams 2,1,3] [--no-train] [--train-only]

For every shape B x n: one JSON line for the self-search on its own (``neighbour_sets(source, k)``: knn with k + 1 columns, the
cell grid for large clouds), then, for each of two sources -- a cloud in general position in the unit cube, and a cloud with
duplicate hubs (an eighth of the rows copies of one point, another eighth eight groups of copies: the lowest-index copies are
named by every copy, in-degrees of n / 8 and n / 64) -- one JSON line with the median and min-max in ms of loss forward +
backward on neighbour sets that are given (both partners build their inverse lists in every pass, as a train step does: no
list cache is hit), HIP events around windows of several passes enqueued from Python, interleaved
repetitions (native, composed, native, ...) after one untimed pass of each:

    native_ms     local_rigidity_loss: one forward call, the list build, one backward launch;
    composed_ms   rigidity.composed_loss: index_points through autograd twice, elementwise torch;
    same_bits_twice: the native loss and gradient of two passes are equal bit for bit; max_err: the native gradient's largest
                  difference from the composed one over the gradient's largest magnitude; max_in_degree: the longest list.

Then the replayed train step (forward model, l2 data term, B = 32, 2048 surface samples, 8192 queries; GraphedStep on two
streams, on one and on three) with ``training.rigidity = {weight: 1, k}`` against the step without the key: ms per replay,
interleaved windows, the kernels of either graph, and (``rigidity_kernels_in_replay``) launches and total ms of the self-search,
the loss's own kernels and the list build as they run inside one replay.
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from nsdp_amd import rigidity, synth                                 # noqa: E402
from nsdp_amd.config import default_config                          # noqa: E402

SHAPES = ((32, 8192), (4, 100000))
N_SURF, N_QUERY, TRAIN_BATCH = 2048, 8192, 32


def _time(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), out


def _stats(ts):
    return round(statistics.median(ts), 4), round(min(ts), 4), round(max(ts), 4)


def _pass(loss_fn, pred, source, idx):
    # a fresh view of the index tensor: hip_attention.inverse_lists caches the lists on the tensor object it is given, which the
    # composed partner's scatter would hit from the second pass on.  A train step searches new neighbour sets every step, so
    # both partners build their lists in every pass here.
    pred.grad = None
    loss = loss_fn(pred, source, idx.view(idx.shape))
    loss.backward()
    return loss.detach(), pred.grad


def _native(pred, source, idx):
    return rigidity.local_rigidity_loss(pred, source, idx=idx)


def _composed(pred, source, idx):
    return rigidity.composed_loss(pred, source, idx)


def _search(source, k, reps, inner):
    B, n = source.shape[0], source.shape[1]
    rigidity.neighbour_sets(source, k)
    times = [_time(lambda: [rigidity.neighbour_sets(source, k) for _ in range(inner)])[0] / inner for _ in range(reps)]
    rec = {"case": "self-search", "B": B, "n": n, "k": k, "passes_per_window": inner}
    rec["search_ms"], rec["search_min"], rec["search_max"] = _stats(times)
    print(json.dumps(rec), flush=True)
    return rec


def _case(name, source, k, reps, inner):
    B, n = source.shape[0], source.shape[1]
    idx = rigidity.neighbour_sets(source, k)
    pred = (source + 0.02 * torch.randn_like(source)).contiguous().requires_grad_(True)
    partners = [("native", _native), ("composed", _composed)]
    first = {key: _pass(fn, pred, source, idx) for key, fn in partners}      # (the untimed pass of each)
    again = _pass(_native, pred, source, idx)
    same = bool(torch.equal(first["native"][0], again[0])) and bool(torch.equal(first["native"][1], again[1]))
    err = float((first["native"][1] - first["composed"][1]).abs().max()) / float(first["composed"][1].abs().max())
    degree = int(torch.bincount(idx[0].reshape(-1).long(), minlength=n).max())
    rec = {"case": name, "B": B, "n": n, "k": k, "passes_per_window": inner, "max_in_degree": degree, "loss": float(first["native"][0]),
           "loss_composed": float(first["composed"][0]), "same_bits_twice": same, "max_err": float(f"{err:.3g}")}
    del first, again
    times = {key: [] for key, _ in partners}
    for _ in range(reps):
        for key, fn in partners:
            times[key].append(_time(lambda: [_pass(fn, pred, source, idx) for _ in range(inner)])[0] / inner)
    for key in ("native", "composed"):
        rec[key + "_ms"], rec[key + "_min"], rec[key + "_max"] = _stats(times[key])
    rec["composed_over_native"] = round(rec["composed_ms"] / rec["native_ms"], 2)
    print(json.dumps(rec), flush=True)
    return rec


def _hubs(source):
    """The cloud with its first eighth one point and its second eighth eight groups of copies."""
    n = source.shape[1]
    out = source.clone()
    out[:, :n // 8] = source[:, :1]
    group = max(n // 64, 1)
    for j in range(8):
        lo = n // 8 + j * group
        out[:, lo:lo + group] = source[:, lo:lo + 1]
    return out.contiguous()


def _train_steps(reps, inner, dev, streams, k):
    from nsdp_amd.graph_step import GraphedStep, capturable_adam
    from nsdp_amd.model import build_model, optimizer_factory
    data = {key: torch.from_numpy(v).to(dev) for key, v in synth.make_batch(1000, TRAIN_BATCH, N_SURF, N_QUERY).items()}
    steps = {}
    for name in ("plain", "rigidity"):
        cfg = default_config("forward")
        cfg["model"]["encoder_kwargs"]["npoints_per_layer"] = [N_SURF, 500, 100]
        if name == "rigidity":
            cfg["training"]["rigidity"] = {"weight": 1.0, "k": k}
        torch.manual_seed(0)
        model, train_fn, _, _ = build_model(cfg, device=dev)
        model.train()
        _, opt = optimizer_factory(cfg["training"], model.parameters())
        capturable_adam(opt)
        gs = GraphedStep(lambda m=model, o=opt, c=cfg, f=train_fn: f.tensor_step(m, o, data, c), max_streams=streams).capture(warmup=3)
        steps[name] = (gs, model, opt)
    for gs, _, _ in steps.values():
        gs()
    torch.cuda.synchronize()
    times = {key: [] for key in steps}
    for _ in range(reps):
        for key, (gs, _, _) in steps.items():
            times[key].append(_time(lambda: [gs() for _ in range(inner)])[0] / inner)
    rec = {"case": "replayed train step", "B": TRAIN_BATCH, "surface": N_SURF, "queries": N_QUERY, "k": k,
           "replays_per_window": inner, "streams": streams}
    for key, (gs, _, _) in steps.items():
        rec[key + "_ms"], rec[key + "_min"], rec[key + "_max"] = _stats(times[key])
        rec[key + "_kernels"], rec[key + "_streams"], rec[key + "_cross_stream_edges"] = (gs.info[i] for i in ("kernels", "streams", "cross_stream_edges"))
        rec[key + "_loss"] = float(gs().detach())
    gs = steps["rigidity"][0]
    rec["rigidity_kernels_in_replay"] = {name: [n, round(ms, 4)] for name, (n, ms) in
                                         ((name, gs.timed_replay(name)) for name in ("knn", "rigidity_", "invert_"))}
    rec["rigidity_minus_plain_ms"] = round(rec["rigidity_ms"] - rec["plain_ms"], 4)
    print(json.dumps(rec), flush=True)
    for gs, _, _ in steps.values():
        gs.close()
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--k", type=int, default=8)
    ap.add_argument("--shapes", type=lambda s: tuple(tuple(int(x) for x in p.split("x")) for p in s.split(",")), default=SHAPES)
    ap.add_argument("--streams", type=lambda s: tuple(int(x) for x in s.split(",")), default=(2, 1, 3),
                    help="streams of the replayed train steps, one comparison each (default 2,1,3)")
    ap.add_argument("--no-train", action="store_true")
    ap.add_argument("--train-only", action="store_true")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    recs = []
    if not args.train_only:
        for B, n in args.shapes:
            source = (torch.rand(B, n, 3, device=dev) - 0.5).contiguous()
            recs.append(_search(source, args.k, args.reps, 3))
            recs.append(_case("clouds", source, args.k, args.reps, 5))
            recs.append(_case("duplicate hubs", _hubs(source), args.k, args.reps, 5))
            del source
            torch.cuda.empty_cache()
    if not args.no_train:
        recs += [_train_steps(args.reps, 5, dev, streams, args.k) for streams in args.streams]
    ok = all(r.get("same_bits_twice", True) for r in recs)
    print(json.dumps({"same_bits_twice_everywhere": ok,
                      "native_slower_than_composed_at": [(r["case"], r["B"], r["n"]) for r in recs
                                                         if r.get("composed_over_native", 1.0) < 1.0]}), flush=True)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
