"""The Chamfer training loss (nsdp_amd/chamfer.py) against two partners, in one process on one GPU.

    python tools/bench_chamfer.py [--reps 7] [--shapes 32x8192,4x100000] [--streams 2,1,3] [--no-train] [--train-only]

For every shape B x n (m = n) and each of two inputs -- two independent clouds in the unit cube, and the collapsed case (all
predictions one point, early training: every target lists prediction 0) -- one JSON line with the median and min-max in ms of
loss forward + backward (the gradient of the predictions; the targets take none, as in a train step), HIP events around windows
of several passes enqueued from Python, interleaved repetitions (native, composed, cdist, native, ...) after one untimed pass
of each:

    native_ms     chamfer_loss: one forward call, the list build, one backward launch;
    composed_ms   chamfer.composed_loss: nn_dist2 with indices twice, index_points through autograd, elementwise torch;
    cdist_ms      torch.cdist(pred, target) ** 2, min over either axis, autograd -- where its B x n x m matrix stays under 16 GiB
                  (null otherwise);
    same_bits_twice: the native loss and gradient of two passes are equal bit for bit; max_err: the native gradient's largest
                  difference from the composed one over the gradient's largest magnitude.

Then the replayed train step (forward model, B = 32, 2048 surface samples, 8192 queries and as many targets; GraphedStep on two
streams, on one and on three) with ``loss: chamfer`` against ``loss: l2``: ms per replay, interleaved windows, the kernels of either graph, and
(``chamfer_kernels_in_replay``) launches and total ms of the searches, the loss's own kernels and the list build as they run
inside one replay.
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from nsdp_amd import chamfer, synth                                  # noqa: E402
from nsdp_amd.config import default_config                          # noqa: E402

SHAPES = ((32, 8192), (4, 100000))
CDIST_MAX_BYTES = 16 << 30
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


def _cdist_loss(pred, target):
    d = torch.cdist(pred, target) ** 2
    return ((d.min(dim=2).values / 2.0).mean(dim=1) + (d.min(dim=1).values / 2.0).mean(dim=1)).mean()


def _pass(loss_fn, pred, target):
    pred.grad = None
    loss = loss_fn(pred, target)
    loss.backward()
    return loss.detach(), pred.grad


def _case(name, pred, target, reps, inner):
    B, n, m = pred.shape[0], pred.shape[1], target.shape[1]
    pred.requires_grad_(True)
    partners = [("native", chamfer.chamfer_loss), ("composed", chamfer.composed_loss)]
    if 4 * B * n * m <= CDIST_MAX_BYTES:
        partners.append(("cdist", _cdist_loss))
    first = {k: _pass(fn, pred, target) for k, fn in partners}      # (the untimed pass of each)
    again = _pass(chamfer.chamfer_loss, pred, target)
    same = bool(torch.equal(first["native"][0], again[0])) and bool(torch.equal(first["native"][1], again[1]))
    err = float((first["native"][1] - first["composed"][1]).abs().max()) / float(first["composed"][1].abs().max())
    rec = {"case": name, "B": B, "n": n, "m": m, "passes_per_window": inner, "loss": float(first["native"][0]),
           "loss_composed": float(first["composed"][0]), "same_bits_twice": same, "max_err": float(f"{err:.3g}")}
    if "cdist" in first:
        rec["loss_cdist"] = float(first["cdist"][0])
    del first, again
    times = {k: [] for k, _ in partners}
    for _ in range(reps):
        for k, fn in partners:
            times[k].append(_time(lambda: [_pass(fn, pred, target) for _ in range(inner)])[0] / inner)
    for k in ("native", "composed", "cdist"):
        rec[k + "_ms"], rec[k + "_min"], rec[k + "_max"] = _stats(times[k]) if k in times else (None, None, None)
    rec["composed_over_native"] = round(rec["composed_ms"] / rec["native_ms"], 2)
    if rec["cdist_ms"] is not None:
        rec["cdist_over_native"] = round(rec["cdist_ms"] / rec["native_ms"], 2)
    print(json.dumps(rec), flush=True)
    return rec


def _train_steps(reps, inner, dev, streams):
    from nsdp_amd.graph_step import GraphedStep, capturable_adam
    from nsdp_amd.model import build_model, optimizer_factory
    data = {k: torch.from_numpy(v).to(dev) for k, v in synth.make_batch(1000, TRAIN_BATCH, N_SURF, N_QUERY).items()}
    steps = {}
    for loss in ("l2", "chamfer"):
        cfg = default_config("forward")
        cfg["model"]["encoder_kwargs"]["npoints_per_layer"] = [N_SURF, 500, 100]
        cfg["training"]["loss"] = loss
        torch.manual_seed(0)
        model, train_fn, _, _ = build_model(cfg, device=dev)
        model.train()
        _, opt = optimizer_factory(cfg["training"], model.parameters())
        capturable_adam(opt)
        gs = GraphedStep(lambda m=model, o=opt, c=cfg, f=train_fn: f.tensor_step(m, o, data, c), max_streams=streams).capture(warmup=3)
        steps[loss] = (gs, model, opt)
    for gs, _, _ in steps.values():
        gs()
    torch.cuda.synchronize()
    times = {k: [] for k in steps}
    for _ in range(reps):
        for k, (gs, _, _) in steps.items():
            times[k].append(_time(lambda: [gs() for _ in range(inner)])[0] / inner)
    rec = {"case": "replayed train step", "B": TRAIN_BATCH, "surface": N_SURF, "queries": N_QUERY, "targets": N_QUERY,
           "replays_per_window": inner, "streams": streams}
    for k, (gs, _, _) in steps.items():
        rec[k + "_ms"], rec[k + "_min"], rec[k + "_max"] = _stats(times[k])
        rec[k + "_kernels"], rec[k + "_streams"], rec[k + "_cross_stream_edges"] = (gs.info[i] for i in ("kernels", "streams", "cross_stream_edges"))
        rec[k + "_loss"] = float(gs().detach())
    # where the difference goes: the loss's own kernels as they run inside the replay (events around the kernels of one name)
    gs = steps["chamfer"][0]
    rec["chamfer_kernels_in_replay"] = {name: [n, round(ms, 4)] for name, (n, ms) in
                                        ((name, gs.timed_replay(name)) for name in ("nn_dist2", "chamfer_", "invert_"))}
    rec["chamfer_minus_l2_ms"] = round(rec["chamfer_ms"] - rec["l2_ms"], 4)
    print(json.dumps(rec), flush=True)
    for gs, _, _ in steps.values():
        gs.close()
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--shapes", type=lambda s: tuple(tuple(int(x) for x in p.split("x")) for p in s.split(",")), default=SHAPES)
    ap.add_argument("--streams", type=lambda s: tuple(int(x) for x in s.split(",")), default=(2, 1, 3),
                    help="streams of the replayed train steps, one comparison each (default 2,1,3: the executor's default, one "
                         "stream, where nothing overlaps and a step is the sum of its kernels)")
    ap.add_argument("--no-train", action="store_true")
    ap.add_argument("--train-only", action="store_true")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    recs = []
    if not args.train_only:
        for B, n in args.shapes:
            target = (torch.rand(B, n, 3, device=dev) - 0.5).contiguous()
            cloud = (torch.rand(B, n, 3, device=dev) - 0.5).contiguous()
            recs.append(_case("clouds", cloud, target, args.reps, 5))
            del cloud
            torch.cuda.empty_cache()
            recs.append(_case("collapsed", torch.full((B, n, 3), 0.1, device=dev), target, args.reps, 1))
            torch.cuda.empty_cache()
    if not args.no_train:
        recs += [_train_steps(args.reps, 5, dev, streams) for streams in args.streams]
    ok = all(r.get("same_bits_twice", True) for r in recs)
    print(json.dumps({"same_bits_twice_everywhere": ok,
                      "native_slower_than_composed_at": [(r["case"], r["B"], r["n"]) for r in recs
                                                         if r.get("composed_over_native", 1.0) < 1.0]}), flush=True)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
