"""Dense inference of one batch of shapes split over GPUs by query point (nsdp_amd.query_shard), timed.

    python -m nsdp_amd.infer CONFIG --gpus N [--backend nccl|gloo] [--batch B] [--surface NS] [--queries NQ]
                             [--steps K] [--warmup W] [--graph] [--weight_file F] [--out DIR] [--decoder-dtype f32|bf16]

Every rank builds the model of the config (forward / backward / arbitrary; procedural weights, or ``--weight_file``), the same
synthetic batch (``synth.make_batch`` with one seed for all ranks: the ranks decode the same shapes) and runs the reference's
``test_on_batch`` through ``query_sharded``: surface samples and NQ mesh vertices per shape, encoded on every rank, decoded in
slices, all-gathered.  ``--gpus 1`` runs the same wrapper at world 1 -- no process group, the gather is the identity -- as the
A/B point (the same work as the unwrapped ``test_on_batch``).  From a bare shell the N ranks are launched here
(torch.distributed.run on 127.0.0.1, rank r -> GPU r, as nsdp_amd.train); under torchrun this process is one of them.

Rank 0 prints one JSON line: ``ms_per_call`` (HIP events around K calls after W warm-ups, the gather included; the maximum over
ranks), query points per second (the B x NQ vertices, as bench.py's dense_inference counts them; the surface samples' decode is
in the time), ``world``, ``backend``, the all-gather form used, each rank's device and PCI address and its calls that replayed /
ran eagerly, and ``ranks_agree`` (every rank's gathered predictions have the same byte checksum).  ``--out DIR`` writes rank 0's
predictions as DIR/<key>.npy.  ``--decoder-dtype bf16`` selects the fused decoder's bf16-operand kernel on every rank
(hip_decoder.MODE; ``decoder_dtype`` in the line); one extra call with the fp32 kernel after the timed region then gives
``max_abs_diff_vs_f32`` and ``l2_vs_f32`` (max over shapes of the RMS point distance) of the mesh-vertex predictions.

    python -m nsdp_amd.infer CONFIG --vertex-counts n1,n2,... [--capacity C] [--graph] [--decoder-dtype f32|bf16] ...

Meshes of DIFFERENT vertex counts in one call (nsdp_amd.ragged; one GPU): B = the number of counts, shape b decodes the first
n_b of the max(counts) synthetic vertices -- the rows the rectangular call at ``--batch B --queries max(counts)`` decodes for
it.  The step is ``ragged.RaggedTestOnBatch`` (capacity C, default the total; ``--graph``: captured once, replayed).  The line
gains ``ragged``, ``vertex_counts``, ``total``, ``capacity`` and, measured after the timed region in the same process in
interleaved repetitions (median; every repetition in ``*_reps``): ``ms_ragged`` (the same step again), ``ms_padded`` (the
rectangular call at B x max(counts), replayed under ``--graph``), ``ms_per_shape_loop`` (B eager calls at batch 1, the only
exact alternative without the packed form) and ``equal_to_padded`` (every shape's rows bit-equal to the padded call's).
``--out DIR``: verts_tgt_pred.npy is the packed [total, 3] array, verts_offsets.npy the [B + 1] offsets.

    python -m nsdp_amd.infer CONFIG --surface-counts n1,n2,... [--vertex-counts ...|--queries NQ] [--decoder-dtype f32|bf16] ...

Surface clouds of DIFFERENT sample counts in one call (one GPU, eager): B = the number of counts, shape b brings the first n_b
rows of the synthetic max(counts)-sample cloud; the encoder's levels are capped at min(counts).  The mesh vertices are ragged
too (``--vertex-counts``, as many counts) or NQ per shape.  The line gains ``ragged_surface``, ``surface_counts``,
``ms_per_call``, ``ms_per_shape_loop`` (B eager calls at batch 1 -- a surface cloud cannot be padded, so this is the only
exact alternative; interleaved repetitions, median, as above) and ``l2_vs_per_shape_loop`` (max over shapes of the RMS point
distance between the two vertex predictions: reported, not asserted -- the dense layers pick tile shapes from the row count, so
the two are close, not bit-equal).  ``--out DIR``: surface_samples_tgt_pred.npy is the packed [total, 3] array with
surface_offsets.npy; verts_tgt_pred.npy is packed with verts_offsets.npy under ``--vertex-counts``, else [B, NQ, 3].

    python -m nsdp_amd.infer CONFIG [--vertex-counts ...|--batch B] --metrics [P]

The evaluation metrics of the whole batch of predicted meshes in one call (eval_metric.compute_evaluation_metrics_batch, P
surface points per mesh, default 30000; rank 0, after the timed region).  The synthetic meshes get synthetic faces -- triples of
distinct vertices, no degenerate triangle -- and targets = the prediction plus a small deterministic offset.  The line gains
``metrics`` ({'l2', 'fnc', 'cd'}, a list per shape), ``metrics_points``, ``metrics_ms_batch`` (one call and its one read-back),
``metrics_ms_per_mesh_loop`` (eval_metric.compute_evaluation_metrics mesh after mesh, its three read-backs per mesh included;
both wall-clock, interleaved repetitions, median) and ``metrics_l2_fnc_max_abs_diff`` (batch against loop; ``cd`` uses
different draws and is not compared).  ``--scan-points N`` beside it scores every predicted mesh against a synthetic scan of N
points that shares no rows with it -- drawn on the displaced target surface -- through eval_metric.scan_metrics_batch (the exact
point-to-surface distance, nsdp_amd.surface_distance): the line gains ``scan_metrics`` ({'p2s', 's2p', 'cd_surface'}, a list
per shape) and ``scan_points``, and the three figures of every mesh go to stderr.

    python -m nsdp_amd.infer CONFIG [--vertex-counts ...|--batch B --queries NQ] --jacobian

The step with the deformation gradient (``test_on_batch(..., jacobian=True)``: the 3x3 Jacobian of the predicted deformation at
every mesh vertex, nsdp_amd.deformation_gradient; one GPU, eager, fp32 kernel).  The line carries ``ms_per_call`` of the step
with the Jacobian beside ``ms_per_call_plain`` of the step without it (interleaved repetitions, median; every repetition in
``*_reps``), ``equal_to_plain`` (the vertices keep their bits) and per shape ``fold_overs`` (vertices with det J <= 0),
``det_min`` and ``det_median``.  ``--out DIR`` also writes verts_tgt_jacobian.npy ([B, NQ, 3, 3], or the packed [total, 3, 3]
rows with verts_offsets.npy under ``--vertex-counts``).  Refused with ``--gpus`` above 1 and with ``--decoder-dtype bf16``.
"""
from __future__ import annotations

import argparse
import json
import os
import sys

SEED_DATA, SEED_WEIGHTS = 1000, 2048      # (bench.py's procedural weights; one batch for every rank)
KEYS = ("surface_samples_tgt_pred", "verts_tgt_pred")


def _checksum(t) -> int:
    """int64 sum over the int32 view: equal sums for bit-equal fp32 tensors."""
    import torch
    return int(t.contiguous().view(torch.int32).to(torch.int64).sum())


def _pyramid(config, ns):
    """The encoder samples at most the points it has: every level of npoints_per_layer capped at the level above it."""
    kw = config["model"]["encoder_kwargs"]
    levels, prev = [], int(ns)
    for p in kw["npoints_per_layer"]:
        prev = min(int(p), prev)
        levels.append(prev)
    kw["npoints_per_layer"] = levels


def build_parser():
    ap = argparse.ArgumentParser(description="Dense inference split over GPUs by query point")
    ap.add_argument("config_file")
    ap.add_argument("--gpus", type=int, default=1, help="ranks, one process per GPU; the query points are split over them")
    ap.add_argument("--backend", default="nccl", choices=["nccl", "gloo"],
                    help="torch.distributed backend (nccl = RCCL; gloo to exercise several ranks on one GPU)")
    ap.add_argument("--batch", type=int, default=None, help="shapes per call (default: the config's test.batch_size, else 1)")
    ap.add_argument("--surface", type=int, default=None,
                    help="surface samples per shape (default: the config's data.num_surf_samples, else the encoder's first level)")
    ap.add_argument("--queries", type=int, default=100000, help="mesh vertices per shape (default 100000, BASELINE config 5)")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--graph", action="store_true",
                    help="capture each rank's encode and local decode once and replay it; the gather runs eagerly after the replay")
    ap.add_argument("--weight_file", default=None, help="weights of the whole model (default: procedural weights)")
    ap.add_argument("--out", default=None, help="directory for rank 0's predictions (<key>.npy)")
    ap.add_argument("--vertex-counts", default=None,
                    help="comma-separated vertex counts, one per shape: decode the meshes as one packed (ragged) set")
    ap.add_argument("--surface-counts", default=None,
                    help="comma-separated surface sample counts, one per shape: encode the clouds as one packed (ragged) set")
    ap.add_argument("--capacity", type=int, default=None,
                    help="rows of the packed vertex buffer (default: the sum of --vertex-counts); a captured graph serves every "
                         "batch of as many shapes whose vertices sum to at most this")
    ap.add_argument("--reps", type=int, default=5, help="--vertex-counts: interleaved repetitions of the comparison timings")
    ap.add_argument("--metrics", type=int, nargs="?", const=30000, default=None, metavar="P",
                    help="evaluation metrics of the predicted batch in one call, P surface points per mesh (default 30000), "
                         "timed against the per-mesh loop")
    ap.add_argument("--scan-points", type=int, default=None, metavar="N",
                    help="with --metrics: score every predicted mesh against a synthetic scan of N points that shares no rows "
                         "with it (exact point-to-surface distance): p2s, s2p and cd_surface per mesh")
    ap.add_argument("--jacobian", action="store_true",
                    help="run the step with the deformation gradient at every mesh vertex; fold-overs and det J per shape")
    ap.add_argument("--decoder-dtype", default=None, choices=["f32", "bf16"],
                    help="operand type of the fused decoder kernel on every rank (default: NSDP_FUSED_DECODER_DTYPE, else f32)")
    return ap


def _synthetic_faces(n: int):
    """Faces for a synthetic mesh of n >= 3 vertices: (i, i+1, i+2) and, from 8 vertices on, (i, i+3, i+7), indices mod n --
    three distinct vertices each."""
    import torch
    i = torch.arange(n, dtype=torch.int32)
    faces = [torch.stack((i, (i + 1) % n, (i + 2) % n), dim=1)]
    if n >= 8:
        faces.append(torch.stack((i, (i + 3) % n, (i + 7) % n), dim=1))
    return torch.cat(faces)


def _metrics(args, pred):
    """The --metrics keys for the predicted vertices (a RaggedPoints or [B, V, 3]): the batch call, then the per-mesh loop."""
    import statistics
    import time
    import torch
    from . import eval_metric
    from .ragged import RaggedPoints
    P = int(args.metrics)
    ragged = isinstance(pred, RaggedPoints)
    rows = [r.contiguous() for r in pred.split()] if ragged else [pred[b] for b in range(pred.shape[0])]
    if min(int(r.shape[0]) for r in rows) < 3:
        sys.exit("nsdp_amd.infer: --metrics needs at least 3 vertices in every mesh")
    dev = rows[0].device
    faces = [_synthetic_faces(int(r.shape[0])).to(dev) for r in rows]
    shift = [0.01 * torch.sin(0.37 * torch.arange(int(r.shape[0]), device=dev, dtype=torch.float32)[:, None]
                              + torch.arange(3, device=dev, dtype=torch.float32)) for r in rows]
    tgts = [r + d for r, d in zip(rows, shift)]
    if ragged:
        batch = {"verts_tgt_pred": RaggedPoints.from_list(rows), "verts_tgt": RaggedPoints.from_list(tgts),
                 "faces": RaggedPoints.from_rows(faces)}
    else:
        batch = {"verts_tgt_pred": torch.stack(rows), "verts_tgt": torch.stack(tgts), "faces": torch.stack(faces)}
    singles = [{"verts_tgt_pred": r[None], "verts_tgt": t[None], "faces": f[None]} for r, t, f in zip(rows, tgts, faces)]
    gen = torch.Generator(device=dev).manual_seed(SEED_DATA)

    def run_batch():
        m = eval_metric.compute_evaluation_metrics_batch(batch, pointcloud_size=P, generator=gen)
        return {k: v.tolist() for k, v in m.items()}

    def run_loop():
        per = [eval_metric.compute_evaluation_metrics(one, pointcloud_size=P, generator=gen) for one in singles]
        return {k: [m[k] for m in per] for k in ("l2", "fnc", "cd")}

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    got, loop = run_batch(), run_loop()                                  # (warm-up of both, and the comparison)
    reps = {"metrics_ms_batch": [], "metrics_ms_per_mesh_loop": []}
    for _ in range(max(1, args.reps)):
        reps["metrics_ms_batch"].append(timed(run_batch))
        reps["metrics_ms_per_mesh_loop"].append(timed(run_loop))
    diff = max(abs(a - b) for k in ("l2", "fnc") for a, b in zip(got[k], loop[k]))
    return {"metrics": got, "metrics_points": P,
            **{k: round(statistics.median(v), 4) for k, v in reps.items()},
            **{k + "_reps": [round(x, 4) for x in v] for k, v in reps.items()},
            "metrics_l2_fnc_max_abs_diff": diff}


def _scan_metrics(args, pred):
    """The --scan-points keys for the predicted vertices (a RaggedPoints or [B, V, 3]): a synthetic scan of N points per shape
    drawn on the displaced surface of --metrics' target (so no scan point is a row of the prediction), then
    eval_metric.scan_metrics_batch -- {'p2s', 's2p', 'cd_surface'}, a list per shape."""
    import torch
    from . import eval_metric
    from .ragged import RaggedPoints
    N, P = int(args.scan_points), int(args.metrics)
    ragged = isinstance(pred, RaggedPoints)
    rows = [r.contiguous() for r in pred.split()] if ragged else [pred[b] for b in range(pred.shape[0])]
    dev = rows[0].device
    faces = [_synthetic_faces(int(r.shape[0])).to(dev) for r in rows]
    gen = torch.Generator(device=dev).manual_seed(SEED_DATA + 1)
    scans = []
    for r, f in zip(rows, faces):
        t = r + 0.01 * torch.sin(0.37 * torch.arange(int(r.shape[0]), device=dev, dtype=torch.float32)[:, None]
                                 + torch.arange(3, device=dev, dtype=torch.float32))
        face_idx, bary = eval_metric.sample_surface_batch(t[None], f[None], N, gen)
        scans.append(eval_metric.sample_points(t[None], f[None], face_idx, bary)[0].contiguous())
    if ragged:
        m = eval_metric.scan_metrics_batch(RaggedPoints.from_list(rows), RaggedPoints.from_rows(faces), RaggedPoints.from_list(scans),
                                           pointcloud_size=P, generator=gen)
    else:
        m = eval_metric.scan_metrics_batch(torch.stack(rows), torch.stack(faces), torch.stack(scans), pointcloud_size=P, generator=gen)
    got = {k: v.tolist() for k, v in m.items()}
    for b in range(len(rows)):
        print(f"scan metrics, mesh {b} ({int(rows[b].shape[0])} vertices, {N} scan points): p2s {got['p2s'][b]:.6g}  "
              f"s2p {got['s2p'][b]:.6g}  cd_surface {got['cd_surface'][b]:.6g}", file=sys.stderr)
    return {"scan_metrics": got, "scan_points": N}


def _ragged(args, config, model, test_fn, dd, counts, ns):
    """The --vertex-counts run (one GPU): timed packed step, then the comparison timings and the bit comparison."""
    import statistics
    import numpy as np
    import torch
    from . import hip_decoder, pointnet2_utils
    from .query_shard import QueryShards, query_sharded
    from .ragged import RaggedPoints, RaggedTestOnBatch
    B, total = len(counts), sum(counts)
    capacity = args.capacity or total
    verts = RaggedPoints.from_list([dd["verts_src"][b, :n] for b, n in enumerate(counts)])
    rdd = {k: v for k, v in dd.items() if k not in ("verts_src", "verts_tgt")}
    rdd["verts_src"] = verts
    step = RaggedTestOnBatch(test_fn, capacity, graph=args.graph)
    padded = query_sharded(test_fn, QueryShards(0, 1), graph=args.graph)
    per_shape = [{"surface_samples_inputs": dd["surface_samples_inputs"][b:b + 1].contiguous(),
                  "surface_samples_src": dd["surface_samples_src"][b:b + 1].contiguous(),
                  "verts_src": dd["verts_src"][b:b + 1, :n].contiguous()} for b, n in enumerate(counts)]

    def run_ragged():
        step(model, rdd, config)

    def run_padded():
        padded(model, dd, config)

    def run_loop():
        for one in per_shape:
            test_fn(model, dict(one), config)

    def timed(fn, n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(n):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / max(1, n)

    for _ in range(max(args.warmup, 1 if args.graph else 0)):      # (--graph: the first call captures)
        run_ragged()
    ms = timed(run_ragged, args.steps)
    replays, eager_calls = step.replays, step.eager_calls
    pred = {k: (rdd[k].packed if k == "verts_tgt_pred" else rdd[k]).clone() for k in KEYS}
    # the comparisons: after the timed region, same process, interleaved repetitions
    run_padded()
    run_loop()
    want = dd["verts_tgt_pred"]
    got = rdd["verts_tgt_pred"].split()
    equal = all(torch.equal(got[b], want[b, :n]) for b, n in enumerate(counts)) and \
        torch.equal(rdd["surface_samples_tgt_pred"], dd["surface_samples_tgt_pred"])
    reps = {"ms_ragged": [], "ms_padded": [], "ms_per_shape_loop": []}
    for _ in range(max(1, args.reps)):
        reps["ms_ragged"].append(timed(run_ragged, args.steps))
        reps["ms_padded"].append(timed(run_padded, args.steps))
        reps["ms_per_shape_loop"].append(timed(run_loop, args.steps))
    pointnet2_utils.check_fps_cluster()      # (a large surface cloud is sampled by a workgroup cluster: no wait may have given up)
    if args.out:
        os.makedirs(args.out, exist_ok=True)
        for k in KEYS:
            np.save(os.path.join(args.out, k + ".npy"), pred[k].cpu().numpy())
        np.save(os.path.join(args.out, "verts_offsets.npy"), verts.offsets.cpu().numpy())
    line = {"metric": "dense_inference_ragged", "model_type": config["model"]["type"], "world": 1, "graph": bool(args.graph),
            "ragged": True, "vertex_counts": counts, "total": total, "capacity": capacity, "batch": B, "surface": ns,
            "queries_padded": B * max(counts), "steps": args.steps, "warmup": args.warmup, "reps": max(1, args.reps),
            "decoder_dtype": hip_decoder.MODE, "ms_per_call": round(ms, 4),
            "query_points_per_s": round(total / (ms / 1e3), 1) if ms > 0 else None,
            "replays": replays, "eager_calls": eager_calls, "padded_replays": padded.replays,
            **{k: round(statistics.median(v), 4) for k, v in reps.items()},
            **{k + "_reps": [round(x, 4) for x in v] for k, v in reps.items()},
            "equal_to_padded": bool(equal)}
    if args.metrics is not None:
        line.update(_metrics(args, rdd["verts_tgt_pred"].like(pred["verts_tgt_pred"])))
        if args.scan_points is not None:
            line.update(_scan_metrics(args, rdd["verts_tgt_pred"].like(pred["verts_tgt_pred"])))
    print(json.dumps(line), flush=True)
    step.close()
    padded.close()
    return 0


def _ragged_surface(args, config, model, test_fn, dd, scounts, vcounts):
    """The --surface-counts run (one GPU, eager): the timed packed step, then B calls at batch 1, interleaved."""
    import statistics
    import numpy as np
    import torch
    from . import hip_decoder, pointnet2_utils
    from .ragged import RaggedPoints
    B = len(scounts)
    surf = RaggedPoints.from_rows([dd["surface_samples_inputs"][b, :n] for b, n in enumerate(scounts)])
    rdd = {"surface_samples_inputs": surf, "surface_samples_src": surf.columns(0, 3)}
    if vcounts:
        rdd["verts_src"] = RaggedPoints.from_list([dd["verts_src"][b, :n] for b, n in enumerate(vcounts)])
    else:
        rdd["verts_src"] = dd["verts_src"]
    nverts = vcounts or [int(dd["verts_src"].shape[1])] * B
    per_shape = [{"surface_samples_inputs": dd["surface_samples_inputs"][b:b + 1, :n].contiguous(),
                  "surface_samples_src": dd["surface_samples_inputs"][b:b + 1, :n, 0:3].contiguous(),
                  "verts_src": dd["verts_src"][b:b + 1, :nverts[b]].contiguous()} for b, n in enumerate(scounts)]
    loop_out = [None] * B

    def run_ragged():
        test_fn(model, rdd, config)

    def run_loop():
        for b, one in enumerate(per_shape):
            loop_out[b] = test_fn(model, dict(one), config)[1]["verts_tgt_pred"]

    def timed(fn, n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(n):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / max(1, n)

    for _ in range(args.warmup):
        run_ragged()
    ms = timed(run_ragged, args.steps)
    run_loop()
    pred = rdd["verts_tgt_pred"]
    rows = pred.split() if vcounts else [pred[b] for b in range(B)]
    l2 = max(float((rows[b].double() - loop_out[b][0].double()).pow(2).sum(-1).mean().sqrt()) for b in range(B) if nverts[b])
    reps = {"ms_ragged": [], "ms_per_shape_loop": []}
    for _ in range(max(1, args.reps)):
        reps["ms_ragged"].append(timed(run_ragged, args.steps))
        reps["ms_per_shape_loop"].append(timed(run_loop, args.steps))
    pointnet2_utils.check_fps_cluster()      # (a large surface cloud is sampled by a workgroup cluster: no wait may have given up)
    if args.out:
        os.makedirs(args.out, exist_ok=True)
        np.save(os.path.join(args.out, "surface_samples_tgt_pred.npy"), rdd["surface_samples_tgt_pred"].packed.cpu().numpy())
        np.save(os.path.join(args.out, "surface_offsets.npy"), surf.offsets.cpu().numpy())
        np.save(os.path.join(args.out, "verts_tgt_pred.npy"), (pred.packed if vcounts else pred).cpu().numpy())
        if vcounts:
            np.save(os.path.join(args.out, "verts_offsets.npy"), pred.offsets.cpu().numpy())
    total_v = sum(nverts)
    line = {"metric": "dense_inference_ragged_surface", "model_type": config["model"]["type"], "world": 1, "graph": False,
            "ragged_surface": True, "surface_counts": scounts, "surface_total": sum(scounts), "ragged": bool(vcounts),
            "vertex_counts": vcounts or None, "queries": None if vcounts else nverts[0], "total": total_v, "batch": B,
            "levels": config["model"]["encoder_kwargs"]["npoints_per_layer"], "steps": args.steps, "warmup": args.warmup,
            "reps": max(1, args.reps), "decoder_dtype": hip_decoder.MODE, "ms_per_call": round(ms, 4),
            "query_points_per_s": round(total_v / (ms / 1e3), 1) if ms > 0 else None,
            **{k: round(statistics.median(v), 4) for k, v in reps.items()},
            **{k + "_reps": [round(x, 4) for x in v] for k, v in reps.items()},
            "l2_vs_per_shape_loop": l2}
    if args.metrics is not None:
        line.update(_metrics(args, pred))
        if args.scan_points is not None:
            line.update(_scan_metrics(args, pred))
    print(json.dumps(line), flush=True)
    return 0


def _jacobian(args, config, model, test_fn, dd, counts, ns):
    """The --jacobian run (one GPU, eager): the step with and without the Jacobian, interleaved; fold-overs and det J per shape."""
    import statistics
    import numpy as np
    import torch
    from . import deformation_gradient, hip_decoder, pointnet2_utils
    from .ragged import RaggedPoints
    rdd = {k: v for k, v in dd.items() if k != "verts_tgt"}
    if counts:
        rdd["verts_src"] = RaggedPoints.from_list([dd["verts_src"][b, :n] for b, n in enumerate(counts)])
    B = len(counts) if counts else int(dd["verts_src"].shape[0])
    nverts = counts or [int(dd["verts_src"].shape[1])] * B
    plain_dd, jac_dd = dict(rdd), dict(rdd)

    def run_plain():
        test_fn(model, plain_dd, config)

    def run_jacobian():
        test_fn(model, jac_dd, config, jacobian=True)

    def timed(fn, n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(n):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / max(1, n)

    for _ in range(max(1, args.warmup)):
        run_plain()
        run_jacobian()
    reps = {"ms_per_call": [], "ms_per_call_plain": []}
    for _ in range(max(1, args.reps)):
        reps["ms_per_call"].append(timed(run_jacobian, args.steps))
        reps["ms_per_call_plain"].append(timed(run_plain, args.steps))
    pointnet2_utils.check_fps_cluster()      # (a large surface cloud is sampled by a workgroup cluster: no wait may have given up)
    raw = lambda t: t.packed if isinstance(t, RaggedPoints) else t
    J, pred = jac_dd["verts_tgt_jacobian"], jac_dd["verts_tgt_pred"]
    equal = all(torch.equal(raw(jac_dd[k]), raw(plain_dd[k])) for k in KEYS)
    det = deformation_gradient.determinant(J)
    rows = list(torch.split(det[:sum(nverts)], nverts)) if counts else [det[b] for b in range(B)]
    folds = deformation_gradient.fold_overs(J).tolist()
    if args.out:
        os.makedirs(args.out, exist_ok=True)
        for k in KEYS:
            np.save(os.path.join(args.out, k + ".npy"), raw(jac_dd[k]).cpu().numpy())
        if counts:
            np.save(os.path.join(args.out, "verts_tgt_jacobian.npy"), J.packed[:sum(nverts)].view(-1, 3, 3).cpu().numpy())
            np.save(os.path.join(args.out, "verts_offsets.npy"), pred.offsets.cpu().numpy())
        else:
            np.save(os.path.join(args.out, "verts_tgt_jacobian.npy"), J.cpu().numpy())
    ms = statistics.median(reps["ms_per_call"])
    line = {"metric": "dense_inference_jacobian", "model_type": config["model"]["type"], "world": 1, "graph": False,
            "jacobian": True, "ragged": bool(counts), "vertex_counts": counts or None, "queries": None if counts else nverts[0],
            "total": sum(nverts), "batch": B, "surface": ns, "steps": args.steps, "warmup": args.warmup, "reps": max(1, args.reps),
            "decoder_dtype": hip_decoder.MODE,
            **{k: round(statistics.median(v), 4) for k, v in reps.items()},
            **{k + "_reps": [round(x, 4) for x in v] for k, v in reps.items()},
            "query_points_per_s": round(sum(nverts) / (ms / 1e3), 1) if ms > 0 else None,
            "equal_to_plain": bool(equal), "fold_overs": [int(f) for f in folds],
            "det_min": [float(r.min()) if r.numel() else None for r in rows],
            "det_median": [float(r.median()) if r.numel() else None for r in rows]}
    print(json.dumps(line), flush=True)
    return 0


def _counts_arg(flag, text, positive=False):
    try:
        counts = [int(c) for c in text.split(",") if c.strip() != ""]
    except ValueError:
        counts = []
    if not counts or min(counts) < (1 if positive else 0) or max(counts) == 0:
        sys.exit(f"nsdp_amd.infer: {flag} wants {'positive' if positive else 'non-negative'} integers n1,n2,..."
                 f"{'' if positive else ' (not all zero)'}, got {text!r}")
    return counts


def main(argv=None):
    argv = list(sys.argv[1:] if argv is None else argv)
    ap = build_parser()
    args = ap.parse_args(argv)
    counts = scounts = None
    if args.surface_counts is not None:
        scounts = _counts_arg("--surface-counts", args.surface_counts, positive=True)
        if args.gpus > 1 or int(os.environ.get("WORLD_SIZE", "1")) > 1:
            sys.exit("nsdp_amd.infer: --surface-counts runs on one GPU (ragged surface clouds are not split over ranks)")
        if args.graph:
            sys.exit("nsdp_amd.infer: --surface-counts runs eagerly (a step over ragged surface clouds is not captured)")
        if args.batch is not None and args.batch != len(scounts):
            sys.exit(f"nsdp_amd.infer: --batch {args.batch} against {len(scounts)} surface counts")
        if args.surface is not None and args.surface != max(scounts):
            sys.exit(f"nsdp_amd.infer: --surface {args.surface} against --surface-counts whose largest is {max(scounts)}")
    if args.vertex_counts is not None:
        try:
            counts = [int(c) for c in args.vertex_counts.split(",") if c.strip() != ""]
        except ValueError:
            counts = []
        if not counts or min(counts) < 0 or max(counts) == 0:
            sys.exit(f"nsdp_amd.infer: --vertex-counts wants non-negative integers n1,n2,... (not all zero), got {args.vertex_counts!r}")
        if args.gpus > 1 or int(os.environ.get("WORLD_SIZE", "1")) > 1:
            sys.exit("nsdp_amd.infer: --vertex-counts runs on one GPU (splitting a ragged set over ranks is not implemented)")
        if args.capacity is not None and args.capacity < sum(counts):
            sys.exit(f"nsdp_amd.infer: --capacity {args.capacity} is below the {sum(counts)} vertices of --vertex-counts")
        if args.batch is not None and args.batch != len(counts):
            sys.exit(f"nsdp_amd.infer: --batch {args.batch} against {len(counts)} vertex counts")
        if scounts and len(scounts) != len(counts):
            sys.exit(f"nsdp_amd.infer: {len(scounts)} surface counts against {len(counts)} vertex counts")
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if args.jacobian:
        if args.gpus > 1 or world > 1:
            sys.exit("nsdp_amd.infer: --jacobian runs on one GPU (query_sharded gathers the predictions alone; splitting the "
                     "Jacobian over ranks is not implemented)")
        if args.decoder_dtype == "bf16":
            sys.exit("nsdp_amd.infer: --jacobian with --decoder-dtype bf16: the bf16-operand decoder kernel has no Jacobian "
                     "form (the fp32 kernel computes it)")
        if scounts or args.graph or args.metrics is not None:
            sys.exit("nsdp_amd.infer: --jacobian runs the eager step over a rectangular surface cloud, alone (not with "
                     "--surface-counts, --graph or --metrics)")
    if args.metrics is not None and args.metrics < 1:
        sys.exit(f"nsdp_amd.infer: --metrics wants a positive number of surface points, got {args.metrics}")
    if args.scan_points is not None and (args.metrics is None or args.scan_points < 1):
        sys.exit(f"nsdp_amd.infer: --scan-points wants a positive number of scan points and goes with --metrics, got {args.scan_points}")
    if args.metrics is not None and counts and min(counts) < 3:
        sys.exit("nsdp_amd.infer: --metrics needs at least 3 vertices in every mesh of --vertex-counts")
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        from .train import launch_ranks
        return launch_ranks(args.gpus, argv, module="nsdp_amd.infer")
    if args.gpus != world:
        sys.exit(f"nsdp_amd.infer: --gpus {args.gpus} but the launcher's WORLD_SIZE is {world}")
    rank, local_rank = int(os.environ.get("RANK", "0")), int(os.environ.get("LOCAL_RANK", "0"))
    local_world = int(os.environ.get("LOCAL_WORLD_SIZE", str(world)))
    from .cpu_budget import cap_thread_pools
    cap_thread_pools(max(1, 16 // max(1, local_world)))
    import numpy as np
    import torch
    import torch.distributed as dist
    if not torch.cuda.is_available():
        sys.exit("nsdp_amd.infer: needs a GPU (the decode has no CPU path)")
    if world > 1:
        from .parallel import rank_device
        index, cpus = rank_device(local_rank, world, args.backend)       # rank r -> GPU r, pinned to its CPU slice
        device = torch.device("cuda", index)
        print(f"nsdp_amd.infer: rank {rank} -> GPU {index}, CPUs {cpus}", file=sys.stderr)
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if args.backend == "nccl":
            dist.init_process_group("nccl", rank=rank, world_size=world, device_id=device)
        else:
            dist.init_process_group(args.backend, rank=rank, world_size=world)
    else:
        index = 0
        device = torch.device("cuda", index)
        torch.cuda.set_device(index)

    from . import hip_decoder, pointnet2_utils, synth
    if args.decoder_dtype is not None:
        hip_decoder.set_mode(args.decoder_dtype)
    from .config import load_config
    from .model import build_model
    from .query_shard import QueryShards, query_sharded
    config = load_config(args.config_file)
    batch = len(scounts or counts) if (scounts or counts) else (args.batch or int(config.get("test", {}).get("batch_size", 1) or 1))
    ns = max(scounts) if scounts else args.surface or int(config.get("data", {}).get("num_surf_samples", 0) or
                             config["model"]["encoder_kwargs"]["npoints_per_layer"][0])
    nq = max(counts) if counts else int(args.queries)
    _pyramid(config, min(scounts) if scounts else ns)      # (ragged surface clouds: the smallest one bounds the levels)
    model, _, _, test_fn = build_model(config, weight_file=args.weight_file, device="cpu")
    if args.weight_file is None:
        state = synth.procedural_state_dict(model.state_dict(), SEED_WEIGHTS)
        model.load_state_dict({k: torch.from_numpy(v) for k, v in state.items()})
    model.to(device).eval()
    data = synth.make_batch(SEED_DATA, batch, ns, nq)
    dd = {k: torch.from_numpy(np.ascontiguousarray(v)).to(device) for k, v in data.items()}
    dd["surface_samples_src"] = dd["surface_samples_inputs"][:, :, 0:3].contiguous()
    dd["verts_src"], dd["verts_tgt"] = dd.pop("space_samples_src"), dd.pop("space_samples_tgt")

    if args.jacobian:
        decoder = getattr(model, "model_deform", model).decoder
        with torch.no_grad():
            why = (hip_decoder.jacobian_refusal(decoder) if hasattr(decoder, "ct1") else
                   f"the {type(decoder).__name__} computes no Jacobian (the cross-attention decoder does)")
        if why is not None:
            sys.exit("nsdp_amd.infer: --jacobian: " + why)
        return _jacobian(args, config, model, test_fn, dd, counts, ns)
    if scounts:
        return _ragged_surface(args, config, model, test_fn, dd, scounts, counts)
    if counts:
        return _ragged(args, config, model, test_fn, dd, counts, ns)
    shards = QueryShards(rank, world)
    step = query_sharded(test_fn, shards, graph=args.graph)

    def fence():
        torch.cuda.synchronize()
        if world > 1:
            dist.barrier()

    for _ in range(max(args.warmup, 1 if args.graph else 0)):      # (--graph: the first call captures)
        step(model, dd, config)
    fence()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(args.steps):
        step(model, dd, config)
    e1.record()
    torch.cuda.synchronize()
    pointnet2_utils.check_fps_cluster()      # (a large surface cloud is sampled by a workgroup cluster: no wait may have given up)
    ms = e0.elapsed_time(e1) / max(1, args.steps)

    props = torch.cuda.get_device_properties(index)
    mine = {"rank": rank, "device_index": index, "pci_domain_id": getattr(props, "pci_domain_id", None),
            "pci_bus_id": getattr(props, "pci_bus_id", None), "hip_visible_devices": os.environ.get("HIP_VISIBLE_DEVICES"),
            "ms_per_call": round(ms, 4), "replays": step.replays, "eager_calls": step.eager_calls,
            "checksums": [_checksum(dd[k]) for k in KEYS]}
    vs_f32 = {}
    if hip_decoder.MODE == "bf16":
        # one eager call with the fp32 kernel, outside the timed region (every rank: the gather is collective)
        pred = {k: dd[k].clone() for k in KEYS}
        with hip_decoder.mode("f32"):
            query_sharded(test_fn, shards)(model, dd, config)
        if rank == 0:
            d = pred["verts_tgt_pred"].double() - dd["verts_tgt_pred"].double()
            vs_f32 = {"max_abs_diff_vs_f32": float(d.abs().max()),
                      "l2_vs_f32": float(d.pow(2).sum(-1).mean(-1).sqrt().max())}
        dd.update(pred)
    ranks = [None] * world
    if world > 1:
        dist.all_gather_object(ranks, mine)
    else:
        ranks = [mine]
    if rank == 0:
        if args.out:
            os.makedirs(args.out, exist_ok=True)
            for k in KEYS:
                np.save(os.path.join(args.out, k + ".npy"), dd[k].cpu().numpy())
        ms_max = max(r["ms_per_call"] for r in ranks)
        line = {"metric": "dense_inference_query_sharded", "model_type": config["model"]["type"], "world": world,
                "backend": args.backend if world > 1 else None, "graph": bool(args.graph), "batch": batch, "surface": ns,
                "queries": nq, "steps": args.steps, "warmup": args.warmup, "decoder_dtype": hip_decoder.MODE,
                **vs_f32, "ms_per_call": ms_max,
                "query_points_per_s": round(batch * nq / (ms_max / 1e3), 1) if ms_max > 0 else None,
                "gather": None if world == 1 else ("all_gather" if shards.list_form else "all_gather_into_tensor"),
                "ranks_agree": all(r["checksums"] == ranks[0]["checksums"] for r in ranks),
                "ranks_share_a_device": len({(r["pci_domain_id"], r["pci_bus_id"]) for r in ranks}) < world,
                "ranks": [{k: r[k] for k in ("rank", "device_index", "pci_domain_id", "pci_bus_id", "hip_visible_devices",
                                             "ms_per_call", "replays", "eager_calls")} for r in ranks]}
        if args.metrics is not None:
            line.update(_metrics(args, dd["verts_tgt_pred"]))
            if args.scan_points is not None:
                line.update(_scan_metrics(args, dd["verts_tgt_pred"]))
        print(json.dumps(line), flush=True)
    if world > 1:
        dist.destroy_process_group()
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
