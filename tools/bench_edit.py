"""An editing session's drag against the call it replaces, in one process on one GPU (profiles/edit_session.txt).

    python tools/bench_edit.py [--sizes 5000,25000,100000] [--reps 5] [--batch 1]
    python tools/bench_edit.py --vertex-counts 25000,9000,40000,12000 [--reps 5]      (profiles/edit_session_ragged.txt)
    python tools/bench_edit.py --handles 3 --track 4,16 [--sizes ...] [--reps 5]       (profiles/edit_handle_sets.txt)

The tosca user-handle configuration's model (FlowArbitrary, npoints_per_layer [5000, 500, 100]; procedural weights), the cloud
= the vertex set (the reference's user-handle data set), one mesh of N uniform vertices per size.  Per size one JSON line with the
median and min-max in ms over ``reps`` interleaved repetitions (session eager, session replayed, full call eager, full call
replayed, session eager, ...), each a window of several calls between two HIP events, after untimed warm-up calls of every
variant; every drag of a window has another translation:

    drag_eager_ms     EditSession.drag, op by op;
    drag_graph_ms     EditSession(graph=True).drag: parameter copy + replay;
    full_eager_ms     the parent's path: test_on_batch_with_arbitrary on the data_dict the same drag stands for (the dict is built
                      before the window; building it is not in the time);
    full_graph_ms     ... through query_sharded(test_on_batch_with_arbitrary, QueryShards(0, 1), graph=True): copy of the inputs +
                      replay;
    open_ms           EditSession.reopen(): network 1, network 2's index sets, the bounds (windows of one);
    bounds_ms, rows_ms   nsdp_handle_bounds and nsdp_handle_rows alone (windows of 200 launches);
    equal             the session's predictions, eager and replayed, are bit-equal to the full call's.

The ratios ``full_eager / drag_eager`` and ``full_graph / drag_graph`` are reported as they come out; nothing is tuned to them.

``--vertex-counts``: B meshes of these vertex counts, packed, the cloud = the vertex set, through a RaggedEditSession -- against
the two ways a packed batch could be dragged without it, interleaved in the same way:

    drag_eager_ms / drag_graph_ms         RaggedEditSession.drag, op by op / copy + replay;
    full_eager_ms                         test_on_batch_with_arbitrary on the ragged data_dict of the same drag (a step with a ragged
                                          cloud reads the counts on the host and is not captured: there is no full_graph);
    per_mesh_eager_ms / per_mesh_graph_ms B batch-1 EditSessions, one per mesh, dragged in turn;
    open_ms                               RaggedEditSession.reopen();
    bounds_ms, rows_ms                    nsdp_handle_bounds_ragged and nsdp_handle_rows_ragged alone (windows of 200 launches).

``--handles H [--track T1,T2]``: a labelled handle set of H labels (labels_from_parts of the first H - 1 parts of the rule: the
first turns about its centroid and moves, the others and the rest of the rule's handle points are pinned), every session with
``graph=True``, interleaved in the same way:

    set_rows_ms / rule_rows_ms            nsdp_handle_set_rows (T = 1) and nsdp_handle_rows alone on the same rows (windows of 200);
    pose_graph_ms / drag_graph_ms         EditSession.pose and a rule EditSession.drag, replayed;
    track_T_ms                            EditSession.track of T poses, replayed: per call and per pose;
    poses_T_ms / drags_T_ms               the same T poses through T replayed pose calls in turn / the parent's way of getting T
                                          poses: T replayed rule drags; per T calls and per pose;
    first_track_T_ms                      the first track of a T, once: its index sets over T * B rows, its buffers and the capture
                                          (host clock around the call and a synchronize);
    equal                                 a pose's predictions are bit-equal to the full call's on reference_pose_dict's data_dict.
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from nsdp_amd import pointnet2_utils as pu, synth                                  # noqa: E402
from nsdp_amd.config import default_config                                         # noqa: E402
from nsdp_amd.edit import (PARTS, EditSession, HandleSpec, Motion, RaggedEditSession, pack_motions, pack_params,  # noqa: E402
                           reference_data_dict, reference_pose_dict)
from nsdp_amd.model import build_model                                             # noqa: E402
from nsdp_amd.model.flow_arbitrary import test_on_batch_with_arbitrary             # noqa: E402
from nsdp_amd.query_shard import QueryShards, query_sharded                        # noqa: E402
from nsdp_amd.ragged import RaggedPoints                                           # noqa: E402

SPEC = HandleSpec("head", (-0.15, -0.2, -0.2), 0.1, False)      # config/tosca/head.yaml's drag
KEYS = ("verts_tgt_pred", "surface_samples_tgt_pred")
KERNEL_WINDOW = 200


def window(fn, n):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for i in range(n):
        fn(i)
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / n


def stats(xs):
    return {"median": round(statistics.median(xs), 4), "min": round(min(xs), 4), "max": round(max(xs), 4)}


def bench_size(model, N, batch, reps, dev):
    verts = torch.from_numpy(synth.uniform(1000, "mesh_verts", (batch, N, 3), -0.5, 0.5)).to(dev)
    calls = 20 if N <= 25000 else 10

    def translation(i):
        return tuple(v * (1.0 + 0.01 * (i % 7)) for v in SPEC.translation)

    eager, graphed = EditSession(model, verts), EditSession(model, verts, graph=True)
    full_graph = query_sharded(test_on_batch_with_arbitrary, QueryShards(0, 1), graph=True)
    # the data_dicts of the drags of a window, built with torch ahead of it (seven distinct translations)
    dicts = [reference_data_dict(verts, None, HandleSpec(SPEC.part, translation(i), SPEC.partial_range, SPEC.cliptail))
             for i in range(7)]
    dicts = [{k: d[k] for k in ("surface_samples_inputs", "verts_src")} for d in dicts]
    variants = {
        "drag_eager_ms": lambda i: eager.drag(SPEC.part, translation(i), clone=False),
        "drag_graph_ms": lambda i: graphed.drag(SPEC.part, translation(i), clone=False),
        "full_eager_ms": lambda i: test_on_batch_with_arbitrary(model, dict(dicts[i % 7]), None),
        "full_graph_ms": lambda i: full_graph(model, dict(dicts[i % 7]), None),
    }
    # results first: the same drag through all four
    want = test_on_batch_with_arbitrary(model, dict(dicts[3]), None)[1]
    got = [eager.drag(SPEC.part, translation(3)), graphed.drag(SPEC.part, translation(3)), full_graph(model, dict(dicts[3]), None)[1]]
    equal = all(torch.equal(g[k], want[k]) for g in got for k in KEYS)
    for fn in variants.values():      # warm-up of every variant (the captures happened above)
        for i in range(3):
            fn(i)
    times = {k: [] for k in variants}
    times["open_ms"] = []
    for _ in range(reps):
        for k, fn in variants.items():
            times[k].append(window(fn, calls))
        times["open_ms"].append(window(lambda i: eager.reopen(), 1))
    # the two kernels alone
    params = torch.from_numpy(pack_params(batch, SPEC.part, SPEC.translation, SPEC.partial_range, SPEC.cliptail)).to(dev)
    rows = torch.empty(batch, N, 7, device=dev)
    tgt = torch.empty(batch, N, 3, device=dev)
    flags = torch.empty(batch, N, dtype=torch.uint8, device=dev)
    bounds = pu.handle_bounds(verts)
    ws = torch.empty(1 << 16, dtype=torch.int32, device=dev)
    kernels = {"bounds_ms": lambda i: pu.handle_bounds(verts, workspace=ws, out=bounds),
               "rows_ms": lambda i: pu.handle_rows(verts, verts, bounds, params, rows, tgt=tgt, handle_out=flags)}
    for fn in kernels.values():
        fn(0)
    for k in kernels:
        times[k] = []
    for _ in range(reps):
        for k, fn in kernels.items():
            times[k].append(window(fn, KERNEL_WINDOW))
    pu.check_fps_cluster()
    line = {"vertices": N, "batch": batch, "calls_per_window": calls, "reps": reps,
            "handle_points": int(eager.drag(SPEC.part, SPEC.translation)["cano_handle_sample_idx"].sum()),
            **{k: stats(v) for k, v in times.items()}, "equal": bool(equal),
            "graph_nodes": {"session": graphed._steps[(False, False)].info, "full_call": full_graph._step.info},
            "replays": graphed.replays}
    med = {k: statistics.median(v) for k, v in times.items()}
    line["full_eager_over_drag_eager"] = round(med["full_eager_ms"] / med["drag_eager_ms"], 3)
    line["full_graph_over_drag_graph"] = round(med["full_graph_ms"] / med["drag_graph_ms"], 3)
    line["full_eager_over_drag_graph"] = round(med["full_eager_ms"] / med["drag_graph_ms"], 3)
    for s in (eager, graphed, full_graph):
        s.close()
    return line


def bench_ragged(model, counts, reps, dev):
    B = len(counts)
    meshes = [torch.from_numpy(synth.uniform(1000 + b, "mesh_verts", (1, n, 3), -0.5, 0.5)).to(dev) for b, n in enumerate(counts)]
    verts = RaggedPoints.from_list([m[0] for m in meshes])
    calls = 20 if sum(counts) <= 25000 else 10

    def translation(i):
        return tuple(v * (1.0 + 0.01 * (i % 7)) for v in SPEC.translation)

    eager, graphed = RaggedEditSession(model, verts), RaggedEditSession(model, verts, graph=True)
    singles = [EditSession(model, m) for m in meshes]
    singles_graph = [EditSession(model, m, graph=True) for m in meshes]
    # the ragged data_dicts of the drags of a window, ahead of it: the session's own reference-shaped inputs (bit-equal to the
    # torch-built ones, tests/test_edit_session_ragged_gpu.py)
    dicts = []
    for i in range(7):
        inputs = eager.drag(SPEC.part, translation(i), with_inputs=True)["surface_samples_inputs"]
        dicts.append({"surface_samples_inputs": inputs, "surface_samples_src": inputs.columns(0, 3), "verts_src": verts})
    variants = {
        "drag_eager_ms": lambda i: eager.drag(SPEC.part, translation(i), clone=False),
        "drag_graph_ms": lambda i: graphed.drag(SPEC.part, translation(i), clone=False),
        "full_eager_ms": lambda i: test_on_batch_with_arbitrary(model, dict(dicts[i % 7]), None),
        "per_mesh_eager_ms": lambda i: [s.drag(SPEC.part, translation(i), clone=False) for s in singles],
        "per_mesh_graph_ms": lambda i: [s.drag(SPEC.part, translation(i), clone=False) for s in singles_graph],
    }
    want = test_on_batch_with_arbitrary(model, dict(dicts[3]), None)[1]
    got = [eager.drag(SPEC.part, translation(3)), graphed.drag(SPEC.part, translation(3))]
    equal = all(torch.equal(g[k].packed, want[k].packed) for g in got for k in KEYS)
    for fn in variants.values():      # warm-up of every variant (the first replayed drags capture)
        for i in range(3):
            fn(i)
    times = {k: [] for k in variants}
    times["open_ms"] = []
    for _ in range(reps):
        for k, fn in variants.items():
            times[k].append(window(fn, calls))
        times["open_ms"].append(window(lambda i: eager.reopen(), 1))
    # the two kernels alone
    cap, n_max = verts.capacity, max(counts)
    params = torch.from_numpy(pack_params(B, SPEC.part, SPEC.translation, SPEC.partial_range, SPEC.cliptail)).to(dev)
    rows, tgt = torch.empty(cap, 7, device=dev), torch.empty(cap, 3, device=dev)
    flags = torch.empty(cap, dtype=torch.uint8, device=dev)
    bounds = pu.handle_bounds_ragged(verts.packed, verts.offsets, n_max)
    ws = torch.empty(1 << 16, dtype=torch.int32, device=dev)
    kernels = {"bounds_ms": lambda i: pu.handle_bounds_ragged(verts.packed, verts.offsets, n_max, workspace=ws, out=bounds),
               "rows_ms": lambda i: pu.handle_rows_ragged(verts.packed, verts.packed, verts.offsets, bounds, params, rows, tgt=tgt,
                                                          handle_out=flags)}
    for fn in kernels.values():
        fn(0)
    for k in kernels:
        times[k] = []
    for _ in range(reps):
        for k, fn in kernels.items():
            times[k].append(window(fn, KERNEL_WINDOW))
    pu.check_fps_cluster()
    line = {"vertex_counts": list(counts), "batch": B, "calls_per_window": calls, "reps": reps,
            "handle_points": int(eager.drag(SPEC.part, SPEC.translation)["cano_handle_sample_idx"].packed.sum()),
            **{k: stats(v) for k, v in times.items()}, "equal": bool(equal),
            "graph_nodes": {"session": graphed._steps[(False, False)].info}, "replays": graphed.replays}
    med = {k: statistics.median(v) for k, v in times.items()}
    line["full_eager_over_drag_eager"] = round(med["full_eager_ms"] / med["drag_eager_ms"], 3)
    line["full_eager_over_drag_graph"] = round(med["full_eager_ms"] / med["drag_graph_ms"], 3)
    line["per_mesh_eager_over_drag_eager"] = round(med["per_mesh_eager_ms"] / med["drag_eager_ms"], 3)
    line["per_mesh_graph_over_drag_graph"] = round(med["per_mesh_graph_ms"] / med["drag_graph_ms"], 3)
    for s in [eager, graphed] + singles + singles_graph:
        s.close()
    return line


def bench_handles(model, N, batch, reps, dev, H, tracks):
    import time
    verts = torch.from_numpy(synth.uniform(1000, "mesh_verts", (batch, N, 3), -0.5, 0.5)).to(dev)
    calls = 20 if N <= 25000 else 10

    def translation(i):
        return tuple(v * (1.0 + 0.01 * (i % 7)) for v in SPEC.translation)

    dragged, posed = EditSession(model, verts, graph=True), EditSession(model, verts, graph=True)
    labels, count = posed.labels_from_parts(PARTS[:H - 1])
    posed.set_handles(labels, count)
    first = (labels == 1)[:, :, None].double()
    pivots = ((verts.double() * first).sum(dim=1) / first.sum(dim=1).clamp(min=1.0)).cpu().numpy()

    def motions(i, scale=1.0):
        return [[Motion.rotate((0, 0, 1), (10.0 + i % 7) * scale, pivot=pivots[b]).then(
            Motion.translate([v * scale for v in translation(i)]))] + [Motion.identity()] * (count - 1) for b in range(batch)]

    def track_of(i, T):
        return [motions(i, (t + 1) / T) for t in range(T)]

    out = posed.pose(motions(3), with_inputs=True)
    dd = reference_pose_dict(verts, None, labels, count, motions=motions(3))
    want = test_on_batch_with_arbitrary(model, {k: dd[k] for k in ("surface_samples_inputs", "surface_samples_src", "verts_src")}, None)[1]
    equal = torch.equal(out["surface_samples_inputs"], dd["surface_samples_inputs"]) and all(torch.equal(out[k], want[k]) for k in KEYS)
    first_track = {}
    for T in tracks:      # the one-off cost of a T, on the host's clock
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        posed.track(track_of(0, T), clone=False)
        torch.cuda.synchronize()
        first_track[f"first_track_{T}_ms"] = round((time.perf_counter() - t0) * 1e3, 3)
    variants = {"drag_graph_ms": lambda i: dragged.drag(SPEC.part, translation(i), clone=False),
                "pose_graph_ms": lambda i: posed.pose(motions(i), clone=False)}
    for T in tracks:
        variants[f"track_{T}_ms"] = lambda i, T=T: posed.track(track_of(i, T), clone=False)
        variants[f"poses_{T}_ms"] = lambda i, T=T: [posed.pose(m, clone=False) for m in track_of(i, T)]
        variants[f"drags_{T}_ms"] = lambda i, T=T: [dragged.drag(SPEC.part, [v * (t + 1) / T for v in translation(i)], clone=False)
                                                    for t in range(T)]
    for fn in variants.values():
        for i in range(3):
            fn(i)
    times = {k: [] for k in variants}
    for _ in range(reps):
        for k, fn in variants.items():
            times[k].append(window(fn, calls if k in ("drag_graph_ms", "pose_graph_ms") else max(2, calls // 4)))
    # the two handle kernels alone, on the same rows
    params = torch.from_numpy(pack_params(batch, SPEC.part, SPEC.translation, SPEC.partial_range, SPEC.cliptail)).to(dev)
    table = torch.from_numpy(pack_motions(batch, count, motions(0))).to(dev)[None]
    rows, tgt = torch.empty(1, batch, N, 7, device=dev), torch.empty(1, batch, N, 3, device=dev)
    flags = torch.empty(batch, N, dtype=torch.uint8, device=dev)
    bounds = pu.handle_bounds(verts)
    kernels = {"rule_rows_ms": lambda i: pu.handle_rows(verts, verts, bounds, params, rows[0], tgt=tgt[0], handle_out=flags),
               "set_rows_ms": lambda i: pu.handle_set_rows(verts, labels, rows, motions=table, tgt=tgt, handle_out=flags)}
    for fn in kernels.values():
        fn(0)
    for k in kernels:
        times[k] = []
    for _ in range(reps):
        for k, fn in kernels.items():
            times[k].append(window(fn, KERNEL_WINDOW))
    pu.check_fps_cluster()
    line = {"vertices": N, "batch": batch, "labels": count, "tracks": list(tracks), "calls_per_window": calls, "reps": reps,
            "handle_points": int(out["cano_handle_sample_idx"].sum()), **{k: stats(v) for k, v in times.items()}, **first_track,
            "equal": bool(equal), "replays": posed.replays, "eager_calls": posed.eager_calls}
    med = {k: statistics.median(v) for k, v in times.items()}
    for T in tracks:
        line[f"per_pose_{T}_ms"] = {k: round(med[f"{k}_{T}_ms"] / T, 4) for k in ("track", "poses", "drags")}
    for s in (dragged, posed):
        s.close()
    return line


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--sizes", default="5000,25000,100000")
    ap.add_argument("--vertex-counts", action="append", default=None, metavar="n1,n2,...",
                    help="a packed batch of meshes of these vertex counts through a RaggedEditSession (may be given several times; "
                         "replaces --sizes and --batch)")
    ap.add_argument("--handles", type=int, default=None, metavar="H",
                    help="a labelled handle set of H labels (2..7) through pose() and track() against rule drags")
    ap.add_argument("--track", default="4,16", metavar="T1,T2", help="with --handles: the track lengths (default 4,16)")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--batch", type=int, default=1)
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        sys.exit("tools/bench_edit.py: needs a GPU (nothing here is a CPU measurement)")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    config = default_config("arbitrary")      # the tosca user-handle configs' model block
    model = build_model(config, device="cpu")[0]
    state = synth.procedural_state_dict(model.state_dict(), 2048)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in state.items()})
    model.to(dev).eval()
    print(json.dumps({"tool": "bench_edit", "device": torch.cuda.get_device_name(0), "model": config["model"]}), flush=True)
    if args.vertex_counts:
        with torch.no_grad():
            for text in args.vertex_counts:
                print(json.dumps(bench_ragged(model, tuple(int(v) for v in text.split(",")), args.reps, dev)), flush=True)
        return 0
    if args.handles is not None:
        if not 2 <= args.handles <= len(PARTS) + 1:
            sys.exit(f"tools/bench_edit.py: --handles wants 2..{len(PARTS) + 1} labels (parts of the rule plus the rest of its handle)")
        tracks = tuple(int(t) for t in args.track.split(",") if t)
        with torch.no_grad():
            for N in (int(s) for s in args.sizes.split(",")):
                print(json.dumps(bench_handles(model, N, args.batch, args.reps, dev, args.handles, tracks)), flush=True)
        return 0
    lines = []
    with torch.no_grad():
        for N in (int(s) for s in args.sizes.split(",")):
            lines.append(bench_size(model, N, args.batch, args.reps, dev))
            print(json.dumps(lines[-1]), flush=True)
    print(f"{'vertices':>9} {'drag eager':>11} {'drag graph':>11} {'full eager':>11} {'full graph':>11} {'open':>9} "
          f"{'bounds':>8} {'rows':>8}  full/drag eager, graph   equal   (ms, medians)")
    for ln in lines:
        m = {k: ln[k]["median"] for k in ln if k.endswith("_ms")}
        print(f"{ln['vertices']:>9} {m['drag_eager_ms']:>11.3f} {m['drag_graph_ms']:>11.3f} {m['full_eager_ms']:>11.3f} "
              f"{m['full_graph_ms']:>11.3f} {m['open_ms']:>9.3f} {m['bounds_ms']:>8.4f} {m['rows_ms']:>8.4f}  "
              f"{ln['full_eager_over_drag_eager']:>6.2f} {ln['full_graph_over_drag_graph']:>6.2f}            {ln['equal']}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
