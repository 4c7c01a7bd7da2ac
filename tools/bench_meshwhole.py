"""Times one ``MeshStore.whole_meshes`` call (nsdp_mesh_batch_whole: the reference's ``load_mesh`` tensors of a batch of meshes
of different sizes in one launch) against the same tensors composed from torch ops, and ``nsdp_amd.evaluate`` over a procedural
tree at ``--batch 8`` against ``--batch 1`` (the reference's way), on one GPU.

    python tools/bench_meshwhole.py [--rounds 20] [--eval-runs 3] [--out profiles/mesh_whole.txt]

Sizes: the README's ragged sets -- eight meshes of 1800 to 7200 vertices, and 25 000 + 9000 + 40 000 + 12 000 vertices -- each mesh
with twice as many faces as vertices and three frames (canonical, source, target).  The two forms are timed with device events
after warm-up, ALTERNATED inside one loop, median and range over the rounds:

  whole     store.whole_meshes(ids, host_ids): two launches (offsets, rows), the offsets made on the device
  composed  per frame a slice of the vertex arena, ``cat`` over the shapes, ``dataset.cano_sample_handle_mask`` per shape, the
            multiply, ``cat`` into 7-wide rows, per topology a slice of the face arena and ``cat``, ``ragged.offsets_of`` (a host
            list and one copy)

``evaluate`` runs over the ``test_unseen_motions`` split of a tree of four identities of 1802 to 7202 vertices (12 pairs) with
the default forward model on procedural weights, no mesh export, 30 000 surface points per mesh for the metrics; the two batch
sizes alternate, pairs per second by the wall clock around the whole loop (the store is built once, outside).
"""
import argparse
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from bench_datastore import _ms, _stats      # noqa: E402  (tools/ is this script's directory)

SETS = {"8 meshes of 1800-7200 vertices": (1800, 2571, 3343, 4114, 4886, 5657, 6429, 7200),
        "25 000 + 9000 + 40 000 + 12 000 vertices": (25000, 9000, 40000, 12000)}
SPHERES = {"ant": (30, 60), "bee": (40, 80), "cow": (50, 100), "doe": (60, 120)}      # 1802, 3202, 5002, 7202 vertices


def kernels(rounds, say):
    import numpy as np
    import torch
    from nsdp_amd import dataset, meshstore
    from nsdp_amd.ragged import RaggedPoints, offsets_of
    dev = torch.device("cuda", 0)
    torch.zeros(1, device=dev)
    torch.cuda.synchronize()
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    g = np.random.RandomState(3)
    for name, counts in SETS.items():
        verts = [(g.rand(v, 3) - 0.5).astype(np.float32) for v in counts for _ in range(3)]
        faces = [g.randint(0, v, size=(2 * v, 3)).astype(np.int32) for v in counts]
        arrays = meshstore.pack(verts, [t for t in range(len(counts)) for _ in range(3)], faces, [])
        store = meshstore.MeshStore.__new__(meshstore.MeshStore)      # (a store around packed arrays: nothing is read from disk)
        store.cfg_data = {"partial_range": 0.1, "arbitrary": True, "inverse": False}
        store.frame_table_host, store.topo_table_host = arrays["frame_table"], arrays["topo_table"]
        for key in ("vert_arena", "face_arena", "frame_table", "topo_table"):
            setattr(store, key, torch.from_numpy(arrays[key]).to(dev))
        B = len(counts)
        host = np.array([[3 * b + c for b in range(B)] for c in range(3)], dtype=np.int32)
        ids = torch.from_numpy(host).to(dev)
        table = arrays["frame_table"]
        boxes = torch.from_numpy(np.stack([table[k, 3:6].copy().view(np.float32) for k in host[0]])).to(dev)      # (B, 6)

        def whole():
            return store.whole_meshes(ids, host)

        def composed():
            planes = []
            for c in range(3):
                rows = [store.vert_arena[int(table[k, 0]):int(table[k, 0]) + (int(table[k, 1]) & 0xFFFFFFFF), :3] for k in host[c]]
                planes.append(torch.cat(rows))
            masks = []
            for b, k in enumerate(host[0]):
                first, n = int(table[k, 0]), int(table[k, 1]) & 0xFFFFFFFF
                masks.append(dataset.cano_sample_handle_mask(0.1, store.vert_arena[None, first:first + n, :3], boxes[b:b + 1, :3],
                                                             boxes[b:b + 1, 3:])[0])
            mask = torch.cat(masks).unsqueeze(1)
            mf = mask.float()
            inputs = torch.cat([planes[1], planes[2] * mf, mf], dim=1)
            tops = [arrays["topo_table"][int(table[k, 1]) >> 32] for k in host[0]]
            packed_faces = torch.cat([store.face_arena[int(f0):int(f0) + int(nf), :3] for f0, nf in tops])
            voff, foff = offsets_of(counts, dev), offsets_of([int(nf) for _, nf in tops], dev)
            return ([RaggedPoints(p, voff, counts) for p in planes], mask, RaggedPoints(inputs, voff, counts),
                    RaggedPoints(packed_faces, foff, [int(nf) for _, nf in tops]))

        a, b = whole(), composed()
        same = all(torch.equal(a[f"verts_{k}"].packed, b[0][c].packed) for c, k in enumerate(("cano", "src", "tgt")))
        same = same and torch.equal(a["cano_handle_vert_idx"], b[1]) and torch.equal(a["verts_flow_inputs"].packed.view(torch.int32),
                                                                                       b[2].packed.view(torch.int32))
        same = same and torch.equal(a["faces"].packed, b[3].packed) and torch.equal(a["faces"].offsets, b[3].offsets)
        forms = [("whole", whole), ("composed", composed)]
        for _, fn in forms:
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        times = {n: [] for n, _ in forms}
        for _ in range(rounds):
            for n, fn in forms:
                times[n].append(_ms(fn, start, stop))
        tv, tf = sum(counts), 2 * sum(counts)
        moved = tv * (48 + 65) + tf * (16 + 12)
        med = {k: statistics.median(v) for k, v in times.items()}
        say(f"{name} ({tv} vertices, {tf} faces; the two forms give equal tensors: {same}):")
        for n, _ in forms:
            say(f"  {n:9s} {_stats(times[n])}")
        say(f"  whole / composed = {med['whole'] / med['composed']:.3f}   whole: {moved / 1e6:.2f} MB read and written = "
            f"{moved / med['whole'] / 1e6:.0f} GB/s")


def evaluation(work, runs, say):
    import torch
    from nsdp_amd import evaluate, meshstore, synth
    from nsdp_amd.config import default_config
    from nsdp_amd.model import build_model
    dev = torch.device("cuda", 0)
    meshes = {k: synth.sphere_mesh(*rs) for k, rs in SPHERES.items()}
    data = synth.write_mesh_dataset_tree(os.path.join(work, "tree"), meshes, ["walk", "jump", "turn"], 3, seed=3)
    cfg = default_config("forward")
    cfg["data"] = dict(data, num_surf_samples=2048, num_space_samples=128)
    cfg["test"] = {"iden_split": "identity_seen", "motion_split": "test_unseen_motions", "num_sampled_pairs": -1, "generate_mesh": False,
                   "generate_pointcloud": False, "pointcloud_size": 30000}
    torch.manual_seed(5)
    model, _, _, test_fn = build_model(cfg, device=dev)
    store = meshstore.MeshStore(cfg, "identity_seen", "test_unseen_motions", device=dev)
    say(f"evaluate: {len(store)} pairs of {sorted(set(v.shape[0] for v, _ in meshes.values()))} vertices, 30 000 surface points per mesh, "
        f"no mesh export")
    rate = {8: [], 1: []}
    for r in range(runs + 1):                                    # (round 0 warms both forms up and is not counted)
        for batch in (8, 1):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            rows = evaluate.evaluate(model, test_fn, store, cfg, os.path.join(work, f"run{batch}"), batch, 27, log=lambda *_: None)
            torch.cuda.synchronize()
            if r:
                rate[batch].append(len(rows) / (time.perf_counter() - t0))
    for batch, xs in rate.items():
        say(f"  --batch {batch}: median {statistics.median(xs):7.1f} pairs/s   range {min(xs):7.1f} .. {max(xs):7.1f}")
    say(f"  --batch 8 / --batch 1 = {statistics.median(rate[8]) / statistics.median(rate[1]):.2f}")


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--eval-runs", type=int, default=3, help="alternated runs of each batch size (0: skip the evaluation)")
    ap.add_argument("--out", default=None, help="also append the lines to this file")
    args = ap.parse_args(argv)
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    kernels(args.rounds, say)
    if args.eval_runs > 0:
        with tempfile.TemporaryDirectory() as tmp:
            evaluation(tmp, args.eval_runs, say)
    if args.out:
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
