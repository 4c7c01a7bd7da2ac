"""Times a training batch from the device-resident store (nsdp_amd/datastore.py) against what the same batch costs composed from
``dataset.prepare_batch``, and ``python -m nsdp_amd.train --dataset --graph`` against ``--synthetic --graph``, on one GPU.

    python tools/bench_datastore.py [--dir DIR] [--rounds 20] [--train-runs 3] [--out profiles/datastore.txt]

Shapes: bench.py's step -- B = 32, 2048 surface and 8192 space rows -- from 200 000-row fp16 frames written by
``synth.write_dataset_tree``.  Kernel forms are timed with device events after warm-up, ALTERNATED inside one loop (new, composed,
new, ...), median and range over the rounds:

  new       two nsdp_subset_draw launches + one nsdp_batch_assemble launch
  composed  what a loader without them has to do: index_select the batch's frames out of frame-major device tensors into nine
            [B, N_full, 3] clouds, then prepare_batch with random_subset (the key sort)
  draw / sort   the surface draw alone against random_subset's sort of B x N_full keys

The trainer is timed from its own log: the time between the SECOND and the LAST "epoch:" line of a run, over the steps in between --
start-up, store loading, the capture of the step (all before the first epoch line) and the checkpoint written after the first epoch
are excluded.  --dataset and --synthetic runs
alternate; the spread between repeated --synthetic runs is the yardstick for the difference.
"""
import argparse
import os
import re
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

B, N_SURF, N_SPACE, N_FULL = 32, 2048, 8192, 200000


def _ms(fn, start, stop):
    start.record()
    fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop)


def _stats(xs):
    return f"median {statistics.median(xs):8.3f} ms   range {min(xs):8.3f} .. {max(xs):8.3f}"


def kernels(data, rounds, say):
    import numpy as np
    import torch
    from nsdp_amd import dataset, datastore
    dev = torch.device("cuda", 0)
    config = {"data": data}
    t0 = time.perf_counter()
    store = datastore.SampleStore(config, "identity_seen", "train_seen", num_sampled_pairs=256, device=dev)
    torch.cuda.synchronize()
    load_s = time.perf_counter() - t0
    F = len(store.frames)
    say(f"store: {F} frames of {N_FULL} surface + {N_FULL} space rows, {store.surface_arena.dtype}; {store.nbytes / 1e6:.1f} MB on the device = "
        f"{store.nbytes / F / 1e6:.2f} MB per frame (12-byte surface records, 8-byte space records); loaded in {load_s:.2f} s by "
        f"{store._workers()} reader threads = {store.nbytes / 1e6 / load_s:.0f} MB/s; {len(store.pairs)} pairs formed, {len(store)} sampled")
    # frame-major tensors for the composition (every frame has N_FULL rows): what a torch-only store would keep
    surf = store.surface_arena.view(F, N_FULL, 6)
    frames = {"surface_samples": surf[..., :3].contiguous(), "surface_normals": surf[..., 3:].contiguous(),
              "space_samples": store.space_arena.view(F, N_FULL, 4)[..., :3].contiguous()}
    picks = np.asarray(store.sample_indices(0)[:B])
    ids = torch.from_numpy(np.ascontiguousarray(store.pair_frames[picks].T)).to(dev)
    counts = torch.full((B,), N_FULL, dtype=torch.int32, device=dev)
    gen = torch.Generator(device=dev).manual_seed(1)
    step = [0]

    def new():
        step[0] += 1
        s = datastore.subset_draw(counts, N_SURF, 1, 0, step[0], datastore.SURFACE)
        q = datastore.subset_draw(counts, N_SPACE, 1, 0, step[0], datastore.SPACE)
        return store.assemble(ids, s, q)

    def composed():
        c, s, t = ({k: v.index_select(0, ids[r].long()) for k, v in frames.items()} for r in range(3))
        return dataset.prepare_batch(data, c, s, t, generator=gen)

    def draw():
        step[0] += 1
        return datastore.subset_draw(counts, N_SURF, 1, 0, step[0], datastore.SURFACE)

    def sort():
        return dataset.random_subset(B, N_FULL, N_SURF, dev, gen)

    forms = [("new", new), ("composed", composed), ("draw", draw), ("sort", sort)]
    for _, fn in forms:
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    times = {name: [] for name, _ in forms}
    for _ in range(rounds):
        for name, fn in forms:
            times[name].append(_ms(fn, start, stop))
    for name, _ in forms:
        say(f"{name:9s} {_stats(times[name])}")
    # the assemble launch alone, and the bytes it moves: per kept surface row 3 records of 12 B + 4 B index (+ 0 noise) read and
    # 6 x 12 + 28 + 1 B written; per kept space row 3 records of 8 B + 4 B index read and 36 B written
    s_idx, q_idx = datastore.subset_draw(counts, N_SURF, 1, 0, 0, 0), datastore.subset_draw(counts, N_SPACE, 1, 0, 0, 1)
    alone = []
    for _ in range(rounds):
        alone.append(_ms(lambda: store.assemble(ids, s_idx, q_idx), start, stop))
    read = B * (N_SURF * (3 * 12 + 4) + N_SPACE * (3 * 8 + 4))
    written = B * (N_SURF * (72 + 28 + 1) + N_SPACE * 36)
    lines = B * 3 * (N_SURF + N_SPACE)
    med = statistics.median(alone)
    say(f"assemble  {_stats(alone)}   reads {read / 1e6:.1f} MB in {lines} records (64-byte lines: {lines * 64 / 1e6:.1f} MB), writes "
        f"{written / 1e6:.1f} MB: {(read + written) / med / 1e6:.1f} GB/s by bytes, {(lines * 64 + written) / med / 1e6:.1f} GB/s by lines")
    say(f"new / composed = {statistics.median(times['new']) / statistics.median(times['composed']):.4f}   "
        f"draw / sort = {statistics.median(times['draw']) / statistics.median(times['sort']):.4f}")


def _trainer(args, env):
    """One trainer run; (wall-clock time, epoch number, batches) of every 'epoch:' line of its log."""
    proc = subprocess.Popen([sys.executable, "-u", "-m", "nsdp_amd.train"] + args, cwd=ROOT, env=env, stdout=subprocess.PIPE,
                            stderr=subprocess.STDOUT, text=True)
    marks = []
    for line in proc.stdout:
        found = re.search(r"(?<!validation )epoch: (\d+) - batches: (\d+)", line)      # (a warning may share the line)
        if found:
            marks.append((time.perf_counter(), int(found.group(1)), int(found.group(2))))
    if proc.wait() != 0:
        raise RuntimeError(f"nsdp_amd.train {' '.join(args)} exited with {proc.returncode}")
    return marks


def trainer(data, work, runs, epochs, say):
    import yaml
    from nsdp_amd.config import default_config
    cfg = default_config("forward")
    cfg["model"]["encoder_kwargs"]["npoints_per_layer"] = [N_SURF, 500, 100]
    cfg["data"] = dict(data, num_surf_samples=N_SURF, num_space_samples=N_SPACE)      # (arbitrary pairs: 576 of them, 256 sampled)
    cfg["training"].update(epochs=epochs, save_frequency=10 ** 6, batch_size=B, iden_split="identity_seen", motion_split="train_seen",
                           num_sampled_pairs=8 * B, load_mesh=False)
    cfg["validation"] = {"frequency": 10 ** 6, "iden_split": "identity_seen", "motion_split": "test_unseen_motions", "batch_size": B,
                         "num_sampled_pairs": B, "load_mesh": False}
    path = os.path.join(work, "config.yaml")
    with open(path, "w") as f:
        yaml.safe_dump(cfg, f)
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    common = [path, os.path.join(work, "run"), "--graph", "--epochs", str(epochs)]
    forms = {"--synthetic": common + ["--synthetic", "8", "--batch", str(B), "--surface", str(N_SURF), "--queries", str(N_SPACE)],
             "--dataset": common + ["--dataset"]}
    per_step = {k: [] for k in forms}
    for r in range(runs):
        for name, args in forms.items():
            marks = _trainer(args, env)
            first = next(m for m in marks if m[1] >= 2)
            steps = (marks[-1][1] - first[1]) * marks[-1][2]
            per_step[name].append((marks[-1][0] - first[0]) * 1e3 / steps)
            say(f"train {name:11s} run {r}: {per_step[name][-1]:8.3f} ms/step over {steps} steps (epochs {first[1] + 1} .. {marks[-1][1]})")
    syn, dat = per_step["--synthetic"], per_step["--dataset"]
    say(f"train --synthetic --graph: {_stats(syn)} per step; spread between repeated runs {max(syn) - min(syn):.3f} ms")
    say(f"train --dataset   --graph: {_stats(dat)} per step; difference of the medians {statistics.median(dat) - statistics.median(syn):+.3f} ms")


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--dir", default=None, help="where the procedural tree is written (default: a temporary directory)")
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--train-runs", type=int, default=3, help="alternated runs of each trainer form (0: skip the trainer)")
    ap.add_argument("--train-epochs", type=int, default=12)
    ap.add_argument("--out", default=None, help="also append the lines to this file")
    args = ap.parse_args(argv)
    import numpy as np
    from nsdp_amd import synth
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    with tempfile.TemporaryDirectory() as tmp:
        root = args.dir or tmp
        t0 = time.perf_counter()
        # 4 identities x (1 training + 1 held-out motion) x 12 frames of 200 000 + 200 000 fp16 rows: arbitrary pairs of a training
        # sequence give 4 x 12 x 12 = 576 pairs over 48 frames
        data = synth.write_dataset_tree(root, ["ant", "bee", "cow", "doe"], ["walk", "jump"], 12, N_FULL, N_FULL, np.float16, seed=3)
        say(f"wrote the procedural tree in {time.perf_counter() - t0:.1f} s")
        data.update(arbitrary=True, num_surf_samples=N_SURF, num_space_samples=N_SPACE)
        kernels(data, args.rounds, say)
        if args.train_runs > 0:
            trainer(data, tmp, args.train_runs, args.train_epochs, say)
    if args.out:
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
