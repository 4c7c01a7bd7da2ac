"""Times a training batch sampled from the device-resident mesh store (nsdp_amd/meshstore.py) against the same batch composed from
torch ops and against ``SampleStore``'s batch of the same sizes, and ``python -m nsdp_amd.train --mesh-dataset --graph`` against
``--dataset --graph`` and ``--synthetic --graph``, on one GPU.

    python tools/bench_meshstore.py [--dir DIR] [--rounds 20] [--train-runs 3] [--out profiles/mesh_store.txt]

Shapes: bench.py's step -- B = 32, 2048 surface and 8192 space rows -- from frames of 20 002 vertices and 40 000 faces (a sphere
of 100 rings x 200 segments, ``synth.write_mesh_dataset_tree``), and, for ``SampleStore``, from the reference's pools of 100 000
surface and 200 000 space rows per frame in fp16 (``synth.write_dataset_tree``).  Kernel forms are timed with device events
after warm-up, ALTERNATED inside one loop (mesh, composed, pool, mesh, ...), median and range over the rounds, at several row
counts:

  mesh      one nsdp_mesh_batch_sample launch
  composed  the same batch from torch ops: randint + searchsorted on the thresholds, index gathers of the corners, the
            barycentric combination, cross and normalise, the offset, then dataset.prepare_batch (handle mask, inputs)
  pool      SampleStore's batch: two nsdp_subset_draw launches + one nsdp_batch_assemble launch

The trainer is timed as tools/bench_datastore.py times it (from its own log, between the second and the last "epoch:" line); the
three forms alternate and the spread between repeated runs of one form is the yardstick for their differences.
"""
import argparse
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from bench_datastore import _ms, _stats, _trainer      # noqa: E402  (tools/ is this script's directory)

B, N_SURF, N_SPACE = 32, 2048, 8192
RINGS, SEGMENTS = 100, 200
POOL_SURF, POOL_SPACE = 100000, 200000
IDENTITIES, MOTIONS, FRAMES = ["ant", "bee", "cow", "doe"], ["walk", "jump"], 12


def kernels(mesh_data, pool_data, rounds, say):
    import numpy as np
    import torch
    from nsdp_amd import dataset, datastore, meshstore
    dev = torch.device("cuda", 0)
    torch.zeros(1, device=dev)
    torch.cuda.synchronize()                                  # (the device is initialised before anything is timed)
    t0 = time.perf_counter()
    store = meshstore.MeshStore({"data": mesh_data}, "identity_seen", "train_seen", num_sampled_pairs=256, device=dev)
    torch.cuda.synchronize()
    load_s = time.perf_counter() - t0
    F = len(store.frames)
    V, NF = store.vert_arena.shape[0] // F, int(store.topo_table_host[0, 1])
    say(f"mesh store: {F} frames of {V} vertices, {store.topo_table.shape[0]} topologies of {NF} faces, {store.thr_rows // NF} canonical "
        f"frames with thresholds; {store.nbytes / 1e6:.2f} MB on the device = {store.nbytes / F / 1e6:.3f} MB per frame "
        f"({16 * V / 1e6:.3f} MB of vertices each); loaded in {load_s:.2f} s by {store._workers()} reader threads = "
        f"{load_s / F * 1e3:.1f} ms per frame; {len(store.pairs)} pairs formed, {len(store)} sampled")
    t0 = time.perf_counter()
    pool = datastore.SampleStore({"data": pool_data}, "identity_seen", "train_seen", num_sampled_pairs=256, device=dev)
    torch.cuda.synchronize()
    pool_s = time.perf_counter() - t0
    say(f"pool store: {len(pool.frames)} frames of {POOL_SURF} surface + {POOL_SPACE} space rows, {pool.surface_arena.dtype}; "
        f"{pool.nbytes / 1e6:.1f} MB on the device = {pool.nbytes / len(pool.frames) / 1e6:.2f} MB per frame; loaded in {pool_s:.2f} s = "
        f"{pool_s / len(pool.frames) * 1e3:.1f} ms per frame; bytes per frame, pool / mesh = {pool.nbytes / len(pool.frames) / (store.nbytes / F):.1f}")
    # frame-major tensors for the composition: what a torch-only mesh store would keep
    verts = store.vert_arena.view(F, V, 4)[..., :3].contiguous()
    faces = store.face_arena[:NF, :3].long().contiguous()
    cano_of = {k: i for i, k in enumerate(sorted(set(int(c) for c in store.pair_frames[:, 0])))}
    thr = (store.thr_arena.view(len(cano_of), NF).long() & 0xFFFFFFFF).contiguous()
    picks = np.asarray(store.sample_indices(0)[:B])
    ids_host = np.ascontiguousarray(store.pair_frames[picks].T)
    ids = torch.from_numpy(ids_host).to(dev)
    thr_rows = torch.tensor([cano_of[int(c)] for c in ids_host[0]], device=dev)
    pool_ids = torch.from_numpy(np.ascontiguousarray(pool.pair_frames[np.asarray(pool.sample_indices(0)[:B])].T)).to(dev)
    counts_s = torch.full((B,), POOL_SURF, dtype=torch.int32, device=dev)
    counts_q = torch.full((B,), POOL_SPACE, dtype=torch.int32, device=dev)
    gen = torch.Generator(device=dev).manual_seed(1)
    step = [0]
    sigma = torch.tensor([0.1, 0.02], device=dev)
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for n, m in ((N_SURF, N_SPACE), (256, 1024), (8192, 32768)):
        store.n, store.m, pool.n, pool.m = n, m, n, m
        data = dict(mesh_data, num_surf_samples=n, num_space_samples=m)
        half = (torch.arange(m, device=dev) >= m // 2).long()
        rows_id = torch.arange(n, dtype=torch.int32, device=dev).repeat(B, 1).contiguous()

        def mesh():
            step[0] += 1
            return store.assemble(ids, 1, 0, step[0])

        def composed():
            r = torch.randint(0, 1 << 31, (B, n + m), device=dev, generator=gen)
            f = torch.searchsorted(thr[thr_rows], r, right=True).clamp_(max=NF - 1)
            corner = faces[f]                                                              # (B, rows, 3)
            uv = torch.rand((2, B, n + m, 1), device=dev, generator=gen)
            flip = uv.sum(0) > 1.0
            u, v = torch.where(flip, 1.0 - uv[0], uv[0]), torch.where(flip, 1.0 - uv[1], uv[1])
            d = (2.0 * torch.rand((B, m, 1), device=dev, generator=gen) - 1.0) * sigma[half][None, :, None]
            clouds = []
            for c in range(3):
                vb = verts.index_select(0, ids[c].long())                                  # (B, V, 3)
                a, b, cc = (torch.gather(vb, 1, corner[..., k:k + 1].expand(-1, -1, 3)) for k in range(3))
                p = (1.0 - u - v) * a + u * b + v * cc
                nrm = torch.linalg.cross(b - a, cc - a)
                nrm = nrm / nrm.norm(dim=-1, keepdim=True).clamp_min(1e-30)
                clouds.append({"surface_samples": p[:, :n], "surface_normals": nrm[:, :n], "space_samples": p[:, n:] + nrm[:, n:] * d})
            return dataset.prepare_batch(data, clouds[0], clouds[1], clouds[2], rows_id)

        def pooled():
            step[0] += 1
            s = datastore.subset_draw(counts_s, n, 1, 0, step[0], datastore.SURFACE)
            q = datastore.subset_draw(counts_q, m, 1, 0, step[0], datastore.SPACE)
            return pool.assemble(pool_ids, s, q)

        forms = [("mesh", mesh), ("composed", composed), ("pool", pooled)]
        for _, fn in forms:
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        times = {name: [] for name, _ in forms}
        for _ in range(rounds):
            for name, fn in forms:
                times[name].append(_ms(fn, start, stop))
        say(f"B = {B}, n = {n}, m = {m}:")
        for name, _ in forms:
            say(f"  {name:9s} {_stats(times[name])}")
        med = {k: statistics.median(v) for k, v in times.items()}
        # per row: ~16 threshold probes of 4 B, one 16-B face, nine 16-B vertices; written: 101 B per surface row, 36 B per space row
        written = B * (n * (72 + 28 + 1) + m * 36)
        gathers = B * (n + m) * 10
        say(f"  mesh / composed = {med['mesh'] / med['composed']:.4f}   mesh / pool = {med['mesh'] / med['pool']:.3f}   "
            f"mesh: {gathers} 16-byte gathers and {written / 1e6:.1f} MB written = {(gathers * 64 + written) / med['mesh'] / 1e6:.0f} GB/s by lines")
    store.n, store.m, pool.n, pool.m = N_SURF, N_SPACE, N_SURF, N_SPACE


def trainer(mesh_data, pool_data, work, runs, epochs, say):
    import yaml
    from nsdp_amd.config import default_config
    paths = {}
    for name, data in (("mesh", mesh_data), ("pool", pool_data)):
        cfg = default_config("forward")
        cfg["model"]["encoder_kwargs"]["npoints_per_layer"] = [N_SURF, 500, 100]
        cfg["data"] = dict(data, num_surf_samples=N_SURF, num_space_samples=N_SPACE)      # (arbitrary pairs: 576 of them, 256 sampled)
        cfg["training"].update(epochs=epochs, save_frequency=10 ** 6, batch_size=B, iden_split="identity_seen", motion_split="train_seen",
                               num_sampled_pairs=8 * B, load_mesh=False)
        cfg["validation"] = {"frequency": 10 ** 6, "iden_split": "identity_seen", "motion_split": "test_unseen_motions", "batch_size": B,
                             "num_sampled_pairs": B, "load_mesh": False}
        paths[name] = os.path.join(work, f"config_{name}.yaml")
        with open(paths[name], "w") as f:
            yaml.safe_dump(cfg, f)
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    tail = [os.path.join(work, "run"), "--graph", "--epochs", str(epochs)]
    forms = {"--synthetic": [paths["mesh"]] + tail + ["--synthetic", "8", "--batch", str(B), "--surface", str(N_SURF), "--queries", str(N_SPACE)],
             "--dataset": [paths["pool"]] + tail + ["--dataset"], "--mesh-dataset": [paths["mesh"]] + tail + ["--mesh-dataset"]}
    per_step = {k: [] for k in forms}
    for r in range(runs):
        for name, args in forms.items():
            marks = _trainer(args, env)
            first = next(m for m in marks if m[1] >= 2)
            steps = (marks[-1][1] - first[1]) * marks[-1][2]
            per_step[name].append((marks[-1][0] - first[0]) * 1e3 / steps)
            say(f"train {name:14s} run {r}: {per_step[name][-1]:8.3f} ms/step over {steps} steps (epochs {first[1] + 1} .. {marks[-1][1]})")
    syn = statistics.median(per_step["--synthetic"])
    for name, xs in per_step.items():
        say(f"train {name:14s} --graph: {_stats(xs)} per step; spread between repeated runs {max(xs) - min(xs):.3f} ms; "
            f"median - synthetic's {statistics.median(xs) - syn:+.3f} ms")


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--dir", default=None, help="where the procedural trees are written (default: a temporary directory)")
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
        sphere = synth.sphere_mesh(RINGS, SEGMENTS)
        mesh_data = synth.write_mesh_dataset_tree(os.path.join(root, "meshes"), {k: sphere for k in IDENTITIES}, MOTIONS, FRAMES, seed=3)
        t1 = time.perf_counter()
        pool_data = synth.write_dataset_tree(os.path.join(root, "pools"), IDENTITIES, MOTIONS, FRAMES, POOL_SURF, POOL_SPACE, np.float16, seed=3)
        say(f"wrote the mesh tree in {t1 - t0:.1f} s and the pool tree in {time.perf_counter() - t1:.1f} s")
        for data in (mesh_data, pool_data):
            data.update(arbitrary=True, num_surf_samples=N_SURF, num_space_samples=N_SPACE)
        kernels(mesh_data, pool_data, args.rounds, say)
        if args.train_runs > 0:
            trainer(mesh_data, pool_data, tmp, args.train_runs, args.train_epochs, say)
    if args.out:
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
