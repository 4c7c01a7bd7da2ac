"""Training harness around the MI355X TDNet path with the loop semantics of the reference's train.py (SURVEY.md
section 8 next-1): seeding, epoch-wise step learning rate, checkpoint cadence, validation cadence and best-model
tracking are the reference's; the model, its train/validate functions and the optimizer come from
``nsdp_amd.model``.  The data loader is whatever yields the reference's ``data_dict`` batches: ``--dataset`` trains from the
data set on disk that ``config["data"]`` names (nsdp_amd.datastore: the reference's directory layout and pair rules, every
frame resident on the device, the splits and batch sizes of the config's ``training`` / ``validation`` sections as in the
reference's train.py:105-135); ``--mesh-dataset`` trains from the MESH sequences of the same layout (nsdp_amd.meshstore:
``data["mesh_file"]`` of every frame resident on the device, surface and space rows sampled afresh inside every batch's launch:
no pre-sampled point files); ``--synthetic`` (the default) uses procedural batches.  Training reads no whole meshes
(``load_mesh``) and not the user-handle data sets (``tosca``, ``dogrec``): those belong to evaluation, ``python -m
nsdp_amd.evaluate CONFIG`` (the test split from the mesh store in packed whole-mesh batches; the reference's test.py and run.py).
Not read from disk at all: partial shapes, and a data set larger than the device's memory.

    python -m nsdp_amd.train config.yaml experiment_dir [--synthetic 4] [--epochs 2]
    python -m nsdp_amd.train config.yaml experiment_dir --dataset [--graph] [--gpus N]
    python -m nsdp_amd.train config.yaml experiment_dir --mesh-dataset [--graph] [--gpus N]
"""
from __future__ import annotations

import argparse
import os
import sys

import numpy as np
import torch

from .checkpoints import load_best_checkpoints, load_checkpoints, save_best_checkpoints, save_checkpoints
from .model import build_model, optimizer_factory
from .model.learningrate import adjust_learning_rate


def seed_everything(seed: int):
    """train.py:68-72: numpy seeds torch, which seeds every GPU."""
    np.random.seed(seed)
    torch.manual_seed(np.random.randint(np.iinfo(np.int32).max))
    if torch.cuda.is_available():
        torch.cuda.manual_seed_all(np.random.randint(np.iinfo(np.int32).max))


class _Average:
    """Running mean of the batch losses of an epoch (utils/logger.py AverageAggregator)."""

    def __init__(self):
        self.total, self.count = 0.0, 0

    def add(self, v):
        self.total += float(v)
        self.count += 1

    @property
    def value(self):
        return self.total / max(self.count, 1)


def fit(model, fns, lr_scheduler, optimizer, train_loader, val_loader, config, experiment_directory, args, device,
        log=print, dp=None):
    """train.py:150-225.  ``fns`` = (train_on_batch, validate_on_batch) from build_model; ``args`` carries
    ``continue_from_epoch`` and ``best_val_loss`` (both updated by the checkpoint loaders and by this loop).
    ``dp``: a nsdp_amd.parallel.DataParallel -- this process is one rank of a data-parallel job (the reference is
    single-process, train.py:74-75): batches are sharded over the ranks, ``train_on_batch`` gets the gradient exchange in
    front of its optimizer step (unless it already carries one: GraphedTrainOnBatch(reducer=...)), epoch / validation
    losses are means over ranks, rank 0 writes the files.  The policy (BatchNorm buffers included) is DataParallel's
    docstring."""
    train_on_batch, validate_on_batch = fns
    load_best_checkpoints(model, experiment_directory, args, device)   # best first, then the latest (train.py:153-156)
    load_checkpoints(model, optimizer, experiment_directory, args, device)
    main = dp is None or dp.is_main
    if dp is not None:
        dp.broadcast_model(model)
        if not getattr(train_on_batch, "exchanges_gradients", False):
            train_on_batch = dp.wrap(train_on_batch)
    epochs = config["training"].get("epochs", 1000)
    save_every = config["training"].get("save_frequency", 20)
    val_every = config["validation"].get("frequency", 10)
    history = []
    for i in range(args.continue_from_epoch, epochs):
        adjust_learning_rate(lr_scheduler, optimizer, i)
        model.train()
        avg = _Average()
        if getattr(train_on_batch, "accepts_next_batch", False):
            # one batch of look-ahead: the step computes the NEXT batch's index sets beside itself (graph_step.PipelinedGeometry)
            nxt = None
            for sample in _with_next(train_loader if dp is None else dp.shard(train_loader), device):
                cur, nxt = sample
                avg.add(train_on_batch(model, optimizer, cur, config, next_data_dict=nxt))
        else:
            for b, sample in enumerate(train_loader if dp is None else dp.shard(train_loader)):
                sample = {k: v.to(device) for k, v in sample.items()}
                avg.add(train_on_batch(model, optimizer, sample, config))
        epoch_loss = avg.value if dp is None else dp.mean(avg.value, device)
        if main:
            log("epoch: {} - batches: {} - loss: {:.5f}".format(i + 1, avg.count, epoch_loss))
        # (training.clip_grad_norm / skip_nonfinite_steps: ONE read of the optimizer's statistics per epoch, never per step;
        # under dp every rank holds the same numbers -- the same averaged gradient, the same fixed-order sum.  None: an
        # optimizer that could clip but was built without the keys)
        st = optimizer.grad_stats() if main and hasattr(optimizer, "grad_stats") else None
        if st is not None:
            log("epoch: {} - gradient norm (last step): {:.5g} - clipped {} / {} steps - skipped {}".format(
                i + 1, st["norm"], st["clipped"], st["steps"], st["skipped"]))
        history.append(("train", i, epoch_loss))
        want_val = i % val_every == 0 and i > 0
        if dp is not None and ((i % save_every) == 0 or want_val):
            dp.broadcast_buffers(model)          # rank 0's BatchNorm statistics are the model's
        if (i % save_every) == 0 and main:
            save_checkpoints(i, model, optimizer, experiment_directory)
        if want_val:
            model.eval()
            vavg = _Average()
            for b, sample in enumerate(val_loader if dp is None else dp.shard(val_loader)):
                sample = {k: v.to(device) for k, v in sample.items()}
                vavg.add(validate_on_batch(model, sample, config))
            val_loss = vavg.value if dp is None else dp.mean(vavg.value, device)
            if main:
                log("validation epoch: {} - loss: {:.5f}".format(i + 1, val_loss))
            history.append(("val", i, val_loss))
            if val_loss < args.best_val_loss:      # (the same number on every rank: same decision everywhere)
                if main:
                    save_best_checkpoints(i, model, experiment_directory, val_loss)
                args.best_val_loss = val_loss
    return history


def _with_next(loader, device):
    """(batch, next batch or None) pairs of ``loader``, both on ``device``."""
    it = iter(loader)
    try:
        cur = {k: v.to(device) for k, v in next(it).items()}
    except StopIteration:
        return
    for sample in it:
        nxt = {k: v.to(device) for k, v in sample.items()}
        yield cur, nxt
        cur = nxt
    yield cur, None


class SyntheticLoader:
    """``n_batches`` procedural data_dict batches per epoch (same generator as bench.py and the parity fixtures).
    ``uncorresponded = m`` (1 <= m <= n_query): targets without correspondences, for a correspondence-free loss
    (``training.loss: chamfer``) -- ``space_samples_tgt`` becomes ``[batch, m, 3]``, the first ``m`` rows of a procedural
    permutation (one per shape) of the corresponded targets: another order and, for m < n_query, another count."""

    def __init__(self, seed, n_batches, batch, n_surf=2048, n_query=8192, uncorresponded=None):
        from . import synth
        if uncorresponded is not None and not 1 <= int(uncorresponded) <= n_query:
            raise ValueError(f"SyntheticLoader: uncorresponded={uncorresponded} target rows must be in [1, n_query={n_query}]")
        self.batches = []
        for i in range(n_batches):
            data = synth.make_batch(seed + i, batch, n_surf, n_query)
            if uncorresponded is not None:
                order = np.argsort(synth.uniform01(seed + i, "uncorresponded", (batch, n_query)), axis=1, kind="stable")
                data["space_samples_tgt"] = np.take_along_axis(data["space_samples_tgt"], order[:, :int(uncorresponded), None], axis=1)
            self.batches.append({k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in data.items()})

    def __iter__(self):
        return iter(self.batches)

    def __len__(self):
        return len(self.batches)

    def shard(self, rank, world_size):
        """This rank's share of an epoch (DataParallel.shard asks for it): of every ``world_size`` consecutive batches the
        rank-th; a trailing partial group is dropped so that all ranks take the same number of steps."""
        groups = len(self.batches) // world_size
        return (self.batches[g * world_size + rank] for g in range(groups))


def initial_weight_files(config, args=None):
    """train.py:140-146: the three weight files that initialise the networks come from the config's ``training``
    section (``weight_file``, ``weight_forward_file``, ``weight_backward_file``); a command-line value, where given,
    overrides the config's.  Returns (weight_file, weight_forward_file, weight_backward_file)."""
    out = []
    for key in ("weight_file", "weight_forward_file", "weight_backward_file"):
        v = config.get("training", {}).get(key, None)
        cli = getattr(args, key, None) if args is not None else None
        out.append(cli if cli is not None else v)
    return tuple(out)


def launch_ranks(n, argv, module="nsdp_amd.train"):
    """``python -m nsdp_amd.train ... --gpus N`` from a bare shell: start the N ranks through torch.distributed.run on
    127.0.0.1 and a free port (rank r -> GPU r); the children see RANK / WORLD_SIZE and take the worker path of main().
    ``module``: the entry point the ranks run (nsdp_amd.infer launches its ranks the same way)."""
    import socket
    import subprocess
    with socket.socket() as sock:
        sock.bind(("127.0.0.1", 0))
        port = sock.getsockname()[1]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")     # dmabuf IPC: what RCCL needs on this driver
    env.setdefault("OMP_NUM_THREADS", str(max(1, 16 // n)))
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={n}", "--master-addr", "127.0.0.1",
           "--master-port", str(port), "-m", module] + list(argv)
    return subprocess.call(cmd, env=env)


def main(argv=None):
    import yaml
    argv = list(sys.argv[1:] if argv is None else argv)
    ap = argparse.ArgumentParser(description="Train a deformation network on MI355X")
    ap.add_argument("config_file")
    ap.add_argument("experiment_directory")
    ap.add_argument("--weight_file", default=None, help="overrides training.weight_file of the config")
    ap.add_argument("--weight_forward_file", default=None, help="overrides training.weight_forward_file")
    ap.add_argument("--weight_backward_file", default=None, help="overrides training.weight_backward_file")
    ap.add_argument("--continue_from_epoch", default=0, type=int)
    ap.add_argument("--seed", type=int, default=27)
    ap.add_argument("--synthetic", type=int, default=None, help="procedural batches per epoch (default 4; not with --dataset)")
    ap.add_argument("--dataset", action="store_true",
                    help="train from the data set on disk that the config's data section names (dataset_dir, split_dir, type "
                         "deform4d / deformtransfer): splits, num_sampled_pairs and batch_size come from its training / validation "
                         "sections; every frame is held on the device (each rank holds all of them).  Not with --synthetic; "
                         "--batch, --surface, --queries and --uncorresponded describe procedural batches and are not used")
    ap.add_argument("--mesh-dataset", dest="mesh_dataset", action="store_true",
                    help="train from the mesh sequences that the config's data section names (as --dataset, with data.mesh_file "
                         "in every frame directory instead of the pre-sampled point files): every frame's vertices are held on "
                         "the device and num_surf_samples / num_space_samples rows are sampled afresh for every batch "
                         "(data.space_sigma: the two offsets of the space rows, default [0.1, 0.02]).  Not with --dataset or "
                         "--synthetic")
    ap.add_argument("--batch", type=int, default=8, help="shapes per batch = per GPU and step (the global batch is this x --gpus)")
    ap.add_argument("--surface", type=int, default=2048, help="surface samples per shape of the procedural batches (default 2048)")
    ap.add_argument("--queries", type=int, default=8192, help="query points per shape of the procedural batches (default 8192)")
    ap.add_argument("--uncorresponded", type=int, default=None, metavar="M",
                    help="procedural targets without correspondences: M permuted target rows per shape (1 <= M <= --queries); "
                         "needs a correspondence-free loss (training.loss: chamfer)")
    ap.add_argument("--epochs", type=int, default=None)
    ap.add_argument("--graph", action="store_true",
                    help="capture the train step once and replay it (nsdp_amd.graph_step.GraphedTrainOnBatch): batches of "
                         "one fixed shape replay, others run eagerly; the sequence of optimizer steps is the eager loop's")
    ap.add_argument("--gpus", type=int, default=None,
                    help="data-parallel ranks, one process per GPU (nsdp_amd.parallel.DataParallel: batches sharded over the "
                         "ranks, one RCCL all-reduce of the flat gradient per step, rank-0 checkpoints).  From a bare shell "
                         "the ranks are launched here; under torchrun (RANK / WORLD_SIZE set) this process is one of them")
    ap.add_argument("--backend", default="nccl", help="torch.distributed backend of the data-parallel job (nccl = RCCL)")
    ap.add_argument("--clip-grad-norm", dest="clip_grad_norm", type=float, default=None, metavar="X",
                    help="overrides training.clip_grad_norm: a bound X > 0 on the L2 norm of all gradients together, applied "
                         "inside the optimizer step (after the data-parallel exchange); the gradients themselves are not rewritten")
    ap.add_argument("--skip-nonfinite", dest="skip_nonfinite", action="store_true",
                    help="sets training.skip_nonfinite_steps: a step whose gradient holds an inf or a NaN changes no weight and no "
                         "optimizer state, and is counted in the per-epoch gradient line")
    args = ap.parse_args(argv)
    if args.dataset and args.synthetic is not None:
        sys.exit(f"nsdp_amd.train: --dataset and --synthetic {args.synthetic} were given together; choose one source of batches")
    if args.mesh_dataset and args.dataset:
        sys.exit("nsdp_amd.train: --mesh-dataset and --dataset were given together; choose one source of batches")
    if args.mesh_dataset and args.synthetic is not None:
        sys.exit(f"nsdp_amd.train: --mesh-dataset and --synthetic {args.synthetic} were given together; choose one source of batches")
    if args.synthetic is None:
        args.synthetic = 4
    if args.surface < 1 or args.queries < 1:
        sys.exit(f"nsdp_amd.train: --surface {args.surface} and --queries {args.queries} must be positive")
    if args.uncorresponded is not None and not 1 <= args.uncorresponded <= args.queries:
        sys.exit(f"nsdp_amd.train: --uncorresponded {args.uncorresponded} must be in [1, --queries {args.queries}]")
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if args.gpus is not None and args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        return launch_ranks(args.gpus, argv)
    if args.gpus is not None and args.gpus != world:
        sys.exit(f"nsdp_amd.train: --gpus {args.gpus} but the launcher's WORLD_SIZE is {world}")
    rank, local_rank = int(os.environ.get("RANK", "0")), int(os.environ.get("LOCAL_RANK", "0"))
    args.best_val_loss = float("inf")
    seed_everything(args.seed)           # (the same seed on every rank: identical initial weights even before the broadcast)
    device = torch.device("cuda", 0)
    if world > 1:
        import torch.distributed as dist
        from .parallel import rank_device
        index, cpus = rank_device(local_rank, world, args.backend)       # rank r -> GPU r, pinned to its CPU slice
        device = torch.device("cuda", index)
        print(f"nsdp_amd.train: rank {rank} -> GPU {index}, CPUs {cpus}", file=sys.stderr)
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if args.backend == "nccl":
            dist.init_process_group("nccl", rank=rank, world_size=world, device_id=device)
        else:
            dist.init_process_group(args.backend, rank=rank, world_size=world)
    with open(args.config_file) as f:
        config = yaml.safe_load(f)
    if args.epochs is not None:
        config["training"]["epochs"] = args.epochs
    if args.clip_grad_norm is not None:
        config["training"]["clip_grad_norm"] = args.clip_grad_norm
    if args.skip_nonfinite:
        config["training"]["skip_nonfinite_steps"] = True
    os.makedirs(args.experiment_directory, exist_ok=True)
    weights = initial_weight_files(config, args)
    say = print if rank == 0 else (lambda *a, **k: None)
    for key, path in zip(("weight_file", "weight_forward_file", "weight_backward_file"), weights):
        if path is not None:
            say("initialising from {} = {}".format(key, path))
    if config["model"]["type"] == "arbitrary" and weights[1] is None and weights[2] is None and weights[0] is None:
        say("WARNING: FlowArbitrary starts from random weights (no weight_forward_file / weight_backward_file in the "
            "config's training section or on the command line)")
    model, train_fn, val_fn, _ = build_model(config, *weights, device=device)
    lr_scheduler, optimizer = optimizer_factory(config["training"], model.parameters())
    dp = None
    if world > 1:
        from .parallel import DataParallel
        dp = DataParallel(model, rank, world)
    if args.graph:
        from .graph_step import GraphedTrainOnBatch
        train_fn = GraphedTrainOnBatch(train_fn, reducer=dp.reducer if dp is not None else None)
    if args.dataset:
        train, val = dataset_loaders(config, args.seed, device, log=say)
    elif args.mesh_dataset:
        train, val = mesh_dataset_loaders(config, args.seed, device, log=say)
    else:
        train, val = synthetic_loaders(args, world)
    fit(model, (train_fn, val_fn), lr_scheduler, optimizer, train, val, config, args.experiment_directory, args, device,
        log=say, dp=dp)
    if dp is not None:
        import torch.distributed as dist
        ok = dp.in_sync(model)
        say("ranks in sync after training: {}".format(ok))
        dist.destroy_process_group()
        if not ok:
            return 1
    return 0


def _store_loaders(store_class, frames, config, seed, device, log):
    """(train loader, validation loader) over two device-resident stores of ``store_class``; ``frames``: how the log line counts
    a store's frames and megabytes.  Every rank builds both stores whole and takes its share of the batches (StoreLoader.shard);
    the validation loader does not shuffle."""
    loaders = []
    for section, default_batch in (("training", 16), ("validation", 1)):
        sec = config[section]
        store = store_class(config, sec["iden_split"], sec["motion_split"], num_sampled_pairs=sec.get("num_sampled_pairs", -1),
                            device=device, load_mesh=sec.get("load_mesh", False))
        log(("Loaded {} {} deformation pairs (" + frames + " on the device)").format(len(store), section, len(store.frames),
                                                                                   store.nbytes / 1e6))
        loaders.append(store.loader(sec.get("batch_size", default_batch), seed if section == "training" else seed + 10000,
                                    noise_generator=None, shuffle=section == "training"))
    return tuple(loaders)


def dataset_loaders(config, seed, device, log=print):
    """The reference's train.py:105-135 over device-resident stores of pre-sampled frames (nsdp_amd.datastore)."""
    from .datastore import SampleStore
    return _store_loaders(SampleStore, "{} frames, {:.1f} MB", config, seed, device, log)


def mesh_dataset_loaders(config, seed, device, log=print):
    """``dataset_loaders`` over device-resident MESH stores (nsdp_amd.meshstore): the same splits, batch sizes, seeds and shuffling."""
    from .meshstore import MeshStore
    return _store_loaders(MeshStore, "{} mesh frames, {:.2f} MB", config, seed, device, log)


def synthetic_loaders(args, world):
    # (one loader of world x synthetic batches: every rank builds the same list and takes its share, DataParallel.shard)
    targets = {} if args.uncorresponded is None else {"uncorresponded": args.uncorresponded}
    train = SyntheticLoader(args.seed, args.synthetic * world, args.batch, n_surf=args.surface, n_query=args.queries, **targets)
    val = SyntheticLoader(args.seed + 10000, max(1, args.synthetic // 4) * world, args.batch, n_surf=args.surface,
                          n_query=args.queries, **targets)
    return train, val


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
