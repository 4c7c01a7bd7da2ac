"""What global gradient-norm clipping costs: HipAdam(max_grad_norm=) against HipAdam, in one process on one GPU, and the
replayed train step with and without ``training.clip_grad_norm``.

    python tools/bench_adam_clip.py [--replays 30000] [--window 1000] [--train-runs 3] [--train-epochs 12] [--out FILE]

The update alone: the parameter set of a TDNet (``build_model`` on the benchmark's configuration), random gradients, the optimizer
step captured (``GraphedStep``) and replayed -- unclipped (one launch: 4 reads + 3 writes of 4 bytes per element, 28 B) and
clipped (three launches: the norm pass reads the gradient again, 32 B).  Windows of ``--window`` replays between device events,
the two forms interleaved window by window until each has run ``--replays`` times, after one untimed window of each.  Reported:
microseconds per update (median and min-max of the windows), the bandwidth either implies, the measured ratio and the ratio
of the traffic, 32 / 28; then the kernels of one replay of either form timed one by one (``GraphedStep.timed_replay``).  A replay
is enqueued by one C call per replay; at these sizes the figures include what that costs.

The trainer: ``python -m nsdp_amd.train CONFIG DIR --synthetic 8 --graph`` at B = 32, 2048 surface samples, 8192 queries, with
and without ``--clip-grad-norm``, ``--train-runs`` alternated runs each, timed from its own log between the second and the last
"epoch:" line as tools/bench_datastore.py times it.  Medians and spreads; there is no pass / fail time.
"""
import argparse
import json
import os
import re
import statistics
import subprocess
import sys
import tempfile
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N_SURF, N_QUERY, B = 2048, 8192, 32


def _config():
    from nsdp_amd.config import default_config
    cfg = default_config("forward")
    cfg["model"]["encoder_kwargs"]["npoints_per_layer"] = [N_SURF, 500, 100]
    return cfg


def _stats(xs):
    return f"median {statistics.median(xs):8.3f}  min {min(xs):8.3f}  max {max(xs):8.3f}"


def update_alone(replays, window, say):
    from nsdp_amd.graph_step import GraphedStep
    from nsdp_amd.hip_adam import HipAdam
    from nsdp_amd.model import build_model
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    model, *_ = build_model(_config(), device=dev)
    shapes = [p.shape for p in model.parameters()]
    numel = sum(p.numel() for p in model.parameters())
    del model
    gen = torch.Generator(device=dev).manual_seed(1)
    forms = {}
    for name, kw in (("unclipped", {}), ("clipped", {"max_grad_norm": 1.0, "skip_nonfinite": True})):
        params = [torch.randn(s, device=dev, generator=gen).requires_grad_(True) for s in shapes]
        for p in params:
            p.grad = 1e-2 * torch.randn(p.shape, device=dev, generator=gen)
        opt = HipAdam(params, lr=1e-5, **kw)
        opt.step()                                      # (the state exists before the capture)
        step = GraphedStep(opt.step, max_streams=1, weights_change=False).capture(warmup=1)
        forms[name] = (step, opt, params)
    say(f"update alone: {len(shapes)} tensors, {numel} elements; graph nodes " +
        ", ".join(f"{k} {v[0].info['nodes']} ({v[0].info['kernels']} kernels)" for k, v in forms.items()))
    times = {k: [] for k in forms}

    def run(step):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(window):
            step()
        b.record()
        b.synchronize()
        return a.elapsed_time(b) * 1e3 / window       # microseconds per replay

    for step, _, _ in forms.values():
        run(step)
    for _ in range(max(1, replays // window)):
        for name, (step, _, _) in forms.items():
            times[name].append(run(step))
    st = forms["clipped"][1].grad_stats()
    say(f"clipped form after the run: {json.dumps(st)}")
    med = {k: statistics.median(v) for k, v in times.items()}
    for name, per in (("unclipped", 28), ("clipped", 32)):
        say(f"{name:9s} us per update: {_stats(times[name])}   {per} B/element: {per * numel / med[name] / 1e6:7.3f} TB/s")
    say(f"clipped / unclipped = {med['clipped'] / med['unclipped']:.3f} measured; traffic 32 / 28 = {32 / 28:.3f}; "
        f"difference {med['clipped'] - med['unclipped']:+.3f} us per step")
    # the kernels of ONE replay of either form with device events around each (serialised by the events: what every kernel takes
    # on its own, without the gaps between dependent launches that the windows above include)
    for name, (step, _, _) in forms.items():
        parts = {k: step.timed_replay(k) for k in ("grad_sumsq", "grad_clip_finalize", "adam_multi")}
        say(f"{name:9s} kernels of one replay, us: " + ", ".join(f"{k} x{n} {1e3 * ms:.2f}" for k, (n, ms) in parts.items()))
    for step, _, _ in forms.values():
        step.close()


def _trainer(args, env):
    """One trainer run; (wall-clock time, epoch number, batches) of every 'epoch: N - batches:' line of its log."""
    proc = subprocess.Popen([sys.executable, "-u", "-m", "nsdp_amd.train"] + args, cwd=ROOT, env=env, stdout=subprocess.PIPE,
                            stderr=subprocess.STDOUT, text=True)
    marks, last = [], ""
    for line in proc.stdout:
        found = re.search(r"(?<!validation )epoch: (\d+) - batches: (\d+)", line)
        if found:
            marks.append((time.perf_counter(), int(found.group(1)), int(found.group(2))))
        if "gradient norm" in line:
            last = line.strip()
    if proc.wait() != 0:
        raise RuntimeError(f"nsdp_amd.train {' '.join(args)} exited with {proc.returncode}")
    return marks, last


def trainer(work, runs, epochs, say):
    import yaml
    cfg = _config()
    cfg["training"].update(epochs=epochs, save_frequency=10 ** 6)
    cfg.setdefault("validation", {})["frequency"] = 10 ** 6
    path = os.path.join(work, "config.yaml")
    with open(path, "w") as f:
        yaml.safe_dump(cfg, f)
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    common = [path, None, "--graph", "--epochs", str(epochs), "--synthetic", "8", "--batch", str(B),
              "--surface", str(N_SURF), "--queries", str(N_QUERY)]
    forms = {"no key": common, "clip_grad_norm": common + ["--clip-grad-norm", "0.01", "--skip-nonfinite"]}
    per_step = {k: [] for k in forms}
    for r in range(runs):
        for name, args in forms.items():
            args = [args[0], os.path.join(work, f"run{r}_{name.replace(' ', '_')}")] + args[2:]      # (a directory of its own: no resume)
            marks, last = _trainer(args, env)
            first = next(m for m in marks if m[1] >= 2)
            steps = (marks[-1][1] - first[1]) * marks[-1][2]
            per_step[name].append((marks[-1][0] - first[0]) * 1e3 / steps)
            say(f"train {name:14s} run {r}: {per_step[name][-1]:8.3f} ms/step over {steps} steps" + (f"   [{last}]" if last else ""))
    plain, clip = per_step["no key"], per_step["clip_grad_norm"]
    say(f"train --graph, no key        : {_stats(plain)} ms per step; spread between repeated runs {max(plain) - min(plain):.3f} ms")
    say(f"train --graph, clip_grad_norm: {_stats(clip)} ms per step; spread {max(clip) - min(clip):.3f} ms; difference of the medians "
        f"{statistics.median(clip) - statistics.median(plain):+.3f} ms")


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--replays", type=int, default=30000)
    ap.add_argument("--window", type=int, default=1000)
    ap.add_argument("--train-runs", type=int, default=3, help="alternated runs of each trainer form (0: skip the trainer)")
    ap.add_argument("--train-epochs", type=int, default=12)
    ap.add_argument("--out", default=None, help="also append the lines to this file")
    args = ap.parse_args(argv)
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    update_alone(args.replays, args.window, say)
    torch.cuda.empty_cache()
    if args.train_runs > 0:
        with tempfile.TemporaryDirectory() as tmp:
            trainer(tmp, args.train_runs, args.train_epochs, say)
    if args.out:
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
