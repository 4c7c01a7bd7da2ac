"""The ray cast (nsdp_amd/ray_cast.py, include/nsdp_raycast.h) in its forms, in one process on one GPU.

    python tools/bench_raycast.py [--reps 5] [--reps-plain 3] [--only NAME[,NAME...]] [--out profiles/ray_cast.txt]

Meshes: the torus grids of tools/bench_surface.py (closed, rows in grid order; the plan's Morton order is applied as a user
would get it).  Inputs:

    four_100k        4 x 100 000 rays against 4 x 200 000 faces
    four_large       the 278 160-vertex ragged set (100000, 61234, 35007, 81919 vertices), as many rays as vertices
    eight_small      eight meshes of 5000, 3100, 7200, 1800, 6400, 2500, 4100, 3900 vertices, as many rays as vertices
    collapsed        100 000 rays against 200 000 faces shrunk to 1e-4 of their size: every block box sits on every ray aimed at it
    thin_along       100 000 rays along the axis of a mesh squeezed to 1 % in y and z: every block lies on the rays' line
    sweep_*          one mesh of F faces with F / 2 rays, F = 2^11 .. 2^17: either side of the default dispatch's threshold

with two bundles each: ``camera`` (one eye per mesh outside it, rays towards points of the surface and a few past it) and
``contains`` (origins uniform in the mesh's box, one direction).  For every input and bundle one JSON line: the median and
min-max in ms of one ``cast_rays`` call, HIP events around every call, the forms interleaved (form 1, form 2, ..., form 1, ...)
after one untimed call of each:

    first_cull / first_plain     first-hit mode (count=False): culling by blocks, depth culling too, rays as given / the plain scan
    count_cull / count_plain     counting mode (count=True)
    ..._cull+reorder             the culled form behind the wrapper's reordering of the rays (the sort is inside the timed call)
    default                      what cast_rays picks by itself (counting mode)

``--evaluate`` adds one line: ``evaluate`` pairs/s with and without ``test.volume_iou`` on a synthetic tree (``evaluate_case``).

``same_bytes``: t and crossings of every form equal the plain scan's bit for bit.  Beside them, for scale: ``closest_ms``, one
``closest_on_mesh`` call with the origins as queries (its default form), and ``torch_mt_ms``, a chunked Moeller-Trumbore test
composed from torch ops (fp32, no exactness of any kind: what one would write without the kernel) on the FIRST ``mt_rays`` rays
of every mesh -- it is too slow to run on all of them; ``torch_mt_ms_scaled`` is that time scaled to all rays.
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from bench_surface import EIGHT_SMALL, FOUR_LARGE, torus           # noqa: E402
from nsdp_amd import ray_cast, surface_distance                    # noqa: E402
from nsdp_amd.ragged import RaggedPoints                           # noqa: E402

DEV = torch.device("cuda:0")
MT_RAYS = 2048


def bundle(kind, v, f, n, seed, direction=(0.0, 0.0, 1.0)):
    """(origins, dirs) [n, 3] for one mesh."""
    g = torch.Generator(device=DEV).manual_seed(seed)
    lo, hi = v.amin(dim=0), v.amax(dim=0)
    if kind == "contains":
        o = lo + torch.rand(n, 3, device=DEV, generator=g) * (hi - lo)
        return o.contiguous(), torch.tensor(direction, device=DEV).expand(n, 3).contiguous()
    eye = (lo + hi) / 2 + torch.tensor([0.3, -0.5, 2.5], device=DEV) * (hi - lo).max()
    rows = f[torch.randint(0, f.shape[0], (n,), device=DEV, generator=g)].long()
    target = (v[rows[:, 0]] + v[rows[:, 1]] + v[rows[:, 2]]) / 3 + 0.2 * (hi - lo) * torch.randn(n, 3, device=DEV, generator=g) * \
        (torch.rand(n, 1, device=DEV, generator=g) < 0.1)
    return eye.expand(n, 3).contiguous(), (target - eye).contiguous()


def make(name, kind):
    """-> (origins, dirs, verts, faces) in a layout cast_rays takes."""
    if name == "four_100k":
        meshes = [torus(100000, 10 + b) for b in range(4)]
        rays = [bundle(kind, v, f, 100000, 20 + b) for b, (v, f) in enumerate(meshes)]
        return (torch.stack([o for o, _ in rays]), torch.stack([d for _, d in rays]), torch.stack([v for v, _ in meshes]),
                torch.stack([f for _, f in meshes]))
    if name in ("four_large", "eight_small"):
        counts = FOUR_LARGE if name == "four_large" else EIGHT_SMALL
        meshes = [torus(V, 30 + b) for b, V in enumerate(counts)]
        rays = [bundle(kind, v, f, V, 40 + b) for b, ((v, f), V) in enumerate(zip(meshes, counts))]
        return (RaggedPoints.from_list([o for o, _ in rays]), RaggedPoints.from_list([d for _, d in rays]),
                RaggedPoints.from_list([v for v, _ in meshes]), RaggedPoints.from_rows([f for _, f in meshes]))
    if name.startswith("sweep_"):
        F = int(name[6:])
        v, f = torus(F // 2, 54)
        o, d = bundle(kind, v, f, F // 2, 55)
        return o, d, v, f
    v, f = torus(100000, 50)
    if name == "collapsed":
        v = ((v - v.mean(dim=0)) * 1e-4 + v.mean(dim=0)).contiguous()
        o, d = bundle("camera", v, f, 100000, 52)
        if kind == "contains":                      # one direction, from far outside, through the collapsed mesh
            o = (v.mean(dim=0) - torch.tensor([0.0, 0.0, 3.0], device=DEV) + 2e-4 * (torch.rand(100000, 3, device=DEV) - 0.5)).contiguous()
            d = torch.tensor([0.0, 0.0, 1.0], device=DEV).expand(100000, 3).contiguous()
        return o, d, v, f
    if name == "thin_along":
        c = v.mean(dim=0)
        v = ((v - c) * torch.tensor([1.0, 0.01, 0.01], device=DEV) + c).contiguous()
        return bundle("contains", v, f, 100000, 53, direction=(1.0, 0.0, 0.0)) + (v, f)
    raise SystemExit(f"unknown input {name}")


FORMS = (("default", {"count": True}), ("first_cull", {"count": False, "cull": True, "reorder": False}),
         ("first_cull+reorder", {"count": False, "cull": True, "reorder": True}), ("first_plain", {"count": False, "cull": False}),
         ("count_cull", {"count": True, "cull": True, "reorder": False}), ("count_cull+reorder", {"count": True, "cull": True, "reorder": True}),
         ("count_plain", {"count": True, "cull": False}))


def _time(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), out


def _packed(x):
    return x.packed if isinstance(x, RaggedPoints) else x


def torch_mt(o, d, tri, chunk=256):
    """A chunked Moeller-Trumbore first hit + crossing count from torch ops: o, d [n, 3], tri [F, 3, 3] -> (t [n], count [n])."""
    e1, e2, v0 = tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0], tri[:, 0]
    ts, cs = [], []
    for lo in range(0, o.shape[0], chunk):
        oc, dc = o[lo:lo + chunk, None], d[lo:lo + chunk, None]
        p = torch.cross(dc.expand(-1, e2.shape[0], -1), e2[None].expand(dc.shape[0], -1, -1), dim=-1)
        det = (e1[None] * p).sum(-1)
        inv = 1.0 / det
        s = oc - v0[None]
        u = (s * p).sum(-1) * inv
        q = torch.cross(s, e1[None].expand(s.shape[0], -1, -1), dim=-1)
        w = (dc * q).sum(-1) * inv
        t = (e2[None] * q).sum(-1) * inv
        hit = (det.abs() > 1e-12) & (u >= 0) & (w >= 0) & (u + w <= 1) & (t > 0)
        ts.append(torch.where(hit, t, torch.full_like(t, float("inf"))).amin(dim=1))
        cs.append(hit.sum(dim=1))
    return torch.cat(ts), torch.cat(cs)


def per_mesh(o, d, v, f):
    """The operands as lists of single meshes (for the torch composition)."""
    if isinstance(o, RaggedPoints):
        return list(zip(o.split(), d.split(), v.split(), f.split()))
    if o.dim() == 2:
        return [(o, d, v, f)]
    return [(o[b], d[b], v[b], f[b]) for b in range(o.shape[0])]


def case(name, kind, reps, reps_plain, say):
    o, d, v, f = make(name, kind)
    plan = ray_cast.RayCastPlan(f, v)
    nq = o.capacity if isinstance(o, RaggedPoints) else o.numel() // 3
    nf = f.capacity if isinstance(f, RaggedPoints) else f.numel() // 3
    B = plan.topology.shapes
    call = lambda kw: ray_cast.cast_rays(o, d, v, plan, return_bary=True, **kw)      # noqa: E731
    first = {key: call(kw) for key, kw in FORMS}                                      # (the untimed call of each)
    bits = lambda h: _packed(h.t).view(torch.int32)                                   # noqa: E731
    ref = first["count_plain"]
    rec = {"input": name, "bundle": kind, "rays": nq, "faces": nf, "open_edges": plan.open_edges,
           "culled_by_default": ray_cast._large(B, nq, nf),
           "same_bytes": all(bool(torch.equal(bits(h), bits(ref))) and bool(torch.equal(_packed(h.face), _packed(ref.face)))
                             for h in first.values())
           and all(bool(torch.equal(_packed(first[k].crossings), _packed(ref.crossings))) for k in ("default", "count_cull", "count_cull+reorder")),
           "hit_share": round(float(_packed(ref.hit).float().mean()), 4),
           "odd_crossings_share": round(float((_packed(ref.crossings) & 1).float().mean()), 4)}
    del first
    times = {key: [] for key, _ in FORMS}
    for r in range(reps):
        for key, kw in FORMS:
            if key.endswith("plain") and r >= reps_plain:
                continue
            times[key].append(_time(lambda: call(kw))[0])
    for key, _ in FORMS:
        rec[key + "_ms"] = [round(statistics.median(times[key]), 3), round(min(times[key]), 3), round(max(times[key]), 3)]
    rec["first_plain_over_cull"] = round(rec["first_plain_ms"][0] / min(rec["first_cull_ms"][0], rec["first_cull+reorder_ms"][0]), 2)
    rec["count_plain_over_cull"] = round(rec["count_plain_ms"][0] / min(rec["count_cull_ms"][0], rec["count_cull+reorder_ms"][0]), 2)
    rec["count_plain_over_default"] = round(rec["count_plain_ms"][0] / rec["default_ms"][0], 2)
    # for scale: closest_on_mesh with the origins as queries, and the torch composition on the first rays of every mesh
    faces_arg = f if isinstance(f, RaggedPoints) or f.dim() == 3 else f[None]
    q_arg, v_arg = (o, v) if isinstance(o, RaggedPoints) or o.dim() == 3 else (o[None], v[None])
    surface_distance.closest_on_mesh(q_arg, v_arg, faces_arg)
    ts = [_time(lambda: surface_distance.closest_on_mesh(q_arg, v_arg, faces_arg))[0] for _ in range(reps)]
    rec["closest_ms"] = [round(statistics.median(ts), 3), round(min(ts), 3), round(max(ts), 3)]
    parts = [(oo[:MT_RAYS], dd[:MT_RAYS], vv[ff.long()]) for oo, dd, vv, ff in per_mesh(o, d, v, f)]
    run = lambda: [torch_mt(*p) for p in parts]                                       # noqa: E731
    run()
    ts = [_time(run)[0] for _ in range(min(reps, 3))]
    done = sum(p[0].shape[0] for p in parts)
    rec["mt_rays"] = done
    rec["torch_mt_ms"] = [round(statistics.median(ts), 3), round(min(ts), 3), round(max(ts), 3)]
    rec["torch_mt_ms_scaled"] = round(statistics.median(ts) * nq / max(done, 1), 1)
    say(json.dumps(rec))


def evaluate_case(reps, say, points=20000):
    """``evaluate`` pairs/s with and without ``test.volume_iou``: a synthetic tree (synth.write_mesh_dataset_tree) of three sphere
    identities of 5002, 7202 and 3002 vertices, 9 pairs in batches of 4, no mesh export, the small forward model of the tests with
    procedural weights; wall time of a whole run (the loader, the step, the metrics, the read-back), the two forms alternated
    after one untimed run of each."""
    import tempfile
    import time
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from helpers import build_product, model_cfg                      # noqa: E402
    from nsdp_amd import evaluate, meshstore, synth                   # noqa: E402
    from nsdp_amd.model.deformation_networks import test_on_batch_with_cano as test_fn      # noqa: E402
    root = tempfile.mkdtemp(prefix="bench_raycast_")
    meshes = {"a": synth.sphere_mesh(50, 100), "b": synth.sphere_mesh(60, 120), "c": synth.sphere_mesh(50, 60)}
    split = "test_unseen_motions"
    cfg = model_cfg("forward", [256, 64, 16])
    cfg["data"] = dict(synth.write_mesh_dataset_tree(os.path.join(root, "tree"), meshes, ["walk", "jump", "turn"], 3, seed=9))
    cfg["test"] = {"iden_split": "identity_seen", "motion_split": split, "num_sampled_pairs": -1, "batch_size": 4,
                   "generate_mesh": False, "generate_pointcloud": False, "pointcloud_size": 30000}
    model = build_product(cfg, 72, DEV)[0].eval()
    store = meshstore.MeshStore(cfg, "identity_seen", split, device=DEV)
    forms = (("plain", {}), ("volume_iou", {"volume_iou": points}))

    def run(name, keys):
        config = dict(cfg, test=dict(cfg["test"], **keys))
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        rows = evaluate.evaluate(model, test_fn, store, config, os.path.join(root, name), 4, 6, log=lambda *_: None)
        torch.cuda.synchronize()
        return len(rows) / (time.perf_counter() - t0), rows

    pairs = {name: run(name, keys)[1] for name, keys in forms}
    rates = {name: [] for name, _ in forms}
    for _ in range(reps):
        for name, keys in forms:
            rates[name].append(run(name, keys)[0])
    rec = {"input": "evaluate", "pairs": len(pairs["plain"]), "vertices": [int(m[0].shape[0]) for m in meshes.values()],
           "volume_iou_points": points, "reps": reps}
    for name, _ in forms:
        rec[name + "_pairs_per_s"] = [round(statistics.median(rates[name]), 2), round(min(rates[name]), 2), round(max(rates[name]), 2)]
    rec["volume_iou_ms_per_pair"] = round(1000.0 / rec["volume_iou_pairs_per_s"][0] - 1000.0 / rec["plain_pairs_per_s"][0], 3)
    say(json.dumps(rec))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--reps-plain", type=int, default=3)
    ap.add_argument("--only", default="four_100k,four_large,eight_small,collapsed,thin_along,sweep_2048,sweep_8192,sweep_32768,sweep_131072")
    ap.add_argument("--out", default=None, help="also append the lines to this file")
    ap.add_argument("--evaluate", action="store_true", help="also time evaluate with and without test.volume_iou")
    args = ap.parse_args()

    def say(line):
        print(line, flush=True)
        if args.out:
            with open(args.out, "a") as fh:
                fh.write(line + "\n")

    for name in args.only.split(","):
        for kind in ("camera", "contains"):
            if name == "thin_along" and kind == "camera":
                continue
            case(name, kind, args.reps, min(args.reps_plain, args.reps), say)
    if args.evaluate:
        evaluate_case(args.reps, say)


if __name__ == "__main__":
    main()
