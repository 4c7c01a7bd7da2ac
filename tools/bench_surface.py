"""The exact point-to-mesh distance (nsdp_amd/surface_distance.py) in all its forms, in one process on one GPU.

    python tools/bench_surface.py [--reps 5] [--reps-plain 3] [--only NAME[,NAME...]]

Inputs (synthetic meshes: a torus grid of W x H vertices with two faces per cell, rows in grid order, a few vertices no face
references where the vertex count is no product; the queries are points of the surface moved by 0.01 of its size):

    four_100k        4 x 100 000 queries against 4 x 200 000 faces
    four_large       the 278 160-vertex ragged set (100000, 61234, 35007, 81919 vertices), as many queries as vertices
    eight_small      eight meshes of 5000, 3100, 7200, 1800, 6400, 2500, 4100, 3900 vertices, as many queries as vertices
    shuffled_faces   100 000 queries against 200 000 faces in a random order (a block of 64 is not compact)
    mid_32k, mid_16k 32 768 queries against 65 536 faces, 16 384 against 32 768: either side of the default dispatch's threshold
    far_queries      100 000 queries 100 box sizes away from 200 000 faces (every face is about as far: nothing can be culled
                     before the nearest block has been seen)

For every input one JSON line: the median and min-max in ms of one ``closest_on_mesh`` call (with barycentric coordinates; the
Morton sort of the reordering forms is inside the timed call), HIP events around every call, the forms interleaved
(form 1, form 2, ..., form 1, ...) after one untimed call of each:

    default          what closest_on_mesh picks by itself
    cull             culling by blocks with the bound pass, rows as given
    cull+reorder     the same after the wrapper's Morton reordering of queries and faces
    nobound          culling without the bound pass, rows as given
    nobound+reorder  the same after reordering
    plain            the plain scan (flags bit 0): every query against every face (--reps-plain repetitions)

and ``same_bits``: dist2 of every form equals the plain scan's bit for bit.  For context only, the last line times the pair of
30 000 x 30 000 ``nn_dist2`` searches the sampled figure costs today.
"""
import argparse
import json
import math
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from nsdp_amd import pointnet2_utils, surface_distance            # noqa: E402
from nsdp_amd.ragged import RaggedPoints                          # noqa: E402

DEV = torch.device("cuda:0")
FOUR_LARGE = (100000, 61234, 35007, 81919)
EIGHT_SMALL = (5000, 3100, 7200, 1800, 6400, 2500, 4100, 3900)


def torus(V, seed):
    """-> (verts [V, 3], faces [2 W H, 3] int32) on the device: a torus grid of W x H <= V vertices, the rest unreferenced."""
    W = max(3, int(math.sqrt(V)))
    H = max(3, V // W)
    g = torch.Generator(device=DEV).manual_seed(seed)
    i, j = torch.meshgrid(torch.arange(H, device=DEV), torch.arange(W, device=DEV), indexing="ij")
    u, w = i.reshape(-1).float() * (2 * math.pi / H), j.reshape(-1).float() * (2 * math.pi / W)
    ring = 1.0 + 0.35 * torch.cos(w)
    grid = torch.stack((ring * torch.cos(u), ring * torch.sin(u), 0.35 * torch.sin(w)), dim=1)
    extra = torch.rand(V - W * H, 3, device=DEV, generator=g) * 2 - 1
    verts = torch.cat((grid, extra)) + torch.rand(3, device=DEV, generator=g)
    a = (i * W + j).reshape(-1)
    b = (i * W + (j + 1) % W).reshape(-1)
    c = (((i + 1) % H) * W + j).reshape(-1)
    d = (((i + 1) % H) * W + (j + 1) % W).reshape(-1)
    faces = torch.stack((torch.stack((a, b, c), 1), torch.stack((b, d, c), 1)), dim=1).reshape(-1, 3).int()
    return verts.contiguous(), faces.contiguous()


def queries(verts, faces, n, seed, far=False):
    g = torch.Generator(device=DEV).manual_seed(seed)
    f = faces[torch.randint(0, faces.shape[0], (n,), device=DEV, generator=g)].long()
    w = torch.rand(n, 3, device=DEV, generator=g) + 1e-3
    w = w / w.sum(1, keepdim=True)
    p = (w[:, 0:1] * verts[f[:, 0]] + w[:, 1:2] * verts[f[:, 1]]) + w[:, 2:3] * verts[f[:, 2]]
    p = p + 0.01 * torch.randn(n, 3, device=DEV, generator=g)
    if far:
        d = torch.randn(n, 3, device=DEV, generator=g)
        p = p + 270.0 * d / d.norm(dim=1, keepdim=True)
    return p.contiguous()


def make(name):
    if name == "four_100k":
        meshes = [torus(100000, 10 + b) for b in range(4)]
        return (torch.stack([queries(v, f, 100000, 20 + b) for b, (v, f) in enumerate(meshes)]), torch.stack([v for v, _ in meshes]),
                torch.stack([f for _, f in meshes]))
    if name in ("four_large", "eight_small"):
        counts = FOUR_LARGE if name == "four_large" else EIGHT_SMALL
        meshes = [torus(V, 30 + b) for b, V in enumerate(counts)]
        return (RaggedPoints.from_list([queries(v, f, V, 40 + b) for b, ((v, f), V) in enumerate(zip(meshes, counts))]),
                RaggedPoints.from_list([v for v, _ in meshes]), RaggedPoints.from_rows([f for _, f in meshes]))
    if name in ("mid_32k", "mid_16k"):
        n = 32768 if name == "mid_32k" else 16384
        v, f = torus(n, 54)
        return queries(v, f, n, 55)[None], v[None], f[None]
    v, f = torus(100000, 50)
    if name == "shuffled_faces":
        f = f[torch.randperm(f.shape[0], device=DEV, generator=torch.Generator(device=DEV).manual_seed(51))].contiguous()
        return queries(v, f, 100000, 52)[None], v[None], f[None]
    if name == "far_queries":
        return queries(v, f, 100000, 53, far=True)[None], v[None], f[None]
    raise SystemExit(f"unknown input {name}")


FORMS = (("default", {}), ("cull", {"cull": True, "reorder": False}), ("cull+reorder", {"cull": True, "reorder": True}),
         ("nobound", {"cull": True, "reorder": False, "bound": False}), ("nobound+reorder", {"cull": True, "reorder": True, "bound": False}),
         ("plain", {"cull": False, "reorder": False}))


def _time(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), out


def _dist2(out):
    return out[0].packed if isinstance(out[0], RaggedPoints) else out[0]


def case(name, reps, reps_plain):
    q, v, f = make(name)
    nq = q.capacity if isinstance(q, RaggedPoints) else q.shape[0] * q.shape[1]
    nf = f.capacity if isinstance(f, RaggedPoints) else f.shape[0] * f.shape[1]
    first = {key: _dist2(surface_distance.closest_on_mesh(q, v, f, **kw)) for key, kw in FORMS}      # (the untimed call of each)
    B = q.batch if isinstance(q, RaggedPoints) else q.shape[0]
    rec = {"input": name, "queries": nq, "faces": nf, "culled_by_default": surface_distance._large(B, nq, nf),
           "same_bits": all(bool(torch.equal(first[key].view(torch.int32), first["plain"].view(torch.int32))) for key, _ in FORMS)}
    del first
    times = {key: [] for key, _ in FORMS}
    for r in range(reps):
        for key, kw in FORMS:
            if key == "plain" and r >= reps_plain:
                continue
            times[key].append(_time(lambda: surface_distance.closest_on_mesh(q, v, f, **kw))[0])
    for key, _ in FORMS:
        rec[key + "_ms"] = [round(statistics.median(times[key]), 3), round(min(times[key]), 3), round(max(times[key]), 3)]
    timed = {key: rec[key + "_ms"][0] for key, _ in FORMS}
    rec["fastest"] = min((k for k in timed if k != "default"), key=timed.get)
    rec["plain_over_default"] = round(timed["plain"] / timed["default"], 2)
    print(json.dumps(rec), flush=True)


def context(reps):
    g = torch.Generator(device=DEV).manual_seed(60)
    a, b = torch.rand(1, 30000, 3, device=DEV, generator=g), torch.rand(1, 30000, 3, device=DEV, generator=g)
    pair = lambda: (pointnet2_utils.nn_dist2(a, b), pointnet2_utils.nn_dist2(b, a))      # noqa: E731
    pair()
    ts = [_time(pair)[0] for _ in range(reps)]
    print(json.dumps({"input": "context: nn_dist2 pair, 30000 x 30000", "pair_ms": [round(statistics.median(ts), 3), round(min(ts), 3),
                                                                                  round(max(ts), 3)]}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--reps-plain", type=int, default=3)
    ap.add_argument("--only", default="four_100k,four_large,eight_small,mid_32k,mid_16k,shuffled_faces,far_queries")
    args = ap.parse_args()
    for name in args.only.split(","):
        case(name, args.reps, min(args.reps_plain, args.reps))
    context(args.reps)


if __name__ == "__main__":
    main()
