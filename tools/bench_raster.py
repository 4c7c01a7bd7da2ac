"""The rasteriser (nsdp_amd/rasterize.py, include/nsdp_raster.h) against the only device route to a depth image the parent has,
``cast_rays`` with one ray per pixel -- in one process on one GPU, the forms interleaved.

    python tools/bench_raster.py [--reps 5] [--only NAME[,NAME...]] [--sizes 256,512,1024] [--no-drags] [--out profiles/rasterize.txt]

Meshes: the latitude-longitude spheres of ``nsdp_amd.edit.sphere_for`` (closed; the plan's Morton order is applied as a user
would get it), slightly flattened so that no two of their axes agree.  Inputs:

    one_5k           1 x 4952 vertices (9900 faces)
    one_100k         1 x 99 683 vertices (199 362 faces)
    four_100k        4 poses of the 99 683-vertex topology (scaled copies), one image each
    packed           the packed set of 24 978, 8980, 39 764 and 11 860 vertices (85 582 in all), one image each
  and the cases expected to lose:
    shuffled         one_100k with its faces shuffled and the order kept (reorder=False): a block of 64 faces covers the screen
    inside           one_100k seen by a pinhole INSIDE the mesh: huge triangles, and the faces behind the eye are dropped
    collapsed        one_100k shrunk to about 8 pixels across in the middle of one tile: every face lands in that tile

For every input and image size S x S one JSON line: the median and min-max in ms of one call, HIP events around every call,
after one untimed call of each form:

    raster_ms        rasterize(..., return_bary=True, count=False)       depth, face, weights
    raster_count_ms  rasterize(..., return_bary=False, count=True)
    raycast_ms       cast_rays over the same pixels' rays (origins on the camera's plane, the viewing direction; first-hit mode,
                     count=False, its default dispatch) -- not timed for ``inside`` (a pinhole's rays are another bundle, and
                     the comparison of interest there is the rasteriser against itself)
    same_hits        the two agree on which pixels are covered, and their depths to 1e-4 of the mesh's size, on all but
                     ``edge_pixels`` pixels (a ray cast shears the fp32 corners per ray, the rasteriser snaps them to 1/256 pixel:
                     the silhouettes differ by design)

``--no-drags`` leaves out the last part: a replayed drag (EditSession(graph=True), the arbitrary model of the tosca configs) of a
sphere of 5000, 25 000 and 100 000 vertices with and without ``render=RenderSpec(one fitted view, 512 x 512)``.
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from nsdp_amd import ray_cast, rasterize as rz, synth              # noqa: E402
from nsdp_amd.edit import EditSession, HandleSpec, RenderSpec, sphere_for       # noqa: E402
from nsdp_amd.ragged import RaggedPoints                           # noqa: E402

DEV = torch.device("cuda:0")
PACKED = (24978, 8980, 39764, 11860)
DIRECTION = (0.3, -0.2, 1.0)
SPEC = HandleSpec("head", (-0.15, -0.2, -0.2), 0.1, False)


def sphere(n, seed=0):
    v, f = sphere_for(n)
    v = v * np.float32([1.0, 0.8, 0.65]) * np.float32(1.0 + 0.05 * seed)
    return torch.from_numpy(np.ascontiguousarray(v, np.float32)).to(DEV), torch.from_numpy(np.ascontiguousarray(f, np.int32)).to(DEV)


def ortho_views(meshes, S):
    """One fitted orthographic camera per mesh and the rays of its pixels: (cams [M, 1, 4, 4], origins [M, S*S, 3], dirs)."""
    cams, origins, dirs = [], [], []
    for v in meshes:
        cam = rz.Camera.fit(v, DIRECTION, S, S)
        m = cam.matrix.astype(np.float64)
        # rows X = s r.p + cx, Y = -s u.p + cy, Z = f.(p - eye): the pixel (px, py) is the line p = eye' + a r - b u + t f
        s = np.linalg.norm(m[0, :3])
        r, u, f = m[0, :3] / s, -m[1, :3] / s, m[2, :3]
        px = np.arange(S) + 0.5
        a, b = (px - m[0, 3]) / s, -(px - m[1, 3]) / s
        o = a[None, :, None] * r + b[:, None, None] * u - m[2, 3] * f       # Z = 0 on the camera's plane
        cams.append(cam.matrix)
        origins.append(torch.from_numpy(o.reshape(-1, 3).astype(np.float32)).to(DEV))
        dirs.append(torch.from_numpy(np.tile(f.astype(np.float32), (S * S, 1))).to(DEV))
    return torch.from_numpy(np.stack(cams)).to(DEV).unsqueeze(1), origins, dirs


def make(name):
    """-> (verts, faces, kwargs of the plan, list of per-mesh vertex tensors, kind of view)."""
    if name == "one_5k":
        v, f = sphere(5000)
        return v, f, {}, [v], "ortho"
    if name in ("one_100k", "shuffled", "inside", "collapsed"):
        v, f = sphere(100000)
        if name == "shuffled":
            f = f[torch.randperm(f.shape[0], device=DEV, generator=torch.Generator(device=DEV).manual_seed(3))].contiguous()
            return v, f, {"reorder": False}, [v], "ortho"
        return v, f, {}, [v], {"one_100k": "ortho", "inside": "inside", "collapsed": "collapsed"}[name]
    if name == "four_100k":
        v, f = sphere(100000)
        poses = torch.stack([v * (1.0 + 0.05 * b) for b in range(4)]).contiguous()
        return poses, f, {}, list(poses), "ortho"
    if name == "packed":
        meshes = [sphere(n, b) for b, n in enumerate(PACKED)]
        return (RaggedPoints.from_list([v for v, _ in meshes]), RaggedPoints.from_rows([f for _, f in meshes]), {},
                [v for v, _ in meshes], "ortho")
    raise SystemExit(f"bench_raster: no input {name!r}")


def _time(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), out


def stats(xs):
    return [round(statistics.median(xs), 3), round(min(xs), 3), round(max(xs), 3)]


def case(name, S, reps, say):
    verts, faces, plan_args, meshes, view = make(name)
    plan = rz.RasterPlan(faces, verts, **plan_args)
    M = len(meshes)
    line = {"input": name, "size": S, "meshes": M, "vertices": sum(int(v.shape[0]) for v in meshes), "faces": int(plan.topology.fcap)}
    forms = {}
    if view == "inside":
        centre = meshes[0].mean(dim=0).cpu().numpy()
        cams = torch.from_numpy(rz.Camera.look_at(centre, centre + np.array(DIRECTION), (0, 1, 0), 90, S, S).matrix).to(DEV).reshape(1, 4, 4)
    else:
        cams, origins, dirs = ortho_views(meshes, S)
        if view == "collapsed":                                   # the whole mesh about 8 pixels across, in the middle of ONE tile
            k = 16.0 / S
            scale = torch.tensor([k, k, 1.0, 1.0], device=DEV).view(1, 1, 4, 1)
            shift = torch.zeros(1, 1, 4, 4, device=DEV)
            shift[0, 0, 0, 3] = shift[0, 0, 1, 3] = S / 2 + 8 - k * S / 2
            cams = cams * scale + shift
        else:
            if isinstance(verts, RaggedPoints):
                o, d = RaggedPoints.from_list(origins), RaggedPoints.from_list(dirs)
            else:
                o, d = (torch.stack(origins), torch.stack(dirs)) if verts.dim() == 3 else (origins[0], dirs[0])
            forms["raycast_ms"] = lambda: ray_cast.cast_rays(o, d, verts, plan, return_bary=True, count=False)
        if not isinstance(verts, RaggedPoints) and verts.dim() == 2:
            cams = cams[0]
    forms["raster_ms"] = lambda: rz.rasterize(verts, plan, cams, S, S, return_bary=True, count=False)
    forms["raster_count_ms"] = lambda: rz.rasterize(verts, plan, cams, S, S, return_bary=False, count=True)
    first = {k: fn() for k, fn in forms.items()}                  # one untimed call of each
    r = first["raster_ms"]
    line["covered_share"] = round(float(r.hit.float().mean()), 4)
    line["dropped"] = int(r.dropped.sum())
    line["max_count"] = int(first["raster_count_ms"].count.max())
    if "raycast_ms" in forms:
        hits = first["raycast_ms"]
        t = (hits.t.packed[:, 0] if isinstance(hits.t, RaggedPoints) else hits.t).reshape(-1)
        hit = (hits.hit.packed[:, 0] if isinstance(hits.hit, RaggedPoints) else hits.hit).reshape(-1)
        depth, rhit = r.depth.reshape(-1), r.hit.reshape(-1)
        size = float(max((v.amax(dim=0) - v.amin(dim=0)).max() for v in meshes))
        agree = (hit == rhit) & (~hit | ((t - depth).abs() <= 1e-4 * size))
        line["edge_pixels"] = int((~agree).sum())
        line["same_hits"] = bool(line["edge_pixels"] <= 0.01 * int(rhit.sum()))
    times = {k: [] for k in forms}
    for _ in range(reps):
        for k, fn in forms.items():
            times[k].append(_time(fn)[0])
    line.update({k: stats(v) for k, v in times.items()})
    if "raycast_ms" in times:
        line["raycast_over_raster"] = round(statistics.median(times["raycast_ms"]) / statistics.median(times["raster_ms"]), 2)
    say(json.dumps(line))
    return line


def drags(reps, say, S=512):
    from nsdp_amd.config import default_config
    from nsdp_amd.model import build_model
    config = default_config("arbitrary")
    model = build_model(config, device="cpu")[0]
    state = synth.procedural_state_dict(model.state_dict(), 2048)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in state.items()})
    model.to(DEV).eval()

    def window(fn, n):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        for i in range(n):
            fn(i)
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) / n

    translation = lambda i: tuple(v * (1.0 + 0.01 * (i % 7)) for v in SPEC.translation)      # noqa: E731
    with torch.no_grad():
        for n in (5000, 25000, 100000):
            v, f = sphere_for(n)
            verts, faces = torch.from_numpy(v)[None].to(DEV), torch.from_numpy(f).to(DEV)
            session = EditSession(model, verts, graph=True, faces=faces)
            pred = session.drag(SPEC.part, translation(0))["verts_tgt_pred"]      # (the view is fitted to what the model predicts)
            views = {"shaded": RenderSpec(rz.Camera.fit(pred, DIRECTION, S, S), S, S),
                     "depth_only": RenderSpec(rz.Camera.fit(pred, DIRECTION, S, S), S, S, shade=False)}
            forms = {"drag_ms": lambda i: session.drag(SPEC.part, translation(i), clone=False)}
            for k, spec in views.items():
                forms[f"drag_render_{k}_ms"] = (lambda i, spec=spec: session.drag(SPEC.part, translation(i), clone=False, render=spec))
            plan = rz.RasterPlan(faces, verts, topology=session.topology)
            forms["rasterize_alone_ms"] = lambda i: rz.rasterize(pred, plan, views["depth_only"].tensor, S, S, return_bary=False)
            for fn in forms.values():
                for i in range(3):
                    fn(i)
            calls = 20 if n <= 25000 else 10
            times = {k: [] for k in forms}
            for _ in range(reps):
                for k, fn in forms.items():
                    times[k].append(window(fn, calls))
            shown = session.drag(SPEC.part, translation(0), render=views["depth_only"])
            line = {"input": "drag", "vertices": int(v.shape[0]), "faces": int(f.shape[0]), "size": S, "replays": session.replays,
                    "covered_share": round(float((shown["tgt_face_image"] >= 0).float().mean()), 4)}
            line.update({k: stats(x) for k, x in times.items()})
            drag = statistics.median(times["drag_ms"])
            line["preview_share_of_drag"] = round((statistics.median(times["drag_render_shaded_ms"]) - drag) / drag, 3)
            line["depth_only_share_of_drag"] = round((statistics.median(times["drag_render_depth_only_ms"]) - drag) / drag, 3)
            say(json.dumps(line))
            session.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--only", default=None)
    ap.add_argument("--sizes", default="256,512,1024")
    ap.add_argument("--no-drags", action="store_true", dest="no_drags")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    names = args.only.split(",") if args.only else ["one_5k", "one_100k", "four_100k", "packed", "shuffled", "inside", "collapsed"]
    sizes = [int(s) for s in args.sizes.split(",")]
    out = open(args.out, "w") if args.out else None

    def say(text):
        print(text, flush=True)
        if out:
            out.write(text + "\n")
            out.flush()

    say(f"# python tools/bench_raster.py --reps {args.reps}   (one MI355X, one process, the forms interleaved; [median, min, max] in ms; "
        "see the tool's module text for the inputs and the forms)")
    with torch.no_grad():
        for name in names:
            for S in sizes:
                case(name, S, args.reps, say)
    if not args.no_drags:
        drags(args.reps, say)
    if out:
        out.close()


if __name__ == "__main__":
    main()
