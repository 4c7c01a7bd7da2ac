"""Times the vertex normals of nsdp_amd/mesh_normals.py (include/nsdp_meshnormals.h) on one GPU, at user sizes:

    python tools/bench_normals.py [--rounds 20] [--no-sessions] [--out profiles/mesh_normals.txt]

  (a) ``vertex_normals`` alone -- two launches over corner lists built once -- against the torch composition that exists without
      it, ``cross`` of the edges + ``index_add_`` of the face normals into the vertices (floating-point atomics: not
      reproducible) + ``normalize``: one sphere of ~5000 and of ~100 000 vertices, four poses of the latter over its one face
      table, and the packed set of ~25 000 + 9000 + 40 000 + 12 000 vertices.  The one-off list build (``MeshTopology``, with and
      without its validating host read) is timed beside them;
  (b) a replayed drag (``EditSession(graph=True)``) with and without ``normals=True`` at ~5000, ~25 000 and ~100 000 vertices,
      and a track of T = 16 poses at ~5000;
  (c) the hub case ``sphere_mesh(2, 50 000)``: two poles of valence 50 000, each ONE workgroup's list (csrc/list_reduce.h's
      workgroup form: 196 gathers per thread and a tree) while every other workgroup is done after six corners per lane.

The forms of a comparison are ALTERNATED inside one loop after warm-up, each call timed with device events, synchronised;
median and range over the rounds.  Meshes are ``synth.sphere_mesh`` with about twice as many segments as rings.
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from bench_datastore import _ms, _stats      # noqa: E402  (tools/ is this script's directory)

PACKED = (25000, 9000, 40000, 12000)


def _alternate(forms, rounds, start, stop):
    import torch
    for _, fn in forms:
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    times = {n: [] for n, _ in forms}
    for _ in range(rounds):
        for n, fn in forms:
            times[n].append(_ms(fn, start, stop))
    return times


def _composition(verts, faces_global):
    """[P, R, 3] positions, [Q, 3] int64 GLOBAL rows -> unit normals by cross + index_add_ + normalize."""
    import torch
    a, b, c = verts[:, faces_global[:, 0]], verts[:, faces_global[:, 1]], verts[:, faces_global[:, 2]]
    n = torch.cross(b - a, c - a, dim=-1)
    s = torch.zeros_like(verts)
    for j in range(3):
        s.index_add_(1, faces_global[:, j], n)
    return torch.nn.functional.normalize(s, dim=-1)


def alone(rounds, say):
    import torch
    from nsdp_amd import mesh_normals as mn
    from nsdp_amd.edit import sphere_for
    from nsdp_amd.ragged import RaggedPoints
    dev = torch.device("cuda", 0)
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    cases = []
    for n, poses in ((5000, 1), (100000, 1), (100000, 4)):
        v, f = (torch.from_numpy(a).to(dev) for a in sphere_for(n))
        verts = torch.stack([v * (1.0 + 0.1 * p) for p in range(poses)]) if poses > 1 else v
        cases.append((f"{poses} x {v.shape[0]} vertices, {f.shape[0]} faces", f, verts, verts.reshape(poses, -1, 3), f.long()))
    meshes = [tuple(torch.from_numpy(a).to(dev) for a in sphere_for(n)) for n in PACKED]
    rv, rf = RaggedPoints.from_list([v for v, _ in meshes]), RaggedPoints.from_rows([f for _, f in meshes])
    base, glob = 0, []
    for v, f in meshes:
        glob.append(f.long() + base)
        base += v.shape[0]
    cases.append((f"packed {' + '.join(str(v.shape[0]) for v, _ in meshes)} vertices, {rf.capacity} faces", rf, rv,
                  rv.packed.reshape(1, -1, 3), torch.cat(glob)))
    hub = tuple(torch.from_numpy(a).to(dev) for a in _hub())
    cases.append((f"hub sphere_mesh(2, 50000): {hub[0].shape[0]} vertices, {hub[1].shape[0]} faces, two poles of valence 50 000", hub[1],
                  hub[0], hub[0].reshape(1, -1, 3), hub[1].long()))
    for name, faces, verts, flat, glob in cases:
        topo = mn.MeshTopology(faces, verts)
        ours = mn.vertex_normals(verts, topo)
        ours = (ours.packed if isinstance(ours, RaggedPoints) else ours).reshape(flat.shape)
        theirs = _composition(flat, glob)
        dev_max = float((ours - theirs).abs().max())
        again = mn.vertex_normals(verts, topo)
        again = (again.packed if isinstance(again, RaggedPoints) else again).reshape(flat.shape)
        forms = [("vertex_normals", lambda: mn.vertex_normals(verts, topo)), ("composition", lambda: _composition(flat, glob)),
                 ("list build", lambda: mn.MeshTopology(faces, verts, validate=False)),
                 ("list build + check", lambda: mn.MeshTopology(faces, verts))]
        times = _alternate(forms, rounds, start, stop)
        med = {k: statistics.median(v) for k, v in times.items()}
        say(f"{name} (largest difference to the composition {dev_max:.2e}; two runs the same bits: "
            f"{bool(torch.equal(ours.view(torch.int32), again.view(torch.int32)))}):")
        for n, _ in forms:
            say(f"  {n:19s} {_stats(times[n])}")
        say(f"  vertex_normals / composition = {med['vertex_normals'] / med['composition']:.3f}   "
            f"list build / vertex_normals = {med['list build'] / med['vertex_normals']:.1f}")


def _hub():
    import numpy as np
    from nsdp_amd import synth
    v, f = synth.sphere_mesh(2, 50000)
    return v.astype(np.float32), f


def sessions(rounds, say):
    import torch
    from nsdp_amd import synth
    from nsdp_amd.config import default_config
    from nsdp_amd.edit import EditSession, Motion, sphere_for
    from nsdp_amd.infer import _pyramid
    from nsdp_amd.model import build_model
    dev = torch.device("cuda", 0)
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    say("replayed drags (EditSession(graph=True), the cloud is the vertex set, default arbitrary model on procedural weights):")
    for n, track in ((5000, None), (25000, None), (100000, None), (5000, 16)):
        v, f = (torch.from_numpy(a).to(dev) for a in sphere_for(n))
        config = default_config("arbitrary")
        _pyramid(config, v.shape[0])
        model = build_model(config, device="cpu")[0]
        state = synth.procedural_state_dict(model.state_dict(), 2048)
        model.load_state_dict({k: torch.from_numpy(w) for k, w in state.items()})
        model.to(dev).eval()
        with torch.no_grad():
            session = EditSession(model, v[None].contiguous(), graph=True, faces=f)
            if track is None:
                call = lambda normals: session.drag("head", (-0.15, -0.2, -0.2), clone=False, normals=normals)
                what = f"drag, {v.shape[0]} vertices"
            else:
                session.set_handles(*session.labels_from_parts(["head"]))
                poses = [[Motion.translate((-0.15 * (t + 1) / track, -0.2 * (t + 1) / track, 0.0)), Motion.identity()] for t in range(track)]
                call = lambda normals: session.track(motions=poses, clone=False, normals=normals)
                what = f"track of T = {track}, {v.shape[0]} vertices"
            forms = [("without normals", lambda: call(False)), ("normals=True", lambda: call(True))]
            times = _alternate(forms, rounds, start, stop)
            session.close()
        med = {k: statistics.median(t) for k, t in times.items()}
        say(f"  {what}:")
        for k, _ in forms:
            say(f"    {k:16s} {_stats(times[k])}")
        say(f"    normals add {med['normals=True'] - med['without normals']:.3f} ms = "
            f"{100.0 * (med['normals=True'] / med['without normals'] - 1.0):.1f} % of the call")
        del model, session
        torch.cuda.empty_cache()


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--no-sessions", action="store_true", help="skip (b), the editing sessions")
    ap.add_argument("--out", default=None, help="also append the lines to this file")
    args = ap.parse_args(argv)
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    alone(args.rounds, say)
    if not args.no_sessions:
        sessions(args.rounds, say)
    if args.out:
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
