"""Times the self-intersection test of nsdp_amd/self_intersect.py (include/nsdp_selfintersect.h) on one GPU:

    python tools/bench_selfintersect.py [--rounds 10] [--no-sessions] [--no-collapsed] [--out profiles/self_intersect.txt]

  (a) the RATE of narrow tests on an all-candidate input -- a soup of triangles whose corners are uniform in one cube, so that
      nearly every pair passes adjacency and the box test -- with budget = 0 (one fused pass): ordered narrow tests per second
      = sum(cand) / time.  The default budget of the Python layer follows from it: the largest power of two b for which
      2^20 faces x b candidates stay under a second;
  (b) the culled form against the unculled form (flag bit 0: every block is visited) -- the only baseline there is, short of an
      F^2 tensor in torch -- under the default budget, on two spheres through each other (a plan: faces in Morton order) of ~5000
      and ~100 000 vertices in all, four poses of the latter, and the packed set of four such meshes;
  (c) the collapsed worst case under the default budget: every vertex in one tiny cube, random faces, so that every face is in
      every other's box and is skipped -- pass 1 is F^2 box and adjacency tests whatever the budget;
  (d) a replayed drag (``EditSession(graph=True)``) with and without ``self_intersections=True`` at ~5000, ~25 000 and ~100 000
      vertices.

The forms of a comparison are ALTERNATED inside one loop after warm-up, each call timed with device events, synchronised;
median and range over the rounds.
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from bench_datastore import _stats      # noqa: E402  (tools/ is this script's directory)
from bench_normals import _alternate    # noqa: E402

PACKED = (25000, 9000, 40000, 12000)
FACE_LIMIT = 1 << 20


def _pair(n, dev):
    """Two spheres through each other, ~n vertices in all -> (verts [V, 3], faces [F, 3]) on the device."""
    import numpy as np
    import torch
    from nsdp_amd.edit import sphere_for
    v, f = sphere_for(max(n // 2, 8))
    verts = np.concatenate([v, v * np.float32(0.8) + np.float32([0.21, 0.05, 0.03])]).astype(np.float32)
    faces = np.concatenate([f, f + len(v)]).astype(np.int32)
    return torch.from_numpy(verts).to(dev), torch.from_numpy(faces).to(dev)


def rate(rounds, say, faces=16384):
    import torch
    from nsdp_amd import self_intersect as si
    dev = torch.device("cuda", 0)
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    g = torch.Generator(device="cpu").manual_seed(1)
    verts = (torch.rand((3 * faces, 3), generator=g) * 2 - 1).to(dev)
    tf = torch.arange(3 * faces, dtype=torch.int32, device=dev).reshape(faces, 3)
    plan = si.SelfIntersectionPlan(tf, verts, reorder=False)
    res = si.self_intersections(verts, plan, budget=0)
    tests, pairs = int(res.cand.sum()), int(res.pairs)
    forms = [("budget 0 (one pass)", lambda: si.self_intersections(verts, plan, budget=0)),
             ("budget 2^30 (two passes)", lambda: si.self_intersections(verts, plan, budget=1 << 30)),
             ("budget 1 (pass 1 + an empty pass 2)", lambda: si.self_intersections(verts, plan, budget=1))]
    times = _alternate(forms, rounds, start, stop)
    med = {k: statistics.median(v) for k, v in times.items()}
    say(f"(a) all-candidate soup, {faces} faces: {tests} ordered narrow tests of {faces * (faces - 1)} ordered pairs, {pairs} intersecting pairs")
    for n, _ in forms:
        say(f"  {n:36s} {_stats(times[n])}")
    narrow = med["budget 2^30 (two passes)"] - med["budget 1 (pass 1 + an empty pass 2)"]
    per_s = tests / (max(narrow, 1e-6) * 1e-3)
    say(f"  pass 2 over pass 1 = {narrow:.3f} ms for {tests} narrow tests (and their box and adjacency tests again): "
        f"{per_s:.3e} narrow tests / s; the fused pass: {tests / (med['budget 0 (one pass)'] * 1e-3):.3e} / s")
    budget = 1
    while FACE_LIMIT * budget * 2 <= per_s:
        budget *= 2
    say(f"  -> the largest power of two b with 2^20 faces x b candidates under a second at that rate: {budget} "
        f"(DEFAULT_BUDGET is {si.DEFAULT_BUDGET})")


def culling(rounds, say):
    import torch
    from nsdp_amd import self_intersect as si
    from nsdp_amd.ragged import RaggedPoints
    dev = torch.device("cuda", 0)
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    cases = []
    for n, poses in ((5000, 1), (100000, 1), (100000, 4)):
        v, f = _pair(n, dev)
        verts = torch.stack([v * (1.0 + 0.1 * p) for p in range(poses)]) if poses > 1 else v
        cases.append((f"{poses} x {v.shape[0]} vertices, {f.shape[0]} faces", f, verts))
    meshes = [_pair(n, dev) for n in PACKED]
    rv, rf = RaggedPoints.from_list([v for v, _ in meshes]), RaggedPoints.from_rows([f for _, f in meshes])
    cases.append((f"packed {' + '.join(str(v.shape[0]) for v, _ in meshes)} vertices, {rf.capacity} faces", rf, rv))
    say("(b) culled against unculled, two spheres through each other, the default budget:")
    for name, faces, verts in cases:
        plan, given = si.SelfIntersectionPlan(faces, verts), si.SelfIntersectionPlan(faces, verts, reorder=False)
        a, b, c = (si.self_intersections(verts, p, cull=k) for p, k in ((plan, True), (plan, False), (given, True)))
        same = all(torch.equal(getattr(a, k), getattr(o, k)) for o in (b, c) for k in ("hits", "partner", "cand", "pairs", "skipped"))
        forms = [("culled, Morton order", lambda: si.self_intersections(verts, plan, cull=True)),
                 ("culled, the given order", lambda: si.self_intersections(verts, given, cull=True)),
                 ("unculled", lambda: si.self_intersections(verts, plan, cull=False)),
                 ("plan (once per topology)", lambda: si.SelfIntersectionPlan(faces, verts, validate=False))]
        times = _alternate(forms, max(rounds // 2, 3), start, stop)
        med = {k: statistics.median(v) for k, v in times.items()}
        say(f"  {name}: pairs {a.pairs.reshape(-1).tolist()}, faces hit {a.faces_hit.reshape(-1).tolist()}, largest cand "
            f"{int(a.cand.max())}; the three forms the same bytes: {same}")
        for n, _ in forms:
            say(f"    {n:26s} {_stats(times[n])}")
        say(f"    unculled / culled = {med['unculled'] / med['culled, Morton order']:.1f}   given order / Morton order = "
            f"{med['culled, the given order'] / med['culled, Morton order']:.2f}")


def collapsed(rounds, say, sizes=(65536, 262144)):
    import torch
    from nsdp_amd import self_intersect as si
    dev = torch.device("cuda", 0)
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    say(f"(c) collapsed meshes under the default budget {si.DEFAULT_BUDGET} (every face skipped; pass 1 is F^2 box + adjacency tests):")
    for faces in sizes:
        g = torch.Generator(device="cpu").manual_seed(2)
        verts = (torch.rand((faces // 2, 3), generator=g) * 1e-3).to(dev)
        tf = torch.randint(0, faces // 2, (faces, 3), generator=g, dtype=torch.int32).to(dev)
        plan = si.SelfIntersectionPlan(tf, verts)
        res = si.self_intersections(verts, plan)
        times = _alternate([("collapsed", lambda: si.self_intersections(verts, plan))], max(rounds // 3, 3), start, stop)
        med = statistics.median(times["collapsed"])
        say(f"  {faces} faces: skipped {int(res.skipped)}, smallest cand {int(res.cand.min())}: {_stats(times['collapsed'])}"
            f"   -> x {(FACE_LIMIT / faces) ** 2:.0f} at 2^20 faces = {med * (FACE_LIMIT / faces) ** 2 * 1e-3:.2f} s (extrapolated)")


def sessions(rounds, say):
    import torch
    from nsdp_amd import synth
    from nsdp_amd.config import default_config
    from nsdp_amd.edit import EditSession
    from nsdp_amd.infer import _pyramid
    from nsdp_amd.model import build_model
    dev = torch.device("cuda", 0)
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    say("(d) replayed drags (EditSession(graph=True), the cloud is the vertex set, default arbitrary model on procedural weights):")
    for n in (5000, 25000, 100000):
        v, f = _pair(n, dev)
        config = default_config("arbitrary")
        _pyramid(config, v.shape[0])
        model = build_model(config, device="cpu")[0]
        state = synth.procedural_state_dict(model.state_dict(), 2048)
        model.load_state_dict({k: torch.from_numpy(w) for k, w in state.items()})
        model.to(dev).eval()
        with torch.no_grad():
            session = EditSession(model, v[None].contiguous(), graph=True, faces=f)
            call = lambda flag: session.drag("head", (-0.15, -0.2, -0.2), clone=False, self_intersections=flag)
            out = call(True)
            found = (out["tgt_self_intersections"].tolist(), out["tgt_self_skipped"].tolist())
            forms = [("without", lambda: call(False)), ("without, again", lambda: call(False)), ("self_intersections=True", lambda: call(True))]
            times = _alternate(forms, rounds, start, stop)
            session.close()
        med = {k: statistics.median(t) for k, t in times.items()}
        say(f"  drag, {v.shape[0]} vertices, {f.shape[0]} faces (pairs {found[0]}, skipped {found[1]}):")
        for k, _ in forms:
            say(f"    {k:24s} {_stats(times[k])}")
        say(f"    the flag adds {med['self_intersections=True'] - med['without']:.3f} ms = "
            f"{100.0 * (med['self_intersections=True'] / med['without'] - 1.0):.1f} % of the call; the same form twice differs by "
            f"{abs(med['without, again'] - med['without']):.3f} ms")
        del model, session
        torch.cuda.empty_cache()


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--no-sessions", action="store_true", help="skip (d), the editing sessions")
    ap.add_argument("--no-collapsed", action="store_true", help="skip (c), the collapsed meshes")
    ap.add_argument("--out", default=None, help="also append the lines to this file")
    args = ap.parse_args(argv)
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    rate(args.rounds, say)
    culling(args.rounds, say)
    if not args.no_collapsed:
        collapsed(args.rounds, say)
    if not args.no_sessions:
        sessions(args.rounds, say)
    if args.out:
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
