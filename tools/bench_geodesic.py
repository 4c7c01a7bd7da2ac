"""Geodesic distances on the device (nsdp_amd/geodesic.py, include/nsdp_geodesic.h), timed on the normals row's meshes: a full
field from one seed and a brush of one eighth of the sphere's radius; the plan's Morton order against a shuffled numbering with
``reorder=False``; rounds, ms per round and the edge-length call alone; ``rounds_per_call`` alternatives.  Baselines, none of them
the code under test: the NO_LOCAL form (one relaxation per round), one relaxation per iteration composed from torch ops
(``scatter_reduce_`` with ``amin`` over the edge list, one host read per ``rounds_per_call`` iterations), and the host heap
Dijkstra of tests/geodesic_ref.py including the copies.  The forms are interleaved round by round on the same device; medians
with their ranges.

    python tools/bench_geodesic.py [--reps 7] [--host-dijkstra] [--lib PATH] > profiles/geodesic.txt

``--lib``: another build of libnsdp_hip.so (``-DNSDP_GEODESIC_BLOCK=256`` on geodesic.hip) to compare block sizes."""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np      # noqa: E402

RADIUS = 0.4
MESHES = {4952: (50, 99), 99683: (223, 447), 24978: (112, 223), 8980: (67, 134), 39764: (141, 282), 11860: (77, 154)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--host-dijkstra", action="store_true", help="time the host heap Dijkstra too (seconds per large mesh)")
    ap.add_argument("--lib", default=None)
    args = ap.parse_args()
    from nsdp_amd import _lib
    if args.lib:
        _lib.SO_PATH = os.path.abspath(args.lib)
    import torch
    from nsdp_amd import geodesic as g, synth
    from nsdp_amd.ragged import RaggedPoints
    dev = torch.device("cuda", 0)
    block = _lib.lib().nsdp_mesh_geodesic_block()
    print(f"block = {block} vertex rows per workgroup, default rounds_per_call = {g.DEFAULT_ROUNDS}, reps = {args.reps}")

    def sphere(V):
        v, f = synth.sphere_mesh(*MESHES[V], radius=RADIUS)
        assert len(v) == V
        return v.astype(np.float32), f

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, out

    def report(name, ts, extra=""):
        print(f"  {name:<34s} median {statistics.median(ts):9.3f} ms   range {min(ts):9.3f} .. {max(ts):9.3f}   {extra}")

    def torch_relax(nbr, length, owner, start, limit, per_call, bound):
        """One relaxation per iteration from torch ops: candidates over the edge list, scatter_reduce_ amin into the rows."""
        P, vcap = start.shape
        d = start.clone()
        base = (torch.arange(P, device=dev) * vcap).view(P, 1)
        src, dst = (base + nbr.long()[None]).reshape(-1), (base + owner[None]).reshape(-1)
        rounds = 0
        while rounds < bound:
            for _ in range(per_call):
                before = d
                cand = d.reshape(-1)[src] + length.reshape(-1)
                cand = torch.where(cand <= limit, cand, torch.full_like(cand, float("inf")))
                d = d.reshape(-1).scatter_reduce(0, dst, cand, "amin", include_self=True).view(P, vcap)
                rounds += 1
            if bool((d == before).all()):
                break
        return d, rounds

    def bench(title, verts, faces, seeds, P=1):
        """verts / faces as geodesic_distances takes them; seeds in its layout."""
        print(title)
        plan = g.GeodesicPlan(faces, verts)
        topo = plan.topology
        nbr, length = g.edge_lengths(verts, plan)
        total = 2 * int(plan.list_offsets[-1])
        owner = torch.repeat_interleave(torch.arange(topo.vcap, device=dev), 2 * (plan.list_offsets[1:] - plan.list_offsets[:-1]).long(),
                                        output_size=total)
        # a shuffled numbering of the same meshes (inside every mesh's own rows), kept by reorder=False
        packed = verts.packed if isinstance(verts, RaggedPoints) else verts.reshape(-1, topo.vcap, 3)[0]
        gen = torch.Generator(device="cpu").manual_seed(1)
        key = torch.rand(topo.vcap, generator=gen).to(dev) + g.shape_ids(topo.vert_offsets, topo.vcap).double()
        perm = torch.argsort(key)
        rank = torch.empty_like(perm)
        rank[perm] = torch.arange(topo.vcap, device=dev)
        shuffled = None
        if not isinstance(verts, RaggedPoints) and P == 1 and topo.kind == "shared":
            sv, sf = packed[perm].contiguous(), rank[faces.long()].to(torch.int32)
            shuffled = (sv, g.GeodesicPlan(sf, sv, reorder=False), rank[seeds.long()])
        for what, limit in (("full field", float("inf")), (f"brush r = {RADIUS / 8:g}", RADIUS / 8)):
            forms = {
                "block-local (the default)": lambda: g.geodesic_distances(verts, plan, seeds, limit=limit, return_stats=True),
                "NO_LOCAL (one relaxation / round)": lambda: g.geodesic_distances(verts, plan, seeds, limit=limit, return_stats=True,
                                                                                  no_local=True, rounds_per_call=64),
                "edge-length call alone": lambda: (g.edge_lengths(verts, plan), {"rounds": 0, "calls": 0}),
            }
            if shuffled is not None:
                forms["shuffled numbering, reorder=False"] = lambda: g.geodesic_distances(shuffled[0], shuffled[1], shuffled[2], limit=limit,
                                                                                           return_stats=True)
            start = g._start(plan, P, (), seeds, None, None)
            start_k = plan.to_plan(start)
            forms["torch scatter_reduce_ relaxation"] = lambda: torch_relax(nbr[:total], length[:, :total], owner, start_k, limit, 64,
                                                                            plan.max_vertices + 1)
            times = {k: [] for k in forms}
            stats = {}
            for k, fn in forms.items():      # warm-up, and the answers against each other
                _, out = timed(fn)
                stats[k] = out[1]
            ref = g.geodesic_distances(verts, plan, seeds, limit=limit)
            ref = ref.packed if isinstance(ref, RaggedPoints) else ref
            tr = plan.to_caller(torch_relax(nbr[:total], length[:, :total], owner, start_k, limit, 64, plan.max_vertices + 1)[0])
            same = torch.equal(ref.reshape(-1).view(torch.int32), tr.reshape(-1).view(torch.int32))
            for _ in range(args.reps):
                for k, fn in forms.items():
                    times[k].append(timed(fn)[0])
            reached = int(torch.isfinite(ref).sum())
            print(f" {what}: {reached} of {ref.numel()} vertices reached; torch relaxation gives the same bits: {same}")
            for k in forms:
                s = stats[k]
                rounds = s["rounds"] if isinstance(s, dict) else s
                extra = ""
                if rounds:
                    extra = f"{rounds} rounds, {statistics.median(times[k]) / rounds:.4f} ms / round"
                    if isinstance(s, dict) and s["calls"]:
                        extra += f", {s['calls']} calls"
                report(k, times[k], extra)
        return plan

    with torch.no_grad():
        v5, f5 = sphere(4952)
        bench("1 x 4952 vertices", torch.from_numpy(v5).to(dev), torch.from_numpy(f5).to(dev), torch.tensor([0], device=dev))
        v1, f1 = sphere(99683)
        tv, tf = torch.from_numpy(v1).to(dev), torch.from_numpy(f1).to(dev)
        plan = bench("1 x 99683 vertices", tv, tf, torch.tensor([0], device=dev))
        print("rounds_per_call on 1 x 99683, full field:")
        per = {n: [] for n in (1, 2, 4, 8, 16, 32, 64)}
        for _ in range(args.reps + 1):
            for n in per:
                ms, (_, st) = timed(lambda: g.geodesic_distances(tv, plan, torch.tensor([0], device=dev), rounds_per_call=n, return_stats=True))
                per[n].append((ms, st))
        for n, rows in per.items():
            report(f"rounds_per_call = {n}", [r[0] for r in rows[1:]], f"{rows[-1][1]['rounds']} rounds in {rows[-1][1]['calls']} calls")
        four = tv[None].repeat(4, 1, 1) * torch.tensor([1.0, 0.9, 1.1, 0.8], device=dev).view(4, 1, 1)
        bench("4 x 99683 vertices (poses of one topology)", four, tf, torch.tensor([0], device=dev), P=4)
        parts = [sphere(n) for n in (24978, 8980, 39764, 11860)]
        rv = RaggedPoints.from_list([torch.from_numpy(v).to(dev) for v, _ in parts])
        rf = RaggedPoints.from_rows([torch.from_numpy(f).to(dev) for _, f in parts])
        bench("packed 24978 + 8980 + 39764 + 11860 vertices", rv, rf, torch.zeros((4, 1), dtype=torch.int64, device=dev))
        if args.host_dijkstra:
            import geodesic_ref as gr
            for name, (v, f) in (("1 x 4952", (v5, f5)), ("1 x 99683", (v1, f1))):
                t0 = time.perf_counter()
                d = gr.geodesic(torch.from_numpy(v).to(dev).cpu().numpy(), f, [0])
                torch.from_numpy(d).to(dev)
                torch.cuda.synchronize()
                print(f"host heap Dijkstra (tests/geodesic_ref.py, numpy table + Python heap + copies), {name}: "
                      f"{(time.perf_counter() - t0) * 1e3:.0f} ms (one run)")


if __name__ == "__main__":
    main()
