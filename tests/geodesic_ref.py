"""numpy emulation of include/nsdp_geodesic.h, as the header writes the rule: the edge table over the corner lists of
tests/mesh_normals_ref.py operation by operation, the sanitising map S on the bits, a heap Dijkstra with ``np.float32`` sums and
limit pruning (distances and the hop counts of its shortest-path tree) -- what the kernels are held to, bit for bit --, a checker
of the fixed-point equation at every vertex, a block-local schedule in numpy (the kernel's shape: blocks of consecutive rows
relaxed to convergence against a snapshot of the others), and an fp64 Dijkstra over fp64 lengths of the same coordinates."""
import heapq

import numpy as np

import mesh_normals_ref as mr

f32 = np.float32
INF = f32(np.inf)


def _bits(x):
    return np.ascontiguousarray(x, dtype=f32).view(np.uint32)


def sanitise(x, limit=np.inf):
    """S: a value whose bits exceed the bits of ``limit`` (negatives, -0, NaN, everything farther) becomes +inf."""
    x = np.ascontiguousarray(x, dtype=f32)
    return np.where(_bits(x) <= _bits(f32(limit)), x, INF).astype(f32)


def edge_table(verts, faces, face_offsets, vert_offsets, dtype=f32):
    """verts (vcap, 3) or (P, vcap, 3) fp32 -> (list_offsets (vcap + 1), list_entries (3 fcap), nbr (6 fcap) int32, length
    (P, 6 fcap) in ``dtype``): position e of the lists, corner c = 3 q + j -> the rows of the face's next two corners and the
    lengths of the edges to them, sqrt((dx dx + dy dy) + dz dz) of d = P_a - P_n, one rounding per operation."""
    verts = np.asarray(verts, dtype=f32)
    poses = verts.reshape((-1,) + verts.shape[-2:])
    vcap = poses.shape[1]
    faces = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    rows, _ = mr.corner_rows(faces, face_offsets, vert_offsets, vcap)
    offsets, entries = mr.corner_lists(faces, face_offsets, vert_offsets, vcap)
    total = int(offsets[vcap])
    c = entries[:total].astype(np.int64)
    q, j = c // 3, c % 3
    a, n1, n2 = rows[q, j], rows[q, (j + 1) % 3], rows[q, (j + 2) % 3]
    nbr = np.zeros(6 * faces.shape[0], dtype=np.int32)
    nbr[0:2 * total:2], nbr[1:2 * total:2] = n1, n2
    length = np.zeros((poses.shape[0], 6 * faces.shape[0]), dtype=dtype)
    for p, pos in enumerate(poses.astype(dtype)):
        for k, n in ((0, n1), (1, n2)):
            d = pos[a] - pos[n]
            with np.errstate(all="ignore"):
                length[p, k:2 * total:2] = np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
    assert length.dtype == dtype
    return offsets, entries, nbr, length


def live_rows(vert_offsets, vcap):
    return int(mr._offsets(vert_offsets, vcap)[-1])


def dijkstra(list_offsets, nbr, length, start, limit=np.inf, live=None, dtype=f32):
    """The fixed point by a heap: ``start`` (vcap,) the seeds, sanitised; a candidate fl(D[u] + w) beyond the limit is pruned.
    Returns (D (vcap,) ``dtype``, hops (vcap,) int64: the edges on the path the heap found, -1 where nothing arrives)."""
    vcap = len(list_offsets) - 1
    live = vcap if live is None else live
    lim = dtype(limit)
    D = sanitise(start, limit).astype(dtype) if dtype == f32 else np.where(np.asarray(start) >= 0, start, np.inf).astype(dtype)
    if dtype != f32:
        D[~(D <= lim)] = np.inf
    D[live:] = np.inf
    hops = np.where(np.isfinite(D), 0, -1).astype(np.int64)
    heap = [(float(D[r]), int(r)) for r in np.flatnonzero(np.isfinite(D))]
    heapq.heapify(heap)
    lo = np.asarray(list_offsets, dtype=np.int64)
    while heap:
        d, r = heapq.heappop(heap)
        if d > D[r]:
            continue
        d = dtype(d)
        for i in range(2 * lo[r], 2 * lo[r + 1]):
            u = nbr[i]
            with np.errstate(all="ignore"):
                cand = d + length[i]
            if not (cand <= lim) or np.signbit(cand):      # S: beyond the limit, NaN, negative
                continue
            if cand < D[u]:
                D[u], hops[u] = cand, hops[r] + 1
                heapq.heappush(heap, (float(cand), int(u)))
    assert D.dtype == dtype
    return D, hops


def _owners(list_offsets):
    lo = np.asarray(list_offsets, dtype=np.int64)
    return np.repeat(np.repeat(np.arange(len(lo) - 1), np.diff(lo)), 2)      # the row of every table entry below 2 lo[vcap]


def relaxed(list_offsets, nbr, length, start, D, limit=np.inf, live=None, rows=None, source=None):
    """min(S(start), min over the lists of S(fl(source[u] + w))) for every row (``rows``: a boolean mask of the rows to relax,
    the others keep D), ``source`` defaulting to D: one relaxation of everything at once."""
    vcap = len(list_offsets) - 1
    live = vcap if live is None else live
    own = _owners(list_offsets)
    src = D if source is None else source
    with np.errstate(all="ignore"):
        cand = sanitise(src[nbr[:own.size]] + length[:own.size], limit)
    out = sanitise(start, limit)
    out[live:] = INF
    out = np.minimum(out, D)
    keep = np.ones(own.size, bool) if rows is None else rows[own]
    np.minimum.at(out, own[keep], cand[keep])
    return out


def fixed_point_violations(list_offsets, nbr, length, start, D, limit=np.inf, live=None):
    """The rows at which D is not min(S(start), min S(fl(D[u] + w))) -- empty for the fixed point (compared as bits)."""
    vcap = len(list_offsets) - 1
    live = vcap if live is None else live
    own = _owners(list_offsets)
    with np.errstate(all="ignore"):
        cand = sanitise(np.asarray(D, f32)[nbr[:own.size]] + length[:own.size], limit)
    want = sanitise(start, limit)
    want[live:] = INF
    np.minimum.at(want, own, cand)
    return np.flatnonzero(_bits(want) != _bits(D))


def block_local(list_offsets, nbr, length, start, block, limit=np.inf, live=None, max_rounds=100000):
    """The kernel's schedule: per round every block of ``block`` consecutive rows takes the other blocks' values as the round
    found them and relaxes its own rows until nothing falls.  Returns (D, rounds) -- the last round is the quiet one."""
    vcap = len(list_offsets) - 1
    live = vcap if live is None else live
    own = _owners(list_offsets)
    u = nbr[:own.size].astype(np.int64)
    w = length[:own.size]
    inside = (u // block) == (own // block)
    D = sanitise(start, limit)
    D[live:] = INF
    for rounds in range(1, max_rounds + 1):
        snap = D.copy()
        with np.errstate(all="ignore"):
            ext = sanitise(snap[u[~inside]] + w[~inside], limit)
        np.minimum.at(D, own[~inside], ext)
        while True:
            with np.errstate(all="ignore"):
                cand = sanitise(D[u[inside]] + w[inside], limit)
            before = D.copy()
            np.minimum.at(D, own[inside], cand)
            if np.array_equal(_bits(before), _bits(D)):
                break
        if np.array_equal(_bits(snap), _bits(D)):
            return D, rounds
    raise AssertionError("no fixed point")


def geodesic(verts, faces, seeds=None, start=None, limit=np.inf, return_hops=False):
    """One mesh, one pose: verts (V, 3), faces (F, 3), ``seeds`` vertex indices at distance 0 and / or ``start`` (V,)."""
    verts = np.asarray(verts, dtype=f32)
    V, F = len(verts), len(faces)
    s = np.full(V, np.inf, f32) if start is None else np.array(start, dtype=f32)
    if seeds is not None:
        seeds = np.asarray(seeds).reshape(-1)
        s[seeds[(seeds >= 0) & (seeds < V)]] = 0
    if F == 0:
        D = sanitise(s, limit)
        return (D, np.where(np.isfinite(D), 0, -1)) if return_hops else D
    lo, _, nbr, length = edge_table(verts, faces, [0, F], [0, V])
    D, hops = dijkstra(lo, nbr, length[0], s, limit)
    return (D, hops) if return_hops else D


# ---------------------------------------------------------------------------------------------------------------- meshes
def strip(n, seed=0):
    """A triangle strip of n >= 3 vertices (n - 2 faces): vertex i at (i / 2, i % 2) with a jitter, faces (i, i + 1, i + 2)
    turned alternately -- a path graph two vertices wide, about n / 2 hops long."""
    rng = np.random.default_rng(seed)
    i = np.arange(n)
    v = np.stack([i * 0.5, (i % 2) * 1.0, np.zeros(n)], axis=1) + rng.uniform(-0.05, 0.05, (n, 3))
    f = np.stack([i[:-2], i[1:-1], i[2:]], axis=1)
    f[1::2] = f[1::2][:, [1, 0, 2]]
    return v.astype(f32), f.astype(np.int32)


def grid(nx, ny):
    """The integer grid [0, nx) x [0, ny): unit squares, one diagonal each; vertex (x, y) is row y * nx + x."""
    x, y = np.meshgrid(np.arange(nx), np.arange(ny))
    v = np.stack([x.reshape(-1), y.reshape(-1), np.zeros(nx * ny)], axis=1).astype(f32)
    a = (y[:-1, :-1] * nx + x[:-1, :-1]).reshape(-1)
    f = np.concatenate([np.stack([a, a + 1, a + nx + 1], axis=1), np.stack([a, a + nx + 1, a + nx], axis=1)])
    return v, f.astype(np.int32)


def sphere_with(V, seed=0):
    """A closed sphere-like mesh of EXACTLY V >= 8 vertices: a latitude-longitude sphere of the largest ring count that fits,
    and the remaining vertices as a fan strip hung on its last vertex (so the graph stays connected)."""
    segs = max(3, int(np.sqrt(V / 2)))
    rings = max(1, (V - 2) // segs)
    v, f = mr.sphere(rings, segs)
    v, f = v.astype(f32), np.asarray(f, np.int64)
    extra = V - len(v)
    assert extra >= 0
    if extra:
        rng = np.random.default_rng(seed)
        base = len(v)
        new = v[-1] + np.cumsum(rng.uniform(0.01, 0.03, (extra, 3)), axis=0)
        chain = np.concatenate([[base - 2, base - 1], base + np.arange(extra)])
        f = np.concatenate([f, np.stack([chain[:-2], chain[1:-1], chain[2:]], axis=1)])
        v = np.concatenate([v, new.astype(f32)])
    assert len(v) == V
    return v, f.astype(np.int32)
