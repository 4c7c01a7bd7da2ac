"""The yardstick of the point-to-mesh distance tests: a brute-force fp64 point-to-triangle distance in numpy over all faces,
degenerate faces (segments, points) included, plus the test meshes and the envelope constant of include/nsdp_surface.h.

Every triangle is treated as the union of its three edge segments and -- where it has an area -- its interior: the distance is
the smallest over the three clamped segment projections and the plane projection where that falls inside.  In fp64 on fp32
inputs this is exact to ~1e-16 relative, eight decimal digits below anything the fp32 kernel is held to."""
import numpy as np

U = 2.0 ** -24
# |dist2 - exact| <= E * U * R2 to first order, R2 the largest squared distance from the query to the face's corners
# (DESIGN.md 4k): the distance itself is off by at most 6 (an edge candidate) or 7 (the interior) units of U * R --
#   1  the corners in the query's frame, A = a - p: each moves by at most U |A|
#   2  the edge vectors e = Q - P, |e| <= 2 R: the far end of the segment (the spanned plane) moves by at most U |e|
#   3  X = P + t e: the product (U t |e| <= 2 U R) and the sum (U |X| <= U R)               -- an edge candidate
#   4  X = (A + b1 ab) + b2 ac: two products (b1 + b2 <= 1: 2 U R in all) and two sums (U R each)   -- the interior
# (errors of t, b1, b2 move X along the segment / inside the plane, where the squared distance is stationary: second order),
# so |d2 - exact| <= 2 d (7 U R) + 3 U d2 (the final dot product) <= 17 U R2 with d <= R.
E = 17.0

# the triangle (0,0,0), (2,0,0), (0,2,0) in the plane z = 0
TRI_A, TRI_B, TRI_C = (0.0, 0.0, 0.0), (2.0, 0.0, 0.0), (0.0, 2.0, 0.0)
REGIONS = [
    # query                 dist2    bary                     where
    ((0.5, 0.5, 3.0),       9.0,     (0.5, 0.25, 0.25)),      # above the interior
    ((0.5, 0.5, -3.0),      9.0,     (0.5, 0.25, 0.25)),      # below it (the other orientation)
    ((0.5, 0.5, 0.0),       0.0,     (0.5, 0.25, 0.25)),      # in the plane, inside
    ((1.0, -2.0, 0.0),      4.0,     (0.5, 0.5, 0.0)),        # beyond edge AB
    ((-1.0, 1.0, 2.0),      5.0,     (0.5, 0.0, 0.5)),        # beyond edge AC, off the plane
    ((2.0, 2.0, 0.0),       2.0,     (0.0, 0.5, 0.5)),        # beyond edge BC
    ((-1.0, -1.0, 1.0),     3.0,     (1.0, 0.0, 0.0)),        # beyond corner A
    ((4.0, -1.0, 0.0),      5.0,     (0.0, 1.0, 0.0)),        # beyond corner B
    ((-1.0, 5.0, 0.0),      10.0,    (0.0, 0.0, 1.0)),        # beyond corner C
    ((1.0, 0.0, 0.0),       0.0,     (0.5, 0.5, 0.0)),        # on edge AB
    ((2.0, 0.0, 0.0),       0.0,     (0.0, 1.0, 0.0)),        # at corner B
]


def _seg(P, e):
    """Closest point of segments P + t e to the origin (fp64, broadcast over leading axes) -> (t, squared distance)."""
    ee = (e * e).sum(-1)
    tn = -(P * e).sum(-1)
    with np.errstate(divide="ignore", invalid="ignore"):
        t = np.where(ee > 0, np.clip(tn / np.where(ee > 0, ee, 1.0), 0.0, 1.0), 0.0)
    X = P + t[..., None] * e
    return t, (X * X).sum(-1)


def closest(p, a, b, c):
    """fp64 closest point of triangles (a, b, c) to points p, all broadcastable to [..., 3] -> (dist2 [...], bary [..., 3])."""
    p, a, b, c = (np.asarray(x, dtype=np.float64) for x in (p, a, b, c))
    A, B, C = a - p, b - p, c - p
    A, B, C = np.broadcast_arrays(A, B, C)
    ab, ac, bc = B - A, C - A, C - B
    shape = A.shape[:-1]
    best = np.full(shape, np.inf)
    bary = np.zeros(shape + (3,))
    for (P, e, i, j) in ((A, ab, 0, 1), (A, ac, 0, 2), (B, bc, 1, 2)):
        t, d = _seg(P, e)
        take = d < best
        best = np.where(take, d, best)
        cand = np.zeros(shape + (3,))
        cand[..., i], cand[..., j] = 1.0 - t, t
        bary = np.where(take[..., None], cand, bary)
    g11, g12, g22 = (ab * ab).sum(-1), (ab * ac).sum(-1), (ac * ac).sum(-1)
    r1, r2 = -(A * ab).sum(-1), -(A * ac).sum(-1)
    det = g11 * g22 - g12 * g12
    v, w = g22 * r1 - g12 * r2, g11 * r2 - g12 * r1
    inside = (det > 1e-24 * g11 * g22) & (v > 0) & (w > 0) & (v + w < det)
    safe = np.where(inside, det, 1.0)
    b1, b2 = v / safe, w / safe
    X = A + b1[..., None] * ab + b2[..., None] * ac
    d = (X * X).sum(-1)
    take = inside & (d < best)
    best = np.where(take, d, best)
    bary = np.where(take[..., None], np.stack((1.0 - b1 - b2, b1, b2), axis=-1), bary)
    return best, bary


def all_faces(query, verts, faces):
    """The fp64 squared distance of every query [n, 3] to every face [F, 3] of one mesh -> [n, F]."""
    v = np.asarray(verts, dtype=np.float64)
    f = np.asarray(faces, dtype=np.int64)
    q = np.asarray(query, dtype=np.float64)
    out = np.empty((q.shape[0], f.shape[0]))
    for lo in range(0, q.shape[0], 256):
        out[lo:lo + 256] = closest(q[lo:lo + 256, None, :], v[f[:, 0]][None], v[f[:, 1]][None], v[f[:, 2]][None])[0]
    return out


def brute(query, verts, faces):
    """-> (dist2 [n] the exact minimum, face [n] the first face at it, all [n, F])."""
    d = all_faces(query, verts, faces)
    if d.shape[1] == 0:
        return np.full(d.shape[0], np.finfo(np.float32).max, dtype=np.float64), np.full(d.shape[0], -1), d
    face = d.argmin(axis=1)
    return d[np.arange(d.shape[0]), face], face, d


def to_face(query, verts, faces, face):
    """The fp64 squared distance and barycentric coordinates of query i to face[i] -> ([n], [n, 3])."""
    v = np.asarray(verts, dtype=np.float64)
    f = np.asarray(faces, dtype=np.int64)[np.asarray(face, dtype=np.int64)]
    return closest(np.asarray(query, dtype=np.float64), v[f[:, 0]], v[f[:, 1]], v[f[:, 2]])


def corner_r2(query, verts, faces, face):
    """The largest squared distance (fp64) from query i to the corners of face[i]: the envelope's unit is U * this."""
    v = np.asarray(verts, dtype=np.float64)
    f = np.asarray(faces, dtype=np.int64)[np.asarray(face, dtype=np.int64)]
    d = v[f] - np.asarray(query, dtype=np.float64)[:, None, :]
    return (d * d).sum(-1).max(axis=1)


def icosphere(level=3):
    """A unit icosahedron subdivided `level` times (20 * 4^level faces: 1280 at 3) -> (verts [V, 3] float32, faces [F, 3] int64)."""
    g = (1.0 + 5.0 ** 0.5) / 2.0
    verts = [(-1, g, 0), (1, g, 0), (-1, -g, 0), (1, -g, 0), (0, -1, g), (0, 1, g), (0, -1, -g), (0, 1, -g), (g, 0, -1), (g, 0, 1),
             (-g, 0, -1), (-g, 0, 1)]
    verts = [np.array(v, dtype=np.float64) / np.linalg.norm(v) for v in verts]
    faces = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
             (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    for _ in range(level):
        mid, out = {}, []

        def midpoint(i, j):
            key = (min(i, j), max(i, j))
            if key not in mid:
                m = verts[i] + verts[j]
                verts.append(m / np.linalg.norm(m))
                mid[key] = len(verts) - 1
            return mid[key]

        for (a, b, c) in faces:
            ab, bc, ca = midpoint(a, b), midpoint(b, c), midpoint(c, a)
            out += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        faces = out
    return np.array(verts, dtype=np.float32), np.array(faces, dtype=np.int64)


def sphere_queries(n, seed, radii=(0.5, 0.9, 1.0, 1.1, 3.0)):
    """n points in random directions at the given radii in turn (inside, near, on, outside the unit sphere), float32."""
    rng = np.random.default_rng(seed)
    d = rng.standard_normal((n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    r = np.asarray(radii, dtype=np.float64)[np.arange(n) % len(radii)]
    return (d * r[:, None]).astype(np.float32)
