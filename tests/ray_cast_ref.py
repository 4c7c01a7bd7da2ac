"""numpy emulation of include/nsdp_raycast.h, operation by operation as the header writes the rule -- the fp32 ray frame and
shear, the exact fp64 edge signs with their symbolic tie-break, the fp64 depth, the 64-bit key -- and the packed entry with its
clamps; then the same questions asked of rational arithmetic (fractions.Fraction of the fp32 sheared corners): is the generic
point (e, e^2) inside the projected triangle, and what is the exact quotient t*.  The GPU tests hold the kernel to the emulation
byte for byte; tests/test_ray_cast_ref_cpu.py holds the emulation to the rationals.

The envelopes:  |t - t*| <= 2^-24 |t*| + 2^-50 max|z|   (T_REL, T_ABS below; 2^-149 more in the denormal range)."""
from fractions import Fraction

import numpy as np

f32, f64 = np.float32, np.float64
FLT_MAX = np.float32(np.finfo(np.float32).max)
START_KEY = (np.uint64(0x7F7FFFFF) << np.uint64(32)) | np.uint64(0xFFFFFFFF)
T_REL, T_ABS = Fraction(1, 2 ** 24), Fraction(1, 2 ** 50)
SHEAR_XY, SHEAR_Z = 6, 3                 # |x - x*| <= 6 * 2^-24 * R,  |z - z*| <= 3 * 2^-24 |z*|


# ------------------------------------------------------------------------------------------------------------------ the rule
def frame(o, d):
    """The ray frames of o, d (n, 3) fp32 -> dict of kx, ky, kz (n), Sx, Sy, Sz (n) fp32, ok (n)."""
    o, d = np.asarray(o, f32).reshape(-1, 3), np.asarray(d, f32).reshape(-1, 3)
    n = len(d)
    r = np.arange(n)
    ad = np.abs(d)
    kz = np.argmax(ad, axis=1)                       # (the first of several equal maxima: the lowest axis)
    kx, ky = (kz + 1) % 3, (kz + 2) % 3
    dz = d[r, kz]
    kx, ky = np.where(dz < 0, ky, kx), np.where(dz < 0, kx, ky)
    ok = ad.max(axis=1) != 0
    den = np.where(ok, dz, f32(1))
    return {"o": o, "kx": kx, "ky": ky, "kz": kz, "Sx": d[r, kx] / den, "Sy": d[r, ky] / den, "Sz": f32(1) / den, "ok": ok}


def shear(fr, c):
    """Corners c (n, m, 3) fp32 (m corners for every ray) in the rays' frames -> x, y, z (n, m) fp32."""
    C = c - fr["o"][:, None, :]
    take = lambda k: np.take_along_axis(C, k[:, None, None], axis=2)[:, :, 0]
    Cz = take(fr["kz"])
    x = take(fr["kx"]) - fr["Sx"][:, None] * Cz
    y = take(fr["ky"]) - fr["Sy"][:, None] * Cz
    z = fr["Sz"][:, None] * Cz
    assert x.dtype == f32 and y.dtype == f32 and z.dtype == f32
    return x, y, z


def edge_sign(Px, Py, Qx, Qy):
    """s(P, Q) and the two exact products; fp32 arrays in."""
    l, r = Qx.astype(f64) * Py.astype(f64), Qy.astype(f64) * Px.astype(f64)
    s = np.sign(l - r)                               # (the rounded difference of two doubles has the sign of the exact one)
    s = np.where(s == 0, np.sign(Qy.astype(f64) - Py.astype(f64)), s)
    s = np.where(s == 0, np.sign(Px.astype(f64) - Qx.astype(f64)), s)
    return s.astype(np.int8), l, r


def face_tests(fr, a, b, c):
    """Faces with corners a, b, c (n, F, 3) against the n rays -> dict: covered, hit (n, F) bool, t (n, F) fp32, bary (n, F, 3)
    fp32 (t, bary meaningful where hit), ties: the number of exactly tied edge functions (equal products)."""
    ax, ay, az = shear(fr, a)
    bx, by, bz = shear(fr, b)
    cx, cy, cz = shear(fr, c)
    su, lu, ru = edge_sign(bx, by, cx, cy)
    sv, lv, rv = edge_sign(cx, cy, ax, ay)
    sw, lw, rw = edge_sign(ax, ay, bx, by)
    covered = (su != 0) & (su == sv) & (sv == sw)
    U, V, W = lu - ru, lv - rv, lw - rw
    det = (U + V) + W
    T = (U * az.astype(f64) + V * bz.astype(f64)) + W * cz.astype(f64)
    hit = covered & (((T > 0) & (det > 0)) | ((T < 0) & (det < 0))) & fr["ok"][:, None]
    with np.errstate(all="ignore"):
        safe = np.where(det == 0, 1.0, det)
        t = (T / safe).astype(f32)
        bary = np.stack([(U / safe).astype(f32), (V / safe).astype(f32), (W / safe).astype(f32)], axis=-1)
    live = fr["ok"][:, None]
    ties = int(((lu == ru) & live).sum() + ((lv == rv) & live).sum() + ((lw == rw) & live).sum())
    return {"covered": covered & live, "hit": hit, "t": t, "bary": bary, "ties": ties, "signs": (su, sv, sw),
            "xyz": ((ax, ay, az), (bx, by, bz), (cx, cy, cz))}


def cast(o, d, verts, faces, row0=0, chunk=256):
    """One mesh (verts (V, 3) fp32, faces (F, 3) valid indices) against n rays -> t (n) fp32, face (n) int32 (row0 + the face, -1:
    none), bary (n, 3) fp32, count (n) int32, covered (n) int32, ties (int)."""
    o, d = np.asarray(o, f32).reshape(-1, 3), np.asarray(d, f32).reshape(-1, 3)
    verts, faces = np.asarray(verts, f32), np.asarray(faces).astype(np.int64)
    n, F = len(o), len(faces)
    t, face = np.full(n, FLT_MAX, f32), np.full(n, -1, np.int32)
    bary, count, covered, ties = np.zeros((n, 3), f32), np.zeros(n, np.int32), np.zeros(n, np.int32), 0
    if F == 0:
        return t, face, bary, count, covered, ties
    tri = verts[faces]                                                   # (F, 3, 3)
    rows = (np.arange(F, dtype=np.uint64) + np.uint64(row0))[None, :]
    for lo in range(0, n, chunk):
        fr = frame(o[lo:lo + chunk], d[lo:lo + chunk])
        k = len(fr["ok"])
        r = face_tests(fr, *(np.broadcast_to(tri[None, :, j], (k, F, 3)) for j in range(3)))
        key = (r["t"].view(np.uint32).astype(np.uint64) << np.uint64(32)) | rows
        key = np.where(r["hit"], key, START_KEY)
        w = np.argmin(key, axis=1)                                       # (keys of hits are distinct: the face row is in them)
        best = key[np.arange(k), w]
        found = best < START_KEY
        t[lo:lo + k] = np.where(found, r["t"][np.arange(k), w], FLT_MAX)
        face[lo:lo + k] = np.where(found, w + row0, -1)
        bary[lo:lo + k] = np.where(found[:, None], r["bary"][np.arange(k), w], f32(0))
        count[lo:lo + k] = r["hit"].sum(axis=1)
        covered[lo:lo + k] = r["covered"].sum(axis=1)
        ties += r["ties"]
    return t, face, bary, count, covered, ties


def clamp_offsets(off, cap):
    out, prev = [], None
    for v in np.asarray(off).astype(np.int64):
        prev = min(max(int(v), 0 if prev is None else prev), cap)
        out.append(prev)
    return out


def ray_cast(origins, dirs, roff, verts, voff, faces, foff):
    """The packed entry with its clamps -> t, face, bary, count over the qcap rows; rows the entry does not write hold NaN / -9."""
    origins, dirs, verts = np.asarray(origins, f32), np.asarray(dirs, f32), np.asarray(verts, f32)
    faces = np.asarray(faces).astype(np.int64)
    qcap, vcap, fcap, B = len(origins), len(verts), len(faces), len(roff) - 1
    ro, vo, fo = clamp_offsets(roff, qcap), clamp_offsets(voff, vcap), clamp_offsets(foff, fcap)
    t, face = np.full(qcap, np.nan, f32), np.full(qcap, -9, np.int32)
    bary, count = np.full((qcap, 3), np.nan, f32), np.full(qcap, -9, np.int32)
    for b in range(B):
        q0, q1, vn = ro[b], ro[b + 1], vo[b + 1] - vo[b]
        f0, f1 = fo[b], (fo[b + 1] if vn > 0 else fo[b])
        local = np.clip(faces[f0:f1], 0, max(vn - 1, 0))
        r = cast(origins[q0:q1], dirs[q0:q1], verts[vo[b]:vo[b + 1]], local, row0=f0)
        t[q0:q1], face[q0:q1], bary[q0:q1], count[q0:q1] = r[:4]
    return t, face, bary, count


# ------------------------------------------------------------------------------------------------------------------ rationals
_EPS = Fraction(1, 2 ** 400)      # below every ratio of two nonzero differences of products of fp32 numbers (>= 2^-298 / 2^130)


def exact_face(xyz):
    """xyz: three (x, y, z) of fp32 sheared corners a, b, c -> (inside, tstar, zmax): is the point (e, e^2), e = 2^-400, strictly
    inside the projected triangle (either orientation) by exact edge functions; the exact quotient t* (None where det* = 0)."""
    (ax, ay, az), (bx, by, bz), (cx, cy, cz) = [[Fraction(float(v)) for v in p] for p in xyz]
    px, py = _EPS, _EPS * _EPS

    def fn(Px, Py, Qx, Qy):
        return (Qx - px) * (Py - py) - (Qy - py) * (Px - px)

    e = [fn(bx, by, cx, cy), fn(cx, cy, ax, ay), fn(ax, ay, bx, by)]
    inside = all(v > 0 for v in e) or all(v < 0 for v in e)
    U, V, W = cx * by - cy * bx, ax * cy - ay * cx, bx * ay - by * ax
    det = U + V + W
    tstar = (U * az + V * bz + W * cz) / det if det != 0 else None
    return inside, tstar, max(abs(az), abs(bz), abs(cz))


def t_bound(tstar, zmax):
    return T_REL * abs(tstar) + T_ABS * zmax + Fraction(1, 2 ** 149)


# ------------------------------------------------------------------------------------------------------------------ meshes
def cube(lo=-1.0, hi=1.0):
    """12 faces, outward, closed."""
    v = np.array([[x, y, z] for x in (lo, hi) for y in (lo, hi) for z in (lo, hi)], f32)
    q = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]
    f = np.array([t for a, b, c, d in q for t in ((a, b, c), (a, c, d))], np.int64)
    return v, f


def uv_sphere(segments=12, rings=10, radius=1.0, grid=None):
    """A UV sphere: 2 poles of valence `segments`, (rings - 1) rings -> 2 * segments * (rings - 1) faces (216 by default).  With
    ``grid`` the coordinates are rounded to multiples of 1 / grid (a power of two: sums and differences of them are exact)."""
    v = [[0.0, 0.0, radius]]
    for i in range(1, rings):
        th = np.pi * i / rings
        for j in range(segments):
            ph = 2 * np.pi * j / segments
            v.append([radius * np.sin(th) * np.cos(ph), radius * np.sin(th) * np.sin(ph), radius * np.cos(th)])
    v.append([0.0, 0.0, -radius])
    v = np.array(v, f64)
    if grid:
        v = np.round(v * grid) / grid
    ring = lambda i, j: 1 + (i - 1) * segments + j % segments
    f, last = [], len(v) - 1
    for j in range(segments):
        f.append((0, ring(1, j), ring(1, j + 1)))
        f.append((last, ring(rings - 1, j + 1), ring(rings - 1, j)))
        for i in range(1, rings - 1):
            f.append((ring(i, j), ring(i + 1, j), ring(i + 1, j + 1)))
            f.append((ring(i, j), ring(i + 1, j + 1), ring(i, j + 1)))
    return v.astype(f32), np.array(f, np.int64)


def sphere(n_lat=40, n_lon=64, radius=1.0):
    """A finer UV sphere (2 * n_lon * (n_lat - 1) faces: 4992 by default)."""
    return uv_sphere(n_lon, n_lat, radius)


def open_edges(faces):
    """Undirected edges not used by exactly two faces."""
    f = np.asarray(faces).astype(np.int64)
    e = np.sort(np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]]), axis=1)
    _, n = np.unique(e, axis=0, return_counts=True)
    return int((n != 2).sum())


def is_convex(v, f):
    """Exactly (rationals): no vertex strictly outside a face's plane, faces outward."""
    V = [[Fraction(float(x)) for x in p] for p in v]
    for a, b, c in f:
        A, B, C = V[a], V[b], V[c]
        u, w = [B[i] - A[i] for i in range(3)], [C[i] - A[i] for i in range(3)]
        nrm = [u[1] * w[2] - u[2] * w[1], u[2] * w[0] - u[0] * w[2], u[0] * w[1] - u[1] * w[0]]
        if any(sum(nrm[i] * (p[i] - A[i]) for i in range(3)) > 0 for p in V):
            return False
    return True


_DIRS = [(1, 0, 0), (0, 1, 0), (0, 0, 1), (-1, 0, 0), (0, -1, 0), (0, 0, -1)] + \
        [(sx, sy, sz) for sx in (1, -1) for sy in (1, -1) for sz in (1, -1)] + \
        [(1, 1, 0), (1, 0, -1), (0, -1, 1), (-1, 1, 0)]


def tie_set(v, f, seed=0, n_random=6, dist=8.0):
    """Rays aimed bitwise at every vertex and every edge midpoint of the mesh (coordinates on a binary grid, so midpoints,
    origins and directions are exact): from OUTSIDE along the axes, the diagonals and random directions (origin = target -
    dist * direction), and from the CENTRE (the origin of coordinates) towards every target -> (o_out, d_out, o_in, d_in)."""
    rng = np.random.default_rng(seed)
    f = np.asarray(f)
    e = np.unique(np.sort(np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]]), axis=1), axis=0)
    targets = np.concatenate([v, (v[e[:, 0]] + v[e[:, 1]]) * f32(0.5)]).astype(f32)
    o, d = [], []
    for tg in targets:
        dirs = [np.array(u, f32) for u in _DIRS]
        while len(dirs) < len(_DIRS) + n_random:
            u = np.round(rng.standard_normal(3) * 64).astype(f32) / f32(64)
            if np.abs(u).max() >= 0.5:                                    # (so that the origin is outside: dist * |u| >= 4)
                dirs.append(u)
        for u in dirs:
            start = (tg - f32(dist) * u).astype(f32)
            o.append(start)
            d.append((tg - start).astype(f32))                            # aimed bitwise: o + 1 * d is the target where exact
    o_in = np.zeros_like(targets)
    return np.array(o, f32), np.array(d, f32), o_in, targets.copy()
