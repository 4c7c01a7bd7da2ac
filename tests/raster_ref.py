"""numpy emulation of include/nsdp_raster.h, operation by operation as the header writes the rule -- the fp32 corner, the snap,
the dropped faces, the exact int64 edge signs with their symbolic tie-break, the fp64 perspective-correct depth and weights, the
64-bit key -- and the packed entry with its clamps; then the same questions asked of rational arithmetic (fractions.Fraction
on the snapped corners and the fp32 Z, W): is the centre displaced by (e, e^2) strictly inside the triangle, and what is the
exact depth d*.  The GPU tests hold the kernel to the emulation byte for byte; tests/test_raster_ref_cpu.py holds the emulation
to the rationals.

The envelope:  |depth - d*| <= 2^-24 |d*| + 11 * 2^-53 max|Z|   (D_REL, D_ABS below; 2^-149 more in the
denormal range)."""
from fractions import Fraction

import numpy as np

from ray_cast_ref import clamp_offsets, cube, open_edges, uv_sphere      # noqa: F401  (the meshes and the offsets clamp are shared)

f32, f64, i64 = np.float32, np.float64, np.int64
FLT_MAX = np.float32(np.finfo(np.float32).max)
NO_FACE = np.uint64(0xFFFFFFFF)
START_KEY = (np.uint64(0xFF7FFFFF) << np.uint64(32)) | NO_FACE
D_REL, D_ABS = Fraction(1, 2 ** 24), Fraction(11, 2 ** 53)
SNAP_MAX = f32(2 ** 24)
FRONT_ONLY = 1


# ------------------------------------------------------------------------------------------------------------------ the rule
def corners(verts, M):
    """verts (n, 3) fp32 under the camera M (16 or 4 x 4, fp32) -> dict of sx, sy (n) int64, Z, W (n) fp32, ok (n)."""
    v, M = np.asarray(verts, f32).reshape(-1, 3), np.asarray(M, f32).reshape(16)
    x, y, z = v[:, 0], v[:, 1], v[:, 2]
    with np.errstate(all="ignore"):
        row = lambda r: ((M[4 * r] * x + M[4 * r + 1] * y) + M[4 * r + 2] * z) + M[4 * r + 3]
        X, Y, Z, W = row(0), row(1), row(2), row(3)
        assert X.dtype == f32 and W.dtype == f32
        px, py = X / W, Y / W
        rx, ry = np.rint(px * f32(256)), np.rint(py * f32(256))
        assert rx.dtype == f32
        ok = (W > 0) & np.isfinite(X) & np.isfinite(Y) & np.isfinite(Z) & np.isfinite(W) & (np.abs(rx) <= SNAP_MAX) & (np.abs(ry) <= SNAP_MAX)
    sx, sy = np.where(ok, rx, 0).astype(i64), np.where(ok, ry, 0).astype(i64)
    return {"sx": sx, "sy": sy, "Z": Z, "W": W, "ok": ok}


def ordered(d):
    """The order-preserving map of fp32 values to uint32."""
    u = np.asarray(d, f32).view(np.uint32)
    return np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000)).astype(np.uint32)


def edge(Px, Py, Qx, Qy, cx, cy):
    """E and s of the ordered pair (P, Q) at the centres (cx, cy); int64 arrays that broadcast."""
    E = (Qx - cx) * (Py - cy) - (Qy - cy) * (Px - cx)
    s = np.sign(E)
    s = np.where(s == 0, np.sign(Qy - Py), s)
    s = np.where(s == 0, np.sign(Px - Qx), s)
    return E, s.astype(np.int8)


def image(verts, faces, M, H, W, front=False, row0=0, chunk=64):
    """One mesh (verts (V, 3) fp32, faces (F, 3) valid indices) under one camera -> dict: depth (H, W) fp32, face (H, W) int32
    (row0 + the face, -1: none), bary (H, W, 3) fp32, count (H, W) int32, dropped (int), ties: the number of edge functions that
    were exactly 0 at a centre, second (H, W) fp32: the depth of the runner-up key (FLT_MAX without one)."""
    faces = np.asarray(faces).astype(i64).reshape(-1, 3)
    F = len(faces)
    c = corners(verts, M)
    best = np.full((H, W), START_KEY, np.uint64)
    second = np.full((H, W), START_KEY, np.uint64)
    bary, count = np.zeros((H, W, 3), f32), np.zeros((H, W), np.int32)
    cy, cx = np.meshgrid(np.arange(H, dtype=i64) * 256 + 128, np.arange(W, dtype=i64) * 256 + 128, indexing="ij")
    good = c["ok"][faces].all(axis=1) if F else np.zeros(0, bool)
    ties = 0
    for lo in range(0, F, chunk):
        sel = np.nonzero(good[lo:lo + chunk])[0] + lo
        if len(sel) == 0:
            continue
        a, b, cc = faces[sel, 0], faces[sel, 1], faces[sel, 2]
        g = lambda name, idx: c[name][idx][:, None, None]
        E0, s0 = edge(g("sx", b), g("sy", b), g("sx", cc), g("sy", cc), cx, cy)
        E1, s1 = edge(g("sx", cc), g("sy", cc), g("sx", a), g("sy", a), cx, cy)
        E2, s2 = edge(g("sx", a), g("sy", a), g("sx", b), g("sy", b), cx, cy)
        assert max(np.abs(E0).max(), np.abs(E1).max(), np.abs(E2).max()) < 2 ** 51
        cov = (s0 != 0) & (s0 == s1) & (s1 == s2)
        if front:
            cov &= s0 > 0
        ties += int((E0 == 0).sum() + (E1 == 0).sum() + (E2 == 0).sum())
        iw = lambda idx: (f64(1.0) / c["W"][idx].astype(f64))[:, None, None]
        Z = lambda idx: c["Z"][idx].astype(f64)[:, None, None]
        with np.errstate(all="ignore"):
            ta, tb, tc = np.abs(E0).astype(f64) * iw(a), np.abs(E1).astype(f64) * iw(b), np.abs(E2).astype(f64) * iw(cc)
            s = (ta + tb) + tc
            safe = np.where(cov, s, 1.0)
            d = (((ta * Z(a) + tb * Z(b)) + tc * Z(cc)) / safe).astype(f32)
            w = np.stack([(ta / safe).astype(f32), (tb / safe).astype(f32), (tc / safe).astype(f32)], axis=-1)
        key = (ordered(d).astype(np.uint64) << np.uint64(32)) | (sel.astype(np.uint64) + np.uint64(row0))[:, None, None]
        key = np.where(cov, key, START_KEY)
        count += cov.sum(axis=0).astype(np.int32)
        k = np.argmin(key, axis=0)
        kmin = np.take_along_axis(key, k[None], axis=0)[0]
        rest = key.copy()
        np.put_along_axis(rest, k[None], START_KEY, axis=0)
        second = np.minimum(np.minimum(second, rest.min(axis=0)), np.maximum(best, kmin))
        better = kmin < best
        bary = np.where(better[..., None], np.take_along_axis(w, k[None, ..., None], axis=0)[0], bary)
        best = np.where(better, kmin, best)

    def depth_of(keys):
        o = (keys >> np.uint64(32)).astype(np.uint32)
        return np.where(o & np.uint32(0x80000000), o ^ np.uint32(0x80000000), ~o).astype(np.uint32).view(f32)

    low = (best & NO_FACE).astype(np.uint32)
    return {"depth": depth_of(best), "face": np.where(low == np.uint32(0xFFFFFFFF), -1, low.astype(i64)).astype(np.int32),
            "bary": bary, "count": count, "dropped": int(F - good.sum()), "ties": ties, "second": depth_of(second)}


def rasterize(verts, voff, faces, foff, cams, image_shape, H, W, flags=0):
    """The packed entry with its clamps -> depth (I, H, W), face, bary (I, H, W, 3), count, dropped (I), ties."""
    verts, faces = np.asarray(verts, f32), np.asarray(faces).astype(i64)
    cams = np.asarray(cams, f32).reshape(-1, 16)
    vcap, fcap, B, I = len(verts), len(faces), len(voff) - 1, len(cams)
    vo, fo = clamp_offsets(voff, vcap), clamp_offsets(foff, fcap)
    out = {"depth": np.empty((I, H, W), f32), "face": np.empty((I, H, W), np.int32), "bary": np.empty((I, H, W, 3), f32),
           "count": np.empty((I, H, W), np.int32), "dropped": np.empty(I, np.int32), "ties": 0}
    for i in range(I):
        b = min(max(int(image_shape[i]), 0), B - 1)
        vn = vo[b + 1] - vo[b]
        f0, f1 = fo[b], (fo[b + 1] if vn > 0 else fo[b])
        local = np.clip(faces[f0:f1], 0, max(vn - 1, 0))
        r = image(verts[vo[b]:vo[b + 1]], local, cams[i], H, W, front=bool(flags & FRONT_ONLY), row0=f0)
        for k in ("depth", "face", "bary", "count"):
            out[k][i] = r[k]
        out["dropped"][i] = r["dropped"]
        out["ties"] += r["ties"]
    return out


# ------------------------------------------------------------------------------------------------------------------ cameras
def ortho(scale, tx, ty, tz=0.0):
    """Screen axes +x and +y of the world, `scale` pixels per unit, depth z + tz, W = 1."""
    return f32([[scale, 0, 0, tx], [0, scale, 0, ty], [0, 0, 1, tz], [0, 0, 0, 1]])


def pinhole(focal, cx, cy, tz):
    """An eye at (0, 0, -tz) looking along +z: X = focal x + cx w, Y = focal y + cy w, Z = W = z + tz."""
    return f32([[focal, 0, cx, cx * tz], [0, focal, cy, cy * tz], [0, 0, 1, tz], [0, 0, 1, tz]])


def cross_check_case():
    """The case of the cross-check with the ray cast -> (verts, faces, M, H, W): a closed UV sphere on the 1/4096 grid under an
    orthographic camera of 16 pixels per unit whose screen axes are +x and +y of the world -- every snapped coordinate
    4096 x + 256 * 24.5 is exact, the poles and the y = 0 meridian lie bitwise on pixel centres -- and depth = z + 2, the
    parameter of a ray cast from z = -2 along (0, 0, 1)."""
    v, f = uv_sphere(grid=4096)
    return v, f, ortho(16, 24.5, 24.5, 2), 49, 49


def cross_check_rays(M, H, W, z0=-2.0):
    """One ray per pixel of `cross_check_case`'s camera, row-major: origins on the plane z = z0 under the pixel centres (exact in
    fp32), directions (0, 0, 1)."""
    M = np.asarray(M, f32)
    ys, xs = np.meshgrid(np.arange(H, dtype=f64) + 0.5, np.arange(W, dtype=f64) + 0.5, indexing="ij")
    o = np.stack([(xs - f64(M[0, 3])) / f64(M[0, 0]), (ys - f64(M[1, 3])) / f64(M[1, 1]), np.full_like(xs, z0)], axis=-1)
    assert np.array_equal(o.astype(f32).astype(f64), o)
    return o.astype(f32).reshape(-1, 3), np.tile(f32([0, 0, 1]), (H * W, 1))


# ------------------------------------------------------------------------------------------------------------------ rationals
_EPS = Fraction(1, 2 ** 200)      # below every ratio of two nonzero edge functions of integers below 2^26


def exact_pixel(a, b, c, cx, cy):
    """a, b, c: (sx, sy, Z, W) of three good corners; the centre (cx, cy) -> (inside, dstar, zmax): is the centre displaced by
    (e, e^2) strictly inside the triangle (either orientation) by exact edge functions, the orientation's sign (+1: all edge
    functions positive), and the exact perspective-correct depth at the centre itself (None where all three edge functions
    are 0)."""
    px, py = Fraction(int(cx)) + _EPS, Fraction(int(cy)) + _EPS * _EPS

    def fn(P, Q, x, y):
        return (Fraction(int(Q[0])) - x) * (Fraction(int(P[1])) - y) - (Fraction(int(Q[1])) - y) * (Fraction(int(P[0])) - x)

    e = [fn(b, c, px, py), fn(c, a, px, py), fn(a, b, px, py)]
    inside = all(v > 0 for v in e) or all(v < 0 for v in e)
    side = 1 if e[0] > 0 else -1
    m = [abs(fn(b, c, Fraction(int(cx)), Fraction(int(cy)))), abs(fn(c, a, Fraction(int(cx)), Fraction(int(cy)))),
         abs(fn(a, b, Fraction(int(cx)), Fraction(int(cy))))]
    t = [m[k] / Fraction(float(p[3])) for k, p in enumerate((a, b, c))]
    s = sum(t)
    dstar = sum(t[k] * Fraction(float(p[2])) for k, p in enumerate((a, b, c))) / s if s != 0 else None
    return inside, side, dstar, max(abs(Fraction(float(p[2]))) for p in (a, b, c))


def d_bound(dstar, zmax):
    return D_REL * abs(dstar) + D_ABS * zmax + Fraction(1, 2 ** 149)
