"""The numpy emulation of nsdp_mesh_batch_sample, from the rule written out in include/nsdp_meshbatch.h -- unsigned 32-bit integers,
and fp32 with one rounding per operation, which is what numpy's float32 arrays compute -- with every clamp of the header, so that
stale tables can be emulated too; and the procedural test meshes.  Shared by tests/test_mesh_store_cpu.py,
tests/test_mesh_store_gpu.py and tests/test_mesh_store_arena_gpu.py."""
import numpy as np

import subset_ref as sr

MESH_SURFACE, MESH_SPACE = 2, 3
MAX_ELEMS = 1 << 21
_U = np.uint32
_F = np.float32
ONE24 = 1 << 24
KEYS = ["surface_samples_cano", "surface_samples_src", "surface_samples_tgt", "surface_normals_cano", "surface_normals_src",
        "surface_normals_tgt", "cano_handle_sample_idx", "surface_samples_inputs", "space_samples_cano", "space_samples_src",
        "space_samples_tgt"]


# ---------------------------------------------------------------------------------------------------------------- test meshes
def tetrahedron():
    verts = np.array([[0.0, 0.0, 0.0], [0.5, 0.0, 0.0], [0.0, 0.375, 0.0], [0.0, 0.0, 0.25]])
    return verts, np.array([[0, 2, 1], [0, 1, 3], [0, 3, 2], [1, 2, 3]], dtype=np.int32)


def octahedron(subdivisions=1):
    """An octahedron whose faces are split into four ``subdivisions`` times (1: 18 vertices, 32 faces), on a sphere of radius 0.3."""
    verts = [(1.0, 0, 0), (-1.0, 0, 0), (0, 1.0, 0), (0, -1.0, 0), (0, 0, 1.0), (0, 0, -1.0)]
    faces = [(0, 2, 4), (2, 1, 4), (1, 3, 4), (3, 0, 4), (2, 0, 5), (1, 2, 5), (3, 1, 5), (0, 3, 5)]
    for _ in range(subdivisions):
        mid, out = {}, []

        def midpoint(a, b):
            key = (min(a, b), max(a, b))
            if key not in mid:
                mid[key] = len(verts)
                verts.append(tuple((np.asarray(verts[a]) + np.asarray(verts[b])) / 2.0))
            return mid[key]

        for a, b, c in faces:
            ab, bc, ca = midpoint(a, b), midpoint(b, c), midpoint(c, a)
            out += [(a, ab, ca), (ab, b, bc), (ca, bc, c), (ab, bc, ca)]
        faces = out
    v = np.asarray(verts, dtype=np.float64)
    return 0.3 * v / np.linalg.norm(v, axis=1, keepdims=True), np.asarray(faces, dtype=np.int32)


def grid(zero_area=(17, 199), seed=3):
    """A jittered 10 x 10 grid of 200 faces over [-0.5, 0.5]^2 with a smooth height; the faces ``zero_area`` are degenerate
    (two corners coincide): 199 is the TRAILING face."""
    g = np.random.RandomState(seed)
    x, y = np.meshgrid(np.linspace(-0.5, 0.5, 11), np.linspace(-0.5, 0.5, 11), indexing="ij")
    verts = np.stack([x, y, 0.1 * np.sin(3.0 * x) * np.cos(2.0 * y)], axis=2).reshape(-1, 3)
    verts[:, :2] += 0.02 * (g.rand(121, 2) - 0.5)
    i, j = np.meshgrid(np.arange(10), np.arange(10), indexing="ij")
    a = (i * 11 + j).reshape(-1)
    faces = np.stack([np.stack([a, a + 11, a + 1], axis=1), np.stack([a + 1, a + 11, a + 12], axis=1)], axis=1).reshape(-1, 3)
    for f in zero_area:
        faces[f, 2] = faces[f, 1]
    return verts, faces.astype(np.int32)


def deform(verts, k):
    """Frame k of a sequence: an analytic deformation of the same vertices (k = 0: the vertices as they are)."""
    v = np.asarray(verts, dtype=np.float64)
    return v + 0.05 * k * np.stack([np.sin(4.0 * v[:, 1] + k), np.cos(3.0 * v[:, 2] - k), np.sin(5.0 * v[:, 0]) * np.cos(k)], axis=1)


# ---------------------------------------------------------------------------------------------------------------- the draw
def words(seed, epoch, step, b, which, j):
    """word(c) of the rows ``j`` (array) of sample ``b``: (4, len(j)) uint32."""
    key = sr.keys(seed, epoch, step, np.asarray([b]), which)[0]
    j = np.asarray(j, dtype=_U)
    out = []
    with np.errstate(over="ignore"):
        for c in range(4):
            rk = sr.mix32(key + _U(0x85EBCA6B) * _U(c + 1))
            out.append(sr.mix32(sr.mix32(j ^ rk) + rk))
    return np.stack(out)


def search(T, r):
    """The header's binary search, probe for probe: f = min(lo, F - 1) after  lo = 0, hi = F; while lo < hi: mid = (lo + hi) >> 1;
    T[mid] > r ? hi = mid : lo = mid + 1.  On non-decreasing T: the first f with T[f] > r."""
    F = len(T)
    lo, hi = np.zeros(len(r), np.int64), np.full(len(r), F, np.int64)
    while np.any(lo < hi):
        live = lo < hi
        mid = (lo + hi) >> 1
        above = T[np.minimum(mid, max(F - 1, 0))].astype(np.int64) > r.astype(np.int64) if F else np.zeros(len(r), bool)
        hi = np.where(live & above, mid, hi)
        lo = np.where(live & ~above, mid + 1, lo)
    return np.minimum(lo, max(F - 1, 0))


def weights(w):
    """(iw, iu, iv) int64 from the rows' words (4, N): the integer form of the barycentric rule; they sum to 2^24."""
    iu, iv = (w[1] >> _U(8)).astype(np.int64), (w[2] >> _U(8)).astype(np.int64)
    flip = iu + iv > ONE24
    iu, iv = np.where(flip, ONE24 - iu, iu), np.where(flip, ONE24 - iv, iv)
    return ONE24 - iu - iv, iu, iv


def as_weight(i):
    return i.astype(_F) * _F(2.0 ** -24)


def triangle(a, b, c, w0, u, v):
    """The header's per-frame rule on float32 arrays a, b, c (N, 3) and weights (N,): (point, unit normal or 0)."""
    w0, u, v = w0[:, None], u[:, None], v[:, None]
    p = ((w0 * a) + (u * b)) + (v * c)
    e1, e2 = b - a, c - a
    cr = np.stack([e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1], e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2],
                   e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]], axis=1)
    length = np.sqrt((cr[:, 0] * cr[:, 0] + cr[:, 1] * cr[:, 1]) + cr[:, 2] * cr[:, 2])
    with np.errstate(divide="ignore", invalid="ignore"):
        nrm = np.where(length[:, None] == 0, _F(0), cr / length[:, None])
    assert p.dtype == _F and nrm.dtype == _F
    return p, nrm


def _clamp(v, lo, hi):
    return lo if v < lo else (hi if v > hi else v)


def sample(arrays, frame_ids, n, m, seed, epoch, step, partial_range, sigma1, sigma2, noise=None, noise_level=0.0):
    """nsdp_mesh_batch_sample on the host arrays of ``meshstore.pack`` (or stale ones: every clamp of the header is applied):
    the eleven tensors of the data_dict as numpy arrays."""
    verts, faces, thr = arrays["vert_arena"], arrays["face_arena"], arrays["thr_arena"].view(np.uint32)
    ftab, ttab = arrays["frame_table"], arrays["topo_table"]
    VR, FR, TR = len(verts), len(faces), len(thr)
    B = frame_ids.shape[1]
    surface = np.zeros((6, B, n, 3), _F)
    handle = np.zeros((B, n, 1), bool)
    inputs = np.zeros((B, n, 7), _F)
    space = np.zeros((3, B, m, 3), _F)
    pr, level = _F(partial_range), _F(noise_level)
    for b in range(B):
        entries = [ftab[_clamp(int(frame_ids[c, b]), 0, len(ftab) - 1)] for c in range(3)]
        frames = []
        for e in entries:
            low = int(e[1]) & 0xFFFFFFFF                                     # (the low word as a signed 32-bit integer)
            count = _clamp(low - (1 << 32) if low >= (1 << 31) else low, 0, min(VR, MAX_ELEMS))
            frames.append((_clamp(int(e[0]), 0, VR - count), count))
        ec = entries[0]
        topo = ttab[_clamp(int(ec[1]) >> 32, 0, len(ttab) - 1)]
        F = _clamp(int(topo[1]), 0, min(FR, TR, MAX_ELEMS))
        face_first = _clamp(int(topo[0]), 0, FR - F)
        thr_first = _clamp(int(ec[2]), 0, TR - F)
        T = thr[thr_first:thr_first + F]
        box = ec[3:6].copy().view(_F)                                        # min x y z, max x y z
        for which, rows in ((MESH_SURFACE, n), (MESH_SPACE, m)):
            if rows == 0:
                continue
            w = words(seed, epoch, step, b, which, np.arange(rows))
            f = search(T, w[0] >> _U(1))
            face = faces[np.clip(face_first + f, 0, FR - 1)][:, :3].astype(np.int64)
            iw, iu, iv = weights(w)
            w0, u, v = as_weight(iw), as_weight(iu), as_weight(iv)
            got = []
            for first, count in frames:
                rec = np.clip(first + np.clip(face, 0, max(count - 1, 0)), 0, VR - 1)
                got.append(triangle(verts[rec[:, 0], :3], verts[rec[:, 1], :3], verts[rec[:, 2], :3], w0, u, v))
            if which == MESH_SURFACE:
                (pc, nc), (ps, ns), (pt, nt) = got
                if noise is not None:
                    ps = ps + level * noise[b]
                mask = (pc[:, 1] < box[1] + pr) | (pc[:, 1] > box[4] - pr) | (pc[:, 2] < box[2] + pr)
                mf = mask.astype(_F)
                for k, a in enumerate((pc, ps, pt, nc, ns, nt)):
                    surface[k, b] = a
                handle[b, :, 0] = mask
                inputs[b] = np.concatenate([ps, pt * mf[:, None], mf[:, None]], axis=1)
            else:
                t = _F(2) * as_weight((w[3] >> _U(8)).astype(np.int64)) - _F(1)
                d = t * np.where(np.arange(rows) < rows // 2, _F(sigma1), _F(sigma2)).astype(_F)
                for k, (p, nrm) in enumerate(got):
                    space[k, b] = p + nrm * d[:, None]
    out = {KEYS[k]: surface[k] for k in range(6)}
    out["cano_handle_sample_idx"], out["surface_samples_inputs"] = handle, inputs
    for k in range(3):
        out[KEYS[8 + k]] = space[k]
    return out
