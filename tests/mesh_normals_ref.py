"""numpy emulation of include/nsdp_meshnormals.h, as the header writes the rule: the corner lists (a stable sort of the live
corners by the packed vertex row they name), the area-weighted face normals and their fixed-order sums per vertex in fp32 with
one rounding per operation (``list_order_ref.ordered_sum`` is the order), the unit normals -- what the kernels are held to, bit
for bit -- and an fp64 evaluation from the same fp32 positions with the magnitudes the error bound of the CPU test needs.

Offsets are taken as the header wants them: non-decreasing from 0 and within the capacities (they are clamped the way
csrc/packed_rows.h clamps them all the same); face indices may be anything."""
import numpy as np

from list_order_ref import ordered_sum

CYCLIC = ((1, 2), (2, 0), (0, 1))          # component k of a cross product: e1[i] e2[j] - e1[j] e2[i]


def _offsets(offsets, cap):
    o = np.clip(np.asarray(offsets, dtype=np.int64), 0, cap)
    return np.maximum.accumulate(o)


def corner_rows(faces, face_offsets, vert_offsets, vcap):
    """faces (fcap, 3) -> (rows (fcap, 3) int64: the packed vertex row every corner names, live (fcap,) bool)."""
    faces = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    fcap = faces.shape[0]
    fo, vo = _offsets(face_offsets, fcap), _offsets(vert_offsets, vcap)
    B = len(fo) - 1
    q = np.arange(fcap)
    live = (q >= fo[0]) & (q < fo[B])
    b = np.clip(np.searchsorted(fo[1:], q, side="right"), 0, B - 1)
    first, n = vo[b], vo[b + 1] - vo[b]
    rows = np.minimum(first[:, None] + np.clip(faces, 0, np.maximum(n - 1, 0)[:, None]), vcap - 1)
    return rows, live


def corner_lists(faces, face_offsets, vert_offsets, vcap):
    """(list_offsets (vcap + 1) int32, list_entries (3 fcap) int32): the stable sort of the live corners by row, zeros behind."""
    rows, live = corner_rows(faces, face_offsets, vert_offsets, vcap)
    corners = np.flatnonzero(np.repeat(live, 3))
    named = rows.reshape(-1)[corners]
    order = np.argsort(named, kind="stable")
    entries = np.zeros(rows.size, dtype=np.int32)
    entries[:corners.size] = corners[order]
    offsets = np.zeros(vcap + 1, dtype=np.int32)
    offsets[1:] = np.cumsum(np.bincount(named, minlength=vcap))
    return offsets, entries


def face_normals(verts, rows, live, dtype=np.float32):
    """verts (vcap, 3) -> N (fcap, 3) in ``dtype`` (one rounding per operation), +0 for dead faces."""
    p = np.asarray(verts, dtype=np.float32).astype(dtype)
    a, b, c = p[rows[:, 0]], p[rows[:, 1]], p[rows[:, 2]]
    e1, e2 = b - a, c - a
    n = np.stack([e1[:, i] * e2[:, j] - e1[:, j] * e2[:, i] for i, j in CYCLIC], axis=1)
    n[~live] = 0
    assert n.dtype == dtype
    return n


def unit(s):
    """sums (R, 3) fp32 -> unit normals (R, 3) fp32 by the header's rule."""
    s = np.asarray(s, dtype=np.float32)
    m = np.abs(s).max(axis=1)
    ok = np.isfinite(s).all(axis=1) & (m > 0)
    out = np.zeros_like(s)
    with np.errstate(all="ignore"):
        t = s[ok] / m[ok, None]
        qn = (t[:, 0] * t[:, 0] + t[:, 1] * t[:, 1]) + t[:, 2] * t[:, 2]
        out[ok] = t / np.sqrt(qn)[:, None]
    assert out.dtype == np.float32
    return out


def vertex_normals(verts, faces, face_offsets, vert_offsets):
    """One pose: verts (vcap, 3) fp32 -> dict of list_offsets, list_entries, face_normals (fcap, 3), sums and normals (vcap, 3),
    every array with the kernel's bits."""
    verts = np.ascontiguousarray(verts, dtype=np.float32)
    vcap = verts.shape[0]
    rows, live = corner_rows(faces, face_offsets, vert_offsets, vcap)
    offsets, entries = corner_lists(faces, face_offsets, vert_offsets, vcap)
    with np.errstate(all="ignore"):
        fn = face_normals(verts, rows, live)
        sums = np.zeros((vcap, 3), dtype=np.float32)
        for r in np.flatnonzero(np.diff(offsets)):
            sums[r] = ordered_sum(fn[entries[offsets[r]:offsets[r + 1]] // 3])
    return {"list_offsets": offsets, "list_entries": entries, "face_normals": fn, "sums": sums, "normals": unit(sums)}


def reference64(verts, faces, face_offsets, vert_offsets):
    """The same fp32 positions in float64: (sums64 (vcap, 3), magnitudes (vcap, 3), lengths (vcap,)) with
    magnitudes[r][k] = the sum over r's corners of M_q[k] = |e1[i] e2[j]| + |e1[j] e2[i]| -- what a rounding error of a term is
    relative to."""
    verts = np.ascontiguousarray(verts, dtype=np.float32)
    vcap = verts.shape[0]
    rows, live = corner_rows(faces, face_offsets, vert_offsets, vcap)
    offsets, entries = corner_lists(faces, face_offsets, vert_offsets, vcap)
    p = verts.astype(np.float64)
    e1, e2 = p[rows[:, 1]] - p[rows[:, 0]], p[rows[:, 2]] - p[rows[:, 0]]
    n = np.stack([e1[:, i] * e2[:, j] - e1[:, j] * e2[:, i] for i, j in CYCLIC], axis=1)
    mag = np.stack([np.abs(e1[:, i] * e2[:, j]) + np.abs(e1[:, j] * e2[:, i]) for i, j in CYCLIC], axis=1)
    n[~live], mag[~live] = 0, 0
    live_entries = entries[:offsets[-1]] // 3
    owner = np.repeat(np.arange(vcap), np.diff(offsets))
    sums, mags = np.zeros((vcap, 3)), np.zeros((vcap, 3))
    np.add.at(sums, owner, n[live_entries])
    np.add.at(mags, owner, mag[live_entries])
    return sums, mags, np.diff(offsets)


def smallest_intermediate(verts, faces, face_offsets, vert_offsets):
    """The smallest non-zero magnitude among the edges, the products, the face normals and the sums of the fp32 evaluation:
    scaling the mesh by 2^-k is exact (and keeps every bit of the normals) as long as this times 2^-2k stays a normal fp32."""
    verts = np.ascontiguousarray(verts, dtype=np.float32)
    rows, live = corner_rows(faces, face_offsets, vert_offsets, verts.shape[0])
    a, b, c = verts[rows[live, 0]], verts[rows[live, 1]], verts[rows[live, 2]]
    e1, e2 = b - a, c - a
    prods = [e1[:, i] * e2[:, j] for i in range(3) for j in range(3) if i != j]
    out = vertex_normals(verts, faces, face_offsets, vert_offsets)
    edge = min(float(np.abs(v[v != 0]).min()) for v in (e1, e2))
    rest = min(float(np.abs(v[v != 0]).min()) for v in prods + [out["face_normals"], out["sums"]])
    return edge, rest


def pack(meshes, vcap=None, fcap=None):
    """[(verts (V, 3), faces (F, 3)), ...] -> (verts (vcap, 3) fp32, faces (fcap, 3) int32, face_offsets, vert_offsets), rows
    beyond the totals zero."""
    vo = np.concatenate([[0], np.cumsum([len(v) for v, _ in meshes])]).astype(np.int32)
    fo = np.concatenate([[0], np.cumsum([len(f) for _, f in meshes])]).astype(np.int32)
    vcap, fcap = max(int(vo[-1]) if vcap is None else vcap, 1), max(int(fo[-1]) if fcap is None else fcap, 1)
    verts, faces = np.zeros((vcap, 3), np.float32), np.zeros((fcap, 3), np.int32)
    for b, (v, f) in enumerate(meshes):
        verts[vo[b]:vo[b + 1]] = np.asarray(v, dtype=np.float32).reshape(-1, 3)
        faces[fo[b]:fo[b + 1]] = np.asarray(f, dtype=np.int32).reshape(-1, 3)
    return verts, faces, fo, vo


# ---------------------------------------------------------------------------------------------------------------- the test meshes
def triangle():
    return np.array([[0.1, 0.2, 0.3], [0.5, 0.1, 0.2], [0.2, 0.6, 0.1]], np.float32), np.array([[0, 1, 2]], np.int32)


def tetrahedron():
    """Counter-clockwise seen from outside (the CPU test holds it to that), not regular: no two sums alike."""
    v = 0.3 * np.array([[1, 1, 1], [1, -1, -1], [-1, 1, -1], [-1, -1, 1]], np.float64) + np.array([[0.01, 0.02, -0.03], [0, 0.04, 0.01],
                                                                                                  [-0.02, 0, 0.03], [0.05, -0.01, 0]])
    return v.astype(np.float32), np.array([[0, 1, 2], [0, 2, 3], [0, 3, 1], [1, 3, 2]], np.int32)


def sphere(rings, segments):
    from nsdp_amd import synth
    v, f = synth.sphere_mesh(rings, segments)
    return v.astype(np.float32), f


def cases():
    """name -> (meshes, vcap or None, fcap or None): the shapes of the GPU bit test, smallest first."""
    tv, tf = tetrahedron()
    tri_v, tri_f = triangle()
    s612, s340 = sphere(6, 12), sphere(3, 40)
    stale = s612[1].copy()
    stale[::7, 0], stale[3::11, 1], stale[5::13, 2] = -3, 1 << 30, 74 + 5           # (beyond the shape, inside the packed set)
    return {
        "triangle": ([(tri_v, tri_f)], None, None),
        "tetrahedron": ([(tv, tf)], None, None),
        "lane": ([s612], None, None),                                               # every list <= 32
        "wave": ([s340], None, None),                                               # the poles: 40 corners
        "workgroup": ([sphere(2, 1100)], None, None),                               # the poles: 1100 corners
        "packed": ([s612, (tv, tf), s340, (tri_v, tri_f)], 300, 420),               # 74 + 4 + 122 + 3 = 203 rows, 144 + 4 + 240 + 1 = 389 faces
        "no_faces": ([s612, (tri_v, np.zeros((0, 3), np.int32)), (tv, tf)], None, 160),
        "isolated": ([(np.concatenate([tv, [[0.7, 0.7, 0.7]]]).astype(np.float32), tf)], None, None),
        "repeated": ([(tv, np.concatenate([tf, [[0, 0, 1], [2, 2, 2]]]).astype(np.int32))], None, None),
        "cancelling": ([(tri_v, np.array([[0, 1, 2], [0, 2, 1]], np.int32))], None, None),
        "stale": ([(tv, tf), (s612[0], stale), (tv, tf)], 90, None),
    }
