"""numpy emulation of nsdp_mesh_batch_whole, as include/nsdp_meshwhole.h writes the rule: the offsets, the three vertex planes, the
handle bytes, the 7-wide input rows and the faces of a batch of whole meshes, padding included, on the host arrays of
``meshstore.pack`` (or stale ones: every clamp of the header is applied).  The GPU tests hold the kernel to this bit for bit."""
import numpy as np

MAX_ELEMS = 1 << 21
KEYS = ["vert_offsets", "face_offsets", "verts", "handle", "inputs", "faces"]
_F = np.float32


def _clamp(v, lo, hi):
    return lo if v < lo else (hi if v > hi else v)


def counts(arrays, frame_ids):
    """(V_b, F_b) of every shape, clamped as the kernel clamps them."""
    ftab, ttab = arrays["frame_table"], arrays["topo_table"]
    VR, FR = len(arrays["vert_arena"]), len(arrays["face_arena"])
    out = []
    for b in range(frame_ids.shape[1]):
        e = ftab[_clamp(int(frame_ids[0, b]), 0, len(ftab) - 1)]
        low = int(e[1]) & 0xFFFFFFFF                                         # (the low word as a signed 32-bit integer)
        V = _clamp(low - (1 << 32) if low >= (1 << 31) else low, 0, min(VR, MAX_ELEMS))
        topo = ttab[_clamp(int(e[1]) >> 32, 0, len(ttab) - 1)]
        out.append((V, _clamp(int(topo[1]), 0, min(FR, MAX_ELEMS))))
    return out


def whole(arrays, frame_ids, vcap, fcap, partial_range):
    verts, faces = arrays["vert_arena"], arrays["face_arena"]
    ftab, ttab = arrays["frame_table"], arrays["topo_table"]
    VR, FR = len(verts), len(faces)
    B = frame_ids.shape[1]
    voff, foff = np.zeros(B + 1, np.int32), np.zeros(B + 1, np.int32)
    planes = np.zeros((3, vcap, 3), _F)
    handle = np.zeros(vcap, np.uint8)
    inputs = np.zeros((vcap, 7), _F)
    faces_out = np.zeros((fcap, 3), np.int32)
    pr = _F(partial_range)
    for b, (V, F) in enumerate(counts(arrays, frame_ids)):
        voff[b + 1] = min(int(voff[b]) + V, vcap)
        foff[b + 1] = min(int(foff[b]) + F, fcap)
        entries = [ftab[_clamp(int(frame_ids[c, b]), 0, len(ftab) - 1)] for c in range(3)]
        ec = entries[0]
        rows = int(voff[b + 1]) - int(voff[b])                               # (fewer than V_b where the batch is truncated)
        i = np.arange(rows)
        p = [verts[np.clip(_clamp(int(e[0]), 0, VR - V) + i, 0, VR - 1), :3] for e in entries]
        box = ec[3:6].copy().view(_F)                                        # min x y z, max x y z
        mask = (p[0][:, 1] < box[1] + pr) | (p[0][:, 1] > box[4] - pr) | (p[0][:, 2] < box[2] + pr)
        mf = mask.astype(_F)
        at = slice(int(voff[b]), int(voff[b + 1]))
        for k in range(3):
            planes[k, at] = p[k]
        handle[at] = mask
        inputs[at] = np.concatenate([p[1], p[2] * mf[:, None], mf[:, None]], axis=1)
        topo = ttab[_clamp(int(ec[1]) >> 32, 0, len(ttab) - 1)]
        face_first = _clamp(int(topo[0]), 0, FR - F)
        q = np.arange(int(foff[b + 1]) - int(foff[b]))
        rec = faces[np.clip(face_first + q, 0, FR - 1), :3]
        faces_out[int(foff[b]):int(foff[b + 1])] = np.clip(rec, 0, max(V - 1, 0))
    return {"vert_offsets": voff, "face_offsets": foff, "verts": planes, "handle": handle, "inputs": inputs, "faces": faces_out}
