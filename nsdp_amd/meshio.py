"""Triangle meshes on disk: a reader of .obj, .ply and .off files and a small writer, on the host, with numpy alone (``trimesh``,
which the reference reads its meshes with, is not a dependency).

``read_mesh(path)`` -> (verts float64 (V, 3), faces int32 (F, 3)).  A file is read once and converted in bulk (the numbers of a
file go through ONE numpy conversion, no ``float()`` per line: a data set is thousands of frames, read at load time under
``cpu_budget``).  Polygons with more than three corners are fan-triangulated from their first corner.

  .obj   ``v x y z`` (further columns, such as colours, are ignored, statement by statement); ``f`` corners in the forms ``a``,
         ``a/b``, ``a/b/c`` and ``a//c``; negative indices count back from the vertices read so far; a trailing backslash
         continues a statement on the next line.  Every other statement is skipped.
  .ply   ``ascii`` and ``binary_little_endian``; a ``vertex`` element whose x, y, z sit among other scalar properties of any
         type; a ``face`` element with one list property of any integer count and index type; further elements of scalar
         properties are skipped, and whatever follows the vertices and the faces (edge or strip lists included) is not read.
         An element with a list property IN FRONT of them is refused (its length cannot be skipped without a walk), as is
         ``binary_big_endian``, by name.
  .off   with the counts on the line after ``OFF`` or on the same line; ``#`` comments.

``MeshError`` (a ValueError) names the file and the reason: a vertex index outside [0, V), a face of fewer than three corners,
no vertices or no faces, an unknown extension, a file that ends early.

``write_mesh(path, verts, faces, colors=None, normals=None)``: .obj (text, 1-based) and binary little-endian .ply (float32
vertices as ``float``, others as ``double``; int32 faces), with per-vertex uint8 RGB where given -- so that a round trip can be
tested and predictions written.  Per-vertex ``normals`` (V, 3) become ``nx ny nz`` properties behind ``x y z`` in the vertex
type (.ply) and ``vn`` statements with ``f a//a b//b c//c`` corners (.obj); ``read_mesh`` reads such a file back to the same
vertices and faces (it skips further properties and what follows a corner's slash).
"""
from __future__ import annotations

import os
import re

import numpy as np


class MeshError(ValueError):
    pass


_PLY_TYPES = {"char": "i1", "int8": "i1", "uchar": "u1", "uint8": "u1", "short": "i2", "int16": "i2", "ushort": "u2", "uint16": "u2",
              "int": "i4", "int32": "i4", "uint": "u4", "uint32": "u4", "float": "f4", "float32": "f4", "double": "f8", "float64": "f8"}


def _numbers(text, dtype, path, what):
    """Every whitespace-separated number of ``text`` in one conversion."""
    try:
        return np.array(text.split(), dtype=dtype)
    except ValueError as e:
        raise MeshError(f"read_mesh: {path}: {what} hold something that is not a number ({e})") from None


def _fan(path, flat, counts):
    """Polygons (``counts[i]`` corners each, concatenated in ``flat``) -> triangles (T, 3), fanned from the first corner."""
    counts = np.asarray(counts, dtype=np.int64)
    if counts.size and int(counts.min()) < 3:
        bad = int(np.nonzero(counts < 3)[0][0])
        raise MeshError(f"read_mesh: {path}: face {bad} has {int(counts[bad])} corners, fewer than three")
    if int(counts.sum()) != flat.shape[0]:
        raise MeshError(f"read_mesh: {path}: the face list holds {flat.shape[0]} corners where its counts announce {int(counts.sum())}")
    if counts.size and int(counts.max()) == 3:
        return flat.reshape(-1, 3)
    start = np.cumsum(counts) - counts
    tris = counts - 2
    poly = np.repeat(np.arange(counts.size), tris)
    k = np.arange(int(tris.sum())) - np.repeat(np.cumsum(tris) - tris, tris) + 1
    s = start[poly]
    return np.stack([flat[s], flat[s + k], flat[s + k + 1]], axis=1)


def _finish(path, verts, faces):
    verts = np.ascontiguousarray(verts, dtype=np.float64).reshape(-1, 3)
    faces = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    if verts.shape[0] == 0:
        raise MeshError(f"read_mesh: {path} has no vertices")
    if faces.shape[0] == 0:
        raise MeshError(f"read_mesh: {path} has no faces")
    if int(faces.min()) < 0 or int(faces.max()) >= verts.shape[0]:
        bad = int(np.nonzero(((faces < 0) | (faces >= verts.shape[0])).any(axis=1))[0][0])
        raise MeshError(f"read_mesh: {path}: triangle {bad} holds a vertex index outside [0, {verts.shape[0]}): {faces[bad].tolist()}")
    return verts, np.ascontiguousarray(faces, dtype=np.int32)


def _stream_faces(path, tok, pos, n_faces):
    """``n_faces`` records ``k i_0 .. i_(k-1)`` from the number stream ``tok`` at ``pos`` -> (flat corners, counts, next pos)."""
    if n_faces == 0:
        return np.zeros(0, np.int64), np.zeros(0, np.int64), pos
    if pos >= tok.shape[0]:
        raise MeshError(f"read_mesh: {path} ends before its face list")
    k = int(tok[pos])
    end = pos + n_faces * (k + 1)
    if k >= 0 and end <= tok.shape[0]:
        block = tok[pos:end].reshape(n_faces, k + 1)
        if np.all(block[:, 0] == k):                                        # one polygon size throughout: no walk
            return block[:, 1:].reshape(-1).astype(np.int64), np.full(n_faces, k, np.int64), end
    counts = np.empty(n_faces, np.int64)
    starts = np.empty(n_faces, np.int64)
    for i in range(n_faces):                                                 # mixed polygons: a walk over the counts
        if pos >= tok.shape[0]:
            raise MeshError(f"read_mesh: {path} ends inside its face list (face {i} of {n_faces})")
        counts[i], starts[i] = tok[pos], pos + 1
        pos += 1 + max(int(tok[pos]), 0)
    if pos > tok.shape[0]:
        raise MeshError(f"read_mesh: {path} ends inside its face list")
    good = np.maximum(counts, 0)
    take = np.repeat(starts, good) + (np.arange(int(good.sum())) - np.repeat(np.cumsum(good) - good, good))
    return tok[take].astype(np.int64), counts, pos


# ---------------------------------------------------------------------------------------------------------------- .obj
_AFTER_SLASH = re.compile(r"/\S*")


def _read_obj(path):
    with open(path, "r", errors="replace") as f:
        lines = [l.strip() for l in f.read().replace("\\\n", " ").splitlines()]      # (a trailing backslash continues a statement)
    v_at = [i for i, l in enumerate(lines) if l[:2] in ("v ", "v\t")]
    f_at = [i for i, l in enumerate(lines) if l[:2] in ("f ", "f\t")]
    cols = [lines[i][2:] for i in v_at]
    widths = {len(c.split()) for c in cols}                                  # (counted per statement: a total that merely divides is no proof)
    if widths and min(widths) < 3:
        raise MeshError(f"read_mesh: {path}: a v statement has fewer than three coordinates")
    if len(widths) == 1:
        verts = _numbers(" ".join(cols), np.float64, path, "its v statements").reshape(len(v_at), -1)[:, :3]
    else:                                                                    # statements of different lengths: the first three of each
        verts = _numbers(" ".join(" ".join(c.split()[:3]) for c in cols), np.float64, path, "its v statements").reshape(-1, 3)
    corners = [_AFTER_SLASH.sub("", lines[i][2:]) for i in f_at]             # a/b/c, a//c, a/b -> a
    counts = np.array([len(c.split()) for c in corners], dtype=np.int64)
    flat = _numbers(" ".join(corners), np.int64, path, "its f statements")
    # a negative index counts back from the vertices read BEFORE its statement; 0 is no index
    before = np.searchsorted(np.asarray(v_at, dtype=np.int64), np.asarray(f_at, dtype=np.int64))
    if int(counts.sum()) == flat.shape[0]:
        seen = np.repeat(before, counts)
        flat = np.where(flat < 0, seen + flat, np.where(flat > 0, flat - 1, -1))
    return _finish(path, verts, _fan(path, flat, counts))


# ---------------------------------------------------------------------------------------------------------------- .ply
def _ply_header(path, raw):
    end = raw.find(b"end_header")
    if raw[:3] != b"ply" or end < 0:
        raise MeshError(f"read_mesh: {path} is not a ply file (no 'ply' ... 'end_header')")
    body = raw.find(b"\n", end) + 1
    fmt, elements = None, []
    for line in raw[:end].decode("ascii", "replace").splitlines()[1:]:
        w = line.split()
        if not w or w[0] in ("comment", "obj_info"):
            continue
        if w[0] == "format":
            fmt = w[1]
        elif w[0] == "element":
            elements.append({"name": w[1], "count": int(w[2]), "props": []})
        elif w[0] == "property" and elements:
            if w[1] == "list":
                elements[-1]["props"].append((w[4], "list", w[2], w[3]))
            else:
                elements[-1]["props"].append((w[2], w[1]))
    if fmt == "binary_big_endian":
        raise MeshError(f"read_mesh: {path} is a binary_big_endian ply file; ascii and binary_little_endian are read")
    if fmt not in ("ascii", "binary_little_endian"):
        raise MeshError(f"read_mesh: {path} has the unknown ply format '{fmt}'")
    for el in elements:
        for p in el["props"]:
            for t in p[2:] if p[1] == "list" else p[1:2]:
                if t not in _PLY_TYPES:
                    raise MeshError(f"read_mesh: {path}: unknown ply property type '{t}'")
    return fmt, elements, body


def _read_ply(path):
    with open(path, "rb") as f:
        raw = f.read()
    fmt, elements, pos = _ply_header(path, raw)
    verts, flat, counts = None, None, None
    tok = _numbers(raw[pos:].decode("ascii", "replace"), np.float64, path, "its body") if fmt == "ascii" else None
    pos = 0 if fmt == "ascii" else pos
    for el in elements:
        if verts is not None and flat is not None:
            break                                                            # (what follows the vertices and the faces is not read)
        name, count, props = el["name"], el["count"], el["props"]
        lists = [p for p in props if p[1] == "list"]
        if name == "face":
            if len(props) != 1 or not lists:
                raise MeshError(f"read_mesh: {path}: the face element must have exactly one list property, it has {[p[0] for p in props]}")
            ct, it = np.dtype("<" + _PLY_TYPES[lists[0][2]]), np.dtype("<" + _PLY_TYPES[lists[0][3]])
            if ct.kind == "f" or it.kind == "f":
                raise MeshError(f"read_mesh: {path}: the face list's count and index types must be integers")
            if fmt == "ascii":
                flat, counts, pos = _stream_faces(path, tok, pos, count)
            else:
                flat, counts, pos = _binary_faces(path, raw, pos, count, ct, it)
            continue
        if lists:
            raise MeshError(f"read_mesh: {path}: element '{name}' in front of the vertices or faces has a list property; such an "
                            f"element is read past only when it follows both")
        if fmt == "ascii":
            end = pos + count * len(props)
            if end > tok.shape[0]:
                raise MeshError(f"read_mesh: {path} ends inside element '{name}'")
            block, pos = tok[pos:end].reshape(count, len(props)), end
            if name == "vertex":
                verts = _xyz(path, props, lambda k: block[:, k])
        else:
            dt = np.dtype([(f"p{k}", "<" + _PLY_TYPES[p[1]]) for k, p in enumerate(props)])
            end = pos + count * dt.itemsize
            if end > len(raw):
                raise MeshError(f"read_mesh: {path} ends inside element '{name}'")
            block, pos = np.frombuffer(raw, dtype=dt, count=count, offset=pos), end
            if name == "vertex":
                verts = _xyz(path, props, lambda k: block[f"p{k}"])
    if verts is None:
        raise MeshError(f"read_mesh: {path} has no vertices")
    if flat is None:
        raise MeshError(f"read_mesh: {path} has no faces")
    return _finish(path, verts, _fan(path, flat, counts))


def _xyz(path, props, column):
    names = [p[0] for p in props]
    if any(a not in names for a in "xyz"):
        raise MeshError(f"read_mesh: {path}: the vertex element has no x, y, z properties (it has {names})")
    return np.stack([np.asarray(column(names.index(a)), dtype=np.float64) for a in "xyz"], axis=1)


def _binary_faces(path, raw, pos, n_faces, ct, it):
    if n_faces == 0:
        return np.zeros(0, np.int64), np.zeros(0, np.int64), pos
    if pos + ct.itemsize > len(raw):
        raise MeshError(f"read_mesh: {path} ends before its face list")
    k = int(np.frombuffer(raw, dtype=ct, count=1, offset=pos)[0])
    if k >= 0:
        rec = np.dtype([("n", ct), ("i", it, (k,))])
        if pos + n_faces * rec.itemsize <= len(raw):
            block = np.frombuffer(raw, dtype=rec, count=n_faces, offset=pos)
            if np.all(block["n"] == k):                                     # one polygon size throughout: no walk
                return block["i"].reshape(-1).astype(np.int64), np.full(n_faces, k, np.int64), pos + n_faces * rec.itemsize
    counts, parts = np.empty(n_faces, np.int64), []
    for i in range(n_faces):                                                 # mixed polygons: a walk over the counts
        if pos + ct.itemsize > len(raw):
            raise MeshError(f"read_mesh: {path} ends inside its face list (face {i} of {n_faces})")
        k = max(int(np.frombuffer(raw, dtype=ct, count=1, offset=pos)[0]), 0)
        counts[i] = k
        pos += ct.itemsize
        if pos + k * it.itemsize > len(raw):
            raise MeshError(f"read_mesh: {path} ends inside its face list (face {i} of {n_faces})")
        parts.append(np.frombuffer(raw, dtype=it, count=k, offset=pos))
        pos += k * it.itemsize
    return np.concatenate(parts).astype(np.int64), counts, pos


# ---------------------------------------------------------------------------------------------------------------- .off
def _read_off(path):
    with open(path, "r", errors="replace") as f:
        text = re.sub(r"#[^\n]*", "", f.read())
    text = text.lstrip()
    if text[:3] != "OFF":
        raise MeshError(f"read_mesh: {path} does not start with OFF")
    tok = _numbers(text[3:], np.float64, path, "its body")                   # (the counts may share the header's line)
    if tok.shape[0] < 3:
        raise MeshError(f"read_mesh: {path} ends before its counts")
    nv, nf = int(tok[0]), int(tok[1])
    if nv < 0 or nf < 0 or 3 + 3 * nv > tok.shape[0]:
        raise MeshError(f"read_mesh: {path} ends inside its {nv} vertices")
    verts = tok[3:3 + 3 * nv].reshape(nv, 3)
    flat, counts, _ = _stream_faces(path, tok, 3 + 3 * nv, nf)
    return _finish(path, verts, _fan(path, flat, counts))


_READERS = {".obj": _read_obj, ".ply": _read_ply, ".off": _read_off}


def read_mesh(path):
    """(verts float64 (V, 3), faces int32 (F, 3)) of an .obj, .ply or .off file; see the module docstring."""
    path = os.fspath(path)
    ext = os.path.splitext(path)[1].lower()
    if ext not in _READERS:
        raise MeshError(f"read_mesh: {path} has the unknown extension '{ext}' (.obj, .ply and .off are read)")
    if not os.path.isfile(path):
        raise MeshError(f"read_mesh: missing file {path}")
    return _READERS[ext](path)


# ---------------------------------------------------------------------------------------------------------------- writer
def write_mesh(path, verts, faces, colors=None, normals=None):
    """Write (verts (V, 3) float, faces (F, 3) int[, colors (V, 3) uint8][, normals (V, 3) float]) as .obj or binary
    little-endian .ply."""
    path = os.fspath(path)
    ext = os.path.splitext(path)[1].lower()
    verts = np.asarray(verts)
    if verts.dtype not in (np.dtype(np.float32), np.dtype(np.float64)):
        verts = verts.astype(np.float64)
    faces = np.asarray(faces)
    if verts.ndim != 2 or verts.shape[1] != 3 or faces.ndim != 2 or faces.shape[1] != 3:
        raise MeshError(f"write_mesh: {path}: verts must be (V, 3) and faces (F, 3), got {verts.shape} and {faces.shape}")
    if colors is not None:
        colors = np.asarray(colors)
        if colors.shape != verts.shape or colors.dtype != np.uint8:
            raise MeshError(f"write_mesh: {path}: colors must be uint8 {verts.shape}, got {colors.dtype} {colors.shape}")
    if normals is not None:
        normals = np.asarray(normals)
        if normals.shape != verts.shape or normals.dtype.kind != "f":
            raise MeshError(f"write_mesh: {path}: normals must be float {verts.shape}, got {normals.dtype} {normals.shape}")
        normals = normals.astype(verts.dtype)                                # (the vertex type)
    if ext == ".obj":
        digits = "%.9g" if verts.dtype == np.float32 else "%.17g"            # (enough to read the same binary number back)
        with open(path, "w") as f:
            if colors is None:
                np.savetxt(f, verts, fmt="v " + " ".join([digits] * 3))
            else:
                np.savetxt(f, np.concatenate([verts.astype(np.float64), colors / 255.0], axis=1), fmt="v " + " ".join([digits] * 3 + ["%.6g"] * 3))
            if normals is None:
                np.savetxt(f, faces.astype(np.int64) + 1, fmt="f %d %d %d")
            else:
                np.savetxt(f, normals, fmt="vn " + " ".join([digits] * 3))
                np.savetxt(f, np.repeat(faces.astype(np.int64) + 1, 2, axis=1), fmt="f %d//%d %d//%d %d//%d")
    elif ext == ".ply":
        real = "float" if verts.dtype == np.float32 else "double"
        fields = [(a, "<" + _PLY_TYPES[real]) for a in "xyz"] + ([(a, "<" + _PLY_TYPES[real]) for a in ("nx", "ny", "nz")] if normals is not None else [])
        fields += ([(c, "u1") for c in ("red", "green", "blue")] if colors is not None else [])
        vrec = np.empty(verts.shape[0], dtype=np.dtype(fields))
        for k, a in enumerate("xyz"):
            vrec[a] = verts[:, k]
        if normals is not None:
            for k, a in enumerate(("nx", "ny", "nz")):
                vrec[a] = normals[:, k]
        if colors is not None:
            for k, c in enumerate(("red", "green", "blue")):
                vrec[c] = colors[:, k]
        frec = np.empty(faces.shape[0], dtype=np.dtype([("n", "u1"), ("i", "<i4", (3,))]))
        frec["n"], frec["i"] = 3, faces
        header = ["ply", "format binary_little_endian 1.0", f"element vertex {verts.shape[0]}"]
        header += [f"property {real} {a}" for a in "xyz"]
        header += [f"property {real} {a}" for a in ("nx", "ny", "nz")] if normals is not None else []
        header += [f"property uchar {c}" for c in ("red", "green", "blue")] if colors is not None else []
        header += [f"element face {faces.shape[0]}", "property list uchar int vertex_indices", "end_header"]
        with open(path, "wb") as f:
            f.write(("\n".join(header) + "\n").encode("ascii"))
            f.write(vrec.tobytes())
            f.write(frec.tobytes())
    else:
        raise MeshError(f"write_mesh: {path} has the unknown extension '{ext}' (.obj and .ply are written)")
