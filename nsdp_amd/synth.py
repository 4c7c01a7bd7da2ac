"""Procedural (torch-RNG-independent) synthetic inputs and weights for the TDNet hot path.

Everything is derived from a counter hash (splitmix64) evaluated in numpy uint64 arithmetic, so the
same (seed, name) gives bit-identical arrays on every machine and numpy version.  Used by
``bench.py`` (synthetic data, there is no dataset on the GPU box), by ``oracle/make_golden.py`` and
by the tests, which must all regenerate exactly the tensors the golden fixtures were made from.

Input layout follows the reference dataset contract:
``surface_samples_inputs[B,NS,7] = src xyz | mask * tgt xyz | mask``
(/root/reference/dataset/dataset_deform4d_flow.py:217-222), queries ``space_samples_src[B,NQ,3]``,
targets ``space_samples_tgt[B,NQ,3]``.
"""
from __future__ import annotations

import zlib

import numpy as np

_M64 = np.uint64(0xFFFFFFFFFFFFFFFF)


def _splitmix64(x: np.ndarray) -> np.ndarray:
    with np.errstate(over="ignore"):
        x = (x + np.uint64(0x9E3779B97F4A7C15)) & _M64
        z = x
        z = ((z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)) & _M64
        z = ((z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)) & _M64
        return z ^ (z >> np.uint64(31))


def _stream_key(seed: int, name: str) -> np.uint64:
    h = zlib.crc32(name.encode("utf-8")) & 0xFFFFFFFF
    k = np.array([(int(seed) & 0xFFFFFFFF) << 32 | h], dtype=np.uint64)
    return _splitmix64(k)[0]


def uniform01(seed: int, name: str, shape) -> np.ndarray:
    """float64 uniforms in [0,1) with 53 random bits, deterministic in (seed, name, flat index)."""
    n = int(np.prod(shape)) if len(tuple(shape)) else 1
    key = _stream_key(seed, name)
    with np.errstate(over="ignore"):
        ctr = (np.arange(n, dtype=np.uint64) * np.uint64(0xD1342543DE82EF95) + key) & _M64
    bits = _splitmix64(ctr) >> np.uint64(11)
    return (bits.astype(np.float64) * (1.0 / 9007199254740992.0)).reshape(shape)


def uniform(seed: int, name: str, shape, lo: float, hi: float) -> np.ndarray:
    return (lo + (hi - lo) * uniform01(seed, name, shape)).astype(np.float32)


def normal(seed: int, name: str, shape) -> np.ndarray:
    """Box-Muller on two independent uniform streams (float32 result)."""
    u1 = uniform01(seed, name + "#u1", shape)
    u2 = uniform01(seed, name + "#u2", shape)
    r = np.sqrt(-2.0 * np.log(1.0 - u1))
    return (r * np.cos(2.0 * np.pi * u2)).astype(np.float32)


def make_batch(seed: int, batch: int, n_surf: int, n_query: int, handle_ratio: float = 0.3):
    """Synthetic batch in the reference's data_dict layout (numpy float32 arrays).

    surf xyz ~ U[-0.5,0.5)^3 (GAPS-normalised meshes live roughly in that cube,
    /root/reference/preprocess/others/process_mesh_local.sh:62-63); handle mask m = (u < ratio);
    inputs = [xyz, m*(xyz + 0.05 n1), m]; queries ~ U[-0.5,0.5)^3; targets = q + 0.01 n2.
    """
    xyz = uniform(seed, "surf_xyz", (batch, n_surf, 3), -0.5, 0.5)
    mask = (uniform01(seed, "handle_mask", (batch, n_surf, 1)) < handle_ratio).astype(np.float32)
    tgt = (xyz + 0.05 * normal(seed, "surf_disp", (batch, n_surf, 3))).astype(np.float32)
    inputs = np.concatenate([xyz, (mask * tgt).astype(np.float32), mask], axis=-1)
    q = uniform(seed, "space_src", (batch, n_query, 3), -0.5, 0.5)
    t = (q + 0.01 * normal(seed, "space_disp", (batch, n_query, 3))).astype(np.float32)
    return {
        "surface_samples_inputs": np.ascontiguousarray(inputs, dtype=np.float32),
        "space_samples_src": q,
        "space_samples_tgt": t,
    }


def procedural_state_dict(template: dict, seed: int) -> dict:
    """Deterministic values for every entry of a ``state_dict`` (keys + shapes from ``template``).

    Every weight is randomised -- including ``ResnetBlockFC.fc_1.weight`` that the reference
    zero-initialises (/root/reference/model/decoder/blocks.py:131) and the BatchNorm running
    statistics -- so that no gradient or eval-mode path is trivially zero.
    Returns numpy arrays (int64 scalar for ``num_batches_tracked``).
    """
    out = {}
    for key, ref in template.items():
        shape = tuple(ref.shape)
        leaf = key.rsplit(".", 1)[-1]
        if leaf == "num_batches_tracked":
            out[key] = np.zeros(shape, dtype=np.int64)
        elif leaf == "running_mean":
            out[key] = uniform(seed, key, shape, -0.1, 0.1)
        elif leaf == "running_var":
            out[key] = uniform(seed, key, shape, 0.5, 1.5)
        elif leaf == "weight" and len(shape) == 1:  # BatchNorm gamma
            out[key] = uniform(seed, key, shape, 0.5, 1.5)
        elif leaf == "bias":
            out[key] = uniform(seed, key, shape, -0.1, 0.1)
        elif leaf == "weight":
            fan_in = int(np.prod(shape[1:]))
            bound = float(np.sqrt(1.0 / max(fan_in, 1)))  # PyTorch-default-like scale: outputs O(1)
            out[key] = uniform(seed, key, shape, -bound, bound)
        else:
            raise KeyError(f"unhandled state_dict entry {key} {shape}")
    return out


def _per_identity(value, identities, what):
    if isinstance(value, dict):
        return {k: int(value[k]) for k in identities}
    if isinstance(value, (list, tuple)):
        if len(value) != len(identities):
            raise ValueError(f"write_dataset_tree: {what} has {len(value)} entries for {len(identities)} identities")
        return {k: int(v) for k, v in zip(identities, value)}
    return {k: int(value) for k in identities}


def dataset_tree_frame(seed: int, identity: str, motion: str, frame: int, frames: int, n_surface: int, n_space: int):
    """The procedural arrays of one frame (float32): surface points, surface normals, space points.  Row i of every frame of an
    identity is the same material point (the reference's files are correspondences); frame 0 of every motion is the identity's
    canonical pose, later frames add a smooth, motion-specific displacement that grows with the frame number."""
    t = frame / max(frames - 1, 1)
    w = uniform(seed, f"{motion}/wave", (3, 3), -1.0, 1.0).astype(np.float64)
    amp = uniform(seed, f"{motion}/amp", (3,), 0.03, 0.08).astype(np.float64)

    def move(p):
        return p + t * amp[None, :] * np.sin(2.0 * np.pi * (p @ w.T) + 0.5)

    surf = uniform(seed, f"{identity}/surface", (n_surface, 3), -0.5, 0.5).astype(np.float64)
    nrm = normal(seed, f"{identity}/normals", (n_surface, 3)).astype(np.float64)
    nrm = nrm + 0.3 * t * np.cos(2.0 * np.pi * (surf @ w.T))
    nrm /= np.maximum(np.linalg.norm(nrm, axis=1, keepdims=True), 1e-6)
    space = uniform(seed, f"{identity}/space", (n_space, 3), -0.5, 0.5).astype(np.float64)
    return move(surf).astype(np.float32), nrm.astype(np.float32), move(space).astype(np.float32)


def write_dataset_tree(root, identities, motions, frames, n_surface, n_space, dtype=np.float16, data_type="deform4d", seed=0,
                       held_out_motions=1, surface_flow_file="surface_points.npz", space_flow_file="flow.npz",
                       norm_params_file="orig_to_gaps.txt"):
    """Write a procedural data set in the reference's directory layout (dataset/dataset_deform4d_flow.py:37-172) and return the
    ``data`` section of a config that reads it:

        root/dataset/<sequence>/<frame %04d>/{surface_flow_file (points, normals), space_flow_file (points), norm_params_file}
        root/splits/<data_type>/{identity_seen, train_seen, test_unseen_motions}.lst

    ``identities`` / ``motions``: names (without '_' or '-').  A sequence is ``identity_motion`` for ``deform4d`` and
    ``identity-motion`` for ``deformtransfer`` (whose source frame depends on the animal in the name: 0003 for cat and lion, 0005
    for horse, else 0001).  ``n_surface`` / ``n_space``: one count, or one per identity (list or dict).  ``dtype``: the files'
    (numpy float16 or float32; a dict per identity is accepted too).  ``identity_seen`` lists the first motion's sequence of every
    identity (its frame 0000 is the canonical pose), ``train_seen`` every sequence but those of the last ``held_out_motions``
    motions, ``test_unseen_motions`` the rest (all of them when nothing is left).  norm_params_file holds the identity matrix."""
    import os
    identities, motions = [str(i) for i in identities], [str(m) for m in motions]
    sep = {"deform4d": "_", "deformtransfer": "-"}.get(data_type)
    if sep is None:
        raise ValueError(f"write_dataset_tree: data_type '{data_type}' is neither 'deform4d' nor 'deformtransfer'")
    for name in identities + motions:
        if "_" in name or "-" in name or not name:
            raise ValueError(f"write_dataset_tree: the name '{name}' must be non-empty and free of '_' and '-'")
    ns, nq = _per_identity(n_surface, identities, "n_surface"), _per_identity(n_space, identities, "n_space")
    dts = dtype if isinstance(dtype, dict) else {k: dtype for k in identities}
    dataset_dir, split_dir = os.path.join(root, "dataset"), os.path.join(root, "splits")
    for iden in identities:
        dt = np.dtype(dts[iden])
        if dt not in (np.dtype(np.float16), np.dtype(np.float32)):
            raise ValueError(f"write_dataset_tree: dtype {dt} is neither float16 nor float32")
        for motion in motions:
            for f in range(int(frames)):
                d = os.path.join(dataset_dir, iden + sep + motion, "%04d" % f)
                os.makedirs(d, exist_ok=True)
                surf, nrm, space = dataset_tree_frame(seed, iden, motion, f, int(frames), ns[iden], nq[iden])
                np.savez(os.path.join(d, surface_flow_file), points=surf.astype(dt), normals=nrm.astype(dt))
                np.savez(os.path.join(d, space_flow_file), points=space.astype(dt))
                np.savetxt(os.path.join(d, norm_params_file), np.eye(4))
    os.makedirs(os.path.join(split_dir, data_type), exist_ok=True)
    held = motions[len(motions) - int(held_out_motions):] if 0 < int(held_out_motions) < len(motions) else []
    lists = {"identity_seen": [i + sep + motions[0] for i in identities],
             "train_seen": [i + sep + m for i in identities for m in motions if m not in held],
             "test_unseen_motions": [i + sep + m for i in identities for m in (held or motions)]}
    for name, seqs in lists.items():
        with open(os.path.join(split_dir, data_type, name + ".lst"), "w") as f:
            f.write("\n".join(seqs) + "\n")
    return {"type": data_type, "dataset_dir": dataset_dir, "split_dir": split_dir, "interval": 1, "arbitrary": False,
            "inverse": False, "fix_coord_system": False, "num_surf_samples": min(ns.values()), "num_space_samples": min(nq.values()),
            "partial_range": 0.1, "noise_level": 0.0, "partial_shape_ratio": 1.0, "norm_params_file": norm_params_file,
            "surface_flow_file": surface_flow_file, "space_flow_file": space_flow_file}


# ---------------------------------------------------------------------------------------------------------------- mesh trees
def sphere_mesh(rings: int, segments: int, radius: float = 0.4):
    """A closed latitude-longitude sphere: (verts float64 (rings * segments + 2, 3), faces int32 (2 * rings * segments, 3)), the
    y axis through the poles.  rings = 100, segments = 200: 20 002 vertices and 40 000 faces."""
    theta = np.pi * (np.arange(rings) + 1) / (rings + 1)
    phi = 2.0 * np.pi * np.arange(segments) / segments
    ring = np.stack([np.outer(np.sin(theta), np.cos(phi)), np.outer(np.cos(theta), np.ones(segments)),
                     np.outer(np.sin(theta), np.sin(phi))], axis=2).reshape(-1, 3)
    verts = radius * np.concatenate([ring, [[0.0, 1.0, 0.0], [0.0, -1.0, 0.0]]])
    north, south = rings * segments, rings * segments + 1
    i, j = np.meshgrid(np.arange(rings - 1), np.arange(segments), indexing="ij")
    a, b = i * segments + j, i * segments + (j + 1) % segments
    quads = np.concatenate([np.stack([a, a + segments, b], axis=2), np.stack([b, a + segments, b + segments], axis=2)]).reshape(-1, 3)
    j = np.arange(segments)
    caps = np.concatenate([np.stack([np.full(segments, north), j, (j + 1) % segments], axis=1),
                           np.stack([np.full(segments, south), (rings - 1) * segments + (j + 1) % segments,
                                     (rings - 1) * segments + j], axis=1)])
    return verts, np.concatenate([quads, caps])[:, [0, 2, 1]].astype(np.int32)           # (outward normals)


def mesh_tree_vertices(seed: int, verts: np.ndarray, motion: str, frame: int, frames: int) -> np.ndarray:
    """The vertices (float64) of one frame of a procedural mesh sequence: frame 0 of every motion is the mesh as given (the
    canonical pose), later frames add ``dataset_tree_frame``'s smooth, motion-specific displacement."""
    t = frame / max(frames - 1, 1)
    w = uniform(seed, f"{motion}/wave", (3, 3), -1.0, 1.0).astype(np.float64)
    amp = uniform(seed, f"{motion}/amp", (3,), 0.03, 0.08).astype(np.float64)
    p = np.asarray(verts, dtype=np.float64)
    return p + t * amp[None, :] * np.sin(2.0 * np.pi * (p @ w.T) + 0.5)


def write_mesh_dataset_tree(root, meshes: dict, motions, frames, mesh_file="mesh_norm.ply", data_type="deform4d", seed=0,
                            held_out_motions=1, norm_params_file="orig_to_gaps.txt", orig2world=None):
    """``write_dataset_tree``'s directory layout and split lists with one MESH per frame instead of the sample files:

        root/dataset/<sequence>/<frame %04d>/{mesh_file, norm_params_file}

    ``meshes``: identity -> (verts (V, 3), faces (F, 3)), the canonical pose; the frames are ``mesh_tree_vertices``'.  The files
    hold fp32 vertices; ``orig2world`` (4, 4; default the identity) is written as norm_params_file and the vertices are stored
    in ORIGINAL coordinates (world = orig2world applied to them) unless "norm" is in ``mesh_file``.  Returns the ``data``
    section of a config that reads the tree through nsdp_amd.meshstore."""
    import os
    from .meshio import write_mesh
    identities, motions = [str(i) for i in meshes], [str(m) for m in motions]
    sep = {"deform4d": "_", "deformtransfer": "-"}.get(data_type)
    if sep is None:
        raise ValueError(f"write_mesh_dataset_tree: data_type '{data_type}' is neither 'deform4d' nor 'deformtransfer'")
    for name in identities + motions:
        if "_" in name or "-" in name or not name:
            raise ValueError(f"write_mesh_dataset_tree: the name '{name}' must be non-empty and free of '_' and '-'")
    o2w = np.eye(4) if orig2world is None else np.asarray(orig2world, dtype=np.float64).reshape(4, 4)
    w2o = np.linalg.inv(o2w)
    dataset_dir, split_dir = os.path.join(root, "dataset"), os.path.join(root, "splits")
    for iden in identities:
        verts, faces = meshes[iden]
        for motion in motions:
            for f in range(int(frames)):
                d = os.path.join(dataset_dir, iden + sep + motion, "%04d" % f)
                os.makedirs(d, exist_ok=True)
                v = mesh_tree_vertices(seed, verts, motion, f, int(frames))
                if "norm" not in mesh_file:
                    v = (w2o[:3, :3] @ v.T + w2o[:3, 3:4]).T
                write_mesh(os.path.join(d, mesh_file), v.astype(np.float32), faces)
                np.savetxt(os.path.join(d, norm_params_file), o2w)
    os.makedirs(os.path.join(split_dir, data_type), exist_ok=True)
    held = motions[len(motions) - int(held_out_motions):] if 0 < int(held_out_motions) < len(motions) else []
    lists = {"identity_seen": [i + sep + motions[0] for i in identities],
             "train_seen": [i + sep + m for i in identities for m in motions if m not in held],
             "test_unseen_motions": [i + sep + m for i in identities for m in (held or motions)]}
    for name, seqs in lists.items():
        with open(os.path.join(split_dir, data_type, name + ".lst"), "w") as f:
            f.write("\n".join(seqs) + "\n")
    return {"type": data_type, "dataset_dir": dataset_dir, "split_dir": split_dir, "interval": 1, "arbitrary": False,
            "inverse": False, "fix_coord_system": False, "num_surf_samples": 256, "num_space_samples": 128,
            "partial_range": 0.1, "noise_level": 0.0, "partial_shape_ratio": 1.0, "norm_params_file": norm_params_file,
            "mesh_file": mesh_file, "space_sigma": [0.1, 0.02]}


def write_handle_mesh_tree(root, meshes: dict, data_type="tosca", mesh_file="mesh_norm.ply", split="test", userhandle=None,
                           norm_params_file="orig_to_gaps.txt"):
    """A procedural user-handle data set (dataset/dataset_userhandle_flow.py: ``tosca`` / ``dogrec``) -- single meshes to drag:

        root/dataset/<name>/0000/{mesh_file, norm_params_file}        root/splits/<data_type>/<split>.lst

    ``meshes``: name -> (verts (V, 3), faces (F, 3)); the files hold fp32 vertices and the identity as norm_params_file.
    ``userhandle``: the drag's settings (default: the head by (-0.15, -0.2, -0.2), the reference's config/tosca/head.yaml).
    Returns the ``data`` section of a config that reads the tree through ``meshstore.HandleMeshStore``."""
    import os
    from .meshio import write_mesh
    if data_type not in ("tosca", "dogrec"):
        raise ValueError(f"write_handle_mesh_tree: data_type '{data_type}' is neither 'tosca' nor 'dogrec'")
    dataset_dir, split_dir = os.path.join(root, "dataset"), os.path.join(root, "splits")
    for name, (verts, faces) in meshes.items():
        d = os.path.join(dataset_dir, str(name), "0000")
        os.makedirs(d, exist_ok=True)
        write_mesh(os.path.join(d, mesh_file), np.asarray(verts).astype(np.float32), faces)
        np.savetxt(os.path.join(d, norm_params_file), np.eye(4))
    os.makedirs(os.path.join(split_dir, data_type), exist_ok=True)
    with open(os.path.join(split_dir, data_type, split + ".lst"), "w") as f:
        f.write("\n".join(str(n) for n in meshes) + "\n")
    handle = {"head": True, "tail": False, "frontleftfoot": False, "frontrightfoot": False, "behindleftfoot": False,
              "behindrightfoot": False, "cliptail": False, "xtrans": -0.15, "ytrans": -0.2, "ztrans": -0.2}
    handle.update(userhandle or {})
    return {"type": data_type, "dataset_dir": dataset_dir, "split_dir": split_dir, "interval": 1, "arbitrary": True, "inverse": False,
            "fix_coord_system": False, "num_surf_samples": 0, "num_space_samples": 0, "partial_range": 0.1, "noise_level": 0.0,
            "partial_shape_ratio": 1.0, "norm_params_file": norm_params_file, "mesh_file": mesh_file, "userhandle": handle}
