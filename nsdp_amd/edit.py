"""Editing session: drag handles on a mesh without re-encoding its source.

    python -m nsdp_amd.edit CONFIG [--vertices N] [--surface N] [--batch B] [--part P --translate dx,dy,dz] [--drags K]
                                   [--graph] [--normals] [--self-intersections] [--render OUT.png [--render-size S]]
                                   [--weight_file F] [--out DIR]
    python -m nsdp_amd.edit CONFIG --vertex-counts n1,n2,... [--surface-counts s1,s2,... | --surface N] [--graph] ...

The reference's interactive editing (run.py, "Interactive Editing / Run-batch-processing"; config/tosca/*.yaml,
config/dogrec/*.yaml; dataset/dataset_userhandle_flow.py) takes one mesh, marks head, tail and feet as handles by a bounding-box
rule (dataset/utils.py: cano_handle_user_define), translates one of them and lets FlowArbitrary deform every vertex -- one whole
``test_on_batch_with_arbitrary`` per drag.  Most of that call does not depend on the drag:

  * network 1 (model_canonicalize) reads the source pose alone: its encoder and its decodes of the cloud and of the vertices;
  * network 2's geometry -- farthest-point sampling, every k-NN set of the pyramid, the final blocks' neighbours, each query's
    nearest anchors -- derives from columns 0:3 of its input, the canonicalised cloud.  A drag changes columns 3:7 only;
  * when the cloud IS the vertex set (the reference's user-handle data set), the second decode repeats the first: the decoder
    treats query rows independently.

An ``EditSession`` computes those once per source mesh and runs, per drag, the handle kernel (include/nsdp_handles.h),
network 2's encoder over cached index sets and one decode (two when the cloud is a separate set):

    s = EditSession(model, verts_src)                    # FlowArbitrary in eval mode, verts_src [B, V, 3] on the GPU
    out = s.drag(part="head", translation=(-0.15, -0.2, -0.2))
    out = s.drag(handle_mask=h, move_mask=m, translation=(0, 0, 0.1))
    s.close()

The drag parameters are read by the kernel from a [B, 8] device tensor, so with ``graph=True`` ONE captured graph (graph_step.
GraphedStep over frozen weights) replays every drag by rule: a drag is one small host-to-device copy and a replay.  A drag by
explicit masks launches the kernel's mask form -- other kernel arguments -- and is a second capture, made at the first such
drag; the two graphs share the session's buffers.

Staleness.  A session is valid for the WEIGHTS and the SOURCE it was opened with: it holds network 1's outputs, network 2's
index sets and (``graph=True``) graphs that froze the weight packs.  After ``load_state_dict`` or any other change of the
parameters call ``reopen()``; for another mesh open another session.

A batch of meshes of DIFFERENT vertex counts -- the reference's batch loop over its user-handle data set, where the cloud is each
mesh's own vertex set -- goes through a ``RaggedEditSession`` over packed sets (nsdp_amd.ragged, include/nsdp_handles_ragged.h):

    s = RaggedEditSession(model, RaggedPoints.from_list([v0, v1, v2]))
    out = s.drag(part=["head", "tail", "head"], translation=(-0.15, -0.2, -0.2))      # RaggedPoints come back

Several handles at once, each with a motion of its own -- turn the head, lift a paw, pin the other feet -- go through a labelled
handle set on either session class (include/nsdp_handle_sets.h): a byte per point names its handle, a pose gives every handle a
3 x 4 motion (``Motion``: translate, rotate about a pivot, affine, composed on the host) or every point a target:

    labels, count = s.labels_from_parts(["head", "frontleftfoot"])      # or any uint8 labels of the caller's
    s.set_handles(labels, count)
    out = s.pose(motions=[Motion.rotate((0, 0, 1), 20, pivot=c), Motion.translate((0, 0, 0.1)), Motion.identity()])
    out = s.pose(targets=recorded_frame)                                # [B, n, 3]: read at the handle points
    out = s.track(motions=[pose_1, ..., pose_T])                        # EditSession: T poses, one pass over T * B rows

    python -m nsdp_amd.edit CONFIG --handles head,frontleftfoot [--rotate-deg 20 --axis 0,0,1] [--translate dx,dy,dz] [--track T]

Vertex normals of the deformed mesh, for whoever shows or exports it (nsdp_amd/mesh_normals.py, include/nsdp_meshnormals.h):
a session opened with ``faces`` builds the mesh's corner lists once and exposes ``verts_src_normals``; ``drag / pose / track(...,
normals=True)`` then add ``verts_tgt_normals`` (shaped as ``verts_tgt_pred``) -- two more launches behind the decode, inside
the captured graph, a graph of its own beside the one without normals.  The predictions are the same bits either way.

    s = EditSession(model, verts_src, faces=faces)       # faces [F, 3] shared by the B shapes, or [B, F, 3]
    out = s.drag(part="head", translation=(-0.15, -0.2, -0.2), normals=True)

    python -m nsdp_amd.edit CONFIG --vertices N --normals [--graph]      # a sphere mesh: the drag with and without normals

Self-intersections of the deformed mesh (nsdp_amd/self_intersect.py, include/nsdp_selfintersect.h): with ``faces``,
``drag / pose / track(..., self_intersections=True)`` add ``faces_tgt_hits`` (per face the faces it passes through; -1: skipped
by the work guard), ``tgt_self_intersections`` (the intersecting pairs of every mesh, of every pose and mesh for a track) and
``tgt_self_skipped`` -- behind the decode, inside a captured graph of its own; the predictions are the same bits either way.

    python -m nsdp_amd.edit CONFIG --vertices N --self-intersections [--graph]      # the counts of every drag, and its time

Every stage of a drag is the kernel the step function runs, on the same operands: the predictions are bit-equal to
``test_on_batch_with_arbitrary`` (``test_on_batch_with_cano`` for a single network) on the data_dict the drag stands for
(tests/test_edit_session_gpu.py, tests/test_edit_session_ragged_gpu.py).

Previews (nsdp_amd/rasterize.py, include/nsdp_raster.h): a session opened with ``faces`` takes ``drag / pose / track(...,
render=RenderSpec(cameras, height, width, shade=True, count=False))`` and adds ``tgt_depth`` and ``tgt_face_image`` [.., K, H, W],
``tgt_dropped`` [.., K] and, with ``shade``, the uint8 ``tgt_image`` [.., K, H, W, 3] of the deformed meshes -- three launches and
the shading's gathers behind the decode, inside the captured graph, a graph of its own per RenderSpec.  The predictions are the
same bits either way.  There is no near-plane clipping: ``tgt_dropped`` counts the faces that reach the camera plane.
``session.render(cameras, height, width, verts=None)`` draws the source mesh or given vertices.

    python -m nsdp_amd.edit CONFIG --vertices N --render OUT.png [--render-size S] [--graph]      # a sphere mesh, one fitted view
"""
from __future__ import annotations

import argparse
import json
import os
import sys
from dataclasses import dataclass

PARTS = ("head", "tail", "frontleftfoot", "frontrightfoot", "behindleftfoot", "behindrightfoot")      # the reference's priority
SEED_DATA, SEED_WEIGHTS = 1000, 2048      # (nsdp_amd.infer's)


@dataclass(eq=False)
class RenderSpec:
    """A preview of every deformed mesh behind a drag (nsdp_amd/rasterize.py, include/nsdp_raster.h): ``cameras`` -- a
    ``Camera``, a sequence of K of them, or a float32 GPU tensor [K, 4, 4] (the same K views of every mesh) or [..., K, 4, 4] --
    and the image's ``height`` and ``width``.  ``shade``: the head-light image ``tgt_image`` beside the depth and face images;
    ``count``: the per-pixel number of covering faces too.  One object per view set: the session keys its captured graph by it,
    and a graph reads the camera tensor where it lies -- write new matrices into ``tensor`` in place to move the camera."""
    cameras: object
    height: int
    width: int
    shade: bool = True
    count: bool = False
    tensor: object = None       # the cameras on the session's device, made at the first use


@dataclass(frozen=True)
class HandleSpec:
    """One drag of the bounding-box rule: which region moves, by how much, and the rule's two settings."""
    part: str
    translation: tuple
    partial_range: float = 0.1
    cliptail: bool = False

    def __post_init__(self):
        if self.part not in PARTS:
            raise ValueError(f"HandleSpec: part must be one of {PARTS}, got {self.part!r}")
        if len(self.translation) != 3:
            raise ValueError(f"HandleSpec: translation is (dx, dy, dz), got {self.translation!r}")

    @classmethod
    def from_config(cls, data_cfg):
        """From the ``data`` block of a reference user-handle config (config/tosca/head.yaml ...): the first of head, tail,
        frontleftfoot, frontrightfoot, behindleftfoot, behindrightfoot that is set -- the reference's if / elif chain -- moves by
        (xtrans, ytrans, ztrans).  No part set: ValueError (the reference fails on an unbound name there)."""
        if not isinstance(data_cfg, dict) or not isinstance(data_cfg.get("userhandle"), dict):
            raise ValueError("HandleSpec.from_config: the config's data block has no `userhandle` section")
        uh = data_cfg["userhandle"]
        part = next((p for p in PARTS if uh.get(p)), None)
        if part is None:
            raise ValueError(f"HandleSpec.from_config: none of {PARTS} is set in data.userhandle -- nothing to move")
        return cls(part=part, translation=tuple(float(uh.get(k, 0.0)) for k in ("xtrans", "ytrans", "ztrans")),
                   partial_range=float(data_cfg.get("partial_range", 0.1)), cliptail=bool(uh.get("cliptail", False)))


def pack_params(B, part, translation, partial_range, cliptail):
    """The [B, 8] int32 host array nsdp_handle_rows reads (include/nsdp_handles.h): ``part`` a name / index or one per shape,
    ``translation`` (dx, dy, dz) or [B, 3], ``partial_range`` and ``cliptail`` scalars or one per shape."""
    import numpy as np
    words = np.zeros((B, 8), dtype=np.int32)
    parts = [part] * B if isinstance(part, (str, int)) else list(part)
    if len(parts) != B:
        raise ValueError(f"drag: {len(parts)} parts for {B} shapes")
    for b, p in enumerate(parts):
        if isinstance(p, str):
            if p not in PARTS:
                raise ValueError(f"drag: part must be one of {PARTS}, got {p!r}")
            p = PARTS.index(p)
        if not 0 <= int(p) < len(PARTS):
            raise ValueError(f"drag: part index {p} outside 0..{len(PARTS) - 1}")
        words[b, 0] = int(p)
    d = np.asarray(translation, dtype=np.float32)
    if d.shape not in ((3,), (B, 3)):
        raise ValueError(f"drag: translation must be (dx, dy, dz) or [{B}, 3], got shape {d.shape}")
    words[:, 1] = np.broadcast_to(np.asarray(cliptail, dtype=bool), (B,)).astype(np.int32)
    f = words.view(np.float32)
    f[:, 2] = np.broadcast_to(np.asarray(partial_range, dtype=np.float32), (B,))
    f[:, 3:6] = np.broadcast_to(d, (B, 3))
    return words


class Motion:
    """x -> A x + t, what one handle does in a pose (include/nsdp_handle_sets.h): composed on the host in float64 and rounded
    ONCE to float32, by ``matrix()``.  A rotation about a pivot c is [R | c - R c]: the pivot is folded into t here, where float64
    is free, so the kernel's arithmetic stays three products and three sums per coordinate for every kind of motion."""
    __slots__ = ("m",)

    def __init__(self, m):
        import numpy as np
        a = np.array(m, dtype=np.float64)
        if a.shape == (12,):
            a = a.reshape(3, 4)
        if a.shape != (3, 4):
            raise ValueError(f"Motion: a 3 x 4 matrix [A | t] (or its 12 numbers, row-major), got shape {a.shape}")
        self.m = a

    @classmethod
    def identity(cls):
        """A pinned handle: its points are handle points whose target is where they are."""
        import numpy as np
        return cls(np.eye(3, 4))

    @classmethod
    def translate(cls, d):
        import numpy as np
        m = np.eye(3, 4)
        m[:, 3] = np.asarray(d, dtype=np.float64).reshape(3)
        return cls(m)

    @classmethod
    def affine(cls, A, t=(0.0, 0.0, 0.0)):
        import numpy as np
        return cls(np.concatenate([np.asarray(A, dtype=np.float64).reshape(3, 3), np.asarray(t, dtype=np.float64).reshape(3, 1)], axis=1))

    @classmethod
    def rotate(cls, axis, degrees, pivot=(0.0, 0.0, 0.0)):
        """By ``degrees`` about the line through ``pivot`` along ``axis`` (right-handed; any non-zero length)."""
        import numpy as np
        a = np.asarray(axis, dtype=np.float64).reshape(3)
        norm = float(np.linalg.norm(a))
        if not norm > 0.0 or not np.isfinite(norm):
            raise ValueError(f"Motion.rotate: the axis must have a finite non-zero length, got {tuple(a)}")
        a = a / norm
        quarter = float(degrees) / 90.0
        if quarter == round(quarter):      # whole quarter turns: cosine and sine are exactly 0, 1 or -1
            c, s = ((1.0, 0.0), (0.0, 1.0), (-1.0, 0.0), (0.0, -1.0))[int(round(quarter)) % 4]
        else:
            c, s = float(np.cos(np.radians(float(degrees)))), float(np.sin(np.radians(float(degrees))))
        K = np.array([[0.0, -a[2], a[1]], [a[2], 0.0, -a[0]], [-a[1], a[0], 0.0]])
        R = c * np.eye(3) + s * K + (1.0 - c) * np.outer(a, a)
        p = np.asarray(pivot, dtype=np.float64).reshape(3)
        return cls.affine(R, p - R @ p)

    def then(self, other):
        """This motion first, ``other`` after it."""
        import numpy as np
        A = other.m[:, :3] @ self.m[:, :3]
        t = other.m[:, :3] @ self.m[:, 3] + other.m[:, 3]
        return Motion(np.concatenate([A, t.reshape(3, 1)], axis=1))

    def matrix(self):
        """[3, 4] float32: the one rounding."""
        import numpy as np
        return self.m.astype(np.float32)

    def __repr__(self):
        return f"Motion({self.m.tolist()})"


def _motion12(m):
    """One motion as 12 float32 numbers (a Motion, or (12,) / (3, 4) numbers); None if ``m`` is not one."""
    import numpy as np
    if isinstance(m, Motion):
        return m.matrix().reshape(12)
    try:
        a = np.asarray(m, dtype=np.float64)
    except (TypeError, ValueError):
        return None
    return a.astype(np.float32).reshape(12) if a.shape in ((12,), (3, 4)) else None


def pack_motions(B, H, motions):
    """The [B, H, 12] float32 host array the labelled kernel reads, row h - 1 of a shape = the motion of its label h.
    ``motions``: one list of H motions (Motion, or 12 numbers) for every shape, a list of B such lists, or an array / tensor
    that already is [B, H, 12] (or [B, H, 3, 4])."""
    import numpy as np
    if hasattr(motions, "detach"):
        motions = motions.detach().cpu().numpy()
    if isinstance(motions, np.ndarray) and motions.dtype != object:
        if motions.shape in ((B, H, 12), (B, H, 3, 4)):
            return np.ascontiguousarray(motions.reshape(B, H, 12), dtype=np.float32)
        if motions.shape in ((H, 12), (H, 3, 4)):
            return np.array(np.broadcast_to(motions.reshape(1, H, 12), (B, H, 12)), dtype=np.float32, order="C")      # (a copy: writable)
        raise ValueError(f"pack_motions: an array of motions must be [{B}, {H}, 12] (B shapes, H handles), got {motions.shape}")
    if isinstance(motions, (Motion, str)) or not hasattr(motions, "__len__"):
        raise ValueError(f"pack_motions: a list of {H} motions, or one such list per shape, got {type(motions).__name__}")
    rows = list(motions)
    flat = [_motion12(m) for m in rows]
    if len(rows) == H and all(f is not None for f in flat):
        return np.array(np.broadcast_to(np.stack(flat)[None], (B, H, 12)), dtype=np.float32, order="C")      # (a copy: writable)
    if len(rows) == B and all(hasattr(r, "__len__") and not isinstance(r, (Motion, str)) for r in rows):
        out = np.empty((B, H, 12), dtype=np.float32)
        for b, shape_motions in enumerate(rows):
            per = [_motion12(m) for m in shape_motions]
            if len(per) != H or any(p is None for p in per):
                raise ValueError(f"pack_motions: shape {b} has {len(per)} motions for {H} handles, or one of them is no 3 x 4 motion")
            out[b] = np.stack(per)
        return out
    raise ValueError(f"pack_motions: {len(rows)} entries are neither {H} motions (one per handle) nor {B} lists (one per shape)")


def _networks_or_refusal(model):
    """The reasons that depend on the model alone -- its type, training mode, autograd -- as a string; without one, the list of
    the model's networks, the deformation network last."""
    import torch
    from .model.deformation_networks import Deformation_Networks
    from .model.flow_arbitrary import FlowArbitrary
    if isinstance(model, FlowArbitrary):
        nets = [model.model_canonicalize, model.model_deform]
    elif isinstance(model, Deformation_Networks):
        nets = [model]
    else:
        return f"the model must be a FlowArbitrary or a Deformation_Networks, got {type(model).__name__}"
    if model.training or any(m.training for m in model.modules()):
        return ("the model is in training mode: a session caches network 1's outputs and replays frozen weights, BatchNorm "
                "would take batch statistics -- call model.eval() first")
    if torch.is_grad_enabled():
        return ("autograd is enabled: a session runs the inference kernels over cached tensors and records no graph -- open it "
                "and drag under torch.no_grad()")
    return nets


def _network_refusal(net2, encoder_needs):
    """The reasons that depend on the storage type and the deformation network; ``encoder_needs``: the methods of its encoder
    the session's layout calls."""
    from . import precision
    if precision.is_bf16():
        return "bf16 storage (NSDP_STORAGE=bf16): the session is built and tested in fp32 storage only"
    if net2.no_input_corr:
        return "this network does not read the handle columns (no_input_corr: a backward-type network): a drag would change nothing"
    if not (all(hasattr(net2.encoder, m) for m in encoder_needs) and hasattr(net2.decoder, "geometry")):
        return (f"the {type(net2.encoder).__name__} / {type(net2.decoder).__name__} pair has no geometry(): it searches inside "
                "its forward pass only, so its index sets cannot be cached across drags")
    return None


def refusal(model, verts_src, surface=None, cano=None, surface_cano=None):
    """Why a session cannot be opened on these arguments (None: it can), each reason named."""
    import torch
    from .ragged import RaggedPoints
    nets = _networks_or_refusal(model)
    if isinstance(nets, str):
        return nets
    given = {"verts_src": verts_src, "surface": surface, "cano": cano, "surface_cano": surface_cano}
    for name, t in given.items():
        if isinstance(t, RaggedPoints):
            return (f"ragged inputs: {name} is a RaggedPoints -- an EditSession holds one rectangular [B, n, 3] set per role; "
                    "RaggedEditSession takes a packed batch of meshes of different sizes")
    why = _network_refusal(nets[-1], ("geometry",))
    if why is not None:
        return why
    for name, t in given.items():
        if t is None:
            continue
        if not torch.is_tensor(t):
            return f"{name} must be a torch.Tensor, got {type(t).__name__}"
        if t.dtype is not torch.float32 or t.dim() != 3 or t.shape[2] != 3:
            return f"{name} must be float32 [B, n, 3], got {t.dtype} {tuple(t.shape)}"
        if not t.is_cuda:
            return f"CPU tensors: {name} is on the CPU -- the session's kernels have no CPU path"
    B = verts_src.shape[0]
    if surface is not None and surface.shape[0] != B:
        return f"surface holds {surface.shape[0]} shapes, verts_src {B}"
    if cano is not None and cano.shape != verts_src.shape:
        return f"cano {tuple(cano.shape)} is not shaped like verts_src {tuple(verts_src.shape)}"
    if surface_cano is not None and (surface is None or surface_cano.shape != surface.shape):
        return "surface_cano goes with a surface of the same shape"
    return None


class _Session:
    """What an editing session is in either layout: the checks at open, the bookkeeping, one drag up to its dispatch -- the
    parameter copy, the mask buffers, capture or eager by (masks, vert_masks) -- and the end.  A layout (EditSession: rectangular
    sets; RaggedEditSession: packed ones) gives

      _refusal(model, verts_src, surface, cano, surface_cano)   why a session cannot be opened on these (None: it can);
      _hold(verts_src, surface, cano, surface_cano)             keeps the sets as it wants them, contiguous;
      _open()                                                   computes everything cached per source and weights;
      _layout()                                                 (B, the tensor that names the device, the shape of a mask over
                                                                the cloud, of one over the vertices);
      _enqueue(masks, vert_masks)                               the GPU work of a drag behind the copies;
      _enqueue_pose(targets, vert)                              the same for a pose of the labelled handle set (set_handles);
      _rule_flags(verts, handle_out, move_out)                  the rule kernel for its flags alone (labels_from_parts);
      _result(pred, own, own_pred, have_verts, with_inputs)     the dict a drag returns;
      _cached                                                   the attributes close() lets go of."""

    def __init__(self, model, verts_src, surface=None, cano=None, surface_cano=None, partial_range=0.1, cliptail=False,
                 graph=False, max_streams=None, faces=None):
        why = self._refusal(model, verts_src, surface, cano, surface_cano)
        if why is not None:
            raise ValueError(self._refused + why)
        self.faces = faces
        from . import query_shard
        from .model.flow_arbitrary import FlowArbitrary
        self.model = model
        self.flow = isinstance(model, FlowArbitrary)
        self.net = model.model_deform if self.flow else model
        # one decode standing for two, and network 1 decoding one set where the step function decodes the concatenation: both
        # rest on the decoder treating every query row on its own -- the fused fp32 decoder (query_shard names what is not)
        for net in ([model.model_canonicalize, self.net] if self.flow else [self.net]):
            query_shard.require_supported(net)
        self._hold(verts_src, surface, cano, surface_cano)
        self.partial_range, self.cliptail = float(partial_range), bool(cliptail)
        self.graph, self.max_streams = bool(graph), max_streams
        self.replays = self.eager_calls = 0
        self._steps = {}
        self._forget_handles()
        self._open()

    @property
    def _refused(self):
        return type(self).__name__ + " refused: "

    def reopen(self):
        """Recompute everything the session caches (after the weights changed) and drop the captured graphs."""
        why = self._refusal(self.model, self.verts, None if self.same else self.surface)
        if why is not None:
            raise ValueError(self._refused + why)
        self._drop_graphs()
        self._tracks = {}      # (a track holds index sets of its own; the labels and their count stay)
        self._open()
        return self

    # ------------------------------------------------------------------ vertex normals
    def _open_normals(self):
        """The last step of ``_open`` (outside any capture): the topology of ``faces`` over the vertices' layout -- the corner
        lists, one host read -- and the source mesh's normals.  Without faces the session holds neither."""
        self.topology = self.verts_src_normals = self.selfint_plan = self.pick_plan = self.brush_plan = self.render_plan = None
        if self.faces is not None:
            from .mesh_normals import MeshTopology, vertex_normals
            self.topology = MeshTopology(self.faces, self.verts)
            self.verts_src_normals = vertex_normals(self.verts, self.topology)

    def _normals_wanted(self, what, normals):
        if normals and self.topology is None:
            raise ValueError(self._refused + f"{what}(normals=True) without faces: the session was opened without `faces`, and "
                             "vertex normals need the mesh's triangles -- open it with faces=...")
        return bool(normals)

    def _selfint_wanted(self, what, wanted):
        """``self_intersections=True`` needs the faces; the plan (the faces in Morton order of the source mesh, no host read:
        the topology is validated) is made at the first such call, outside any capture."""
        if wanted and self.topology is None:
            raise ValueError(self._refused + f"{what}(self_intersections=True) without faces: the session was opened without "
                             "`faces`, and self-intersections are between the mesh's triangles -- open it with faces=...")
        if wanted and self.selfint_plan is None:
            from .self_intersect import SelfIntersectionPlan
            self.selfint_plan = SelfIntersectionPlan(self.faces, self.verts, topology=self.topology)
        return bool(wanted)

    def pick(self, origins, directions, verts=None):
        """A click as a ray (nsdp_amd/ray_cast.py, include/nsdp_raycast.h): the first face of mesh ``b`` that the rays ``origins
        + t directions`` of shape ``b`` meet ([B, n, 3] fp32 on the GPU; RaggedPoints over the batch for a packed session) --
        against the source mesh, or against ``verts``, a vertex set of the same topology such as a drag's ``verts_tgt_pred``.
        Returns ``t`` (FLT_MAX without a hit), ``face`` (local to its mesh, -1: none), ``bary`` (the weights of the face's
        corners), ``vertex`` (the hit face's corner of the largest weight, the lowest corner on ties; local, -1: none) and
        ``label``: the vertex's handle label of ``set_handles`` -- the ``vert_labels``, or the labels themselves where the cloud
        is the vertex set -- 0 without a hit, None before any labels are set.  A call of its own: it is no part of a drag's
        graph and the predictions keep their bits.  The plan (the faces in Morton order of the source mesh) is made at the
        first pick."""
        import torch
        from .ragged import RaggedPoints, shape_ids
        if self.topology is None:
            raise ValueError(self._refused + "pick() without faces: the session was opened without `faces`, and a ray meets the "
                             "mesh's triangles -- open it with faces=...")
        from .ray_cast import RayCastPlan, cast_rays, hit_vertices
        if self.pick_plan is None:
            self.pick_plan = RayCastPlan(self.faces, self.verts, topology=self.topology)
        with torch.no_grad():
            hits = cast_rays(origins, directions, self.verts if verts is None else verts, self.pick_plan, return_bary=True, count=False)
            vertex = hit_vertices(hits, self.pick_plan)
            labels = self._vlabels if self._vert_labelled else (self._labels if self.same else None)
            label = None
            if labels is not None:
                if isinstance(vertex, RaggedPoints):
                    topo, v = self.topology, vertex.packed[:, 0]
                    owner = shape_ids(origins.offsets, origins.capacity).clamp(max=topo.shapes - 1)
                    rows = (v.long().clamp(min=0) + topo.vert_offsets[:-1].long()[owner]).clamp(0, topo.vcap - 1)
                    label = vertex.like(torch.where(v >= 0, labels.reshape(-1)[rows], labels.new_zeros(())).unsqueeze(1))
                else:
                    got = torch.gather(labels, 1, vertex.long().clamp(min=0))
                    label = torch.where(vertex >= 0, got, torch.zeros_like(got))
        return {"t": hits.t, "face": hits.face, "bary": hits.bary, "vertex": vertex, "label": label}

    def _with_self_intersections(self, pred, lead=None):
        """``pred`` with the self-intersections of its vertices (nsdp_amd/self_intersect.py): the entry's launches behind the
        decode.  The predictions themselves are not touched."""
        from .self_intersect import self_intersections
        verts = pred["verts_tgt_pred"]
        r = self_intersections(verts if lead is None else verts.view(lead + tuple(verts.shape[-2:])), self.selfint_plan)
        out = dict(pred)
        out["faces_tgt_hits"], out["tgt_self_intersections"], out["tgt_self_skipped"] = r.hits, r.pairs, r.skipped
        return out

    def _with_normals(self, pred, lead=None):
        """``pred`` with the normals of its vertices: two launches behind the decode (``lead``: a track's (T, B) in front of
        [V, 3]).  The predictions themselves are not touched."""
        from .mesh_normals import vertex_normals
        verts = pred["verts_tgt_pred"]
        out = dict(pred)
        out["verts_tgt_normals"] = vertex_normals(verts if lead is None else verts.view(lead + tuple(verts.shape[-2:])), self.topology)
        return out

    # ------------------------------------------------------------------ previews
    def _render_wanted(self, what, render):
        """``render=RenderSpec(...)`` needs the faces; the plan (the faces in Morton order of the source mesh, no host read: the
        topology is validated) and the spec's camera tensor are made at the first such call, outside any capture."""
        if render is None:
            return None
        if not isinstance(render, RenderSpec):
            raise ValueError(f"{what}: render must be a RenderSpec(cameras, height, width), got {type(render).__name__}")
        if self.topology is None:
            raise ValueError(self._refused + f"{what}(render=...) without faces: the session was opened without `faces`, and a "
                             "rasteriser draws the mesh's triangles -- open it with faces=...")
        from .rasterize import RasterPlan, camera_tensor
        if self.render_plan is None:
            self.render_plan = RasterPlan(self.faces, self.verts, topology=self.topology)
        if render.tensor is None:
            render.tensor = camera_tensor(render.cameras, self.topology.device)
            if hasattr(render.tensor, "contiguous"):
                render.tensor = render.tensor.contiguous()
        return render

    def _with_render(self, pred, spec, lead=None):
        """``pred`` with the images of its vertices (no near-plane clipping: ``tgt_dropped`` counts the faces that reach the
        camera plane): three launches behind the decode, and the shading's gathers.  The predictions are not touched."""
        from .rasterize import rasterize, shade
        verts = pred["verts_tgt_pred"]
        verts = verts if lead is None else verts.view(lead + tuple(verts.shape[-2:]))
        r = rasterize(verts, self.render_plan, spec.tensor, spec.height, spec.width, return_bary=spec.shade, count=spec.count)
        out = dict(pred)
        out["tgt_depth"], out["tgt_face_image"], out["tgt_dropped"] = r.depth, r.face, r.dropped
        if spec.count:
            out["tgt_count_image"] = r.count
        if spec.shade:
            out["tgt_image"] = shade(r, verts, self.render_plan, normals=pred.get("verts_tgt_normals"))
        return out

    def render(self, cameras, height, width, verts=None, shade=True, count=False):
        """The source mesh, or ``verts`` -- a vertex set of the same topology such as a drag's ``verts_tgt_pred`` -- under
        ``cameras`` (what ``RenderSpec`` takes): ``tgt_depth``, ``tgt_face_image`` [.., K, H, W], ``tgt_dropped`` [.., K] and with
        ``shade`` the uint8 ``tgt_image`` [.., K, H, W, 3].  A call of its own, no part of a drag's graph."""
        import torch
        spec = self._render_wanted("render", RenderSpec(cameras, height, width, shade, count))
        v = self.verts if verts is None else verts
        with torch.no_grad():
            out = self._with_render({"verts_tgt_pred": v.packed if hasattr(v, "packed") else v}, spec)
        return {k: out[k] for k in ("tgt_depth", "tgt_face_image", "tgt_dropped", "tgt_count_image", "tgt_image") if k in out}

    # ------------------------------------------------------------------ one drag
    def _mask_buffer(self, name, like_rows, value, device):
        import torch
        buf = getattr(self, name)
        if buf is None:
            buf = torch.empty(like_rows, dtype=torch.uint8, device=device)
            setattr(self, name, buf)
        if not torch.is_tensor(value) or not value.is_cuda:
            raise ValueError(self._refused + "CPU tensors: the masks of a drag must be GPU tensors")
        if value.dtype not in (torch.bool, torch.uint8) or tuple(value.shape) != tuple(like_rows):
            raise ValueError(f"drag: a mask must be bool / uint8 {tuple(like_rows)}, got {value.dtype} {tuple(value.shape)}")
        buf.copy_(value, non_blocking=True)

    def drag(self, part=None, translation=(0.0, 0.0, 0.0), handle_mask=None, move_mask=None, vert_handle_mask=None,
             vert_move_mask=None, partial_range=None, cliptail=None, with_inputs=False, clone=True, normals=False,
             self_intersections=False, render=None):
        """One drag of every shape.  By rule: ``part`` (a name of PARTS, one per shape, or a HandleSpec) moves by ``translation``
        ((dx, dy, dz) or [B, 3]).  By explicit regions: ``handle_mask`` / ``move_mask`` over the cloud (bool / uint8 on the GPU:
        [B, n] for a rectangular cloud, (scap,) for a packed one) replace the rule; with a separate cloud ``vert_handle_mask`` /
        ``vert_move_mask`` ([B, V], packed (cap,)) do so for the vertices (without them ``verts_tgt`` and
        ``cano_handle_vert_idx`` are None).

        Returns ``verts_tgt_pred``, ``surface_samples_tgt_pred``, ``verts_tgt``, ``cano_handle_vert_idx`` and
        ``cano_handle_sample_idx``, and with ``with_inputs`` ``surface_samples_inputs`` = [src | mask * tgt | mask], what the step
        function takes as it is -- shaped as the session's ``_result`` says.  The tensors are the caller's own; ``clone=False``
        hands out the session's buffers, overwritten by the next drag.  ``normals=True`` (a session opened with ``faces``) adds
        ``verts_tgt_normals``, the unit vertex normals of ``verts_tgt_pred`` in its shape.  ``self_intersections=True`` (faces
        too) adds ``faces_tgt_hits`` (per face the faces it passes through, -1: skipped by the work guard),
        ``tgt_self_intersections`` (int64, the intersecting pairs of every mesh) and ``tgt_self_skipped`` -- the fields of
        ``nsdp_amd.self_intersect.self_intersections`` on ``verts_tgt_pred``.  ``render=RenderSpec(cameras, height, width)``
        (faces too) adds ``tgt_depth`` and ``tgt_face_image`` [.., K, H, W], ``tgt_dropped`` [.., K] (the faces that reach the
        camera plane: there is no near-plane clipping) and, with the spec's ``shade``, the uint8 ``tgt_image`` [.., K, H, W, 3]
        -- ``nsdp_amd.rasterize.rasterize`` on ``verts_tgt_pred``, inside the captured graph."""
        import torch
        from ._lib import on_device
        normals = self._normals_wanted("drag", normals)
        selfint = self._selfint_wanted("drag", self_intersections)
        render = self._render_wanted("drag", render)
        if torch.is_grad_enabled():
            raise ValueError(self._refused + "autograd is enabled -- drag under torch.no_grad()")
        if self.model.training:
            raise ValueError(self._refused + "the model is in training mode -- call model.eval() (and reopen() if the weights "
                             "changed)")
        if isinstance(part, HandleSpec):
            spec, part, translation = part, part.part, part.translation
            partial_range = spec.partial_range if partial_range is None else partial_range
            cliptail = spec.cliptail if cliptail is None else cliptail
        masks = handle_mask is not None or move_mask is not None
        B, on, cloud_rows, vert_rows = self._layout()
        if masks:
            if handle_mask is None or move_mask is None or part is not None:
                raise ValueError("drag: handle_mask and move_mask go together and replace `part`")
            if (vert_handle_mask is None) != (vert_move_mask is None) or (self.same and vert_handle_mask is not None):
                raise ValueError("drag: vert_handle_mask and vert_move_mask go together, with a separate cloud only")
            part = 0
        elif part is None:
            raise ValueError(f"drag: name the part that moves (one of {PARTS}) or give handle_mask and move_mask")
        elif vert_handle_mask is not None or vert_move_mask is not None:
            raise ValueError("drag: vertex masks go with handle_mask and move_mask")
        vert_masks = masks and vert_handle_mask is not None
        words = pack_params(B, part, translation, self.partial_range if partial_range is None else partial_range,
                            self.cliptail if cliptail is None else cliptail)
        with on_device(on):
            # the one host-to-device copy of a drag, stream-ordered in front of the kernels that read it (pageable memory: the
            # runtime has taken the bytes when copy_ returns, so the host array is free at once)
            self.params.copy_(torch.from_numpy(words), non_blocking=True)
            if masks:
                self._mask_buffer("_mask_h", cloud_rows, handle_mask, on.device)
                self._mask_buffer("_mask_m", cloud_rows, move_mask, on.device)
                if vert_masks:
                    self._mask_buffer("_vmask_h", vert_rows, vert_handle_mask, on.device)
                    self._mask_buffer("_vmask_m", vert_rows, vert_move_mask, on.device)
            key = (masks, vert_masks)
            pred = self._dispatch_normals(key, lambda: self._enqueue(*key), normals, selfint=selfint, render=render)
            own, own_pred = self._owners(clone)
            return self._add_normals(self._result(pred, own, own_pred, self.same or not masks or vert_masks, with_inputs), pred, own_pred)

    def _dispatch_normals(self, key, enqueue, normals, lead=None, selfint=False, render=None):
        """``_dispatch``; with ``normals`` the vertex normals behind the same work, with ``selfint`` the self-intersections,
        with ``render`` the images, each under a key of its own (another graph): calls without the flags keep their graph and
        their bits."""
        if not normals and not selfint and render is None:
            return self._dispatch(key, enqueue)

        def work():
            pred = enqueue()
            if normals:
                pred = self._with_normals(pred, lead)
            if render is not None:
                pred = self._with_render(pred, render, lead)
            return self._with_self_intersections(pred, lead) if selfint else pred
        return self._dispatch(key + (("normals",) if normals else ()) + (("self_intersections",) if selfint else ()) +
                              (("render", id(render), render.height, render.width, render.shade, render.count) if render is not None
                               else ()), work)

    def _add_normals(self, out, pred, own_pred, shape=None):
        if "verts_tgt_normals" in pred:
            n = own_pred(pred["verts_tgt_normals"])
            out["verts_tgt_normals"] = self._over_verts(n if shape is None else n.view(shape))
        for name in ("faces_tgt_hits", "tgt_self_intersections", "tgt_self_skipped", "tgt_depth", "tgt_face_image", "tgt_dropped",
                     "tgt_count_image", "tgt_image"):
            if name in pred:
                out[name] = own_pred(pred[name])
        return out

    @staticmethod
    def _over_verts(t):
        return t

    def _dispatch(self, key, enqueue):
        """The GPU work of one call behind its copies: op by op, or (``graph=True``) captured at the first call of this ``key``
        and replayed from then on."""
        if self.graph:
            if key not in self._steps:
                from .graph_step import GraphedStep
                self._steps[key] = GraphedStep(enqueue, self.max_streams, weights_change=False).capture(warmup=1)
            self.replays += 1
            return self._steps[key]()
        self.eager_calls += 1
        return enqueue()

    def _owners(self, clone):
        own = (lambda t: t.clone()) if clone else (lambda t: t)      # the session's buffers: the next drag overwrites them
        return own, (own if self.graph else (lambda t: t))           # (an eager drag's predictions are fresh tensors)

    # ------------------------------------------------------------------ labelled handle sets
    def _forget_handles(self):
        self._labels = self._vlabels = self._motions = self._targets = self._vtargets = None
        self._count, self._vert_labelled, self._tracks = 0, False, {}

    def _drop_set_graphs(self):
        for key in [k for k in self._steps if k[0] in ("pose", "track")]:
            self._steps.pop(key).close()

    def _session_tensor(self, value, shape, dtype, what):
        """Refuses ``value`` unless it is a GPU tensor of ``shape`` and ``dtype``."""
        import torch
        if not torch.is_tensor(value):
            raise ValueError(f"{what} must be a torch.Tensor, got {type(value).__name__}")
        if not value.is_cuda:
            raise ValueError(self._refused + f"CPU tensors: {what} must be a GPU tensor")
        if value.dtype is not dtype or tuple(value.shape) != tuple(shape):
            raise ValueError(f"{what} must be {str(dtype).replace('torch.', '')} {tuple(shape)}, got "
                             f"{str(value.dtype).replace('torch.', '')} {tuple(value.shape)}")

    def _session_copy(self, name, value):
        """``value`` copied into the session's buffer ``name``, made at first use (the graphs read the buffer)."""
        import torch
        buf = getattr(self, name)
        if buf is None:
            buf = torch.empty_like(value, memory_format=torch.contiguous_format)
            setattr(self, name, buf)
        buf.copy_(value, non_blocking=True)

    def set_handles(self, labels, count, vert_labels=None):
        """The handle set the next poses move: ``labels`` uint8 on the GPU over the cloud ([B, n]; (scap,) for a packed cloud),
        0 = a free point, h in 1..``count`` = a point of handle h (a larger label is a free point).  ``count`` = H is the
        caller's, so nothing is read back.  ``vert_labels`` ([B, V]; packed (cap,)): the same for the vertices of a separate
        cloud; without them ``verts_tgt`` and ``cano_handle_vert_idx`` come back None, as for drags by masks.  The labels are
        copied.  Setting them again with the same ``count`` keeps the captured graphs of the poses."""
        import torch
        from ._lib import on_device
        if isinstance(count, bool) or not isinstance(count, int) or not 1 <= count <= 255:
            raise ValueError(f"set_handles: count must be an integer in 1..255 (the labels are bytes), got {count!r}")
        B, on, cloud_rows, vert_rows = self._layout()
        if vert_labels is not None and self.same:
            raise ValueError("set_handles: vert_labels go with a separate cloud only (here the cloud is the vertex set)")
        self._session_tensor(labels, cloud_rows, torch.uint8, "set_handles: labels")
        if vert_labels is not None:
            self._session_tensor(vert_labels, vert_rows, torch.uint8, "set_handles: vert_labels")
        with on_device(on):
            self._session_copy("_labels", labels)
            self._vert_labelled = vert_labels is not None      # (the buffer stays: a captured graph reads it)
            if self._vert_labelled:
                self._session_copy("_vlabels", vert_labels)
            if count != self._count:      # (the motion tables are [.., H, 12]: other kernel arguments)
                self._drop_set_graphs()
                self._tracks = {}
                self._motions = torch.empty((B, count, 12), dtype=torch.float32, device=on.device)
                self._count = count
        return self

    def _pose_checks(self, what, motions, targets, vert_targets):
        import torch
        if torch.is_grad_enabled():
            raise ValueError(self._refused + f"autograd is enabled -- {what} under torch.no_grad()")
        if self.model.training:
            raise ValueError(self._refused + "the model is in training mode -- call model.eval() (and reopen() if the weights "
                             "changed)")
        if self._labels is None:
            raise ValueError(f"{what} before set_handles: the session has no labelled handle set")
        if (motions is None) == (targets is None):
            raise ValueError(f"{what}: exactly one of motions and targets (got {'neither' if motions is None else 'both'})")
        if vert_targets is not None:
            if targets is None:
                raise ValueError(f"{what}: vert_targets go with targets")
            if not self._vert_labelled:
                raise ValueError(f"{what}: vert_targets without vert_labels -- set_handles(labels, count, vert_labels) names the "
                                 "vertices they belong to" + (" (here the cloud is the vertex set: targets are theirs)" if self.same else ""))
        # the vertices' own rows: with a separate cloud, when their labels are set and this form has something to move them by
        return not self.same and self._vert_labelled and (targets is None or vert_targets is not None)

    def pose(self, motions=None, targets=None, vert_targets=None, with_inputs=False, clone=True, normals=False,
             self_intersections=False, render=None):
        """One pose of every shape's labelled handle set (``set_handles``).  ``motions``: anything ``pack_motions`` takes -- one
        list of H motions for every shape, a list per shape, or a [B, H, 12] array; one host-to-device copy.  ``targets``: a
        target per cloud point instead, a float32 GPU tensor over the cloud's layout with 3 columns ([B, n, 3]; (scap, 3)),
        read at the handle points only; ``vert_targets`` the same for the vertices of a separate cloud.  Returns what ``drag``
        returns, in the same shapes (``normals=True``: with ``verts_tgt_normals``; ``self_intersections=True``: with ``drag``'s
        three fields; ``render=RenderSpec(...)``: with ``drag``'s images)."""
        import torch
        from ._lib import on_device
        normals = self._normals_wanted("pose", normals)
        selfint = self._selfint_wanted("pose", self_intersections)
        render = self._render_wanted("pose", render)
        vert = self._pose_checks("pose", motions, targets, vert_targets)
        B, on, cloud_rows, vert_rows = self._layout()
        if targets is None:
            words = pack_motions(B, self._count, motions)
        else:
            self._session_tensor(targets, cloud_rows + (3,), torch.float32, "pose: targets")
            if vert:
                self._session_tensor(vert_targets, vert_rows + (3,), torch.float32, "pose: vert_targets")
        with on_device(on):
            if targets is None:
                self._motions.copy_(torch.from_numpy(words), non_blocking=True)
            else:
                self._session_copy("_targets", targets)
                if vert:
                    self._session_copy("_vtargets", vert_targets)
            key = ("pose", targets is not None, vert)
            pred = self._dispatch_normals(key, lambda: self._enqueue_pose(*key[1:]), normals, selfint=selfint, render=render)
            own, own_pred = self._owners(clone)
            return self._add_normals(self._result(pred, own, own_pred, self.same or vert, with_inputs), pred, own_pred)

    def labels_from_parts(self, parts, verts=False):
        """Labels for ``set_handles`` from the bounding-box rule: the rule kernel runs once per named part and its ``move_out``
        becomes label i + 1 for the i-th part (earlier parts win where regions overlap); label ``count`` = len(parts) + 1 =
        every other handle point of the rule.  Returns ``(labels, count)`` over the cloud (``verts=True``: over the vertices of
        a separate cloud).  Set-up work, not per drag: len(parts) launches and a few array operations."""
        import torch
        from ._lib import on_device
        parts = list(parts)
        if not 1 <= len(parts) <= 254 or any(p not in PARTS for p in parts):
            raise ValueError(f"labels_from_parts: 1..254 names of {PARTS}, got {parts!r}")
        B, on, cloud_rows, vert_rows = self._layout()
        rows = vert_rows if verts and not self.same else cloud_rows
        count = len(parts) + 1
        with on_device(on):
            handle = torch.zeros(rows, dtype=torch.uint8, device=on.device)      # (zeros: padding rows, which no kernel writes, are free points)
            move = torch.zeros(rows, dtype=torch.uint8, device=on.device)
            labels = None
            for i in reversed(range(len(parts))):
                words = pack_params(B, parts[i], (0.0, 0.0, 0.0), self.partial_range, self.cliptail)
                self.params.copy_(torch.from_numpy(words), non_blocking=True)
                self._rule_flags(verts and not self.same, handle, move)
                if labels is None:
                    labels = handle * count
                labels = torch.where(move != 0, torch.full_like(labels, i + 1), labels)
        return labels, count

    def labels_from_brush(self, strokes, verts=False, pose_verts=None):
        """Labels for ``set_handles`` from brush strokes on the mesh (nsdp_amd/geodesic.py, include/nsdp_geodesic.h):
        ``strokes`` is a list of ``(vertex, radius)`` -- ``vertex`` what ``pick()`` returns as ``"vertex"``, or any [B] / [B, s]
        integer tensor of local vertex indices (-1: none, the stroke labels nothing in that shape), ``radius`` a float or a [B]
        tensor -- and stroke i labels every vertex within ``radius`` of its seeds ALONG the mesh's edges with i + 1 (closed at
        the radius; earlier strokes win where they overlap); ``count = len(strokes)``.  Distances are measured on the source
        mesh, or on ``pose_verts``, a vertex set of the same topology such as a drag's ``verts_tgt_pred``.  Returns ``(labels,
        count)`` as ``labels_from_parts`` does: over the cloud -- where the cloud is separate the vertex labels are carried to
        it through ``closest_on_mesh`` + ``transfer_vertex_labels`` on the source mesh, and ``verts=True`` gives the vertex
        labels themselves.  Set-up work, no part of a drag's graph: the predictions keep their bits.  The plan (the vertices in
        Morton order of the source mesh) is made at the first brush."""
        import torch
        from .ragged import RaggedPoints, shape_ids
        if self.topology is None:
            raise ValueError(self._refused + "labels_from_brush() without faces: the session was opened without `faces`, and a "
                             "brush measures along the mesh's triangles -- open it with faces=...")
        strokes = list(strokes)
        if not 1 <= len(strokes) <= 255 or any(not isinstance(s, (tuple, list)) or len(s) != 2 for s in strokes):
            raise ValueError(f"labels_from_brush: 1..255 strokes (vertex, radius), got {len(strokes)}")
        from .geodesic import GeodesicPlan, geodesic_distances
        B, on, cloud_rows, vert_rows = self._layout()
        topo = self.topology
        with torch.no_grad():
            if self.brush_plan is None:
                self.brush_plan = GeodesicPlan(self.faces, self.verts, topology=topo)
            mesh = self.verts if pose_verts is None else pose_verts
            ragged = isinstance(self.verts, RaggedPoints)
            labels = torch.zeros(vert_rows, dtype=torch.uint8, device=on.device)
            self.brush_stats = []
            for i in reversed(range(len(strokes))):
                vertex, radius = strokes[i]
                if isinstance(vertex, RaggedPoints):
                    vertex = vertex.padded(-1)
                if not torch.is_tensor(vertex) or vertex.is_floating_point() or vertex.dim() < 1 or vertex.shape[0] != B:
                    raise ValueError(f"labels_from_brush: stroke {i}: vertex must be an integer tensor [B] or [B, s] over the {B} "
                                     "shapes (pick()'s \"vertex\")")
                seeds = vertex.to(on.device).reshape(B, -1)
                if torch.is_tensor(radius):
                    if radius.numel() != B:
                        raise ValueError(f"labels_from_brush: stroke {i}: radius must be a float or [B] = [{B}]")
                    per_shape = radius.to(on.device, torch.float32).reshape(B)
                    limit = float(per_shape.max())      # (set-up work: one read; a path within r_b has every prefix within it)
                else:
                    per_shape, limit = None, float(radius)
                if not limit >= 0.0:
                    raise ValueError(f"labels_from_brush: stroke {i}: radius {limit} is NaN or negative")
                dist, stats = geodesic_distances(mesh, self.brush_plan, seeds, limit=limit, return_stats=True)
                self.brush_stats.insert(0, stats)      # (per stroke, in the strokes' order: rounds and calls)
                dist = dist.packed[:, 0] if ragged else dist.reshape(vert_rows)
                if per_shape is None:
                    inside = dist <= limit
                elif ragged:
                    inside = dist <= per_shape[shape_ids(topo.vert_offsets, topo.vcap).clamp(max=B - 1)]
                else:
                    inside = dist <= per_shape[:, None]
                labels = torch.where(inside, torch.full_like(labels, i + 1), labels)
            if self.same or verts:
                return labels, len(strokes)
            return self._labels_to_cloud(labels, cloud_rows), len(strokes)

    def _labels_to_cloud(self, vert_labels, cloud_rows):
        """Vertex labels carried to a separate cloud: every cloud point takes the label of the closest mesh point's corner of
        the largest weight (``closest_on_mesh`` on the source mesh, ``transfer_vertex_labels``' rule)."""
        import torch
        from .ragged import RaggedPoints, shape_ids
        from .surface_distance import closest_on_mesh, transfer_vertex_labels
        if not isinstance(self.verts, RaggedPoints):
            B = self.verts.shape[0]
            faces = self.faces if self.faces.dim() == 3 else self.faces[None].expand(B, -1, -1)
            _, face, bary = closest_on_mesh(self.surface, self.verts, faces.contiguous())
            return transfer_vertex_labels(vert_labels, faces, face, bary).reshape(cloud_rows)
        cloud = RaggedPoints.from_list(list(self.surface)) if self.rect else self.surface
        _, face, bary = closest_on_mesh(cloud, self.verts, self.faces)
        topo, B = self.topology, self.verts.batch
        owner = shape_ids(cloud.offsets, cloud.capacity).clamp(max=B - 1)
        f = face.packed[:, 0]
        rows = (f.long().clamp(min=0) + topo.face_offsets.long()[owner]).clamp(0, topo.fcap - 1)
        corner = torch.argmax(bary.packed, dim=1, keepdim=True)
        local = torch.gather(topo.faces.long()[rows], 1, corner)[:, 0]
        vrow = (local + topo.vert_offsets.long()[owner]).clamp(0, topo.vcap - 1)
        out = torch.where(f >= 0, vert_labels[vrow], torch.zeros_like(vert_labels[vrow]))
        return out.reshape(cloud_rows)

    # ------------------------------------------------------------------ the end
    def _drop_graphs(self):
        for step in self._steps.values():
            step.close()
        self._steps = {}

    def close(self):
        self._drop_graphs()
        self._forget_handles()
        for name in self._cached + ("topology", "verts_src_normals", "selfint_plan", "pick_plan", "brush_plan", "render_plan"):
            setattr(self, name, None)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


class EditSession(_Session):
    """See the module text.  ``verts_src`` [B, V, 3] fp32 on the GPU; ``surface`` [B, S, 3]: the cloud network 2 encodes (None:
    the vertex set itself, as in the reference's user-handle data set); ``cano`` / ``surface_cano``: the coordinates the
    bounding-box rule is evaluated on (None: the source coordinates -- what the reference does, every frame of its pairs being
    frame 0000).  ``partial_range`` / ``cliptail``: the rule's settings, defaults of every drag.

    ``model``: a FlowArbitrary in eval mode, or one Deformation_Networks of the forward type (no network 1: canonical = source,
    only the index sets are cached).

    ``graph=True``: the first drag captures everything behind the parameter copy; later drags are copy + replay (``replays``;
    ``eager_calls`` counts drags run op by op).

    ``faces``: the mesh's triangles, int32 / int64 on the GPU -- [F, 3] shared by the B shapes or [B, F, 3] -- for
    ``verts_src_normals`` and ``normals=True`` (nsdp_amd.mesh_normals.MeshTopology: one host read at open)."""

    _refusal = staticmethod(refusal)
    _cached = ("geometry", "buf", "_surf_idx")

    def _hold(self, verts_src, surface, cano, surface_cano):
        self.verts = verts_src.contiguous()
        self.same = surface is None
        self.surface = self.verts if self.same else surface.contiguous()
        self.verts_rule = self.verts if cano is None else cano.contiguous()
        self.surface_rule = (self.verts_rule if self.same else self.surface) if surface_cano is None else surface_cano.contiguous()

    def _layout(self):
        return self.verts.shape[0], self.verts, tuple(self.surface.shape[:2]), tuple(self.verts.shape[:2])

    # ------------------------------------------------------------------ the cached state
    def _open(self):
        import torch
        from . import pointnet2_utils as pu
        with torch.no_grad():
            dev = self.verts.device
            B, V, S = self.verts.shape[0], self.verts.shape[1], self.surface.shape[1]
            if self.flow:
                sets = [self.surface] if self.same else [self.surface, self.verts]
                outs = self.model.canonicalize(sets, self.surface)
                self.surf2cano, self.verts2cano = outs[0].contiguous(), outs[-1].contiguous()
            else:
                self.surf2cano, self.verts2cano = self.surface, self.verts
            # the deformation network's input rows: columns 0:3 written here, once; 3:7 by every drag's kernel
            self.buf = torch.zeros((B, S, 7), dtype=torch.float32, device=dev)
            self.buf[:, :, 0:3] = self.surf2cano
            self.geometry = self.net.geometry(self.verts2cano, self.buf)
            self._surf_idx = None if self.same else self.net.decoder.geometry(self.surf2cano, self.geometry["encoder"]["anchors"])["query_idx"]
            self.bounds = pu.handle_bounds(self.surface_rule)
            self.verts_bounds = self.bounds if self.same else pu.handle_bounds(self.verts_rule)
            self.params = torch.zeros((B, 8), dtype=torch.int32, device=dev)
            self.surface_tgt = torch.empty((B, S, 3), dtype=torch.float32, device=dev)
            self.surface_handle = torch.empty((B, S), dtype=torch.uint8, device=dev)
            self._mask_h = self._mask_m = self._vmask_h = self._vmask_m = None      # (made by the first drag by masks)
            if self.same:
                self.verts_tgt, self.verts_handle, self._vrows = self.surface_tgt, self.surface_handle, None
            else:
                self.verts_tgt = torch.empty((B, V, 3), dtype=torch.float32, device=dev)
                self.verts_handle = torch.empty((B, V), dtype=torch.uint8, device=dev)
                self._vrows = torch.empty((B, V, 7), dtype=torch.float32, device=dev)      # (the kernel's required output)
            self._open_normals()

    # ------------------------------------------------------------------ one drag
    def _enqueue(self, masks, vert_masks):
        """Everything of a drag that runs on the GPU behind the parameter copy: capturable, reads device tensors only."""
        from . import pointnet2_utils as pu
        hm, mm = (self._mask_h, self._mask_m) if masks else (None, None)
        pu.handle_rows(self.surface_rule, self.surface, self.bounds, self.params, self.buf, hm, mm, tgt=self.surface_tgt,
                       handle_out=self.surface_handle)
        if not self.same and (not masks or vert_masks):
            vh, vm = (self._vmask_h, self._vmask_m) if masks else (None, None)
            pu.handle_rows(self.verts_rule, self.verts, self.verts_bounds, self.params, self._vrows, vh, vm, tgt=self.verts_tgt,
                           handle_out=self.verts_handle)
        return self._network(self.buf, self.geometry, self.verts2cano, self.surf2cano, self._surf_idx)

    def _network(self, buf, geometry, verts2cano, surf2cano, surf_idx):
        """Network 2 over input rows whose columns 3:7 a handle kernel has just written: the encoder over the cached index sets
        and one decode (two with a separate cloud)."""
        net = self.net
        enc = net.encode(buf, geometry=geometry)
        out = {"verts_tgt_pred": net.decode(verts2cano, enc)}
        if not self.same:
            enc_s = dict(enc)
            enc_s["query_idx"], enc_s["query_points"] = surf_idx, surf2cano
            out["surface_samples_tgt_pred"] = net.decode(surf2cano, enc_s)
        return out

    def _enqueue_pose(self, targets, vert):
        """``_enqueue`` for a pose of the labelled handle set: the labelled kernel in place of the rule's."""
        from . import pointnet2_utils as pu
        one = lambda t: t.unsqueeze(0)      # (the kernel's operands carry a leading pose dimension: T = 1 here)
        mo, tg, vtg = (None, one(self._targets), one(self._vtargets) if vert else None) if targets else (one(self._motions), None, None)
        pu.handle_set_rows(self.surface, self._labels, one(self.buf), mo, tg, tgt=one(self.surface_tgt), handle_out=self.surface_handle)
        if vert:
            pu.handle_set_rows(self.verts, self._vlabels, one(self._vrows), mo, vtg, tgt=one(self.verts_tgt),
                               handle_out=self.verts_handle)
        return self._network(self.buf, self.geometry, self.verts2cano, self.surf2cano, self._surf_idx)

    def _rule_flags(self, verts, handle_out, move_out):
        """The rule kernel once on ``self.params`` as they stand, for its flags alone (labels_from_parts)."""
        import torch
        from . import pointnet2_utils as pu
        rule, src, bounds = (self.verts_rule, self.verts, self.verts_bounds) if verts else (self.surface_rule, self.surface, self.bounds)
        rows = torch.empty(tuple(src.shape[:2]) + (7,), dtype=torch.float32, device=src.device)      # (the kernel's required output)
        pu.handle_rows(rule, src, bounds, self.params, rows, handle_out=handle_out, move_out=move_out)

    # ------------------------------------------------------------------ T poses per call
    def _track_state(self, T):
        """What a track of T poses holds beside the session's own state, made at the first track of this T: the [T * B, S, 7]
        input rows (pose-major; columns 0:3 written here, once), the canonical coordinates repeated T times, network 2's index
        sets over those T * B rows -- searched once here on the repeated coordinates, which gives every copy its shape's sets --
        and the buffers of the targets.  Network 1 is not run: its outputs are the session's."""
        import torch
        from types import SimpleNamespace
        if T not in self._tracks:
            B, S, V = self.surface.shape[0], self.surface.shape[1], self.verts.shape[1]
            dev = self.verts.device
            st = SimpleNamespace(targets=None, vtargets=None)
            st.surf2cano = self.surf2cano.repeat(T, 1, 1).contiguous()
            st.verts2cano = st.surf2cano if self.same else self.verts2cano.repeat(T, 1, 1).contiguous()
            st.buf = torch.zeros((T * B, S, 7), dtype=torch.float32, device=dev)
            st.buf[:, :, 0:3] = st.surf2cano
            st.geometry = self.net.geometry(st.verts2cano, st.buf)
            st.surf_idx = None if self.same else self.net.decoder.geometry(st.surf2cano, st.geometry["encoder"]["anchors"])["query_idx"]
            st.motions = torch.empty((T, B, self._count, 12), dtype=torch.float32, device=dev)
            st.surface_tgt = torch.empty((T, B, S, 3), dtype=torch.float32, device=dev)
            if self.same:
                st.verts_tgt, st.vrows = st.surface_tgt, None
            else:
                st.verts_tgt = torch.empty((T, B, V, 3), dtype=torch.float32, device=dev)
                st.vrows = torch.empty((T, B, V, 7), dtype=torch.float32, device=dev)      # (the kernel's required output)
            self._tracks[T] = st
        return self._tracks[T]

    def _enqueue_track(self, T, targets, vert):
        from . import pointnet2_utils as pu
        st = self._tracks[T]
        B, S = self.surface.shape[0], self.surface.shape[1]
        mo, tg, vtg = (None, st.targets, st.vtargets if vert else None) if targets else (st.motions, None, None)
        pu.handle_set_rows(self.surface, self._labels, st.buf.view(T, B, S, 7), mo, tg, tgt=st.surface_tgt, handle_out=self.surface_handle)
        if vert:
            pu.handle_set_rows(self.verts, self._vlabels, st.vrows, mo, vtg, tgt=st.verts_tgt, handle_out=self.verts_handle)
        return self._network(st.buf, st.geometry, st.verts2cano, st.surf2cano, st.surf_idx)

    def track(self, motions=None, targets=None, vert_targets=None, with_inputs=False, clone=True, normals=False,
              self_intersections=False, render=None):
        """T poses of the labelled handle set in one call: ``motions`` [T, B, H, 12] or a list of T ``pack_motions`` inputs, or
        ``targets`` [T, B, n, 3] on the GPU (``vert_targets`` [T, B, V, 3] for the vertices of a separate cloud).  One launch of
        the labelled kernel writes the T * B input rows, network 2 runs once over them; a drag of a small mesh is bound by its
        launches, and here the same launches carry T times the rows.

        Returns ``verts_tgt_pred`` and ``verts_tgt`` [T, B, V, 3], ``surface_samples_tgt_pred`` [T, B, S, 3], the handle masks
        [B, .] (they do not depend on the pose) and with ``with_inputs`` ``surface_samples_inputs`` [T, B, S, 7]; with
        ``normals=True`` ``verts_tgt_normals`` [T, B, V, 3] -- the T * B poses in the same two launches; with
        ``self_intersections=True`` ``faces_tgt_hits`` [T, B, F], ``tgt_self_intersections`` and ``tgt_self_skipped`` [T, B];
        with ``render=RenderSpec(...)`` ``tgt_depth`` and ``tgt_face_image`` [T, B, K, H, W] and ``drag``'s other images.

        A track shares with the session network 1's outputs, the labels and the handle masks; its input rows, its index sets
        (those of the session's, over T * B rows) and its graphs -- one per (form, T) -- are its own and are made at the first
        track of a T.  Its predictions are network 2's on T * B rows: the dense layers pick their tiles by row count, so a pose
        of a track equals the same pose through ``pose`` to rounding, not bit for bit."""
        import numpy as np
        import torch
        from ._lib import on_device
        normals = self._normals_wanted("track", normals)
        selfint = self._selfint_wanted("track", self_intersections)
        render = self._render_wanted("track", render)
        vert = self._pose_checks("track", motions, targets, vert_targets)
        B, S, V, H = self.surface.shape[0], self.surface.shape[1], self.verts.shape[1], self._count
        if targets is not None:
            if not torch.is_tensor(targets) or targets.dim() != 4:
                raise ValueError(f"track: targets must be a float32 GPU tensor [T, {B}, {S}, 3]")
            T = int(targets.shape[0])
            self._session_tensor(targets, (T, B, S, 3), torch.float32, "track: targets")
            if vert:
                self._session_tensor(vert_targets, (T, B, V, 3), torch.float32, "track: vert_targets")
        elif isinstance(motions, np.ndarray) or hasattr(motions, "detach"):
            words = motions.detach().cpu().numpy() if hasattr(motions, "detach") else motions
            if words.ndim != 4 or tuple(words.shape[1:]) != (B, H, 12):
                raise ValueError(f"track: an array of motions must be [T, {B}, {H}, 12], got {tuple(words.shape)}")
            T = int(words.shape[0])
            words = np.ascontiguousarray(words, dtype=np.float32)
        else:
            poses = list(motions)
            T = len(poses)
            words = np.stack([pack_motions(B, H, m) for m in poses]) if T else None
        if T < 1:
            raise ValueError("track: at least one pose")
        if T * B > 65535:
            raise ValueError(self._refused + f"a track of T={T} poses of B={B} shapes: T * B must be at most 65535 (the labelled "
                             "kernel's grid)")
        with on_device(self.verts):
            st = self._track_state(T)
            if targets is None:
                st.motions.copy_(torch.from_numpy(words), non_blocking=True)
            else:
                for name, value in (("targets", targets), ("vtargets", vert_targets if vert else None)):
                    if value is not None:
                        if getattr(st, name) is None:
                            setattr(st, name, torch.empty_like(value, memory_format=torch.contiguous_format))
                        getattr(st, name).copy_(value, non_blocking=True)
            key = ("track", T, targets is not None, vert)
            pred = self._dispatch_normals(key, lambda: self._enqueue_track(*key[1:]), normals, lead=(T, B), selfint=selfint,
                                          render=render)
            own, own_pred = self._owners(clone)
            have_verts = self.same or vert
            out = {"verts_tgt_pred": own_pred(pred["verts_tgt_pred"]).view(T, B, V, 3)}
            out["surface_samples_tgt_pred"] = (out["verts_tgt_pred"] if self.same
                                               else own_pred(pred["surface_samples_tgt_pred"]).view(T, B, S, 3))
            out["verts_tgt"] = own(st.verts_tgt) if have_verts else None
            out["cano_handle_vert_idx"] = own(self.verts_handle).view(torch.bool) if have_verts else None
            out["cano_handle_sample_idx"] = (out["cano_handle_vert_idx"] if self.same
                                             else own(self.surface_handle).view(torch.bool))
            if with_inputs:
                out["surface_samples_inputs"] = torch.cat([self.surface.unsqueeze(0).expand(T, B, S, 3),
                                                           st.buf.view(T, B, S, 7)[..., 3:7]], dim=-1)
            return self._add_normals(out, pred, own_pred, (T, B, V, 3))

    def _result(self, pred, own, own_pred, have_verts, with_inputs):
        """``verts_tgt_pred`` [B, V, 3], ``surface_samples_tgt_pred`` [B, S, 3], ``verts_tgt``, ``cano_handle_vert_idx`` and
        ``cano_handle_sample_idx`` (bool), and with ``with_inputs`` the reference-shaped ``surface_samples_inputs`` [B, S, 7]
        = [src | mask * tgt | mask] (what test_on_batch_with_arbitrary and eval_metric take)."""
        import torch
        out = {"verts_tgt_pred": own_pred(pred["verts_tgt_pred"])}
        out["surface_samples_tgt_pred"] = (out["verts_tgt_pred"] if self.same
                                           else own_pred(pred["surface_samples_tgt_pred"]))
        out["verts_tgt"] = own(self.verts_tgt) if have_verts else None
        out["cano_handle_vert_idx"] = own(self.verts_handle).view(torch.bool) if have_verts else None
        out["cano_handle_sample_idx"] = (out["cano_handle_vert_idx"] if self.same
                                         else own(self.surface_handle).view(torch.bool))
        if with_inputs:
            out["surface_samples_inputs"] = torch.cat([self.surface, self.buf[:, :, 3:7]], dim=-1)
        return out


# ------------------------------------------------------------------------------------------- a packed batch of different meshes
def ragged_refusal(model, verts_src, surface=None, cano=None, surface_cano=None):
    """Why a RaggedEditSession cannot be opened on these arguments (None: it can), each reason named."""
    import torch
    from . import hip_decoder
    from .ragged import RaggedPoints
    nets = _networks_or_refusal(model)
    if isinstance(nets, str):
        return nets
    if not isinstance(verts_src, RaggedPoints):
        return (f"verts_src must be a RaggedPoints (B meshes packed), got {type(verts_src).__name__} -- EditSession takes a "
                "rectangular [B, V, 3] tensor")
    given = {"verts_src": verts_src, "surface": surface, "cano": cano, "surface_cano": surface_cano}
    for name, t in given.items():
        if (isinstance(t, RaggedPoints) or torch.is_tensor(t)) and not t.is_cuda:
            return f"CPU tensors: {name} is on the CPU -- the session's kernels have no CPU path"
    why = _network_refusal(nets[-1], ("geometry", "ragged_geometry"))
    if why is not None:
        return why
    for net in nets:      # (what encoding a packed cloud and decoding a packed query set refuse, by their own names)
        why = net.ragged_surface_refusal() if isinstance(surface, RaggedPoints) or surface is None else (
            hip_decoder.ragged_refusal(net.decoder) if hip_decoder.supported(net.decoder) else
            "decoder geometry: the packed vertices are decoded by the fused kernels, built for dim=200, hidden_dim=128, "
            "n_blocks=5, out_dim=3")
        if why is not None:
            return why
    B = verts_src.batch
    for name, t in given.items():
        if isinstance(t, RaggedPoints):
            if t.packed.dtype is not torch.float32 or t.packed.shape[1] != 3:
                return f"{name} must hold float32 [capacity, 3] rows, got {t.packed.dtype} {tuple(t.packed.shape)}"
        elif t is not None:
            if name == "cano":
                return f"{name} must be a RaggedPoints, got {type(t).__name__}"
            if not torch.is_tensor(t):
                return f"{name} must be a RaggedPoints or a torch.Tensor, got {type(t).__name__}"
            if t.dtype is not torch.float32 or t.dim() != 3 or t.shape[2] != 3:
                return f"{name} must be float32 [B, S, 3], got {t.dtype} {tuple(t.shape)}"
    if torch.is_tensor(surface) and surface.shape[0] != B:
        return f"surface holds {surface.shape[0]} shapes, verts_src {B}"
    if isinstance(surface, RaggedPoints) and surface.batch != B:
        return f"surface holds {surface.batch} shapes, verts_src {B}"
    if cano is not None and not verts_src.same_layout(cano):
        return f"cano ({cano!r}) is not over the same layout as verts_src ({verts_src!r})"
    if surface_cano is not None:
        if surface is None:
            return "surface_cano goes with a surface over the same layout"
        if isinstance(surface, RaggedPoints) != isinstance(surface_cano, RaggedPoints) or (
                not surface.same_layout(surface_cano) if isinstance(surface, RaggedPoints) else surface_cano.shape != surface.shape):
            return "surface_cano is not over the same layout as the surface"
    for name, t in (("verts_src", verts_src), ("surface", surface)):
        if isinstance(t, RaggedPoints):
            for b, n in enumerate(t.counts):
                if n == 0:
                    return f"an empty shape: shape {b} of {name} has no points"
    cloud = verts_src if surface is None else surface
    if isinstance(cloud, RaggedPoints):
        for net in nets:
            npoints, ks, _ = net.encoder._pyramid_args()
            tb = net.encoder.transformer_begin
            need = [(npoints[0], "points the first level samples")]
            need += [(k, "neighbours of " + what) for what, k in (("the first attention block", None if tb.group_all else tb.k),
                                                                  ("the first set abstraction", ks[0][0])) if k is not None]
            for b, n in enumerate(cloud.counts):
                for k, what in need:
                    if n < k:
                        return f"shape {b} of the cloud has {n} points, fewer than the {k} {what}"
    return None


class RaggedEditSession(_Session):
    """An EditSession over a PACKED batch of B meshes of different vertex counts (nsdp_amd.ragged) -- the reference's batch loop
    over its user-handle data set, where the cloud network 2 encodes is each mesh's own vertex set.  Opened once, it holds network
    1's outputs, network 2's index sets (Deformation_Networks.ragged_geometry) and the per-shape bounding boxes; a drag is one
    [B, 8] host-to-device copy, the packed handle kernel (include/nsdp_handles_ragged.h), network 2's encoder over the cached
    sets and one ragged decode (two with a separate cloud).  Nothing of a drag reads an offsets tensor back: the counts are the
    host's at open, so with ``graph=True`` the drags by rule replay one captured graph and the drags by masks a second.

    ``verts_src``: RaggedPoints [cap, 3] on the GPU.  ``surface``: None (the cloud is the vertex set), a RaggedPoints [scap, 3]
    of B clouds of different sample counts, or a rectangular [B, S, 3] tensor.  ``cano`` / ``surface_cano``: the coordinates the
    bounding-box rule is evaluated on, over the layouts of ``verts_src`` / ``surface`` (None: the source coordinates).

    ``faces``: a RaggedPoints of the meshes' triangles ([fcap, 3] int32 / int64 rows, indices local to their mesh) for
    ``verts_src_normals`` and ``normals=True``; the normals come back as RaggedPoints over the vertices' offsets.

    The predictions are bit-equal to the step function on the ragged data_dict the drag stands for
    (tests/test_edit_session_ragged_gpu.py).  Staleness: as for EditSession -- ``reopen()`` after the weights changed."""

    _refusal = staticmethod(ragged_refusal)
    _cached = ("geometry", "buf", "inputs", "_vert_idx")

    def _hold(self, verts_src, surface, cano, surface_cano):
        import torch
        from .ragged import RaggedPoints
        tight = lambda r: RaggedPoints(r.packed.contiguous(), r.offsets, r.counts)      # (the host counts: read once, here)
        self.verts = tight(verts_src)
        self.same = surface is None
        self.rect = torch.is_tensor(surface)
        self.surface = self.verts if self.same else (surface.contiguous() if self.rect else tight(surface))
        self.verts_rule = self.verts if cano is None else tight(cano)
        if surface_cano is None:
            self.surface_rule = self.verts_rule if self.same else self.surface
        else:
            self.surface_rule = surface_cano.contiguous() if self.rect else tight(surface_cano)

    def _over_verts(self, t):
        return self.verts.like(t)

    def _layout(self):
        cloud_rows = tuple(self.surface.shape[:2]) if self.rect else (self.surface.capacity,)
        return self.verts.batch, self.verts.packed, cloud_rows, (self.verts.capacity,)

    # ------------------------------------------------------------------ the cached state
    def _open(self):
        import torch
        from . import pointnet2_utils as pu
        with torch.no_grad():
            dev = self.verts.device
            verts, surface, net = self.verts, self.surface, self.net
            B, vcap = verts.batch, verts.capacity
            if self.flow:
                outs = self.model.canonicalize([surface] if self.same else [surface, verts], surface)
                self.surf2cano, self.verts2cano = outs[0], outs[-1]
            else:
                self.surf2cano, self.verts2cano = surface, verts
            # the deformation network's input rows: columns 0:3 written here, once; 3:7 by every drag's kernel
            if self.rect:
                S = surface.shape[1]
                self.buf = torch.zeros((B, S, 7), dtype=torch.float32, device=dev)
                self.buf[:, :, 0:3] = self.surf2cano
                self.inputs = self.buf
                self.geometry = {"encoder": net.encoder.geometry(self.buf)}      # (net.geometry's encoder part)
                anchors = self.geometry["encoder"]["anchors"]
                self.geometry["query_idx"] = net.decoder.geometry(self.surf2cano, anchors)["query_idx"]
                self.geometry["query_points"] = self.surf2cano
                self._vert_idx = net.query_geometry_ragged(self.verts2cano, anchors)["query_idx"]
                self.bounds = pu.handle_bounds(self.surface_rule)
                self.surface_tgt = torch.empty((B, S, 3), dtype=torch.float32, device=dev)
                self.surface_handle = torch.empty((B, S), dtype=torch.uint8, device=dev)
            else:
                scap, total = surface.capacity, surface.total
                self.buf = torch.zeros((scap, 7), dtype=torch.float32, device=dev)
                self.buf[:total, 0:3] = self.surf2cano.packed[:total]
                self.inputs = surface.like(self.buf)
                self.geometry = net.ragged_geometry(self.surf2cano, self.inputs)
                anchors = self.geometry["encoder"]["anchors"]
                self._vert_idx = (self.geometry["query_idx"] if self.same
                                  else net.query_geometry_ragged(self.verts2cano, anchors)["query_idx"])
                self.bounds = pu.handle_bounds_ragged(self.surface_rule.packed, surface.offsets, max(surface.counts))
                # (zeros: the padding rows, which no kernel writes, are handed out with the rest)
                self.surface_tgt = torch.zeros((scap, 3), dtype=torch.float32, device=dev)
                self.surface_handle = torch.zeros((scap,), dtype=torch.uint8, device=dev)
            self.params = torch.zeros((B, 8), dtype=torch.int32, device=dev)
            self._mask_h = self._mask_m = self._vmask_h = self._vmask_m = None      # (made by the first drag by masks)
            if self.same:
                self.verts_bounds, self.verts_tgt, self.verts_handle, self._vrows = self.bounds, self.surface_tgt, self.surface_handle, None
            else:
                self.verts_bounds = pu.handle_bounds_ragged(self.verts_rule.packed, verts.offsets, max(verts.counts))
                self.verts_tgt = torch.zeros((vcap, 3), dtype=torch.float32, device=dev)
                self.verts_handle = torch.zeros((vcap,), dtype=torch.uint8, device=dev)
                self._vrows = torch.empty((vcap, 7), dtype=torch.float32, device=dev)      # (the kernel's required output)
            self._open_normals()

    # ------------------------------------------------------------------ one drag
    def _enqueue(self, masks, vert_masks):
        """Everything of a drag that runs on the GPU behind the parameter copy: capturable, reads device tensors only."""
        from . import pointnet2_utils as pu
        hm, mm = (self._mask_h, self._mask_m) if masks else (None, None)
        if self.rect:
            pu.handle_rows(self.surface_rule, self.surface, self.bounds, self.params, self.buf, hm, mm, tgt=self.surface_tgt,
                           handle_out=self.surface_handle)
        else:
            pu.handle_rows_ragged(self.surface_rule.packed, self.surface.packed, self.surface.offsets, self.bounds, self.params,
                                  self.buf, hm, mm, tgt=self.surface_tgt, handle_out=self.surface_handle)
        if not self.same and (not masks or vert_masks):
            vh, vm = (self._vmask_h, self._vmask_m) if masks else (None, None)
            pu.handle_rows_ragged(self.verts_rule.packed, self.verts.packed, self.verts.offsets, self.verts_bounds, self.params,
                                  self._vrows, vh, vm, tgt=self.verts_tgt, handle_out=self.verts_handle)
        return self._network()

    def _network(self):
        """Network 2 over the input rows a handle kernel has just written: the encoder over the cached index sets and one ragged
        decode (two with a separate cloud)."""
        net = self.net
        if self.rect:
            enc = net.encode(self.buf, geometry=self.geometry)
        else:
            enc = net.encode(self.inputs, ragged_geometry=self.geometry)
        enc_v = dict(enc)
        enc_v["query_idx"], enc_v["query_points"] = self._vert_idx, self.verts2cano
        out = {"verts_tgt_pred": net.decode(self.verts2cano, enc_v).packed}
        if not self.same:
            pred = net.decode(self.surf2cano, enc)      # (its query_idx / query_points are the cloud's)
            out["surface_samples_tgt_pred"] = pred if self.rect else pred.packed
        return out

    def _enqueue_pose(self, targets, vert):
        """``_enqueue`` for a pose of the labelled handle set: the labelled kernels in place of the rule's."""
        from . import pointnet2_utils as pu
        mo, tg, vtg = (None, self._targets, self._vtargets if vert else None) if targets else (self._motions, None, None)
        if self.rect:
            one = lambda t: None if t is None else t.unsqueeze(0)      # (a leading pose dimension: T = 1)
            pu.handle_set_rows(self.surface, self._labels, one(self.buf), one(mo), one(tg), tgt=one(self.surface_tgt),
                               handle_out=self.surface_handle)
        else:
            pu.handle_set_rows_ragged(self.surface.packed, self.surface.offsets, self._labels, self.buf, mo, tg,
                                      tgt=self.surface_tgt, handle_out=self.surface_handle)
        if vert:
            pu.handle_set_rows_ragged(self.verts.packed, self.verts.offsets, self._vlabels, self._vrows, mo, vtg,
                                      tgt=self.verts_tgt, handle_out=self.verts_handle)
        return self._network()

    def _rule_flags(self, verts, handle_out, move_out):
        """The rule kernel once on ``self.params`` as they stand, for its flags alone (labels_from_parts)."""
        import torch
        from . import pointnet2_utils as pu
        if not verts and self.rect:
            rows = torch.empty(tuple(self.surface.shape[:2]) + (7,), dtype=torch.float32, device=self.surface.device)
            pu.handle_rows(self.surface_rule, self.surface, self.bounds, self.params, rows, handle_out=handle_out, move_out=move_out)
            return
        rule, src, bounds = (self.verts_rule, self.verts, self.verts_bounds) if verts else (self.surface_rule, self.surface, self.bounds)
        rows = torch.empty((src.capacity, 7), dtype=torch.float32, device=src.device)      # (the kernel's required output)
        pu.handle_rows_ragged(rule.packed, src.packed, src.offsets, bounds, self.params, rows, handle_out=handle_out, move_out=move_out)

    def track(self, *args, **kwargs):
        raise ValueError(self._refused + "a track over a packed session: the packed index sets name packed rows -- T poses would "
                         "need them rebuilt over T copies of the packed layout, which is not done here; call pose() per pose, or "
                         "track() on an EditSession per mesh")

    def _result(self, pred, own, own_pred, have_verts, with_inputs):
        """``verts_tgt_pred``, ``verts_tgt`` and ``cano_handle_vert_idx`` as RaggedPoints over the vertices' offsets (the handle
        as [cap, 1] bool rows), ``surface_samples_tgt_pred`` and ``cano_handle_sample_idx`` over the cloud's layout (the same
        objects when the cloud is the vertex set), and with ``with_inputs`` ``surface_samples_inputs``: a RaggedPoints of
        [scap, 7] rows (or [B, S, 7]) the step function takes as it is."""
        import torch
        over_cloud = (lambda t: t) if self.rect else self.surface.like
        out = {"verts_tgt_pred": self.verts.like(own_pred(pred["verts_tgt_pred"]))}
        out["surface_samples_tgt_pred"] = (out["verts_tgt_pred"] if self.same
                                           else over_cloud(own_pred(pred["surface_samples_tgt_pred"])))
        out["verts_tgt"] = self.verts.like(own(self.verts_tgt)) if have_verts else None
        out["cano_handle_vert_idx"] = self.verts.like(own(self.verts_handle).view(torch.bool).unsqueeze(-1)) if have_verts else None
        if self.same:
            out["cano_handle_sample_idx"] = out["cano_handle_vert_idx"]
        else:
            h = own(self.surface_handle).view(torch.bool)
            out["cano_handle_sample_idx"] = h if self.rect else self.surface.like(h.unsqueeze(-1))
        if with_inputs:
            if self.rect:
                out["surface_samples_inputs"] = torch.cat([self.surface, self.buf[:, :, 3:7]], dim=-1)
            else:
                out["surface_samples_inputs"] = self.surface.like(torch.cat([self.surface.packed, self.buf[:, 3:7]], dim=-1))
        return out


def reference_data_dict(verts_src, surface, spec_or_params, cano=None, surface_cano=None):
    """The data_dict one drag stands for, built with torch alone (the reference's cano_handle_user_define as array expressions):
    what the session's results are compared with.  ``spec_or_params``: a HandleSpec (the same drag for every shape) or the
    [B, 8] int32 array of pack_params."""
    import numpy as np
    import torch
    B = verts_src.shape[0]
    words = (pack_params(B, spec_or_params.part, spec_or_params.translation, spec_or_params.partial_range, spec_or_params.cliptail)
             if isinstance(spec_or_params, HandleSpec) else np.asarray(spec_or_params))
    dev = verts_src.device
    part = torch.from_numpy(words[:, 0].copy()).to(dev).view(B, 1)
    clip = torch.from_numpy(words[:, 1].copy() != 0).to(dev).view(B, 1)
    f = torch.from_numpy(words.view(np.float32).copy()).to(dev)
    r, d = f[:, 2:3], f[:, None, 3:6]

    def one(src, rule):
        rule = src if rule is None else rule
        lo, hi = rule.amin(dim=1), rule.amax(dim=1)
        x, y, z = rule[:, :, 0], rule[:, :, 1], rule[:, :, 2]
        head = y < lo[:, 1:2] + r
        tail = y > hi[:, 1:2] - r
        tail = torch.where(clip, tail & (z > -r), tail)
        foot = z < lo[:, 2:3] + r
        handle = head | tail | foot
        left, right, front, behind = foot & (x > 0), foot & (x < 0), foot & (y < 0), foot & (y > 0)
        regions = (head, tail, left & front, right & front, left & behind, right & behind)
        move = torch.zeros_like(head)
        for i, reg in enumerate(regions):
            move = torch.where(part == i, reg, move)
        tgt = src + d * move[:, :, None].float()
        return handle, tgt

    vh, vt = one(verts_src, cano)
    sh, st = (vh, vt) if surface is None else one(surface, surface_cano)
    surf = surface if surface is not None else verts_src
    maskf = sh[:, :, None].float()
    return {"surface_samples_inputs": torch.cat([surf, st * maskf, maskf], dim=-1).contiguous(),
            "surface_samples_src": surf.contiguous(), "verts_src": verts_src.contiguous(), "verts_tgt": vt,
            "cano_handle_vert_idx": vh, "cano_handle_sample_idx": sh}


def reference_pose_dict(verts_src, surface, labels, count, motions=None, targets=None, vert_labels=None, vert_targets=None):
    """The data_dict one pose of a labelled handle set stands for, built with torch alone, what ``pose`` and the labelled kernels
    are compared with: per coordinate ((M0 * x + M1 * y) + M2 * z) + M3 as SEPARATE multiplications and additions in the order of
    include/nsdp_handle_sets.h (no addcmul, no matmul: each would round elsewhere), free points copied.  ``labels`` [B, n] uint8
    over the cloud (``surface``, or the vertices when it is None), ``vert_labels`` [B, V] for the vertices of a separate cloud
    (without them ``verts_tgt`` and ``cano_handle_vert_idx`` are None); ``motions``: anything ``pack_motions`` takes, or
    ``targets`` [B, n, 3] (``vert_targets`` [B, V, 3])."""
    import torch
    if (motions is None) == (targets is None):
        raise ValueError(f"reference_pose_dict: exactly one of motions and targets (got {'neither' if motions is None else 'both'})")
    B, dev = verts_src.shape[0], verts_src.device
    table = None if motions is None else torch.from_numpy(pack_motions(B, count, motions)).to(dev)

    def one(src, lab, tgt_given):
        if table is None:
            handle = lab != 0
            moved = tgt_given
        else:
            handle = (lab >= 1) & (lab <= count)
            pick = (lab.long() - 1).clamp(0, count - 1)                                  # (a free point's pick is not used)
            M = torch.gather(table, 1, pick[:, :, None].expand(B, lab.shape[1], 12))      # [B, n, 12]: a copy of the rows
            x, y, z = src[:, :, 0], src[:, :, 1], src[:, :, 2]
            cols = []
            for c in range(3):
                acc = M[:, :, 4 * c] * x
                acc = acc + M[:, :, 4 * c + 1] * y
                acc = acc + M[:, :, 4 * c + 2] * z
                cols.append(acc + M[:, :, 4 * c + 3])
            moved = torch.stack(cols, dim=-1)
        return handle, torch.where(handle[:, :, None], moved, src)

    same = surface is None
    surf = verts_src if same else surface
    sh, st = one(surf, labels, targets)
    if same:
        vh, vt = sh, st
    elif vert_labels is not None and (targets is None or vert_targets is not None):
        vh, vt = one(verts_src, vert_labels, vert_targets)
    else:
        vh = vt = None
    maskf = sh[:, :, None].float()
    return {"surface_samples_inputs": torch.cat([surf, st * maskf, maskf], dim=-1).contiguous(),
            "surface_samples_src": surf.contiguous(), "verts_src": verts_src.contiguous(), "verts_tgt": vt,
            "cano_handle_vert_idx": vh, "cano_handle_sample_idx": sh}


# ---------------------------------------------------------------------------------------------------------------- the tool
def build_parser():
    ap = argparse.ArgumentParser(description="Drag handles on a (synthetic) mesh through an editing session, timed")
    ap.add_argument("config_file")
    ap.add_argument("--vertices", type=int, default=25000, help="mesh vertices per shape (default 25000)")
    ap.add_argument("--surface", type=int, default=None,
                    help="samples of a separate surface cloud (default: none -- the cloud is the vertex set, as in the "
                         "reference's user-handle data set)")
    ap.add_argument("--batch", type=int, default=None, help="shapes per call (default: the config's test.batch_size, else 1)")
    ap.add_argument("--vertex-counts", default=None, metavar="n1,n2,...",
                    help="a packed batch of meshes of these vertex counts through a RaggedEditSession (replaces --vertices and "
                         "--batch; the cloud is the vertex set unless --surface-counts or --surface is given)")
    ap.add_argument("--surface-counts", default=None, metavar="s1,s2,...",
                    help="with --vertex-counts: a separate packed cloud of these sample counts, one per mesh")
    ap.add_argument("--part", default=None, choices=PARTS, help="the region that moves (default: the config's data.userhandle)")
    ap.add_argument("--translate", default=None, metavar="dx,dy,dz",
                    help="its translation (default: the config's xtrans, ytrans, ztrans)")
    ap.add_argument("--handles", default=None, metavar="p1,p2,...",
                    help="a labelled handle set from these parts of the rule (labels_from_parts): the first takes --rotate-deg "
                         "about its own centroid plus --translate, the others are pinned, through pose() -- or track() with --track")
    ap.add_argument("--rotate-deg", type=float, default=0.0, help="with --handles: the first handle's rotation in degrees")
    ap.add_argument("--axis", default="0,0,1", metavar="ax,ay,az", help="with --handles: the rotation's axis (default 0,0,1)")
    ap.add_argument("--track", type=int, default=None, metavar="T",
                    help="with --handles: T poses per call, pose i the motion scaled by (i + 1) / T")
    ap.add_argument("--drags", type=int, default=10, help="timed drags (each with another translation)")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--graph", action="store_true", help="capture the drag once and replay it")
    ap.add_argument("--normals", action="store_true",
                    help="drag a latitude-longitude sphere (synth.sphere_mesh) of at most --vertices vertices (every count of "
                         "--vertex-counts) and time the drag with and without the deformed mesh's vertex normals")
    ap.add_argument("--self-intersections", action="store_true", dest="self_intersections",
                    help="drag the sphere mesh of --normals and print, per drag, the intersecting face pairs of every deformed "
                         "mesh (self_intersections=True), and the drag's time with them")
    ap.add_argument("--pick", default=None, metavar="ox,oy,oz,dx,dy,dz",
                    help="drag the sphere mesh of --normals and print what the ray from (ox, oy, oz) along (dx, dy, dz) picks -- t, "
                         "face, barycentric weights, vertex -- on the source mesh and on the last drag's prediction (pick())")
    ap.add_argument("--brush", action="append", default=None, metavar="ox,oy,oz,dx,dy,dz,radius",
                    help="(repeatable) on the sphere mesh of --normals: pick the vertex the ray from (ox, oy, oz) along (dx, dy, dz) "
                         "meets and brush a handle of that geodesic radius around it (labels_from_brush); the handles are set and "
                         "posed -- the first by --rotate-deg about its centroid plus --translate, the others pinned")
    ap.add_argument("--render", default=None, metavar="OUT.png",
                    help="drag the sphere mesh of --normals with a preview (render=RenderSpec: one fitted view of every deformed "
                         "mesh, rasterised behind the decode) and write the first mesh's shaded image of the last drag as a PNG")
    ap.add_argument("--render-size", type=int, default=512, dest="render_size", metavar="S", help="the preview is S x S pixels")
    ap.add_argument("--weight_file", default=None, help="weights of the whole model (default: procedural weights)")
    ap.add_argument("--out", default=None, help="directory for the last drag's predictions (<key>.npy)")
    return ap


def spec_from_args(args, config):
    """The drag of the command line: --part / --translate over the config's data.userhandle; without either, head by
    (-0.15, -0.2, -0.2) -- config/tosca/head.yaml's."""
    data = config.get("data") or {}
    base = HandleSpec.from_config(data) if isinstance(data.get("userhandle"), dict) and any(data["userhandle"].get(p) for p in PARTS) \
        else HandleSpec("head", (-0.15, -0.2, -0.2), float(data.get("partial_range", 0.1)),
                        bool((data.get("userhandle") or {}).get("cliptail", False)))
    part = args.part or base.part
    translation = base.translation
    if args.translate is not None:
        try:
            translation = tuple(float(v) for v in args.translate.split(","))
        except ValueError:
            translation = ()
        if len(translation) != 3:
            sys.exit(f"nsdp_amd.edit: --translate wants dx,dy,dz, got {args.translate!r}")
    return HandleSpec(part, translation, base.partial_range, base.cliptail)


def counts_from_args(args):
    """(--vertex-counts, --surface-counts) as lists of positive integers, (None, None) without --vertex-counts."""
    def numbers(text, flag):
        try:
            vals = [int(v) for v in text.split(",")]
        except ValueError:
            vals = []
        if not vals or min(vals) < 1:
            sys.exit(f"nsdp_amd.edit: {flag} wants positive integers n1,n2,..., got {text!r}")
        return vals
    if args.vertex_counts is None:
        if args.surface_counts is not None:
            sys.exit("nsdp_amd.edit: --surface-counts goes with --vertex-counts")
        return None, None
    verts = numbers(args.vertex_counts, "--vertex-counts")
    surf = None if args.surface_counts is None else numbers(args.surface_counts, "--surface-counts")
    if surf is not None and (len(surf) != len(verts) or args.surface is not None):
        sys.exit("nsdp_amd.edit: --surface-counts wants one count per mesh of --vertex-counts, and not --surface beside it")
    return verts, surf


def sphere_for(vertices):
    """(verts float32 (V, 3), faces int32 (F, 3)) of the synth.sphere_mesh with the most vertices V = rings * segments + 2 <=
    ``vertices`` among those with about twice as many segments as rings."""
    import numpy as np
    from . import synth
    if vertices < 8:
        sys.exit(f"nsdp_amd.edit: --normals wants at least 8 vertices per mesh, got {vertices}")
    segments = max(int(np.sqrt(2.0 * (vertices - 2))), 3)
    rings = max((vertices - 2) // segments, 2)
    verts, faces = synth.sphere_mesh(rings, segments)
    return verts.astype(np.float32), faces


def _setup(args, smallest_cloud):
    """What both forms of the command line do first: the thread cap, the GPU, the config and its drag, the pyramid cut to the
    smallest cloud, the model (procedural weights without --weight_file) -- and the two helpers of the timed windows."""
    from .cpu_budget import cap_thread_pools
    cap_thread_pools(16)
    import torch
    if not torch.cuda.is_available():
        sys.exit("nsdp_amd.edit: needs a GPU (the session has no CPU path)")
    device = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    from . import synth
    from .config import load_config
    from .infer import _pyramid
    from .model import build_model
    config = load_config(args.config_file)
    spec = spec_from_args(args, config)
    _pyramid(config, smallest_cloud)
    model, _, _, test_fn = build_model(config, weight_file=args.weight_file, device="cpu")
    if args.weight_file is None:
        state = synth.procedural_state_dict(model.state_dict(), SEED_WEIGHTS)
        model.load_state_dict({k: torch.from_numpy(v) for k, v in state.items()})
    model.to(device).eval()

    def timed(fn, n=1):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for i in range(n):
            fn(i)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / max(1, n)

    def translation(i):      # (another drag every time: nothing of a previous one can be reused)
        return tuple(v * (1.0 + 0.01 * i) for v in spec.translation)

    return device, config, spec, model, test_fn, timed, translation


def _timed_with_normals(args, session, spec, translation, timed, warm):
    """--normals: the same drags with ``normals=True`` (--graph: a graph of its own, captured by the first of them); None without."""
    if not args.normals:
        return None
    for i in range(warm):
        session.drag(spec.part, translation(i), normals=True)
    return timed(lambda i: session.drag(spec.part, translation(i), clone=False, normals=True), args.drags)


def _timed_with_render(args, session, verts, spec, translation, timed, warm, ms_drag):
    """--render: the same drags with ``render=RenderSpec(...)`` (--graph: a graph of its own), the camera fitted to the first
    drag's prediction (one host read, before the timed drags), the last drag's first image written as a PNG -> the JSON fields;
    {} without."""
    if not args.render:
        return {}
    from .rasterize import Camera, write_png
    size = args.render_size
    view = RenderSpec(Camera.fit(session.drag(spec.part, translation(0))["verts_tgt_pred"], (0.3, -0.2, 1.0), size, size), size, size)
    for i in range(warm):
        session.drag(spec.part, translation(i), render=view)
    ms = timed(lambda i: session.drag(spec.part, translation(i), clone=False, render=view), args.drags)
    out = session.drag(spec.part, translation(args.drags - 1), render=view)
    image = out["tgt_image"].reshape((-1, size, size, 3))[0]
    write_png(args.render, image)
    return {"render": args.render, "render_size": size, "ms_per_drag_render": round(ms, 4), "render_ms": round(ms - ms_drag, 4),
            "render_over_drag": round(ms / ms_drag, 4) if ms_drag > 0 else None,
            "render_covered": int((out["tgt_face_image"] >= 0).sum()), "render_dropped": int(out["tgt_dropped"].sum())}


def _timed_with_self_intersections(args, session, spec, translation, timed, warm):
    """--self-intersections: the same drags with ``self_intersections=True`` (--graph: a graph of its own) -> the JSON fields:
    the time, and per drag the intersecting pairs, the faces with a hit and the faces the work guard skipped of every mesh."""
    import torch
    if not args.self_intersections:
        return {}
    for i in range(warm):
        session.drag(spec.part, translation(i), self_intersections=True)
    ms = timed(lambda i: session.drag(spec.part, translation(i), clone=False, self_intersections=True), args.drags)
    rows = []
    for i in range(args.drags):
        out = session.drag(spec.part, translation(i), self_intersections=True)
        rows.append(torch.stack([out["tgt_self_intersections"].reshape(-1), out["tgt_self_skipped"].reshape(-1).long()]))
    counts = torch.stack(rows).tolist()      # (one read for all drags)
    for i, (pairs, skipped) in enumerate(counts):
        print(f"drag {i}: self-intersecting face pairs per mesh {pairs}, faces skipped by the guard {skipped}", flush=True)
    return {"self_intersections": True, "ms_per_drag_self_intersections": round(ms, 4),
            "self_intersection_pairs": [c[0] for c in counts], "self_intersection_skipped": [c[1] for c in counts]}


def pick_from_args(args):
    """--pick ox,oy,oz,dx,dy,dz -> the six numbers (None without the flag)."""
    if args.pick is None:
        return None
    try:
        ray = [float(x) for x in args.pick.split(",")]
    except ValueError:
        ray = []
    if len(ray) != 6:
        sys.exit(f"nsdp_amd.edit: --pick wants six numbers ox,oy,oz,dx,dy,dz, got {args.pick!r}")
    return ray


def _picked(ray, session, out, batch, device, timed, drags):
    """--pick: the ray against the source mesh and against the last drag's prediction, printed -> the JSON fields (with the
    time of one pick against the prediction: a call of its own beside the drag)."""
    import torch
    if ray is None:
        return {}
    o = torch.tensor(ray[:3], dtype=torch.float32, device=device).expand(batch, 1, 3).contiguous()
    d = torch.tensor(ray[3:], dtype=torch.float32, device=device).expand(batch, 1, 3).contiguous()
    fields = {"pick_ray": ray}
    for name, verts in (("source", None), ("prediction", out["verts_tgt_pred"])):
        r = session.pick(o, d, verts)
        row = torch.cat([r["t"].double(), r["face"].double(), r["vertex"].double(), r["bary"][:, 0].double()], dim=1).tolist()
        for b, (t, face, vertex, b0, b1, b2) in enumerate(row):
            hit = f"t {t:.6g}  face {int(face)}  bary ({b0:.4f}, {b1:.4f}, {b2:.4f})  vertex {int(vertex)}" if face >= 0 else "no hit"
            print(f"pick on the {name} mesh, shape {b}: {hit}", flush=True)
        fields["pick_" + name] = [{"t": t if face >= 0 else None, "face": int(face), "vertex": int(vertex), "bary": [b0, b1, b2]}
                                  for t, face, vertex, b0, b1, b2 in row]
    fields["ms_per_pick"] = round(timed(lambda i: session.pick(o, d, out["verts_tgt_pred"]), drags), 4)
    return fields


def brushes_from_args(args):
    """--brush ox,oy,oz,dx,dy,dz,radius (repeatable) -> a list of seven numbers per brush (None without the flag)."""
    if not args.brush:
        return None
    out = []
    for text in args.brush:
        try:
            row = [float(x) for x in text.split(",")]
        except ValueError:
            row = []
        if len(row) != 7 or not row[6] >= 0.0:
            sys.exit(f"nsdp_amd.edit: --brush wants seven numbers ox,oy,oz,dx,dy,dz,radius with radius >= 0, got {text!r}")
        out.append(row)
    if len(out) > 255:
        sys.exit("nsdp_amd.edit: at most 255 --brush handles (the labels are bytes)")
    return out


def _brushed(brushes, session, args, spec, batch, device, timed):
    """--brush: every ray picked on the source mesh, a handle brushed around each picked vertex, the handles set and posed
    -- the size of each handle, the rounds and the milliseconds printed -> the JSON fields."""
    import numpy as np
    import torch
    if brushes is None:
        return {}
    strokes = []
    for row in brushes:
        o = torch.tensor(row[:3], dtype=torch.float32, device=device).expand(batch, 1, 3).contiguous()
        d = torch.tensor(row[3:6], dtype=torch.float32, device=device).expand(batch, 1, 3).contiguous()
        strokes.append((session.pick(o, d)["vertex"], row[6]))
    session.labels_from_brush(strokes)      # (the first brush makes the plan)
    box = {}
    ms_brush = timed(lambda i: box.update(r=session.labels_from_brush(strokes)), args.drags)
    labels, count = box["r"]
    stats = list(session.brush_stats)
    vlabels = None if session.same else session.labels_from_brush(strokes, verts=True)[0]
    session.set_handles(labels, count, vlabels)
    own = labels if vlabels is None else vlabels
    sizes = torch.stack([(own == h + 1).sum(dim=1) for h in range(count)], dim=1)                        # [B, count]
    first = (own == 1)[:, :, None].double()
    pivots = (session.verts.double() * first).sum(dim=1) / first.sum(dim=1).clamp(min=1.0)
    seeds = torch.stack([s[0].reshape(batch, -1)[:, 0] for s in strokes], dim=1)
    sizes, pivots, seeds = sizes.tolist(), pivots.cpu().numpy(), seeds.tolist()                            # (set-up reads)
    try:
        axis = tuple(float(v) for v in args.axis.split(","))
    except ValueError:
        axis = ()
    if len(axis) != 3 or not any(axis):
        sys.exit(f"nsdp_amd.edit: --axis wants a non-zero ax,ay,az, got {args.axis!r}")
    motions = [[Motion.rotate(axis, args.rotate_deg, pivot=pivots[b]).then(Motion.translate(np.asarray(spec.translation, np.float64)))]
               + [Motion.identity()] * (count - 1) for b in range(batch)]
    for _ in range(max(args.warmup, 1)):
        session.pose(motions)
    ms_pose = timed(lambda i: session.pose(motions, clone=False), args.drags)
    for b in range(batch):
        for h in range(count):
            print(f"brush {h} on shape {b}: vertex {seeds[b][h]}, radius {brushes[h][6]:g}: {sizes[b][h]} points, "
                  f"{stats[h]['rounds']} rounds in {stats[h]['calls']} calls", flush=True)
    print(f"{count} brush(es): {ms_brush:.3f} ms; a pose of the brushed handles: {ms_pose:.3f} ms", flush=True)
    return {"brushes": brushes, "brush_vertices": seeds, "brush_handle_sizes": sizes, "brush_rounds": [s["rounds"] for s in stats],
            "brush_calls": [s["calls"] for s in stats], "ms_per_brush_set": round(ms_brush, 4), "ms_per_brushed_pose": round(ms_pose, 4)}


def _normals_fields(ms_drag, ms_normals, faces):
    return {"normals": True, "faces": faces, "ms_per_drag_normals": round(ms_normals, 4),
            "normals_ms": round(ms_normals - ms_drag, 4), "normals_over_drag": round(ms_normals / ms_drag, 4) if ms_drag > 0 else None}


def main_ragged(args, vertex_counts, surface_counts):
    """--vertex-counts: the packed session on synthetic meshes, timed against the parent's two alternatives -- the ragged step
    function per drag, and one batch-1 EditSession per mesh dragged in turn."""
    B = len(vertex_counts)
    spheres = [sphere_for(n) for n in vertex_counts] if args.normals or args.self_intersections else None
    if spheres is not None:
        vertex_counts = [int(v.shape[0]) for v, _ in spheres]
    cloud_counts = surface_counts or ([args.surface] * B if args.surface else vertex_counts)
    device, config, spec, model, test_fn, timed, translation = _setup(args, min(cloud_counts))
    import numpy as np
    import torch
    from . import pointnet2_utils, synth
    from .infer import _checksum
    from .ragged import RaggedPoints
    if spheres is None:
        meshes = [torch.from_numpy(synth.uniform(SEED_DATA + b, "mesh_verts", (1, n, 3), -0.5, 0.5)).to(device)
                  for b, n in enumerate(vertex_counts)]
    else:
        meshes = [torch.from_numpy(v)[None].to(device) for v, _ in spheres]
    verts = RaggedPoints.from_list([m[0] for m in meshes])
    faces = None if spheres is None else RaggedPoints.from_rows([torch.from_numpy(f).to(device) for _, f in spheres])
    clouds, surface = None, None
    if surface_counts is not None:
        clouds = [torch.from_numpy(synth.uniform(SEED_DATA + b, "mesh_surface", (1, n, 3), -0.5, 0.5)).to(device)
                  for b, n in enumerate(surface_counts)]
        surface = RaggedPoints.from_list([c[0] for c in clouds])
    elif args.surface is not None:
        clouds = [torch.from_numpy(synth.uniform(SEED_DATA + b, "mesh_surface", (1, args.surface, 3), -0.5, 0.5)).to(device)
                  for b in range(B)]
        surface = torch.cat(clouds, dim=0)

    warm = max(args.warmup, 1)
    with torch.no_grad():
        box = {}
        timed(lambda i: box.update(s=RaggedEditSession(model, verts, surface, partial_range=spec.partial_range,
                                                       cliptail=spec.cliptail, graph=args.graph, faces=faces)))      # (also packs the weights)
        session = box["s"]
        ms_open = timed(lambda i: session.reopen())
        out = {}
        for i in range(warm):      # (--graph: the first drag captures)
            session.drag(spec.part, translation(i))
        ms_drag = timed(lambda i: out.update(session.drag(spec.part, translation(i), clone=False)), args.drags)
        ms_normals = _timed_with_normals(args, session, spec, translation, timed, warm)
        selfint_fields = _timed_with_self_intersections(args, session, spec, translation, timed, warm)
        out = session.drag(spec.part, translation(args.drags - 1), with_inputs=True)
        inputs = out["surface_samples_inputs"]
        dd = {"surface_samples_inputs": inputs, "verts_src": verts,
              "surface_samples_src": inputs.columns(0, 3) if isinstance(inputs, RaggedPoints) else inputs[:, :, 0:3].contiguous()}
        for _ in range(warm):
            test_fn(model, dict(dd), config)
        full = {}
        ms_full = timed(lambda i: full.update(test_fn(model, dict(dd), config)[1]), args.drags)
        packed = lambda t: t.packed if isinstance(t, RaggedPoints) else t
        equal = all(torch.equal(packed(out[k]), packed(full[k])) for k in ("verts_tgt_pred", "surface_samples_tgt_pred"))
        # the parent's other alternative: one batch-1 session per mesh, dragged in turn
        singles = [EditSession(model, m, None if clouds is None else clouds[b], partial_range=spec.partial_range,
                               cliptail=spec.cliptail, graph=args.graph) for b, m in enumerate(meshes)]
        for i in range(warm):
            for s1 in singles:
                s1.drag(spec.part, translation(i))
        ms_singles = timed(lambda i: [s1.drag(spec.part, translation(i), clone=False) for s1 in singles], args.drags)
        for s1 in singles:
            s1.close()
        pointnet2_utils.check_fps_cluster()
    if args.out:
        os.makedirs(args.out, exist_ok=True)
        for k in ("verts_tgt_pred", "surface_samples_tgt_pred", "verts_tgt"):
            np.save(os.path.join(args.out, k + ".npy"), packed(out[k]).cpu().numpy())
    line = {"metric": "edit_session_ragged", "model_type": config["model"]["type"], "graph": bool(args.graph), "batch": B,
            "vertex_counts": vertex_counts, "surface_counts": surface_counts, "surface": args.surface,
            "cloud_is_vertex_set": surface is None, "part": spec.part, "translation": list(spec.translation),
            "partial_range": spec.partial_range, "cliptail": spec.cliptail, "drags": args.drags, "warmup": args.warmup,
            "handle_points": int(packed(out["cano_handle_sample_idx"]).sum()),
            "ms_per_drag": round(ms_drag, 4), "ms_open": round(ms_open, 4), "ms_full_call": round(ms_full, 4),
            "ms_per_mesh_sessions": round(ms_singles, 4),
            "full_call_over_drag": round(ms_full / ms_drag, 3) if ms_drag > 0 else None,
            "per_mesh_sessions_over_drag": round(ms_singles / ms_drag, 3) if ms_drag > 0 else None,
            "replays": session.replays, "eager_calls": session.eager_calls, "equal_to_full_call": bool(equal),
            "checksum": _checksum(packed(out["verts_tgt_pred"]))}
    if args.normals:
        line.update(_normals_fields(ms_drag, ms_normals, sum(int(f.shape[0]) for _, f in spheres)))
    line.update(selfint_fields)
    print(json.dumps(line), flush=True)
    session.close()
    return 0


def handles_from_args(args):
    """(--handles as a list of part names, --axis as three floats); (None, None) without --handles."""
    if args.handles is None:
        if args.track is not None or (args.rotate_deg and not args.brush):
            sys.exit("nsdp_amd.edit: --track and --rotate-deg go with --handles (--rotate-deg with --brush too)")
        return None, None
    names = [p for p in args.handles.split(",") if p]
    if not names or any(p not in PARTS for p in names) or len(set(names)) != len(names):
        sys.exit(f"nsdp_amd.edit: --handles wants distinct names of {PARTS}, got {args.handles!r}")
    try:
        axis = tuple(float(v) for v in args.axis.split(","))
    except ValueError:
        axis = ()
    if len(axis) != 3 or not any(axis):
        sys.exit(f"nsdp_amd.edit: --axis wants a non-zero ax,ay,az, got {args.axis!r}")
    if args.track is not None and args.track < 1:
        sys.exit("nsdp_amd.edit: --track wants a positive integer")
    return names, axis


def main_handles(args, names, axis):
    """--handles: a labelled handle set from the rule's parts, the first handle rotated about its own centroid and translated,
    the others pinned -- one pose per call, or with --track T poses per call (pose i: the motion scaled by (i + 1) / T)."""
    device, config, spec, model, test_fn, timed, translation = _setup(args, args.surface or args.vertices)
    import numpy as np
    import torch
    from . import pointnet2_utils, synth
    from .infer import _checksum
    from .model.deformation_networks import test_on_batch_with_cano
    batch = args.batch or int((config.get("test") or {}).get("batch_size", 1) or 1)
    verts = torch.from_numpy(synth.uniform(SEED_DATA, "mesh_verts", (batch, args.vertices, 3), -0.5, 0.5)).to(device)
    surface = None if args.surface is None else \
        torch.from_numpy(synth.uniform(SEED_DATA, "mesh_surface", (batch, args.surface, 3), -0.5, 0.5)).to(device)
    T = args.track
    with torch.no_grad():
        session = EditSession(model, verts, surface, partial_range=spec.partial_range, cliptail=spec.cliptail, graph=args.graph)
        labels, count = session.labels_from_parts(names)
        session.set_handles(labels, count, None if surface is None else session.labels_from_parts(names, verts=True)[0])
        cloud = verts if surface is None else surface
        first = (labels == 1)[:, :, None].double()
        pivots = ((cloud.double() * first).sum(dim=1) / first.sum(dim=1).clamp(min=1.0)).cpu().numpy()      # [B, 3], set-up

        def motions(scale, i=0):
            d = np.asarray(translation(i), dtype=np.float64) * scale
            return [[Motion.rotate(axis, args.rotate_deg * scale, pivot=pivots[b]).then(Motion.translate(d))]
                    + [Motion.identity()] * (count - 1) for b in range(batch)]

        def call(i, **kw):
            if T is None:
                return session.pose(motions(1.0, i), **kw)
            return session.track([motions((t + 1) / T, i) for t in range(T)], **kw)

        for i in range(max(args.warmup, 1)):      # (--graph: the first call captures)
            call(i)
        out = {}
        ms_call = timed(lambda i: out.update(call(i, clone=False)), args.drags)
        out = call(args.drags - 1, with_inputs=True)
        inputs = out["surface_samples_inputs"]
        if T is None:
            dd = {"surface_samples_inputs": inputs, "verts_src": verts, "surface_samples_src": inputs[:, :, 0:3].contiguous()}
            full = test_fn(model, dd, config)[1]
        else:      # a track is network 2 over T * B rows: its own step function on those rows and network 1's cached outputs
            rows = torch.cat([session.surf2cano.repeat(T, 1, 1), inputs[..., 3:7].reshape(T * batch, -1, 4)], dim=-1).contiguous()
            dd = {"surface_samples_inputs": rows, "surface_samples_src": rows[:, :, 0:3].contiguous(),
                  "verts_src": session.verts2cano.repeat(T, 1, 1).contiguous()}
            full = test_on_batch_with_cano(session.net, dd, config)[1]
        equal = all(torch.equal(out[k].reshape(full[k].shape), full[k]) for k in ("verts_tgt_pred", "surface_samples_tgt_pred"))
        pointnet2_utils.check_fps_cluster()
    if args.out:
        os.makedirs(args.out, exist_ok=True)
        for k in ("verts_tgt_pred", "surface_samples_tgt_pred", "verts_tgt"):
            np.save(os.path.join(args.out, k + ".npy"), out[k].cpu().numpy())
    poses = T or 1
    line = {"metric": "edit_session_handle_sets", "model_type": config["model"]["type"], "graph": bool(args.graph), "batch": batch,
            "vertices": args.vertices, "surface": args.surface, "cloud_is_vertex_set": surface is None, "handles": names,
            "labels": count, "rotate_deg": args.rotate_deg, "axis": list(axis), "translation": list(spec.translation),
            "track": T, "partial_range": spec.partial_range, "cliptail": spec.cliptail, "drags": args.drags, "warmup": args.warmup,
            "handle_points": int(out["cano_handle_sample_idx"].sum()), "ms_per_call": round(ms_call, 4),
            "ms_per_pose": round(ms_call / poses, 4), "replays": session.replays, "eager_calls": session.eager_calls,
            "equal_to_full_call": bool(equal), "checksum": _checksum(out["verts_tgt_pred"])}
    print(json.dumps(line), flush=True)
    session.close()
    return 0


def main(argv=None):
    args = build_parser().parse_args(list(sys.argv[1:] if argv is None else argv))
    brushes = brushes_from_args(args)
    vertex_counts, surface_counts = counts_from_args(args)
    names, axis = handles_from_args(args)
    if names is not None:
        if args.normals:
            sys.exit("nsdp_amd.edit: --normals times drags by rule (--part), not --handles")
        if args.self_intersections:
            sys.exit("nsdp_amd.edit: --self-intersections times drags by rule (--part), not --handles")
        if args.pick is not None:
            sys.exit("nsdp_amd.edit: --pick goes with drags by rule (--part), not --handles")
        if args.render:
            sys.exit("nsdp_amd.edit: --render goes with drags by rule (--part), not --handles")
        if brushes is not None:
            sys.exit("nsdp_amd.edit: --brush makes its own handles: not with --handles")
        if vertex_counts is not None:
            sys.exit("nsdp_amd.edit: --handles goes with --vertices / --batch, not with --vertex-counts")
        if args.vertices < 1 or (args.surface is not None and args.surface < 1) or args.drags < 1:
            sys.exit("nsdp_amd.edit: --vertices, --surface and --drags want positive integers")
        return main_handles(args, names, axis)
    if vertex_counts is not None:
        if (args.surface is not None and args.surface < 1) or args.drags < 1:
            sys.exit("nsdp_amd.edit: --surface and --drags want positive integers")
        if args.pick is not None:
            sys.exit("nsdp_amd.edit: --pick goes with --vertices / --batch, not with --vertex-counts")
        if args.render:
            sys.exit("nsdp_amd.edit: --render goes with --vertices / --batch, not with --vertex-counts")
        if brushes is not None:
            sys.exit("nsdp_amd.edit: --brush goes with --vertices / --batch, not with --vertex-counts")
        return main_ragged(args, vertex_counts, surface_counts)
    ray = pick_from_args(args)
    if args.vertices < 1 or (args.surface is not None and args.surface < 1) or args.drags < 1:
        sys.exit("nsdp_amd.edit: --vertices, --surface and --drags want positive integers")
    if args.render and not 1 <= args.render_size <= 4096:
        sys.exit(f"nsdp_amd.edit: --render-size wants 1 .. 4096 pixels, got {args.render_size}")
    sphere = sphere_for(args.vertices) if (args.normals or args.self_intersections or ray is not None or brushes is not None
                                           or args.render) else None
    if sphere is not None:
        args.vertices = int(sphere[0].shape[0])
    device, config, spec, model, test_fn, timed, translation = _setup(args, args.surface or args.vertices)
    import numpy as np
    import torch
    from . import pointnet2_utils, synth
    from .infer import _checksum
    batch = args.batch or int((config.get("test") or {}).get("batch_size", 1) or 1)
    if sphere is None:
        verts, faces = torch.from_numpy(synth.uniform(SEED_DATA, "mesh_verts", (batch, args.vertices, 3), -0.5, 0.5)).to(device), None
    else:
        verts = torch.from_numpy(sphere[0])[None].repeat(batch, 1, 1).to(device)
        faces = torch.from_numpy(sphere[1]).to(device)
    surface = None if args.surface is None else \
        torch.from_numpy(synth.uniform(SEED_DATA, "mesh_surface", (batch, args.surface, 3), -0.5, 0.5)).to(device)
    with torch.no_grad():
        box = {}
        timed(lambda i: box.update(s=EditSession(model, verts, surface, partial_range=spec.partial_range, cliptail=spec.cliptail,
                                                 graph=args.graph, faces=faces)))      # (the first open also packs the weights)
        session = box["s"]
        ms_open = timed(lambda i: session.reopen())
        out = {}
        for i in range(max(args.warmup, 1)):      # (--graph: the first drag captures)
            session.drag(spec.part, translation(i))
        ms_drag = timed(lambda i: out.update(session.drag(spec.part, translation(i), clone=False)), args.drags)
        ms_normals = _timed_with_normals(args, session, spec, translation, timed, max(args.warmup, 1))
        selfint_fields = _timed_with_self_intersections(args, session, spec, translation, timed, max(args.warmup, 1))
        selfint_fields.update(_timed_with_render(args, session, verts, spec, translation, timed, max(args.warmup, 1), ms_drag))
        out = session.drag(spec.part, translation(args.drags - 1), with_inputs=True)
        pick_fields = _picked(ray, session, out, batch, device, timed, args.drags)
        pick_fields.update(_brushed(brushes, session, args, spec, batch, device, timed))
        dd = {"surface_samples_inputs": out["surface_samples_inputs"], "verts_src": verts,
              "surface_samples_src": out["surface_samples_inputs"][:, :, 0:3].contiguous()}
        for _ in range(max(args.warmup, 1)):
            test_fn(model, dict(dd), config)
        full = {}
        ms_full = timed(lambda i: full.update(test_fn(model, dict(dd), config)[1]), args.drags)
        equal = all(torch.equal(out[k], full[k]) for k in ("verts_tgt_pred", "surface_samples_tgt_pred"))
        pointnet2_utils.check_fps_cluster()
    if args.out:
        os.makedirs(args.out, exist_ok=True)
        for k in ("verts_tgt_pred", "surface_samples_tgt_pred", "verts_tgt"):
            np.save(os.path.join(args.out, k + ".npy"), out[k].cpu().numpy())
    line = {"metric": "edit_session", "model_type": config["model"]["type"], "graph": bool(args.graph), "batch": batch,
            "vertices": args.vertices, "surface": args.surface, "cloud_is_vertex_set": surface is None, "part": spec.part,
            "translation": list(spec.translation), "partial_range": spec.partial_range, "cliptail": spec.cliptail,
            "drags": args.drags, "warmup": args.warmup, "handle_points": int(out["cano_handle_sample_idx"].sum()),
            "ms_per_drag": round(ms_drag, 4), "ms_open": round(ms_open, 4), "ms_full_call": round(ms_full, 4),
            "full_call_over_drag": round(ms_full / ms_drag, 3) if ms_drag > 0 else None,
            "replays": session.replays, "eager_calls": session.eager_calls, "equal_to_full_call": bool(equal),
            "checksum": _checksum(out["verts_tgt_pred"])}
    if args.normals:
        line.update(_normals_fields(ms_drag, ms_normals, int(sphere[1].shape[0])))
    line.update(selfint_fields)
    line.update(pick_fields)
    print(json.dumps(line), flush=True)
    session.close()
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
