"""Test-split evaluation from the device-resident mesh store: the reference's test.py loop (and, for the user-handle data sets,
its run.py loop) over packed batches of whole meshes of different sizes.

    python -m nsdp_amd.evaluate CONFIG [--batch N] [--weight_file F] [--seed S] [--limit K]

The reference walks its test split one pair at a time: it loads three meshes on the host, deforms every vertex of the source,
computes the metrics with one ``.item()`` each and writes five mesh files.  Here the split's frames are resident on the device
(nsdp_amd.meshstore); a batch of ``--batch`` pairs of DIFFERENT vertex counts is one launch of nsdp_mesh_batch_whole beside the
sampled clouds (``MeshStore.eval_loader``), one packed decode (nsdp_amd.ragged), one ``compute_evaluation_metrics_batch`` and
ONE ``.tolist()``; mesh export takes one device-to-host copy per batch.

The store is built from ``config["test"]``: ``iden_split``, ``motion_split``, ``num_sampled_pairs``; ``batch_size`` is the
default of ``--batch`` and ``weight_file`` that of ``--weight_file``.  Without a weight file the best checkpoint of the
experiment directory (``config["experiment"]``: ``out_dir`` / ``name``) is loaded, ``checkpoints.load_best_checkpoints``.

Output, in the experiment directory:
  <motion_split>.txt    one line per pair and a closing line of means.  Like the reference's loop (test.py:136-139) a metric
                        enters its mean only where its value is <= 1.0; how many values were left out is printed;
  <motion_split>.json   every per-pair value unfiltered, with the pair's names;
  <motion_split>/<mesh_folder>/{source,canonical,deformed,target,handle}/   with ``test.generate_mesh``: the meshes through
                        ``meshio.write_mesh`` under the reference's file names (utils/generation.py:11-35), vertices grey 0.75,
                        handle vertices red on source and canonical and blue on target; the handle mesh is the target's faces
                        whose three vertices are all handles; the deformed mesh is written uncoloured unless
                        ``test.vert_pred_color`` is set (below).
A pair's ``loss`` is what the step function returns for the BATCH the pair was in (the mean over its shapes of
compute_l2_error); at ``--batch 1`` it is the pair's own, as in the reference.

``data.type`` ``tosca`` / ``dogrec`` (``meshstore.HandleMeshStore``) is the reference's run.py: every batch opens a
``RaggedEditSession`` on its packed vertices -- the cloud being each mesh's own vertex set -- drags with
``HandleSpec.from_config(config["data"])``, exports the source, deformed, target and handle meshes into a folder named after the
drag (``drag_folder_name``), and computes no metrics.

Vertex normals, opt-in (nsdp_amd/mesh_normals.py; with neither key the files are byte for byte what they were):
  test.export_normals: true               the source, deformed and target meshes are written with per-vertex normals computed on
                                          the device -- the three vertex sets as three poses of the batch's one topology -- which
                                          travel in the batch's ONE device-to-host copy;
  test.vertex_normal_consistency: true    adds ``vnc`` to every pair: the mean over the vertices of |n_pred . n_gt|
                                          (``vertex_normal_consistency``), in the .txt, the .json and the batch's one ``.tolist()``.

Self-intersections, opt-in (nsdp_amd/self_intersect.py; without the key the files are byte for byte what they were):
  test.self_intersections: true           adds to every pair ``si``, the intersecting face pairs of the predicted mesh, ``si_faces``,
                                          the share of its faces with a hit, and ``si_gt``, the pairs of the TARGET mesh -- which
                                          tells a defect of the data from one of the model -- in the .txt, the .json and the batch's
                                          one ``.tolist()``.  Their means are plain means (the <= 1.0 filter is the metrics').  Faces
                                          the work guard skipped are named in a WARNING line.

Volume IoU, opt-in (nsdp_amd/ray_cast.py; without the key the files are byte for byte what they were):
  test.volume_iou: N                      adds ``iou`` to every pair: the volume IoU of the predicted against the target mesh from N
                                          uniform samples in the pair's joint bounding box (``ray_cast.volume_iou``; the draws are
                                          seeded by (seed, step): ``iou_generator``), in the .txt, the .json and the batch's one
                                          ``.tolist()``, with a plain mean.  Inside is the parity of ray crossings: it means
                                          something on closed meshes only, so a batch with open edges gets a WARNING line that
                                          names its pairs.

Error colours and views, opt-in (nsdp_amd/rasterize.py; without the keys the files are byte for byte what they were):
  test.vert_pred_color: true              with ``test.generate_mesh`` the deformed mesh is written with per-vertex colours, the jet
                                          map of |pred - tgt| clipped at 0.2 (``rasterize.error_colors``: the reference's
                                          generate_meshes(..., vert_pred_color=True)); they are computed on the device and travel in
                                          the batch's ONE device-to-host copy of the meshes;
  test.render: {views: K, size: S}        writes <motion_split>/<render_folder>/<src>_to_<tgt>_view<k>.png, K (1 .. 6) views of
                                          S x S pixels of every PREDICTED mesh, shaded with the error colours, rasterised on the
                                          device.  The cameras are fitted to the pair's TARGET mesh (its bounding box, read back once
                                          per batch) from the fixed directions ``VIEW_DIRECTIONS``: a function of the data and the
                                          config only.  ``dropped``, the faces the views lost over all K (a face that reaches the
                                          camera plane is dropped whole: there is no near-plane clipping; 0 for these fitted
                                          orthographic cameras unless a vertex is not finite), goes into the pair's row.

Refused by name: ``test.generate_pointcloud`` (point-cloud export).  Out of scope: ``--gpus N``, graph replay of the whole step.
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np
import torch

METRICS = ("l2", "fnc", "cd")
PARTS = ("source", "canonical", "deformed", "target", "handle")
GREY, RED, BLUE = (191, 191, 191), (255, 0, 0), (0, 0, 255)      # ((0.75 * 255).astype(uint8) = 191, as the reference rounds it)


class EvaluateError(ValueError):
    pass


# ---------------------------------------------------------------------------------------------------------------- names
def export_names(pair_info, ext) -> dict:
    """The five files of a pair, relative to the mesh folder (utils/generation.py:11-35): ``<seq>_<frame>.<ext>`` for source and
    canonical, ``<src_seq>_<src_frame>_to_<tgt_seq>_<tgt_frame>.<ext>`` for deformed, target and handle."""
    _, cano_seq, cano_frame, _, src_seq, src_frame, tgt_seq, tgt_frame = pair_info
    pair = f"{src_seq}_{src_frame}_to_{tgt_seq}_{tgt_frame}.{ext}"
    return {"source": os.path.join("source", f"{src_seq}_{src_frame}.{ext}"),
            "canonical": os.path.join("canonical", f"{cano_seq}_{cano_frame}.{ext}"),
            "deformed": os.path.join("deformed", pair), "target": os.path.join("target", pair), "handle": os.path.join("handle", pair)}


def drag_folder_name(data_cfg) -> str:
    """utils/generation.py:129-161: ``drag``, the first part that is set, ``_x%.2fy%.2fz%.2f``, ``_ratio%.2f``, ``_cliptail``."""
    from .edit import PARTS as HANDLE_PARTS
    uh = data_cfg["userhandle"]
    name = "drag" + next(("_" + p for p in HANDLE_PARTS if uh.get(p)), "")
    name += "_x%.2fy%.2fz%.2f" % (uh["xtrans"], uh["ytrans"], uh["ztrans"])
    name += "_ratio%.2f" % data_cfg["partial_range"]
    return name + ("_cliptail" if uh.get("cliptail") else "")


def filtered_means(rows, keys=METRICS):
    """(means, left_out) over per-pair dicts: a value enters its key's mean only where it is <= 1.0 (test.py:138; a NaN does not);
    ``left_out[key]`` counts the others.  A key without a value that entered has the mean NaN."""
    means, left_out = {}, {}
    for k in keys:
        kept = [r[k] for r in rows if r[k] <= 1.0]
        means[k] = float(np.mean(kept)) if kept else float("nan")
        left_out[k] = len(rows) - len(kept)
    return means, left_out


def refuse_pointclouds(config):
    if config.get("test", {}).get("generate_pointcloud"):
        raise EvaluateError("evaluate: test.generate_pointcloud (point-cloud export) is not supported; set it to false "
                            "(test.generate_mesh writes the meshes)")


def metric_samples(pred, faces, count, seed, step):
    """The surface draws of batch ``step``: ``sample_surface_batch`` on the predicted meshes with a generator seeded by
    (seed, step), so that a batch's metrics can be reproduced from its predictions."""
    from .eval_metric import sample_surface_batch
    g = torch.Generator(device=pred.device).manual_seed((int(seed) * 1000003 + int(step)) & 0x7FFFFFFFFFFFFFFF)
    return sample_surface_batch(pred.like(pred.packed.detach()), faces, int(count), g)


# ---------------------------------------------------------------------------------------------------------------- export
def _to_host(vertex_sets, handle, faces):
    """ONE device-to-host copy of what a batch's export needs: the [cap, 3] fp32 vertex sets, the [cap] handle flags and the
    [fcap, 3] int32 faces travel as the words of one int32 tensor."""
    parts = [v.contiguous().view(torch.int32).reshape(-1) for v in vertex_sets]
    parts += [handle.reshape(-1).to(torch.int32), faces.contiguous().reshape(-1)]
    flat = torch.cat(parts).cpu().numpy()
    cap, at, out = vertex_sets[0].shape[0], 0, []
    for _ in vertex_sets:
        out.append(flat[at:at + cap * 3].view(np.float32).reshape(cap, 3))
        at += cap * 3
    return out, flat[at:at + cap].astype(bool), flat[at + cap:].reshape(-1, 3)


def batch_normals(faces, vertex_sets):
    """Unit vertex normals [P, cap, 3] of P vertex sets (RaggedPoints over one layout) that share the packed topology ``faces``
    (a RaggedPoints of int32 rows): the corner lists once, two launches for all P.  The store has clamped every face index
    into its mesh, so nothing is read back to validate them."""
    from .mesh_normals import MeshTopology, vertex_normals
    topology = MeshTopology(faces, vertex_sets[0], validate=False)
    return vertex_normals(torch.stack([v.packed.detach() for v in vertex_sets]), topology)


def vertex_normal_consistency(n_pred, n_gt, offsets):
    """[B] float64: per shape the mean over its vertices of |n_pred . n_gt| -- 1 where the predicted surface is oriented like
    the target's everywhere, in [0, 1] always.  ``n_pred`` / ``n_gt`` [cap, 3] fp32 unit normals (zeros where a vertex has
    none), ``offsets`` the vertices' [B + 1] int32.  The dot is fp32, ((x x' + y y') + z z'); the mean goes through
    nsdp_segment_mean_f32 -- double accumulation in a fixed order, one fp32 result per shape -- three times: the mean m, then
    the means of the two fp32 halves of the residuals v - m (formed in double), which are ~2^-24 of m's size, so that their own
    fp32 roundings fall below 1e-14.  m + the two corrections, added in double, is the double-precision mean of the fp32 dots."""
    from .eval_metric import _dot_rows
    from .pointnet2_utils import segment_mean
    from .ragged import shape_ids
    B = int(offsets.numel()) - 1
    v = _dot_rows(n_pred, n_gt).abs().contiguous()
    m = segment_mean(v, offsets).double()
    r = v.double() - m[shape_ids(offsets, int(v.shape[0])).clamp(max=B - 1)]
    hi = r.float()
    lo = (r - hi.double()).float()
    return (m + segment_mean(hi, offsets).double()) + segment_mean(lo, offsets).double()


SI_KEYS = ("si", "si_faces", "si_gt")


def batch_self_intersections(faces, pred, target):
    """{si, si_faces, si_gt, si_skipped} as [B] float64 of a batch: the predicted and the target vertex sets (RaggedPoints over
    one layout) as two poses of the packed topology ``faces``, one call (the plan's Morton order is the prediction's).  The
    store has clamped every face index into its mesh, so nothing is read back to validate them."""
    from .self_intersect import SelfIntersectionPlan, self_intersections
    plan = SelfIntersectionPlan(faces, pred.like(pred.packed.detach()), validate=False)
    r = self_intersections(torch.stack([pred.packed.detach(), target.packed.detach()]), plan)
    count = (faces.offsets[1:] - faces.offsets[:-1]).clamp(min=1).double()
    return {"si": r.pairs[0].double(), "si_faces": r.faces_hit[0].double() / count, "si_gt": r.pairs[1].double(),
            "si_skipped": r.skipped.sum(dim=0).double()}


def iou_generator(device, seed, step):
    """The generator of batch ``step``'s volume-IoU samples: seeded by (seed, step), apart from ``metric_samples``' draws."""
    return torch.Generator(device=device).manual_seed(((int(seed) * 1000003 + int(step)) * 2 + 1) & 0x7FFFFFFFFFFFFFFF)


def batch_volume_iou(faces, pred, target, points, seed, step):
    """{iou, iou_open} as [B] float64 of a batch: the volume IoU of the predicted against the target vertex sets (RaggedPoints
    over one layout, two poses of the packed topology ``faces``) from ``points`` samples per pair, and every mesh's open edges.
    The store has clamped every face index into its mesh, so nothing is read back to validate them -- nor for the open edges,
    which stay on the device."""
    from .ray_cast import RayCastPlan, volume_iou
    verts = pred.like(pred.packed.detach())
    plan = RayCastPlan(faces, verts, validate=False)
    iou = volume_iou(verts, target.like(target.packed.detach()), plan, int(points), iou_generator(verts.device, seed, step))[0]
    return {"iou": iou, "iou_open": plan.open_edges_per_mesh.double()}


VIEW_DIRECTIONS = ((0.3, -0.2, 1.0), (-1.0, -0.2, 0.3), (0.3, -0.2, -1.0), (1.0, -0.2, -0.3), (0.2, -1.0, 0.2), (0.2, 1.0, -0.2))


def render_settings(test):
    """(views, size) of ``test.render``; (0, 0) without the key."""
    cfg = test.get("render")
    if not cfg:
        return 0, 0
    views, size = (cfg.get("views", 1), cfg.get("size", 512)) if isinstance(cfg, dict) else (None, None)
    ok = lambda v, top: isinstance(v, int) and not isinstance(v, bool) and 1 <= v <= top
    if not ok(views, len(VIEW_DIRECTIONS)) or not ok(size, 4096):
        raise EvaluateError(f"evaluate: test.render = {cfg!r}: {{views: 1 .. {len(VIEW_DIRECTIONS)}, size: 1 .. 4096}}")
    return views, size


def batch_views(faces, pred, target, colors, views, size):
    """(uint8 [B, views, size, size, 3] on the host, dropped [B][views]) of a batch: every predicted mesh (RaggedPoints) under
    ``views`` orthographic cameras fitted to its TARGET mesh from ``VIEW_DIRECTIONS``, shaded with the per-vertex ``colors``
    [cap, 3].  One read-back of the targets' bounding boxes, one of the images, one of the counts.  The store has clamped every
    face index into its mesh, so nothing is read back to validate them."""
    from .rasterize import Camera, RasterPlan, rasterize, shade
    from .ragged import shape_ids
    B, t = target.batch, target.packed.detach()
    where = shape_ids(target.offsets, target.capacity).unsqueeze(1).expand(-1, 3)
    lo = torch.full((B + 1, 3), float("inf"), device=t.device).scatter_reduce(0, where, t, "amin")[:B]
    hi = torch.full((B + 1, 3), float("-inf"), device=t.device).scatter_reduce(0, where, t, "amax")[:B]
    box = torch.stack([lo, hi]).cpu().numpy()
    cams = np.stack([[Camera.fit_box(box[0, b], box[1, b], VIEW_DIRECTIONS[k], size, size).matrix for k in range(views)]
                     for b in range(B)])
    verts = pred.like(pred.packed.detach())
    plan = RasterPlan(faces, verts, validate=False)
    r = rasterize(verts, plan, torch.from_numpy(cams).to(t.device), size, size)
    return shade(r, verts, plan, colors=colors).cpu().numpy(), r.dropped.tolist()


def export_meshes(directory, pair_infos, ext, verts, handle, faces, vert_counts, face_counts, normals=None, deformed_colors=None):
    """Write the meshes of a batch that is already on the host.  ``verts``: part -> [cap, 3] fp32 for "source", "deformed",
    "target" and, where it is exported, "canonical"; ``handle`` [cap] bool; ``faces`` [fcap, 3] int32, local indices;
    ``normals``: part -> [cap, 3] fp32 for the parts that are written with normals; ``deformed_colors``: [cap, 3] uint8 for
    the deformed mesh (written uncoloured without)."""
    from .meshio import write_mesh
    normals = normals or {}
    v0 = f0 = 0
    for info, nv, nf in zip(pair_infos, vert_counts, face_counts):
        names = export_names(info, ext)
        h, f = handle[v0:v0 + nv], faces[f0:f0 + nf]
        red, blue = np.tile(np.array(GREY, np.uint8), (nv, 1)), np.tile(np.array(GREY, np.uint8), (nv, 1))
        red[h], blue[h] = RED, BLUE
        for part, of, colors, sel in (("source", "source", red, f), ("canonical", "canonical", red, f), ("deformed", "deformed", None, f),
                                      ("target", "target", blue, f), ("handle", "target", blue, f[h[f].all(axis=1)])):
            if verts.get(of) is None:
                continue
            if part == "deformed" and deformed_colors is not None:
                colors = np.ascontiguousarray(deformed_colors[v0:v0 + nv])
            path = os.path.join(directory, names[part])
            os.makedirs(os.path.dirname(path), exist_ok=True)
            if normals.get(part) is None:
                write_mesh(path, verts[of][v0:v0 + nv], sel, colors)
            else:
                write_mesh(path, verts[of][v0:v0 + nv], sel, colors, normals[part][v0:v0 + nv])
        v0, f0 = v0 + nv, f0 + nf


# ---------------------------------------------------------------------------------------------------------------- the loops
def evaluate(model, test_fn, store, config, experiment_directory, batch, seed, log=print, limit=None) -> list:
    """The loop of the module docstring over ``store`` (a ``meshstore.MeshStore`` of the test split, or a ``HandleMeshStore``):
    -> the per-pair dicts, in the split's order.  ``test_fn``: the step function of ``build_model`` (either one: both read the
    same keys).  ``limit``: only the first ``limit`` pairs."""
    from .meshstore import HandleMeshStore
    refuse_pointclouds(config)
    test = config.get("test", {})
    os.makedirs(experiment_directory, exist_ok=True)
    model.eval()
    loader = store.eval_loader(batch, seed)
    if limit is not None:
        loader.samples = loader.samples[:max(int(limit), 0)]
    if isinstance(store, HandleMeshStore):
        return _drag_loop(model, store, loader, config, experiment_directory, log)
    from .eval_metric import compute_evaluation_metrics_batch
    split = test.get("motion_split", store.motion_split)
    mesh_dir = os.path.join(experiment_directory, split, test.get("mesh_folder", "meshes")) if test.get("generate_mesh") else None
    ext = test.get("mesh_format", "ply")
    with_normals, with_vnc = bool(test.get("export_normals")) and mesh_dir is not None, bool(test.get("vertex_normal_consistency"))
    with_si = bool(test.get("self_intersections"))
    iou_points = test.get("volume_iou") or 0
    if isinstance(iou_points, bool) or not isinstance(iou_points, int) or iou_points < 0:
        raise EvaluateError(f"evaluate: test.volume_iou = {test.get('volume_iou')!r}: the samples per pair, a positive integer "
                            "(not true / false)")
    with_colors = bool(test.get("vert_pred_color")) and mesh_dir is not None
    views, size = render_settings(test)
    render_dir = os.path.join(experiment_directory, split, test.get("render_folder", "renders")) if views else None
    metrics = METRICS + (("vnc",) if with_vnc else ())
    read = metrics + ((SI_KEYS + ("si_skipped",)) if with_si else ()) + (("iou", "iou_open") if iou_points else ())
    # (read: what the batch's one read-back carries)
    rows = []
    with open(os.path.join(experiment_directory, split + ".txt"), "w") as txt:
        def say(line):
            txt.write(line + "\n")
            log(line)
        for step, data_dict in enumerate(loader):
            loss, out = test_fn(model, data_dict, config, compute_loss=True)
            pred, faces = out["verts_tgt_pred"], out["faces"]
            samples = metric_samples(pred, faces, test.get("pointcloud_size", 30000), seed, step)
            m = compute_evaluation_metrics_batch(out, samples=samples)
            if with_normals or with_vnc:
                n_pred, n_tgt, n_src = batch_normals(faces, [pred, out["verts_tgt"], out["verts_src"]])
            if with_vnc:
                m["vnc"] = vertex_normal_consistency(n_pred, n_tgt, pred.offsets)
            if with_si:
                m.update(batch_self_intersections(faces, pred, out["verts_tgt"]))
            if iou_points:
                m.update(batch_volume_iou(faces, pred, out["verts_tgt"], iou_points, seed, step))
            if with_vnc or with_si or iou_points:
                values = torch.stack([m[k].double() for k in read]).tolist()      # (fp32 -> double is exact: the same numbers)
            else:
                values = torch.stack([m[k] for k in METRICS]).tolist()      # the batch's ONE read-back of metrics
            infos = [store.pairs[i] for i in out["index"]]
            if with_colors or views:
                from .rasterize import error_colors, to_uint8, vertex_errors, write_png
                colors = error_colors(vertex_errors(pred.packed, out["verts_tgt"].packed))
            if views:
                images, dropped = batch_views(faces, pred, out["verts_tgt"], colors, views, size)
                os.makedirs(render_dir, exist_ok=True)
                for b, info in enumerate(infos):
                    stem = os.path.splitext(os.path.basename(export_names(info, "png")["deformed"]))[0]
                    for k in range(views):
                        write_png(os.path.join(render_dir, f"{stem}_view{k}.png"), images[b, k])
            if iou_points:
                at_iou = len(read) - 2
                not_closed = [int(out["index"][b]) for b in range(len(infos)) if values[at_iou + 1][b]]
                if not_closed:
                    say("WARNING: pairs {}: the mesh has open edges ({}); inside is the parity of ray crossings and the iou of "
                        "these pairs depends on where the holes are".format(not_closed, ", ".join(
                            str(int(values[at_iou + 1][b])) for b in range(len(infos)) if values[at_iou + 1][b])))
            for b, info in enumerate(infos):
                row = {"index": int(out["index"][b]), "pair_info": list(info), "loss": float(loss)}
                row.update({k: values[c][b] for c, k in enumerate(metrics)})
                tail = ""
                if with_si:
                    at = len(metrics)
                    row.update({"si": int(values[at][b]), "si_faces": values[at + 1][b], "si_gt": int(values[at + 2][b])})
                    tail = "  si {:d}  si_faces {:.6e}  si_gt {:d}".format(row["si"], row["si_faces"], row["si_gt"])
                    if values[at + 3][b]:
                        say("WARNING: pair {:5d}: the work guard skipped {:d} faces of the predicted or the target mesh; their "
                            "intersections are not counted".format(row["index"], int(values[at + 3][b])))
                if iou_points:
                    row["iou"] = values[at_iou][b]
                    tail += "  iou {:.6e}".format(row["iou"])
                if views:
                    row["dropped"] = int(sum(dropped[b]))
                    tail += "  dropped {:d}".format(row["dropped"])
                rows.append(row)
                say("pair {:5d} {}_{} -> {}_{}  loss {:.6e}  ".format(row["index"], info[4], info[5], info[6], info[7], row["loss"])
                    + "  ".join("{} {:.6e}".format(k, row[k]) for k in metrics) + tail)
            if mesh_dir is not None:
                extra = [n_src, n_pred, n_tgt] if with_normals else []      # (in the same copy)
                if with_colors:                                             # (and the colours: bytes widened to words for the trip)
                    extra = extra + [to_uint8(colors).to(torch.int32).view(torch.float32)]
                sets, handle, f = _to_host([out["verts_src"].packed, out["verts_cano"].packed, pred.packed.detach(),
                                            out["verts_tgt"].packed] + extra, out["cano_handle_vert_idx"], faces.packed)
                export_meshes(mesh_dir, infos, ext, dict(zip(("source", "canonical", "deformed", "target"), sets)), handle, f,
                              pred.counts, faces.counts, dict(zip(("source", "deformed", "target"), sets[4:7] if with_normals else [])),
                              sets[-1].view(np.int32).astype(np.uint8) if with_colors else None)
        means, left_out = filtered_means(rows, metrics)
        say("mean over {} pairs (values <= 1.0 only)  ".format(len(rows)) + "  ".join("{} {:.6e}".format(k, means[k]) for k in metrics)
            + "  left out: " + ", ".join("{} {}".format(k, left_out[k]) for k in metrics))
        if with_si:
            means.update({k: float(np.mean([r[k] for r in rows])) if rows else float("nan") for k in SI_KEYS})
            say("mean over {} pairs (every value)  ".format(len(rows)) + "  ".join("{} {:.6e}".format(k, means[k]) for k in SI_KEYS))
        if iou_points:
            means["iou"] = float(np.mean([r["iou"] for r in rows])) if rows else float("nan")
            say("mean over {} pairs (every value)  iou {:.6e}".format(len(rows), means["iou"]))
    with open(os.path.join(experiment_directory, split + ".json"), "w") as f:
        json.dump({"pairs": rows, "means": means, "left_out": left_out}, f, indent=1)
    return rows


@torch.no_grad()
def _drag_loop(model, store, loader, config, experiment_directory, log):
    """run.py:119-139 over packed batches: one RaggedEditSession per batch, one drag, four meshes per pair, no metrics."""
    from .edit import HandleSpec, RaggedEditSession
    test = config.get("test", {})
    spec = HandleSpec.from_config(config["data"])
    mesh_dir = os.path.join(experiment_directory, drag_folder_name(config["data"]), test.get("mesh_folder", "meshes"))
    ext = test.get("mesh_format", "ply")
    rows = []
    for data_dict in loader:
        src, faces = data_dict["verts_src"], data_dict["faces"]
        with RaggedEditSession(model, src, partial_range=spec.partial_range, cliptail=spec.cliptail) as session:
            out = session.drag(spec)
            infos = [store.pairs[i] for i in data_dict["index"]]
            if test.get("generate_mesh", True):
                parts = [src, out["verts_tgt_pred"], out["verts_tgt"]]
                extra = list(batch_normals(faces, parts)) if test.get("export_normals") else []      # (in the same copy)
                sets, handle, f = _to_host([p.packed for p in parts] + extra, out["cano_handle_vert_idx"].packed, faces.packed)
                export_meshes(mesh_dir, infos, ext, dict(zip(("source", "deformed", "target"), sets)), handle, f, src.counts,
                              faces.counts, dict(zip(("source", "deformed", "target"), sets[3:])))
        for i, info in zip(data_dict["index"], infos):
            rows.append({"index": int(i), "pair_info": list(info)})
            log("dragged {} ({}) -> {}".format(info[4], spec.part, os.path.join(mesh_dir, export_names(info, ext)["deformed"])))
    return rows


def build_parser():
    ap = argparse.ArgumentParser(description="Evaluate a deformation network on the test split of a mesh data set (MI355X)")
    ap.add_argument("config_file")
    ap.add_argument("--batch", type=int, default=None, help="pairs per packed batch (default: test.batch_size of the config, else 1)")
    ap.add_argument("--weight_file", default=None, help="overrides test.weight_file; without either the experiment's best checkpoint")
    ap.add_argument("--seed", type=int, default=27, help="of the sampled clouds and of the metrics' surface draws")
    ap.add_argument("--limit", type=int, default=None, metavar="K", help="only the first K pairs of the split")
    return ap


def main(argv=None):
    import yaml
    from .checkpoints import load_best_checkpoints
    from .meshstore import HandleMeshStore, MeshStore
    from .datastore import HANDLE_KINDS
    from .model import build_model
    args = build_parser().parse_args(sys.argv[1:] if argv is None else argv)
    with open(args.config_file) as f:
        config = yaml.safe_load(f)
    try:
        refuse_pointclouds(config)
    except EvaluateError as e:
        sys.exit(f"nsdp_amd.evaluate: {e}")
    test = config["test"]
    experiment_directory = os.path.join(config["experiment"]["out_dir"], config["experiment"]["name"])
    os.makedirs(experiment_directory, exist_ok=True)
    device = torch.device("cuda", 0)
    weight_file = args.weight_file or test.get("weight_file")
    model, _, _, test_fn = build_model(config, weight_file, device=device)
    if weight_file is None:
        args.continue_from_epoch = None
        load_best_checkpoints(model, experiment_directory, args, device)
        if args.continue_from_epoch is None:
            print(f"WARNING: no weight file and no modelbest_* checkpoint in {experiment_directory}: the weights are random")
    store_class = HandleMeshStore if config["data"].get("type") in HANDLE_KINDS else MeshStore
    store = store_class(config, test.get("iden_split"), test["motion_split"], num_sampled_pairs=test.get("num_sampled_pairs", -1),
                        device=device)
    print("Loaded {} test deformation pairs ({} mesh frames, {:.2f} MB on the device)".format(len(store), len(store.frames),
                                                                                            store.nbytes / 1e6))
    rows = evaluate(model, test_fn, store, config, experiment_directory, args.batch or test.get("batch_size", 1), args.seed,
                    limit=args.limit)
    return 0 if rows else 1


if __name__ == "__main__":
    sys.exit(main())
