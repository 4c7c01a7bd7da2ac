"""Labelled handle sets through the editing sessions (nsdp_amd.edit: set_handles, pose, track, labels_from_parts) on the GPU.

A pose equals, bit for bit, the reference-shaped step function (test_on_batch_with_arbitrary / test_on_batch_with_cano) on the
data_dict reference_pose_dict builds with torch alone -- every stage of a pose is the kernel the step function runs, on the same
operands -- for both session classes, eager and replayed, next to rule drags on the same buffers.  A track of T poses equals
network 2's own step function on the T * B rows it stands for; against the same poses through ``pose`` it is held to rounding.

Every comparison is held non-vacuous: 0 < handle points < all points and every label 1..H occurs, in every set of labels."""
import numpy as np
import pytest
import torch

from helpers import build_product, l2_err, model_cfg
from nsdp_amd.edit import EditSession, Motion, RaggedEditSession, pack_motions, reference_pose_dict
from nsdp_amd.ragged import RaggedPoints
from test_edit_session_gpu import _skip_variants, _step_fn, _where, torch_data_dict

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
KEYS = ("verts_tgt_pred", "surface_samples_tgt_pred")
TOL_L2 = 1e-4                                         # tests/test_model_gpu.py: the suite's bar against the oracle
H = 3
CASES = [(mtype, B, separate) for mtype in ("arbitrary", "forward") for separate in (False, True) for B in (1, 2)]


@pytest.fixture(scope="module")
def models():
    _skip_variants()
    out = {}
    for mtype, seed in (("arbitrary", 71), ("forward", 72)):
        model, _, _ = build_product(model_cfg(mtype, [256, 64, 16]), seed, DEV)
        out[mtype] = model.eval()
    return out


def _points(B, n, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(B, n, 3, generator=g) - 0.5).to(DEV)


def _labels(points, flip=False):
    """Three handles cut from a cloud in the cube [-0.5, 0.5]^3 and a band of label 4 -- above H, hence free -- over [..., n]
    points: 1 = low y, 2 = low z, 3 = high y, the rest free.  ``flip``: other regions (for setting labels a second time)."""
    x, y, z = (points[..., c] for c in ((2, 0, 1) if flip else (0, 1, 2)))
    lab = torch.zeros(points.shape[:-1], dtype=torch.uint8, device=points.device)
    lab[x > 0.4] = 4
    lab[y > 0.3] = 3
    lab[z < -0.3] = 2
    lab[y < -0.3] = 1
    handle = (lab >= 1) & (lab <= H)
    assert 0 < int(handle.sum()) < handle.numel() and all(bool((lab == h).any()) for h in range(1, H + 2)), "vacuous labels"
    for b in range(points.shape[0] if points.dim() == 3 else 0):      # ... and in every shape
        assert all(bool((lab[b] == h).any()) for h in range(1, H + 1)) and not bool(handle[b].all()), b
    return lab


def _pose(B, i):
    """Pose i of B shapes, each shape with motions of its own: handle 1 turns about a pivot, 2 moves, 3 is pinned."""
    return [[Motion.rotate((0.2 * b, 1.0, 0.5 + i), 15.0 + 10.0 * i + 5.0 * b, pivot=(0.1 * i, -0.3, 0.05 * b)),
             Motion.translate((0.1 + 0.05 * i, -0.1 * b - 0.02, 0.05 * (i + 1))), Motion.identity()] for b in range(B)]


def _setup(B, separate, seed, n=300, s=256):
    verts = _points(B, n, seed)
    surface = _points(B, s, seed + 1) if separate else None
    labels = _labels(verts if surface is None else surface)
    vlabels = _labels(verts) if separate else None
    return verts, surface, labels, vlabels


def _equals_step(mtype, model, out, want, tag):
    assert torch.equal(out["surface_samples_inputs"], want["surface_samples_inputs"]), (tag, "inputs")
    for k in ("verts_tgt", "cano_handle_vert_idx", "cano_handle_sample_idx"):
        assert out[k].dtype == want[k].dtype and torch.equal(out[k], want[k]), (tag, k)
    step_in = {k: want[k] for k in ("surface_samples_inputs", "surface_samples_src", "verts_src")}
    _, full = _step_fn(mtype)(model, dict(step_in), None)
    for k in KEYS:
        assert out[k].shape == full[k].shape and torch.equal(out[k], full[k]), (tag, k, _where(out[k], full[k]))
    return full


@pytest.mark.parametrize("mtype,B,separate", CASES)
def test_successive_poses_equal_the_step_function(models, mtype, B, separate):
    model = models[mtype]
    verts, surface, labels, vlabels = _setup(B, separate, 10 * B + separate)
    with torch.no_grad():
        session = EditSession(model, verts, surface).set_handles(labels, H, vlabels)
        outs = []
        for i in range(3):
            out = session.pose(motions=_pose(B, i), with_inputs=True)
            want = reference_pose_dict(verts, surface, labels, H, motions=_pose(B, i), vert_labels=vlabels)
            _equals_step(mtype, model, out, want, (mtype, B, separate, i))
            outs.append(out)
        assert session.eager_calls == 3 and session.replays == 0
        assert not torch.equal(outs[0]["verts_tgt_pred"], outs[1]["verts_tgt_pred"])
        # a pinned handle's points are handle points whose target is where they are; a label above H is a free point
        pinned = (labels if vlabels is None else vlabels) == 3
        assert torch.equal(outs[2]["verts_tgt"][pinned], verts[pinned]) and bool(outs[2]["cano_handle_vert_idx"][pinned].all())
        assert not bool(outs[2]["cano_handle_vert_idx"][(labels if vlabels is None else vlabels) == 4].any())
        # motions as the [B, H, 12] array, and one list broadcast over the shapes
        again = session.pose(motions=pack_motions(B, H, _pose(B, 0)))
        assert all(torch.equal(again[k], outs[0][k]) for k in KEYS)
        one = session.pose(motions=_pose(1, 1)[0], with_inputs=True)
        _equals_step(mtype, model, one, reference_pose_dict(verts, surface, labels, H, motions=_pose(1, 1)[0], vert_labels=vlabels), "broadcast")
        if separate:      # without vertex labels the vertices' target and handle are not defined
            none = session.set_handles(labels, H).pose(motions=_pose(B, 0))
            assert none["verts_tgt"] is None and none["cano_handle_vert_idx"] is None
            assert all(torch.equal(none[k], outs[0][k]) for k in KEYS)
        session.close()


@pytest.mark.parametrize("mtype,B,separate", CASES)
def test_poses_by_targets_equal_the_step_function(models, mtype, B, separate):
    model = models[mtype]
    verts, surface, labels, vlabels = _setup(B, separate, 30 * B + separate)
    cloud = verts if surface is None else surface
    with torch.no_grad():
        session = EditSession(model, verts, surface).set_handles(labels, H, vlabels)
        for i in range(2):      # the handle positions of a "recorded frame": nothing parametric about them
            targets = cloud + 0.05 * (i + 1) * torch.sin(7.0 * cloud + i)
            vtargets = verts + 0.05 * (i + 1) * torch.sin(7.0 * verts + i) if separate else None
            out = session.pose(targets=targets, vert_targets=vtargets, with_inputs=True)
            want = reference_pose_dict(verts, surface, labels, H, targets=targets, vert_labels=vlabels, vert_targets=vtargets)
            _equals_step(mtype, model, out, want, (mtype, B, separate, i))
            assert bool(out["cano_handle_sample_idx"][labels == 4].all())      # with targets every non-zero label is a handle
        if separate:
            none = session.pose(targets=cloud)
            assert none["verts_tgt"] is None and none["cano_handle_vert_idx"] is None and none["verts_tgt_pred"] is not None
        session.close()


@pytest.mark.parametrize("separate", [False, True])
def test_a_pose_a_rule_drag_and_the_pose_again(models, separate):
    model = models["arbitrary"]
    B = 2
    verts, surface, labels, vlabels = _setup(B, separate, 51 + separate)
    with torch.no_grad():
        for graph in (False, True):
            session = EditSession(model, verts, surface, graph=graph).set_handles(labels, H, vlabels)
            first = session.pose(motions=_pose(B, 0), with_inputs=True)
            _equals_step("arbitrary", model, first, reference_pose_dict(verts, surface, labels, H, motions=_pose(B, 0), vert_labels=vlabels), "first")
            drag = session.drag("head", (-0.15, -0.2, -0.2), with_inputs=True)
            _equals_step("arbitrary", model, drag, torch_data_dict(verts, surface, "head", (-0.15, -0.2, -0.2)), "drag")
            third = session.pose(motions=_pose(B, 0), with_inputs=True)
            for k in KEYS + ("verts_tgt", "cano_handle_vert_idx", "cano_handle_sample_idx", "surface_samples_inputs"):
                assert torch.equal(third[k], first[k]), (graph, k)
            assert not torch.equal(drag["verts_tgt_pred"], first["verts_tgt_pred"])
            if graph:      # the forms sit beside each other: one graph each
                assert len(session._steps) == 2 and session.replays == 3 and session.eager_calls == 0
            session.close()


@pytest.mark.parametrize("separate", [False, True])
def test_replayed_poses_equal_eager_poses(models, separate):
    model = models["arbitrary"]
    B = 2
    verts, surface, labels, vlabels = _setup(B, separate, 61 + separate)
    cloud = verts if surface is None else surface
    with torch.no_grad():
        eager = EditSession(model, verts, surface).set_handles(labels, H, vlabels)
        graphed = EditSession(model, verts, surface, graph=True).set_handles(labels, H, vlabels)
        kept = []
        for i in (0, 1, 2, 0):
            a, b = eager.pose(motions=_pose(B, i)), graphed.pose(motions=_pose(B, i))
            for k in KEYS + ("verts_tgt", "cano_handle_vert_idx", "cano_handle_sample_idx"):
                assert torch.equal(a[k], b[k]), (i, k)
            kept.append((a, b))
        # every pose after the capture is a replay (the capturing call replays its graph too: `replays` counts calls)
        assert graphed.replays == 4 and graphed.eager_calls == 0 and len(graphed._steps) == 1 and eager.eager_calls == 4
        for a, b in kept:      # the tensors handed out are the caller's own: later replays did not overwrite them
            assert all(torch.equal(a[k], b[k]) for k in KEYS)
        assert all(torch.equal(kept[0][1][k], kept[3][1][k]) for k in KEYS)
        # the same count again: the graph stays, and the next pose is a replay with the new labels' result
        step = graphed._steps[("pose", False, separate)]
        new, vnew = _labels(cloud, flip=True), (_labels(verts, flip=True) if separate else None)
        assert not torch.equal(new, labels)
        eager.set_handles(new, H, vnew)
        graphed.set_handles(new, H, vnew)
        a, b = eager.pose(motions=_pose(B, 1), with_inputs=True), graphed.pose(motions=_pose(B, 1), with_inputs=True)
        assert graphed._steps[("pose", False, separate)] is step and len(graphed._steps) == 1 and graphed.replays == 5
        _equals_step("arbitrary", model, b, reference_pose_dict(verts, surface, new, H, motions=_pose(B, 1), vert_labels=vnew), "relabelled")
        assert all(torch.equal(a[k], b[k]) for k in KEYS) and not torch.equal(b["verts_tgt_pred"], kept[1][1]["verts_tgt_pred"])
        # the targets form is a second graph beside it; another count drops the graphs of these forms only
        t = cloud + 0.1
        vt = verts + 0.1 if separate else None
        a, b = eager.pose(targets=t, vert_targets=vt), graphed.pose(targets=t, vert_targets=vt)
        assert len(graphed._steps) == 2 and all(torch.equal(a[k], b[k]) for k in KEYS + ("verts_tgt",))
        graphed.drag("head", (0.1, 0.0, 0.0))
        assert len(graphed._steps) == 3
        two = torch.where(new == 3, torch.zeros_like(new), new)
        vtwo = torch.where(vnew == 3, torch.zeros_like(vnew), vnew) if separate else None
        graphed.set_handles(two, 2, vtwo)
        assert list(graphed._steps) == [(False, False)]
        b = graphed.pose(motions=[Motion.translate((0.1, 0.0, 0.0)), Motion.identity()], with_inputs=True)
        _equals_step("arbitrary", model, b, reference_pose_dict(verts, surface, two, 2, motions=[Motion.translate((0.1, 0.0, 0.0)),
                                                                                                 Motion.identity()], vert_labels=vtwo), "count 2")
        if separate:      # vertex labels taken away and given back: the graph that reads them replays on the session's own buffer
            m2 = [Motion.translate((0.1, 0.0, 0.0)), Motion.identity()]
            assert graphed.set_handles(two, 2).pose(motions=m2)["verts_tgt"] is None
            other = torch.where(vtwo == 2, torch.full_like(vtwo, 1), vtwo)      # (the pinned vertices now move too)
            b = graphed.set_handles(two, 2, other).pose(motions=m2, with_inputs=True)
            _equals_step("arbitrary", model, b, reference_pose_dict(verts, surface, two, 2, motions=m2, vert_labels=other), "given back")
            assert not torch.equal(b["verts_tgt"], verts) and len(graphed._steps) == 3
        eager.close()
        graphed.close()
        assert graphed._labels is None and graphed._tracks == {} and graphed._steps == {}


def test_a_cloud_above_the_one_workgroup_boundary(models):
    """8200 vertices, cloud = vertex set: the sampling, the searches and the session's own kernels take their large-cloud paths."""
    model = models["arbitrary"]
    verts = _points(1, 8200, 41)
    labels = _labels(verts)
    with torch.no_grad():
        session = EditSession(model, verts).set_handles(labels, H)
        out = session.pose(motions=_pose(1, 1), with_inputs=True)
        _equals_step("arbitrary", model, out, reference_pose_dict(verts, None, labels, H, motions=_pose(1, 1)), "8200")
        session.close()


def test_labels_from_parts(models):
    model = models["arbitrary"]
    B = 2
    verts, surface = _points(B, 1200, 81), _points(B, 1024, 82)
    parts = ["head", "frontleftfoot", "tail"]
    with torch.no_grad():
        for cloud_is_verts in (True, False):
            session = EditSession(model, verts, None if cloud_is_verts else surface)
            cloud = verts if cloud_is_verts else surface
            labels, count = session.labels_from_parts(parts)
            assert count == 4 and labels.dtype is torch.uint8 and labels.shape == cloud.shape[:2]
            want = torch.zeros_like(labels)
            regions = [torch_data_dict(cloud, None, p, (1.0, 0.0, 0.0)) for p in parts]
            want[regions[0]["cano_handle_vert_idx"]] = 4                       # every other handle point of the rule
            for i in reversed(range(3)):                                       # earlier parts win where regions overlap
                want[(regions[i]["verts_tgt"] != cloud).any(-1)] = i + 1
            assert torch.equal(labels, want) and all(bool((labels == h).any()) for h in range(5))
            if not cloud_is_verts:
                vlabels, vcount = session.labels_from_parts(parts, verts=True)
                assert vcount == 4 and vlabels.shape == verts.shape[:2] and bool((vlabels == 1).any())
            # the rule's own drag, restated: head moves, every other handle point is pinned
            lab2, c2 = session.labels_from_parts(["head"])
            d = (-0.15, -0.2, -0.2)
            pose = session.set_handles(lab2, c2, session.labels_from_parts(["head"], verts=True)[0] if not cloud_is_verts else None) \
                .pose(motions=[Motion.translate(d), Motion.identity()])
            drag = session.drag("head", d)
            assert torch.equal(pose["cano_handle_sample_idx"], drag["cano_handle_sample_idx"])
            assert torch.equal(pose["verts_tgt"], drag["verts_tgt"])           # (a uniform cloud holds no zero coordinate)
            assert all(torch.equal(pose[k], drag[k]) for k in KEYS)
            session.close()


# ---------------------------------------------------------------------------------------------------- a packed batch
COUNTS = (700, 300, 512)
CLOUD_COUNTS = (256, 300, 257)


@pytest.mark.parametrize("mtype", ["arbitrary", "forward"])
@pytest.mark.parametrize("separate", [False, True])
def test_packed_poses_equal_the_ragged_step_function(models, mtype, separate):
    model = models[mtype]
    g = torch.Generator().manual_seed(90 + separate)
    verts = [(torch.rand(n, 3, generator=g) - 0.5).to(DEV) for n in COUNTS]
    clouds = [(torch.rand(n, 3, generator=g) - 0.5).to(DEV) for n in CLOUD_COUNTS] if separate else None
    B = len(COUNTS)
    rv = RaggedPoints.from_list(verts)
    rs = RaggedPoints.from_list(clouds) if separate else None
    surf = clouds if separate else verts
    lab = [_labels(c[None])[0] for c in surf]
    vlab = [_labels(v[None])[0] for v in verts] if separate else None

    def packed(rp, per_shape, dtype):
        out = torch.zeros((rp.capacity,) + tuple(per_shape[0].shape[1:]), dtype=dtype, device=DEV)
        out[:rp.total] = torch.cat(per_shape)
        return out

    def want_of(i, targets=None, vtargets=None):
        """The ragged data_dict of pose i, shape by shape at batch 1."""
        dds = [reference_pose_dict(verts[b][None], clouds[b][None] if separate else None, lab[b][None], H,
                                   motions=None if targets is not None else [_pose(B, i)[b]],
                                   targets=None if targets is None else targets[b][None], vert_labels=vlab[b][None] if separate else None,
                                   vert_targets=None if vtargets is None else vtargets[b][None]) for b in range(B)]
        inputs = RaggedPoints.from_rows([d["surface_samples_inputs"][0] for d in dds])
        return {"surface_samples_inputs": inputs, "surface_samples_src": inputs.columns(0, 3), "verts_src": rv,
                "verts_tgt": torch.cat([d["verts_tgt"][0] for d in dds]),
                "cano_handle_vert_idx": torch.cat([d["cano_handle_vert_idx"][0] for d in dds]),
                "cano_handle_sample_idx": torch.cat([d["cano_handle_sample_idx"][0] for d in dds])}

    def check(out, want, tag):
        total_v, total_s = rv.total, (rs.total if separate else rv.total)
        assert torch.equal(out["surface_samples_inputs"].packed[:total_s], want["surface_samples_inputs"].packed[:total_s]), tag
        assert torch.equal(out["verts_tgt"].packed[:total_v], want["verts_tgt"]), tag
        assert torch.equal(out["cano_handle_vert_idx"].packed[:total_v, 0], want["cano_handle_vert_idx"]), tag
        assert torch.equal(out["cano_handle_sample_idx"].packed[:total_s, 0], want["cano_handle_sample_idx"]), tag
        _, full = _step_fn(mtype)(model, {k: want[k] for k in ("surface_samples_inputs", "surface_samples_src", "verts_src")}, None)
        for k in KEYS:
            assert torch.equal(out[k].packed, full[k].packed), (tag, k)

    with torch.no_grad():
        labels = packed(rs if separate else rv, lab, torch.uint8)
        vlabels = packed(rv, vlab, torch.uint8) if separate else None
        eager = RaggedEditSession(model, rv, rs).set_handles(labels, H, vlabels)
        graphed = RaggedEditSession(model, rv, rs, graph=True).set_handles(labels, H, vlabels)
        for i in (0, 1, 0):
            want = want_of(i)
            check(eager.pose(motions=_pose(B, i), with_inputs=True), want, ("eager", i))
            check(graphed.pose(motions=_pose(B, i), with_inputs=True), want, ("replayed", i))
        tg = [c + 0.05 * torch.sin(5.0 * c) for c in surf]
        vtg = [v + 0.05 * torch.sin(5.0 * v) for v in verts] if separate else None
        want = want_of(0, tg, vtg)
        kw = dict(targets=packed(rs if separate else rv, tg, torch.float32),
                  vert_targets=packed(rv, vtg, torch.float32) if separate else None, with_inputs=True)
        check(eager.pose(**kw), want, "eager targets")
        check(graphed.pose(**kw), want, "replayed targets")
        check(graphed.pose(**kw), want, "replayed targets again")
        assert graphed.replays == 5 and graphed.eager_calls == 0 and len(graphed._steps) == 2 and eager.replays == 0
        with pytest.raises(ValueError, match="RaggedEditSession refused: a track over a packed session.*packed rows"):
            graphed.track(motions=[_pose(B, 0)])
        eager.close()
        graphed.close()


# ---------------------------------------------------------------------------------------------------- tracks
def _track_dict(session, inputs, T):
    """The T * B-row data_dict a track stands for, for network 2's own step function: network 1's cached outputs repeated T
    times beside the track's columns 3:7.  That call searches the same coordinates and so gets the same index sets; network 1's
    batch size does not enter."""
    B, S = inputs.shape[1], inputs.shape[2]
    rows = torch.cat([session.surf2cano.repeat(T, 1, 1), inputs[..., 3:7].reshape(T * B, S, 4)], dim=-1).contiguous()
    return {"surface_samples_inputs": rows, "surface_samples_src": rows[:, :, 0:3].contiguous(),
            "verts_src": session.verts2cano.repeat(T, 1, 1).contiguous()}


@pytest.mark.parametrize("mtype,B,separate", CASES)
def test_a_track_equals_network_2_on_its_rows(models, mtype, B, separate):
    from nsdp_amd.model.deformation_networks import test_on_batch_with_cano
    model = models[mtype]
    T = 3
    verts, surface, labels, vlabels = _setup(B, separate, 70 * B + separate)
    V, S = verts.shape[1], (surface if separate else verts).shape[1]
    poses = [_pose(B, i) for i in range(T)]
    with torch.no_grad():
        eager = EditSession(model, verts, surface).set_handles(labels, H, vlabels)
        graphed = EditSession(model, verts, surface, graph=True).set_handles(labels, H, vlabels)
        out = eager.track(motions=poses, with_inputs=True)
        assert out["verts_tgt_pred"].shape == (T, B, V, 3) and out["surface_samples_tgt_pred"].shape == (T, B, S, 3)
        assert out["verts_tgt"].shape == (T, B, V, 3) and out["surface_samples_inputs"].shape == (T, B, S, 7)
        singles = []
        for t in range(T):      # the handle side of every pose: reference_pose_dict's bits
            want = reference_pose_dict(verts, surface, labels, H, motions=poses[t], vert_labels=vlabels)
            assert torch.equal(out["surface_samples_inputs"][t], want["surface_samples_inputs"]), t
            assert torch.equal(out["verts_tgt"][t], want["verts_tgt"]), t
            assert torch.equal(out["cano_handle_vert_idx"], want["cano_handle_vert_idx"])
            assert torch.equal(out["cano_handle_sample_idx"], want["cano_handle_sample_idx"])
            singles.append(eager.pose(motions=poses[t]))
        _, full = test_on_batch_with_cano(eager.net, _track_dict(eager, out["surface_samples_inputs"], T), None)
        for k in KEYS:
            assert torch.equal(out[k].reshape(full[k].shape), full[k]), (k, _where(out[k].reshape(full[k].shape), full[k]))
        # each pose of the track against the same pose through pose(): two fp32 evaluations of one function whose dense layers
        # pick their tiles by row count (T * B rows here, B there), so they are not bit-equal.  Each side is within the suite's
        # bar of 1e-4 (helpers.l2_err against the oracle) of exact arithmetic, hence within twice that bar of the other.
        for t in range(T):
            for k in KEYS:
                err = l2_err(out[k][t].cpu().numpy(), singles[t][k].cpu().numpy())
                assert err <= 2 * TOL_L2, (t, k, err)
        # the replay equals eager; a second track of the same T is a replay
        a = graphed.track(motions=poses)
        b = graphed.track(motions=torch.from_numpy(np.stack([pack_motions(B, H, p) for p in poses])))
        assert graphed.replays == 2 and graphed.eager_calls == 0 and list(graphed._steps) == [("track", T, False, separate)]
        for k in KEYS + ("verts_tgt", "cano_handle_vert_idx", "cano_handle_sample_idx"):
            assert torch.equal(a[k], out[k]) and torch.equal(b[k], out[k]), k
        other = graphed.track(motions=poses[::-1])
        assert graphed.replays == 3 and len(graphed._steps) == 1 and torch.equal(other["verts_tgt"][0], out["verts_tgt"][2])
        assert not torch.equal(other["verts_tgt_pred"], out["verts_tgt_pred"])
        # targets, T = 2: another (form, T), another capture; a pose and a drag beside it still stand
        cloud = verts if surface is None else surface
        tg = torch.stack([cloud + 0.05 * (i + 1) * torch.sin(7.0 * cloud) for i in range(2)])
        vtg = torch.stack([verts + 0.05 * (i + 1) * torch.sin(7.0 * verts) for i in range(2)]) if separate else None
        c, d = eager.track(targets=tg, vert_targets=vtg, with_inputs=True), graphed.track(targets=tg, vert_targets=vtg)
        assert len(graphed._steps) == 2 and all(torch.equal(c[k], d[k]) for k in KEYS + ("verts_tgt",))
        for t in range(2):
            want = reference_pose_dict(verts, surface, labels, H, targets=tg[t], vert_labels=vlabels, vert_targets=None if vtg is None else vtg[t])
            assert torch.equal(c["surface_samples_inputs"][t], want["surface_samples_inputs"]) and torch.equal(c["verts_tgt"][t], want["verts_tgt"])
        _, full = test_on_batch_with_cano(eager.net, _track_dict(eager, c["surface_samples_inputs"], 2), None)
        assert all(torch.equal(c[k].reshape(full[k].shape), full[k]) for k in KEYS)
        p = graphed.pose(motions=poses[0])
        assert all(torch.equal(p[k], singles[0][k]) for k in KEYS)
        # reopen() and close() drop the track's buffers and graphs with the rest
        assert set(graphed._tracks) == {3, 2}
        graphed.reopen()
        assert graphed._tracks == {} and graphed._steps == {}
        again = graphed.track(motions=poses)
        assert all(torch.equal(again[k], out[k]) for k in KEYS)
        graphed.close()
        eager.close()
        assert graphed._tracks == {} and graphed._steps == {}


# ---------------------------------------------------------------------------------------------------- refusals
def test_refusals(models):
    model = models["arbitrary"]
    B = 2
    verts, surface, labels, vlabels = _setup(B, True, 95)
    rv = RaggedPoints.from_list([verts[0], verts[1, :260]])
    with torch.no_grad():
        packed = RaggedEditSession(model, rv)
        with pytest.raises(ValueError, match="RaggedEditSession refused: a track over a packed session"):
            packed.track(motions=[[Motion.identity()]])
        with pytest.raises(ValueError, match=r"labels must be uint8 \(560,\)"):
            packed.set_handles(labels, H)
        packed.close()
        s = EditSession(model, verts, surface)
        for call in (lambda: s.pose(motions=_pose(B, 0)), lambda: s.track(motions=[_pose(B, 0)])):
            with pytest.raises(ValueError, match="before set_handles"):
                call()
        with pytest.raises(ValueError, match=r"labels must be uint8 \(2, 256\), got bool"):
            s.set_handles(labels.bool(), H)
        with pytest.raises(ValueError, match=r"labels must be uint8 \(2, 256\), got uint8 \(2, 255\)"):
            s.set_handles(labels[:, :255], H)
        with pytest.raises(ValueError, match="CPU tensors: set_handles: labels"):
            s.set_handles(labels.cpu(), H)
        with pytest.raises(ValueError, match=r"vert_labels must be uint8 \(2, 300\)"):
            s.set_handles(labels, H, labels)
        for count in (0, 256, 2.0, True):
            with pytest.raises(ValueError, match="count must be an integer in 1..255"):
                s.set_handles(labels, count)
        with pytest.raises(ValueError, match="before set_handles"):      # (a refused set_handles sets nothing)
            s.pose(motions=_pose(B, 0))
        s.set_handles(labels, H)
        with pytest.raises(ValueError, match="neither 3 motions .* nor 2 lists"):
            s.pose(motions=[Motion.identity()] * 2)
        with pytest.raises(ValueError, match=r"must be \[2, 3, 12\]"):
            s.pose(motions=torch.zeros(2, 4, 12))
        with pytest.raises(ValueError, match=r"must be \[T, 2, 3, 12\]"):
            s.track(motions=torch.zeros(2, 3, 12))
        with pytest.raises(ValueError, match="exactly one of motions and targets .got neither"):
            s.pose()
        with pytest.raises(ValueError, match="exactly one of motions and targets .got both"):
            s.pose(motions=_pose(B, 0), targets=surface)
        with pytest.raises(ValueError, match="exactly one of motions and targets .got neither"):
            s.track()
        with pytest.raises(ValueError, match="vert_targets without vert_labels"):
            s.pose(targets=surface, vert_targets=verts)
        with pytest.raises(ValueError, match="vert_targets without vert_labels"):
            s.track(targets=surface[None], vert_targets=verts[None])
        with pytest.raises(ValueError, match=r"targets must be float32 \(2, 256, 3\)"):
            s.pose(targets=verts)
        with pytest.raises(ValueError, match="CPU tensors: pose: targets"):
            s.pose(targets=surface.cpu())
        with pytest.raises(ValueError, match="at least one pose"):
            s.track(motions=[])
        with pytest.raises(ValueError, match=r"T \* B must be at most 65535"):
            s.track(motions=torch.zeros(32768, 2, 3, 12))
        same = EditSession(model, verts)
        with pytest.raises(ValueError, match="vert_labels go with a separate cloud only"):
            same.set_handles(vlabels, H, vlabels)
        with pytest.raises(ValueError, match="names of"):
            same.labels_from_parts(["nose"])
        same.close()
        with torch.enable_grad():
            with pytest.raises(ValueError, match="autograd is enabled"):
                s.pose(motions=_pose(B, 0))
        assert s.pose(motions=_pose(B, 0))["verts_tgt_pred"].shape == (2, 300, 3)      # still usable
        s.close()
