"""nsdp_amd.edit.RaggedEditSession on the GPU: one session over a packed batch of meshes of different vertex counts.  A drag
equals, bit for bit, the reference-shaped step function (test_on_batch_with_arbitrary / test_on_batch_with_cano) on the ragged
data_dict the drag stands for, built here with torch alone, shape by shape -- with the cloud as the vertex set, as a separate
packed cloud and as a rectangular one.  Each shape is within the suite's bar of the oracle on that shape alone; during a drag
nothing is searched, network 1 does not run and no offsets tensor is read back; a replayed drag equals the eager one; a cloud
above the one-workgroup kernels' 8192 points too; refusals.

Every comparison of handles is held non-vacuous: for every shape and drag 0 < #moved and 0 < #handle < n_b (a foot quadrant
holds about 2.5 % of a uniform cube, so quadrant parts go to shapes of at least 257 points only, under fixed seeds)."""
import pytest
import torch

from helpers import build_product, l2_err, model_cfg, nondeterministic_knobs
from nsdp_amd import edit
from nsdp_amd.edit import PARTS, EditSession, RaggedEditSession
from nsdp_amd.ragged import RaggedPoints

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
KEYS = ("verts_tgt_pred", "surface_samples_tgt_pred")
TOL_L2 = 1e-4                                         # tests/test_model_gpu.py: the suite's bar against the oracle
VERTS = (300, 257, 640, 65)
CLOUDS = (256, 300, 64, 513)                          # a separate packed cloud
RECT = 300                                            # ... and a rectangular one
T0 = (-0.15, -0.2, -0.2)
T1 = [(-0.15, 0.15, -0.15), (0.15, -0.2, 0.2), (0.1, 0.2, -0.1), (0.05, 0.1, -0.1)]
# four successive drags: the second with another part and translation per shape, the last repeating the first.  Quadrant parts
# where the shape has at least 257 points in every role: shapes 0, 1, 2 with the cloud as the vertex set, shape 1 otherwise.
DRAGS_SAME = [("head", T0), (["tail", "frontleftfoot", "behindrightfoot", "head"], T1),
              (["frontrightfoot", "tail", "frontleftfoot", "tail"], (-0.15, -0.2, 0.2)), ("head", T0)]
DRAGS_SEP = [("head", T0), (["tail", "frontleftfoot", "head", "tail"], T1),
             (["head", "behindrightfoot", "tail", "head"], (-0.15, -0.2, 0.2)), ("head", T0)]
LAYOUTS = ("same", "packed", "rect")


def _skip_variants():
    from nsdp_amd import hip_decoder, precision
    from nsdp_amd.model import deformation_networks as dn
    knobs = nondeterministic_knobs()
    if not hip_decoder.ENABLED:
        knobs.append("NSDP_FUSED_DECODER=0")      # (refused by the session: the layered decoder has no ragged form)
    if precision.is_bf16():
        knobs.append("NSDP_STORAGE=bf16")         # (refused by the session)
    if not dn.ENCODE_ONCE:
        knobs.append("NSDP_ENCODE_ONCE=0")        # (refused by the session)
    if knobs:
        pytest.skip("the session does not apply under " + ", ".join(knobs))


@pytest.fixture(scope="module")
def models():
    _skip_variants()
    out = {}
    for mtype, seed in (("arbitrary", 71), ("forward", 72)):
        cfg = model_cfg(mtype, [256, 64, 16])
        model, _, state = build_product(cfg, seed, DEV)
        out[mtype] = (model.eval(), cfg, state)
    return out


def _shapes(counts, seed, device=DEV):
    g = torch.Generator().manual_seed(seed)
    return [(torch.rand(n, 3, generator=g) - 0.5).to(device) for n in counts]


def _inputs(layout, seed=0, device=DEV):
    """(vertex shapes, cloud shapes or None, the session's verts_src, the session's surface)."""
    verts = _shapes(VERTS, 10 + seed, device)
    rv = RaggedPoints.from_list(verts)
    if layout == "same":
        return verts, None, rv, None
    if layout == "packed":
        clouds = _shapes(CLOUDS, 20 + seed, device)
        return verts, clouds, rv, RaggedPoints.from_list(clouds)
    clouds = _shapes((RECT,) * len(VERTS), 30 + seed, device)
    return verts, clouds, rv, torch.stack(clouds).contiguous()


def _per_shape(B, part, translation):
    parts = [part] * B if isinstance(part, str) else list(part)
    d = torch.as_tensor(translation, dtype=torch.float32)
    return parts, (d.expand(B, 3) if d.dim() == 1 else d).contiguous()


def torch_shape(src, part, d, r=0.1, cliptail=False):
    """One shape of one drag as the reference's data set builds it (dataset/utils.py: cano_handle_user_define on the source
    coordinates), in the array expressions of tests/test_edit_session_gpu.py::torch_data_dict: -> handle [n], move [n], tgt."""
    lo, hi = src.amin(dim=0), src.amax(dim=0)
    x, y, z = src[:, 0], src[:, 1], src[:, 2]
    head = y < lo[1] + r
    tail = y > hi[1] - r
    if cliptail:
        tail = tail & (z > -r)
    foot = z < lo[2] + r
    handle = head | tail | foot
    left, right, front, behind = foot & (x > 0), foot & (x < 0), foot & (y < 0), foot & (y > 0)
    move = (head, tail, left & front, right & front, left & behind, right & behind)[PARTS.index(part)]
    return handle, move, src + d.to(src.device) * move[:, None].float()


def torch_data_dict(verts, clouds, rect, part, translation, r=0.1, cliptail=False):
    """The ragged data_dict of one drag, shape by shape, and the per-shape pieces it was made of."""
    B = len(verts)
    parts, d = _per_shape(B, part, translation)
    vert_side = [torch_shape(verts[b], parts[b], d[b], r, cliptail) for b in range(B)]
    cloud_side = vert_side if clouds is None else [torch_shape(clouds[b], parts[b], d[b], r, cliptail) for b in range(B)]
    for b in range(B):      # no comparison of nothing with nothing
        for (h, m, _), what in ((vert_side[b], "vertices"), (cloud_side[b], "cloud")):
            assert 0 < int(m.sum()) and 0 < int(h.sum()) < h.numel(), (b, parts[b], what, int(m.sum()), int(h.sum()), h.numel())
    surf = verts if clouds is None else clouds
    rows = [torch.cat([surf[b], cloud_side[b][2] * cloud_side[b][0][:, None].float(), cloud_side[b][0][:, None].float()], dim=-1)
            for b in range(B)]
    if rect:
        inputs = torch.stack(rows).contiguous()
        src = torch.stack(surf).contiguous()
    else:
        inputs = RaggedPoints.from_rows(rows)
        src = inputs.columns(0, 3)
    return {"surface_samples_inputs": inputs, "surface_samples_src": src, "verts_src": RaggedPoints.from_list(verts),
            "verts_tgt": torch.cat([v[2] for v in vert_side]), "cano_handle_vert_idx": torch.cat([v[0] for v in vert_side]),
            "cano_handle_sample_idx": torch.stack([c[0] for c in cloud_side]) if rect else torch.cat([c[0] for c in cloud_side])}


def _step_fn(mtype):
    from nsdp_amd.model.deformation_networks import test_on_batch_with_cano
    from nsdp_amd.model.flow_arbitrary import test_on_batch_with_arbitrary
    return test_on_batch_with_arbitrary if mtype == "arbitrary" else test_on_batch_with_cano


def _t(x):
    return x.packed if isinstance(x, RaggedPoints) else x


def _flat(x):
    """A handle mask as one row per point: [cap, 1] packed rows, or [B, S] of a rectangular cloud."""
    return x.packed[:, 0] if isinstance(x, RaggedPoints) else x


def _where(a, b):
    rows = (a != b).reshape(-1, a.shape[-1]).any(-1).nonzero()
    return f"{rows.shape[0]} of {a.numel() // a.shape[-1]} rows differ, first: {rows[:4].reshape(-1).tolist()}"


def _drag_equals_step(mtype, model, session, verts, clouds, layout, part, translation, tag):
    out = session.drag(part=part, translation=translation, with_inputs=True)
    want = torch_data_dict(verts, clouds, layout == "rect", part, translation)
    assert isinstance(out["verts_tgt_pred"], RaggedPoints) and out["verts_tgt_pred"].counts == VERTS
    assert isinstance(out["surface_samples_inputs"], RaggedPoints) == (layout != "rect")
    assert torch.equal(_t(out["surface_samples_inputs"]), _t(want["surface_samples_inputs"])), (tag, "inputs")
    assert torch.equal(out["verts_tgt"].packed, want["verts_tgt"]), (tag, "verts_tgt")
    for k in ("cano_handle_vert_idx", "cano_handle_sample_idx"):
        assert _flat(out[k]).dtype is torch.bool and torch.equal(_flat(out[k]), want[k]), (tag, k)
    step_in = {k: want[k] for k in ("surface_samples_inputs", "surface_samples_src", "verts_src")}
    _, full = _step_fn(mtype)(model, dict(step_in), None)
    for k in KEYS:
        assert _t(out[k]).shape == _t(full[k]).shape and torch.equal(_t(out[k]), _t(full[k])), (tag, k, _where(_t(out[k]), _t(full[k])))
    # the reference-shaped inputs the session hands out feed the step function as they are
    inputs = out["surface_samples_inputs"]
    src = inputs.columns(0, 3) if isinstance(inputs, RaggedPoints) else inputs[:, :, 0:3].contiguous()
    _, again = _step_fn(mtype)(model, {"surface_samples_inputs": inputs, "verts_src": want["verts_src"], "surface_samples_src": src}, None)
    assert torch.equal(again["verts_tgt_pred"].packed, out["verts_tgt_pred"].packed), tag
    return out


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("mtype", ["arbitrary", "forward"])
def test_successive_drags_equal_the_step_function(models, mtype, layout):
    model = models[mtype][0]
    verts, clouds, rv, surface = _inputs(layout)
    drags = DRAGS_SAME if layout == "same" else DRAGS_SEP
    with torch.no_grad():
        session = RaggedEditSession(model, rv, surface)
        outs = [_drag_equals_step(mtype, model, session, verts, clouds, layout, part, d, (mtype, layout, i))
                for i, (part, d) in enumerate(drags)]
        assert session.eager_calls == len(drags) and session.replays == 0
        for k in KEYS:      # the first drag again gives the first result again, and another drag another
            assert torch.equal(_t(outs[0][k]), _t(outs[3][k])) and not torch.equal(_t(outs[0][k]), _t(outs[2][k]))
        if layout == "same":
            assert outs[0]["surface_samples_tgt_pred"] is outs[0]["verts_tgt_pred"]
            assert outs[0]["cano_handle_sample_idx"] is outs[0]["cano_handle_vert_idx"]
        else:
            assert _t(outs[0]["surface_samples_tgt_pred"]).shape == ((len(VERTS), RECT, 3) if layout == "rect" else (sum(CLOUDS), 3))
        # rule settings of a drag's own, through a HandleSpec
        spec = edit.HandleSpec("tail", (0.05, 0.1, -0.1), 0.2, True)
        out = session.drag(spec)
        want = torch_data_dict(verts, clouds, layout == "rect", "tail", spec.translation, r=0.2, cliptail=True)
        _, full = _step_fn(mtype)(model, {k: want[k] for k in ("surface_samples_inputs", "surface_samples_src", "verts_src")}, None)
        assert all(torch.equal(_t(out[k]), _t(full[k])) for k in KEYS) and torch.equal(out["verts_tgt"].packed, want["verts_tgt"])
        session.close()


@pytest.mark.parametrize("layout", ["same", "packed"])
def test_each_shape_against_the_oracle_and_its_own_batch_one_session(models, layout):
    """The forward type (no composition of two networks): each shape's rows within the suite's bar of the oracle on that shape
    alone at batch 1, and the handle-side outputs bit-equal to a batch-1 EditSession on that mesh."""
    from oracle import tdnet_ref
    model, cfg, state = models["forward"]
    sd = tdnet_ref.to_torch_state(state)
    verts, clouds, rv, surface = _inputs(layout, seed=3)
    part, d = (DRAGS_SAME if layout == "same" else DRAGS_SEP)[1]
    parts, dd = _per_shape(len(VERTS), part, d)
    with torch.no_grad():
        session = RaggedEditSession(model, rv, surface)
        out = session.drag(part, d, with_inputs=True)
        torch_data_dict(verts, clouds, False, part, d)      # (its assertions: every shape moves something)
        vert_rows, surf_rows = out["verts_tgt_pred"].split(), out["surface_samples_tgt_pred"].split()
        in_rows = out["surface_samples_inputs"].split()
        vt, vh = out["verts_tgt"].split(), out["cano_handle_vert_idx"].split()
        sh = out["cano_handle_sample_idx"].split()
        for b, nv in enumerate(VERTS):
            cloud = verts[b] if clouds is None else clouds[b]
            ref = tdnet_ref.model_forward(sd, cfg["model"], {"surface_samples_inputs": in_rows[b][None].cpu(),
                                                             "q": torch.cat([verts[b], cloud])[None].cpu()}, queries_key="q").numpy()[0]
            ev = l2_err(vert_rows[b][None].cpu().numpy(), ref[None, :nv])
            es = l2_err(surf_rows[b][None].cpu().numpy(), ref[None, nv:])
            print(f"{layout} shape {b} ({cloud.shape[0]} cloud points, {nv} vertices): l2 error against the oracle, vertices {ev:.3e}, "
                  f"cloud {es:.3e}")
            assert ev <= TOL_L2 and es <= TOL_L2, (b, ev, es)
            one = EditSession(model, verts[b][None].contiguous(), None if clouds is None else clouds[b][None].contiguous())
            o1 = one.drag(parts[b], tuple(dd[b].tolist()), with_inputs=True)
            one.close()
            assert torch.equal(o1["surface_samples_inputs"][0], in_rows[b]), b
            assert torch.equal(o1["verts_tgt"][0], vt[b]) and torch.equal(o1["cano_handle_vert_idx"][0], vh[b][:, 0]), b
            assert torch.equal(o1["cano_handle_sample_idx"][0], sh[b][:, 0]), b
        session.close()


def test_a_drag_searches_nothing_and_leaves_network_1_alone(models, monkeypatch):
    from nsdp_amd import pointnet2_utils as pu
    from nsdp_amd.model import ops
    model = models["arbitrary"][0]
    names = [(ops, "geometry_pyramid_ragged"), (ops, "geometry_pyramid"), (ops, "knn_indices"), (pu, "knn"), (pu, "knn_ragged"),
             (pu, "knn_ragged_source"), (pu, "furthest_point_sample_ragged"), (pu, "furthest_point_sample")]
    calls = {name: 0 for _, name in names}
    calls["net1"] = 0

    def counted(owner, name):
        real = getattr(owner, name)

        def fn(*a, **k):
            calls[name] += 1
            return real(*a, **k)
        monkeypatch.setattr(owner, name, fn)

    for owner, name in names:
        counted(owner, name)
    hooks = [m.register_forward_hook(lambda *a: calls.__setitem__("net1", calls["net1"] + 1))
             for m in model.model_canonicalize.modules()]
    try:
        for layout in LAYOUTS:
            verts, clouds, rv, surface = _inputs(layout, seed=5)
            for k in calls:
                calls[k] = 0
            with torch.no_grad():
                session = RaggedEditSession(model, rv, surface)
                opened = dict(calls)
                assert opened["net1"] >= 2 and opened["knn_ragged"] >= 2 and opened["knn"] >= 1, (layout, opened)
                if layout == "rect":
                    assert opened["geometry_pyramid"] >= 1 and opened["knn_indices"] >= 2, opened
                else:
                    assert opened["geometry_pyramid_ragged"] >= 2 and opened["knn_ragged_source"] >= 2, opened
                    assert opened["furthest_point_sample_ragged"] >= 2, opened      # (network 1's cloud and network 2's)
                for part, d in (DRAGS_SAME if layout == "same" else DRAGS_SEP):
                    session.drag(part, d)
                n = (len(VERTS), RECT) if layout == "rect" else (rv.capacity if layout == "same" else surface.capacity,)
                session.drag(handle_mask=torch.ones(n, dtype=torch.bool, device=DEV), move_mask=torch.zeros(n, dtype=torch.bool, device=DEV))
                assert calls == opened, (layout, opened, calls)
                session.reopen()
                assert calls == {k: 2 * v for k, v in opened.items()}, (layout, opened, calls)
                session.close()
    finally:
        for h in hooks:
            h.remove()


class _NoReadBack:
    """Counts every read-back of the given offsets tensors to the host: RaggedPoints.counts computed from the device (a set
    without host counts), and .tolist() / .cpu() / .item() / .numpy() on those very tensors."""

    def __init__(self, monkeypatch, offsets):
        self.reads = 0
        ptrs = {o.data_ptr() for o in offsets}
        real_counts = RaggedPoints.counts.fget

        def counts(r):
            if r._counts is None:
                self.reads += 1
            return real_counts(r)
        monkeypatch.setattr(RaggedPoints, "counts", property(counts))
        for name in ("tolist", "cpu", "item", "numpy"):
            real = getattr(torch.Tensor, name)

            def fn(t, *a, _real=real, **k):
                if t.is_cuda and t.dtype is torch.int32 and t.data_ptr() in ptrs:
                    self.reads += 1
                return _real(t, *a, **k)
            monkeypatch.setattr(torch.Tensor, name, fn)


@pytest.mark.parametrize("layout", LAYOUTS)
def test_replayed_drags_equal_eager_drags(models, layout, monkeypatch):
    model = models["arbitrary"][0]
    verts, clouds, rv, surface = _inputs(layout, seed=7)
    drags = DRAGS_SAME if layout == "same" else DRAGS_SEP
    n = (len(VERTS), RECT) if layout == "rect" else ((rv if layout == "same" else surface).capacity,)
    g = torch.Generator().manual_seed(3)
    hm, mm = (torch.rand(n, generator=g) < 0.4).to(DEV), (torch.rand(n, generator=g) < 0.2).to(DEV)
    vhm, vmm = (torch.rand(rv.capacity, generator=g) < 0.4).to(DEV), (torch.rand(rv.capacity, generator=g) < 0.2).to(DEV)
    vert_masks = {} if layout == "same" else dict(vert_handle_mask=vhm, vert_move_mask=vmm)
    every = KEYS + ("verts_tgt", "cano_handle_vert_idx", "cano_handle_sample_idx")
    with torch.no_grad():
        eager, graphed = RaggedEditSession(model, rv, surface), RaggedEditSession(model, rv, surface, graph=True)
        watch = _NoReadBack(monkeypatch, [rv.offsets] + ([surface.offsets] if isinstance(surface, RaggedPoints) else []))
        kept = []
        for i, (part, d) in enumerate(drags):
            a, b = eager.drag(part, d), graphed.drag(part, d)
            for k in every:
                assert torch.equal(_t(a[k]), _t(b[k])), (i, k)
            kept.append((a, b))
        assert graphed.replays == len(drags) and graphed.eager_calls == 0 and len(graphed._steps) == 1
        for a, b in kept[:-1]:      # the tensors handed out are the caller's own: later replays did not overwrite them
            assert all(torch.equal(_t(a[k]), _t(b[k])) for k in every)
        # a drag by explicit masks: the kernel's mask form is other kernel arguments, hence a SECOND capture
        a = eager.drag(handle_mask=hm, move_mask=mm, translation=(0.0, 0.1, -0.1), **vert_masks)
        b = graphed.drag(handle_mask=hm, move_mask=mm, translation=(0.0, 0.1, -0.1), **vert_masks)
        assert len(graphed._steps) == 2 and graphed.replays == len(drags) + 1
        assert all(torch.equal(_t(a[k]), _t(b[k])) for k in every)
        assert torch.equal(_flat(b["cano_handle_sample_idx"]), hm)
        moved = (mm if layout == "same" else vmm)[:, None].float()
        assert torch.equal(b["verts_tgt"].packed, rv.packed + torch.tensor((0.0, 0.1, -0.1), device=DEV) * moved)
        b2 = graphed.drag(handle_mask=mm, move_mask=hm, translation=(0.0, 0.1, -0.1), **vert_masks)      # replayed, other masks
        a2 = eager.drag(handle_mask=mm, move_mask=hm, translation=(0.0, 0.1, -0.1), **vert_masks)
        assert len(graphed._steps) == 2 and all(torch.equal(_t(a2[k]), _t(b2[k])) for k in KEYS)
        assert not torch.equal(b2["verts_tgt_pred"].packed, b["verts_tgt_pred"].packed)
        # ... then by rule again, replayed from the first graph
        c = graphed.drag(*drags[0])
        assert all(torch.equal(_t(c[k]), _t(kept[0][0][k])) for k in KEYS) and len(graphed._steps) == 2
        # clone=False hands out the replay's own buffers: the next replay overwrites them
        own = graphed.drag(*drags[2], clone=False)
        first = own["verts_tgt_pred"].packed.clone()
        assert torch.equal(first, kept[2][0]["verts_tgt_pred"].packed)
        graphed.drag(*drags[0])
        assert torch.equal(own["verts_tgt_pred"].packed, kept[0][0]["verts_tgt_pred"].packed)
        assert not torch.equal(own["verts_tgt_pred"].packed, first)
        if layout != "same":      # without vertex masks the vertices' target and handle are not defined
            none = eager.drag(handle_mask=hm, move_mask=mm)
            assert none["verts_tgt"] is None and none["cano_handle_vert_idx"] is None and none["verts_tgt_pred"] is not None
        assert watch.reads == 0, f"{watch.reads} read-back(s) of an offsets tensor during the drags"
        eager.close()
        graphed.close()


def test_a_cloud_above_the_one_workgroup_boundary(models):
    """(8200, 300) vertices, cloud = vertex set: the sampling, the searches and the session's own kernels take their large-cloud
    paths for the first shape, in one packed call with a small one."""
    from nsdp_amd import pointnet2_utils as pu
    model = models["arbitrary"][0]
    counts = (8200, 300)
    verts = _shapes(counts, 41)
    rv = RaggedPoints.from_list(verts)
    with torch.no_grad():
        session = RaggedEditSession(model, rv)
        out = session.drag(["tail", "frontleftfoot"], [(-0.15, 0.15, -0.15), (0.15, -0.2, 0.2)], with_inputs=True)
        want = torch_data_dict(verts, None, False, ["tail", "frontleftfoot"], [(-0.15, 0.15, -0.15), (0.15, -0.2, 0.2)])
        assert torch.equal(out["surface_samples_inputs"].packed, want["surface_samples_inputs"].packed)
        assert torch.equal(out["verts_tgt"].packed, want["verts_tgt"])
        _, full = _step_fn("arbitrary")(model, {k: want[k] for k in ("surface_samples_inputs", "surface_samples_src", "verts_src")}, None)
        for k in KEYS:
            assert torch.equal(out[k].packed, full[k].packed), (k, _where(out[k].packed, full[k].packed))
        session.close()
    pu.check_fps_cluster()


def test_gpu_side_refusals(models):
    model = models["arbitrary"][0]
    verts, clouds, rv, surface = _inputs("packed", seed=9)
    S = RaggedEditSession
    with torch.no_grad():
        with pytest.raises(ValueError, match="CPU tensors: surface"):
            S(model, rv, surface=surface.to("cpu"))
        with pytest.raises(ValueError, match="CPU tensors: cano"):
            S(model, rv, cano=rv.to("cpu"))
        with pytest.raises(ValueError, match="verts_src must be a RaggedPoints"):
            S(model, torch.stack(_shapes((300, 300), 1)))
        with pytest.raises(ValueError, match="an empty shape: shape 1 of verts_src"):
            S(model, RaggedPoints.from_list([verts[0], verts[0][:0]]))
        with pytest.raises(ValueError, match="shape 1 of the cloud has 63 points, fewer than the 64 points the first level samples"):
            S(model, RaggedPoints.from_list([verts[0], verts[1][:63]]))
        with pytest.raises(ValueError, match="shape 2 of the cloud has 10 points, fewer than"):
            S(model, rv, surface=RaggedPoints.from_list([clouds[0], clouds[1], clouds[2][:10], clouds[3]]))
        with pytest.raises(ValueError, match="surface holds 3 shapes, verts_src 4"):
            S(model, rv, surface=torch.stack(_shapes((256,) * 3, 1)))
        with pytest.raises(ValueError, match="surface holds 2 shapes, verts_src 4"):
            S(model, rv, surface=RaggedPoints.from_list(clouds[:2]))
        with pytest.raises(ValueError, match="is not over the same layout as verts_src"):
            S(model, rv, cano=RaggedPoints.from_list(verts[::-1]))
        with pytest.raises(ValueError, match="surface_cano is not over the same layout"):
            S(model, rv, surface=surface, surface_cano=rv)
        with pytest.raises(ValueError, match="does not read the handle columns"):
            S(model.model_canonicalize, rv)
        with pytest.raises(ValueError, match="ragged inputs: verts_src.*RaggedEditSession"):
            EditSession(model, rv)
        session = S(model, rv)
        cap = rv.capacity
        with pytest.raises(ValueError, match="name the part"):
            session.drag()
        with pytest.raises(ValueError, match="part must be one of"):
            session.drag("nose")
        with pytest.raises(ValueError, match="1 parts for 4 shapes"):
            session.drag(["head"])
        with pytest.raises(ValueError, match="go together"):
            session.drag(handle_mask=torch.ones(cap, dtype=torch.bool, device=DEV))
        with pytest.raises(ValueError, match="CPU tensors"):
            session.drag(handle_mask=torch.ones(cap, dtype=torch.bool), move_mask=torch.ones(cap, dtype=torch.bool))
        with pytest.raises(ValueError, match="bool / uint8"):
            m = torch.ones(cap - 1, dtype=torch.bool, device=DEV)
            session.drag(handle_mask=m, move_mask=m)
        with pytest.raises(ValueError, match="separate cloud only"):
            m = torch.ones(cap, dtype=torch.bool, device=DEV)
            session.drag(handle_mask=m, move_mask=m, vert_handle_mask=m, vert_move_mask=m)
        model.train()
        try:
            with pytest.raises(ValueError, match="training mode"):
                session.drag("head")
            with pytest.raises(ValueError, match="training mode"):
                session.reopen()
        finally:
            model.eval()
        with torch.enable_grad():
            with pytest.raises(ValueError, match="autograd is enabled"):
                session.drag("head")
            with pytest.raises(ValueError, match="autograd is enabled"):
                S(model, rv)
        assert session.drag("head", (0.1, 0.0, 0.0))["verts_tgt_pred"].packed.shape == (cap, 3)      # still usable
        session.close()
