"""nsdp_amd.edit.EditSession on the GPU: a drag through the session equals, bit for bit, the reference-shaped step function
(test_on_batch_with_arbitrary / test_on_batch_with_cano) on the data_dict the drag stands for, built here with torch alone -- every
stage of a drag is the kernel the step function runs, on the same operands.  During a drag nothing is searched and network 1
does not run; a replayed drag equals the eager one; 8200 vertices (above the one-workgroup kernels' 8192) too; refusals."""
import pytest
import torch

from helpers import build_product, model_cfg, nondeterministic_knobs
from nsdp_amd import edit
from nsdp_amd.edit import PARTS, EditSession

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
KEYS = ("verts_tgt_pred", "surface_samples_tgt_pred")
# three successive drags with different parts and translations (the second: another part and translation per shape), then the first again
DRAGS = [("head", (-0.15, -0.2, -0.2)),
         (["tail", "frontleftfoot"], [(-0.15, 0.15, -0.15), (0.15, -0.2, 0.2)]),
         ("behindrightfoot", (-0.15, -0.2, 0.2)),
         ("head", (-0.15, -0.2, -0.2))]


def _skip_variants():
    from nsdp_amd import hip_decoder, precision
    from nsdp_amd.model import deformation_networks as dn
    knobs = nondeterministic_knobs()
    if not hip_decoder.ENABLED:
        knobs.append("NSDP_FUSED_DECODER=0")      # (refused by the session: the layered decoder's tiles follow the row count)
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
        model, _, _ = build_product(model_cfg(mtype, [256, 64, 16]), seed, DEV)
        out[mtype] = model.eval()
    return out


def _points(B, n, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(B, n, 3, generator=g) - 0.5).to(DEV)


def _per_shape(B, part, translation):
    parts = [part] * B if isinstance(part, str) else list(part)[:B]
    d = torch.as_tensor(translation, dtype=torch.float32)
    d = d.expand(B, 3) if d.dim() == 1 else d[:B]
    return parts, d.contiguous()


def torch_data_dict(verts, surface, part, translation, r=0.1, cliptail=False):
    """The data_dict of one drag as the reference's data set builds it (dataset/utils.py: cano_handle_user_define on the source
    coordinates, dataset_userhandle_flow.py: inputs = [src | mask * tgt | mask]), in torch array expressions."""
    B = verts.shape[0]
    parts, d = _per_shape(B, part, translation)
    sel = torch.tensor([PARTS.index(p) for p in parts], device=DEV).view(B, 1)
    d = d.to(DEV).view(B, 1, 3)

    def one(src):
        lo, hi = src.amin(dim=1), src.amax(dim=1)
        x, y, z = src[:, :, 0], src[:, :, 1], src[:, :, 2]
        head = y < lo[:, 1:2] + r
        tail = y > hi[:, 1:2] - r
        if cliptail:
            tail = tail & (z > -r)
        foot = z < lo[:, 2:3] + r
        handle = head | tail | foot
        left, right, front, behind = foot & (x > 0), foot & (x < 0), foot & (y < 0), foot & (y > 0)
        move = torch.zeros_like(head)
        for i, region in enumerate((head, tail, left & front, right & front, left & behind, right & behind)):
            move = torch.where(sel == i, region, move)
        return handle, src + d * move[:, :, None].float()

    vh, vt = one(verts)
    sh, st = (vh, vt) if surface is None else one(surface)
    surf = verts if surface is None else surface
    maskf = sh[:, :, None].float()
    return {"surface_samples_inputs": torch.cat([surf, st * maskf, maskf], dim=-1).contiguous(), "surface_samples_src": surf,
            "verts_src": verts, "verts_tgt": vt, "cano_handle_vert_idx": vh, "cano_handle_sample_idx": sh}


def _step_fn(mtype):
    from nsdp_amd.model.deformation_networks import test_on_batch_with_cano
    from nsdp_amd.model.flow_arbitrary import test_on_batch_with_arbitrary
    return test_on_batch_with_arbitrary if mtype == "arbitrary" else test_on_batch_with_cano


def _where(a, b):
    rows = (a != b).any(-1).nonzero()
    return f"{rows.shape[0]} of {a.shape[0] * a.shape[1]} rows differ, first (shape, row): {rows[:4].tolist()}"


def _drag_equals_step(mtype, model, session, verts, surface, part, translation, tag):
    B = verts.shape[0]
    parts, d = _per_shape(B, part, translation)
    out = session.drag(part=parts if B > 1 else parts[0], translation=d, with_inputs=True)
    want = torch_data_dict(verts, surface, parts, d)
    assert torch.equal(out["surface_samples_inputs"], want["surface_samples_inputs"]), (tag, "inputs")
    for k in ("verts_tgt", "cano_handle_vert_idx", "cano_handle_sample_idx"):
        assert out[k].dtype == want[k].dtype and torch.equal(out[k], want[k]), (tag, k)
    assert 0 < int(want["cano_handle_sample_idx"].sum()) < want["cano_handle_sample_idx"].numel(), tag
    _, full = _step_fn(mtype)(model, dict(want), None)
    for k in KEYS:
        assert out[k].shape == full[k].shape and torch.equal(out[k], full[k]), (tag, k, _where(out[k], full[k]))
    # the reference-shaped inputs the session hands out feed the step function as they are
    _, again = _step_fn(mtype)(model, {"surface_samples_inputs": out["surface_samples_inputs"], "verts_src": verts,
                                      "surface_samples_src": out["surface_samples_inputs"][:, :, 0:3].contiguous()}, None)
    assert torch.equal(again["verts_tgt_pred"], out["verts_tgt_pred"]), tag
    return out


@pytest.mark.parametrize("mtype,B,separate", [("arbitrary", 1, False), ("arbitrary", 2, False), ("arbitrary", 1, True),
                                              ("arbitrary", 2, True), ("forward", 2, False), ("forward", 1, True)])
def test_successive_drags_equal_the_step_function(models, mtype, B, separate):
    model = models[mtype]
    verts = _points(B, 300, 10 * B + separate)
    surface = _points(B, 256, 20 * B + separate) if separate else None
    with torch.no_grad():
        session = EditSession(model, verts, surface)
        outs = [_drag_equals_step(mtype, model, session, verts, surface, part, d, (mtype, B, separate, i))
                for i, (part, d) in enumerate(DRAGS)]
        assert session.eager_calls == len(DRAGS) and session.replays == 0
        for k in KEYS:      # the first drag again gives the first result again, and another drag another
            assert torch.equal(outs[0][k], outs[3][k]) and not torch.equal(outs[0][k], outs[2][k])
        if not separate:
            assert outs[0]["surface_samples_tgt_pred"] is outs[0]["verts_tgt_pred"]
        # rule settings of a drag's own, and a HandleSpec
        spec = edit.HandleSpec("tail", (0.05, 0.1, -0.1), 0.2, True)
        out = session.drag(spec)
        want = torch_data_dict(verts, surface, "tail", spec.translation, r=0.2, cliptail=True)
        _, full = _step_fn(mtype)(model, dict(want), None)
        assert all(torch.equal(out[k], full[k]) for k in KEYS) and torch.equal(out["verts_tgt"], want["verts_tgt"])
        ref = edit.reference_data_dict(verts, surface, spec)
        assert all(torch.equal(ref[k], want[k]) for k in want)
        session.close()


def test_a_drag_searches_nothing_and_leaves_network_1_alone(models, monkeypatch):
    from nsdp_amd import pointnet2_utils as pu
    from nsdp_amd.model import ops
    model = models["arbitrary"]
    calls = {"geometry_pyramid": 0, "knn_indices": 0, "knn": 0, "furthest_point_sample": 0, "net1": 0}

    def counted(owner, name):
        real = getattr(owner, name)

        def fn(*a, **k):
            calls[name] += 1
            return real(*a, **k)
        monkeypatch.setattr(owner, name, fn)

    counted(ops, "geometry_pyramid")
    counted(ops, "knn_indices")
    counted(pu, "knn")
    counted(pu, "furthest_point_sample")
    hooks = [m.register_forward_hook(lambda *a: calls.__setitem__("net1", calls["net1"] + 1))
             for m in model.model_canonicalize.modules()]
    try:
        for separate in (False, True):
            verts = _points(2, 300, 5)
            surface = _points(2, 256, 6) if separate else None
            for k in calls:
                calls[k] = 0
            with torch.no_grad():
                session = EditSession(model, verts, surface)
                opened = dict(calls)
                assert opened["geometry_pyramid"] >= 1 and opened["knn_indices"] >= 2 and opened["net1"] >= 2, opened
                for part, d in DRAGS:
                    session.drag(part, d)
                session.drag(handle_mask=verts.new_ones(2, surface.shape[1] if separate else 300, dtype=torch.bool),
                             move_mask=verts.new_zeros(2, surface.shape[1] if separate else 300, dtype=torch.bool))
                assert calls == opened, (separate, opened, calls)
                session.reopen()
                assert calls["geometry_pyramid"] == 2 * opened["geometry_pyramid"] and calls["net1"] == 2 * opened["net1"]
                session.close()
    finally:
        for h in hooks:
            h.remove()


@pytest.mark.parametrize("separate", [False, True])
def test_replayed_drags_equal_eager_drags(models, separate):
    model = models["arbitrary"]
    B = 2
    verts = _points(B, 300, 31)
    surface = _points(B, 256, 32) if separate else None
    n = 256 if separate else 300
    g = torch.Generator().manual_seed(3)
    hm, mm = (torch.rand(B, n, generator=g) < 0.4).to(DEV), (torch.rand(B, n, generator=g) < 0.2).to(DEV)
    vhm, vmm = (torch.rand(B, 300, generator=g) < 0.4).to(DEV), (torch.rand(B, 300, generator=g) < 0.2).to(DEV)
    vert_masks = dict(vert_handle_mask=vhm, vert_move_mask=vmm) if separate else {}
    with torch.no_grad():
        eager, graphed = EditSession(model, verts, surface), EditSession(model, verts, surface, graph=True)
        kept = []
        for i, (part, d) in enumerate(DRAGS):
            a, b = eager.drag(part, d), graphed.drag(part, d)
            for k in KEYS + ("verts_tgt", "cano_handle_vert_idx", "cano_handle_sample_idx"):
                assert torch.equal(a[k], b[k]), (i, k)
            kept.append((a, b))
        assert graphed.replays == len(DRAGS) and graphed.eager_calls == 0 and len(graphed._steps) == 1
        for a, b in kept[:-1]:      # the tensors handed out are the caller's own: later replays did not overwrite them
            assert all(torch.equal(a[k], b[k]) for k in KEYS)
        # a drag by explicit masks after the drags by rule: the kernel's mask form is other kernel arguments, hence a SECOND
        # capture (nsdp_amd/edit.py says so); then by rule again, replayed from the first graph
        a = eager.drag(handle_mask=hm, move_mask=mm, translation=(0.0, 0.1, -0.1), **vert_masks)
        b = graphed.drag(handle_mask=hm, move_mask=mm, translation=(0.0, 0.1, -0.1), **vert_masks)
        assert len(graphed._steps) == 2 and graphed.replays == len(DRAGS) + 1
        assert all(torch.equal(a[k], b[k]) for k in KEYS + ("verts_tgt", "cano_handle_sample_idx"))
        assert torch.equal(b["cano_handle_sample_idx"], hm)
        assert torch.equal(b["verts_tgt"], verts + torch.tensor((0.0, 0.1, -0.1), device=DEV) * (vmm if separate else mm)[:, :, None].float())
        b2 = graphed.drag(handle_mask=mm, move_mask=hm, translation=(0.0, 0.1, -0.1), **vert_masks)      # replayed, other masks
        a2 = eager.drag(handle_mask=mm, move_mask=hm, translation=(0.0, 0.1, -0.1), **vert_masks)
        assert len(graphed._steps) == 2 and all(torch.equal(a2[k], b2[k]) for k in KEYS)
        assert not torch.equal(b2["verts_tgt_pred"], b["verts_tgt_pred"])
        c = graphed.drag(*DRAGS[0])
        assert all(torch.equal(c[k], kept[0][0][k]) for k in KEYS) and len(graphed._steps) == 2
        # clone=False hands out the replay's own buffers: the next replay overwrites them
        own = graphed.drag(*DRAGS[2], clone=False)
        first = own["verts_tgt_pred"].clone()
        assert torch.equal(first, kept[2][0]["verts_tgt_pred"])
        graphed.drag(*DRAGS[0])
        assert torch.equal(own["verts_tgt_pred"], kept[0][0]["verts_tgt_pred"]) and not torch.equal(own["verts_tgt_pred"], first)
        if separate:      # without vertex masks the vertices' target and handle are not defined
            none = eager.drag(handle_mask=hm, move_mask=mm)
            assert none["verts_tgt"] is None and none["cano_handle_vert_idx"] is None and none["verts_tgt_pred"] is not None
        eager.close()
        graphed.close()


def test_a_cloud_above_the_one_workgroup_boundary(models):
    """8200 vertices, cloud = vertex set: the sampling, the searches and the session's own kernels take their large-cloud paths."""
    model = models["arbitrary"]
    verts = _points(1, 8200, 41)
    with torch.no_grad():
        session = EditSession(model, verts)
        _drag_equals_step("arbitrary", model, session, verts, None, "tail", (-0.15, 0.15, -0.15), "8200")
        session.close()


def test_gpu_side_refusals(models):
    from nsdp_amd.ragged import RaggedPoints
    model = models["arbitrary"]
    verts = _points(2, 300, 51)
    with torch.no_grad():
        with pytest.raises(ValueError, match="CPU tensors: surface"):
            EditSession(model, verts, surface=torch.zeros(2, 256, 3))
        with pytest.raises(ValueError, match="CPU tensors: cano"):
            EditSession(model, verts, cano=verts.cpu())
        with pytest.raises(ValueError, match="ragged inputs: surface"):
            EditSession(model, verts, surface=RaggedPoints.from_list([verts[0], verts[1, :100]]))
        with pytest.raises(ValueError, match="surface holds 1 shapes"):
            EditSession(model, verts, surface=_points(1, 256, 1))
        with pytest.raises(ValueError, match="not shaped like verts_src"):
            EditSession(model, verts, cano=_points(2, 299, 1))
        with pytest.raises(ValueError, match="does not read the handle columns"):
            EditSession(model.model_canonicalize, verts)
        session = EditSession(model, verts)
        with pytest.raises(ValueError, match="name the part"):
            session.drag()
        with pytest.raises(ValueError, match="part must be one of"):
            session.drag("nose")
        with pytest.raises(ValueError, match="2 shapes"):
            session.drag(["head"])
        with pytest.raises(ValueError, match="go together"):
            session.drag(handle_mask=verts.new_ones(2, 300, dtype=torch.bool))
        with pytest.raises(ValueError, match="CPU tensors"):
            session.drag(handle_mask=torch.ones(2, 300, dtype=torch.bool), move_mask=torch.ones(2, 300, dtype=torch.bool))
        with pytest.raises(ValueError, match="bool / uint8"):
            session.drag(handle_mask=verts.new_ones(2, 299, dtype=torch.bool), move_mask=verts.new_ones(2, 299, dtype=torch.bool))
        with pytest.raises(ValueError, match="separate cloud only"):
            m = verts.new_ones(2, 300, dtype=torch.bool)
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
                EditSession(model, verts)
        assert session.drag("head", (0.1, 0.0, 0.0))["verts_tgt_pred"].shape == (2, 300, 3)      # still usable
        session.close()
