"""CPU: the Chamfer loss's yardstick against itself (tests/chamfer_ref.py: closed form against fp64 autograd, the l2 identity),
the boundary of the feature -- include/nsdp_chamfer.h declares the entries and the built library exports them at ABI version
18, bad arguments come back as a status with a message before anything could be launched --, the refusals of
``chamfer_loss`` by name, the config switch of the step functions and the uncorresponded targets of ``SyntheticLoader``."""
import ctypes
import os
import re

import pytest
import torch

import chamfer_ref
from nsdp_amd import _lib, build as nsdp_build, chamfer
from nsdp_amd.ragged import RaggedPoints

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "nsdp_chamfer.h")
ENTRY_POINTS = ["nsdp_chamfer_backward", "nsdp_chamfer_forward", "nsdp_chamfer_forward_workspace_bytes"]


def _clouds(B, n, m, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(B, n, 3, generator=g), torch.randn(B, m, 3, generator=g)


# ------------------------------------------------------------------------------------------------------------ the yardstick
@pytest.mark.parametrize("B,n,m,w_pt,w_tp", [(1, 17, 9, 1.0, 1.0), (3, 40, 64, 0.5, 2.0), (2, 33, 33, 1.0, 0.0), (2, 5, 70, 0.0, 1.0)])
def test_closed_form_equals_fp64_autograd_on_tie_free_clouds(B, n, m, w_pt, w_tp):
    P, Q = _clouds(B, n, m, 100 * n + m)
    d = chamfer_ref.dist2_64(P, Q)
    idx_pt, idx_tp = d.argmin(dim=2), d.argmin(dim=1)
    chamfer_ref.assert_minimisers(P, Q, idx_pt, idx_tp)
    loss, dP, dQ = chamfer_ref.autograd64(P, Q, w_pt, w_tp)
    cf = chamfer_ref.closed_form(P, Q, idx_pt, idx_tp, w_pt, w_tp)
    for name, want in (("dP", dP), ("dQ", dQ)):
        grad, mass, lengths = cf[name]
        assert float((grad - want).abs().max()) <= 1e-13 * float(mass.max()) + 1e-300, name
        assert bool((grad.abs() <= mass * (1 + 1e-12)).all())
        assert int(lengths.sum()) == B * (m if name == "dP" else n)
    # an upstream gradient scales the closed form
    assert torch.equal(chamfer_ref.closed_form(P, Q, idx_pt, idx_tp, w_pt, w_tp, g=4.0)["dP"][0], 4.0 * cf["dP"][0])
    assert float(loss) > 0


def test_l2_identity_where_the_nearest_neighbour_is_the_correspondent():
    """Well-separated corresponded targets, in any row order, w_tp = 0: the Chamfer loss is compute_l2_error on the unpermuted
    rows, up to rounding (and its gradient the l2 gradient)."""
    from nsdp_amd.model.utils import compute_l2_error
    g = torch.Generator().manual_seed(5)
    B, n = 2, 50
    grid = torch.stack(torch.meshgrid(torch.arange(5.0), torch.arange(5.0), torch.arange(2.0), indexing="ij"), -1).reshape(1, n, 3)
    P = (grid + 0.05 * torch.randn(B, n, 3, generator=g)).float()
    T = (P + 0.1 * torch.randn(B, n, 3, generator=g)).float()
    perm = torch.stack([torch.randperm(n, generator=g) for _ in range(B)])
    Q = torch.gather(T, 1, perm[:, :, None].expand(B, n, 3))
    P64 = P.double().requires_grad_(True)
    loss, _ = chamfer_ref.loss64(P64, Q, 1.0, 0.0)
    loss.backward()
    P64b = P.double().requires_grad_(True)
    l2 = compute_l2_error(P64b, T.double())
    l2.backward()
    assert abs(loss.item() - l2.item()) <= 1e-14 * l2.item()
    assert float((P64.grad - P64b.grad).abs().max()) <= 1e-15
    # with the sets equal the loss is exactly 0
    assert float(chamfer_ref.loss64(P, P.clone())[0]) == 0.0


def test_depth_follows_the_documented_operation_order():
    T = torch.tensor([0, 1, 2, 32, 33, 64, 65, 1024, 1025, 8200, 100000])
    assert chamfer_ref.depth(T).tolist() == [0, 0, 1, 31, 6, 6, 7, 21, 12, 40, 398]
    assert chamfer_ref.envelope_c(T).tolist() == [6.0 + d for d in chamfer_ref.depth(T).tolist()]


# ------------------------------------------------------------------------------------------------------------- the boundary
@pytest.fixture(scope="module")
def so():
    if not os.path.exists(_lib.SO_PATH):
        nsdp_build.build()
    lib = ctypes.CDLL(_lib.SO_PATH)
    lib.nsdp_last_error.restype = ctypes.c_char_p
    lib.nsdp_chamfer_forward_workspace_bytes.restype = ctypes.c_size_t
    return lib


def test_header_declares_and_library_exports_the_entries(so):
    with open(HEADER) as f:
        text = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(nsdp_[a-z0-9_]+)\s*\(", text)))
    assert declared == ENTRY_POINTS
    for name in ENTRY_POINTS:
        assert hasattr(so, name), name
    assert so.nsdp_abi_version() >= 18
    assert not set(ENTRY_POINTS) & set(_lib.declared_symbols())          # (nsdp_hip.h keeps its own table of entries)
    assert os.path.basename(HEADER) in open(nsdp_build.__file__).read()
    assert nsdp_build.PER_FILE["chamfer.hip"] == nsdp_build.EXACT


def test_bad_arguments_return_status_before_any_launch(so):
    one = ctypes.c_void_p(16)      # (a non-null pointer the library must not touch)
    f32 = ctypes.c_float
    assert so.nsdp_chamfer_forward_workspace_bytes(0) == 0 and so.nsdp_chamfer_forward_workspace_bytes(65536) == 0
    assert so.nsdp_chamfer_forward_workspace_bytes(3) == 24 and so.nsdp_chamfer_forward_workspace_bytes(65535) == 8 * 65535

    def fwd(B=2, n=4, m=5, w=1.0, ptr=one, ws=one):
        return so.nsdp_chamfer_forward(ptr, ptr, B, n, m, f32(w), f32(1.0), ws, ptr, ptr, ptr, ptr, ptr, ptr, None)

    def bwd(B=2, n=4, m=5, w_list=1.0, ptr=one, lists=one, w_direct=1.0):
        return so.nsdp_chamfer_backward(ptr, ptr, ptr, lists, lists, ptr, B, n, m, f32(w_direct), f32(w_list), ptr, None)

    for call, name in ((fwd, b"chamfer_forward"), (bwd, b"chamfer_backward")):
        for kw, word in (({"B": 0}, b"batch"), ({"B": 65536}, b"batch"), ({"n": 0}, b"n=0"), ({"n": (1 << 20) + 1}, b"n=1048577"),
                         ({"m": 0}, b"m=0"), ({"m": (1 << 20) + 1}, b"m=1048577"), ({"B": 4096, "n": 1 << 20}, b"2^31"),
                         ({"ptr": None}, b"null")):
            assert call(**kw) == -1, kw
            assert word in so.nsdp_last_error() and name in so.nsdp_last_error(), (kw, so.nsdp_last_error())
        assert call(n=0, ptr=None) == -1 and b"n=0" in so.nsdp_last_error()      # sizes are judged before pointers
    assert fwd(w=float("nan")) == -1 and b"finite" in so.nsdp_last_error()
    assert fwd(ws=None) == -1 and b"null" in so.nsdp_last_error()
    assert fwd(ws=ctypes.c_void_p(20)) == -1 and b"aligned" in so.nsdp_last_error()
    assert bwd(w_direct=float("inf")) == -1 and b"finite" in so.nsdp_last_error()
    assert bwd(lists=None) == -1 and b"offsets" in so.nsdp_last_error()      # (without lists only where the list weight is 0)


# ------------------------------------------------------------------------------------------------------------- the refusals
def test_refusals_are_named():
    P, Q = _clouds(2, 6, 9, 1)
    assert "CPU tensors" in chamfer.refusal(P, Q)
    with pytest.raises(_lib.NsdpHipError, match="chamfer_loss: CPU tensors: pred is on the CPU"):
        chamfer.chamfer_loss(P, Q)
    assert "dtype: pred must be torch.float32, got torch.bfloat16" in chamfer.refusal(P.bfloat16(), Q)
    assert "dtype: target must be torch.float32, got torch.float64" in chamfer.refusal(P, Q.double())
    ragged = RaggedPoints.from_list([P[0], P[1]])
    why = chamfer.refusal(ragged, Q)
    assert "ragged inputs: pred is a RaggedPoints" in why and "training is rectangular" in why
    assert "ragged inputs: target is a RaggedPoints" in chamfer.refusal(P, ragged)
    assert "mismatched B: pred holds 2 shapes, target 3" in chamfer.refusal(P, _clouds(3, 6, 9, 2)[1])
    assert "shape: target must be [B, points, 3]" in chamfer.refusal(P, Q[:, :, :2])
    assert "shape: pred must be [B, points, 3]" in chamfer.refusal(P[0], Q)
    assert "limits: n = 0 points" in chamfer.refusal(P[:, :0], Q)
    assert "limits: m = 0 points" in chamfer.refusal(P, Q[:, :0])
    big = torch.empty((1, chamfer.MAX_POINTS + 1, 3), device="meta")
    assert "limits: m = 1048577 points" in chamfer.refusal(torch.empty((1, 4, 3), device="meta"), big)
    assert "limits: n = 1048577 points" in chamfer.refusal(big, torch.empty((1, 4, 3), device="meta"))
    assert "limits: B = 0 shapes" in chamfer.refusal(P[:0], Q[:0])
    assert "must be a torch.Tensor" in chamfer.refusal(P.numpy(), Q)
    for bad in (P.bfloat16(), ragged, P[:, :0]):
        with pytest.raises(_lib.NsdpHipError, match="chamfer_loss: "):
            chamfer.chamfer_loss(bad, Q)


# ---------------------------------------------------------------------------------------------------------- the config switch
def test_config_switch():
    from nsdp_amd.model.utils import compute_l2_error
    for cfg in ({}, None, {"model": {"type": "forward"}}, {"training": {}}, {"training": None}, {"training": {"loss": "l2"}},
                {"training": {"loss": "l2", "chamfer": {"w_pred_to_target": 3.0}}}):
        assert chamfer.training_loss(cfg) is compute_l2_error, cfg      # today's path: the very function
    fn = chamfer.training_loss({"training": {"loss": "chamfer"}})
    assert fn.func is chamfer.chamfer_loss and fn.keywords == {"w_pred_to_target": 1.0, "w_target_to_pred": 1.0}
    fn = chamfer.training_loss({"training": {"loss": "chamfer", "chamfer": {"w_pred_to_target": 0.5, "w_target_to_pred": 0}}})
    assert fn.keywords == {"w_pred_to_target": 0.5, "w_target_to_pred": 0.0}
    with pytest.raises(ValueError, match="'l1'.*l2.*chamfer"):
        chamfer.training_loss({"training": {"loss": "l1"}})
    with pytest.raises(ValueError, match="unknown keys \\['weight'\\]"):
        chamfer.training_loss({"training": {"loss": "chamfer", "chamfer": {"weight": 1.0}}})


def test_step_functions_read_the_configured_loss(monkeypatch):
    """_loss_with_cano, the FlowArbitrary loss function and both validate_on_batch_* hand the prediction to what the config names
    (a stand-in model on the CPU; the chamfer entry is replaced by a recorder, the l2 path runs as it is)."""
    from nsdp_amd.model import deformation_networks as dn, flow_arbitrary as fa
    from nsdp_amd.model.utils import compute_l2_error
    seen = []

    def recorder(pred, target, w_pred_to_target=1.0, w_target_to_pred=1.0, return_per_shape=False):
        seen.append((tuple(pred.shape), tuple(target.shape), w_pred_to_target, w_target_to_pred))
        return pred.sum() * 0 + 7.0

    monkeypatch.setattr(chamfer, "chamfer_loss", recorder)
    P, Q = _clouds(2, 6, 9, 3)
    data = {"space_samples_src": P, "surface_samples_inputs": torch.zeros(2, 4, 7), "space_samples_tgt": Q}
    same = dict(data, space_samples_tgt=P + 1.0)
    cano, arb = (lambda q, s, **kw: q * 2.0), (lambda q, a, b, c: q * 2.0)
    cfg = {"training": {"loss": "chamfer", "chamfer": {"w_target_to_pred": 0.25}}}
    assert float(dn._loss_with_cano(cano, data, cfg)) == 7.0 and float(fa._loss_with_arbitrary(arb, data, cfg)) == 7.0
    assert dn.validate_on_batch_with_cano(cano, data, cfg) == 7.0 and fa.validate_on_batch_with_arbitrary(arb, data, cfg) == 7.0
    assert seen == [((2, 6, 3), (2, 9, 3), 1.0, 0.25)] * 4
    want = float(compute_l2_error(P * 2.0, P + 1.0))
    for cfg in ({}, {"training": {"loss": "l2"}}):
        assert float(dn._loss_with_cano(cano, same, cfg)) == want and float(fa._loss_with_arbitrary(arb, same, cfg)) == want
        assert dn.validate_on_batch_with_cano(cano, same, cfg) == want
        assert fa.validate_on_batch_with_arbitrary(arb, same, cfg) == want
    assert len(seen) == 4


def test_synthetic_loader_yields_uncorresponded_targets():
    from nsdp_amd import train
    plain = train.SyntheticLoader(7, 2, 3, n_surf=16, n_query=40)
    loose = train.SyntheticLoader(7, 2, 3, n_surf=16, n_query=40, uncorresponded=25)
    full = train.SyntheticLoader(7, 2, 3, n_surf=16, n_query=40, uncorresponded=40)
    for a, b, c in zip(plain, loose, full):
        for key in ("surface_samples_inputs", "space_samples_src"):
            assert torch.equal(a[key], b[key]) and torch.equal(a[key], c[key])
        assert tuple(b["space_samples_tgt"].shape) == (3, 25, 3) and tuple(c["space_samples_tgt"].shape) == (3, 40, 3)
        for s in range(3):
            rows = {tuple(r) for r in a["space_samples_tgt"][s].tolist()}
            assert {tuple(r) for r in c["space_samples_tgt"][s].tolist()} == rows                 # a permutation of the rows
            assert {tuple(r) for r in b["space_samples_tgt"][s].tolist()} < rows                  # ... and a different count
            assert not torch.equal(c["space_samples_tgt"][s], a["space_samples_tgt"][s])
    for bad in (0, 41):
        with pytest.raises(ValueError, match="uncorresponded"):
            train.SyntheticLoader(7, 1, 1, n_surf=16, n_query=40, uncorresponded=bad)
