"""CPU: the local-rigidity loss's yardstick against itself (tests/rigidity_ref.py: closed form against fp64 autograd), the
boundary of the feature -- include/nsdp_rigidity.h declares the entries and the built library exports them at ABI version 20,
bad arguments come back as a status with a message before anything could be launched --, the refusals of
``local_rigidity_loss`` and ``neighbour_sets`` by name, the config switch and the four step functions."""
import ctypes
import os
import re

import pytest
import torch

import rigidity_ref
from nsdp_amd import _lib, build as nsdp_build, rigidity
from nsdp_amd.ragged import RaggedPoints

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "nsdp_rigidity.h")
ENTRY_POINTS = ["nsdp_rigidity_backward", "nsdp_rigidity_forward", "nsdp_rigidity_forward_workspace_bytes"]


def _operands(B, n, K, seed):
    g = torch.Generator().manual_seed(seed)
    S = torch.randn(B, n, 3, generator=g)
    P = S + 0.3 * torch.randn(B, n, 3, generator=g)
    idx = torch.randint(0, n, (B, n, K), generator=g, dtype=torch.int64).int()
    return P, S, idx


# ------------------------------------------------------------------------------------------------------------ the yardstick
@pytest.mark.parametrize("B,n,K,w", [(3, 65, 8, 1.0), (1, 1, 1, 1.0), (2, 2, 7, 0.25), (1, 40, 32, 3.0)])
def test_closed_form_equals_fp64_autograd(B, n, K, w):
    P, S, idx = _operands(B, n, K, 100 * n + K)
    loss, dP = rigidity_ref.autograd64(P, S, idx, w)
    r = rigidity_ref.resid64(P, S, idx)[0]
    grad, mass, lengths = rigidity_ref.closed_form(P, idx, r, w)
    assert float((grad - dP).abs().max()) <= 1e-13 * float(mass.max()) + 1e-300
    assert bool((grad.abs() <= mass * (1 + 1e-12)).all())
    assert int(lengths.sum()) == B * n * K
    assert torch.equal(rigidity_ref.closed_form(P, idx, r, w, g=4.0)[0], 4.0 * grad)      # an upstream gradient scales it
    assert float(rigidity_ref.from_resid(r, w)[0]) == float(loss)
    assert float(loss) > 0 or n == 1


def test_yardstick_zero_cases_and_rigid_motions():
    P, S, idx = _operands(2, 33, 4, 7)
    assert float(rigidity_ref.loss64(S, S.clone(), idx)[0]) == 0.0
    own = torch.arange(33, dtype=torch.int32)[None, :, None].expand(2, 33, 4).contiguous()
    r, cur, rest = rigidity_ref.resid64(P, S, own)
    assert bool((r == 0).all()) and bool((cur == 0).all()) and bool((rest == 0).all())     # entries naming their own row
    q, _ = torch.linalg.qr(torch.randn(3, 3, dtype=torch.float64, generator=torch.Generator().manual_seed(1)))
    moved = S.double() @ q.T + torch.tensor([0.5, -2.0, 1.0], dtype=torch.float64)
    r, cur, rest = rigidity_ref.resid64(moved, S, idx)
    assert float((r.abs() / (cur + rest).clamp_min(1e-300)).max()) <= 1e-14                 # an isometry keeps every length


def test_depth_follows_the_documented_operation_order():
    T = torch.tensor([0, 1, 2, 32, 33, 64, 65, 1024, 1025, 8200, 100000])
    assert rigidity_ref.depth(T).tolist() == [0, 0, 1, 31, 6, 6, 7, 21, 12, 40, 398]
    assert rigidity_ref.envelope_c(T, 1).tolist() == [7.0 + d for d in rigidity_ref.depth(T).tolist()]
    assert rigidity_ref.envelope_c(T, 8).tolist() == [7.0 + max(7, d) for d in rigidity_ref.depth(T).tolist()]
    with open(HEADER) as f:
        text = f.read()
    for phrase in ("(depth K - 1)", "(depth T - 1)", "(depth ceil(T/64) + 5)", "(depth ceil(T/256) + 7)",
                   "(6 + max(K - 1, depth(T))) * 2^-24", "6 * 2^-24 * (cur + rest)"):
        assert phrase in text, phrase


# ------------------------------------------------------------------------------------------------------------- the boundary
@pytest.fixture(scope="module")
def so():
    if not os.path.exists(_lib.SO_PATH):
        nsdp_build.build()
    lib = ctypes.CDLL(_lib.SO_PATH)
    lib.nsdp_last_error.restype = ctypes.c_char_p
    lib.nsdp_rigidity_forward_workspace_bytes.restype = ctypes.c_size_t
    return lib


def test_header_declares_and_library_exports_the_entries(so):
    with open(HEADER) as f:
        text = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(nsdp_[a-z0-9_]+)\s*\(", text)))
    assert declared == ENTRY_POINTS
    for name in ENTRY_POINTS:
        assert hasattr(so, name), name
    assert so.nsdp_abi_version() >= 20
    assert not set(ENTRY_POINTS) & set(_lib.declared_symbols())          # (nsdp_hip.h keeps its own table of entries)
    assert os.path.basename(HEADER) in open(nsdp_build.__file__).read()
    assert nsdp_build.PER_FILE["rigidity.hip"] == nsdp_build.EXACT


def test_bad_arguments_return_status_before_any_launch(so):
    one = ctypes.c_void_p(16)      # (a non-null pointer the library must not touch)
    f32 = ctypes.c_float
    assert so.nsdp_rigidity_forward_workspace_bytes(0) == 0 and so.nsdp_rigidity_forward_workspace_bytes(65536) == 0
    assert so.nsdp_rigidity_forward_workspace_bytes(3) == 3 * 65 * 8 and so.nsdp_rigidity_forward_workspace_bytes(65535) == 65535 * 65 * 8

    def fwd(B=2, n=4, K=3, w=1.0, ptr=one, ws=one):
        return so.nsdp_rigidity_forward(ptr, ptr, ptr, B, n, K, f32(w), ws, ptr, ptr, ptr, None)

    def bwd(B=2, n=4, K=3, w=1.0, ptr=one, lists=one):
        return so.nsdp_rigidity_backward(ptr, ptr, ptr, lists, lists, ptr, B, n, K, f32(w), ptr, None)

    for call, name in ((fwd, b"rigidity_forward"), (bwd, b"rigidity_backward")):
        for kw, word in (({"B": 0}, b"batch"), ({"B": 65536}, b"batch"), ({"n": 0}, b"n=0"), ({"n": (1 << 20) + 1}, b"n=1048577"),
                         ({"K": 0}, b"K=0"), ({"K": 33}, b"K=33"), ({"B": 64, "n": 1 << 20, "K": 32}, b"2^31"),
                         ({"B": 65535, "n": 32769, "K": 1}, b"2^31"), ({"ptr": None}, b"null")):
            assert call(**kw) == -1, kw
            assert word in so.nsdp_last_error() and name in so.nsdp_last_error(), (kw, so.nsdp_last_error())
        assert call(n=0, ptr=None) == -1 and b"n=0" in so.nsdp_last_error()      # sizes are judged before pointers
        assert call(B=1, n=1 << 20, K=32, ptr=None) == -1 and b"null" in so.nsdp_last_error()      # (the largest shape is a size it takes)
        assert call(w=float("nan")) == -1 and b"finite" in so.nsdp_last_error()
        assert call(w=float("inf")) == -1 and b"finite" in so.nsdp_last_error()
    assert fwd(ws=None) == -1 and b"null" in so.nsdp_last_error()
    assert fwd(ws=ctypes.c_void_p(20)) == -1 and b"aligned" in so.nsdp_last_error()
    assert bwd(lists=None) == -1 and b"null" in so.nsdp_last_error()


# ------------------------------------------------------------------------------------------------------------- the refusals
def test_refusals_are_named():
    P, S, idx = _operands(2, 6, 3, 1)
    assert rigidity.refusal(P, S) is not None and "CPU tensors" in rigidity.refusal(P, S, idx)
    with pytest.raises(_lib.NsdpHipError, match="local_rigidity_loss: CPU tensors: pred is on the CPU"):
        rigidity.local_rigidity_loss(P, S, idx=idx)
    assert "dtype: pred must be torch.float32, got torch.bfloat16" in rigidity.refusal(P.bfloat16(), S, idx)
    assert "dtype: source must be torch.float32, got torch.float64" in rigidity.refusal(P, S.double(), idx)
    assert "dtype: idx must be torch.int32, got torch.int64" in rigidity.refusal(P, S, idx.long())
    ragged = RaggedPoints.from_list([P[0], P[1]])
    why = rigidity.refusal(ragged, S, idx)
    assert "ragged inputs: pred is a RaggedPoints" in why and "training is rectangular" in why
    assert "ragged inputs: source is a RaggedPoints" in rigidity.refusal(P, ragged, idx)
    assert "mismatched B: pred holds 2 shapes, source 3" in rigidity.refusal(P, _operands(3, 6, 3, 2)[1], idx)
    assert "mismatched n: pred holds 6 points per shape, source 5" in rigidity.refusal(P, S[:, :5], idx)
    assert "shape: source must be [B, points, 3]" in rigidity.refusal(P, S[:, :, :2], idx)
    assert "shape: pred must be [B, points, 3]" in rigidity.refusal(P[0], S, idx)
    assert "shape: idx must be [B, n, K] = [2, 6, K], got (2, 5, 3)" in rigidity.refusal(P, S, idx[:, :5])
    assert "shape: idx must be [B, n, K]" in rigidity.refusal(P, S, idx[:, :, 0])
    assert "limits: K = 0 neighbours" in rigidity.refusal(P, S, idx[:, :, :0])
    assert "limits: K = 33 neighbours" in rigidity.refusal(P, S, torch.zeros(2, 6, 33, dtype=torch.int32))
    assert "limits: n = 0 points" in rigidity.refusal(P[:, :0], S[:, :0], idx[:, :0])
    assert "limits: B = 0 shapes" in rigidity.refusal(P[:0], S[:0], idx[:0])
    big = torch.empty((1, rigidity.MAX_POINTS + 1, 3), device="meta")
    assert "limits: n = 1048577 points" in rigidity.refusal(big, big)
    full = torch.empty((64, 1 << 20, 3), device="meta")
    assert "limits: B * n * K = 2147483648" in rigidity.refusal(full, full, torch.empty((64, 1 << 20, 32), dtype=torch.int32, device="meta"))
    assert "must be a torch.Tensor" in rigidity.refusal(P.numpy(), S, idx)
    for bad in (P.bfloat16(), ragged, P[:, :0]):
        with pytest.raises(_lib.NsdpHipError, match="local_rigidity_loss: "):
            rigidity.local_rigidity_loss(bad, S, idx=idx)
    # the self-search: k + 1 columns must exist, within the loss's K
    with pytest.raises(_lib.NsdpHipError, match="neighbour_sets: limits: k \\+ 1 = 7 columns of the self-search exceed the n = 6 points"):
        rigidity.neighbour_sets(S, 6)
    with pytest.raises(_lib.NsdpHipError, match="neighbour_sets: limits: k = 33 neighbours"):
        rigidity.neighbour_sets(torch.zeros(1, 100, 3), 33)
    with pytest.raises(_lib.NsdpHipError, match="neighbour_sets: limits: k = 0 neighbours"):
        rigidity.neighbour_sets(S, 0)


# ---------------------------------------------------------------------------------------------------------- the config switch
def test_config_switch():
    for cfg in ({}, None, {"model": {"type": "forward"}}, {"training": {}}, {"training": None}, {"training": {"rigidity": None}},
                {"training": {"loss": "chamfer"}}):
        assert rigidity.training_regulariser(cfg) is None, cfg
    reg = rigidity.training_regulariser({"training": {"rigidity": {"weight": 0.5}}})
    assert callable(reg) and (reg.weight, reg.k) == (0.5, 8)
    reg = rigidity.training_regulariser({"training": {"loss": "chamfer", "rigidity": {"weight": 2, "k": 4}}})
    assert (reg.weight, reg.k) == (2.0, 4)
    with pytest.raises(ValueError, match="unknown keys \\['w'\\]"):
        rigidity.training_regulariser({"training": {"rigidity": {"weight": 1.0, "w": 2.0}}})
    with pytest.raises(ValueError, match="'weight' is required"):
        rigidity.training_regulariser({"training": {"rigidity": {"k": 4}}})
    with pytest.raises(ValueError, match="k = 33"):
        rigidity.training_regulariser({"training": {"rigidity": {"weight": 1.0, "k": 33}}})
    with pytest.raises(ValueError, match="must be a mapping"):
        rigidity.training_regulariser({"training": {"rigidity": 0.5}})


def test_step_functions_add_the_configured_regulariser(monkeypatch):
    """_loss_with_cano, the FlowArbitrary loss function and both validate_on_batch_* add the regulariser of the prediction
    against space_samples_src to the data term (a stand-in model on the CPU; the rigidity entry is replaced by a recorder, the
    l2 data term runs as it is).  Without the key they do not come near it."""
    from nsdp_amd.model import deformation_networks as dn, flow_arbitrary as fa
    from nsdp_amd.model.utils import compute_l2_error
    seen = []

    def recorder(pred, source, k=8, weight=1.0, idx=None, return_per_shape=False):
        seen.append((tuple(pred.shape), source, k, weight))
        return pred.sum() * 0 + 7.0

    monkeypatch.setattr(rigidity, "local_rigidity_loss", recorder)
    g = torch.Generator().manual_seed(3)
    P = torch.randn(2, 6, 3, generator=g)
    data = {"space_samples_src": P, "surface_samples_inputs": torch.zeros(2, 4, 7), "space_samples_tgt": P + 1.0}
    cano, arb = (lambda q, s, **kw: q * 2.0), (lambda q, a, b, c: q * 2.0)
    want = float(compute_l2_error(P * 2.0, P + 1.0))
    cfg = {"training": {"rigidity": {"weight": 0.25, "k": 3}}}
    total = float(compute_l2_error(P * 2.0, P + 1.0) + 7.0)
    assert float(dn._loss_with_cano(cano, data, cfg)) == total and float(fa._loss_with_arbitrary(arb, data, cfg)) == total
    assert dn.validate_on_batch_with_cano(cano, data, cfg) == total and fa.validate_on_batch_with_arbitrary(arb, data, cfg) == total
    assert len(seen) == 4 and all(s[0] == (2, 6, 3) and s[1] is P and s[2:] == (3, 0.25) for s in seen)
    monkeypatch.setattr(rigidity, "local_rigidity_loss", None)      # (without the key nothing may call it)
    for cfg in ({}, {"training": {"loss": "l2"}}, {"training": {"rigidity": None}}):
        assert float(dn._loss_with_cano(cano, data, cfg)) == want and float(fa._loss_with_arbitrary(arb, data, cfg)) == want
        assert dn.validate_on_batch_with_cano(cano, data, cfg) == want
        assert fa.validate_on_batch_with_arbitrary(arb, data, cfg) == want
    assert len(seen) == 4
