"""CPU: the boundary of the deformation gradient -- include/nsdp_jacobian.h declares the two entries and the built library exports
them at ABI version 19, outside nsdp_hip.h's table; bad arguments come back as a status with the entry's name before anything
could be launched --, the helpers of nsdp_amd.deformation_gradient, and the yardstick against itself (tests/decoder_jac_ref.py:
fp64 autograd against fp64 central differences away from ReLU kinks)."""
import ctypes
import math
import os
import re

import pytest
import torch

import decoder_jac_ref as ref
from nsdp_amd import _lib, build as nsdp_build, deformation_gradient as dg
from nsdp_amd.ragged import RaggedPoints

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "nsdp_jacobian.h")
ENTRY_POINTS = ["nsdp_decoder_jacobian_fwd", "nsdp_decoder_jacobian_fwd_ragged"]


# ------------------------------------------------------------------------------------------------------------- the boundary
@pytest.fixture(scope="module")
def so():
    if not os.path.exists(_lib.SO_PATH):
        nsdp_build.build()
    lib = ctypes.CDLL(_lib.SO_PATH)
    lib.nsdp_last_error.restype = ctypes.c_char_p
    return lib


def test_header_declares_and_library_exports_the_entries(so):
    with open(HEADER) as f:
        text = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(nsdp_[a-z0-9_]+)\s*\(", text)))
    assert declared == ENTRY_POINTS
    for name in ENTRY_POINTS:
        assert hasattr(so, name), name
    assert so.nsdp_abi_version() >= 19
    assert not set(ENTRY_POINTS) & set(_lib.declared_symbols())          # (nsdp_hip.h keeps its own table of entries)
    assert os.path.basename(HEADER) in open(nsdp_build.__file__).read()
    assert "decoder_jacobian.hip" in nsdp_build.sources()
    assert nsdp_build.PER_FILE.get("decoder_jacobian.hip", nsdp_build.FAST) == nsdp_build.PER_FILE.get("decoder_fused.hip", nsdp_build.FAST)


def test_bad_arguments_return_status_before_any_launch(so):
    one = ctypes.c_void_p(16)      # (a non-null pointer the library must not touch)
    weights = (ctypes.c_void_p * 17)(*([16] * 17))

    def rect(B=2, NQ=4, A=8, D=200, H=128, nw=17, ptr=one, jac=one, w=weights):
        return so.nsdp_decoder_jacobian_fwd(ptr, ptr, ptr, ptr, ptr, ptr, ptr, w, nw, B, NQ, A, 7, D, H, ptr, jac, None)

    def ragged(B=2, cap=4, A=8, D=200, H=128, nw=17, ptr=one, jac=one, w=weights, offsets=one):
        return so.nsdp_decoder_jacobian_fwd_ragged(ptr, offsets, ptr, ptr, ptr, ptr, ptr, ptr, w, nw, B, cap, A, 7, D, H, ptr, jac, None)

    for call, name in ((rect, b"decoder_jacobian_fwd"), (ragged, b"decoder_jacobian_fwd_ragged")):
        for kw, word in (({"D": 96}, b"dim=200"), ({"H": 64}, b"hidden_dim=128"), ({"nw": 16}, b"17 packed weight pointers"),
                         ({"ptr": None}, b"null"), ({"jac": None}, b"null"), ({"w": None}, b"null"), ({"B": 65536}, b"batch")):
            assert call(**kw) == -1, kw
            assert word in so.nsdp_last_error() and name in so.nsdp_last_error(), (kw, so.nsdp_last_error())
    assert ragged(offsets=None) == -1 and b"decoder_jacobian_fwd_ragged: null pointer (offsets)" in so.nsdp_last_error()
    assert ragged(A=0) == -1 and b"decoder_jacobian_fwd_ragged: no anchors" in so.nsdp_last_error()
    # nothing to do is not an error, and touches nothing (as the forward entries)
    assert rect(NQ=0, ptr=None) == 0 and rect(B=0) == 0 and ragged(cap=0, ptr=None) == 0


# --------------------------------------------------------------------------------------------------------------- the helpers
def _rotation(axis, angle):
    axis = torch.tensor(axis, dtype=torch.float64)
    axis = axis / axis.norm()
    K = torch.tensor([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]], dtype=torch.float64)
    return torch.eye(3, dtype=torch.float64) + math.sin(angle) * K + (1 - math.cos(angle)) * (K @ K)


def test_cofactor_determinant_and_normals():
    g = torch.Generator().manual_seed(3)
    J = torch.randn(2, 5, 3, 3, generator=g, dtype=torch.float64)
    det = dg.determinant(J)
    assert torch.allclose(det, torch.linalg.det(J), rtol=1e-12, atol=1e-12)
    eye = torch.eye(3, dtype=torch.float64)
    assert torch.allclose(J.transpose(-1, -2) @ dg.cofactor(J), det[..., None, None] * eye, atol=1e-12)
    assert torch.allclose(dg.cofactor(J), det[..., None, None] * torch.linalg.inv(J).transpose(-1, -2), atol=1e-10)
    # a rotation carries a normal as itself
    R = _rotation([1.0, 2.0, -0.5], 0.7)
    n = torch.nn.functional.normalize(torch.randn(6, 3, generator=g, dtype=torch.float64), dim=-1)
    assert torch.allclose(dg.transform_normals(R.expand(6, 3, 3), n), n @ R.T, atol=1e-14)
    # a stretch along x tilts the normal of a slanted face away from x
    S = torch.diag(torch.tensor([2.0, 1.0, 1.0], dtype=torch.float64))
    got = dg.transform_normals(S, torch.tensor([1.0, 1.0, 0.0], dtype=torch.float64) / math.sqrt(2))
    assert torch.allclose(got, torch.tensor([1.0, 2.0, 0.0], dtype=torch.float64) / math.sqrt(5), atol=1e-15)
    # singular J: no inverse is formed, the result is finite (rank 2: still a direction; rank <= 1: the zero vector)
    flat = torch.diag(torch.tensor([1.0, 1.0, 0.0]))
    assert torch.equal(dg.transform_normals(flat, torch.tensor([0.0, 0.0, 1.0])), torch.tensor([0.0, 0.0, 1.0]))
    for sing in (torch.zeros(3, 3), torch.ones(3, 3), flat):
        assert torch.isfinite(dg.transform_normals(sing, torch.tensor([0.6, 0.0, 0.8]))).all()
        assert float(dg.determinant(sing)) == 0.0
    with pytest.raises(ValueError, match=r"\[\.\.\., 3, 3\]"):
        dg.cofactor(torch.zeros(4, 9))


def test_fold_overs_counts_per_shape_and_compose_is_a_matmul():
    eye = torch.eye(3)
    flip = torch.diag(torch.tensor([1.0, -1.0, 1.0]))      # det -1: a fold-over
    flat = torch.diag(torch.tensor([1.0, 0.0, 1.0]))       # det 0 counts
    J = torch.stack([torch.stack([eye, flip, eye, flat]), torch.stack([eye, eye, eye, eye])])
    assert dg.fold_overs(J).tolist() == [2, 0]
    # packed: counts [3, 0, 2] in a capacity of 7; the padding rows hold fold-overs that must not be counted
    rows = torch.stack([flip, eye, flip, eye, flat, flip, flip])
    offsets = torch.tensor([0, 3, 3, 5], dtype=torch.int32)
    assert dg.fold_overs(rows, offsets).tolist() == [2, 0, 1]
    packed = RaggedPoints(rows.reshape(7, 9), offsets)
    assert dg.fold_overs(packed).tolist() == [2, 0, 1]
    assert dg.determinant(packed).shape == (7,)
    g = torch.Generator().manual_seed(4)
    A, B = torch.randn(2, 3, 3, 3, generator=g), torch.randn(2, 3, 3, 3, generator=g)
    assert torch.equal(dg.compose(A, B), A @ B)
    pa, pb = RaggedPoints(torch.randn(7, 9, generator=g), offsets), RaggedPoints(torch.randn(7, 9, generator=g), offsets)
    pc = dg.compose(pa, pb)
    assert isinstance(pc, RaggedPoints) and pc.offsets is offsets
    assert torch.equal(pc.packed, (pa.packed.view(7, 3, 3) @ pb.packed.view(7, 3, 3)).reshape(7, 9))


def test_infer_command_refuses_what_has_no_jacobian(capsys):
    """``python -m nsdp_amd.infer ... --jacobian`` names its refusals before anything is built or a GPU is asked for."""
    from nsdp_amd import infer
    for extra, word in ((["--gpus", "2"], "runs on one GPU"), (["--decoder-dtype", "bf16"], "bf16-operand decoder kernel has no Jacobian"),
                        (["--graph"], "eager step"), (["--surface-counts", "64,32"], "eager step")):
        with pytest.raises(SystemExit) as e:
            infer.main(["no_such_config.yaml", "--jacobian"] + extra)
        assert "--jacobian" in str(e.value.code) and word in str(e.value.code), (extra, e.value.code)


# ------------------------------------------------------------------------------------------------------------- the yardstick
def test_fp64_autograd_agrees_with_fp64_central_differences_away_from_kinks():
    """h = 1e-7 keeps a central-difference stencil inside one linear piece for every query whose kink distance exceeds 1e-5
    (pre-activations move by at most |W| h << 1e-5); there the two agree to 1e-6 relative, per query."""
    _, state = ref.decoder(11)
    sd = {k: torch.from_numpy(v) for k, v in state.items()}
    xyz_q, anchors, feats, z = (torch.from_numpy(a).double() for a in ref.inputs(5, 2, 96, 16))
    enc = {"z": z, "anchors": anchors, "anchor_feats": feats}
    idx = ref.knn_idx(xyz_q, anchors, ref.KW["nneigh"])
    out, J, kink = ref.value_jacobian_kink(sd, xyz_q, enc, idx)
    assert out.dtype is torch.float64 and J.shape == (2, 96, 3, 3) and kink.shape == (2, 96)
    fd = ref.central_differences(sd, xyz_q, enc, idx, 1e-7)
    err = ref.rel_frobenius(fd, J)
    clear = kink > 1e-5
    assert int(clear.sum()) >= 0.7 * clear.numel(), "too few queries away from a kink to say anything"
    assert float(err[clear].max()) <= 1e-6, float(err[clear].max())
    assert not torch.allclose(J, J.transpose(-1, -2), rtol=1e-3, atol=0)      # J is not symmetric: [i, j] is pinned by fd
    # the restatement is the oracle's decoder where that one searches the same neighbours
    from oracle import tdnet_ref
    want = tdnet_ref.cross_transformer_decoder(tdnet_ref._SD({k: v.double() for k, v in sd.items()}, "", False), xyz_q, enc, ref.KW)
    assert float((out - want).abs().max()) <= 1e-12
