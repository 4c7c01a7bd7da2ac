"""CPU-only checks of the packed ("ragged") query sets (nsdp_amd.ragged): the RaggedPoints container, the three C entry
points at the library boundary, and the gfx950 assembly of the ragged decoder kernels (they exist and carry no scratch)."""
import ctypes
import os
import re
import shutil
import subprocess

import pytest
import torch

from nsdp_amd import _lib
from nsdp_amd import build as nsdp_build
from nsdp_amd.ragged import RaggedPoints, l2_error

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
ENTRY_POINTS = ("nsdp_knn_ragged", "nsdp_decoder_fused_fwd_ragged", "nsdp_decoder_fused_fwd_bf16_ragged")


def _shapes(counts, seed=0):
    g = torch.Generator().manual_seed(seed)
    return [torch.rand((n, 3), generator=g) for n in counts]


# ---- the container ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("counts,capacity", [((5, 3, 9), None), ((4, 0, 7), None), ((0, 2, 0), None), ((5, 3, 9), 40),
                                             ((1,), 1), ((3001, 0, 1, 15, 16, 17, 255, 256, 257), 4096)])
def test_from_list_split_padded_round_trip(counts, capacity):
    shapes = _shapes(counts)
    r = RaggedPoints.from_list(shapes, capacity=capacity)
    total = sum(counts)
    assert r.batch == len(counts) and r.capacity == (total if capacity is None else capacity) and r.total == total
    assert r.counts == tuple(counts)
    assert r.offsets.dtype == torch.int32 and r.offsets.tolist() == [sum(counts[:i]) for i in range(len(counts) + 1)]
    assert r.packed.shape == (r.capacity, 3) and torch.equal(r.packed[:total], torch.cat(shapes))
    assert not r.packed[total:].any()                       # (padding rows of a set packed here are zero)
    back = r.split()
    assert len(back) == len(counts)
    for a, b in zip(back, shapes):
        assert a.shape == b.shape and torch.equal(a, b)
    p = r.padded()
    assert p.shape == (len(counts), max(counts), 3)
    for b, n in enumerate(counts):
        assert torch.equal(p[b, :n], shapes[b]) and not p[b, n:].any()
    # and back from the padded form
    again = RaggedPoints.from_list([p[b, :n] for b, n in enumerate(counts)], capacity=capacity)
    assert torch.equal(again.packed, r.packed) and torch.equal(again.offsets, r.offsets)


def test_offsets_alone_carry_no_host_counts_until_asked():
    shapes = _shapes((4, 0, 7))
    r = RaggedPoints.from_list(shapes, capacity=16)
    bare = RaggedPoints(r.packed, r.offsets)
    assert bare._counts is None
    assert bare.batch == 3 and bare.capacity == 16          # (no read-back needed for these)
    assert bare._counts is None
    assert [t.shape[0] for t in bare.split()] == [4, 0, 7] and bare.counts == (4, 0, 7)
    # offsets that are not monotone or leave the buffer are read the way the kernels read them: clamped
    odd = RaggedPoints(r.packed, torch.tensor([0, 9, 3, 400], dtype=torch.int32))
    assert odd.counts == (9, 0, 7) and odd.total == 16


def test_like_keeps_the_offsets():
    r = RaggedPoints.from_list(_shapes((2, 5)), capacity=9)
    out = r.like(torch.ones(9, 3))
    assert out.offsets is r.offsets and out.counts == (2, 5) and out.capacity == 9
    with pytest.raises(ValueError, match="capacity"):
        r.like(torch.ones(8, 3))


def test_refusals():
    with pytest.raises(ValueError, match=r"\[n, 3\]"):
        RaggedPoints.from_list([torch.zeros(4, 3), torch.zeros(4, 2)])
    with pytest.raises(ValueError, match=r"\[n, 3\]"):
        RaggedPoints.from_list([torch.zeros(1, 4, 3)])
    with pytest.raises(ValueError, match="capacity"):
        RaggedPoints.from_list(_shapes((5, 6)), capacity=10)
    with pytest.raises(ValueError, match="no shapes"):
        RaggedPoints.from_list([])
    with pytest.raises(ValueError, match="int32"):
        RaggedPoints(torch.zeros(4, 3), torch.tensor([0, 4]))            # (int64 offsets)
    with pytest.raises(ValueError, match="counts"):
        RaggedPoints(torch.zeros(4, 3), torch.tensor([0, 4], dtype=torch.int32), counts=(5,))


def test_ragged_l2_error_is_the_mean_of_the_per_shape_errors():
    from nsdp_amd.model.utils import compute_l2_error
    counts = (7, 0, 3, 12)
    pred, tgt = _shapes(counts, 1), _shapes(counts, 2)
    rp = RaggedPoints.from_list(pred, capacity=30)
    rp.packed[sum(counts):] = float("nan")                  # (padding rows may hold anything)
    rt = RaggedPoints.from_list(tgt)
    want = torch.stack([compute_l2_error(p[None], t[None]) for p, t in zip(pred, tgt) if p.shape[0]]).mean()
    got = l2_error(rp, rt)
    assert torch.isfinite(got) and abs(float(got) - float(want)) < 1e-6


# ---- the library boundary -----------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def so():
    if not os.path.exists(_lib.SO_PATH):
        nsdp_build.build()
    lib = ctypes.CDLL(_lib.SO_PATH)
    lib.nsdp_last_error.restype = ctypes.c_char_p
    return lib


def test_header_declares_and_library_exports_the_ragged_entry_points(so):
    names = _lib.declared_symbols()
    for must in ENTRY_POINTS:
        assert must in names, must
        assert hasattr(so, must), must
    assert so.nsdp_abi_version() >= 9


def test_bad_arguments_return_status(so):
    # null pointers -> NSDP_EINVAL with a message
    assert so.nsdp_knn_ragged(None, None, None, 2, 64, 100, 7, None, None, None) == -1
    assert b"null" in so.nsdp_last_error()
    for name in ENTRY_POINTS[1:]:
        rc = getattr(so, name)(None, None, None, None, None, None, None, None, None, 17, 2, 64, 100, 7, 200, 128, None, None)
        assert rc == -1, name
        assert b"null" in so.nsdp_last_error()
    # nothing to do -> 0, before any pointer is looked at
    assert so.nsdp_knn_ragged(None, None, None, 0, 64, 100, 7, None, None, None) == 0
    assert so.nsdp_knn_ragged(None, None, None, 2, 0, 100, 7, None, None, None) == 0
    for name in ENTRY_POINTS[1:]:
        for B, cap in ((0, 64), (2, 0)):
            assert getattr(so, name)(None, None, None, None, None, None, None, None, None, 17, B, cap, 100, 7, 200, 128,
                                     None, None) == 0, (name, B, cap)


def test_python_mirrors_refuse_cpu_tensors():
    from nsdp_amd import hip_decoder, pointnet2_utils as pu
    r = RaggedPoints.from_list(_shapes((4, 5)))
    with pytest.raises(RuntimeError, match="GPU"):
        pu.knn_ragged(r.packed, r.offsets, torch.zeros(2, 16, 3), 7)

    from helpers import build_product, model_cfg
    model, _, _ = build_product(model_cfg("forward", [256, 64, 16]), 3, "cpu")
    dec = model.eval().decoder
    assert hip_decoder.supported(dec)
    enc = {"z": torch.zeros(2, 256), "anchors": torch.zeros(2, 16, 3), "anchor_feats": torch.zeros(2, 16, 256)}
    with torch.no_grad(), pytest.raises(RuntimeError, match="GPU"):
        hip_decoder.decoder_forward_ragged(dec, r, enc)
    with torch.no_grad(), pytest.raises(RuntimeError, match="GPU"):
        model.decode(r, enc)
    with pytest.raises(RuntimeError, match="autograd"):      # (and with autograd on the refusal names it)
        with torch.enable_grad():
            hip_decoder.decoder_forward_ragged(dec, r, enc)


# ---- the kernels, as compiled -------------------------------------------------------------------------------------------

def _asm(src):
    flags = [f for f in nsdp_build.COMMON if f not in ("-fPIC", "-Wall")] + nsdp_build.PER_FILE.get(src, nsdp_build.FAST)
    out = subprocess.run([HIPCC] + flags + ["-S", "--cuda-device-only", "-o", "-", os.path.join(ROOT, "nsdp_amd", "csrc", src)],
                         capture_output=True, text=True, check=True)
    return out.stdout


@pytest.mark.skipif(shutil.which(HIPCC) is None, reason="hipcc not available")
@pytest.mark.parametrize("src,dense,ragged", [
    ("decoder_fused.hip", r"decoder_fused_fwd_kernelILb0E", r"decoder_fused_fwd_kernelILb1E"),      # two instantiations
    ("decoder_fused_bf16.hip", r"decoder_fused_fwd_bf16_kernelE", r"decoder_fused_ragged_bf16_kernelE")])      # two kernels
def test_ragged_decoder_kernels_exist_and_carry_no_scratch(src, dense, ragged):
    """Both operand types: the ragged kernel is in the gfx950 assembly beside the rectangular one, is the same MFMA chain
    (as many matrix instructions) and holds no scratch_ instruction -- the chain keeps three 52-register vectors live at the
    256-VGPR limit, a per-lane shape index would spill it."""
    lines = _asm(src).split("\n")
    found = {}
    for name in (dense, ragged):
        starts = [i for i, l in enumerate(lines) if re.match(r"^_Z\w*" + name + r"\w*:", l)]
        assert len(starts) == 1, (src, name, len(starts))
        body = lines[starts[0]:]
        ends = [i for i, l in enumerate(body) if l.startswith(".Lfunc_end")]
        assert ends, (src, name)
        found[name] = body[:ends[0]]
    for name, body in found.items():
        scratch = [l.strip() for l in body if "scratch_" in l]
        assert not scratch, (src, name, scratch[:3])
    mfma = {name: sum("v_mfma" in l for l in body) for name, body in found.items()}
    assert mfma[dense] > 100 and mfma[ragged] == mfma[dense], (src, mfma)
    # the ragged form makes the shape index uniform before it forms the table bases
    assert any("v_readfirstlane_b32" in l for l in found[ragged]), src
