"""CPU-only checks of the bf16-operand fused decoder (nsdp_decoder_fused_fwd_bf16, hip_decoder.MODE = "bf16"): the weight
pack's k permutation against an index-level model of the two MFMA instructions, the mode plumbing, the export and the assembly
audit of its translation unit."""
import ctypes
import os
import re
import shutil

import numpy as np
import pytest
import torch

from nsdp_amd import _lib, hip_decoder


def _bf16_rne(x):
    """fp32 -> bf16 (as float64 values), round to nearest even, by integer arithmetic on the bits (finite inputs only):
    independent of torch's conversion."""
    u = np.asarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    r = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16) << 16
    return r.astype(np.uint32).view(np.float32).astype(np.float64)


def _values(rng, shape):
    """sign * [0.25, 4): products of two bf16 values span 8 binades, so a 208-term sum is exact in fp64 in any order."""
    return (rng.uniform(0.25, 4.0, size=shape) * rng.choice([-1.0, 1.0], size=shape)).astype(np.float32)


def _mfma_16x16x32(a_frag, b_frag):
    """v_mfma_f32_16x16x32_bf16 with zero C: lane l holds A[row l&15][k = 8(l>>4)+j] and B[k = 8(l>>4)+j][col l&15], j < 8;
    returns D as [lane][reg] with col = l&15, row = 4(l>>4) + reg."""
    return _mfma(a_frag, b_frag, 8)


def _mfma_16x16x16(a_frag, b_frag):
    """v_mfma_f32_16x16x16_bf16: k = 4(l>>4)+j, j < 4; the same C/D layout."""
    return _mfma(a_frag, b_frag, 4)


def _mfma(a_frag, b_frag, n):
    A = np.zeros((16, 4 * n)); B = np.zeros((4 * n, 16))
    for l in range(64):
        for j in range(n):
            A[l & 15, n * (l >> 4) + j] = a_frag[l, j]
            B[n * (l >> 4) + j, l & 15] = b_frag[l, j]
    D = A @ B
    out = np.zeros((64, 4))
    for l in range(64):
        for r in range(4):
            out[l, r] = D[4 * (l >> 4) + r, l & 15]
    return out


@pytest.mark.parametrize("ti", [13, 8])
def test_frag_bf16_matches_an_index_level_model_of_the_instruction(ti):
    rng = np.random.default_rng(100 + ti)
    to = 3
    W = _values(rng, (16 * to, 16 * ti))
    X = _values(rng, (16 * ti, 16))                     # [channel][query row]: the activation of 16 rows
    pack = hip_decoder._frag_bf16(torch.from_numpy(W))
    assert pack.dtype is torch.bfloat16 and tuple(pack.shape) == (to, ti * 256) and pack.is_contiguous()
    pk = pack.float().numpy().astype(np.float64)
    # the previous layer's accumulators: lane (li, g) holds channels 16 t + 4 g + r of row li in register r of tile t
    acc = np.zeros((ti, 64, 4), dtype=np.float32)
    for t in range(ti):
        for l in range(64):
            for r in range(4):
                acc[t, l, r] = X[16 * t + 4 * (l >> 4) + r, l & 15]
    accb = _bf16_rne(acc)                               # C -> B: v_cvt_pk_bf16_f32, element order kept
    Y = np.zeros((16 * to, 16))
    for o in range(to):
        d = np.zeros((64, 4))
        for kb in range(ti // 2):
            a_frag = pk[o, kb * 512:(kb + 1) * 512].reshape(64, 8)
            b_frag = np.concatenate([accb[2 * kb], accb[2 * kb + 1]], axis=1)       # tile 2 kb then tile 2 kb + 1
            d += _mfma_16x16x32(a_frag, b_frag)
        if ti & 1:
            base = (ti // 2) * 512
            d += _mfma_16x16x16(pk[o, base:base + 256].reshape(64, 4), accb[ti - 1])
        for l in range(64):
            for r in range(4):
                Y[16 * o + 4 * (l >> 4) + r, l & 15] = d[l, r]
    want = _bf16_rne(W) @ _bf16_rne(X)
    assert np.array_equal(Y, want)


def test_mode_plumbing():
    assert hip_decoder.MODE == os.environ.get("NSDP_FUSED_DECODER_DTYPE", "f32")
    before = hip_decoder.MODE
    with hip_decoder.mode("bf16"):
        assert hip_decoder.MODE == "bf16"
        with hip_decoder.mode("f32"):
            assert hip_decoder.MODE == "f32"
        assert hip_decoder.MODE == "bf16"
    assert hip_decoder.MODE == before
    with pytest.raises(RuntimeError):
        with hip_decoder.mode("bf16"):
            raise RuntimeError("restored on the way out")
    assert hip_decoder.MODE == before
    for bad in ("fp16", "BF16", "", None):
        with pytest.raises(ValueError):
            hip_decoder.set_mode(bad)
        with pytest.raises(ValueError):
            with hip_decoder.mode(bad):
                pass
    assert hip_decoder.MODE == before
    try:
        hip_decoder.set_mode("bf16")
        assert hip_decoder.MODE == "bf16"
    finally:
        hip_decoder.set_mode(before)


def test_default_mode_is_f32_in_a_fresh_interpreter():
    import subprocess
    import sys
    env = {k: v for k, v in os.environ.items() if k != "NSDP_FUSED_DECODER_DTYPE"}
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = "from nsdp_amd import hip_decoder; print(hip_decoder.MODE)"
    out = subprocess.run([sys.executable, "-c", code], cwd=root, env=env, capture_output=True, text=True, timeout=300)
    assert out.stdout.strip() == "f32", out.stderr[-400:]
    out = subprocess.run([sys.executable, "-c", code], cwd=root, env=dict(env, NSDP_FUSED_DECODER_DTYPE="bf16"),
                         capture_output=True, text=True, timeout=300)
    assert out.stdout.strip() == "bf16", out.stderr[-400:]
    out = subprocess.run([sys.executable, "-c", code], cwd=root, env=dict(env, NSDP_FUSED_DECODER_DTYPE="half"),
                         capture_output=True, text=True, timeout=300)
    assert out.returncode != 0 and "ValueError" in out.stderr


def test_infer_parser_accepts_the_decoder_dtype():
    from nsdp_amd import infer
    ap = infer.build_parser()
    assert ap.parse_args(["cfg.yaml"]).decoder_dtype is None
    assert ap.parse_args(["cfg.yaml", "--decoder-dtype", "bf16", "--gpus", "2"]).decoder_dtype == "bf16"
    assert ap.parse_args(["cfg.yaml", "--decoder-dtype", "f32"]).decoder_dtype == "f32"
    with pytest.raises(SystemExit):
        ap.parse_args(["cfg.yaml", "--decoder-dtype", "fp16"])


def test_library_exports_the_bf16_decoder():
    assert "nsdp_decoder_fused_fwd_bf16" in _lib.declared_symbols()
    if not os.path.exists(_lib.SO_PATH):
        from nsdp_amd import build
        build.build()
    so = ctypes.CDLL(_lib.SO_PATH)
    assert hasattr(so, "nsdp_decoder_fused_fwd_bf16")
    assert so.nsdp_abi_version() >= 8
    so.nsdp_prof_name.restype = ctypes.c_char_p
    names = [so.nsdp_prof_name(k).decode() for k in range(so.nsdp_prof_num_kinds())]
    assert names[-1] == "decoder_fwd_bf16_kernel" and names.index("decoder_fwd_kernel") == 9      # appended, not renumbered
    # bad arguments come back as a status, as for every entry point
    so.nsdp_last_error.restype = ctypes.c_char_p
    assert so.nsdp_decoder_fused_fwd_bf16(None, None, None, None, None, None, None, None, 17, 1, 16, 4, 7, 200, 128,
                                          None, None) == -1
    assert b"null" in so.nsdp_last_error()


from test_no_inflight_spills import HIPCC, _asm, _parked_loads  # noqa: E402  (the audit's helpers, applied to the new file)


@pytest.mark.skipif(shutil.which(HIPCC) is None, reason="hipcc not available")
def test_bf16_decoder_kernel_has_no_scratch_and_parks_no_load_in_flight():
    """decoder_fused_bf16.hip issues its weight-fragment loads by hand, like decoder_fused.hip: it must compile for gfx950 with
    no scratch at all, and no destination of a hand-issued load may be copied to an AGPR before its wait."""
    _, text = _asm(("decoder_fused_bf16.hip", None))
    lines = text.split("\n")
    starts = [i for i, l in enumerate(lines) if re.match(r"^_Z\w*decoder_fused_fwd_bf16_kernel\w*:", l)]
    assert len(starts) == 1
    body = lines[starts[0]:]
    ends = [i for i, l in enumerate(body) if l.startswith(".Lfunc_end")]
    body = body[:ends[0]]
    assert not [l.strip() for l in body if "scratch_" in l]
    text = "\n".join(body)
    assert len(re.findall(r"v_mfma_f32_16x16x32_bf16", text)) >= 398       # 3 x 78 per slot + 48 + 48 + 32 + 32 + 4
    assert len(re.findall(r"v_mfma_f32_16x16x16_bf16", text)) >= 55        # the odd 13th tile: 3 x 13 + 8 + 8
    assert len(re.findall(r"v_mfma_f32_16x16x4_f32", text)) >= 13          # fc_delta.0 stays fp32
    assert "v_cvt_pk_bf16_f32" in text
    bad = _parked_loads(body, 0, len(body), hand_issued_only=True)
    assert not bad, bad[:3]
