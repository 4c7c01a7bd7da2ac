"""Fused cross-attention decoder forward (no-grad path) over ``nsdp_decoder_fused_fwd``.

Reference: CrossTransformerDecoder.forward, model/decoder/crosstransformer_decoder.py:45-70 and
CrossTransformerBlock.forward, model/decoder/blocks.py:48-95.  The per-shape pieces (anchor key / value
tables, the global token: a few hundred rows) go through the ordinary HIP linear; everything that scales
with the number of query points (7-NN, 18 dense layers, the 8-token softmax) is one kNN launch and one fused
kernel launch.  There is no fallback: shapes the kernel was not built for raise.
"""
from __future__ import annotations

import contextlib
import ctypes

import torch
import torch.nn.functional as F

from . import _lib, hip_linear, pointnet2_utils, precision

import os

ENABLED = os.environ.get("NSDP_FUSED_DECODER", "1") != "0"   # off: the layer-by-layer kernels (debug / A-B timing)
MODES = ("f32", "bf16")


def _check_mode(name) -> str:
    if name not in MODES:
        raise ValueError(f"fused decoder dtype must be one of {MODES}, got {name!r}")
    return name


# Operand type of the fused kernel's matrix products.  "f32": nsdp_decoder_fused_fwd (the default, pinned to the oracle at 1e-4).
# "bf16": nsdp_decoder_fused_fwd_bf16 -- weights and layer inputs rounded to bf16 as MFMA operands only, everything else fp32;
# a different numerical contract (about 0.4 % relative on the decoder output), taken in either storage mode.  Read when a
# forward runs, so a captured graph (graph_step) keeps the kernel it was captured with.
MODE = _check_mode(os.environ.get("NSDP_FUSED_DECODER_DTYPE", "f32"))
# FlowArbitrary under MODE "bf16": network 1's decoder -- whose per-point outputs are the coordinates network 2 samples, groups
# and searches, so that its error is amplified by those discrete selections (nsdp_amd/precision.py, NSDP_BF16_NET1) -- keeps the
# fp32 kernel and only network 2's decoder takes the bf16-operand one.  "bf16": both do.
NET1_MODE = _check_mode(os.environ.get("NSDP_FUSED_DECODER_NET1", "f32"))


def set_mode(name: str) -> None:
    global MODE
    MODE = _check_mode(name)


@contextlib.contextmanager
def mode(name: str):
    """``with hip_decoder.mode("bf16"): ...`` -- the fused decoder's operand type inside the block, restored after it."""
    global MODE
    prev, MODE = MODE, _check_mode(name)
    try:
        yield
    finally:
        MODE = prev


def canonicalize_mode():
    """The context FlowArbitrary decodes its first network in (see NET1_MODE)."""
    return mode("f32") if (MODE == "bf16" and NET1_MODE == "f32") else contextlib.nullcontext()


def fused_for_inference() -> bool:
    """Does the no-grad forward of a supported decoder take a fused kernel?  The fp32 kernel needs fp32 storage (under bf16
    storage the layered bf16 path runs); the bf16-operand kernel is taken in either storage mode."""
    return ENABLED and (MODE == "bf16" or not precision.is_bf16())


DIM, HIDDEN, NBLOCKS, OUT = 200, 128, 5, 3
DP, HP = 208, 128            # channel counts padded to multiples of 16 (one MFMA tile)


def supported(decoder) -> bool:
    """The kernel is specialised for the one decoder geometry every NSDP configuration uses."""
    ct = decoder.ct1
    return (decoder.dim == DIM and decoder.init_enc.out_features == HIDDEN and decoder.n_blocks == NBLOCKS
            and decoder.fc_out.out_features == OUT and ct.reduce_dim and ct.nneigh >= 1)


def _pad2(w, rows, cols):
    return F.pad(w, (0, cols - w.shape[1], 0, rows - w.shape[0])).contiguous()


def _frag(w):
    """Row-major zero-padded [16*To, 16*Ti] -> fragment-major [To][Ti][lane = 16 g + li][4]: the 64 float4 one
    wave-wide MFMA A-operand load reads (row 16 to + li, columns 16 ti + 4 g .. + 3) become one contiguous KiB."""
    to, ti = w.shape[0] // 16, w.shape[1] // 16
    return w.view(to, 16, ti, 4, 4).permute(0, 2, 3, 1, 4).contiguous()


def _frag_bf16(w):
    """Row-major zero-padded [16*To, 16*Ti] -> the bf16 A-operand pack of nsdp_decoder_fused_fwd_bf16, [To, Ti*256] bf16
    (rounded to nearest even).  Per out tile: k blocks of two input tiles (2 kb, 2 kb + 1) as [lane = 16 g + li][8], element
    j < 4 = W[16 to + li][16 (2 kb) + 4 g + j], j >= 4 = W[16 to + li][16 (2 kb + 1) + 4 g + (j - 4)] -- hardware slot
    k = 8 g + j of v_mfma_f32_16x16x32_bf16, whose B operand in the same slot is the converted accumulator (tile, register
    j & 3) of the previous layer; then, for odd Ti, the last tile alone as [lane][4] (k = 4 g + j of the K = 16 instruction)."""
    to, ti = w.shape[0] // 16, w.shape[1] // 16
    wv = w.to(torch.bfloat16).view(to, 16, ti, 4, 4)                  # [to, li, tile, g, j]
    pairs = ti // 2
    parts = [wv[:, :, :2 * pairs].reshape(to, 16, pairs, 2, 4, 4)     # [to, li, kb, half, g, j]
             .permute(0, 2, 4, 1, 3, 5).reshape(to, pairs * 512)]      # [to, kb, g, li, half, j]
    if ti & 1:
        parts.append(wv[:, :, ti - 1].permute(0, 2, 1, 3).reshape(to, 256))   # [to, g, li, j]
    return torch.cat(parts, dim=1).contiguous()


def _pad1(b, n):
    return F.pad(b, (0, n - b.shape[0])).contiguous()


class _Pack:
    """Zero-padded copies of the decoder weights in the layout of include/nsdp_hip.h, rebuilt whenever a
    parameter changes (optimizer steps bump ``_version``; load_state_dict copies in place and bumps it too)."""

    def __init__(self, frag=_frag):
        self.frag = frag            # _frag: fp32 packs; _frag_bf16: the permuted bf16 packs of the bf16-operand kernel
        self.key = None
        self.tensors = None
        self.ptrs = None
        self.tables = None
        self.gamma_rows = None

    def get(self, dec):
        params = list(dec.parameters())
        key = tuple((p.data_ptr(), p._version) for p in params) + (hip_linear._weights_epoch,)
        if key == self.key:
            return self
        ct = dec.ct1
        _frag = self.frag
        with torch.no_grad():
            d0, d2 = ct.fc_delta[0], ct.fc_delta[2]
            g0, g2 = ct.fc_gamma[0], ct.fc_gamma[2]
            t = [
                _pad2(torch.cat([d0.weight, d0.bias[:, None]], dim=1), DP, 4),
                _frag(_pad2(d2.weight, DP, DP)), _pad1(d2.bias, DP),
                _frag(_pad2(g0.weight, DP, DP)), _pad1(g0.bias, DP),
                _frag(_pad2(g2.weight, DP, DP)), _pad1(g2.bias, DP),
                _frag(_pad2(dec.init_enc.weight, HP, DP)), _pad1(dec.init_enc.bias, HP),
                torch.stack([_frag(_pad2(l.weight, HP, DP)) for l in dec.fc_c]).contiguous(),
                torch.stack([_pad1(l.bias, HP) for l in dec.fc_c]).contiguous(),
                torch.stack([_frag(_pad2(b.fc_0.weight, HP, HP)) for b in dec.blocks]).contiguous(),
                torch.stack([_pad1(b.fc_0.bias, HP) for b in dec.blocks]).contiguous(),
                torch.stack([_frag(_pad2(b.fc_1.weight, HP, HP)) for b in dec.blocks]).contiguous(),
                torch.stack([_pad1(b.fc_1.bias, HP) for b in dec.blocks]).contiguous(),
                _frag(_pad2(dec.fc_out.weight, 16, HP)), _pad1(dec.fc_out.bias, 16),
            ]
            self.gamma_rows = (_pad2(g0.weight, DP, DP), _pad2(g2.weight, DP, DP))   # row-major, for the global token
            # projections producing the per-shape tables directly at the padded width
            self.tables = {
                "w_qs": _pad2(ct.w_qs.weight, DP, ct.w_qs.in_features),
                "w_ks": _pad2(ct.w_ks.weight, DP, ct.w_ks.in_features),
                "w_vs": _pad2(ct.w_vs.weight, DP, ct.w_vs.in_features),
                "w_kg": _pad2(ct.w_k_global.weight, DP, ct.w_k_global.in_features),
                "w_vg": _pad2(ct.w_v_global.weight, DP, ct.w_v_global.in_features),
            }
        self.tensors = t
        self.ptrs = (ctypes.c_void_p * len(t))(*[x.data_ptr() for x in t])
        self.key = key
        return self


def _setup(dec, encoding):
    """What both forms of the fused call share: the geometry check, the operand type, the weight pack of that type and the
    encoding as the fp32 table kernels want it.  -> (bf16, pack, z, anchors, feats, context the tables are built in)."""
    if not supported(dec):
        raise _lib.NsdpHipError("fused decoder: built for dim=200, hidden_dim=128, n_blocks=5, out_dim=3")
    z, anchors, feats = encoding["z"], encoding["anchors"], encoding["anchor_feats"]
    if z.dim() != 2:
        raise _lib.NsdpHipError("fused decoder: per-query latent codes are not used by any NSDP configuration")
    bf16 = MODE == "bf16"
    slot = "_fused_pack_bf16" if bf16 else "_fused_pack"
    pack = dec.__dict__.get(slot)
    if pack is None:
        pack = dec.__dict__[slot] = _Pack(_frag_bf16 if bf16 else _frag)
    pack = pack.get(dec)
    # bf16 storage (bf16-operand mode only): the encoding is upcast and the per-shape tables are built by the fp32 kernels
    tables_f32 = precision.storage(torch.float32) if precision.is_bf16() else contextlib.nullcontext()
    if precision.is_bf16():
        z, feats = z.float(), feats.float()
    return bf16, pack, z, anchors.contiguous().float(), feats, tables_f32


def _shape_tables(pack, z, feats):
    """The per-shape tables of the fused kernels (a few hundred rows, through the ordinary HIP linear): qk [B,A,DP], vtab
    [B,A,DP], a_g [B,DP], v_g [B,DP]."""
    tb = pack.tables
    lin = lambda x, w, *a, **k: hip_linear.linear(x, w, *a, pack_owner=w, **k)      # (constant tables: packs cached on them)
    q = lin(z, tb["w_qs"])                                                  # [B,DP] (pad channels = 0)
    k_g = lin(z, tb["w_kg"])
    v_g = lin(z, tb["w_vg"]).contiguous()
    kf = lin(feats, tb["w_ks"])                                             # [B,A,DP]
    vtab = lin(feats, tb["w_vs"]).contiguous()
    qk = (q.unsqueeze(1) - kf).contiguous()
    t = pack.tensors
    h = lin(q - k_g, pack.gamma_rows[0], t[4], relu_out=True)               # global-token logits
    a_g = lin(h, pack.gamma_rows[1], t[6]).contiguous()
    return qk, vtab, a_g, v_g


def decoder_forward(dec, xyz_q: torch.Tensor, encoding: dict) -> torch.Tensor:
    """xyz_q [B,NQ,3] + encoding {z [B,C], anchors [B,A,3], anchor_feats [B,A,C]} -> [B,NQ,3]."""
    return _decode(dec, xyz_q, encoding, False)


def _decode(dec, xyz_q, encoding, jacobian):
    """decoder_forward (-> out) and decoder_jacobian (-> (out, jac)): one setup, one search, one table build, one launch."""
    bf16, pack, z, anchors, feats, tables_f32 = _setup(dec, encoding)
    ct = dec.ct1
    B, NQ, _ = xyz_q.shape
    A = anchors.shape[1]
    xyz_q_in = xyz_q
    xyz_q = xyz_q.contiguous().float()
    with torch.no_grad(), _lib.on_device(xyz_q), tables_f32:
        idx = encoding.get("query_idx") if encoding.get("query_points") is xyz_q_in else None      # (searched ahead: Deformation_Networks.geometry)
        if idx is None:
            idx = pointnet2_utils.knn(xyz_q, anchors, ct.nneigh)                # [B,NQ,k] int32
        qk, vtab, a_g, v_g = _shape_tables(pack, z, feats)
        out = torch.empty(B, NQ, OUT, dtype=torch.float32, device=xyz_q.device)
        jac = torch.empty(B, NQ, OUT, 3, dtype=torch.float32, device=xyz_q.device) if jacobian else None
        name = "nsdp_decoder_jacobian_fwd" if jacobian else "nsdp_decoder_fused_fwd_bf16" if bf16 else "nsdp_decoder_fused_fwd"
        _lib.check(getattr(_lib.lib(), name)(
            _lib.fptr(xyz_q, "xyz_q"), _lib.fptr(anchors, "anchors"), _lib.iptr(idx, "idx"),
            _lib.fptr(qk, "qk"), _lib.fptr(vtab, "vtab"), _lib.fptr(a_g, "a_g"), _lib.fptr(v_g, "v_g"),
            pack.ptrs, len(pack.tensors), B, NQ, A, ct.nneigh, DIM, HIDDEN, _lib.fptr(out, "out"),
            *((_lib.fptr(jac, "jac"),) if jacobian else ()), _lib.stream_ptr()),
            name)
    return (out, jac) if jacobian else out


def ragged_refusal(dec):
    """Why a packed query set cannot be decoded right now (None: it can).  The packed form exists as the fused kernels alone
    -- there is no layered path to fall to -- so every condition under which the rectangular call would take the layers is a
    refusal here."""
    if torch.is_grad_enabled():
        return ("autograd is enabled: a packed (ragged) query set is decoded by the fused inference kernels only, which have "
                "no backward -- call under torch.no_grad()")
    if not ENABLED:
        return "the fused decoder is switched off (NSDP_FUSED_DECODER=0 / hip_decoder.ENABLED = False) and the layered decoder has no ragged form"
    if MODE != "bf16" and precision.is_bf16():
        return ("bf16 storage with the fp32 fused kernel (hip_decoder.MODE = 'f32'): the rectangular call runs the layered bf16 "
                "decoder there, which has no ragged form -- select the bf16-operand kernel (NSDP_FUSED_DECODER_DTYPE=bf16)")
    if not supported(dec):
        return "decoder geometry: the fused kernels are built for dim=200, hidden_dim=128, n_blocks=5, out_dim=3"
    return None


def decoder_forward_ragged(dec, points, encoding: dict, out=None):
    """``decoder_forward`` for a packed query set: points = RaggedPoints (packed [cap,3], offsets [B+1] on the device) + the
    encoding of B shapes -> RaggedPoints over [cap,3] (rows at or beyond offsets[B] are not written; ``out``: a [cap,3] buffer
    of the caller's).  One kNN launch and one fused launch whose grids follow cap and B alone -- nothing here reads the
    offsets on the host, so the call can be captured once and replayed for any mix of sizes.  No layered fallback."""
    why = ragged_refusal(dec)
    if why is not None:
        raise _lib.NsdpHipError("ragged decode refused: " + why)
    return _decode_ragged(dec, points, encoding, out, False)


def _decode_ragged(dec, points, encoding, out, jacobian, jac=None):
    """decoder_forward_ragged (-> out) and decoder_jacobian_ragged (-> (out, jac)) behind their refusals."""
    bf16, pack, z, anchors, feats, tables_f32 = _setup(dec, encoding)
    ct = dec.ct1
    xyz_q = points.packed.contiguous().float()
    cap, (B, A) = xyz_q.shape[0], anchors.shape[:2]
    if xyz_q.dim() != 2 or xyz_q.shape[1] != 3:
        raise _lib.NsdpHipError(f"ragged decode: packed points must be [cap, 3], got {tuple(xyz_q.shape)}")
    if points.batch != B:
        raise _lib.NsdpHipError(f"ragged decode: {points.batch} shapes of points against an encoding of {B}")
    with torch.no_grad(), _lib.on_device(xyz_q), tables_f32:
        if out is None:
            out = torch.empty(cap, OUT, dtype=torch.float32, device=xyz_q.device)
        elif tuple(out.shape) != (cap, OUT):
            raise _lib.NsdpHipError(f"ragged decode: out must be [{cap}, {OUT}], got {tuple(out.shape)}")
        if jacobian and jac is None:
            jac = torch.empty(cap, OUT * 3, dtype=torch.float32, device=xyz_q.device)
        elif jacobian and tuple(jac.shape) != (cap, OUT * 3):
            raise _lib.NsdpHipError(f"ragged decode: jac must be [{cap}, {OUT * 3}], got {tuple(jac.shape)}")
        if cap:
            idx = encoding.get("query_idx") if encoding.get("query_points") is points else None      # (searched ahead: Deformation_Networks.ragged_geometry)
            if idx is None:
                idx = pointnet2_utils.knn_ragged(xyz_q, points.offsets, anchors, ct.nneigh)      # [cap,k] int32
            elif tuple(idx.shape) != (cap, ct.nneigh):
                raise _lib.NsdpHipError(f"ragged decode: cached query_idx must be [{cap}, {ct.nneigh}], got {tuple(idx.shape)}")
            qk, vtab, a_g, v_g = _shape_tables(pack, z, feats)
            name = ("nsdp_decoder_jacobian_fwd_ragged" if jacobian else
                    "nsdp_decoder_fused_fwd_bf16_ragged" if bf16 else "nsdp_decoder_fused_fwd_ragged")
            _lib.check(getattr(_lib.lib(), name)(
                _lib.fptr(xyz_q, "xyz_q"), _lib.iptr(points.offsets, "offsets"), _lib.fptr(anchors, "anchors"), _lib.iptr(idx, "idx"),
                _lib.fptr(qk, "qk"), _lib.fptr(vtab, "vtab"), _lib.fptr(a_g, "a_g"), _lib.fptr(v_g, "v_g"),
                pack.ptrs, len(pack.tensors), B, cap, A, ct.nneigh, DIM, HIDDEN, _lib.fptr(out, "out"),
                *((_lib.fptr(jac, "jac"),) if jacobian else ()), _lib.stream_ptr()),
                name)
    return (points.like(out), points.like(jac)) if jacobian else points.like(out)


def jacobian_refusal(dec):
    """Why the deformation gradient cannot be computed right now (None: it can).  The Jacobian exists as the fp32 fused kernel
    alone (include/nsdp_jacobian.h): no layered path, no bf16-operand form, no backward."""
    if torch.is_grad_enabled():
        return ("autograd is enabled: the Jacobian is computed by a fused inference kernel in forward mode, which has no "
                "backward -- call under torch.no_grad()")
    if not ENABLED:
        return "the fused decoder is switched off (NSDP_FUSED_DECODER=0 / hip_decoder.ENABLED = False) and the layered decoder computes no Jacobian"
    if precision.is_bf16():
        return "bf16 storage: the Jacobian kernel runs on the fp32 weight pack in fp32 storage only"
    if MODE == "bf16":
        return ("bf16 mode (hip_decoder.MODE = 'bf16'): the bf16-operand kernel has no Jacobian form -- select the fp32 kernel "
                "(NSDP_FUSED_DECODER_DTYPE=f32)")
    if not supported(dec):
        return "decoder geometry: the fused kernels are built for dim=200, hidden_dim=128, n_blocks=5, out_dim=3"
    return None


def decoder_jacobian(dec, xyz_q: torch.Tensor, encoding: dict):
    """``decoder_forward`` together with the deformation gradient: -> (out [B,NQ,3], jac [B,NQ,3,3]), jac[..., i, j] =
    d out[..., i] / d xyz_q[..., j] with the neighbour indices held fixed (nsdp_decoder_jacobian_fwd).  ``out`` has the bits
    ``decoder_forward`` gives.  Refused with its reason where it cannot run (jacobian_refusal)."""
    why = jacobian_refusal(dec)
    if why is not None:
        raise _lib.NsdpHipError("decoder Jacobian refused: " + why)
    return _decode(dec, xyz_q, encoding, True)


def decoder_jacobian_ragged(dec, points, encoding: dict, out=None, jac=None):
    """``decoder_forward_ragged`` together with the deformation gradient: -> (RaggedPoints over [cap,3], RaggedPoints over
    [cap,9]: row-major 3x3 per row; rows at or beyond offsets[B] are not written; ``out`` / ``jac``: buffers of the caller's)."""
    why = jacobian_refusal(dec)
    if why is not None:
        raise _lib.NsdpHipError("decoder Jacobian refused: " + why)
    return _decode_ragged(dec, points, encoding, out, True, jac)
