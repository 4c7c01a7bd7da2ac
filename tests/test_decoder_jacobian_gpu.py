"""GPU: the deformation gradient of the fused decoder (nsdp_decoder_jacobian_fwd, include/nsdp_jacobian.h).  The value keeps the
bits of the fused forward; J agrees per query with fp64 autograd of the torch restatement (tests/decoder_jac_ref.py) on the
kernel's own neighbour indices; the packed form gives every row the rectangular call's bits and leaves the padding alone; the
step functions carry it to ``verts_tgt_jacobian``; the refusals are named; both entries stay inside their operands in the
poisoned arena."""
import contextlib
import ctypes

import numpy as np
import pytest
import torch

import decoder_jac_ref as ref
from helpers import build_product, model_cfg, to_dev
from nsdp_amd import _lib, deformation_gradient as dg, hip_decoder, pointnet2_utils as pu, precision, synth
from nsdp_amd.ragged import RaggedPoints

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)

# per-query relative Frobenius bound: the project's oracle-parity bound of this kernel's values, applied per query
BOUND = 1e-4
# a query may miss BOUND only if its fp64 kink distance is below this (a rounding-level sign flip of a pre-activation changes a
# ReLU mask), and at most this share of a case may be excused
EXCUSE_KINK, EXCUSE_SHARE = 1e-6, 0.03
CANARY = -7.5


@pytest.fixture(autouse=True)
def _fp32_fused():
    """The Jacobian exists in fp32 storage with the fused decoder on; the process's knobs are put back behind each test."""
    with contextlib.ExitStack() as cfg:
        cfg.enter_context(precision.storage(torch.float32))
        cfg.enter_context(hip_decoder.mode("f32"))
        cfg.callback(setattr, hip_decoder, "ENABLED", hip_decoder.ENABLED)
        hip_decoder.ENABLED = True
        yield


def _t(a):
    return torch.from_numpy(a)


def _case(B, NQ, A, nneigh=7):
    dec, state = ref.decoder(11, nneigh=nneigh)
    dec = dec.to(DEV)
    xyz_q, anchors, feats, z = ref.inputs(5, B, NQ, A)
    enc = {"z": _t(z).to(DEV), "anchors": _t(anchors).to(DEV), "anchor_feats": _t(feats).to(DEV)}
    q = _t(xyz_q).to(DEV)
    idx = pu.knn(q, enc["anchors"], nneigh)                       # the kernel's own search, shared by every call below
    enc.update(query_idx=idx, query_points=q)
    cpu = {"sd": {k: _t(v) for k, v in state.items()}, "xyz_q": _t(xyz_q),
           "enc": {"z": _t(z), "anchors": _t(anchors), "anchor_feats": _t(feats)}}
    return dec, q, enc, idx, cpu


def _first_difference(a, b):
    rows = (a != b).reshape(a.shape[0], -1).any(-1).nonzero().flatten()
    return f"{rows.numel()} rows differ, first: {rows[:8].tolist()}"


# (1,1,7): one query, a partial tile; (2,5,16): a full tile plus a tile of one; (3,329,32): 83 tiles -- the last workgroup's
# second wave is surplus; (2,2048,16): queries enough for the share of excusable misses to mean something
@pytest.mark.parametrize("B,NQ,A,nneigh", [(1, 1, 7, 7), (2, 5, 16, 7), (3, 329, 32, 7), (2, 2048, 16, 7), (2, 5, 16, 1), (2, 5, 16, 3)])
def test_value_keeps_its_bits_and_jacobian_matches_fp64_autograd(B, NQ, A, nneigh):
    dec, q, enc, idx, cpu = _case(B, NQ, A, nneigh)
    with torch.no_grad():
        want = hip_decoder.decoder_forward(dec, q, enc)
        out, jac = hip_decoder.decoder_jacobian(dec, q, enc)
        via_module = dec(q, enc, jacobian=True)
    assert out.shape == (B, NQ, 3) and jac.shape == (B, NQ, 3, 3) and jac.dtype is torch.float32
    # asking for the Jacobian does not move a vertex
    assert torch.equal(out, want), _first_difference(out.reshape(-1, 3), want.reshape(-1, 3))
    assert torch.equal(via_module[0], out) and torch.equal(via_module[1], jac)
    assert bool(torch.isfinite(jac).all())
    _, J64, kink = ref.value_jacobian_kink(cpu["sd"], cpu["xyz_q"].double(), cpu["enc"], idx.cpu())
    err = ref.rel_frobenius(jac.cpu(), J64)
    miss = err > BOUND
    excusable = kink < EXCUSE_KINK
    worst_pass = float(err[~miss].max()) if bool((~miss).any()) else 0.0
    print(f"\n(B, NQ, A, k) = {(B, NQ, A, nneigh)}: {int(miss.sum())} of {miss.numel()} queries miss {BOUND:g} "
          f"({int((miss & excusable).sum())} excused, kink < {EXCUSE_KINK:g}); worst passing error {worst_pass:.3e}, "
          f"median {float(err.median()):.3e}; queries with kink < {EXCUSE_KINK:g}: {int(excusable.sum())}")
    bad = miss & ~excusable
    assert not bool(bad.any()), (f"{int(bad.sum())} queries away from every kink miss {BOUND:g}: worst {float(err[bad].max()):.3e} "
                                 f"at kink distance {float(kink[bad][err[bad].argmax()]):.3e}")
    assert int((miss & excusable).sum()) <= EXCUSE_SHARE * miss.numel()
    # J is not symmetric: a transposed convention cannot pass
    if NQ >= 5:
        assert float(ref.rel_frobenius(jac.cpu().transpose(-1, -2), J64).median()) > 100 * BOUND


def test_ragged_rows_equal_the_rectangular_calls_and_padding_is_untouched():
    counts = [5, 0, 1, 330]
    B, total = len(counts), sum(counts)
    cap = total + 23
    dec, _, enc, _, _ = _case(B, max(counts), 32)
    enc = {k: enc[k] for k in ("z", "anchors", "anchor_feats")}
    pts = [_t(synth.uniform(41, f"ragged_{b}", (n, 3), -0.5, 0.5)).to(DEV) for b, n in enumerate(counts)]
    r = RaggedPoints.from_list(pts, capacity=cap)
    out_buf = torch.full((cap, 3), CANARY, device=DEV)
    jac_buf = torch.full((cap, 9), CANARY, device=DEV)
    with torch.no_grad():
        out, jac = hip_decoder.decoder_jacobian_ragged(dec, r, enc, out=out_buf, jac=jac_buf)
        plain = hip_decoder.decoder_forward_ragged(dec, r, enc)
        via_module = dec(r, enc, jacobian=True)
    assert isinstance(out, RaggedPoints) and isinstance(jac, RaggedPoints) and out.packed is out_buf and jac.packed is jac_buf
    assert jac.offsets is r.offsets and jac.packed.shape == (cap, 9)
    assert bool((out_buf[total:] == CANARY).all()) and bool((jac_buf[total:] == CANARY).all()), "padding rows were written"
    assert torch.equal(out_buf[:total], plain.packed[:total])
    assert torch.equal(via_module[0].packed[:total], out_buf[:total]) and torch.equal(via_module[1].packed[:total], jac_buf[:total])
    lo = 0
    with torch.no_grad():
        for b, n in enumerate(counts):
            if n:
                one = {k: v[b:b + 1].contiguous() for k, v in enc.items()}
                w_out, w_jac = hip_decoder.decoder_jacobian(dec, pts[b][None].contiguous(), one)
                assert torch.equal(out_buf[lo:lo + n], w_out[0]), (b, _first_difference(out_buf[lo:lo + n], w_out[0]))
                assert torch.equal(jac_buf[lo:lo + n], w_jac[0].reshape(n, 9)), (b, _first_difference(jac_buf[lo:lo + n], w_jac[0].reshape(n, 9)))
            lo += n
    assert dg.fold_overs(jac).shape == (B,) and int(dg.fold_overs(jac)[1]) == 0


# ---- step functions --------------------------------------------------------------------------------------------------------
def _setup(mtype, batch, ns, seed):
    cfg = model_cfg(mtype, [ns, 64, 16])
    model, _, _ = build_product(cfg, seed, DEV)
    model.eval()
    dd = to_dev(synth.make_batch(seed, batch, ns, 4), DEV)
    dd.pop("space_samples_src"), dd.pop("space_samples_tgt")
    dd["surface_samples_src"] = dd["surface_samples_inputs"][:, :, :3].contiguous()
    return cfg, model, dd


def _verts(counts, seed):
    return [_t(synth.uniform(seed, f"verts_{b}", (n, 3), -0.5, 0.5)).to(DEV) for b, n in enumerate(counts)]


@pytest.mark.parametrize("packed", [False, True])
def test_cano_step_returns_the_same_vertices_and_the_decoders_jacobian(packed, monkeypatch):
    from nsdp_amd.model import deformation_networks as dn
    monkeypatch.setattr(dn, "ENCODE_ONCE", True)
    cfg, model, dd = _setup("forward", 2, 256, 81)
    verts = _verts([37, 37] if not packed else [37, 6], 82)
    dd["verts_src"] = RaggedPoints.from_list(verts) if packed else torch.stack(verts)
    _, plain = dn.test_on_batch_with_cano(model, dict(dd), cfg)
    assert "verts_tgt_jacobian" not in plain
    _, got = dn.test_on_batch_with_cano(model, dict(dd), cfg, jacobian=True)
    raw = lambda t: t.packed if isinstance(t, RaggedPoints) else t
    assert torch.equal(raw(got["verts_tgt_pred"]), raw(plain["verts_tgt_pred"]))
    assert torch.equal(raw(got["surface_samples_tgt_pred"]), raw(plain["surface_samples_tgt_pred"]))
    J = got["verts_tgt_jacobian"]
    with torch.no_grad():
        w_out, w_jac = model.decode(dd["verts_src"], model.encode(dd["surface_samples_inputs"]), jacobian=True)
    assert torch.equal(raw(J), raw(w_jac)) and torch.equal(raw(w_out), raw(plain["verts_tgt_pred"]))
    if packed:
        assert isinstance(J, RaggedPoints) and J.packed.shape == (43, 9) and bool(torch.isfinite(J.packed).all())
    else:
        assert J.shape == (2, 37, 3, 3) and bool(torch.isfinite(J).all())


@pytest.mark.parametrize("packed", [False, True])
def test_arbitrary_step_composes_the_two_networks_jacobians(packed, monkeypatch):
    from nsdp_amd.model import deformation_networks as dn
    from nsdp_amd.model.flow_arbitrary import _split, test_on_batch_with_arbitrary
    monkeypatch.setattr(dn, "ENCODE_ONCE", True)
    cfg, model, dd = _setup("arbitrary", 2, 256, 83)
    verts = _verts([19, 19] if not packed else [19, 4], 84)
    dd["verts_src"] = RaggedPoints.from_list(verts) if packed else torch.stack(verts)
    _, plain = test_on_batch_with_arbitrary(model, dict(dd), cfg)
    _, got = test_on_batch_with_arbitrary(model, dict(dd), cfg, jacobian=True)
    raw = lambda t: t.packed if isinstance(t, RaggedPoints) else t
    assert torch.equal(raw(got["verts_tgt_pred"]), raw(plain["verts_tgt_pred"]))
    assert torch.equal(raw(got["surface_samples_tgt_pred"]), raw(plain["surface_samples_tgt_pred"]))
    # the chain rule by hand: J2 at the canonical vertices times J1 at the source vertices
    src, tgt, mask = _split(dd)
    n1, n2 = model.model_canonicalize, model.model_deform
    with torch.no_grad():
        enc1 = n1.encode(src)
        surf2cano = n1.decode(src.contiguous(), enc1)
        q1, J1 = n1.decode(dd["verts_src"], enc1, jacobian=True)
        enc2 = n2.encode(model.deform_input(surf2cano, tgt, mask))
        out2, J2 = n2.decode(q1, enc2, jacobian=True)
    assert torch.equal(raw(out2), raw(plain["verts_tgt_pred"]))
    want = dg.compose(J2, J1)
    J = got["verts_tgt_jacobian"]
    assert type(J) is type(want) and torch.equal(raw(J), raw(want))
    assert bool(torch.isfinite(raw(J)).all())
    if packed:
        assert J.packed.shape == (23, 9)
    else:
        assert J.shape == (2, 19, 3, 3)
        assert torch.equal(J, J2 @ J1) and not torch.equal(J, J1 @ J2)


# ---- refusals --------------------------------------------------------------------------------------------------------------
def test_refusals_are_named():
    dec, q, enc, _, _ = _case(1, 4, 7)
    with torch.no_grad():
        assert hip_decoder.jacobian_refusal(dec) is None
    with torch.enable_grad():
        assert "autograd is enabled" in hip_decoder.jacobian_refusal(dec)
        with pytest.raises(_lib.NsdpHipError, match="decoder Jacobian refused: autograd is enabled"):
            hip_decoder.decoder_jacobian(dec, q, enc)
        with pytest.raises(_lib.NsdpHipError, match="autograd is enabled"):
            dec(q, enc, jacobian=True)
    with torch.no_grad():
        with hip_decoder.mode("bf16"):
            with pytest.raises(_lib.NsdpHipError, match="bf16 mode"):
                hip_decoder.decoder_jacobian(dec, q, enc)
            with pytest.raises(_lib.NsdpHipError, match="bf16 mode"):
                hip_decoder.decoder_jacobian_ragged(dec, RaggedPoints.from_list([q[0]]), enc)
        with precision.storage(torch.bfloat16):
            with pytest.raises(_lib.NsdpHipError, match="bf16 storage"):
                hip_decoder.decoder_jacobian(dec, q, enc)
        hip_decoder.ENABLED = False
        try:
            with pytest.raises(_lib.NsdpHipError, match="switched off"):
                hip_decoder.decoder_jacobian(dec, q, enc)
        finally:
            hip_decoder.ENABLED = True
        from nsdp_amd.model.decoder import CrossTransformerDecoder
        other = CrossTransformerDecoder(dim_inp=64, dim=96, nneigh=7, hidden_dim=64, out_dim=3).to(DEV)
        assert "decoder geometry" in hip_decoder.jacobian_refusal(other)
        with pytest.raises(_lib.NsdpHipError, match="decoder geometry"):
            other(torch.zeros(1, 4, 3, device=DEV), {}, jacobian=True)


# ---- poisoned arena --------------------------------------------------------------------------------------------------------
def test_both_entries_inside_the_poisoned_arena():
    """Every operand of the two entries between guards, ``out`` and ``jac`` poisoned on entry: no byte outside the declared
    outputs changes, every element of the real rows is written, and the padding rows of the packed form stay poisoned."""
    from poison_arena import PoisonArena
    from test_poisoned_arena_gpu import _modules
    B, NQ, A, KN = 3, 329, 32, 7
    dec, state = ref.decoder(11)
    dec = dec.to(DEV)
    xyz_q, anchors, feats, z = ref.inputs(5, B, NQ, A)
    counts = [NQ, 0, 6]
    total, cap = sum(counts), sum(counts) + 21
    packed = np.zeros((cap, 3), np.float32)
    packed[:total] = np.concatenate([xyz_q[b, :n] for b, n in enumerate(counts)])
    offsets = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    a = PoisonArena(DEV, 96 << 20)
    with a.routed(*_modules()), torch.no_grad():
        t = {k: a.input(k, _t(v)) for k, v in dict(xyz_q=xyz_q, anchors=anchors, feats=feats, z=z, packed=packed, offsets=offsets).items()}
        pack = hip_decoder._Pack(hip_decoder._frag).get(dec)
        pack.tensors = [a.input(f"weights[{i}]", w.cpu()) for i, w in enumerate(pack.tensors)]
        pack.ptrs = (ctypes.c_void_p * len(pack.tensors))(*[w.data_ptr() for w in pack.tensors])
        idx = a.input("idx", pu.knn(t["xyz_q"], t["anchors"], KN).cpu())
        idx_r = a.input("idx_ragged", pu.knn_ragged(t["packed"], t["offsets"], t["anchors"], KN).cpu())
        qk, vtab, a_g, v_g = (a.input(n, x.cpu()) for n, x in zip(("qk", "vtab", "a_g", "v_g"), hip_decoder._shape_tables(pack, t["z"], t["feats"])))
        out, jac = a.output("out", (B, NQ, 3)), a.output("jac", (B, NQ, 3, 3))
        out_r, jac_r = a.output("ragged.out", (cap, 3), rows=total), a.output("ragged.jac", (cap, 9), rows=total)
        p = lambda x: ctypes.c_void_p(x.data_ptr())
        L = _lib.lib()
        _lib.check(L.nsdp_decoder_jacobian_fwd(p(t["xyz_q"]), p(t["anchors"]), p(idx), p(qk), p(vtab), p(a_g), p(v_g), pack.ptrs, 17,
                                               B, NQ, A, KN, 200, 128, p(out), p(jac), _lib.stream_ptr()), "nsdp_decoder_jacobian_fwd")
        _lib.check(L.nsdp_decoder_jacobian_fwd_ragged(p(t["packed"]), p(t["offsets"]), p(t["anchors"]), p(idx_r), p(qk), p(vtab), p(a_g),
                                                      p(v_g), pack.ptrs, 17, B, cap, A, KN, 200, 128, p(out_r), p(jac_r),
                                                      _lib.stream_ptr()), "nsdp_decoder_jacobian_fwd_ragged")
        a.check(written=[out, jac, out_r[:total], jac_r[:total]])
    assert {"nsdp_decoder_jacobian_fwd", "nsdp_decoder_jacobian_fwd_ragged"} <= a.called
    assert bool(torch.isnan(out_r[total:]).all()) and bool(torch.isnan(jac_r[total:]).all())
    assert bool(torch.isfinite(jac).all()) and bool(torch.isfinite(jac_r[:total]).all())
    lo = 0
    for b, n in enumerate(counts):
        assert torch.equal(out_r[lo:lo + n], out[b, :n]) and torch.equal(jac_r[lo:lo + n], jac[b, :n].reshape(n, 9)), b
        lo += n
