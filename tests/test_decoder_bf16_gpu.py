"""The bf16-operand fused decoder (nsdp_decoder_fused_fwd_bf16, hip_decoder.MODE = "bf16") on the GPU: its accuracy against
the fp32 fused kernel with the layered bf16-storage decoder as the yardstick, exact row independence (slices, batches, query
shards), tails, the untouched default, weight tracking, refusals, the model-level error, graph replay and the CLI.

The decoder and its inputs are those of tests/test_decoder_gpu.py (procedural weights, seeds 11 / 5)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from helpers import l2_err
from nsdp_amd import _lib, hip_decoder, precision
from nsdp_amd.query_shard import QueryShards, query_sharded
from test_decoder_gpu import KW, _decoder, _inputs
from test_query_shard_gpu import KEYS, ROOT, _first_difference, _Local, _setup, _skip_variants, _step_fn

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
BF = torch.bfloat16


def _case(B, NQ, A, wseed=11, iseed=5):
    dec, _ = _decoder(wseed)
    dec = dec.to(DEV)
    xyz_q, anchors, feats, z = _inputs(iseed, B, NQ, A)
    enc = {"z": torch.from_numpy(z).to(DEV), "anchors": torch.from_numpy(anchors).to(DEV),
           "anchor_feats": torch.from_numpy(feats).to(DEV)}
    return dec, torch.from_numpy(xyz_q).to(DEV), enc


def _bf16(dec, q, enc):
    with torch.no_grad(), hip_decoder.mode("bf16"):
        return dec(q, enc)


def _f32(dec, q, enc):
    with torch.no_grad(), hip_decoder.mode("f32"):
        return dec(q, enc)


@pytest.mark.parametrize("B,NQ,A", [(2, 2048, 16), (3, 333, 32), (1, 100001, 16)])
def test_bf16_fused_is_no_worse_than_the_layered_bf16_decoder(B, NQ, A):
    """Truth: the fp32 fused kernel (pinned to the oracle at 1e-4 by tests/test_decoder_gpu.py).  Yardstick: the layered
    decoder under bf16 storage (default NSDP_BF16_TRUNK) on the same encoding, stored in bf16 as that path stores it.  The new
    kernel rounds a strict subset of what the layered path rounds, so l2(bf16 fused) <= 1.25 x l2(layered bf16); the quarter
    covers the different order of the fp32 accumulation.  An fp64 emulation of the two rounding schemes on these weights and
    inputs gave 6.8e-4 against 1.12e-3 at (2, 2048, 16) and 7.7e-4 against 1.20e-3 at (3, 333, 32)."""
    if precision.is_bf16() or not hip_decoder.ENABLED:
        pytest.skip("the truth of this comparison is the fp32 fused kernel under fp32 storage")
    dec, q, enc = _case(B, NQ, A)
    truth = _f32(dec, q, enc).cpu().numpy()
    fused = _bf16(dec, q, enc).cpu().numpy()
    enc16 = dict(enc, z=enc["z"].to(BF), anchor_feats=enc["anchor_feats"].to(BF))
    with torch.no_grad(), hip_decoder.mode("f32"), precision.storage(BF):
        layered = dec(q, enc16).float().cpu().numpy()
    assert fused.shape == (B, NQ, 3) and np.isfinite(fused).all()
    e_new, e_lay = l2_err(fused, truth), l2_err(layered, truth)
    rms = float(np.sqrt((truth.astype(np.float64) ** 2).sum(-1).mean()))
    msg = f"(B, NQ, A) = {(B, NQ, A)}: l2(bf16 fused, f32 fused) = {e_new:.3e}, l2(layered bf16, f32 fused) = {e_lay:.3e}, " \
          f"ratio {e_new / e_lay:.3f}, output RMS norm {rms:.3f}"
    print("\n" + msg)
    assert e_lay > 0 and e_new <= 1.25 * e_lay, msg


@pytest.mark.parametrize("NQ", [333, 2051])
def test_rows_are_independent_of_slice_and_batch(NQ):
    _skip_variants()
    dec, q, enc = _case(3, NQ, 16)
    whole = _bf16(dec, q, enc)
    cuts = [0, 7, 40, 41, NQ]
    parts = [_bf16(dec, q[:, a:b].contiguous(), enc) for a, b in zip(cuts, cuts[1:])]
    got = torch.cat(parts, dim=1)
    assert torch.equal(got, whole), _first_difference(got, whole)
    for b in range(3):          # a shape decoded alone == inside the batch of three
        one = {k: v[b:b + 1].contiguous() for k, v in enc.items()}
        alone = _bf16(dec, q[b:b + 1].contiguous(), one)
        assert torch.equal(alone, whole[b:b + 1]), (b, _first_difference(alone, whole[b:b + 1]))
    for world in (3,):          # decode_sharded's semantics in one process: the ranks' slices, concatenated
        parts = [_bf16(dec, QueryShards(r, world).local(q), enc) for r in range(world)]
        assert [p.shape[1] for p in parts] == [QueryShards(r, world).bounds(NQ)[1] - QueryShards(r, world).bounds(NQ)[0]
                                               for r in range(world)]
        got = torch.cat(parts, dim=1)
        assert torch.equal(got, whole), _first_difference(got, whole)


def test_query_shards_of_the_model_concatenate_to_the_whole_call():
    """query_shard.decode_local under mode bf16 and fp32 storage (require_supported passes: it asks for the fused decoder)."""
    _skip_variants()
    from nsdp_amd.query_shard import decode_local
    cfg, model, dd = _setup("forward", 2, 256, 3001, 65)
    with torch.no_grad(), hip_decoder.mode("bf16"):
        enc = model.encode(dd["surface_samples_inputs"])
        whole = model.decode(dd["verts_src"], enc)
        got = torch.cat([decode_local(model, dd["verts_src"], enc, QueryShards(r, 3)) for r in range(3)], dim=1)
    assert torch.equal(got, whole), _first_difference(got, whole)
    with torch.no_grad(), hip_decoder.mode("f32"):
        assert not torch.equal(model.decode(dd["verts_src"], enc), whole)


def test_tails():
    """Row counts around one wave's 16 rows and two waves' 32, and config 5's odd 100 001: every row stored, none invented."""
    dec, q, enc = _case(2, 100033, 16)
    long = _bf16(dec, q, enc)
    assert long.shape == (2, 100033, 3) and bool(torch.isfinite(long).all())
    for NQ in (1, 15, 16, 17, 31, 32, 33, 100001):
        out = _bf16(dec, q[:, :NQ].contiguous(), enc)
        assert out.shape == (2, NQ, 3) and out.dtype is torch.float32
        assert bool(torch.isfinite(out).all())
        assert torch.equal(out, long[:, :NQ]), (NQ, _first_difference(out, long[:, :NQ]))


def test_default_mode_is_untouched_and_bf16_differs():
    if precision.is_bf16() or not hip_decoder.ENABLED or hip_decoder.MODE != "f32":
        pytest.skip("compares the default configuration with itself")
    dec, q, enc = _case(2, 2048, 16)
    with torch.no_grad():
        never_touched = dec(q, enc).clone()          # hip_decoder.MODE as imported
    assert torch.equal(_f32(dec, q, enc), never_touched)
    other = _bf16(dec, q, enc)
    assert not torch.equal(other, never_touched)
    with torch.no_grad():
        assert torch.equal(dec(q, enc), never_touched)        # the context manager put the default back
    # the fp32 kernel through the C ABI is not disturbed by the bf16 pack living on the same module
    assert "_fused_pack" in dec.__dict__ and "_fused_pack_bf16" in dec.__dict__


def test_bf16_storage_takes_the_bf16_kernel_on_the_upcast_encoding():
    """Mode bf16 under bf16 STORAGE: the fused bf16 kernel runs there too (mode f32 keeps the layered path); the bf16-stored
    encoding is upcast and the per-shape tables are built in fp32 -- the same bits as the fp32-storage call on the upcast."""
    dec, q, enc = _case(2, 333, 16)
    enc16 = dict(enc, z=enc["z"].to(BF), anchor_feats=enc["anchor_feats"].to(BF))
    with precision.storage(BF):
        out = _bf16(dec, q, enc16)
        layered = _f32(dec, q, enc16)
    up = dict(enc, z=enc16["z"].float(), anchor_feats=enc16["anchor_feats"].float())
    want = _bf16(dec, q, up)
    assert out.dtype is torch.float32 and torch.equal(out, want), _first_difference(out, want)
    assert not torch.equal(layered.float(), out)


def test_bf16_pack_tracks_weight_updates():
    """The mirror of test_fused_decoder_tracks_weight_updates: an in-place parameter update and a load_state_dict both reach
    the bf16 pack, and the result is that of a fresh decoder with the same state."""
    dec, q, enc = _case(2, 64, 16, wseed=3, iseed=9)
    a = _bf16(dec, q, enc).clone()
    with torch.no_grad():
        dec.fc_out.bias.add_(1.0)
    b = _bf16(dec, q, enc).clone()
    torch.testing.assert_close(b, a + 1.0, rtol=0, atol=1e-5)
    with torch.no_grad():
        dec.blocks[2].fc_0.weight.mul_(1.5)
    c = _bf16(dec, q, enc).clone()
    assert not torch.equal(c, b)
    other, _ = _decoder(11)
    dec.load_state_dict(other.state_dict())
    d = _bf16(dec, q, enc).clone()
    assert not torch.equal(d, c)
    fresh = other.to(DEV)
    assert torch.equal(d, _bf16(fresh, q, enc))


def test_refusals_and_fall_throughs():
    from nsdp_amd.model.decoder import CrossTransformerDecoder
    other = CrossTransformerDecoder(dim_inp=64, dim=96, nneigh=7, hidden_dim=64, out_dim=3).to(DEV).eval()
    assert not hip_decoder.supported(other)
    with hip_decoder.mode("bf16"), pytest.raises(_lib.NsdpHipError):
        hip_decoder.decoder_forward(other, torch.zeros(1, 4, 3, device=DEV), {})
    # through the module a decoder of another geometry (four blocks) takes the layered path, whatever the mode
    _, q, enc = _case(2, 200, 16)
    four = CrossTransformerDecoder(**dict(KW, n_blocks=4)).to(DEV).eval()
    assert not hip_decoder.supported(four)
    with hip_decoder.mode("bf16"), pytest.raises(_lib.NsdpHipError):
        hip_decoder.decoder_forward(four, q, enc)
    assert torch.equal(_bf16(four, q, enc), _f32(four, q, enc))
    # with gradients enabled the mode is ignored: the layered (differentiable) path runs
    dec, q, enc = _case(2, 200, 16)
    with torch.enable_grad():
        with hip_decoder.mode("bf16"):
            g16 = dec(q, enc)
        with hip_decoder.mode("f32"):
            g32 = dec(q, enc)
    assert g16.requires_grad and torch.equal(g16, g32)
    assert not torch.equal(_bf16(dec, q, enc), g16.detach())


@pytest.mark.parametrize("mtype", ["forward", "arbitrary"])
def test_model_level_error_is_within_the_bf16_storage_error(mtype):
    """test_on_batch of the tiny model: (fp32 storage + decoder mode bf16) against the all-fp32 call is no further than the
    all-bf16-storage call is -- it contains that path's decoder roundings at most and none of its encoder's.  For FlowArbitrary
    the composition amplifies network 1's error (README, config 3); the bar is the same inequality.  It holds because
    FlowArbitrary's first network keeps the fp32 kernel under mode bf16 (hip_decoder.NET1_MODE = "f32", the default): measured
    8.0e-3 against 1.7e-1 for bf16 storage.  With both networks on the bf16 kernel (NET1_MODE = "bf16", printed below, not
    asserted) the same model gave 2.3e-1: network 2's discrete selections on network 1's output points flip."""
    _skip_variants()
    cfg, model, dd = _setup(mtype, 2, 256, 3001, 65)
    step = _step_fn(mtype)
    with hip_decoder.mode("f32"):
        _, ref = step(model, dict(dd), cfg)
        ref = {k: ref[k].cpu().numpy() for k in KEYS}
        with precision.storage(BF):
            _, st = step(model, dict(dd), cfg)
            st = {k: st[k].float().cpu().numpy() for k in KEYS}
    with hip_decoder.mode("bf16"):
        _, new = step(model, dict(dd), cfg)
        new = {k: new[k].cpu().numpy() for k in KEYS}
    if mtype == "arbitrary":
        was = hip_decoder.NET1_MODE
        try:
            hip_decoder.NET1_MODE = "bf16"
            with hip_decoder.mode("bf16"):
                _, both = step(model, dict(dd), cfg)
        finally:
            hip_decoder.NET1_MODE = was
        for k in KEYS:
            print(f"\narbitrary {k}, both networks on the bf16 kernel: l2 vs fp32 = {l2_err(both[k].cpu().numpy(), ref[k]):.3e}")
    for k in KEYS:
        e_new, e_st = l2_err(new[k], ref[k]), l2_err(st[k], ref[k])
        msg = f"{mtype} {k}: l2(fp32 storage + bf16 decoder, fp32) = {e_new:.3e}, l2(bf16 storage, fp32) = {e_st:.3e}"
        print("\n" + msg)
        assert 0 < e_new <= e_st, msg


@pytest.mark.parametrize("mtype", ["forward", "arbitrary"])
@pytest.mark.parametrize("rank,world", [(0, 1), (1, 3)])
def test_replayed_sharded_call_equals_eager_in_bf16_mode(mtype, rank, world):
    """query_sharded(graph=True) under mode bf16: the replay equals the eager call bit for bit.  The mode is read when the
    forward runs, i.e. at capture time: a captured step keeps the kernel it was captured with, and a later set_mode() does not
    change what it replays."""
    _skip_variants()
    cfg, model, dd = _setup(mtype, 2, 256, 3001, 65)
    cls = QueryShards if world == 1 else _Local
    eager = query_sharded(_step_fn(mtype), cls(rank, world))
    graphed = query_sharded(_step_fn(mtype), cls(rank, world), graph=True)
    before = hip_decoder.MODE
    try:
        hip_decoder.set_mode("bf16")
        _, e = eager(model, dict(dd), cfg)
        e = {k: e[k].clone() for k in KEYS}
        for _ in range(2):
            _, g = graphed(model, dict(dd), cfg)
            for k in KEYS:
                assert torch.equal(g[k], e[k]), (k, _first_difference(g[k], e[k]))
        assert graphed.replays == 2 and graphed.eager_calls == 0
        hip_decoder.set_mode("f32")
        _, e32 = eager(model, dict(dd), cfg)
        assert not torch.equal(e32["verts_tgt_pred"], e["verts_tgt_pred"])
        _, g = graphed(model, dict(dd), cfg)          # still the captured bf16 kernel
        for k in KEYS:
            assert torch.equal(g[k], e[k]), (k, _first_difference(g[k], e[k]))
        assert graphed.replays == 3
    finally:
        hip_decoder.set_mode(before)
        graphed.close()


def _infer(tmp_path, name, *flags):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "LOCAL_WORLD_SIZE",
                                                             "MASTER_ADDR", "MASTER_PORT")}
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    out = tmp_path / name
    p = subprocess.run([sys.executable, "-m", "nsdp_amd.infer", str(tmp_path / "forward.yaml"), "--batch", "2", "--surface", "256",
                        "--queries", "4099", "--steps", "2", "--warmup", "1", "--out", str(out), *flags],
                       capture_output=True, text=True, timeout=600, cwd=ROOT, env=env)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, p.stdout[-2000:]
    return json.loads(lines[0]), {k: np.load(out / (k + ".npy")) for k in KEYS}


@pytest.mark.timeout(1300)
def test_infer_cli_two_ranks_equal_one_rank_in_bf16_mode(tmp_path):
    """`python -m nsdp_amd.infer --gpus 2 --backend gloo --decoder-dtype bf16 --queries 4099` on one GPU: the ranks agree and
    rank 0's arrays are byte-equal to the one-rank run's; the line names the dtype and the distance to the fp32 kernel."""
    _skip_variants()
    import yaml
    from nsdp_amd.config import default_config
    cfg = default_config("forward")
    cfg["model"]["encoder_kwargs"]["npoints_per_layer"] = [256, 64, 16]
    (tmp_path / "forward.yaml").write_text(yaml.safe_dump(cfg))
    one, pred1 = _infer(tmp_path, "one", "--gpus", "1", "--decoder-dtype", "bf16")
    two, pred2 = _infer(tmp_path, "two", "--gpus", "2", "--backend", "gloo", "--decoder-dtype", "bf16")
    ref, pred0 = _infer(tmp_path, "ref", "--gpus", "1", "--decoder-dtype", "f32")
    assert one["world"] == 1 and two["world"] == 2 and two["backend"] == "gloo"
    assert two["ranks_agree"] is True
    assert one["decoder_dtype"] == "bf16" and two["decoder_dtype"] == "bf16" and ref["decoder_dtype"] == "f32"
    assert "l2_vs_f32" not in ref and "max_abs_diff_vs_f32" not in ref
    for line in (one, two):
        assert 0 < line["l2_vs_f32"] <= line["max_abs_diff_vs_f32"] * 3 ** 0.5 and line["max_abs_diff_vs_f32"] < 0.1, line
    assert one["l2_vs_f32"] == two["l2_vs_f32"]
    for k in KEYS:
        assert pred1[k].shape == (2, 256 if k.startswith("surface") else 4099, 3)
        assert np.array_equal(pred1[k].view(np.int32), pred2[k].view(np.int32)), k
    assert not np.array_equal(pred1["verts_tgt_pred"], pred0["verts_tgt_pred"])
    d = pred1["verts_tgt_pred"].astype(np.float64) - pred0["verts_tgt_pred"].astype(np.float64)
    assert abs(float(np.abs(d).max()) - one["max_abs_diff_vs_f32"]) < 1e-12
