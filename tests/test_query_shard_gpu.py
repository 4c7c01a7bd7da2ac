"""Query-point sharding of dense inference on the GPU (nsdp_amd.query_shard): every rank's slice decoded on its own and put
back together is bit-identical to the whole decode -- the fused fp32 decoder and the anchor kNN treat every query row on its own.
The ranks are run one after the other in this process (no process group: their local predictions are concatenated), at the
forward model's full size, FlowArbitrary's full size and BASELINE config 5's size; the replayed call against the eager one; and
``python -m nsdp_amd.infer`` as two ranks over gloo on one GPU against its one-rank run."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from helpers import build_product, model_cfg, nondeterministic_knobs, to_dev
from nsdp_amd import synth
from nsdp_amd.query_shard import QueryShards, decode_local, query_sharded

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = ("surface_samples_tgt_pred", "verts_tgt_pred")


def _skip_variants():
    from nsdp_amd import hip_decoder, precision
    from nsdp_amd.model import deformation_networks as dn
    knobs = nondeterministic_knobs()
    if not hip_decoder.ENABLED:
        knobs.append("NSDP_FUSED_DECODER=0")      # (the layered decoder: tile shapes follow the row count)
    if precision.is_bf16():
        knobs.append("NSDP_STORAGE=bf16")         # (refused by query_sharded)
    if not dn.ENCODE_ONCE:
        knobs.append("NSDP_ENCODE_ONCE=0")        # (refused by query_sharded)
    if knobs:
        pytest.skip("bit equality of sliced and whole decodes does not apply under " + ", ".join(knobs))


def _setup(mtype, batch, ns, nq, seed):
    cfg = model_cfg(mtype, [min(ns, 2048), 500 if ns >= 2048 else 64, 100 if ns >= 2048 else 16])
    model, _, _ = build_product(cfg, seed, DEV)
    model.eval()
    dd = to_dev(synth.make_batch(seed, batch, ns, nq), DEV)
    dd["surface_samples_src"] = dd["surface_samples_inputs"][:, :, :3].contiguous()
    dd["verts_src"], dd["verts_tgt"] = dd.pop("space_samples_src"), dd.pop("space_samples_tgt")
    return cfg, model, dd


def _step_fn(mtype):
    from nsdp_amd.model.deformation_networks import test_on_batch_with_cano
    from nsdp_amd.model.flow_arbitrary import test_on_batch_with_arbitrary
    return test_on_batch_with_arbitrary if mtype == "arbitrary" else test_on_batch_with_cano


def _first_difference(a, b):
    rows = (a != b).any(-1).nonzero()
    return f"{rows.shape[0]} rows differ, first (shape, query): {rows[:8].tolist()}"


def _sharded_equals_whole(mtype, cfg, model, dd, worlds):
    """Every rank of every world runs its local step (encode + its slices); concatenated in rank order == the unsharded step."""
    step_fn = _step_fn(mtype)
    _, whole = step_fn(model, dict(dd), cfg)
    whole = {k: whole[k].clone() for k in KEYS}
    for world in worlds:
        parts = {k: [] for k in KEYS}
        for rank in range(world):
            local = query_sharded(step_fn, QueryShards(rank, world)).local(model, dict(dd))
            for k in KEYS:
                t, n = local[k]
                lo, hi = QueryShards(rank, world).bounds(n)
                assert n == whole[k].shape[1] and t.shape == (whole[k].shape[0], hi - lo, 3), (world, rank, k, t.shape)
                parts[k].append(t)
        for k in KEYS:
            got = torch.cat(parts[k], dim=1)
            assert torch.equal(got, whole[k]), (mtype, world, k, _first_difference(got, whole[k]))


def test_forward_model_sliced_decode_is_bit_identical():
    """Forward model at full size, B = 2, NS = 2048, 10 007 vertices (not a multiple of 16): worlds 2, 3, 8."""
    _skip_variants()
    cfg, model, dd = _setup("forward", 2, 2048, 10007, 61)
    _sharded_equals_whole("forward", cfg, model, dd, (2, 3, 8))


def test_flow_arbitrary_sliced_decode_is_bit_identical():
    """FlowArbitrary at full size, B = 2: network 1 decodes the whole surface plus each rank's vertices, network 2 the slices."""
    _skip_variants()
    cfg, model, dd = _setup("arbitrary", 2, 2048, 10007, 62)
    _sharded_equals_whole("arbitrary", cfg, model, dd, (2, 3, 8))


def test_config5_size_sliced_decode_is_bit_identical():
    """BASELINE config 5's size for the forward model: B = 4, 100 000 vertices per shape."""
    _skip_variants()
    cfg, model, dd = _setup("forward", 4, 2048, 100000, 63)
    _sharded_equals_whole("forward", cfg, model, dd, (2, 3, 8))


@pytest.mark.parametrize("mtype", ["forward", "arbitrary"])
def test_empty_slices_decode_to_nothing(mtype):
    """5 vertices over 8 ranks: ranks 5-7 hold no vertex -- the kNN and fused-decoder calls take an empty slice -- and the
    concatenation still equals the whole decode (the 256 surface samples are split too)."""
    _skip_variants()
    cfg, model, dd = _setup(mtype, 2, 256, 5, 64)
    _sharded_equals_whole(mtype, cfg, model, dd, (8,))
    if mtype == "forward":
        with torch.no_grad():
            enc = model.encode(dd["surface_samples_inputs"])
            empty = decode_local(model, dd["verts_src"], enc, QueryShards(7, 8))
        assert empty.shape == (2, 0, 3)


class _Local(QueryShards):
    """One rank's view without a process group: gather() hands back the local rows."""

    def gather(self, local, nq):
        lo, hi = self.bounds(nq)
        assert local.shape[1] == hi - lo
        return local


@pytest.mark.parametrize("mtype", ["forward", "arbitrary"])
@pytest.mark.parametrize("rank,world", [(0, 1), (1, 3)])
def test_replayed_sharded_call_equals_eager(mtype, rank, world):
    """query_sharded(graph=True): the first call captures this rank's encode and local decode over static copies of the batch,
    later calls replay it; a new batch written into the caller's tensors is picked up.  Bit-equal to the eager call."""
    _skip_variants()
    cfg, model, dd = _setup(mtype, 2, 256, 3001, 65)
    cls = QueryShards if world == 1 else _Local
    eager = query_sharded(_step_fn(mtype), cls(rank, world))
    graphed = query_sharded(_step_fn(mtype), cls(rank, world), graph=True)
    batches = [dd, {k: v.clone() for k, v in dd.items()}]
    nxt = to_dev(synth.make_batch(66, 2, 256, 3001), DEV)
    batches[1]["surface_samples_inputs"].copy_(nxt["surface_samples_inputs"])
    batches[1]["surface_samples_src"].copy_(nxt["surface_samples_inputs"][:, :, :3])
    batches[1]["verts_src"].copy_(nxt["space_samples_src"])
    try:
        outs = []
        for b in (0, 1, 0):
            _, e = eager(model, dict(batches[b]), cfg)
            _, g = graphed(model, dict(batches[b]), cfg)
            for k in KEYS:
                assert torch.equal(g[k], e[k]), (b, k, _first_difference(g[k], e[k]))
            outs.append(g["verts_tgt_pred"].clone())
        assert graphed.replays == 3
        assert not torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2])
        # one dict passed again and again (the predictions written back into it do not count as inputs): every call replays
        same = dict(batches[1])
        for _ in range(3):
            _, g = graphed(model, same, cfg)
            assert torch.equal(g["verts_tgt_pred"], outs[1])
        assert graphed.replays == 6 and graphed.eager_calls == 0
    finally:
        graphed.close()


def test_rccl_exchange_fills_the_gather_buffer_world1():
    """The collective of QueryShards.gather on a one-rank RCCL communicator (the one this box can build): all_gather_into_tensor
    into the [world, B, m, C] buffer seen as [world * B, m, C] -- what an N-GPU job runs, at N = 1."""
    import socket
    import torch.distributed as dist
    with socket.socket() as sock:
        sock.bind(("127.0.0.1", 0))
        port = sock.getsockname()[1]
    saved = {k: os.environ.get(k) for k in ("MASTER_ADDR", "MASTER_PORT")}
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    torch.cuda.set_device(DEV)
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=DEV)
    try:
        sh = QueryShards(0, 1)
        send = torch.arange(3 * 5 * 3, dtype=torch.float32, device=DEV).view(3, 5, 3)
        buf = torch.full((1, 3, 5, 3), -1.0, device=DEV)
        sh.exchange(buf, send)
        torch.cuda.synchronize()
        assert not sh.list_form
        assert torch.equal(buf[0], send)
    finally:
        dist.destroy_process_group()
        for k, v in saved.items():      # (later tests start subprocesses: they must not inherit this rendezvous)
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _infer(tmp_path, name, *flags):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "LOCAL_WORLD_SIZE",
                                                             "MASTER_ADDR", "MASTER_PORT")}
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    out = tmp_path / name
    p = subprocess.run([sys.executable, "-m", "nsdp_amd.infer", str(tmp_path / "forward.yaml"), "--batch", "2", "--surface", "256",
                        "--queries", "1001", "--steps", "2", "--warmup", "1", "--out", str(out), *flags],
                       capture_output=True, text=True, timeout=600, cwd=ROOT, env=env)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, p.stdout[-2000:]
    return json.loads(lines[0]), {k: np.load(out / (k + ".npy")) for k in KEYS}


@pytest.mark.timeout(1300)
def test_infer_two_ranks_over_gloo_equal_one_rank(tmp_path):
    """`python -m nsdp_amd.infer --gpus 2 --backend gloo --graph` (two ranks on whatever devices the box has; every call a replay,
    the last one's output gathered and written): the ranks agree and rank 0's predictions are bit-equal to the eager one-rank
    run's."""
    _skip_variants()
    import yaml
    from nsdp_amd.config import default_config
    cfg = default_config("forward")
    cfg["model"]["encoder_kwargs"]["npoints_per_layer"] = [256, 64, 16]
    (tmp_path / "forward.yaml").write_text(yaml.safe_dump(cfg))
    one, pred1 = _infer(tmp_path, "one", "--gpus", "1")
    two, pred2 = _infer(tmp_path, "two", "--gpus", "2", "--backend", "gloo", "--graph")
    assert one["world"] == 1 and two["world"] == 2 and two["backend"] == "gloo"
    assert two["ranks_agree"] is True
    assert [r["rank"] for r in two["ranks"]] == [0, 1]
    for r in two["ranks"]:
        assert {"device_index", "pci_domain_id", "pci_bus_id", "hip_visible_devices"} <= set(r)
        assert r["replays"] == 1 + 2 and r["eager_calls"] == 0, r          # (--warmup 1 --steps 2: all of them replayed)
    assert one["ranks"][0]["replays"] == 0 and one["ranks"][0]["eager_calls"] == 1 + 2
    assert two["gather"] == "all_gather"      # (gloo, device tensors: the list form)
    assert one["ms_per_call"] > 0 and two["ms_per_call"] > 0
    for k in KEYS:
        assert pred1[k].shape == (2, 256 if k.startswith("surface") else 1001, 3)
        assert np.array_equal(pred1[k].view(np.int32), pred2[k].view(np.int32)), k
