"""Query-point sharding of dense inference on CPU (nsdp_amd.query_shard): the partition, the gloo all-gather at world 2 and 3,
and the sharded step functions around stub networks against the unsharded calls."""
import os
import socket

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from nsdp_amd.query_shard import QueryShards, query_sharded


@pytest.mark.parametrize("world", [1, 2, 3, 4, 7, 8, 16])
def test_bounds_cover_in_order_without_overlap(world):
    for nq in sorted({0, 1, 2, 3, 5, 15, 16, 17, 100, 10007, 100000, world - 1, world, world + 1, 3 * world - 1,
                      3 * world, 3 * world + 1}):
        m = -(-nq // world)
        spans = [QueryShards(r, world).bounds(nq) for r in range(world)]
        assert spans[0][0] == 0 and spans[-1][1] == nq
        for (lo, hi), (lo2, _) in zip(spans, spans[1:]):
            assert lo <= hi == lo2                               # contiguous, ordered, disjoint
        sizes = [hi - lo for lo, hi in spans]
        assert all(0 <= s <= m for s in sizes) and sum(sizes) == nq
        full = [s == m for s in sizes]
        assert full == sorted(full, reverse=True), (nq, world, sizes)      # only the last ranks are short
        assert sizes == sorted(sizes, reverse=True), (nq, world, sizes)


def test_bounds_edge_cases():
    assert QueryShards(0, 1).bounds(10007) == (0, 10007)
    assert [QueryShards(r, 8).bounds(5) for r in range(8)] == [(0, 1), (1, 2), (2, 3), (3, 4), (4, 5), (5, 5), (5, 5), (5, 5)]
    assert [QueryShards(r, 4).bounds(4 * 3 - 1) for r in range(4)] == [(0, 3), (3, 6), (6, 9), (9, 11)]
    assert [QueryShards(r, 3).bounds(4) for r in range(3)] == [(0, 2), (2, 4), (4, 4)]
    with pytest.raises(ValueError):
        QueryShards(2, 2)


def test_world1_gather_is_the_identity():
    x = torch.arange(2 * 7 * 3, dtype=torch.float32).view(2, 7, 3)
    assert QueryShards(0, 1).gather(x, 7) is x
    with pytest.raises(ValueError):
        QueryShards(0, 1).gather(x[:, :5], 7)


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _spawn(target, world, *args):
    port = _free_port()
    ctx = mp.get_context("spawn")
    out = ctx.Queue()
    procs = [ctx.Process(target=target, args=(r, world, port, out) + args) for r in range(world)]
    for p in procs:
        p.start()
    res = dict(out.get(timeout=150) for _ in range(world))
    for p in procs:
        p.join(timeout=30)
        assert p.exitcode == 0
    return res


def _coded(b, q, c):
    # every value names its (shape, query, channel): a misplaced row shows
    return float(b * 1_000_000 + q * 10 + c)


def _worker_gather(rank, world, port, out, B, C, nqs):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        sh = QueryShards(rank, world)
        ok = []
        for nq in nqs:
            lo, hi = sh.bounds(nq)
            local = torch.tensor([[[_coded(b, q, c) for c in range(C)] for q in range(lo, hi)] for b in range(B)],
                                 dtype=torch.float64).view(B, hi - lo, C)
            full = sh.gather(local, nq)
            want = torch.tensor([[[_coded(b, q, c) for c in range(C)] for q in range(nq)] for b in range(B)],
                                dtype=torch.float64).view(B, nq, C)
            ok.append((nq, tuple(full.shape), bool(torch.equal(full, want)), full.is_contiguous()))
            assert not sh.list_form or nq == 0      # (gloo with host tensors: all_gather_into_tensor)
        out.put((rank, ok))
    finally:
        dist.destroy_process_group()


@pytest.mark.timeout(180)
@pytest.mark.parametrize("world", [2, 3])
def test_gather_reassembles_uneven_and_empty_chunks_over_gloo(world):
    # 1 and 2 < world at world 3: empty ranks; 7, 11: uneven last chunks; 12: even; 0: nothing anywhere
    nqs = [1, 2, 7, 11, 12, 0, 2 * world - 1]
    res = _spawn(_worker_gather, world, 2, 3, nqs)
    for rank in range(world):
        for nq, shape, equal, contiguous in res[rank]:
            assert shape == (2, nq, 3), (rank, nq)
            assert equal, (rank, nq)
            assert contiguous, (rank, nq)


class _StubNet(torch.nn.Module):
    """encode / decode with the Deformation_Networks split; decode is row-wise (every query on its own)."""

    def __init__(self, seed):
        super().__init__()
        g = torch.Generator().manual_seed(seed)
        self.w_enc = torch.nn.Parameter(torch.randn(7, 5, generator=g))
        self.w_dec = torch.nn.Parameter(torch.randn(3, 3, generator=g))

    def encode(self, inputs, queries=None):
        x = inputs if inputs.shape[-1] == 7 else torch.cat([inputs, inputs[..., :1].expand(*inputs.shape[:-1], 4)], -1)
        return {"z": torch.tanh(x @ self.w_enc).mean(1)}

    def decode(self, points, encoding):
        return torch.sin(points @ self.w_dec) * encoding["z"][:, None, :3] + points

    def forward(self, points, inputs):
        return self.decode(points, self.encode(inputs))


def _batch(B, ns, nq):
    from nsdp_amd import synth
    d = {k: torch.from_numpy(v) for k, v in synth.make_batch(5, B, ns, nq).items()}
    d["surface_samples_src"] = d["surface_samples_inputs"][:, :, :3].contiguous()
    d["verts_src"], d["verts_tgt"] = d.pop("space_samples_src"), d.pop("space_samples_tgt")
    return d


def _stub_model(mtype):
    if mtype == "forward":
        return _StubNet(1)
    from nsdp_amd.model.flow_arbitrary import FlowArbitrary
    return FlowArbitrary({}, _StubNet(2), _StubNet(3))


def _step_fn(mtype):
    from nsdp_amd.model.deformation_networks import test_on_batch_with_cano
    from nsdp_amd.model.flow_arbitrary import test_on_batch_with_arbitrary
    return test_on_batch_with_cano if mtype == "forward" else test_on_batch_with_arbitrary


def _worker_step(rank, world, port, out, mtype, B, ns, nq):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        model = _stub_model(mtype)
        d = _batch(B, ns, nq)
        ref_loss, ref = _step_fn(mtype)(model, dict(d), {}, compute_loss=True)
        loss, got = query_sharded(_step_fn(mtype), QueryShards(rank, world))(model, dict(d), {}, compute_loss=True)
        out.put((rank, (loss == ref_loss, [torch.equal(got[k], ref[k]) for k in ("surface_samples_tgt_pred", "verts_tgt_pred")])))
    finally:
        dist.destroy_process_group()


@pytest.mark.timeout(180)
@pytest.mark.parametrize("mtype", ["forward", "arbitrary"])
@pytest.mark.parametrize("world,nq", [(2, 101), (3, 2)])
def test_query_sharded_step_equals_the_unsharded_call_over_gloo(mtype, world, nq):
    """Every rank's gathered predictions and loss equal the unwrapped step function's (nq = 2 at world 3: an empty rank)."""
    res = _spawn(_worker_step, world, mtype, 2, 17, nq)
    for rank in range(world):
        loss_equal, equal = res[rank]
        assert loss_equal and all(equal), (rank, loss_equal, equal)


@pytest.mark.parametrize("mtype", ["forward", "arbitrary"])
def test_query_sharded_world1_equals_the_unsharded_call(mtype):
    model = _stub_model(mtype)
    d = _batch(3, 11, 29)
    ref_loss, ref = _step_fn(mtype)(model, dict(d), {}, compute_loss=True)
    loss, got = query_sharded(_step_fn(mtype), QueryShards(0, 1))(model, dict(d), {}, compute_loss=True)
    assert loss == ref_loss
    for k in ("surface_samples_tgt_pred", "verts_tgt_pred"):
        assert torch.equal(got[k], ref[k]), k


def test_query_sharded_refuses_what_it_cannot_split():
    from nsdp_amd import precision
    from nsdp_amd.model import deformation_networks as dn
    from nsdp_amd.model.deformation_networks import validate_on_batch_with_cano
    with pytest.raises(TypeError):
        query_sharded(validate_on_batch_with_cano, QueryShards(0, 1))
    step = query_sharded(_step_fn("forward"), QueryShards(0, 1))
    prev, dn.ENCODE_ONCE = dn.ENCODE_ONCE, False
    try:
        with pytest.raises(RuntimeError, match="NSDP_ENCODE_ONCE"):
            step(_stub_model("forward"), _batch(1, 5, 4), {})
    finally:
        dn.ENCODE_ONCE = prev
    with precision.storage(torch.bfloat16):
        with pytest.raises(NotImplementedError):
            step(_stub_model("forward"), _batch(1, 5, 4), {})


class _PassThroughStep:
    """graph_step.GraphedStep's interface without a GPU: capture() records nothing, a "replay" runs the function."""

    def __init__(self, fn, max_streams=None, weights_change=True):
        self.fn = fn

    def capture(self, warmup=3):
        return self

    def __call__(self):
        return self.fn()

    def close(self):
        pass


@pytest.mark.parametrize("mtype", ["forward", "arbitrary"])
def test_graph_mode_replays_when_the_caller_passes_one_dict_again(mtype, monkeypatch):
    """graph=True keys its replay on the inputs the local form reads: the predictions written back into the caller's dict, the
    targets and other entries do not turn the next call with that same dict into an eager one.  Inputs of other shapes do."""
    from nsdp_amd import graph_step
    monkeypatch.setattr(graph_step, "GraphedStep", _PassThroughStep)
    model = _stub_model(mtype).eval()
    d = _batch(2, 11, 29)
    _, ref = _step_fn(mtype)(model, dict(d), {})
    step = query_sharded(_step_fn(mtype), QueryShards(0, 1), graph=True)
    d["name"] = "shape_0"
    for _ in range(4):
        _, got = step(model, d, {})
        for k in ("surface_samples_tgt_pred", "verts_tgt_pred"):
            assert torch.equal(got[k], ref[k]), k
    assert step.replays == 4 and step.eager_calls == 0
    assert set(step._static) == set(step.local_fn.inputs)
    step(model, _batch(2, 11, 30), {})
    assert step.replays == 4 and step.eager_calls == 1


def test_layered_decoders_are_refused():
    """The sharded decode is bit-identical on the fused fp32 decoder only: NSDP_FUSED_DECODER=0 and decoder geometries the fused
    kernel was not built for are refused before anything runs."""
    from nsdp_amd import hip_decoder
    from nsdp_amd.config import default_config
    from nsdp_amd.model import build_model
    from nsdp_amd.query_shard import decode_local
    cfg = default_config("forward")
    model = build_model(cfg, device="cpu")[0].eval()
    pts = torch.zeros(1, 4, 3)
    prev, hip_decoder.ENABLED = hip_decoder.ENABLED, False
    try:
        with pytest.raises(NotImplementedError, match="fused"):
            decode_local(model, pts, {}, QueryShards(0, 1))
        with pytest.raises(NotImplementedError, match="fused"):
            query_sharded(_step_fn("forward"), QueryShards(0, 1)).local(model, _batch(1, 5, 4))
    finally:
        hip_decoder.ENABLED = prev
    cfg["model"]["decoder_kwargs"]["hidden_dim"] = 64
    with pytest.raises(NotImplementedError, match="fused"):
        decode_local(build_model(cfg, device="cpu")[0], pts, {}, QueryShards(0, 1))
