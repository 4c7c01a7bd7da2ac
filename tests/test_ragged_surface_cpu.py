"""CPU-only checks of ragged SURFACE clouds (nsdp_amd.ragged: shapes of different sample counts encoded at once): the container's
``from_rows`` / ``columns``, the two packed-source entry points at the library boundary and the refusals that need no GPU."""
import ctypes
import os

import pytest
import torch

from nsdp_amd import _lib
from nsdp_amd import build as nsdp_build
from nsdp_amd.ragged import RaggedPoints, RaggedTestOnBatch

ENTRY_POINTS = ("nsdp_furthest_point_sampling_ragged", "nsdp_knn_ragged_source")


def _rows(counts, width, seed=0):
    g = torch.Generator().manual_seed(seed)
    return [torch.rand((n, width), generator=g) for n in counts]


# ---- the container ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("counts,width,capacity", [((5, 3, 9), 7, None), ((4, 0, 7), 7, 20), ((1,), 1, None), ((6, 2), 4, 8)])
def test_from_rows_round_trip(counts, width, capacity):
    shapes = _rows(counts, width)
    r = RaggedPoints.from_rows(shapes, capacity=capacity)
    total = sum(counts)
    assert r.batch == len(counts) and r.counts == tuple(counts) and r.total == total
    assert r.capacity == (total if capacity is None else capacity) and r.packed.shape == (r.capacity, width)
    assert r.offsets.dtype == torch.int32 and r.offsets.tolist() == [sum(counts[:i]) for i in range(len(counts) + 1)]
    assert torch.equal(r.packed[:total], torch.cat(shapes)) and not r.packed[total:].any()
    for a, b in zip(r.split(), shapes):
        assert a.shape == b.shape and torch.equal(a, b)
    again = RaggedPoints.from_rows(r.split(), capacity=capacity)
    assert torch.equal(again.packed, r.packed) and torch.equal(again.offsets, r.offsets)


def test_columns_keep_offsets_and_counts():
    shapes = _rows((5, 3, 9), 7)
    r = RaggedPoints.from_rows(shapes, capacity=20)
    parts = [r.columns(0, 3), r.columns(3, 6), r.columns(6, 7)]
    for p, (lo, hi) in zip(parts, ((0, 3), (3, 6), (6, 7))):
        assert p.offsets is r.offsets and p.counts == r.counts and p.capacity == r.capacity
        assert p.packed.is_contiguous() and p.packed.shape == (20, hi - lo)
        assert torch.equal(p.packed, r.packed[:, lo:hi])
        for a, b in zip(p.split(), shapes):
            assert torch.equal(a, b[:, lo:hi])
        assert r.same_layout(p)
    back = torch.cat([p.packed for p in parts], dim=1)
    assert torch.equal(back, r.packed)
    # a set built from device offsets alone keeps none either
    bare = RaggedPoints(r.packed, r.offsets)
    assert bare.columns(0, 3)._counts is None
    for lo, hi in ((-1, 3), (3, 3), (5, 8)):
        with pytest.raises(ValueError, match="columns"):
            r.columns(lo, hi)
    assert not r.same_layout(RaggedPoints.from_rows(_rows((5, 4, 8), 7), capacity=20))
    assert not r.same_layout(torch.zeros(20, 3))


def test_from_rows_refusals_and_from_list_still_wants_three_columns():
    with pytest.raises(ValueError, match="no shapes"):
        RaggedPoints.from_rows([])
    with pytest.raises(ValueError, match="one C"):
        RaggedPoints.from_rows([torch.zeros(4, 7), torch.zeros(4, 3)])
    with pytest.raises(ValueError, match="one C"):
        RaggedPoints.from_rows([torch.zeros(1, 4, 7)])
    with pytest.raises(ValueError, match="capacity"):
        RaggedPoints.from_rows(_rows((5, 6), 7), capacity=10)
    with pytest.raises(ValueError, match="dtype"):
        RaggedPoints.from_rows([torch.zeros(4, 7), torch.zeros(4, 7, dtype=torch.float64)])
    with pytest.raises(ValueError, match=r"\[n, 3\]"):
        RaggedPoints.from_list([torch.zeros(4, 2)])
    with pytest.raises(ValueError, match=r"\[n, 3\]"):
        RaggedPoints.from_list([torch.zeros(4, 7)])


# ---- the library boundary -----------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def so():
    if not os.path.exists(_lib.SO_PATH):
        nsdp_build.build()
    lib = ctypes.CDLL(_lib.SO_PATH)
    lib.nsdp_last_error.restype = ctypes.c_char_p
    return lib


def test_header_declares_and_library_exports_the_packed_source_entry_points(so):
    names = _lib.declared_symbols()
    for must in ENTRY_POINTS:
        assert must in names, must
        assert hasattr(so, must), must
    assert so.nsdp_abi_version() >= 10


def test_bad_arguments_return_status(so):
    one = ctypes.c_void_p(16)      # (a non-null pointer the library must not touch before it has checked the sizes)
    fps, knn = so.nsdp_furthest_point_sampling_ragged, so.nsdp_knn_ragged_source
    # (xyz, offsets, B, cap, n_max, nsamples, tmp, idx_out, stream)
    assert fps(None, None, 2, 64, 64, 4, None, None, None) == -1 and b"null" in so.nsdp_last_error()
    assert fps(one, one, 2, 64, 64, 0, None, one, None) == -1 and b"nsamples" in so.nsdp_last_error()
    assert fps(one, one, 2, 64, 64, -3, None, one, None) == -1 and b"nsamples" in so.nsdp_last_error()
    assert fps(one, one, 70000, 64, 64, 4, None, one, None) == -1 and b"batch" in so.nsdp_last_error()
    assert fps(one, one, 2, 0, 64, 4, None, one, None) == -1 and b"cap" in so.nsdp_last_error()
    assert fps(one, one, 2, 64, 0, 4, None, one, None) == -1 and b"n_max" in so.nsdp_last_error()
    assert fps(one, one, 2, 20000, 9000, 4, None, one, None) == -1 and b"scratch" in so.nsdp_last_error()
    assert fps(None, None, 0, 64, 64, 4, None, None, None) == 0      # nothing to do, before any pointer is looked at
    # (query, query_offsets, source, offsets, B, n, qcap, cap, n_max, k, idx_out, dist2_out, stream)
    assert knn(None, None, None, None, 2, 4, 0, 64, 64, 5, None, None, None) == -1 and b"null" in so.nsdp_last_error()
    assert knn(one, None, one, None, 2, 4, 0, 64, 64, 5, one, None, None) == -1 and b"null" in so.nsdp_last_error()
    assert knn(one, None, one, one, 2, 4, 0, 64, 64, 65, one, None, None) == -1 and b"k=65" in so.nsdp_last_error()
    assert knn(one, None, one, one, 2, 4, 0, 64, 8, 9, one, None, None) == -1 and b"n_max" in so.nsdp_last_error()
    assert knn(one, None, one, one, 70000, 4, 0, 64, 64, 5, one, None, None) == -1 and b"batch" in so.nsdp_last_error()
    assert knn(one, one, one, one, 2, 0, 64, 0, 64, 5, one, None, None) == -1 and b"cap" in so.nsdp_last_error()
    for B, n, qcap, k in ((0, 4, 0, 5), (2, 0, 0, 5), (2, 4, 0, 0)):      # nothing to do
        assert knn(None, None, None, None, B, n, qcap, 64, 64, k, None, None, None) == 0, (B, n, qcap, k)
    assert knn(None, one, None, None, 2, 4, 0, 64, 64, 5, None, None, None) == 0      # (a packed query set of no rows)


def test_python_mirrors_refuse_cpu_tensors():
    from nsdp_amd import pointnet2_utils as pu
    r = RaggedPoints.from_rows(_rows((40, 50), 3))
    with pytest.raises(RuntimeError, match="GPU"):
        pu.furthest_point_sample_ragged(r.packed, r.offsets, 16, 50)
    with pytest.raises(RuntimeError, match="GPU"):
        pu.knn_ragged_source(r.packed, r.packed, r.offsets, 8, 50, query_offsets=r.offsets)
    with pytest.raises(RuntimeError, match="GPU"):
        pu.knn_ragged_source(torch.zeros(2, 16, 3), r.packed, r.offsets, 8, 50)


# ---- refusals that need no GPU ------------------------------------------------------------------------------------------

def _model(mtype="forward", npl=(256, 64, 16)):
    from helpers import build_product, model_cfg
    cfg = model_cfg(mtype, list(npl))
    model, _, _ = build_product(cfg, 3, "cpu")
    return cfg, model.eval()


def test_encoder_refusals_and_validation_name_their_reason():
    cfg, model = _model()
    surf = RaggedPoints.from_rows(_rows((300, 64), 7))
    with torch.enable_grad(), pytest.raises(ValueError, match="autograd"):
        model.encode(surf)
    model.train()
    try:
        with torch.no_grad(), pytest.raises(ValueError, match="training mode"):
            model.encode(surf)
    finally:
        model.eval()
    with torch.no_grad():
        with pytest.raises(ValueError, match="geometry="):
            model.encode(surf, geometry={"encoder": {}})
        with pytest.raises(ValueError, match="PipelinedGeometry"):
            model.geometry(torch.zeros(2, 10, 3), surf)
        with pytest.raises(ValueError, match="columns"):
            model.encode(surf.columns(0, 3))                      # (a 3-column cloud against an encoder with features)
        # validation on the host: each names the shape and the number
        with pytest.raises(ValueError, match=r"shape 1 has 63 samples, fewer than the 64 points"):
            model.encode(RaggedPoints.from_rows(_rows((300, 63), 7)))
        with pytest.raises(ValueError, match=r"shape 1 is empty"):
            model.encode(RaggedPoints.from_rows(_rows((300, 0, 70), 7)))
    cfg2, small = _model(npl=(256, 8, 4))                         # (8 centres: the neighbour counts become the binding bound)
    k = small.encoder.transformer_begin.k
    assert k > 8
    with torch.no_grad(), pytest.raises(ValueError, match=rf"shape 0 has {k - 1} samples, fewer than the {k} neighbours"):
        small.encode(RaggedPoints.from_rows(_rows((k - 1, 300), 7)))


def test_alternate_encoder_is_refused():
    from helpers import build_product
    cfg = {"model": {"type": "forward", "use_normals": False, "encoder": "pointnet++", "decoder": "crossatten",
                     "encoder_kwargs": {"npoints_per_layer": [256, 64, 16], "nneighbor": 16, "d_transformer": 256,
                                        "nfinal_transformers": 3},
                     "decoder_kwargs": _model()[0]["model"]["decoder_kwargs"]}}
    model, _, _ = build_product(cfg, 3, "cpu")
    with torch.no_grad(), pytest.raises(ValueError, match=r"pointnet\+\+"):
        model.eval().encode(RaggedPoints.from_rows(_rows((300, 64), 7)))


def test_step_functions_want_both_surface_inputs_ragged():
    from nsdp_amd.model.deformation_networks import test_on_batch_with_cano as step
    cfg, model = _model()
    surf = RaggedPoints.from_rows(_rows((300, 64), 7))
    with pytest.raises(ValueError, match="both"):
        step(model, {"surface_samples_inputs": surf, "surface_samples_src": torch.zeros(2, 64, 3), "verts_src": torch.zeros(2, 5, 3)}, cfg)
    other = RaggedPoints.from_rows(_rows((64, 300), 3))
    with pytest.raises(ValueError, match="not packed like"):
        step(model, {"surface_samples_inputs": surf, "surface_samples_src": other, "verts_src": torch.zeros(2, 5, 3)}, cfg)


def test_query_sharded_refuses_ragged_surfaces():
    from nsdp_amd.query_shard import _refuse_ragged
    surf = RaggedPoints.from_rows(_rows((300, 64), 7))
    with pytest.raises(NotImplementedError, match="surface"):
        _refuse_ragged({"surface_samples_inputs": surf, "surface_samples_src": surf.columns(0, 3), "verts_src": torch.zeros(2, 5, 3)})
    _refuse_ragged({"surface_samples_inputs": torch.zeros(2, 64, 7), "verts_src": torch.zeros(2, 5, 3)})


def test_ragged_step_wrapper_runs_ragged_surfaces_eagerly_even_with_graph():
    calls = []

    def fake_step(model, dd, config):
        calls.append(dd)
        dd["surface_samples_tgt_pred"] = dd["surface_samples_src"]
        dd["verts_tgt_pred"] = dd["verts_src"]
        return 0.0, dd

    surf = RaggedPoints.from_rows(_rows((30, 64), 7))
    verts = [torch.rand(5, 3), torch.rand(9, 3)]
    step = RaggedTestOnBatch(fake_step, 100, graph=True)
    dd = {"surface_samples_inputs": surf, "surface_samples_src": surf.columns(0, 3), "verts_src": verts}
    _, out = step(None, dd, None)
    assert step.eager_calls == 1 and step.replays == 0 and step._step is None
    assert calls[0]["surface_samples_inputs"] is surf                       # passed through as it is
    assert isinstance(out["surface_samples_tgt_pred"], RaggedPoints) and out["verts_tgt_pred"].counts == (5, 9)
