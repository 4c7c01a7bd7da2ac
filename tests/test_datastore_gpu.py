"""GPU: the device-resident data store (nsdp_amd/datastore.py, include/nsdp_batch.h).  The draw against its numpy emulation bit
for bit and within derived uniformity bounds; the assembled batch against the oracle's per-sample contract, against
``prepare_batch`` over torch-stacked frames and against the reference's recorded ``__getitem__`` outputs; the loader's epochs,
shards and partial batch; a short training run from a tree on disk, replayed and eager."""
import argparse
import os

import numpy as np
import pytest
import torch

import datastore_tree as dt
import subset_ref as sr
from helpers import model_cfg
from nsdp_amd import dataset, datastore, synth, train
from oracle import dataset_ref

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
KEYS = ["surface_samples_cano", "surface_samples_src", "surface_samples_tgt", "surface_normals_cano", "surface_normals_src",
        "surface_normals_tgt", "cano_handle_sample_idx", "surface_samples_inputs", "space_samples_cano", "space_samples_src",
        "space_samples_tgt"]


def _counts(values):
    return torch.tensor(values, dtype=torch.int32, device=DEV)


# ------------------------------------------------------------------------------------------------------------------ the draw
@pytest.mark.parametrize("n_full", [1, 2, 3, 5, 63, 64, 65, 1000, 200000, 1 << 20])
def test_draw_equals_the_emulation(n_full):
    for n_keep in sorted({1, n_full, min(n_full, 2048)}):
        key = dict(seed=(3 << 32) | 77, epoch=2, step=n_keep % 7, which=sr.SPACE if n_keep == 1 else sr.SURFACE)
        rows = datastore.subset_draw(_counts([n_full] * 3), n_keep, **key).cpu().numpy()            # B = 3: three keys
        assert rows.shape == (3, n_keep) and rows.dtype == np.int32
        assert np.array_equal(rows, sr.draw([n_full] * 3, n_keep, **key)), (n_full, n_keep)
        assert rows.min() >= 0 and rows.max() < n_full
        assert all(len(np.unique(r)) == n_keep for r in rows)
        if n_keep > 8:
            assert not np.array_equal(rows[0], rows[1]) and not np.array_equal(rows[1], rows[2])


def test_draw_with_different_n_full_inside_one_batch():
    n_full = [5, 1000, 200000, 1 << 20, 64]
    rows = datastore.subset_draw(_counts(n_full), 5, seed=9, epoch=0, step=3, which=sr.SURFACE).cpu().numpy()
    assert np.array_equal(rows, sr.draw(n_full, 5, 9, 0, 3, sr.SURFACE))
    for r, n in zip(rows, n_full):
        assert r.min() >= 0 and r.max() < n and len(np.unique(r)) == 5
    assert sorted(rows[0].tolist()) == [0, 1, 2, 3, 4]


@pytest.mark.parametrize("n_full,n_keep", [(64, 16), (65, 16), (1000, 250)])
def test_draw_is_uniform_within_six_sigma(n_full, n_keep):
    """One launch of 4096 keys; the bounds are Binomial(4096, p) +- 6 standard deviations (test_datastore_cpu.py)."""
    rows = datastore.subset_draw(_counts([n_full] * 4096), n_keep, seed=31337, epoch=1, step=0, which=sr.SURFACE).cpu().numpy()
    assert all(len(np.unique(r)) == n_keep for r in rows[:64])
    assert not sr.uniformity_violations(rows, n_full, n_keep)


def test_random_subset_by_bijection():
    a = dataset.random_subset(3, 1000, 200, DEV, method="bijection", key=(5, 1, 2, sr.SURFACE))
    assert a.dtype == torch.int32 and np.array_equal(a.cpu().numpy(), sr.draw([1000] * 3, 200, 5, 1, 2, sr.SURFACE))
    b = dataset.random_subset(2, 50, 80, DEV, method="bijection")            # n_keep beyond n_full: all rows, like the sort
    assert b.shape == (2, 50) and all(sorted(r.tolist()) == list(range(50)) for r in b)
    assert not torch.equal(b, dataset.random_subset(2, 50, 80, DEV, method="bijection"))      # successive calls differ
    assert dataset.random_subset(2, 50, 20, DEV).shape == (2, 20)                                # the default is the sort
    with pytest.raises(ValueError, match="neither"):
        dataset.random_subset(2, 50, 20, DEV, method="shuffle")


# ------------------------------------------------------------------------------------------------------------------ assemble
def _raw_frame(data, seq, frame):
    """A frame as the reference reads it (dataset_deform4d_flow.py:137-157): float32 arrays, coordinates fixed on request."""
    d = os.path.join(data["dataset_dir"], seq, frame)
    s, q = np.load(os.path.join(d, data["surface_flow_file"])), np.load(os.path.join(d, data["space_flow_file"]))
    out = {"surface_samples": s["points"].astype(np.float32), "surface_normals": s["normals"].astype(np.float32),
           "space_samples": q["points"].astype(np.float32)}
    if data["fix_coord_system"]:
        out = {k: np.ascontiguousarray(np.stack([v[:, 0], -v[:, 2], v[:, 1]], axis=1)) for k, v in out.items()}
    return out


def _same(got, want, what):
    """atol = 0 (and -0 == 0, as numpy compares); shapes and dtypes as well."""
    assert got.shape == want.shape and got.dtype == want.dtype, what
    if want.dtype == np.bool_:
        assert np.array_equal(got, want), what
    else:
        np.testing.assert_allclose(got, want, rtol=0, atol=0, err_msg=what)


def _bits_equal(a, b):
    a, b = a.contiguous(), b.contiguous()
    if a.dtype == torch.bool:
        return a.shape == b.shape and torch.equal(a, b)
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.view(torch.int32), b.view(torch.int32))


@pytest.fixture(scope="module")
def mixed_trees(tmp_path_factory):
    """Two identities of different counts; 'mixed': ant in fp16 files and bee in fp32 (fp32 arenas); 'half': all fp16."""
    root = tmp_path_factory.mktemp("assemble")
    spec = dict(identities=["ant", "bee"], motions=["walk", "jump"], frames=3, n_surface=[40, 52], n_space=[24, 30], seed=5)
    return {"mixed": synth.write_dataset_tree(str(root / "mixed"), dtype={"ant": np.float16, "bee": np.float32}, **spec),
            "half": synth.write_dataset_tree(str(root / "half"), dtype=np.float16, **spec)}


@pytest.mark.parametrize("files", ["mixed", "half"])
@pytest.mark.parametrize("inverse", [False, True])
@pytest.mark.parametrize("noise_level", [0.0, 0.02])
def test_assemble_equals_the_oracle_and_prepare_batch(mixed_trees, files, inverse, noise_level):
    data = dict(mixed_trees[files], num_surf_samples=16, num_space_samples=8, inverse=inverse, noise_level=noise_level)
    store = datastore.SampleStore({"data": data}, "identity_seen", "train_seen", device=DEV)
    want = torch.float32 if files == "mixed" else torch.float16
    assert store.surface_arena.dtype == want and store.space_arena.dtype == want and store.draw_space and (store.n, store.m) == (16, 8)
    assert store.surface_arena.shape[1] == 6 and store.space_arena.shape[1] == 4 and store.frame_table.shape == (len(store.frames), 6)
    assert len(store.frames) == 6 and store.nbytes <= store.byte_budget
    g = np.random.RandomState(3)
    # B = 3 across both identities against the oracle, sample by sample; then three samples of ONE identity against prepare_batch
    for picks in ([0, len(store.pairs) - 1, 2], [i for i, p in enumerate(store.pairs) if p[1].startswith("bee")][:3]):
        pairs = [store.pairs[i] for i in picks]
        full = [_raw_frame(data, p[1], p[2])["surface_samples"].shape[0] for p in pairs]
        full_space = [_raw_frame(data, p[1], p[2])["space_samples"].shape[0] for p in pairs]
        surf_idx = np.stack([g.permutation(n)[:16] for n in full]).astype(np.int32)
        space_idx = np.stack([g.permutation(n)[:8] for n in full_space]).astype(np.int32)
        noise = g.randn(3, 16, 3).astype(np.float32)
        ids = torch.from_numpy(np.ascontiguousarray(store.pair_frames[picks].T)).to(DEV)
        out = store.assemble(ids, torch.from_numpy(surf_idx).to(DEV), torch.from_numpy(space_idx).to(DEV), torch.from_numpy(noise).to(DEV))
        assert sorted(out) == sorted(KEYS) and all(out[k].is_contiguous() for k in KEYS)
        raws = [[_raw_frame(data, p[1], p[2]), _raw_frame(data, p[4], p[5]), _raw_frame(data, p[6], p[7])] for p in pairs]
        for b, (cano, src, tgt) in enumerate(raws):
            np.random.seed(b)
            ref = dataset_ref.sample_contract(data, cano, src, tgt, surf_idxs=surf_idx[b], noise=noise[b])
            s_src, s_tgt = (tgt, src) if inverse else (src, tgt)
            ref.update({"space_samples_cano": cano["space_samples"][space_idx[b]], "space_samples_src": s_src["space_samples"][space_idx[b]],
                        "space_samples_tgt": s_tgt["space_samples"][space_idx[b]]})        # (the oracle draws its own space rows)
            for key in KEYS:
                _same(out[key][b].cpu().numpy(), ref[key], f"{key} of sample {b}")
        if len({p[1] for p in pairs}) == 1:
            stack = lambda c: {k: torch.from_numpy(np.stack([r[c][k] for r in raws])).to(DEV) for k in raws[0][0]}
            torch_out = dataset.prepare_batch(data, stack(0), stack(1), stack(2), torch.from_numpy(surf_idx).to(DEV),
                                              torch.from_numpy(space_idx).to(DEV), torch.from_numpy(noise).to(DEV))
            assert sorted(torch_out) == sorted(KEYS)
            for key in KEYS:
                assert _bits_equal(out[key], torch_out[key]), key
    box = store.frame_bbox(0)
    first = _raw_frame(data, store.frames[0].seq, store.frames[0].name)["surface_samples"]
    assert np.array_equal(box[0], first.min(axis=0)) and np.array_equal(box[1], first.max(axis=0))      # of the FULL cloud


def test_every_row_kept_when_space_counts_equal_the_request(tmp_path):
    data = synth.write_dataset_tree(str(tmp_path), ["ant"], ["walk", "jump"], 3, 20, 8, np.float16)
    data.update(num_surf_samples=16, num_space_samples=8)
    store = datastore.SampleStore({"data": data}, "identity_seen", "train_seen", device=DEV)
    assert not store.draw_space and store.m == 8
    batch = next(iter(store.loader(2, seed=1)))
    pair = store.pairs[store.loader(2, seed=1).epoch_samples(0)[1]]
    assert np.array_equal(batch["space_samples_tgt"][1].cpu().numpy(), _raw_frame(data, pair[6], pair[7])["space_samples"])


@pytest.mark.parametrize("name", sorted(dt.cases("item")))
def test_assemble_equals_the_references_recorded_samples(tmp_path, name):
    z, cfg = dt.golden(), dt.cases("item")[name]
    data = dt.case_data(dt.rebuild(cfg["tree"], str(tmp_path)), cfg)
    store = datastore.SampleStore({"data": data}, "identity_seen", cfg["motion_split"], device=DEV)
    indices = z[f"item/{name}/indices"].tolist()
    take = lambda what: torch.from_numpy(np.stack([z[f"item/{name}/{i}/{what}"] for i in indices])).to(DEV)
    picks = [store.sample_indices(0)[i] for i in indices]
    ids = torch.from_numpy(np.ascontiguousarray(store.pair_frames[picks].T)).to(DEV)
    noise = take("noise") if data["noise_level"] > 0.0 else None
    out = store.assemble(ids, take("surf_idx"), take("space_idx"), noise)
    for b, i in enumerate(indices):
        for key in KEYS:
            _same(out[key][b].cpu().numpy(), z[f"item/{name}/{i}/{key}"], f"{name}: {key} of sample {i}")


# ------------------------------------------------------------------------------------------------------------------ the loader
@pytest.fixture(scope="module")
def train_tree(tmp_path_factory):
    """Two identities x three motions (one held out) x three frames, 300 surface and 200 space rows: 12 training pairs."""
    data = synth.write_dataset_tree(str(tmp_path_factory.mktemp("train")), ["ant", "bee"], ["walk", "jump", "turn"], 3, 300, 200,
                                    np.float16, seed=9)
    data.update(num_surf_samples=256, num_space_samples=128)
    return data


def _equal_batches(a, b):
    return sorted(a) == sorted(b) and all(_bits_equal(a[k], b[k]) for k in a)


def test_loader_epochs_shards_and_the_partial_batch(train_tree):
    store = datastore.SampleStore({"data": train_tree}, "identity_seen", "train_seen", device=DEV)
    assert len(store) == 12
    loader = store.loader(5, seed=4)
    assert len(loader) == 3
    epochs = [list(loader), list(loader)]
    assert [b["surface_samples_inputs"].shape[0] for b in epochs[0]] == [5, 5, 2]                # the last batch: what remains
    for e, batches in enumerate(epochs):
        samples = loader.epoch_samples(e)
        assert sorted(samples.tolist()) == list(range(12))                                        # every pair once
        for step, batch in enumerate(batches):
            picks = samples[step * 5:(step + 1) * 5]
            ids = torch.from_numpy(np.ascontiguousarray(store.pair_frames[picks].T)).to(DEV)
            surf = torch.from_numpy(sr.draw([300] * len(picks), 256, 4, e, step, sr.SURFACE)).to(DEV)
            space = torch.from_numpy(sr.draw([200] * len(picks), 128, 4, e, step, sr.SPACE)).to(DEV)
            assert _equal_batches(batch, store.assemble(ids, surf, space))
            assert all(v.device == DEV for v in batch.values())
    assert not np.array_equal(loader.epoch_samples(0), loader.epoch_samples(1))
    again = list(store.loader(5, seed=4))
    assert all(_equal_batches(a, b) for a, b in zip(again, epochs[0])) and len(again) == 3        # one seed: equal batches
    other = list(store.loader(5, seed=5))
    assert not _equal_batches(other[0], epochs[0][0])
    # shard: of every world_size consecutive batches the rank-th, the trailing partial group dropped (SyntheticLoader.shard)
    whole = list(store.loader(2, seed=4))                                                         # six batches
    for world in (2, 4):
        for rank in range(world):
            mine = list(store.loader(2, seed=4).shard(rank, world))
            assert len(mine) == 6 // world
            assert all(_equal_batches(m, whole[g * world + rank]) for g, m in enumerate(mine))
    synthetic = train.SyntheticLoader(1, 6, 1, n_surf=8, n_query=8)
    assert len(list(synthetic.shard(1, 4))) == len(list(store.loader(2, seed=4).shard(1, 4))) == 1
    # a validation store: the list as formed, no shuffle
    val = datastore.SampleStore({"data": train_tree}, "identity_seen", "test_unseen_motions", device=DEV)
    vl = val.loader(4, seed=4)
    assert not vl.shuffle and vl.epoch_samples(0).tolist() == vl.epoch_samples(1).tolist() == list(range(len(val)))


# ------------------------------------------------------------------------------------------------------------------ training
def _tiny_config(train_tree):
    cfg = model_cfg("forward", [256, 64, 16])
    cfg["data"] = dict(train_tree)
    cfg["training"] = {"epochs": 4, "save_frequency": 2, "optimizer": "Adam", "lr": 5e-4, "lr_step": 2, "lr_decay": 0.1,
                       "weight_decay": 0.0, "iden_split": "identity_seen", "motion_split": "train_seen", "batch_size": 5}
    cfg["validation"] = {"frequency": 2, "iden_split": "identity_seen", "motion_split": "test_unseen_motions", "batch_size": 3}
    return cfg


def test_training_from_the_store_replayed_and_eager(train_tree, tmp_path):
    from nsdp_amd.graph_step import GraphedTrainOnBatch, capturable_adam
    from nsdp_amd.model import build_model, optimizer_factory
    cfg = _tiny_config(train_tree)
    hists = []
    for graph in (False, True):
        train.seed_everything(27)
        model, train_fn, val_fn, _ = build_model(cfg, device=DEV)
        sched, opt = optimizer_factory(cfg["training"], model.parameters())
        capturable_adam(opt)        # (both runs on the fused capturable Adam: the same arithmetic, so the runs can be held EQUAL)
        loader, val = train.dataset_loaders(cfg, 27, DEV, log=lambda *_: None)
        assert len(loader) == 3 and loader.batch == 5 and val.batch == 3 and loader.shuffle and not val.shuffle
        fn = GraphedTrainOnBatch(train_fn) if graph else train_fn
        args = argparse.Namespace(continue_from_epoch=0, best_val_loss=float("inf"))
        sub = tmp_path / ("g" if graph else "e")
        sub.mkdir()
        hists.append(train.fit(model, (fn, val_fn), sched, opt, loader, val, cfg, str(sub), args, DEV, log=lambda *_: None))
        if graph:
            assert fn.replays >= 4 and fn.eager_calls >= 4          # (the partial batch of every epoch runs eagerly)
    e, g = [[h[2] for h in hist if h[0] == "train"] for hist in hists]
    ve, vg = [[h[2] for h in hist if h[0] == "val"] for hist in hists]
    print("epoch losses", e, "validation", ve)
    assert len(e) == len(g) == 4 and e == g, (e, g)
    assert ve == vg and len(ve) >= 1, (ve, vg)
    assert all(np.isfinite(e)) and e[-1] < e[0]


def test_a_step_on_a_loader_batch_equals_the_step_on_prepare_batch(train_tree):
    from nsdp_amd.model import build_model, optimizer_factory
    cfg = _tiny_config(train_tree)
    store = datastore.SampleStore(cfg, "identity_seen", "train_seen", device=DEV)
    loader = store.loader(4, seed=8)
    batch = next(iter(loader))
    picks = loader.epoch_samples(0)[:4]
    pairs = [store.pairs[i] for i in picks]
    raws = [[_raw_frame(cfg["data"], p[1], p[2]), _raw_frame(cfg["data"], p[4], p[5]), _raw_frame(cfg["data"], p[6], p[7])] for p in pairs]
    stack = lambda c: {k: torch.from_numpy(np.stack([r[c][k] for r in raws])).to(DEV) for k in raws[0][0]}
    surf = torch.from_numpy(sr.draw([300] * 4, 256, 8, 0, 0, sr.SURFACE)).to(DEV)
    space = torch.from_numpy(sr.draw([200] * 4, 128, 8, 0, 0, sr.SPACE)).to(DEV)
    torch_batch = dataset.prepare_batch(cfg["data"], stack(0), stack(1), stack(2), surf, space)
    losses = []
    for data_dict in (batch, torch_batch):
        train.seed_everything(27)
        model, train_fn, _, _ = build_model(cfg, device=DEV)
        _, opt = optimizer_factory(cfg["training"], model.parameters())
        model.train()
        losses.append([float(train_fn(model, opt, data_dict, cfg)) for _ in range(2)])
    assert losses[0] == losses[1] and all(np.isfinite(losses[0])), losses
