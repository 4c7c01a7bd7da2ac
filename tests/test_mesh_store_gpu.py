"""GPU: the device-resident mesh store (nsdp_amd/meshstore.py, include/nsdp_meshbatch.h).  The kernel against the numpy emulation of
its rule (tests/mesh_sample_ref.py) bit for bit on all four outputs; what a face index as correspondence guarantees; the loader's
epochs, shards, partial batch and ``inverse``; a train step on a loader batch against ``dataset.prepare_batch``; a short
``--mesh-dataset`` training run, replayed and eager.  Nothing statistical runs here: tests/test_mesh_store_cpu.py checks the
rule's distributions on the emulation."""
import argparse

import numpy as np
import pytest
import torch

import mesh_sample_ref as mr
from helpers import model_cfg
from nsdp_amd import dataset, meshstore, synth, train

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
PARTIAL_RANGE = 0.125          # exact in fp32: the hand-placed faces below sit exactly on bbox_min + range / bbox_max - range


def _upload(arrays):
    return {k: torch.from_numpy(v.view(np.int32) if v.dtype == np.uint32 else v).to(DEV) for k, v in arrays.items()}


def _launch(dev_arrays, ids, n, m, key, noise=None, level=0.0, partial_range=PARTIAL_RANGE, sigma=(0.1, 0.02)):
    a = dev_arrays
    return meshstore.mesh_batch_sample(a["vert_arena"], a["face_arena"], a["thr_arena"], a["frame_table"], a["topo_table"],
                                       torch.from_numpy(ids).to(DEV), n, m, *key, partial_range, sigma[0], sigma[1],
                                       None if noise is None else torch.from_numpy(noise).to(DEV), level)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _assert_bit_equal(got, want, what=""):
    assert sorted(got) == sorted(mr.KEYS)
    for k in mr.KEYS:
        g = got[k].cpu().numpy()
        assert g.shape == want[k].shape and g.dtype == want[k].dtype, (what, k, g.shape, want[k].shape, g.dtype)
        assert np.array_equal(_bits(g), _bits(want[k])), (what, k, int((_bits(g) != _bits(want[k])).sum()))


# ------------------------------------------------------------------------------------------------------------------ the kernel
@pytest.fixture(scope="module")
def three_topologies():
    """Nine frames: a tetrahedron (F = 4), an octahedron-derived mesh (F = 32) and the grid (F = 200, two zero-area faces), each
    as (cano, src, tgt).  Placed by hand, with PARTIAL_RANGE = 1/8:
      * the tetrahedron's canonical frame has min z = 0 and one face in the plane z = 1/8 = bbox_min.z + range, spanning y from 0
        to 1/2: its rows sit exactly ON the third bound (z < bound is false) and are handles only through y;
      * the octahedron's canonical frame has y in [0, 5/8], one face in the plane y = 1/8 = bbox_min.y + range and one in the
        plane y = 1/2 = bbox_max.y - range: rows exactly on the first and the second bound;
      * the grid's tgt frame collapses a face that has area in the canonical frame: a normal of (0, 0, 0) there."""
    tet_v = np.array([[0.0, 0.0, 0.125], [0.25, 0.5, 0.125], [0.5, 0.0625, 0.125], [0.125, 0.25, 0.0]])
    tet_f = np.array([[0, 1, 2], [0, 3, 1], [1, 3, 2], [2, 3, 0]], dtype=np.int32)
    oct_v, oct_f = mr.octahedron()
    oct_c = oct_v.copy()
    oct_c[:, 1] += 0.3125
    oct_c[3, 1], oct_c[2, 1] = 0.0, 0.625                                   # the two poles: bbox_min.y and bbox_max.y
    free = [f for f in oct_f if 2 not in f and 3 not in f]
    low = free[0]
    high = next(f for f in free if not set(f) & set(low))
    oct_c[low, 1], oct_c[high, 1] = 0.125, 0.5
    grid_v, grid_f = mr.grid()
    grid_t = mr.deform(grid_v, 2)
    grid_t[grid_f[50, 2]] = grid_t[grid_f[50, 1]]
    frames = [tet_v, mr.deform(tet_v, 1), mr.deform(tet_v, 2), oct_c, mr.deform(oct_v, 1), mr.deform(oct_v, 2),
              grid_v, mr.deform(grid_v, 1), grid_t]
    arrays = meshstore.pack([f.astype(np.float32) for f in frames], [0, 0, 0, 1, 1, 1, 2, 2, 2], [tet_f, oct_f, grid_f], [0, 3, 6])
    ids = np.array([[0, 3, 6], [1, 4, 7], [2, 5, 8]], dtype=np.int32)
    return arrays, _upload(arrays), ids


@pytest.mark.parametrize("with_noise,key", [(False, (77, 0, 3)), (True, ((5 << 32) | 9, 2, 11))])
def test_kernel_equals_the_emulation_bit_for_bit(three_topologies, with_noise, key):
    arrays, dev, ids = three_topologies
    g = np.random.RandomState(2)
    for n in (1, 63, 64, 65, 257):
        noise = g.randn(3, n, 3).astype(np.float32) if with_noise else None
        for m in (0, 1, 2, 7, 130):
            level = 0.02 if with_noise else 0.0
            got = _launch(dev, ids, n, m, key, noise, level)
            want = mr.sample(arrays, ids, n, m, *key, PARTIAL_RANGE, 0.1, 0.02, noise, level)
            _assert_bit_equal(got, want, (n, m))
    # what the hand-placed frames are there for, on the last (largest) case
    cano, mask = want["surface_samples_cano"], want["cano_handle_sample_idx"][..., 0]
    box = [arrays["frame_table"][k, 3:6].copy().view(np.float32) for k in (0, 3, 6)]
    head = np.stack([cano[b, :, 1] < box[b][1] + np.float32(PARTIAL_RANGE) for b in range(3)])
    tail = np.stack([cano[b, :, 1] > box[b][4] - np.float32(PARTIAL_RANGE) for b in range(3)])
    foot = np.stack([cano[b, :, 2] < box[b][2] + np.float32(PARTIAL_RANGE) for b in range(3)])
    assert all((c & ~o1 & ~o2).any() for c, o1, o2 in ((head, tail, foot), (tail, head, foot), (foot, head, tail)))      # each fires ALONE
    assert 0 < mask.mean() < 1 and np.array_equal(mask, head | tail | foot)
    on_foot = cano[0, :, 2] == np.float32(0.125)                                        # the tetrahedron's face in z = min + range
    on_head, on_tail = cano[1, :, 1] == np.float32(0.125), cano[1, :, 1] == np.float32(0.5)
    assert on_foot.sum() > 20 and on_head.sum() >= 1 and on_tail.sum() >= 1, (on_foot.sum(), on_head.sum(), on_tail.sum())
    assert (on_foot & ~mask[0]).any() and (on_head & ~mask[1]).any() and (on_tail & ~mask[1]).any()      # on a bound: no handle
    nc, nt = want["surface_normals_cano"][2], want["surface_normals_tgt"][2]
    flat = ~nt.any(axis=1)
    assert flat.sum() > 0 and nc[flat].any(axis=1).all()                                # degenerate in tgt alone: (0, 0, 0) there
    if with_noise:
        assert not np.array_equal(want["surface_samples_src"], mr.sample(arrays, ids, 257, 0, *key, PARTIAL_RANGE, 0.1, 0.02)["surface_samples_src"])


def test_another_key_gives_other_rows(three_topologies):
    _, dev, ids = three_topologies
    base = _launch(dev, ids, 64, 7, (1, 0, 0))
    assert all(torch.equal(base[k], v) for k, v in _launch(dev, ids, 64, 7, (1, 0, 0)).items())
    for key in ((2, 0, 0), (1, 1, 0), (1, 0, 1), (1 | (1 << 32), 0, 0)):
        other = _launch(dev, ids, 64, 7, key)
        assert not torch.equal(base["surface_samples_cano"], other["surface_samples_cano"]), key
        assert not torch.equal(base["space_samples_cano"], other["space_samples_cano"]), key


def test_both_batch_kernels_write_a_row_identically():
    """csrc/batch_rows.h is one definition: the rows that nsdp_mesh_batch_sample draws, laid out as fp32 sample pools and handed
    to nsdp_batch_assemble with the same box, range and noise, come back as the same eleven tensors bit for bit.  B = 3, n = 300,
    m = 70: more than one 256-lane block of surface rows, neither count a multiple of 256."""
    from nsdp_amd import datastore
    B, n, m, key, level = 3, 300, 70, (21, 1, 6), 0.02
    verts, faces = mr.grid()
    arrays = meshstore.pack([mr.deform(verts, k).astype(np.float32) for k in range(5)], [0] * 5, [faces], [0, 1, 2])
    dev = _upload(arrays)
    ids = np.array([[0, 1, 2], [1, 2, 3], [2, 3, 4]], dtype=np.int32)                   # (cano, src, tgt) of the three samples
    clean = _launch(dev, ids, n, m, key)
    # sample b's pools: frames 3b (cano), 3b + 1 (src), 3b + 2 (tgt), each of n surface records [point | normal] and m space
    # records [point | 0]; every entry of the sample carries the box of its canonical MESH frame
    surf = torch.cat([torch.cat([clean[f"surface_samples_{k}"][b], clean[f"surface_normals_{k}"][b]], dim=1)
                      for b in range(B) for k in ("cano", "src", "tgt")]).contiguous()
    space = torch.cat([torch.nn.functional.pad(clean[f"space_samples_{k}"][b], (0, 1)) for b in range(B) for k in ("cano", "src", "tgt")]).contiguous()
    assert surf.shape == (9 * n, 6) and space.shape == (9 * m, 4) and surf.dtype == space.dtype == torch.float32
    table = np.zeros((9, 6), dtype=np.int64)
    for f in range(9):
        table[f, :3] = f * n, f * m, n | (m << 32)
        table[f, 3:6] = arrays["frame_table"][ids[0, f // 3], 3:6]
    pool_ids = torch.arange(9, dtype=torch.int32, device=DEV).reshape(B, 3).T.contiguous()
    surf_idx = torch.arange(n, dtype=torch.int32, device=DEV).repeat(B, 1)
    noise = np.random.RandomState(8).randn(B, n, 3).astype(np.float32)
    pooled = datastore.batch_assemble(surf, space, torch.from_numpy(table).to(DEV), pool_ids, surf_idx, None, m, PARTIAL_RANGE,
                                      torch.from_numpy(noise).to(DEV), level)
    sampled = _launch(dev, ids, n, m, key, noise, level)
    _assert_bit_equal(pooled, {k: v.cpu().numpy() for k, v in sampled.items()})         # (fp32 as uint32, the mask as bytes)
    assert 0 < sampled["cano_handle_sample_idx"].float().mean() < 1                     # the rule decides both ways
    assert (sampled["surface_samples_src"] != clean["surface_samples_src"]).any()       # the noise is there


# ------------------------------------------------------------------------------------------------------------------ correspondence
def test_a_face_index_is_the_correspondence():
    # src == tgt frame: the same rows, bit for bit
    verts, faces = mr.grid()
    arrays = meshstore.pack([verts.astype(np.float32), mr.deform(verts, 1).astype(np.float32)], [0, 0], [faces], [0])
    out = _launch(_upload(arrays), np.array([[0], [1], [1]], dtype=np.int32), 257, 130, (3, 1, 4))
    for what in ("surface_samples", "surface_normals", "space_samples"):
        assert torch.equal(out[f"{what}_src"].view(torch.int32), out[f"{what}_tgt"].view(torch.int32)), what
    assert not torch.equal(out["surface_samples_src"], out["surface_samples_cano"])
    # tgt = cano - 1/2 on a mesh of coordinates 0 and 1: every product w * x is a scaling by a power of two and every partial
    # sum a multiple of 2^-25 of magnitude <= 1 (cano) or <= 1/2 (tgt), so no operation rounds and tgt - cano is the offset
    cube = np.array([[x, y, z] for x in (0.0, 1.0) for y in (0.0, 1.0) for z in (0.0, 1.0)])
    cube_f = np.array([[0, 1, 3], [0, 3, 2], [4, 6, 7], [4, 7, 5], [0, 4, 5], [0, 5, 1], [2, 3, 7], [2, 7, 6], [0, 2, 6], [0, 6, 4],
                       [1, 5, 7], [1, 7, 3]], dtype=np.int32)
    arrays = meshstore.pack([cube.astype(np.float32), (cube - 0.5).astype(np.float32)], [0, 0], [cube_f], [0])
    out = _launch(_upload(arrays), np.array([[0], [0], [1]], dtype=np.int32), 257, 0, (8, 0, 2))
    diff = out["surface_samples_tgt"] - out["surface_samples_cano"]
    assert torch.equal(diff, torch.full_like(diff, -0.5))
    assert torch.equal(out["surface_normals_tgt"].view(torch.int32), out["surface_normals_cano"].view(torch.int32))
    assert torch.equal(out["surface_samples_src"], out["surface_samples_cano"])


# ------------------------------------------------------------------------------------------------------------------ the loader
@pytest.fixture(scope="module")
def mesh_tree(tmp_path_factory):
    """Three identities of three topologies x three motions (one held out) x three frames: 18 training pairs."""
    meshes = {"tet": mr.tetrahedron(), "oct": mr.octahedron(), "grid": mr.grid()}
    o2w = np.array([[0.9, 0.1, 0.0, 0.02], [-0.1, 0.9, 0.05, 0.0], [0.0, -0.05, 1.0, -0.01], [0, 0, 0, 1]])
    return synth.write_mesh_dataset_tree(str(tmp_path_factory.mktemp("meshes")), meshes, ["walk", "jump", "turn"], 3, mesh_file="mesh.obj",
                                         seed=9, orig2world=o2w)


def _host_arrays(store):
    return {"vert_arena": store.vert_arena.cpu().numpy(), "face_arena": store.face_arena.cpu().numpy(),
            "thr_arena": store.thr_arena.cpu().numpy().view(np.uint32), "frame_table": store.frame_table_host,
            "topo_table": store.topo_table_host}


def _equal_batches(a, b):
    return sorted(a) == sorted(b) and all(a[k].shape == b[k].shape and torch.equal(a[k].view(torch.uint8) if a[k].dtype == torch.bool
                                                                                   else a[k].view(torch.int32), b[k].view(torch.uint8) if
                                                                                   b[k].dtype == torch.bool else b[k].view(torch.int32)) for k in a)


def test_store_holds_the_meshes(mesh_tree):
    store = meshstore.MeshStore({"data": mesh_tree}, "identity_seen", "train_seen", device=DEV)
    assert len(store) == 18 and len(store.frames) == 18 and store.topo_table.shape == (3, 2) and (store.n, store.m) == (256, 128)
    assert store.vert_arena.shape == (6 * (4 + 18 + 121), 4) and store.face_arena.shape == (4 + 32 + 200, 4)
    assert store.thr_arena.shape == (4 + 32 + 200,)                                     # three canonical frames
    assert store.nbytes == 16 * 858 + 16 * 236 + 4 * 236 + 48 * 18 + 16 * 3 <= store.byte_budget
    for k, fr in enumerate(store.frames):
        verts, faces = meshstore.read_frame(mesh_tree, fr.dir)
        got_v, got_f = store.mesh(k)
        assert got_v.dtype == torch.float32 and got_f.dtype == torch.int32 and got_v.device == DEV
        assert np.array_equal(got_v.cpu().numpy(), verts) and np.array_equal(got_f.cpu().numpy(), faces)
        lo, hi = store.frame_bbox(k)
        assert np.array_equal(lo, verts.min(axis=0)) and np.array_equal(hi, verts.max(axis=0))      # of the VERTICES
    assert torch.all(store.vert_arena[:, 3] == 0) and torch.all(store.face_arena[:, 3] == 0)


def test_loader_epochs_shards_the_partial_batch_and_inverse(mesh_tree):
    store = meshstore.MeshStore({"data": mesh_tree}, "identity_seen", "train_seen", device=DEV)
    arrays = _host_arrays(store)
    loader = store.loader(5, seed=4)
    assert isinstance(loader, meshstore.MeshLoader) and len(loader) == 4
    epochs = [list(loader), list(loader)]
    assert [b["surface_samples_inputs"].shape[0] for b in epochs[0]] == [5, 5, 5, 3]              # the last batch: what remains
    for e, batches in enumerate(epochs):
        samples = loader.epoch_samples(e)
        assert sorted(samples.tolist()) == list(range(18))                                        # every pair once
        for step, batch in enumerate(batches):
            ids = np.ascontiguousarray(store.pair_frames[samples[step * 5:(step + 1) * 5]].T)
            assert _equal_batches(batch, store.assemble(torch.from_numpy(ids).to(DEV), 4, e, step))
            assert all(v.device == DEV and v.is_contiguous() for v in batch.values())
            if step in (0, 3):
                _assert_bit_equal(batch, mr.sample(arrays, ids, 256, 128, 4, e, step, 0.1, 0.1, 0.02), (e, step))
    assert not np.array_equal(loader.epoch_samples(0), loader.epoch_samples(1))
    again = list(store.loader(5, seed=4))
    assert all(_equal_batches(a, b) for a, b in zip(again, epochs[0])) and len(again) == 4        # one seed: equal batches
    assert not _equal_batches(list(store.loader(5, seed=5))[0], epochs[0][0])
    # the same samples at another step or epoch: other rows
    ids = torch.from_numpy(np.ascontiguousarray(store.pair_frames[:5].T)).to(DEV)
    assert not _equal_batches(store.assemble(ids, 4, 0, 0), store.assemble(ids, 4, 0, 1))
    assert not _equal_batches(store.assemble(ids, 4, 0, 0), store.assemble(ids, 4, 1, 0))
    # shard: of every world_size consecutive batches the rank-th, the trailing partial group dropped
    whole = list(store.loader(3, seed=4))                                                         # six batches
    for world in (2, 4):
        for rank in range(world):
            mine = list(store.loader(3, seed=4).shard(rank, world))
            assert len(mine) == 6 // world
            assert all(_equal_batches(m, whole[g * world + rank]) for g, m in enumerate(mine))
    # a validation store: the list as formed, no shuffle
    val = meshstore.MeshStore({"data": mesh_tree}, "identity_seen", "test_unseen_motions", device=DEV)
    vl = val.loader(4, seed=4)
    assert not vl.shuffle and vl.epoch_samples(0).tolist() == vl.epoch_samples(1).tolist() == list(range(len(val)))
    # inverse swaps src and tgt; noise (on the new src) comes from the generator
    inv = meshstore.MeshStore({"data": dict(mesh_tree, inverse=True)}, "identity_seen", "train_seen", device=DEV)
    a, b = epochs[0][0], next(iter(inv.loader(5, seed=4)))
    for what in ("surface_samples", "surface_normals", "space_samples"):
        assert torch.equal(a[f"{what}_src"], b[f"{what}_tgt"]) and torch.equal(a[f"{what}_tgt"], b[f"{what}_src"]), what
        assert torch.equal(a[f"{what}_cano"], b[f"{what}_cano"])
    noisy = meshstore.MeshStore({"data": dict(mesh_tree, noise_level=0.02)}, "identity_seen", "train_seen", device=DEV)
    gens = [torch.Generator(device=DEV).manual_seed(3) for _ in range(2)]
    c, d = (next(iter(noisy.loader(5, seed=4, noise_generator=g))) for g in gens)
    assert _equal_batches(c, d) and not torch.equal(c["surface_samples_src"], a["surface_samples_src"])
    assert torch.equal(c["surface_samples_tgt"], a["surface_samples_tgt"])
    assert torch.equal(c["surface_samples_inputs"][..., :3], c["surface_samples_src"])


# ------------------------------------------------------------------------------------------------------------------ training
def _tiny_config(mesh_tree):
    cfg = model_cfg("forward", [256, 64, 16])
    cfg["data"] = dict(mesh_tree)
    cfg["training"] = {"epochs": 2, "save_frequency": 2, "optimizer": "Adam", "lr": 5e-4, "lr_step": 2, "lr_decay": 0.1,
                       "weight_decay": 0.0, "iden_split": "identity_seen", "motion_split": "train_seen", "batch_size": 9}
    cfg["validation"] = {"frequency": 1, "iden_split": "identity_seen", "motion_split": "test_unseen_motions", "batch_size": 3}
    return cfg


def test_a_step_on_a_loader_batch_equals_the_step_on_prepare_batch(mesh_tree):
    """``prepare_batch`` is fed the EMULATION's sampled clouds as full frames with identity row indices.  It takes the handle
    mask's box from the full canonical cloud, so two rows are appended to it that hold the corners of the canonical frame's
    vertex box (the store's documented box; identity indices never pick them): every sampled row lies inside that box, which
    the bit-equal batches confirm."""
    from nsdp_amd.model import build_model, optimizer_factory
    cfg = _tiny_config(mesh_tree)
    store = meshstore.MeshStore(cfg, "identity_seen", "train_seen", device=DEV)
    loader = store.loader(4, seed=8)
    batch = next(iter(loader))
    picks = loader.epoch_samples(0)[:4]
    ids = np.ascontiguousarray(store.pair_frames[picks].T)
    ref = mr.sample(_host_arrays(store), ids, 256, 128, 8, 0, 0, 0.1, 0.1, 0.02)
    boxes = np.stack([np.stack(store.frame_bbox(int(c))) for c in ids[0]])                # (B, 2, 3)
    full = {}
    for name in ("cano", "src", "tgt"):
        extra = boxes if name == "cano" else np.zeros_like(boxes)
        full[name] = {"surface_samples": np.concatenate([ref[f"surface_samples_{name}"], extra], axis=1),
                      "surface_normals": np.concatenate([ref[f"surface_normals_{name}"], np.zeros_like(boxes)], axis=1),
                      "space_samples": ref[f"space_samples_{name}"]}
        full[name] = {k: torch.from_numpy(np.ascontiguousarray(v)).to(DEV) for k, v in full[name].items()}
    rows = torch.arange(256, dtype=torch.int32, device=DEV).repeat(4, 1).contiguous()
    torch_batch = dataset.prepare_batch(cfg["data"], full["cano"], full["src"], full["tgt"], rows)
    assert _equal_batches(batch, torch_batch)
    losses = []
    for data_dict in (batch, torch_batch):
        train.seed_everything(27)
        model, train_fn, _, _ = build_model(cfg, device=DEV)
        _, opt = optimizer_factory(cfg["training"], model.parameters())
        model.train()
        losses.append([float(train_fn(model, opt, data_dict, cfg)) for _ in range(2)])
    assert losses[0] == losses[1] and all(np.isfinite(losses[0])), losses


def test_training_from_the_mesh_store_replayed_and_eager(mesh_tree, tmp_path):
    from nsdp_amd.graph_step import GraphedTrainOnBatch, capturable_adam
    from nsdp_amd.model import build_model, optimizer_factory
    cfg = _tiny_config(mesh_tree)
    hists, weights = [], []
    for graph in (False, True):
        train.seed_everything(27)
        model, train_fn, val_fn, _ = build_model(cfg, device=DEV)
        sched, opt = optimizer_factory(cfg["training"], model.parameters())
        capturable_adam(opt)        # (both runs on the fused capturable Adam: the same arithmetic, so the runs can be held EQUAL)
        loader, val = train.mesh_dataset_loaders(cfg, 27, DEV, log=lambda *_: None)
        assert isinstance(loader, meshstore.MeshLoader) and len(loader) == 2 and loader.batch == 9 and val.batch == 3
        assert loader.shuffle and not val.shuffle
        fn = GraphedTrainOnBatch(train_fn) if graph else train_fn
        args = argparse.Namespace(continue_from_epoch=0, best_val_loss=float("inf"))
        sub = tmp_path / ("g" if graph else "e")
        sub.mkdir()
        hists.append(train.fit(model, (fn, val_fn), sched, opt, loader, val, cfg, str(sub), args, DEV, log=lambda *_: None))
        weights.append({k: v.detach().clone() for k, v in model.state_dict().items()})
        if graph:
            assert fn.replays >= 2 and fn.eager_calls >= 1
    e, g = [[h[2] for h in hist if h[0] == "train"] for hist in hists]
    ve, vg = [[h[2] for h in hist if h[0] == "val"] for hist in hists]
    print("epoch losses", e, "validation", ve)
    assert len(e) == len(g) == 2 and e == g, (e, g)
    assert ve == vg and len(ve) >= 1, (ve, vg)
    assert all(np.isfinite(e))
    assert all(torch.equal(weights[0][k], weights[1][k]) for k in weights[0])
