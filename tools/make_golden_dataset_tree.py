"""Generates tests/golden/dataset_tree.npz: two tiny procedural data-set trees (nsdp_amd.synth.write_dataset_tree) and what the
REFERENCE's dataset classes make of them -- pair lists, reshuffled lists and a few ``__getitem__`` outputs.  The reference's
classes are imported from a read-only checkout (``tkinter``, ``skimage``, ``open3d`` and ``trimesh`` stubbed: unused by what runs
here); the fixture holds data only: arrays and name lists.  Run on the build machine only:

    python tools/make_golden_dataset_tree.py --reference /path/to/NSDP

tests/test_datastore_cpu.py and tests/test_datastore_gpu.py rebuild the trees from the recorded arrays (tests/datastore_tree.py).
"""
import argparse
import copy
import json
import os
import sys
import tempfile
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from nsdp_amd import synth  # noqa: E402

TREES = {
    # two identities of different counts, one of them in fp32 files: the surface arena of a store over both is fp32
    "deform4d": dict(identities=["bear", "fox"], motions=["walk", "jump", "turn"], frames=5, n_surface=[24, 30], n_space=[16, 20],
                     dtype={"bear": np.float16, "fox": np.float32}, data_type="deform4d", seed=41),
    # the animals that pick the source frame of the evaluation pairs (0003, 0005, 0001)
    "deformtransfer": dict(identities=["cat", "horse", "dog"], motions=["run"], frames=7, n_surface=24, n_space=16,
                           dtype=np.float16, data_type="deformtransfer", seed=43, held_out_motions=0),
}
PAIR_CASES = [(kind, arbitrary, split) for kind in TREES for arbitrary in (False, True) for split in ("train_seen", "test_unseen_motions")]
SAMPLED = 5
# (name, tree, data overrides, motion split, indices)
ITEM_CASES = [
    ("forward", "deform4d", dict(arbitrary=False, inverse=False), "train_seen", [0, 3, 7]),
    ("backward_noise", "deform4d", dict(arbitrary=False, inverse=True, noise_level=0.02, interval=2), "train_seen", [1, 2]),
    ("arbitrary_eval", "deform4d", dict(arbitrary=True), "test_unseen_motions", [2, 5]),
    ("transfer_fixed", "deformtransfer", dict(arbitrary=True, fix_coord_system=True), "test_unseen_motions", [0, 4, 9]),
]
NUM_SURF, NUM_SPACE = 16, 8


def case_name(kind, arbitrary, split):
    return f"{kind}/{'arbitrary' if arbitrary else 'canonical'}/{split}"


def import_reference(path):
    for name in ("tkinter", "skimage", "open3d", "trimesh"):
        sys.modules.setdefault(name, types.ModuleType(name))
    sys.modules["tkinter"].E = "e"
    sys.modules["skimage"].io = sys.modules["skimage"].transform = None
    try:
        import tqdm  # noqa: F401
    except ImportError:
        sys.modules["tqdm"] = types.ModuleType("tqdm")
        sys.modules["tqdm"].tqdm = lambda x, **k: x
    sys.path.insert(0, path)
    from dataset import dataset_dict
    return dataset_dict


def pair_array(pairs):
    return np.array([[str(v) for v in p["pair_info"]] for p in pairs], dtype=np.str_).reshape(len(pairs), 8)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reference", required=True, help="checkout of the reference implementation (read only)")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "dataset_tree.npz"))
    args = ap.parse_args()
    classes = import_reference(os.path.abspath(args.reference))
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        data = {}
        for kind, spec in TREES.items():
            data[kind] = synth.write_dataset_tree(os.path.join(tmp, kind), **spec)
            base = data[kind]["dataset_dir"]
            for seq in sorted(os.listdir(base)):
                for frame in sorted(os.listdir(os.path.join(base, seq))):
                    d = os.path.join(base, seq, frame)
                    s, q = np.load(os.path.join(d, data[kind]["surface_flow_file"])), np.load(os.path.join(d, data[kind]["space_flow_file"]))
                    out[f"tree/{kind}/{seq}/{frame}/surface_points"] = s["points"]
                    out[f"tree/{kind}/{seq}/{frame}/surface_normals"] = s["normals"]
                    out[f"tree/{kind}/{seq}/{frame}/space_points"] = q["points"]
            for split in ("identity_seen", "train_seen", "test_unseen_motions"):
                with open(os.path.join(data[kind]["split_dir"], kind, split + ".lst")) as f:
                    out[f"split/{kind}/{split}"] = np.array(f.read().split("\n"), dtype=np.str_)
        for kind, arbitrary, split in PAIR_CASES:
            cfg = {"data": dict(data[kind], arbitrary=arbitrary, interval=2 if arbitrary else 1)}
            name = case_name(kind, arbitrary, split)
            out[f"pairs/{name}/config"] = np.array(json.dumps(dict(tree=kind, arbitrary=arbitrary, interval=cfg["data"]["interval"],
                                                                   motion_split=split, num_sampled_pairs=SAMPLED)), dtype=np.str_)
            ds = classes[kind](cfg, "identity_seen", split)
            out[f"pairs/{name}/loaded"] = pair_array(ds.sample_deform_pairs)
            ds.random_shuffle_samples(-1)
            out[f"pairs/{name}/reshuffled"] = pair_array(ds.sample_deform_pairs)
            ds = classes[kind](cfg, "identity_seen", split, num_sampled_pairs=SAMPLED)
            out[f"pairs/{name}/loaded_sampled"] = pair_array(ds.sample_deform_pairs)
            ds.random_shuffle_samples(SAMPLED)
            out[f"pairs/{name}/reshuffled_sampled"] = pair_array(ds.sample_deform_pairs)
        for name, kind, over, split, indices in ITEM_CASES:
            cfg = {"data": dict(data[kind], num_surf_samples=NUM_SURF, num_space_samples=NUM_SPACE)}
            cfg["data"].update(over)
            ds = classes[kind](copy.deepcopy(cfg), "identity_seen", split)
            assert max(indices) < len(ds) - 1, (name, len(ds))          # (the last index of a train split reshuffles)
            out[f"item/{name}/indices"] = np.array(indices, dtype=np.int64)
            out[f"item/{name}/config"] = np.array(json.dumps(dict(over, tree=kind, motion_split=split, num_surf_samples=NUM_SURF,
                                                                  num_space_samples=NUM_SPACE)), dtype=np.str_)
            for i in indices:
                np.random.seed(1000 + i)
                item = ds[i]
                info = ds.sample_deform_pairs[i]["pair_info"]
                full = np.load(os.path.join(cfg["data"]["dataset_dir"], info[1], info[2], cfg["data"]["surface_flow_file"]))["points"].shape[0]
                full_space = np.load(os.path.join(cfg["data"]["dataset_dir"], info[1], info[2], cfg["data"]["space_flow_file"]))["points"].shape[0]
                np.random.seed(1000 + i)                                  # replay the draws of __getitem__, in its order
                out[f"item/{name}/{i}/surf_idx"] = np.random.permutation(full)[:NUM_SURF].astype(np.int32)
                if cfg["data"]["noise_level"] > 0.0:
                    out[f"item/{name}/{i}/noise"] = np.random.randn(NUM_SURF, 3).astype(np.float32)
                assert full_space > NUM_SPACE
                out[f"item/{name}/{i}/space_idx"] = np.random.permutation(full_space)[:NUM_SPACE].astype(np.int32)
                for key, value in item.items():
                    if key != "index":
                        out[f"item/{name}/{i}/{key}"] = np.asarray(value)
    np.savez_compressed(args.out, **out)
    print("wrote", args.out, os.path.getsize(args.out), "bytes,", len(out), "entries")


if __name__ == "__main__":
    main()
