"""tests/golden/dataset_tree.npz (tools/make_golden_dataset_tree.py) for the data-store tests: the recorded trees rebuilt on disk,
the recorded cases and their configurations."""
import json
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "dataset_tree.npz")
FILES = {"norm_params_file": "orig_to_gaps.txt", "surface_flow_file": "surface_points.npz", "space_flow_file": "flow.npz"}
_cache = {}


def golden():
    if "z" not in _cache:
        with np.load(GOLDEN) as z:
            _cache["z"] = {k: z[k] for k in z.files}
    return _cache["z"]


def rebuild(kind, root):
    """Write the recorded tree ``kind`` under ``root`` (files in the recorded dtypes) and return the ``data`` section for it."""
    z = golden()
    dataset_dir, split_dir = os.path.join(root, kind, "dataset"), os.path.join(root, kind, "splits")
    prefix = f"tree/{kind}/"
    for key in z:
        if key.startswith(prefix) and key.endswith("/surface_points"):
            seq, frame = key[len(prefix):].split("/")[:2]
            d = os.path.join(dataset_dir, seq, frame)
            os.makedirs(d, exist_ok=True)
            base = f"{prefix}{seq}/{frame}/"
            np.savez(os.path.join(d, FILES["surface_flow_file"]), points=z[base + "surface_points"], normals=z[base + "surface_normals"])
            np.savez(os.path.join(d, FILES["space_flow_file"]), points=z[base + "space_points"])
            np.savetxt(os.path.join(d, FILES["norm_params_file"]), np.eye(4))
    os.makedirs(os.path.join(split_dir, kind), exist_ok=True)
    for key in z:
        if key.startswith(f"split/{kind}/"):
            with open(os.path.join(split_dir, kind, key.rsplit("/", 1)[1] + ".lst"), "w") as f:
                f.write("\n".join(str(s) for s in z[key]))
    data = {"type": kind, "dataset_dir": dataset_dir, "split_dir": split_dir, "interval": 1, "arbitrary": False, "inverse": False,
            "fix_coord_system": False, "num_surf_samples": 16, "num_space_samples": 8, "partial_range": 0.1, "noise_level": 0.0,
            "partial_shape_ratio": 1.0}
    data.update(FILES)
    return data


def cases(group):
    """{case name: its recorded config} of ``group`` ('pairs' or 'item')."""
    z = golden()
    out = {}
    for key in z:
        if key.startswith(group + "/") and key.endswith("/config"):
            out[key[len(group) + 1:-len("/config")]] = json.loads(str(z[key]))
    return out


def case_data(data, cfg):
    """The ``data`` section of a recorded case over a rebuilt tree's."""
    out = dict(data)
    out.update({k: v for k, v in cfg.items() if k not in ("tree", "motion_split", "num_sampled_pairs")})
    return out


def pair_rows(pairs):
    return [[str(v) for v in p] for p in pairs]
