"""Write a procedural data set in the reference's directory layout (nsdp_amd.synth.write_dataset_tree) and print the ``data``
section of a config that reads it -- the only data the tests and tools/bench_datastore.py have; nothing is downloaded.

    python tools/make_procedural_dataset.py DIR --identities bear fox --motions walk jump turn --frames 8 \\
        --surface 200000 --space 200000 --dtype float16 [--type deformtransfer]
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from nsdp_amd import synth  # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("dir")
    ap.add_argument("--identities", nargs="+", default=["bear", "fox"])
    ap.add_argument("--motions", nargs="+", default=["walk", "jump"])
    ap.add_argument("--frames", type=int, default=4)
    ap.add_argument("--surface", type=int, nargs="+", default=[200000], help="surface rows per frame: one count, or one per identity")
    ap.add_argument("--space", type=int, nargs="+", default=[200000], help="space rows per frame: one count, or one per identity")
    ap.add_argument("--dtype", choices=["float16", "float32"], default="float16")
    ap.add_argument("--type", dest="data_type", choices=["deform4d", "deformtransfer"], default="deform4d")
    ap.add_argument("--held-out-motions", type=int, default=1, help="motions kept for test_unseen_motions.lst")
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args(argv)
    one = lambda v: v[0] if len(v) == 1 else v
    data = synth.write_dataset_tree(args.dir, args.identities, args.motions, args.frames, one(args.surface), one(args.space),
                                    np.dtype(args.dtype).type, data_type=args.data_type, seed=args.seed,
                                    held_out_motions=args.held_out_motions)
    import yaml
    print(yaml.safe_dump({"data": data}, sort_keys=False))
    return 0


if __name__ == "__main__":
    sys.exit(main())
