#!/usr/bin/env python3
"""Register one pair of clouds with a trained model, in one engine call (Engine.register: sampler, network, decode, initial
transform and optionally ICP on the full clouds, all on the device).

    python register_pair.py --config F --model CKPT --source a.npy --target b.npy [--refine p2p|plane|generalized] [--its K] [--seed S]

CKPT is a `.aln3` checkpoint as train.py writes it.  Prints the 4x4 that maps the source onto the target, then fitness and rmse
of the refinement (n/a without --refine)."""
import argparse
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

from config import load_config, configGlobal as cfg  # noqa: E402

REFINE = {None: None, "p2p": "point", "plane": "plane", "generalized": "generalized"}


def parse_args(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("--config", required=True, help="Config file of the model")
    p.add_argument("--model", required=True, help="Checkpoint (.aln3)")
    p.add_argument("--source", required=True, help="[n, >=3] .npy cloud to move")
    p.add_argument("--target", required=True, help="[m, >=3] .npy cloud to move it onto")
    p.add_argument("--refine", choices=["p2p", "plane", "generalized"], default=None, help="ICP refinement of the network's transform on the full clouds")
    p.add_argument("--its", type=int, default=30, help="ICP iterations")
    p.add_argument("--seed", type=int, default=0, help="Seed of the sampler's draw")
    return p.parse_args(argv)


def main(argv=None):
    args = parse_args(argv)
    load_config(args.config)
    import alignnet3d
    engine = alignnet3d.Engine(cfg)
    engine.load(args.model)
    source, target = (np.load(f)[:, :3] for f in (args.source, args.target))
    res = engine.register([source], [target], seed=args.seed, refine=REFINE[args.refine], its=args.its)
    engine.close()
    np.set_printoptions(precision=17, suppress=False, linewidth=200)
    for row in res["transforms"][0]:
        print(" ".join(repr(float(v)) for v in row))
    if args.refine:
        print("fitness %r rmse %r" % (float(res["fitness"][0]), float(res["rmse"][0])))
    else:
        print("fitness n/a rmse n/a")
    return res


if __name__ == "__main__":
    main()
