#!/usr/bin/env python3
"""Global registration of the val pairs on the GPU: the `o3_gicp` ICP baseline of the reference (icp.py:85-143, 150-213 with
variant "o3_gicp" and no refine): RANSAC on FPFH feature matches of the 5 cm voxel-downsampled FULL clouds, no ICP after it.

    python icp_global.py --config configs/icp_<dataset>_o3_gicp.json [--use_old_results] [--seed S]

Writes into <logdir>/val/eval000000 what train.py's ICP mode writes (pred_translations.npy = T[:3, 3], pred_angles.npy = the z component
of T's rotation vector, zero pred_s1_pc1centers.npy, eval.json / eval_180.json with mean_time = registration wall time / nval), which is
what `train.py train --config configs/icp_<dataset>_o3_gicp_p2p.json` then refines with point-to-point ICP.  The clouds are uploaded to
HBM once and registered in chunks (alignnet_global_register_dataset); the random draws of a pair are selected by --seed and the pair's
example id in val.txt, so a pair's result does not depend on the split around it.  Open3D is not available next to this stack: the
computation is this project's restatement (tests/global_reg_ref.py), statistically, not numerically, comparable with the reference's."""
import argparse
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import icp_global_common as common  # noqa: E402
from icp_global_common import cfg  # noqa: E402

GLOBAL_CHUNK = common.GLOBAL_CHUNK   # pairs per registration call
ACCEPTS = "icp_global.py accepts evaluation.special.mode = \"icp\" with icp.variant = \"o3_gicp\" and no icp.refine"


def parse_args(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("--config", required=True, help="Config file (icp_*_o3_gicp.json)")
    p.add_argument("--use_old_results", action="store_true", help="Re-evaluate the stored results instead of registering")
    p.add_argument("--seed", type=int, default=0, help="Seed of the RANSAC draws")
    return p.parse_args(argv)


def check_config():
    special = cfg.evaluation.special if cfg.evaluation.has("special") else None
    if special is None or special.mode != "icp":
        raise ValueError("%s (this config has %s)" % (ACCEPTS, "no evaluation.special" if special is None else "mode = %r" % (special.mode,)))
    icp = special.icp
    refine = icp.refine if icp.has("refine") else None
    if icp.variant != "o3_gicp" or refine is not None:
        raise ValueError("%s (this config has variant = %r, refine = %r; the refine step is `train.py train` on that config)"
                         % (ACCEPTS, icp.variant, refine))
    return icp


def run(flags):
    common.run(flags, check_config(), "Global registration", "RANSAC draws",
               lambda engine, rows, streams, constrained: engine.global_register_rows(rows, constrained=constrained, seed=flags.seed, streams=streams),
               lambda constrained, nval, total_time, fitness: "Global registration (o3_gicp: FPFH + RANSAC, %s estimate, seed %d) on %d pairs: %.3f s, mean fitness %.3f"
               % ("z-constrained" if constrained else "full-rotation", flags.seed, nval, total_time, fitness))


def main(argv=None):
    common.main(parse_args(argv), check_config, run)


if __name__ == "__main__":
    main()
