#!/usr/bin/env python3
"""Fast global registration of the val pairs on the GPU: the `o3_gicp_fast` ICP baseline of the reference (icp.py:121-143, 150-213 with
variant "o3_gicp_fast" and no refine): FGR (Zhou, Park, Koltun, ECCV 2016) on FPFH feature matches of the 5 cm voxel-downsampled FULL
clouds, maximum_correspondence_distance 0.025, no ICP after it.

    python icp_global_fast.py --config configs/icp_<dataset>_o3_gicp_fast.json [--use_old_results] [--seed S]

The twin of icp_global.py: it writes into <logdir>/val/eval000000 what train.py's ICP mode writes (pred_translations.npy = T[:3, 3],
pred_angles.npy = the z component of T's rotation vector, zero pred_s1_pc1centers.npy, eval.json / eval_180.json with mean_time =
registration wall time / nval), which is what `train.py train --config configs/icp_<dataset>_o3_gicp_fast_p2p.json` then refines with
point-to-point ICP.  The clouds are uploaded to HBM once and registered in chunks (alignnet_fgr_register_dataset); the tuple draws of a
pair are selected by --seed and the pair's example id in val.txt.  Open3D is not available next to this stack: the computation is this
project's restatement (tests/fgr_ref.py), statistically, not numerically, comparable with the reference's.  decrease_mu is passed as False:
the default of the Open3D 0.7 Python binding as remembered, which could not be checked; DECREASE_MU below is the one
place to change if that is wrong."""
import argparse
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import icp_global_common as common  # noqa: E402
from icp_global_common import cfg  # noqa: E402

DECREASE_MU = False
MAXIMUM_CORRESPONDENCE_DISTANCE = 0.025   # icp.py:136
ACCEPTS = "icp_global_fast.py accepts evaluation.special.mode = \"icp\" with icp.variant = \"o3_gicp_fast\" and no icp.refine"


def parse_args(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("--config", required=True, help="Config file (icp_*_o3_gicp_fast.json)")
    p.add_argument("--use_old_results", action="store_true", help="Re-evaluate the stored results instead of registering")
    p.add_argument("--seed", type=int, default=0, help="Seed of the tuple draws")
    return p.parse_args(argv)


def check_config():
    special = cfg.evaluation.special if cfg.evaluation.has("special") else None
    if special is None or special.mode != "icp":
        raise ValueError("%s (this config has %s)" % (ACCEPTS, "no evaluation.special" if special is None else "mode = %r" % (special.mode,)))
    icp = special.icp
    refine = icp.refine if icp.has("refine") else None
    if icp.variant != "o3_gicp_fast" or refine is not None:
        raise ValueError("%s (this config has variant = %r, refine = %r; o3_gicp is icp_global.py, the refine step is `train.py train` on that config)"
                         % (ACCEPTS, icp.variant, refine))
    return icp


def run(flags):
    common.run(flags, check_config(), "Fast global registration", "tuple draws",
               lambda engine, rows, streams, constrained: engine.fgr_register_rows(
                   rows, constrained=constrained, decrease_mu=DECREASE_MU, seed=flags.seed, streams=streams,
                   maximum_correspondence_distance=MAXIMUM_CORRESPONDENCE_DISTANCE),
               lambda constrained, nval, total_time, fitness: "Fast global registration (o3_gicp_fast: FPFH + FGR, %s estimate, decrease_mu %s, seed %d) on %d pairs: "
               "%.3f s, mean fitness %.3f" % ("z-constrained" if constrained else "full-rotation", DECREASE_MU, flags.seed, nval, total_time, fitness))


def main(argv=None):
    common.main(parse_args(argv), check_config, run)


if __name__ == "__main__":
    main()
