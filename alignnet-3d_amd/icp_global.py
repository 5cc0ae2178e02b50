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
import datetime
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import provider  # noqa: E402
import evaluation  # noqa: E402
import train  # noqa: E402
from config import load_config, save_config, configGlobal as cfg  # noqa: E402

logger = train.logger
GLOBAL_CHUNK = 1024   # pairs per registration call
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
    icp = check_config()
    val = provider.getDataFiles("%s/split/val.txt" % cfg.data.basepath)
    nval = len(val)
    constrained = bool(icp.with_constraint)
    packed = provider.use_packed_cache()
    labels = provider.load_batch(val, override_batch_size=nval, dont_load_pointclouds=True)
    gt_t, gt_a, gt_c1 = labels[2], labels[3], labels[4]
    eval_dir = "%s/val/eval%s" % (cfg.logging.logdir, str(0).zfill(6))
    total_time = 0.0
    if flags.use_old_results and os.path.isfile("%s/pred_translations.npy" % eval_dir):
        pred_t = np.load("%s/pred_translations.npy" % eval_dir)
        pred_a = np.load("%s/pred_angles.npy" % eval_dir)
        pred_c = np.load("%s/pred_s1_pc1centers.npy" % eval_dir)
        logger.info("Global registration results of %s re-evaluated" % eval_dir)
    else:
        import alignnet3d
        engine = alignnet3d.Engine(cfg)
        packed.upload(engine)
        rows = packed.rows_of(val)
        streams = np.asarray([int(e) for e in val], np.int64)
        if streams.min() < 0 or streams.max() >= 1 << 24:
            raise ValueError("example ids of val.txt must lie in [0, 2^24) to select the RANSAC draws")
        pred_t, pred_a = np.empty((nval, 3), np.float32), np.empty((nval, 1), np.float32)
        pred_c = np.zeros((nval, 3), np.float32)   # the transforms are about the origin (icp.py:193-194)
        fitness = np.empty(nval)
        for s in range(0, nval, GLOBAL_CHUNK):
            e = min(s + GLOBAL_CHUNK, nval)
            t0 = time.time()
            res = engine.global_register_rows(rows[s:e], constrained=constrained, seed=flags.seed, streams=streams[s:e])
            total_time += time.time() - t0
            T = res["transforms"]
            pred_t[s:e] = T[:, :3, 3]
            pred_a[s:e, 0] = evaluation.rotvec_z(T[:, :3, :3])
            fitness[s:e] = res["fitness"]
        engine.close()
        os.makedirs(eval_dir, exist_ok=True)
        np.save("%s/pred_translations.npy" % eval_dir, pred_t)
        np.save("%s/pred_angles.npy" % eval_dir, pred_a)
        np.save("%s/pred_s1_pc1centers.npy" % eval_dir, pred_c)
        logger.info("Global registration (o3_gicp: FPFH + RANSAC, %s estimate, seed %d) on %d pairs: %.3f s, mean fitness %.3f"
                    % ("z-constrained" if constrained else "full-rotation", flags.seed, nval, total_time, float(fitness.mean())))
    mean_time = total_time / nval
    for inv in (False, True):
        ev = evaluation.evaluate(cfg, val, pred_t, pred_a, gt_t, gt_a, pred_c, gt_c1, eval_dir=eval_dir, accept_inverted_angle=inv, mean_time=mean_time)
        logger.info(evaluation.ns_to_dict(ev))


def main(argv=None):
    flags = parse_args(argv)
    load_config(flags.config)
    check_config()   # before anything is written or an engine is made
    os.makedirs(cfg.logging.logdir, exist_ok=True)
    copyfile = "%s/config.json" % cfg.logging.logdir
    if os.path.exists(copyfile):
        copyfile = "%s_%s.json" % (copyfile[:-5], datetime.datetime.today().strftime("%Y-%m-%d_%H-%M-%S"))
    save_config(copyfile)
    train.setup_logging(cfg.logging.logdir, 0)
    logger.debug(cfg)
    run(flags)


if __name__ == "__main__":
    main()
