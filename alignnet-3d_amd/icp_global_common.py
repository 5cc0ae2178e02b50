"""What icp_global.py (o3_gicp: RANSAC) and icp_global_fast.py (o3_gicp_fast: FGR) share: the val pairs of the HBM-resident dataset are
registered in chunks, streams = example ids, and the results written into <logdir>/val/eval000000 as train.py's ICP mode writes them."""
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


def run(flags, icp, title, draws, register, summary):
    """icp: the checked evaluation.special.icp node.  title: "Global registration" / "Fast global registration" (the re-evaluation's log
    line); draws: what the example ids select (error message); register(engine, rows, streams, constrained) -> result dict of one chunk;
    summary(constrained, nval, total_time, mean_fitness) -> the log line after registering."""
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
        logger.info("%s results of %s re-evaluated" % (title, eval_dir))
    else:
        import alignnet3d
        engine = alignnet3d.Engine(cfg)
        packed.upload(engine)
        rows = packed.rows_of(val)
        streams = np.asarray([int(e) for e in val], np.int64)
        if streams.min() < 0 or streams.max() >= 1 << 24:
            raise ValueError("example ids of val.txt must lie in [0, 2^24) to select the %s" % draws)
        pred_t, pred_a = np.empty((nval, 3), np.float32), np.empty((nval, 1), np.float32)
        pred_c = np.zeros((nval, 3), np.float32)   # the transforms are about the origin (icp.py:193-194)
        fitness = np.empty(nval)
        for s in range(0, nval, GLOBAL_CHUNK):
            e = min(s + GLOBAL_CHUNK, nval)
            t0 = time.time()
            res = register(engine, rows[s:e], streams[s:e], constrained)
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
        logger.info(summary(constrained, nval, total_time, float(fitness.mean())))
    mean_time = total_time / nval
    for inv in (False, True):
        ev = evaluation.evaluate(cfg, val, pred_t, pred_a, gt_t, gt_a, pred_c, gt_c1, eval_dir=eval_dir, accept_inverted_angle=inv, mean_time=mean_time)
        logger.info(evaluation.ns_to_dict(ev))


def main(flags, check_config, run_command):
    load_config(flags.config)
    check_config()   # before anything is written or an engine is made
    os.makedirs(cfg.logging.logdir, exist_ok=True)
    copyfile = "%s/config.json" % cfg.logging.logdir
    if os.path.exists(copyfile):
        copyfile = "%s_%s.json" % (copyfile[:-5], datetime.datetime.today().strftime("%Y-%m-%d_%H-%M-%S"))
    save_config(copyfile)
    train.setup_logging(cfg.logging.logdir, 0)
    logger.debug(cfg)
    run_command(flags)
