"""GPU: held data end to end.  A tiny KITTI-style tree (one sequence, 5 frames, 2 tracks) as a tracker would leave it -> make_kitti_dataset.py
--held -> train.py in held mode with evaluation.reg_eval on a checkpoint of random weights: one speed file per track, eval_held.json, no eval.json."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import alignnet3d
from alignnet3d import tracklets as T

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "alignnet-3d_amd")
FRAMES = {1: range(0, 5), 2: range(1, 4)}   # track id -> its frames: 4 pairs and 2 pairs


def _box(track, frame):
    """(x, y, z, h, w, l, ry) in the camera frame: two cars driving along the camera's z at different speeds, downhill by 0.3 m per frame"""
    return np.array([3.0 * track - 4.0, 1.6 + 0.3 * frame, 12.0 + 6.0 * track + (0.8 + 0.3 * track) * frame, 1.5, 1.7, 4.0, 0.05 * track])


def _make_tree(root):
    rng = np.random.default_rng(8)
    os.makedirs(os.path.join(root, "training", "velodyne", "0000"))
    os.makedirs(os.path.join(root, "training", "label_02"))
    lines = []
    for frame in range(5):
        pts = [np.concatenate([rng.uniform(5, 40, (80, 1)), rng.uniform(-15, 15, (80, 1)), rng.uniform(-1.7, -1.5, (80, 1))], 1)]   # ground returns
        for track, frames in FRAMES.items():
            if frame not in frames:
                continue
            b = _box(track, frame)
            c, s = np.cos(b[6]), np.sin(b[6])
            local = rng.uniform([-b[5] / 2, -b[3], -b[4] / 2], [b[5] / 2, 0.0, b[4] / 2], (150, 3)) * 0.95
            cam = local @ np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]]).T + b[:3]
            pts.append(cam @ T.R)                                                                                                 # velodyne = camera @ R
            # 17 columns and a score, as trackers write them
            lines.append("%d %d Car 0 0 -1.5 100 120 200 220 %.4f %.4f %.4f %.4f %.4f %.4f %.4f 0.93\n" % (frame, track, b[3], b[4], b[5], b[0], b[1], b[2], b[6]))
        scan = np.concatenate(pts).astype(np.float32)
        np.concatenate([scan, np.zeros((len(scan), 1), np.float32)], 1).tofile(os.path.join(root, "training", "velodyne", "0000", "%06d.bin" % frame))
    open(os.path.join(root, "training", "label_02", "0000.txt"), "w").write("".join(lines))


def _run(script, args, cwd):
    env = dict(os.environ, PYTHONPATH=PKG + os.pathsep + ROOT)
    r = subprocess.run([sys.executable, os.path.join(PKG, script)] + args, cwd=cwd, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return r.stdout + r.stderr


def test_held_dataset_and_held_evaluation(gpu_required, tmp_path):
    kitti, data = tmp_path / "tracker_out", tmp_path / "HeldTiny"
    _make_tree(str(kitti))
    out = _run("make_kitti_dataset.py", ["--kitti", str(kitti), "--out", str(data), "--held", "--frame-rate", "10"], str(tmp_path))
    assert "wrote 6 pairs (0 train, 6 val)" in out
    assert open(data / "split" / "train.txt").read() == "" and open(data / "split" / "val.txt").read().split() == [str(i) for i in range(6)]
    metas = [json.load(open(data / "meta" / ("%08d.json" % i))) for i in range(6)]
    assert sorted(m["trackid"] for m in metas) == [1, 1, 1, 1, 2, 2]
    for i, m in enumerate(metas):
        assert m["timestamps"] == [m["frames"][0] / 10.0, m["frames"][1] / 10.0] and m["rel_angle"] == 0.0
        assert np.array_equal(np.load(data / "transform" / ("%08d.npy" % i)), np.eye(4))
        p1, p2 = np.load(data / "pointcloud1" / ("%08d.npy" % i)), np.load(data / "pointcloud2" / ("%08d.npy" % i))
        assert 100 <= len(p1) <= 160 and 100 <= len(p2) <= 160
        # nothing was subtracted from the second crop: it sits 0.3 m lower, where the scan has it (FromKITTIScene would have levelled the two)
        assert -0.45 < p2[:, 2].mean() - p1[:, 2].mean() < -0.15
    # a checkpoint of random weights in another run's logdir, then the held evaluation
    user = {"data": {"basepath": str(data)}, "logging": {"basedir": str(tmp_path / "logs")},
            "model": {"num_points": 64, "angles": {"num_bins": 12, "accept_inverted_angle": True},
                      "options": {"s1transformer": [[32, 64, 96], [[64, 32], 0.7]], "s2transformer": [[32, 64, 128], [[64, 32], 0.7]],
                                  "embedding": [32, 64, 160], "remaining_transform_prediction": [[64, 32], 0.7]}},
            "training": {"batch_size": 4},
            "evaluation": {"special": {"mode": "held", "held": {"model": str(tmp_path / "other_run")}}, "reg_eval": {"threshold": 0.5}}}
    cfgp = tmp_path / "HeldRun.json"
    json.dump(user, open(cfgp, "w"))
    sys.path.insert(0, PKG)
    import config as cfgmod
    cfgmod.reset_config()
    try:
        eng = alignnet3d.Engine(cfgmod.load_config(str(cfgp)))
        os.makedirs(tmp_path / "other_run")
        eng.save(str(tmp_path / "other_run" / "model-0.aln3"))
        eng.close()
    finally:
        cfgmod.reset_config()
    out = _run("train.py", ["eval_only", "--config", str(cfgp), "--eval_epoch", "0"], str(tmp_path))
    ev = tmp_path / "logs" / "HeldRun" / "val" / "eval000000"
    assert "Held evaluation: 2 tracks" in out
    for track, frames in FRAMES.items():
        speeds = [float(x) for x in open(ev / ("track%d.txt" % track)).read().split()]
        assert len(speeds) == len(frames) - 1 and np.isfinite(speeds).all() and min(speeds) >= 0.0
    q = json.load(open(ev / "eval_held.json"))
    assert sorted(q) == ["mean_time", "reg_eval"] and sorted(q["reg_eval"]) == ["fitness", "inlier_rmse"]
    assert np.isfinite([q["mean_time"], q["reg_eval"]["fitness"], q["reg_eval"]["inlier_rmse"]]).all() and 0.0 <= q["reg_eval"]["fitness"] <= 1.0
    assert not (ev / "eval.json").exists() and not (ev / "eval_180.json").exists()
    assert (ev / "reg_fitness.npy").exists() and np.load(ev / "pred_translations.npy").shape == (6, 3)
