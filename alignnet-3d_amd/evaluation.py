"""Metrics of the drop-in (counterpart of the reference's evaluation.py:16-46,128-289), vectorised: the
reference re-opens one JSON per sample per call; here the per-sample work is array arithmetic and the meta files
are read once.  eval.json / eval_180.json keep the reference schema."""
import copy
import datetime
import json
import os
from argparse import Namespace
from shutil import copyfile

import numpy as np

_T_THRESH = np.array([0.02, 0.1, 0.2])
_A_THRESH = np.array([1.0, 5.0, 10.0])


def ns_to_dict(ns):
    return {k: ns_to_dict(v) if type(v) == Namespace else v for k, v in ns.__dict__.items()}


def eval_translation(t, gt_t):
    dist = np.linalg.norm(np.asarray(t)[:2] - np.asarray(gt_t)[:2])
    return dist, (dist < _T_THRESH).astype(int)


def angle_diff(a, b):
    return float(((b - a) + np.pi) % (np.pi * 2.0) - np.pi)


def eval_angle(a, gt_a, accept_inverted_angle):
    dist = np.abs(angle_diff(a, gt_a)) / np.pi * 180.0
    if accept_inverted_angle:
        dist = np.minimum(dist, np.abs(angle_diff(a + np.pi, gt_a)) / np.pi * 180.0)
    return dist, (dist < _A_THRESH).astype(int)


def eval_transform(t, gt_t, a, gt_a, accept_inverted_angle):
    return np.minimum(eval_translation(t, gt_t)[1], eval_angle(a, gt_a, accept_inverted_angle)[1])


def rot_z(angle):
    c, s = np.cos(angle), np.sin(angle)
    return np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])


def get_mat_angle(translation=None, rotation=None, rotation_center=(0.0, 0.0, 0.0)):
    """4x4: rotate about z by `rotation` around `rotation_center`, then translate (tp_utils/pointcloud.py:279-289);
    the initial guess handed to the ICP refinement (train.py:465-467)."""
    c = np.asarray(rotation_center, np.float64).reshape(3)
    m1, m2, m3 = np.eye(4), np.eye(4), np.eye(4)
    m1[:3, 3] = -c
    m3[:3, 3] = c
    if translation is not None:
        m3[:3, 3] += np.asarray(translation, np.float64).reshape(3)
    if rotation is not None:
        m2[:3, :3] = rot_z(float(np.ravel(rotation)[0]))
    return m3 @ m2 @ m1


def rotvec_z(R):
    """z component of the rotation vector of each rotation matrix in R [..., 3, 3]: what the ICP baseline stores as the predicted
    angle (icp.py:197-199, Rotation.from_dcm(R).as_rotvec()[2]) -- not atan2(R10, R00), which agrees only for a rotation about z.
    Same steps as SciPy's: the quaternion by the largest of (trace, R00, R11, R22) (well conditioned at every angle), w >= 0, then
    angle = 2 atan2(|v|, w) and v scaled by angle / sin(angle / 2), by its Taylor series below angle 1e-3."""
    R = np.asarray(R, np.float64)
    shape = R.shape[:-2]
    m = R.reshape(-1, 3, 3)
    q = np.empty((m.shape[0], 4))   # x, y, z, w
    d = np.stack([m[:, 0, 0], m[:, 1, 1], m[:, 2, 2], m[:, 0, 0] + m[:, 1, 1] + m[:, 2, 2]], 1)
    choice = d.argmax(1)
    w = choice == 3
    q[w, 0] = m[w, 2, 1] - m[w, 1, 2]
    q[w, 1] = m[w, 0, 2] - m[w, 2, 0]
    q[w, 2] = m[w, 1, 0] - m[w, 0, 1]
    q[w, 3] = 1.0 + d[w, 3]
    for i in range(3):
        j, k = (i + 1) % 3, (i + 2) % 3
        s = choice == i
        q[s, i] = 1.0 - d[s, 3] + 2.0 * m[s, i, i]
        q[s, j] = m[s, j, i] + m[s, i, j]
        q[s, k] = m[s, k, i] + m[s, i, k]
        q[s, 3] = m[s, k, j] - m[s, j, k]
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    q[q[:, 3] < 0] *= -1.0
    angle = 2.0 * np.arctan2(np.linalg.norm(q[:, :3], axis=1), q[:, 3])
    small = np.abs(angle) <= 1e-3
    scale = np.empty_like(angle)
    a2 = angle[small] ** 2
    scale[small] = 2.0 + a2 / 12.0 + 7.0 * a2 * a2 / 2880.0
    scale[~small] = angle[~small] / np.sin(angle[~small] / 2.0)
    return (scale * q[:, 2]).reshape(shape)


def translate_transform_to_new_center_of_rotation(pred_translations, pred_angles, pred_centers, gt_pc1centers):
    """Same map as tp_utils/pointcloud.py:309-318: t' = -d + Rz(angle) d + t with d = new_centre - old_centre."""
    out = np.zeros_like(pred_translations)
    for i, (t, a, c, g) in enumerate(zip(pred_translations, pred_angles, pred_centers, gt_pc1centers)):
        d = g - c
        out[i] = -d + rot_z(float(np.ravel(a)[0])) @ d + t
    return out


def process_velocities(tracks, eval_dir, avg_window):
    """Smoothed speed per track (evaluation.py:82-110): every run of consecutive frames of a (sequence, tracklet) becomes one track
    that starts at rest one frame earlier; the speed at a frame is the norm (xy) of the mean velocity over the frames within
    +- avg_window.  Writes <eval_dir>/velocities/track<id:09>.txt, one value per line, as the reference does; returns {id: [speeds]}."""
    if eval_dir is None:
        return None
    vdir = eval_dir + "/velocities"
    os.makedirs(vdir, exist_ok=True)
    velocities = {}
    for inter_id, traj in tracks.items():
        frames = sorted(traj)
        for start in [f for f in frames if f - 1 not in traj]:
            tid = inter_id + start - 1      # the track begins with the pose before its first prediction
            vel = [np.zeros(3)]             # (0, 0, 0) over 0.1 s
            f = start
            while f in traj:
                t, dt = traj[f]
                vel.append(np.asarray(t, np.float64) / dt)
                f += 1
            vel = np.asarray(vel)
            speeds = [float(np.linalg.norm(vel[max(0, i - avg_window):i + avg_window + 1].mean(axis=0)[:2])) for i in range(len(vel))]
            velocities[tid] = speeds
            with open("%s/track%09d.txt" % (vdir, tid), "w") as fh:
                for v in speeds:
                    fh.write("%s\n" % v)
    return velocities


def evaluate_held(cfg, val_idxs, all_pred_translations, all_pred_angles, all_gt_translations, all_gt_angles, eval_dir=None, avg_window=5, mean_time=0):
    """Held data -- a tracker's output, no ground truth (evaluation.py:49-78, called at train.py:506-508): a smoothed speed per track from the meta
    keys trackid, frames, timestamps.  Restated with the reference's quirks: the time between the frames is max(0.05, t2 - t1); tracks and frames
    keep the first-seen order of val_idxs, a later example of the same (trackid, frame2) replaces the earlier one's value in its place; the speed at
    position i is the xy norm of the mean velocity over positions [max(0, i - avg_window + 1), i + avg_window + 1) -- not process_velocities' window;
    the files are <eval_dir>/track<trackid>.txt (eval_dir itself, the id unpadded), one value per line; and the speeds are computed only while
    writing, so eval_dir=None returns an empty dict.  The angles and the ground truth are not read.  Returns (velocities, dict(mean_time))."""
    tracks = {}
    for idx, file_idx in enumerate(val_idxs):
        with open("%s/meta/%s.json" % (cfg.data.basepath, str(file_idx).zfill(8))) as fh:
            meta = json.load(fh)
        timestamp1, timestamp2 = meta["timestamps"]
        time_passed = np.maximum(0.05, timestamp2 - timestamp1)
        tracks.setdefault(meta["trackid"], {})[meta["frames"][1]] = all_pred_translations[idx] / time_passed
    velocities = {}
    if eval_dir is None:
        return velocities, dict(mean_time=mean_time)
    for trackid, track in tracks.items():
        vel = list(track.values())
        speeds = velocities.setdefault(trackid, [])
        with open("%s/track%s.txt" % (eval_dir, trackid), "w") as fh:
            for i in range(len(vel)):
                window = vel[max(0, i - avg_window + 1):i + avg_window + 1]
                total = window[0]
                for v in window[1:]:        # left to right, as the reference's mean over an object array adds them
                    total = total + v
                speed = np.linalg.norm((total / len(window))[:2])
                speeds.append(speed)
                fh.write("%s\n" % speed)
    return velocities, dict(mean_time=mean_time)


def reg_eval_summary(reg_eval, eval_dir=None):
    """Namespace(fitness, inlier_rmse): the plain means of the per-pair arrays (fitness_per_pair, rmse_per_pair); with eval_dir the arrays are
    written there as reg_fitness.npy / reg_inlier_rmse.npy.  No pair gives 0 / 0."""
    fit, rmse = (np.asarray(a, np.float64).ravel() for a in reg_eval)
    assert fit.shape == rmse.shape, "one fitness and one inlier rmse per pair"
    if eval_dir is not None:
        os.makedirs(eval_dir, exist_ok=True)
        np.save("%s/reg_fitness.npy" % eval_dir, fit)
        np.save("%s/reg_inlier_rmse.npy" % eval_dir, rmse)
    return Namespace(fitness=float(fit.mean()) if fit.size else 0.0, inlier_rmse=float(rmse.mean()) if rmse.size else 0.0)


def _bucket():
    z = lambda: np.zeros(3, dtype=float)
    return dict(corr_levels_translation=z(), corr_levels_angles=z(), corr_levels=z(), mean_dist_translation=0.0,
                mean_sq_dist_translation=0.0, mean_dist_angle=0.0, mean_sq_dist_angle=0.0, num=0)


_DIST_KEYS = (("all", np.inf), ("5m", 5.0), ("10m", 10.0), ("15m", 15.0), ("20m", 20.0))


def _summarise(node):
    def one(k):
        b = node[k]
        return Namespace(corr_levels=b["corr_levels"].tolist(), corr_levels_translation=b["corr_levels_translation"].tolist(),
                         mean_dist_translation=b["mean_dist_translation"], mean_sq_dist_translation=b["mean_sq_dist_translation"],
                         corr_levels_angles=b["corr_levels_angles"].tolist(), mean_dist_angle=b["mean_dist_angle"],
                         mean_sq_dist_angle=b["mean_sq_dist_angle"], num=b["num"])
    top = one("all")
    for k in ("5m", "10m", "15m", "20m"):
        setattr(top, "eval_" + k, one(k))
    return top


def evaluate(cfg, val_idxs, all_pred_translations, all_pred_angles, all_gt_translations, all_gt_angles, all_pred_centers,
             all_gt_pc1centers, eval_dir=None, accept_inverted_angle=False, detailed_eval=False, avg_window=5, mean_time=0, reg_eval=None):
    """reg_eval (this project's, not a reference argument): None leaves result.reg_eval at the zeros the reference writes (evaluation.py:213, 271);
    (fitness_per_pair, rmse_per_pair) -- Engine.evaluate_registration_rows at every pair's final transform -- fills it with their plain means, a
    pair without inliers counting as 0 in both as Open3D reports it, and writes the arrays to reg_fitness.npy / reg_inlier_rmse.npy in eval_dir."""
    new_t = translate_transform_to_new_center_of_rotation(all_pred_translations, all_pred_angles, all_pred_centers, all_gt_pc1centers)
    measures = {k: _bucket() for k, _ in _DIST_KEYS}
    measures["val"] = {k: _bucket() for k, _ in _DIST_KEYS}
    measures["test"] = {k: _bucket() for k, _ in _DIST_KEYS}
    base = cfg.data.basepath
    per_transform = []
    tracks = {}
    have_meta = os.path.isdir("%s/meta" % base)
    for i, vi in enumerate(val_idxs):
        # test/val membership as in evaluation.py:157-161.  The reference leaves `is_test` unbound for base paths
        # that contain neither marker (quirk A6(viii)); here such samples count as validation samples.
        is_test = False
        meta = None
        if have_meta:      # one read per sample serves the split (:157) and the velocity tracks (:215); the reference reads it twice
            try:
                with open("%s/meta/%s.json" % (base, str(vi).zfill(8))) as fh:
                    meta = json.load(fh)
            except OSError:
                meta = None
        if "KITTI_tracklets" in base:
            is_test = meta is not None and "trackids" in meta and meta["trackids"][0] in [2, 6, 7, 8, 10]
        elif "Synth" in base:
            is_test = i >= 1000
        if meta is not None and "seq" in meta:   # evaluation.py:215-224: the UN-recentred prediction, 0.1 s between frames
            inter = meta["seq"] * 10000000 + meta["trackids"][0] * 10000
            tracks.setdefault(inter, {})[meta["frames"][1]] = (np.asarray(all_pred_translations[i], np.float64), 0.1)
        a, ga = float(np.ravel(all_pred_angles[i])[0]), float(np.ravel(all_gt_angles[i])[0])
        dt, lt = eval_translation(new_t[i], all_gt_translations[i])
        da, la = eval_angle(a, ga, accept_inverted_angle)
        dt, da = float(dt), float(da)
        lv = np.minimum(lt, la)
        if dt <= 10000:
            cd = np.linalg.norm(all_gt_pc1centers[i])
            for node in (measures, measures["test" if is_test else "val"]):
                for key, lim in _DIST_KEYS:
                    if cd > lim:
                        continue
                    b = node[key]
                    b["num"] += 1
                    b["corr_levels_translation"] += lt
                    b["mean_dist_translation"] += dt
                    b["mean_sq_dist_translation"] += dt * dt
                    b["corr_levels_angles"] += la
                    b["mean_dist_angle"] += da
                    b["mean_sq_dist_angle"] += da * da
                    b["corr_levels"] += lv
        if detailed_eval:
            per_transform.append([lv, dt, da])
    for node in (measures, measures["val"], measures["test"]):
        for key, _ in _DIST_KEYS:
            b = node[key]
            n = float(b["num"]) if b["num"] else 1e-20   # "make numbers really large, indicates eval is not valid"
            for k in ("corr_levels_translation", "corr_levels_angles", "corr_levels"):
                b[k] = b[k] / n
            b["mean_dist_translation"] /= n
            b["mean_dist_angle"] /= n
            b["mean_sq_dist_translation"] = float(np.sqrt(b["mean_sq_dist_translation"] / n))
            b["mean_sq_dist_angle"] = float(np.sqrt(b["mean_sq_dist_angle"] / n))
    if tracks:
        process_velocities(tracks, eval_dir, avg_window)
    result = _summarise(measures)
    result.val = _summarise(measures["val"])
    result.test = _summarise(measures["test"])
    result.reg_eval = Namespace(fitness=0.0, inlier_rmse=0.0) if reg_eval is None else reg_eval_summary(reg_eval, eval_dir)
    result.mean_time = mean_time
    if eval_dir is not None:
        os.makedirs(eval_dir, exist_ok=True)
        filename = "%s/eval%s.json" % (eval_dir, "_180" if accept_inverted_angle else "")
        if os.path.isfile(filename):
            copyfile(filename, "%s_%s.json" % (filename[:-5], datetime.datetime.today().strftime("%Y-%m-%d_%H-%M-%S")))
            if mean_time == 0:
                prev = json.load(open(filename))
                if "mean_time" in prev:
                    result.mean_time = prev["mean_time"]
        with open(filename, "w") as fh:
            json.dump(ns_to_dict(result), fh)
    return (result, per_transform) if detailed_eval else result
