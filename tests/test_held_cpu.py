"""CPU: held evaluation.  evaluation.evaluate_held against the reference's own run (tests/golden/held_vectors.json, made by
tests/golden/make_held_golden.py), the held dataset's pairs and meta (alignnet3d/tracklets.py), and evaluate's reg_eval keyword."""
import json
import os
import sys
import types

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
PKG = os.path.join(os.path.dirname(HERE), "alignnet-3d_amd")
if PKG not in sys.path:
    sys.path.insert(0, PKG)

import evaluation   # noqa: E402
from alignnet3d import tracklets as T   # noqa: E402

HJ = json.load(open(os.path.join(HERE, "golden", "held_vectors.json")))


@pytest.fixture()
def held_root(tmp_path):
    os.makedirs(tmp_path / "meta")
    for vi, m in zip(HJ["val_idxs"], HJ["metas"]):
        json.dump(m, open(tmp_path / "meta" / ("%08d.json" % vi), "w"))
    return types.SimpleNamespace(data=types.SimpleNamespace(basepath=str(tmp_path)))


def test_golden_covers_what_it_should():
    lens = sorted(len(v) for v in HJ["runs"][0]["velocities"].values())
    assert lens == [1, 4, 14]
    keys = [(m["trackid"], m["frames"][1]) for m in HJ["metas"]]
    assert len(keys) - len(set(keys)) == 1                                              # one (trackid, frame2) occurs twice
    gaps = [m["timestamps"][1] - m["timestamps"][0] for m in HJ["metas"]]
    assert min(gaps) < 0 and sum(g < 0.05 for g in gaps) >= 2
    assert [r["avg_window"] for r in HJ["runs"]] == [1, 5, None] and not HJ["runs"][2]["with_eval_dir"]


@pytest.mark.parametrize("run", range(len(HJ["runs"])))
def test_evaluate_held_reproduces_the_reference(held_root, tmp_path, run):
    """Every returned value bit for bit, the order of the tracks, and every track file character for character."""
    want = HJ["runs"][run]
    pred = np.array(HJ["pred_translations"], np.float32)
    n = len(pred)
    ed = None
    if want["with_eval_dir"]:
        ed = str(tmp_path / "out")
        os.makedirs(ed)
    kw = {} if want["avg_window"] is None else {"avg_window": want["avg_window"]}
    reads = []
    real_load = evaluation.json.load
    try:
        evaluation.json = types.SimpleNamespace(load=lambda fh: (reads.append(fh.name), real_load(fh))[1], dump=evaluation.json.dump)
        vel, info = evaluation.evaluate_held(held_root, HJ["val_idxs"], pred, np.zeros((n, 1), np.float32), np.zeros((n, 3), np.float32),
                                             np.zeros((n, 1), np.float32), eval_dir=ed, mean_time=0.125, **kw)
    finally:
        evaluation.json = json
    assert len(reads) == n and len(set(reads)) == n                                     # the meta file is read once per sample
    assert info == want["result"] == {"mean_time": 0.125}
    assert [int(k) for k in vel] == want["track_order"]
    assert {str(k): [float(x) for x in v] for k, v in vel.items()} == want["velocities"]
    got = {f: open(os.path.join(ed, f)).read() for f in sorted(os.listdir(ed))} if ed else {}
    assert got == want["files"]
    if ed is None:
        assert vel == {}


def _labels(rows):
    """A label file's text: (frame, track, class) rows with fixed boxes."""
    return "".join("%d %d %s 0 0 -1.5 100 120 200 220 1.5 1.6 3.9 %.2f 1.6 %.2f -1.57 0.99\n" % (f, t, c, 2.0 + t, 10.0 + f) for f, t, c in rows)


def test_held_pairs_and_meta(tmp_path):
    # track 3: frames 0 1 2 . 4 5 (a hole at 3); track 11: frames 1 2; a pedestrian and a DontCare row besides; an 18th column as trackers add it
    rows = [(0, 3, "Car"), (1, 3, "Car"), (2, 3, "Car"), (4, 3, "Car"), (5, 3, "Car"), (1, 11, "Car"), (2, 11, "Car"), (1, 5, "Pedestrian"),
            (2, 5, "Pedestrian"), (0, -1, "DontCare")]
    path = tmp_path / "0004.txt"
    path.write_text(_labels(rows))
    labels = T.read_labels(str(path))
    stamps_path = tmp_path / "stamps.txt"
    stamps_path.write_text("".join("%.3f\n" % (50.0 + 0.11 * f) for f in range(6)))
    stamps = T.read_timestamps(str(stamps_path))
    assert stamps.dtype == np.float64 and len(stamps) == 6
    held = T.held_pairs(labels, ("Car",), stamps, seq=4)
    plain = T.pairs(labels, ("Car",), seq=4)
    key = lambda p: (p.seq, p.frames, p.track, p.cls, p.rows, p.box1.tolist(), p.box2.tolist())
    assert [key(p) for p in held] == [key(p) for p in plain]                                               # the pairs of pairs(...)
    assert [(p.track, p.frames) for p in held] == [(3, (0, 1)), (3, (1, 2)), (11, (1, 2)), (3, (4, 5))]    # no pair across the hole 2 -> 4
    assert all(p.timestamps == (float(stamps[p.frames[0]]), float(stamps[p.frames[1]])) for p in held)       # from the file
    by_rate = T.held_pairs(labels, ("Car",), T.rate_timestamps(10.0), seq=4, gap=2)
    assert [(p.track, p.frames, p.timestamps) for p in by_rate] == [(3, (0, 2), (0.0, 0.2)), (3, (2, 4), (0.2, 0.4))]   # or from the frame rate
    with pytest.raises(ValueError):
        T.held_pairs(labels, ("Car",), stamps[:3], seq=4)
    with pytest.raises(ValueError):
        T.rate_timestamps(0.0)
    m = T.held_meta(held[2])
    assert list(m) == ["start_position", "start_angle", "end_position", "end_angle", "translation", "rel_angle", "class", "frames", "timestamps", "trackid"]
    assert m["trackid"] == 4 * 10000 + 11 and m["frames"] == [1, 2] and m["class"] == "Car"
    assert m["timestamps"] == [float(stamps[1]), float(stamps[2])]
    plain_meta = T.meta(plain[2])
    for k in ("start_position", "end_position", "translation"):
        got = np.loadtxt(m[k].splitlines())
        assert got.shape == np.loadtxt(plain_meta[k].splitlines()).shape == (3,) and not got.any()
    assert m["start_angle"] == m["end_angle"] == m["rel_angle"] == 0.0
    json.dumps(m)
    # the crop arguments of a held pair: zero labels and NO z_difference taken from the second crop
    index = {f: f for f in range(6)}
    frames, boxes, dz, lab = T.extract_args(held, index, held=True)
    frames0, boxes0, dz0, lab0 = T.extract_args(plain, index)
    assert np.array_equal(frames, frames0) and np.array_equal(boxes, boxes0)
    assert not dz.any() and not lab.any() and lab.shape == (4, 12) and lab0.any()


def test_make_kitti_dataset_parser_held_options():
    import make_kitti_dataset as M
    a = M.parse_args(["--kitti", "/k", "--out", "/o"])
    assert (a.held, a.timestamps_dir, a.frame_rate) == (False, None, 10.0)
    a = M.parse_args(["--kitti", "/k", "--out", "/o", "--held", "--timestamps-dir", "/t", "--frame-rate", "12.5"])
    assert (a.held, a.timestamps_dir, a.frame_rate) == (True, "/t", 12.5)
    for bad in ("0", "-1", "nan"):
        with pytest.raises(SystemExit):
            M.parse_args(["--kitti", "/k", "--out", "/o", "--held", "--frame-rate", bad])


def test_evaluate_reg_eval_keyword(tmp_path):
    """reg_eval=None: the bytes of eval.json are those of a call without the keyword and no array file appears; given: only reg_eval moves."""
    ev = np.load(os.path.join(HERE, "golden", "eval_vectors.npz"))
    ej = json.load(open(os.path.join(HERE, "golden", "eval_vectors.json")))
    root = tmp_path / ej["kitti_dirname"]
    os.makedirs(root / "meta")
    for i, m in enumerate(ej["kitti_meta"]):
        json.dump(m, open(root / "meta" / ("%08d.json" % i), "w"))
    cfg = types.SimpleNamespace(data=types.SimpleNamespace(basepath=str(root)))
    args = ([int(v) for v in ev["kitti_val"]], ev["kitti_pred_t"], ev["kitti_pred_a"], ev["kitti_gt_t"], ev["kitti_gt_a"], ev["kitti_pred_c"], ev["kitti_gt_c"])
    out = {}
    n = len(args[0])
    rng = np.random.default_rng(1)
    fit, rmse = rng.uniform(0, 1, n), rng.uniform(0, 0.02, n)
    fit[3] = rmse[3] = 0.0   # a pair without inliers counts as 0 in both
    for name, kw in (("plain", {}), ("none", {"reg_eval": None}), ("given", {"reg_eval": (fit, rmse)})):
        ed = tmp_path / name
        evaluation.evaluate(cfg, *args, eval_dir=str(ed), mean_time=0.25, **kw)
        out[name] = open(ed / "eval.json", "rb").read()
        assert os.path.isfile(ed / "reg_fitness.npy") == os.path.isfile(ed / "reg_inlier_rmse.npy") == (name == "given")
    assert out["plain"] == out["none"]
    a, b = json.loads(out["none"]), json.loads(out["given"])
    assert a["reg_eval"] == {"fitness": 0.0, "inlier_rmse": 0.0}
    assert b["reg_eval"] == {"fitness": float(fit.mean()), "inlier_rmse": float(rmse.mean())}
    a.pop("reg_eval"); b.pop("reg_eval")
    assert a == b
    assert np.array_equal(np.load(tmp_path / "given" / "reg_fitness.npy"), fit) and np.array_equal(np.load(tmp_path / "given" / "reg_inlier_rmse.npy"), rmse)
