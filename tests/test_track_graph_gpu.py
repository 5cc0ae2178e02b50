"""GPU: track_graph.py end to end on a tiny KITTI-shaped tree (tests/tracklet_cases.write_kitti_tree: the crops are random points, so this is a
plumbing test, not an accuracy test).  The edges of track*.json are what direct register_rows / evaluate_registration_rows calls give for the same
pairs, the optimised poses what pose_graph_optimize gives for those edges, the speed files follow from poses and timestamps; the module's main and
the command line (a fresh child process) write the same files."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import alignnet3d
from alignnet3d import tracklets as T, tracks
from tests import tracklet_cases as K

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "alignnet-3d_amd")
MAX_SKIP, THRESHOLD, FRAMES = 3, 0.5, 6


@pytest.fixture(scope="module")
def setup(gpu_required, tmp_path_factory):
    tmp = tmp_path_factory.mktemp("track_graph")
    kitti = tmp / "tracker_out"
    K.write_kitti_tree(str(kitti), seed=5, n_seq=2, n_frames=FRAMES, max_points=1200)
    os.makedirs(tmp / "trainset" / "split")              # the model's config names its training set: only the split files are read
    for name in ("train", "val"):
        open(tmp / "trainset" / "split" / (name + ".txt"), "w").close()
    user = {"data": {"basepath": str(tmp / "trainset")}, "logging": {"basedir": str(tmp / "logs")},
            "model": {"num_points": 64, "angles": {"num_bins": 12, "accept_inverted_angle": True},
                      "options": {"s1transformer": [[32, 64, 96], [[64, 32], 0.7]], "s2transformer": [[32, 64, 128], [[64, 32], 0.7]],
                                  "embedding": [32, 64, 160], "remaining_transform_prediction": [[64, 32], 0.7]}},
            "training": {"batch_size": 4}}
    cfgp = tmp / "Tracks.json"
    json.dump(user, open(cfgp, "w"))
    sys.path.insert(0, PKG)
    import config as cfgmod
    cfgmod.reset_config()
    try:
        eng = alignnet3d.Engine(cfgmod.load_config(str(cfgp)))
        # a checkpoint whose network answers "no motion" (all weights zero: every output is its bias): the ICP refinement then starts from the
        # identity, and crops that moved by a few decimetres leave inliers for the information matrices
        for name, shape, _ in eng.variables():
            if name.endswith("weights"):
                eng.set_variable(name, np.zeros(shape, np.float32))
        eng.save(str(tmp / "model-0.aln3"))
        eng.close()
    finally:
        cfgmod.reset_config()
    args = ["--config", str(cfgp), "--model", str(tmp / "model-0.aln3"), "--kitti", str(kitti), "--max-skip", str(MAX_SKIP), "--classes", "Car,Pedestrian",
            "--refine", "p2p", "--threshold", str(THRESHOLD), "--frame-rate", "10"]
    import track_graph
    try:
        graphs, results = track_graph.main(args + ["--out", str(tmp / "out_main")])
    finally:
        cfgmod.reset_config()
    return dict(tmp=tmp, kitti=kitti, cfgp=cfgp, args=args, graphs=graphs, results=results)


def _tracks(out_dir):
    return {n[:-5]: json.load(open(os.path.join(out_dir, n))) for n in sorted(os.listdir(out_dir)) if n.endswith(".json")}


def test_files_and_graph_shapes(setup):
    out = _tracks(setup["tmp"] / "out_main")
    # per sequence: the Car over all frames (one graph), the Pedestrian missing in frame 1 (a hole: frame 0 alone has no pair inside its stretch, so
    # the stretch is frames 2..5), the second Car with labels dropped in places
    assert len(out) == len(setup["graphs"]) >= 4
    print("statuses:", [(r["status"], r["solves"]) for r in setup["results"]], "translations up to %.3g" % max(np.abs(g["T"][:, :3, 3]).max() for g in setup["graphs"]))
    assert any(r["solves"] > 0 for r in setup["results"])        # (the optimiser had something to do)
    for g in setup["graphs"]:
        assert np.all(np.diff(g["frames"]) == 1) and np.array_equal(g["poses"][0], np.eye(4))
        gaps = g["frames"][g["j"]] - g["frames"][g["i"]]
        assert np.all((gaps >= 1) & (gaps <= MAX_SKIP)) and np.array_equal(g["uncertain"], gaps > 1)
    full = out["track0"]
    assert full["frames"] == list(range(FRAMES)) and len(full["edges"]) == sum(FRAMES - s for s in range(1, MAX_SKIP + 1))
    assert full["timestamps"] == [f / 10.0 for f in range(FRAMES)]
    ped = [t for name, t in out.items() if t["seq"] == 0 and t["track"] == 1]
    assert [t["frames"] for t in ped] == [list(range(2, FRAMES))]
    for name, t in out.items():
        n = len(t["frames"])
        assert np.asarray(t["poses"]).shape == (n, 4, 4) and np.asarray(t["chained_poses"]).shape == (n, 4, 4)
        assert t["pruned"] == [e["frames"] for e in t["edges"] if e["pruned"]] and all(e["uncertain"] for e in t["edges"] if e["pruned"])
        speeds = [float(x) for x in open(setup["tmp"] / "out_main" / (name + ".txt")).read().split()]
        assert len(speeds) == n - 1 and np.isfinite(speeds).all()
        assert np.array_equal(speeds, tracks.speeds(np.asarray(t["poses"]), t["timestamps"], t["anchor"]))
        assert t["objective"][1] <= t["objective"][0] and t["status"] in alignnet3d.Engine.POSE_GRAPH_STATUS


def test_edges_equal_direct_calls_and_poses_equal_the_optimiser(setup):
    """Sequence 0 again by hand: the same pairs, crops, register_rows and evaluate_registration_rows calls, build_graphs, pose_graph_optimize."""
    sys.path.insert(0, PKG)
    import config as cfgmod
    cfgmod.reset_config()
    try:
        eng = alignnet3d.Engine(cfgmod.load_config(str(setup["cfgp"])))
    finally:
        cfgmod.reset_config()
    eng.load(str(setup["tmp"] / "model-0.aln3"))
    labels = T.read_labels(os.path.join(setup["kitti"], "training", "label_02", "0000.txt"))
    pairs = [p for s in range(1, MAX_SKIP + 1) for p in T.held_pairs(labels, ["Car", "Pedestrian"], T.rate_timestamps(10.0), 0, gap=s)]
    scans = {f: T.read_scan(str(setup["kitti"]), 0, f) for f in range(FRAMES)}
    off = T.extract(eng, scans, pairs, install=True, held=True)
    _, p2 = eng.tracklet_read(off)
    centres = np.stack([p2[off[b, 1]:off[b + 1, 1]].astype(np.float64).mean(0) if off[b + 1, 1] > off[b, 1] else np.zeros(3) for b in range(len(pairs))])
    rows = np.arange(len(pairs), dtype=np.int32)
    reg = eng.register_rows(rows, 0, refine="point", its=30)
    ev = eng.evaluate_registration_rows(rows, reg["transforms"], threshold=THRESHOLD, centers=centres, want_information=True)
    mine = tracks.build_graphs(pairs, reg["transforms"], ev["information"], centres, MAX_SKIP)
    res = eng.pose_graph_optimize(mine, threshold=THRESHOLD)
    eng.close()
    theirs = [(g, r) for g, r in zip(setup["graphs"], setup["results"]) if g["seq"] == 0]
    assert len(theirs) == len(mine)
    out = _tracks(setup["tmp"] / "out_main")
    for (g, r), h, s in zip(theirs, mine, res):
        for k in ("frames", "i", "j", "T", "info", "c", "uncertain", "poses"):
            assert np.array_equal(g[k], h[k]), k
        for k in ("poses", "chi2", "weights", "pruned"):
            assert np.array_equal(r[k], s[k]), k
        name = "track%d" % g["track"] + ("" if g["first"] else "_%d" % g["frames"][0])
        t = out[name]
        assert np.array_equal(np.asarray(t["poses"]), s["poses"]) and np.array_equal(np.asarray(t["chained_poses"]), h["poses"])
        assert np.array_equal(np.asarray([e["transform"] for e in t["edges"]]).reshape(-1, 4, 4), h["T"])
        assert np.array_equal(np.asarray([e["information"] for e in t["edges"]]).reshape(-1, 6, 6), h["info"])
        assert [e["weight"] for e in t["edges"]] == s["weights"].tolist()


def test_command_line_writes_the_same_files(setup):
    out = setup["tmp"] / "out_cli"
    env = dict(os.environ, PYTHONPATH=PKG + os.pathsep + ROOT)
    r = subprocess.run([sys.executable, os.path.join(PKG, "track_graph.py")] + setup["args"] + ["--out", str(out)], cwd=str(setup["tmp"]), env=env,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "Track graphs: %d graphs" % len(setup["graphs"]) in r.stdout
    a, b = setup["tmp"] / "out_main", out
    assert sorted(os.listdir(a)) == sorted(os.listdir(b))
    for n in os.listdir(a):
        assert open(a / n).read() == open(b / n).read(), n
