"""GPU: the drop-in with evaluation.register = "device" (one Engine.register_rows call per evaluation batch) against the host loop it replaces,
on a tiny dataset on disk: 40 val pairs at batch 16, so the last batch is partial.  Both runs draw from the device sampler (ALIGNNET_DEVICE_DATASET)
under the same np.random seed, so they see the same batches.  And register_pair.py against Engine.register."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import alignnet3d
from tests.test_dropin_gpu import _make_dataset, PKG, ROOT

pytestmark = pytest.mark.gpu
FILES = ("pred_translations", "pred_angles", "pred_s1_pc1centers", "pred_s1_pc2centers", "pred_s2_pc1centers", "pred_s2_pc2centers",
         "pred_s2_pc1angles", "pred_s2_pc2angles")
SEEDED = "import sys, numpy as np; np.random.seed(4242); sys.path.insert(0, %r); import train; train.main(sys.argv[1:])" % PKG


def _train_py(args, cwd, **env):
    e = dict(os.environ, PYTHONPATH=PKG + os.pathsep + ROOT, ALIGNNET_DEVICE_DATASET="1", **env)
    r = subprocess.run([sys.executable, "-c", SEEDED] + args, cwd=cwd, env=e, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return r.stdout + r.stderr


def _read(d):
    out = {f: open(os.path.join(d, f + ".npy"), "rb").read() for f in FILES}
    for j in ("eval.json", "eval_180.json"):
        out[j] = json.load(open(os.path.join(d, j)))
    return out


def _mean_loss(log):
    lines = [ln for ln in log.splitlines() if "val mean loss:" in ln]
    assert lines, log[-2000:]
    return lines[-1].split("val mean loss:")[1].strip()


@pytest.fixture(scope="module")
def run(gpu_required, tmp_path_factory):
    tmp = tmp_path_factory.mktemp("register_dropin")
    root = tmp / "SynthTiny"
    _make_dataset(str(root), n=56)
    open(root / "split" / "val.txt", "w").write("\n".join(map(str, range(16, 56))) + "\n")
    user = {"data": {"basepath": str(root)}, "logging": {"basedir": str(tmp / "logs")},
            "model": {"num_points": 64, "angles": {"num_bins": 12, "accept_inverted_angle": True},
                      "options": {"s1transformer": [[32, 64, 96], [[64, 32], 0.7]], "s2transformer": [[32, 64, 128], [[64, 32], 0.7]],
                                  "embedding": [32, 64, 160], "remaining_transform_prediction": [[64, 32], 0.7]}},
            "training": {"batch_size": 16, "num_epochs": 1, "learning_rate": 0.002}}
    cfgp = tmp / "TinyRun.json"
    json.dump(user, open(cfgp, "w"))
    _train_py(["train", "--config", str(cfgp)], str(tmp))
    user["evaluation"] = {"register": "device"}
    cfgd = tmp / "TinyRunDevice.json"
    json.dump(user, open(cfgd, "w"))
    logdir = tmp / "logs" / "TinyRun"
    os.symlink(str(logdir), str(tmp / "logs" / "TinyRunDevice"))   # the second config evaluates the same checkpoint
    return dict(tmp=tmp, cfg=cfgp, cfg_device=cfgd, logdir=logdir, root=root, user=user)


def test_eval_only_device_equals_host(run):
    ev = run["logdir"] / "val" / "eval000000"
    host_log = _train_py(["eval_only", "--config", str(run["cfg"]), "--eval_epoch", "0"], str(run["tmp"]))
    host = _read(ev)
    dev_log = _train_py(["eval_only", "--config", str(run["cfg_device"]), "--eval_epoch", "0"], str(run["tmp"]))
    dev = _read(ev)
    assert "one register call per batch" in dev_log and "one register call per batch" not in host_log
    for f in FILES:
        assert host[f] == dev[f], f + ".npy differs"
    for j in ("eval.json", "eval_180.json"):
        a, b = dict(host[j]), dict(dev[j])
        a.pop("mean_time", None); b.pop("mean_time", None)
        assert a == b and a["num"] == 40, j
    assert _mean_loss(host_log) == _mean_loss(dev_log) and float(_mean_loss(host_log)) > 0.0


def test_eval_only_refine_device_agrees_with_host(run):
    ev = run["logdir"] / "val" / "eval000000" / "refined_p2p_7"
    args = ["eval_only", "--config", str(run["cfg"]), "--eval_epoch", "0", "--refineICP", "--its", "7"]
    host_log = _train_py(args, str(run["tmp"]), ALIGNNET_REGISTER="host")
    host = {f: np.load(ev / (f + ".npy")) for f in FILES}
    dev_log = _train_py(args, str(run["tmp"]), ALIGNNET_REGISTER="device")   # the environment wins over the config's default
    dev = {f: np.load(ev / (f + ".npy")) for f in FILES}
    assert "one register call per batch" in dev_log and "one register call per batch" not in host_log
    np.testing.assert_allclose(dev["pred_translations"], host["pred_translations"], rtol=0, atol=1e-6)
    d = np.abs(dev["pred_angles"] - host["pred_angles"])
    assert np.minimum(d, 2 * np.pi - d).max() <= 1e-6
    assert not dev["pred_s2_pc1centers"].any() and dev["pred_s2_pc1centers"].shape == (40, 3)
    assert _mean_loss(host_log) == _mean_loss(dev_log)
    # --use_old_results with --refineICP takes the inits from files: the host loop, with a log line
    old_log = _train_py(args + ["--use_old_results"], str(run["tmp"]), ALIGNNET_REGISTER="device")
    assert "falling back to host" in old_log and "one register call per batch" not in old_log


def test_register_pair_prints_what_engine_register_returns(run):
    src = np.load(run["root"] / "pointcloud1" / "00000020.npy")
    dst = np.load(run["root"] / "pointcloud2" / "00000020.npy")
    ckpt = str(run["logdir"] / "model-0.aln3")
    eng = alignnet3d.Engine(json.load(open(run["logdir"] / "config.json")))   # the merged config as train.py saved it
    eng.load(ckpt)
    for extra, kw in ((["--refine", "p2p", "--its", "9", "--seed", "3"], dict(refine="point", its=9, seed=3)), ([], dict())):
        want = eng.register([src[:, :3]], [dst[:, :3]], **kw)
        e = dict(os.environ, PYTHONPATH=PKG + os.pathsep + ROOT)
        r = subprocess.run([sys.executable, os.path.join(PKG, "register_pair.py"), "--config", str(run["cfg"]), "--model", ckpt,
                            "--source", str(run["root"] / "pointcloud1" / "00000020.npy"), "--target", str(run["root"] / "pointcloud2" / "00000020.npy")] + extra,
                           cwd=str(run["tmp"]), env=e, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
        lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
        T = np.array([[float(v) for v in ln.split()] for ln in lines[-5:-1]])
        np.testing.assert_array_equal(T, want["transforms"][0])
        if extra:
            assert lines[-1] == "fitness %r rmse %r" % (float(want["fitness"][0]), float(want["rmse"][0]))
        else:
            assert lines[-1] == "fitness n/a rmse n/a"
    eng.close()
