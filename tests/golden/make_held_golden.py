#!/usr/bin/env python3
"""Generate tests/golden/held_vectors.json from the REFERENCE's evaluation.evaluate_held (evaluation.py:49-78).  Run only in the build container,
where /root/reference exists; the committed file is data only: the synthetic inputs made here, the dicts the reference returned and the text of
every track file it wrote.

evaluate_held builds `np.array([(vec3, dt), ...])` per track, which the NumPy of the reference's era made an object array of shape (n, 2) and
NumPy 2 refuses: for this run the reference module's `np` is make_golden.py's proxy, as for process_velocities there."""
import json
import os
import sys
import tempfile
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import REF, _LegacyRaggedNumpy, stub_modules   # noqa: E402

WINDOWS = (1, 5)


def make_inputs(rng):
    """(metas, val_idxs, predicted translations float32 [n, 3]).  Three tracks of 1, 4 and 14 frames (with avg_window 5 both window ends clip on the
    short ones and positions 4 .. 8 of the long one see a full window), examples interleaved and the long track's frames out of order (first-seen
    order is the file's order), one (trackid, frame2) given twice, timestamp gaps below 0.05 s (one of them negative)."""
    rows = [(7, 3, 0.1)]                                                          # (trackid, frame2, t2 - t1)
    rows += [(20003, f, 0.1) for f in (11, 12, 13, 14)]
    rows += [(12, f, 0.1 + 0.001 * f) for f in (5, 4, 6, 7, 9, 8, 10, 11, 12, 13, 14, 15, 17, 16)]
    order = rng.permutation(len(rows))
    rows = [rows[i] for i in order]
    rows.append((20003, 12, 0.2))                                                 # the same (trackid, frame2) again: replaces the value, keeps the place
    rows[3] = (rows[3][0], rows[3][1], 0.01)                                      # below the 0.05 floor
    rows[9] = (rows[9][0], rows[9][1], -0.3)                                      # a tracker's clock going backwards: floored too
    metas = []
    for i, (tid, f2, dt) in enumerate(rows):
        t1 = round(100.0 + 0.1 * f2, 6)
        metas.append({"class": "Car", "frames": [f2 - 1, f2], "timestamps": [t1, round(t1 + dt, 6)], "trackid": tid})
    val = [100 + 3 * i for i in range(len(rows))]                                 # file ids are not positions
    pred = (rng.normal(size=(len(rows), 3)) * [1.5, 0.4, 0.05]).astype(np.float32)
    return metas, val, pred


def main():
    assert os.path.isdir(REF), "the reference tree is needed to make this fixture"
    stub_modules()
    sys.path.insert(0, os.path.join(REF, "tp_utils"))
    sys.path.insert(0, REF)
    import evaluation
    assert os.path.abspath(evaluation.__file__) == os.path.join(REF, "evaluation.py"), evaluation.__file__
    evaluation.np = _LegacyRaggedNumpy(np)
    rng = np.random.default_rng(20261020)
    metas, val, pred = make_inputs(rng)
    out = {"metas": metas, "val_idxs": val, "pred_translations": [[float(x) for x in row] for row in pred], "runs": []}
    with tempfile.TemporaryDirectory() as tmp:
        os.makedirs(os.path.join(tmp, "meta"))
        for vi, m in zip(val, metas):
            json.dump(m, open(os.path.join(tmp, "meta", "%08d.json" % vi), "w"))
        cfg = types.SimpleNamespace(data=types.SimpleNamespace(basepath=tmp))
        zeros3, zeros1 = np.zeros((len(val), 3), np.float32), np.zeros((len(val), 1), np.float32)
        for window in WINDOWS + (None,):
            ed = None
            kw = {}
            if window is not None:
                ed = os.path.join(tmp, "eval_w%d" % window)
                os.makedirs(ed)
                kw = {"avg_window": window}
            vel, info = evaluation.evaluate_held(cfg, val, pred, zeros1, zeros3, zeros1, eval_dir=ed, mean_time=0.125, **kw)
            files = {f: open(os.path.join(ed, f)).read() for f in sorted(os.listdir(ed))} if ed else {}
            out["runs"].append({"avg_window": window, "with_eval_dir": ed is not None, "velocities": {str(k): [float(x) for x in v] for k, v in vel.items()},
                                "track_order": [int(k) for k in vel], "result": info, "files": files})
    json.dump(out, open(os.path.join(HERE, "held_vectors.json"), "w"), indent=1, sort_keys=True)
    print("held fixtures:", len(val), "examples,", sum(len(r["files"]) for r in out["runs"]), "track files")


if __name__ == "__main__":
    main()
