"""Planted yaw class logits (tests/test_yaw_class_cpu.py, tests/test_yaw_class_gpu.py).

The arg-max over the stage-2 class logits (models/tp8.py:296) is the one discontinuous choice of the forward pass.  The cases here put chosen class and
residual logits in front of it through the last layer of the stage-2 head: zero weights into the columns 3 onwards, the planted values as biases
(0 * x + b = b exactly, in the engine and in the oracle).  Every cloud of both towers then sees the same logits, exact ties included."""
import numpy as np

from oracle import alignnet_ref as R
from tests.helpers import small_cfg, oracle_params

N, B, SEED = 64, 3, 7
TOP = np.float32(1.25)


def _classes(nb, top):
    v = np.linspace(-1.0, 0.5, nb).astype(np.float32)
    v[list(top)] = TOP
    return v


def residuals(nb):
    """One value per class in [-1, 1), neighbouring classes at least 14 / nb apart (7 is coprime to every nb used): a residual read at another index turns
    stage 3's frame by at least 14 pi / nb^2 rad."""
    return (2.0 * ((7 * np.arange(nb)) % nb) / nb - 1.0).astype(np.float32)


def _wrap_residuals(r6):
    r = residuals(12)
    r[6] = r6
    return r


# name: (nb, class logits, residual logits, the class that must be taken, the other class of the tie or None)
CASES = {
    "nb12_lone_0": (12, _classes(12, [0]), residuals(12), 0, None),
    "nb12_lone_11": (12, _classes(12, [11]), residuals(12), 11, None),
    "nb12_tie_4_9": (12, _classes(12, [4, 9]), residuals(12), 4, 9),
    "nb12_tie_0_11": (12, _classes(12, [0, 11]), residuals(12), 0, 11),
    "nb12_all_equal": (12, np.full(12, 0.75, np.float32), residuals(12), 0, 11),
    "nb17_tie_8_16": (17, _classes(17, [8, 16]), residuals(17), 8, 16),          # 37 output columns: the head's last column tile is partial
    "nb72_tie_5_69": (72, _classes(72, [5, 69]), residuals(72), 5, 69),          # both in lane 5 of the arg-max loop
    "nb72_tie_3_64": (72, _classes(72, [3, 64]), residuals(72), 3, 64),          # lanes 3 and 0: only the cross-lane tie-break sees it
    "nb72_lone_70": (72, _classes(72, [70]), residuals(72), 70, None),           # only the loop's second trip sees it
    # class 6 of 12 sits at pi: with residual 0, ang + pi lands on 2 pi32 within an ulp; with +-7.5 the decoded angle is pi +- 0.625 pi
    "nb12_wrap_0": (12, _classes(12, [6]), _wrap_residuals(0.0), 6, None),
    "nb12_wrap_plus": (12, _classes(12, [6]), _wrap_residuals(7.5), 6, None),
    "nb12_wrap_minus": (12, _classes(12, [6]), _wrap_residuals(-7.5), 6, None),
}
TIES = sorted(k for k, c in CASES.items() if c[4] is not None)


def last_fc(spec):
    return "siamese/transformer2/mlp/fc%d" % (len(spec.s2_fc) + 1)


def plant(P32, spec, cls_logits, res_logits):
    nb = spec.num_bins
    P = dict(P32)
    W, b = P[last_fc(spec) + "/weights"].copy(), P[last_fc(spec) + "/biases"].copy()
    assert W.shape[1] == 3 + 2 * nb and len(cls_logits) == nb and len(res_logits) == nb
    W[:, 3:] = 0.0
    b[3:3 + nb], b[3 + nb:] = cls_logits, res_logits
    P[last_fc(spec) + "/weights"], P[last_fc(spec) + "/biases"] = W, b
    return P


def other_wins(case):
    """The class logits of a tie case with the OTHER tied class as the lone winner (what a kernel that took the last maximum, or broke the cross-lane tie
    the other way, would have turned by)."""
    nb, cl, res, want, other = CASES[case]
    cl = cl.copy()
    cl[other] = np.float32(1.5)
    return cl


def setup(case, backbone="pointnet", cls_logits=None, **widths):
    """(cfg, spec, planted fp32 parameters, clouds) of a case."""
    nb, cl, res, want, other = CASES[case]
    cfg = small_cfg(N=N, nb=nb, backbone=backbone, **widths)
    cfg["training"]["batch_size"] = B
    spec, P32 = oracle_params(cfg)
    P = plant(P32, spec, cl if cls_logits is None else cls_logits, res)
    return cfg, spec, P, R.synth_pairs(B, N, seed=SEED, dtype=np.float32)


def oracle(spec, P, d, yaw_cls=None):
    return R.get_model({k: v.astype(np.float64) for k, v in P.items()}, spec, d["pcs1"].astype(np.float64), d["pcs2"].astype(np.float64), yaw_cls=yaw_cls)
