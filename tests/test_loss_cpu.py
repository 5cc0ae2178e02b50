"""CPU: the references, cases and bars of the loss-kernel tests (tests/loss_ref.py, tests/loss_cases.py) checked on their own -- the value cases are
decided, the oracle's gradient is a gradient, the out-of-range rule of angle2class holds and leaves the shipped bin counts alone -- and the eight wrong
kernels, restated, that the GPU test's checks (loss_ref.judge / judge_classes, the same functions) must refuse."""
import os
import re

import numpy as np

from alignnet3d import _capi
from oracle import alignnet_ref as R
from tests import loss_cases as LC
from tests import loss_ref as LR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32


def test_case_list_covers_every_shape_the_kernels_branch_on():
    cs = LC.VALUE_CASES
    assert 20 <= len(cs) <= 25 and len(set(cs)) == len(cs)
    assert {c[0] for c in cs} == {1, 2, 3, 63, 64, 65, 129, 1025} and sum(c[0] > 130 for c in cs) == 1
    assert {c[1] for c in cs} == set(LC.BIN_COUNTS) == {1, 2, 12, 16, 17, 50, 64, 65, 130}
    assert {c[2] for c in cs} == {True, False} and {c[3:] for c in cs} == {(0.5, 1.0), (0.1, 1.5), (0.25, 0.0)}
    a = np.concatenate([LC.value_case(c)["labels"][k].ravel() for c in cs for k in ("pc1_angles", "pc2_angles")])
    assert a.dtype == F and (np.abs(a) == 100).sum() >= 10 and (a == F(-1e-9)).sum() >= 5 and (a == 0).sum() >= 10 and np.signbit(a[a == 0]).any()
    assert R.floor_mod(F(-1e-9), LC.TWOPI) == LC.TWOPI   # the float32 floor-mod of -1e-9 is 2 pi itself
    ties = wraps = same = 0
    for c in cs:
        d = LC.value_case(c)
        lg = d["o2"][:, 3:3 + d["nb"]]
        ties += int(((lg == lg.max(axis=1, keepdims=True)).sum(axis=1) > 1).sum())
        win = np.argmax(lg, axis=1)
        raw = win * (2 * np.pi / d["nb"]) + d["o2"][np.arange(len(win)), 3 + d["nb"] + win] * (np.pi / d["nb"])
        wraps += int(((raw + np.pi < 0) | (raw + np.pi >= 2 * np.pi)).sum())
        same += int((d["labels"]["pc1_angles"] == d["labels"]["pc2_angles"]).sum())
        for k in ("o2", "s1c", "o3"):
            assert d[k].dtype == F
        assert d is not LC.value_case(c) and all(np.array_equal(d[k], LC.value_case(c)[k]) for k in ("o2", "s1c", "o3"))   # deterministic
    assert ties >= 30 and wraps >= 300 and same >= 10


def test_huber_knees_are_hit_exactly():
    """errors of exactly 0, +-1 and +-2 among the centres and translations (multiples of 1/8: the float32 subtraction is exact)"""
    seen1, seen3 = set(), set()
    for c in LC.VALUE_CASES:
        d = LC.value_case(c)
        ep, s2c = LR.endpoints(d, F)
        B, lab = d["B"], d["labels"]
        cc = np.concatenate([lab["pc1_centers"], lab["pc2_centers"]])
        seen1 |= set(np.unique(np.concatenate([(d["s1c"] - cc).ravel(), (s2c - cc).ravel()])).tolist())
        seen3 |= set(np.unique(ep["pred_translations"] - lab["translations"]).tolist())
        assert np.all(np.round(ep["pred_translations"] * 8) == ep["pred_translations"] * 8)
    assert {0.0, 1.0, -1.0} <= seen1 and {0.0, 2.0, -2.0, 2.125} <= seen3


def test_value_cases_are_decided():
    """no label class differs between the float32 and the float64 oracle, and the tf.cond margin |tot0 - tot1| exceeds 1e-4 max(1, tot) for every term"""
    for c in LC.VALUE_CASES:
        assert LR.undecided(c) == 0, LC.case_id(c)
        r = LR.reference(c)
        for t, tot in enumerate(r["v64"]["tot"]):
            if len(tot) == 2:
                assert abs(tot[0] - tot[1]) > 1e-4 * max(1.0, max(tot)), (LC.case_id(c), t, tot)
        assert LR.choice_of(r["v64"]["tot"]) == LR.choice_of(r["v32"]["tot"])
    chosen = [LR.choice_of(LR.reference(c)["v64"]["tot"])[t] for c in LC.VALUE_CASES if c[2] for t in range(3)]
    assert 0 in chosen and 1 in chosen


def test_bars_come_from_the_oracle_and_stay_below_the_ceiling():
    u_v, u_g = LR.bars()
    print("u_v %.3g" % u_v, " ".join("%s %.3g" % kv for kv in u_g.items()))
    assert 1e-7 < u_v < LR.CEILING / 4
    for k in LR.GRAD_KEYS:
        assert 2e-8 < u_g[k] < LR.CEILING
    # the numbers the documents quote (tests/test_loss_gpu.py)
    assert abs(u_v / 1.47e-5 - 1) < 0.05 and abs(u_g["d_o2"] / 3.9e-5 - 1) < 0.05 and abs(u_g["d_s1c"] / 7.4e-8 - 1) < 0.05


def test_sweep_undecided_entries_sit_on_a_boundary():
    """On the boundary sweep the float32 and float64 oracle may disagree -- only within 4 float32 steps of a boundary."""
    for nb in LC.BIN_COUNTS:
        apc = float(LC.TWOPI) / nb
        for case in LC.sweep_cases(nb):
            v32, v64 = LR.oracle_values(case, F), LR.oracle_values(case, np.float64)
            a1, a2 = case["labels"]["pc1_angles"][:, 0].astype(np.float64), case["labels"]["pc2_angles"][:, 0].astype(np.float64)
            targets = (a1, a2, (a2 - a1)[:, None] + np.zeros((1, case["B"])))
            for t in range(3):
                for v in range(2):
                    m = v32["cls"][t][v] != v64["cls"][t][v]
                    x = (targets[t][m] + v * float(F(np.pi))) % float(LC.TWOPI)
                    q = (x + apc / 2) / apc
                    dist = np.abs(q - np.round(q)) * apc   # distance to the nearest boundary, radians
                    assert np.all(dist <= 4 * float(np.spacing(F(2 * np.pi)))), (nb, t, v, dist.max())


def test_oracle_gradient_is_the_gradient():
    """float64 autograd against central differences in float64, two small cases (smooth where they stand: labels decided, no error on a knee moves)"""
    for c in ((2, 17, False, 0.25, 0.0), (3, 12, True, 0.1, 1.5)):
        case = LR.reference(c)["case"]
        g = LR.reference(c)["g64"]
        _, s2c = LR.endpoints(case, F)
        base = dict(s1c=case["s1c"].astype(np.float64), s2c=s2c.astype(np.float64), o2=case["o2"].astype(np.float64), o3=case["o3"].astype(np.float64))

        def f(x):
            B = case["B"]
            ep = {"pred_s1_pc1centers": x["s1c"][:B], "pred_s1_pc2centers": x["s1c"][B:], "pred_s2_pc1centers": x["s2c"][:B], "pred_s2_pc2centers": x["s2c"][B:],
                  "pred_pc1angle_logits": x["o2"][:B, 3:], "pred_pc2angle_logits": x["o2"][B:, 3:],
                  "pred_translations": x["o3"][:, :3] + (x["s2c"][B:] - x["s2c"][:B]), "pred_remaining_angle_logits": x["o3"][:, 3:]}
            return float(R.get_loss(LR.spec_of(case), ep, *[np.asarray(case["labels"][k], np.float64) for k in LC.LABEL_KEYS])[0])
        h, rng = 1e-6, np.random.RandomState(5)
        for key, gk in (("s1c", "d_s1c"), ("s2c", "d_s2c"), ("o2", "d_o2"), ("o3", "d_o3")):
            idx = [np.unravel_index(i, base[key].shape) for i in rng.choice(base[key].size, min(base[key].size, 24), replace=False)]
            for i in idx:
                if key == "o2" and i[1] < 3:
                    continue   # o2[:, :3] enters through s2c, a leaf of its own here
                xp, xm = {k: v.copy() for k, v in base.items()}, {k: v.copy() for k, v in base.items()}
                xp[key][i] += h
                xm[key][i] -= h
                num = (f(xp) - f(xm)) / (2 * h)
                # (an error standing exactly on a Huber knee has a one-sided second derivative: the central difference is off by h / 2 times the jump
                #  times the term's weight, below 1e-7 here)
                assert abs(num - g[gk][i]) <= 1e-6 * max(1.0, np.abs(g[gk]).max()), (c, key, i, num, g[gk][i])


def test_out_of_range_rule():
    """(class + 0.5) apc + residual == sh modulo 2 pi and 0 <= class < nb for every swept label and every bin count; the recorded nb = 17 label and the
    sweeps of nb = 17, 19 do hit the float32 quotient nb; the kernels' float32 restatement agrees with the oracle there."""
    hits = {}
    for nb in LC.BIN_COUNTS + (19,):
        lab = LC.sweep_labels(nb)
        k, res = R.angle2class(lab.reshape(-1, 1), nb)
        res = res[:, 0]
        kk, kres, sh = LR.kernel_class_rule(lab, nb, "wrap")
        raw = LR.kernel_class_rule(lab, nb, "raw")[0]
        hits[nb] = int((raw == nb).sum())
        assert k.dtype == np.int32 and k.min() >= 0 and k.max() < nb
        assert np.array_equal(k, kk) and np.array_equal(k, np.where(raw == nb, 0, raw)) and np.array_equal(res, kres)
        apc = LC.TWOPI / F(nb)
        back = (k.astype(np.float64) + 0.5) * float(apc) + res.astype(np.float64)
        d = np.abs((back - sh.astype(np.float64) + np.pi) % float(LC.TWOPI) - np.pi)
        assert d.max() <= 4 * float(np.spacing(LC.TWOPI)), (nb, d.max())
        if hits[nb]:
            assert np.all(np.abs(res[raw == nb] / F(np.pi / nb) + 1) < 1e-4)   # the label residual of such an entry: -1, against class 0
    assert hits[17] >= 1 and hits[19] >= 1 and all(hits[nb] == 0 for nb in (1, 2, 12, 16, 50, 64, 65, 130)), hits
    k, res = R.angle2class(np.array([[LC.OUT_OF_RANGE_17]], F), 17)
    assert k[0] == 0 and abs(float(res[0, 0]) / float(F(np.pi / 17)) + 1.0000031) < 1e-6
    assert LR.kernel_class_rule(LC.OUT_OF_RANGE_17, 17, "raw")[0] == 17 and LR.kernel_class_rule(LC.OUT_OF_RANGE_17, 17, "raw")[2] == F(6.283185005187988)


def _angle2class_before(angle, nb):
    """oracle/alignnet_ref.py angle2class as it stood before the out-of-range rule"""
    dt = angle.dtype.type
    twopi = dt(np.float32(2.0 * np.pi))
    a = R.floor_mod(angle, twopi)
    apc = twopi / dt(nb)
    sh = R.floor_mod(a + apc / dt(2.0), twopi)
    cls = (sh / apc).astype(np.int32)
    return cls[:, 0], sh - (cls.astype(angle.dtype) * apc + apc / dt(2.0))


def test_shipped_bin_counts_keep_their_bits():
    """nb = 10, 12, 36, 50: the oracle is unchanged, bit for bit, on a dense sweep (200,000 labels in [-7, 7], every boundary +-3 steps, the last 4096
    float32 numbers below 2 pi and below each wrap of the shifted angle), in float32 and float64; no quotient reaches nb."""
    g = np.random.RandomState(3)
    for nb in (10, 12, 36, 50):
        top = LC.TWOPI - (LC.TWOPI / F(nb)) / F(2)
        tail = [top, LC.TWOPI]
        for _ in range(4096):
            tail += [np.nextafter(tail[-2], F(0)), np.nextafter(tail[-1], F(0))]
        lab = np.concatenate([g.uniform(-7, 7, 200000).astype(F), LC.sweep_labels(nb), np.array(tail, F)]).reshape(-1, 1)
        for dt in (F, np.float64):
            x = lab.astype(dt)
            (k0, r0), (k1, r1) = _angle2class_before(x, nb), R.angle2class(x, nb)
            assert k0.max() == nb - 1 and k0.min() == 0
            assert np.array_equal(k0, k1) and r0.tobytes() == r1.tobytes() and k1.dtype == k0.dtype and r1.dtype == r0.dtype
        assert LR.kernel_class_rule(lab[:, 0], nb, "raw")[0].max() == nb - 1


def test_model_passes_and_every_wrong_kernel_is_refused():
    """The loss as the kernels state it (loss_ref.loss_model) passes the GPU test's own checks on every case it is run on; with one mutation each it is
    refused.  Cases: all value cases but B = 1025, and the sweeps of nb = 12, 17 (classes)."""
    cases = [c for c in LC.VALUE_CASES if c[0] <= 130]
    sweeps = [s for nb in (12, 17) for s in LC.sweep_cases(nb)]
    sweep_ref = [LR.oracle_values(s, F)["cls"] for s in sweeps]

    def failures(mutation):
        out = []
        for c in cases:
            out += [(LC.case_id(c), b) for b in LR.judge(LR.loss_model(LR.reference(c)["case"], mutation), c)]
        for s, ref in zip(sweeps, sweep_ref):
            out += [(s["id"], b) for b in LR.judge_classes(LR.model_classes(s, np.zeros(2 * s["B"], F), mutation), ref, s["nb"])]
        return out
    assert failures(None) == []
    for m in LR.MUTATIONS:
        bad = failures(m)
        print(m, len(bad), bad[0] if bad else None)
        assert bad, m
    assert len(LR.MUTATIONS) == 8
    # which check refuses what: the row-slice mutation only where B has a partial slice behind a full one; the clamp only on the sweep's classes
    assert {x[0].split("-")[0] for x in failures("last_row_slice_dropped")} == {"B65", "B129"}
    assert all(x[0].startswith("sweep-nb17") for x in failures("class_nb_clamped"))
    assert all("d_o2" in x[1] for x in failures("towers_lose_s3"))


def test_header_declares_the_hook_and_capi_binds_it():
    text = open(os.path.join(ROOT, "include", "alignnet_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    m = re.search(r"\bint alignnet_debug_loss\s*\(([^)]*)\)", code)
    assert m and len(m.group(1).split(",")) == 22 == len(_capi.SYMBOLS["alignnet_debug_loss"][1])
    assert re.search(r"#define\s+ALIGNNET_ABI_VERSION\s+1\b", text) and _capi.ABI_VERSION == 1
    import alignnet3d
    assert hasattr(alignnet3d.load_library(), "alignnet_debug_loss") and hasattr(alignnet3d.Engine, "debug_loss")
