"""Inputs of the loss-kernel tests (tests/test_loss_cpu.py, tests/test_loss_gpu.py): head outputs and labels for alignnet_debug_loss, deterministic
from a seed, every value float32.  No reference lives here (tests/loss_ref.py)."""
import numpy as np

F = np.float32
TWOPI = F(2.0 * np.pi)
LABEL_KEYS = ("translations", "rel_angles", "pc1_centers", "pc2_centers", "pc1_angles", "pc2_angles")

# (B, num_bins, accept_inverted, early_stage_factor, angle_factor): between them every B of 1, 2, 3, 63, 64, 65, 129, 1025 (once), every bin count of
# 1, 2, 12, 16, 17, 50, 64, 65, 130, both settings of accept_inverted and the three factor pairs.  B = 65 / nb = 12 and B = 129 / nb = 12 also serve the
# launch-shape test (the first is copied into the second).
VALUE_CASES = (
    (1, 12, True, 0.5, 1.0), (1, 1, False, 0.1, 1.5), (2, 2, True, 0.5, 1.0), (2, 17, False, 0.25, 0.0), (2, 64, True, 0.5, 1.0),
    (3, 12, True, 0.1, 1.5), (3, 16, False, 0.5, 1.0), (3, 130, True, 0.5, 1.0), (3, 65, False, 0.1, 1.5),
    (63, 12, True, 0.5, 1.0), (63, 17, False, 0.1, 1.5), (64, 16, True, 0.1, 1.5), (64, 50, False, 0.5, 1.0), (64, 2, True, 0.25, 0.0),
    (65, 12, True, 0.5, 1.0), (65, 64, False, 0.1, 1.5), (65, 65, True, 0.25, 0.0),
    (129, 12, True, 0.5, 1.0), (129, 50, True, 0.1, 1.5), (129, 130, False, 0.5, 1.0), (129, 1, True, 0.5, 1.0),
    (1025, 12, True, 0.5, 1.0),
)
BIN_COUNTS = (1, 2, 12, 16, 17, 50, 64, 65, 130)
# seeds chosen (tests/test_loss_cpu.py asserts it) so that no label class of a value case is undecided between the float32 and the float64 oracle
SEEDS = {(1025, 12, True, 0.5, 1.0): 221}   # default: the case's position in VALUE_CASES
SWEEP_CHUNK = 128
OUT_OF_RANGE_17 = F(6.098385334014893)   # nb = 17: sh = 6.283185005187988, float32 sh / apc = 17.0


def case_id(c):
    return "B%d-nb%d-%s-esf%g-af%g" % (c[0], c[1], "inv" if c[2] else "noinv", c[3], c[4])


def _grid(g, shape, span):
    """multiples of 1/8 in [-span, span]: sums and differences of a few of them are exact in float32"""
    return (g.randint(-8 * span, 8 * span + 1, size=shape) / 8.0).astype(F)


def _knees(g, err, k0):
    """the first entries of err become the Huber knees 0, +-1, +-2 (and 2.125, just past the stage-3 knee), starting at knee k0"""
    knees = (0.0, 1.0, -1.0, 2.0, -2.0, 2.125)
    flat = err.reshape(-1)
    for t in range(min(flat.size, len(knees))):
        flat[t] = knees[(k0 + t) % len(knees)]
    return err


def make_case(B, nb, seed, inverted=True):
    """dict: o2 [2B, 3 + 2 nb], s1c [2B, 3], o3 [B, 3 + 2 nb], labels {six tensors}.
    inverted with an odd nb: label + pi of the label -1e-9 is a bin boundary itself (pi + apc / 2 = (nb + 1) / 2 bins), undecided between float32 and float64
    by construction; such a case takes -1e-3 in its place (the sweep covers boundaries, for classes)."""
    g = np.random.RandomState(1000 + seed)
    ld = 3 + 2 * nb
    # ---- angles: uniform in [-7, 7]; a few at +-100; 0, -0.0 and -1e-9 (float32 floor-mod: 2 pi itself); a1 == a2
    a1, a2 = g.uniform(-7, 7, B).astype(F), g.uniform(-7, 7, B).astype(F)
    same = F(g.uniform(-7, 7))
    tiny = F(-1e-3) if (inverted and nb % 2) else F(-1e-9)
    special = ((F(100.0), F(-100.0)), (F(0.0), F(-0.0)), (tiny, a2[0]), (same, same), (F(-100.0), F(3.0)), (F(-0.0), tiny))
    for t in range(min(B, len(special)) if B > 3 else 1):
        a1[t], a2[t] = special[(seed + t) % len(special)]
    # ---- centres and translations on the 1/8 grid, errors with the Huber knees among them
    c1, c2, tr = _grid(g, (B, 3), 4), _grid(g, (B, 3), 4), _grid(g, (B, 3), 4)
    cc = np.concatenate([c1, c2])
    e1 = _knees(g, _grid(g, (2 * B, 3), 3), seed)
    e2 = _knees(g, _grid(g, (2 * B, 3), 3), seed + 2)
    e3 = _knees(g, _grid(g, (B, 3), 4), seed + 3)
    s1c = (cc + e1).astype(F)
    s2c = (cc + e2).astype(F)
    o2 = np.zeros((2 * B, ld), F)
    o2[:, :3] = s2c - s1c
    o3 = np.zeros((B, ld), F)
    o3[:, :3] = e3 + tr - (s2c[B:] - s2c[:B])
    # ---- class logits, with exact arg-max ties (the first maximum must win): across the two 64-lane trips when nb > 64
    o2[:, 3:3 + nb] = g.normal(0, 2, (2 * B, nb)).astype(F)
    o3[:, 3:3 + nb] = g.normal(0, 2, (B, nb)).astype(F)
    if nb > 1:
        ties = (((seed + 1) % (2 * B), nb // 3, nb - 1), ((seed + B) % (2 * B), 1 if nb > 65 else 0, 65 if nb > 65 else nb - 1))
        for row, k1, k2 in ties:
            if k1 != k2:
                o2[row, 3 + k1] = o2[row, 3 + k2] = o2[row, 3:3 + nb].max() + F(0.5)
    # ---- residual logits; every third cloud's decoded residual is (0.9 .. 1.9) pi either way, so that theta wraps at +-pi and dth spans (-2 pi, 2 pi)
    o2[:, 3 + nb:] = g.normal(0, 0.7, (2 * B, nb)).astype(F)
    o3[:, 3 + nb:] = g.normal(0, 0.7, (B, nb)).astype(F)
    win = np.argmax(o2[:, 3:3 + nb], axis=1)
    for row in range(seed % 3, 2 * B, 3):
        o2[row, 3 + nb + win[row]] = F(g.choice([-1.0, 1.0]) * g.uniform(0.9, 1.9) * nb)
    labels = dict(translations=tr, rel_angles=(a2 - a1).reshape(B, 1), pc1_centers=c1, pc2_centers=c2, pc1_angles=a1.reshape(B, 1), pc2_angles=a2.reshape(B, 1))
    return dict(B=B, nb=nb, o2=o2, s1c=s1c, o3=o3, labels={k: np.ascontiguousarray(v, F) for k, v in labels.items()})


def value_case(c):
    d = make_case(c[0], c[1], SEEDS.get(c, VALUE_CASES.index(c)), c[2])
    d.update(accept_inverted=c[2], esf=float(F(c[3])), af=float(F(c[4])), id=case_id(c))
    return d


def sweep_labels(nb):
    """every bin boundary k apc - apc / 2, k = 0 .. nb (the last one is the wrap), and up to 3 float32 steps either side; nb = 17 also holds the
    recorded out-of-range label.  Sorted, float32."""
    apc = TWOPI / F(nb)
    out = []
    for k in range(nb + 1):
        x = F(k) * apc - apc / F(2.0)
        lo = hi = x
        out.append(x)
        for _ in range(3):
            lo, hi = np.nextafter(lo, F(-np.inf)), np.nextafter(hi, F(np.inf))
            out += [lo, hi]
    if nb == 17:
        out.append(OUT_OF_RANGE_17)
    return np.unique(np.array(out, F))


def sweep_cases(nb):
    """The sweep as problems of at most SWEEP_CHUNK pairs: tower 1's labels walk up the sweep, tower 2's walk down it, so the pair term sees their differences;
    all logits zero (theta = 0: the pair target is a2 - a1 itself).  For classes only."""
    lab = sweep_labels(nb)
    out = []
    for s in range(0, len(lab), SWEEP_CHUNK):
        a1 = lab[s:s + SWEEP_CHUNK]
        a2 = lab[::-1][s:s + SWEEP_CHUNK]
        B, ld = len(a1), 3 + 2 * nb
        z = np.zeros((B, 3), F)
        labels = dict(translations=z, rel_angles=(a2 - a1).reshape(B, 1), pc1_centers=z, pc2_centers=z, pc1_angles=a1.reshape(B, 1), pc2_angles=a2.reshape(B, 1))
        out.append(dict(B=B, nb=nb, o2=np.zeros((2 * B, ld), F), s1c=np.zeros((2 * B, 3), F), o3=np.zeros((B, ld), F),
                        labels={k: np.ascontiguousarray(v, F) for k, v in labels.items()}, accept_inverted=True, esf=0.5, af=1.0, id="sweep-nb%d-%d" % (nb, s)))
    return out
