"""NumPy restatement that DEFINES what the one-call registration (Engine.register / register_rows, csrc/alignnet_register.hip) computes between
the network's outputs and the ICP refinement.  Checked on the CPU against the host code it restates (tests/test_register_cpu.py:
models.tp8.classLogits2angle, evaluation.get_mat_angle) and on the GPU against the kernels (tests/test_register_gpu.py)."""
import numpy as np


def decode(logits, nb):
    """models/tp8.py:55-65 classLogits2angle for logits [B, 2 nb] (float32): the class is the FIRST maximum of logits[:, :nb] (np.argmax), the angle
    float64(class) * (2 pi / nb) + float64(logits[nb + class]) -- a product and a sum, each rounded once -- minus 2 pi when it is > pi.  The
    residual is taken as it is (not de-normalised).  Returns [B] float64."""
    logits = np.asarray(logits)
    assert logits.ndim == 2 and logits.shape[1] == 2 * nb
    k = 2 * np.pi / float(nb)
    cls = np.argmax(logits[:, :nb], axis=1)
    res = logits[np.arange(len(logits)), nb + cls].astype(np.float64)
    angle = cls.astype(np.float64) * k + res
    return np.where(angle > np.pi, angle - 2 * np.pi, angle)


def pred_angle(a1, a2, ar):
    """train.py:456, in that order."""
    return (a2 - a1) + ar


def network_transform(t, angle, c):
    """evaluation.py:46-57 get_mat_angle(t, angle, rotation_center=c) = Tr(c + t) Rz(angle) Tr(-c) in closed form, the sums in the order the two 4x4
    products take them: R (-c) first, then + (c + t).  t, c: [3] (float32 values widened), angle: float64.  Returns [4, 4] float64."""
    t = np.asarray(t).astype(np.float64).reshape(3)
    c = np.asarray(c).astype(np.float64).reshape(3)
    a = np.float64(angle)
    cs, sn = np.cos(a), np.sin(a)
    T = np.eye(4)
    T[0, 0], T[0, 1], T[1, 0], T[1, 1] = cs, -sn, sn, cs
    T[0, 3] = (cs * (-c[0]) + (-sn) * (-c[1])) + (c[0] + t[0])
    T[1, 3] = (sn * (-c[0]) + cs * (-c[1])) + (c[1] + t[1])
    T[2, 3] = (-c[2]) + (c[2] + t[2])
    return T
