"""Engine: the session-like object the drop-in train.py drives.

It plays the role of the TF graph + Session of the reference: construction =
train.py:190-227 (placeholders, get_model, get_loss, optimizer), `forward` = the eval
`sess.run` (train.py:447-449), `train_step` = the train `sess.run` (train.py:368).
All arithmetic happens in libalignnet_hip.so on the GPU; this file only marshals."""
import ctypes as C

import numpy as np

from . import _capi

OUTPUT_NAMES = ("pred_translations", "pred_remaining_angle_logits", "pred_s1_pc1centers", "pred_s1_pc2centers",
                "pred_s2_pc1centers", "pred_s2_pc2centers", "pred_pc1angle_logits", "pred_pc2angle_logits")

SUMMARY_NAMES = (
    "losses/translation", "losses/angle",
    "losses_stages/stage1_pc1_transl_loss", "losses_stages/stage1_pc2_transl_loss",
    "losses_stages/stage2_pc1_transl_loss", "losses_stages/stage2_pc2_transl_loss",
    "losses_stages/stage3_transl_loss",
    "losses_stages/stage2_pc1_angle_loss", "losses_stages/stage2_pc1_angle_class_loss",
    "losses_stages/stage2_pc1_angle_residual_loss",
    "losses_stages/stage2_pc2_angle_loss", "losses_stages/stage2_pc2_angle_class_loss",
    "losses_stages/stage2_pc2_angle_residual_loss",
    "losses_stages/stage3_angle_loss", "losses_stages/stage3_angle_class_loss",
    "losses_stages/stage3_angle_residual_loss")  # models/tp8.py:336-353 order


# include/alignnet_hip.h ALIGNNET_KERNEL_*: which backbone instantiation an eval forward launched (get_option("last_backbone_kernel"))
KERNEL_IDS = {"pointnet_fused": 1, "pointnet_fused<64,128>": 2, "pointnet_fused<64,128,k16>": 3, "pointnet_fused<tp64>": 4,
              "pointnet_split": 5, "pointnet_split<64,128>": 6, "pointnet_split_persist": 7, "pointnet_fused<64,128,k16,tp64>": 8, "dgcnn_fused": 10, "dgcnn_fused<64,128>": 11,
              "dgcnn_split": 12, "dgcnn_split<64,128>": 13}
KERNEL_NAMES = {v: k for k, v in KERNEL_IDS.items()}
ICP_FULL_ROTATION = 1   # include/alignnet_hip.h ALIGNNET_ICP_FULL_ROTATION: flags bit of alignnet_icp_register*
FGR_DECREASE_MU = 2     # include/alignnet_hip.h ALIGNNET_FGR_DECREASE_MU: flags bit of alignnet_fgr_register*


class EngineError(RuntimeError):
    pass


def default_model_config():
    """The SynthCars layer widths (reference configs/SynthCars.json:12-15) at N=1024 -- the
    operating point of BASELINE.json.  Same nesting as the merged reference config."""
    return {
        "data": {"num_channels": 3, "ntrain": 0},
        "model": {
            "backbone": "pointnet", "num_points": 1024,
            "options": {
                "angle_factor": 1.0, "early_stage_factor": 0.5,
                "s1transformer": [[64, 128, 256], [[512, 256], 0.7]],
                "s2transformer": [[64, 128, 512], [[512, 256], 0.7]],
                "embedding": [64, 128, 1024],
                "remaining_transform_prediction": [[512, 256], 0.7],
            },
            "angles": {"num_bins": 50, "accept_inverted_angle": True},
        },
        "training": {
            "batch_size": 128, "learning_rate": 0.005,
            "optimizer": {"optimizer": "adam"},
            "lr_extension": {"mode": "decay", "per": "epoch", "step": 30, "rate": 0.5},
            "bn_extension": {"mode": "decay", "per": "epoch", "step": 30, "rate": 0.5, "init": 0.5, "clip": 0.99},
        },
        "gpu_index": 0,
    }


def _to_dict(cfg):
    """Accept a plain dict or the config NameSpace (config.py:9-29)."""
    if isinstance(cfg, dict):
        return cfg
    out = {}
    for k, v in cfg.__dict__.items():
        out[k] = _to_dict(v) if hasattr(v, "__dict__") and not isinstance(v, (list, tuple, str)) else v
    return out


def make_c_config(cfg, device=None, seed=0):
    d = _to_dict(cfg)
    m, o, t = d["model"], d["model"]["options"], d.get("training", {})
    c = _capi.Config()
    c.abi_version = _capi.ABI_VERSION
    c.device = int(d.get("gpu_index", 0) if device is None else device)
    c.num_points = int(m["num_points"])
    c.num_channels = int(d["data"]["num_channels"])
    c.num_bins = int(m["angles"]["num_bins"])
    bk = m["backbone"]
    if bk not in ("pointnet", "dgcnn"):
        raise AssertionError(bk)  # models/tp8.py:68
    c.backbone = 0 if bk == "pointnet" else 1
    c.s1_conv, c.s1_fc = _capi.Widths.of(o["s1transformer"][0]), _capi.Widths.of(o["s1transformer"][1][0])
    c.s2_conv, c.s2_fc = _capi.Widths.of(o["s2transformer"][0]), _capi.Widths.of(o["s2transformer"][1][0])
    c.emb_conv = _capi.Widths.of(o["embedding"])
    c.rem_fc = _capi.Widths.of(o["remaining_transform_prediction"][0])
    keep = lambda v: -1.0 if v is None else float(v)
    c.s1_keep, c.s2_keep = keep(o["s1transformer"][1][1]), keep(o["s2transformer"][1][1])
    c.rem_keep = keep(o["remaining_transform_prediction"][1])
    c.angle_factor, c.early_stage_factor = float(o["angle_factor"]), float(o["early_stage_factor"])
    c.accept_inverted_angle = int(bool(m["angles"]["accept_inverted_angle"]))
    c.batch_size = int(t.get("batch_size", 1))
    c.ntrain = int(d["data"].get("ntrain", 0))
    c.learning_rate = float(t.get("learning_rate", 0.001))
    lr, bn = t.get("lr_extension", {}), t.get("bn_extension", {})
    c.lr_step, c.lr_rate = int(lr.get("step", 0)), float(lr.get("rate", 1.0))
    c.lr_per_epoch = int(lr.get("per", "epoch") == "epoch")
    c.bn_init, c.bn_rate, c.bn_clip = float(bn.get("init", 0.5)), float(bn.get("rate", 0.5)), float(bn.get("clip", 0.99))
    c.bn_step, c.bn_per_epoch = int(bn.get("step", 0)), int(bn.get("per", "epoch") == "epoch")
    opt = t.get("optimizer", {}).get("optimizer", "adam")
    if opt not in ("adam", "momentum"):
        raise AssertionError("Invalid optimizer")  # train.py:216
    c.optimizer = 0 if opt == "adam" else 1
    c.momentum = float(t.get("optimizer", {}).get("momentum", 0.9))
    # the engine implements loss "separate" with hard angle classes (every shipped config); anything else must not train silently
    loss = t.get("loss", {})
    if isinstance(loss, dict):
        if loss.get("loss", "separate") != "separate":
            raise AssertionError("training.loss.loss=%r: only the 'separate' loss is built (models/tp8.py:401-407; 'p2p' is never "
                                 "enabled by a shipped config, SURVEY 8.A4)" % loss.get("loss"))
        if (loss.get("options", {}) or {}).get("soft_angle_classes", False):
            raise AssertionError("training.loss.options.soft_angle_classes is not built (models/tp8.py:253-274; no shipped config enables it)")
    c.seed = int(seed)
    return c


def _fp(a):
    return a.ctypes.data_as(_capi.FP)


def _dp(a):
    """double* of a float64 array; None (an output the caller does not want) stays None"""
    return None if a is None else a.ctypes.data_as(C.POINTER(C.c_double))


def _ip(a):
    """int32_t* of an int32 array, None as _dp"""
    return None if a is None else a.ctypes.data_as(C.POINTER(C.c_int32))


def _lp(a):
    """int64_t* of an int64 array, None as _dp"""
    return None if a is None else a.ctypes.data_as(C.POINTER(C.c_int64))


def _pack_pairs(sources, targets):
    """Lists of [n, 3] clouds as the host entry points take them: (p1, p2, off) = the two float32 blobs and the [B + 1, 2] int64 table of the
    pairs' row offsets into them."""
    B = len(sources)
    off = np.zeros((B + 1, 2), np.int64)
    off[1:, 0] = np.cumsum([len(s) for s in sources]); off[1:, 1] = np.cumsum([len(t) for t in targets])
    cat = lambda L: np.ascontiguousarray(np.concatenate([np.asarray(x, np.float32).reshape(-1, 3) for x in L], 0)) if L else np.zeros((0, 3), np.float32)
    return cat(sources), cat(targets), off


def _one_pair(source, target, T=None):
    """The one pair of a debug_* hook: (p1, p2, Tm) = the two clouds as contiguous float32 [n, 3] and the 4x4 `T` as 16 float64 (None without T)."""
    p1 = np.ascontiguousarray(np.asarray(source, np.float32).reshape(-1, 3)); p2 = np.ascontiguousarray(np.asarray(target, np.float32).reshape(-1, 3))
    return p1, p2, None if T is None else np.ascontiguousarray(np.asarray(T, np.float64).reshape(16))


def centroid_inits(points1, points2, offsets, rows):
    """icp.py:62-66 get_centroid_init for the examples at `rows` of packed tables (points1 / points2 [n, >=3], offsets
    [n + 1, 2] as uploaded with Engine.upload_dataset): identity rotation, translation = mean(pc2) - mean(pc1), the means
    taken in float64 over the float64 copy of the cloud as Open3D's points hold it.  [B, 4, 4] float64; a pair with an
    empty cloud keeps translation 0 (the reference's mean of nothing is NaN)."""
    rows = np.asarray(rows, np.int64).reshape(-1)
    out = np.tile(np.eye(4), (rows.size, 1, 1))
    for k, i in enumerate(rows):
        (a1, a2), (b1, b2) = offsets[i], offsets[i + 1]
        if b1 > a1 and b2 > a2:
            out[k, :3, 3] = np.array(points2[a2:b2, :3], np.float64).mean(axis=0) - np.array(points1[a1:b1, :3], np.float64).mean(axis=0)
    return out


class Engine:
    def __init__(self, cfg=None, device=None, seed=0):
        self._lib = _capi.load_library()
        self._h = _capi.H()
        self.cfg = _to_dict(cfg) if cfg is not None else default_model_config()
        self._c = make_c_config(self.cfg, device, seed)
        if self._lib.alignnet_create(C.byref(self._c), C.byref(self._h)) != 0:
            raise EngineError(self._lib.alignnet_last_error(None).decode())
        self.num_points = self._c.num_points
        self.num_bins = self._c.num_bins
        self._dataset_sizes = None   # source sizes of the uploaded dataset's rows
        self._inflight = []   # output arrays of submitted, not yet waited-for batches (forward_submit / forward_wait)

    def close(self):
        if getattr(self, "_h", None):
            self._lib.alignnet_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc):
        if rc != 0:
            raise EngineError(self._lib.alignnet_last_error(self._h).decode())

    # ---- variables ---------------------------------------------------------
    def variables(self):
        """[(name, (rows, cols), trainable)] in graph-construction order."""
        out = []
        name, r, c, t = C.c_char_p(), C.c_int32(), C.c_int32(), C.c_int32()
        for i in range(self._lib.alignnet_num_params(self._h)):
            self._check(self._lib.alignnet_param_info(self._h, i, C.byref(name), C.byref(r), C.byref(c), C.byref(t)))
            out.append((name.value.decode(), (r.value, c.value), bool(t.value)))
        return out

    def get_variable(self, name):
        shp = dict((n, s) for n, s, _ in self.variables())[name]
        a = np.empty(shp[0] * shp[1], np.float32)
        self._check(self._lib.alignnet_get_param(self._h, name.encode(), _fp(a), a.size))
        return a.reshape(shp) if shp[0] > 1 else a

    def set_variable(self, name, value):
        a = np.ascontiguousarray(value, np.float32).ravel()
        self._check(self._lib.alignnet_set_param(self._h, name.encode(), _fp(a), a.size))

    def set_variables(self, d):
        for k, v in d.items():
            self.set_variable(k, v)

    def init_variables(self, seed=0):
        self._check(self._lib.alignnet_init_params(self._h, seed))

    # ---- eval sess.run (train.py:447-449) -----------------------------------
    def _alloc_outputs(self, B):
        nb2 = 2 * self.num_bins
        widths = dict(pred_translations=3, pred_remaining_angle_logits=nb2, pred_s1_pc1centers=3, pred_s1_pc2centers=3,
                      pred_s2_pc1centers=3, pred_s2_pc2centers=3, pred_pc1angle_logits=nb2, pred_pc2angle_logits=nb2)
        arrs = {k: np.empty((B, widths[k]), np.float32) for k in OUTPUT_NAMES}
        o = _capi.Outputs()
        for k in OUTPUT_NAMES:
            setattr(o, k, _fp(arrs[k]))
        return arrs, o

    def _check_pcs(self, pcs1, pcs2):
        # the feed is float64 in the reference (provider.py:110-119) and cast to the float32 placeholder
        p1 = np.ascontiguousarray(pcs1, np.float32)
        p2 = np.ascontiguousarray(pcs2, np.float32)
        if p1.ndim != 3 or p1.shape != p2.shape or p1.shape[1] != self.num_points or p1.shape[2] != 3:
            raise ValueError(f"pcs must be [B,{self.num_points},3] and equal-shaped, got {p1.shape} and {p2.shape}")
        return p1, p2

    def forward(self, pcs1, pcs2):
        p1, p2 = self._check_pcs(pcs1, pcs2)
        arrs, o = self._alloc_outputs(p1.shape[0])
        self._check(self._lib.alignnet_forward(self._h, _fp(p1), _fp(p2), p1.shape[0], C.byref(o)))
        return arrs

    # ---- pipelined host path: up to two batches in flight, the copy-in of batch i + 1 under the forward of batch i ----
    def forward_submit(self, pcs1, pcs2):
        """Queue one batch (returns at once); the matching forward_wait() returns its outputs.  At most two submits without a wait."""
        p1, p2 = self._check_pcs(pcs1, pcs2)
        arrs, o = self._alloc_outputs(p1.shape[0])
        self._check(self._lib.alignnet_forward_submit(self._h, _fp(p1), _fp(p2), p1.shape[0], C.byref(o)))
        self._inflight.append(arrs)   # (the C side writes into these arrays at wait(): keep them alive)

    def forward_wait(self):
        if not self._inflight:
            raise EngineError("forward_wait: no batch in flight")
        self._check(self._lib.alignnet_forward_wait(self._h))
        return self._inflight.pop(0)

    def forward_stream(self, batches):
        """Generator over an iterable of (pcs1, pcs2): yields each batch's outputs in order, with two batches in flight."""
        pending = 0
        for pcs1, pcs2 in batches:
            if pending == 2:
                yield self.forward_wait()
                pending -= 1
            self.forward_submit(pcs1, pcs2)
            pending += 1
        while pending:
            yield self.forward_wait()
            pending -= 1

    def forward_device(self, d_pcs1, d_pcs2, B, d_out_ptrs=None):
        """Device pointers (ints); d_out_ptrs: dict name -> device pointer, or None to skip copies out."""
        o = _capi.Outputs()
        for k in OUTPUT_NAMES:
            p = (d_out_ptrs or {}).get(k)
            setattr(o, k, C.cast(C.c_void_p(p), _capi.FP) if p else None)
        self._check(self._lib.alignnet_forward_device(self._h, C.c_void_p(d_pcs1), C.c_void_p(d_pcs2), B, C.byref(o)))

    def synchronize(self):
        self._check(self._lib.alignnet_synchronize(self._h))

    # ---- loss on the last eval forward (train.py:448 `loss` fetch) --------------
    def _labels(self, labels, B):
        keys = ("translations", "rel_angles", "pc1_centers", "pc2_centers", "pc1_angles", "pc2_angles")
        widths = (3, 1, 3, 3, 1, 1)
        arrs, L = [], _capi.Labels()
        for k, w in zip(keys, widths):
            a = np.ascontiguousarray(labels[k], np.float32).reshape(B, w)
            arrs.append(a)
            setattr(L, k, _fp(a))
        return arrs, L

    def eval_loss(self, labels, B):
        keep, L = self._labels(labels, B)
        loss, summ = C.c_float(), (C.c_float * 16)()
        self._check(self._lib.alignnet_eval_loss(self._h, C.byref(L), B, C.byref(loss), summ))
        return loss.value, dict(zip(SUMMARY_NAMES, list(summ)))

    # ---- train sess.run (train.py:368) -------------------------------------------
    def _train_call(self, fn, pcs1, pcs2, labels, dropout_u):
        p1, p2 = self._check_pcs(pcs1, pcs2)
        B = p1.shape[0]
        keep, L = self._labels(labels, B)
        arrs, o = self._alloc_outputs(B)
        res = _capi.StepResult()
        u = None
        if dropout_u is not None:
            u = np.ascontiguousarray(np.concatenate([np.asarray(x, np.float32).ravel() for x in dropout_u]), np.float32)
        self._check(fn(self._h, _fp(p1), _fp(p2), C.byref(L), B, _fp(u) if u is not None else None, C.byref(res), C.byref(o)))
        out = dict(step=res.step, loss=res.loss, learning_rate=res.learning_rate, bn_decay=res.bn_decay,
                   summaries=dict(zip(SUMMARY_NAMES, list(res.summaries))))
        out.update(arrs)
        return out

    def train_forward_backward(self, pcs1, pcs2, labels, dropout_u=None):
        """Forward (batch statistics, EMA update), loss and backward; gradients stay on the device.
        dropout_u: optional list [s1 tower0, s2 tower0, s1 tower1, s2 tower1, pair head] of uniforms."""
        return self._train_call(self._lib.alignnet_train_forward_backward, pcs1, pcs2, labels, dropout_u)

    def train_step(self, pcs1, pcs2, labels, dropout_u=None):
        return self._train_call(self._lib.alignnet_train_step, pcs1, pcs2, labels, dropout_u)

    def train_step_device(self, d_pcs1, d_pcs2, d_labels, B, want_result=False):
        """d_labels: dict name -> device pointer (int)."""
        L = _capi.Labels()
        for k in ("translations", "rel_angles", "pc1_centers", "pc2_centers", "pc1_angles", "pc2_angles"):
            setattr(L, k, C.cast(C.c_void_p(d_labels[k]), _capi.FP))
        res = _capi.StepResult()
        self._check(self._lib.alignnet_train_step_device(self._h, C.c_void_p(d_pcs1), C.c_void_p(d_pcs2), C.byref(L), B,
                                                         C.byref(res) if want_result else None))
        return dict(step=res.step, loss=res.loss) if want_result else None

    # ---- HBM-resident dataset + device sampler (include/alignnet_hip.h; replaces provider.load_batch + jitter) ----
    def upload_dataset(self, points1, points2, offsets, labels):
        """points*: [sum n, 3]; offsets: [n_examples + 1, 2] int64 row offsets; labels: [n_examples, 12]
        (alignnet3d/packed.py layout).  Copied to HBM once."""
        p1 = np.ascontiguousarray(points1, np.float32).reshape(-1, 3)
        p2 = np.ascontiguousarray(points2, np.float32).reshape(-1, 3)
        off = np.ascontiguousarray(offsets, np.int64).reshape(-1, 2)
        lab = np.ascontiguousarray(labels, np.float32).reshape(off.shape[0] - 1, 12)
        assert off[-1, 0] == p1.shape[0] and off[-1, 1] == p2.shape[0], "offsets do not cover the point blobs"
        self._check(self._lib.alignnet_dataset_upload(self._h, _fp(p1), _fp(p2), off.ctypes.data_as(C.POINTER(C.c_int64)),
                                                      _fp(lab), off.shape[0] - 1))
        self._dataset_sizes = np.diff(off[:, 0])   # source sizes per row (evaluate_registration_rows splits its correspondences by them)

    @staticmethod
    def _rows(rows):
        r = np.ascontiguousarray(rows, np.int32).ravel()
        return r, r.ctypes.data_as(C.POINTER(C.c_int32))

    def sample_batch(self, rows, seed, jitter_sigma=0.0, jitter_clip=0.05):
        """Draw the batch on the device; returns (d_pcs1, d_pcs2, {label name: device pointer})."""
        r, rp = self._rows(rows)
        self._check(self._lib.alignnet_dataset_sample(self._h, rp, r.size, int(seed), float(jitter_sigma), float(jitter_clip)))
        p1, p2, L = C.c_void_p(), C.c_void_p(), _capi.Labels()
        self._check(self._lib.alignnet_dataset_batch(self._h, C.byref(p1), C.byref(p2), C.byref(L)))
        names = ("translations", "rel_angles", "pc1_centers", "pc2_centers", "pc1_angles", "pc2_angles")
        return p1.value, p2.value, {k: C.cast(getattr(L, k), C.c_void_p).value for k in names}

    def train_step_rows(self, rows, seed, jitter_sigma=0.01, jitter_clip=0.05):
        """sample (with the reference's jitter defaults, provider.py:60) + full training step, no host batch."""
        r, rp = self._rows(rows)
        res = _capi.StepResult()
        self._check(self._lib.alignnet_train_step_dataset(self._h, rp, r.size, int(seed), float(jitter_sigma), float(jitter_clip),
                                                          C.byref(res)))
        return dict(step=res.step, loss=res.loss, learning_rate=res.learning_rate, bn_decay=res.bn_decay,
                    summaries=dict(zip(SUMMARY_NAMES, list(res.summaries))))

    def forward_rows(self, rows, seed):
        r, rp = self._rows(rows)
        arrs, o = self._alloc_outputs(r.size)
        self._check(self._lib.alignnet_forward_dataset(self._h, rp, r.size, int(seed), C.byref(o)))
        return arrs

    # ---- ICP refinement on the full clouds (icp.py:69-78 / train.py:463-484) ------
    centroid_inits = staticmethod(centroid_inits)

    def _icp_call(self, fn, lead, inits, B, extra):
        """One call of the ICP family, fn(handle, *lead, B, init, *extra, out, fitness, rmse, iterations): lead = the clouds (blobs and offsets, or
        rows), extra = what stands between init and the outputs.  Returns dict(transforms, fitness, rmse, iterations)."""
        init = np.ascontiguousarray(inits, np.float64).reshape(B, 16)
        out = np.empty((B, 16), np.float64)
        fit, rmse, it = np.empty(B, np.float64), np.empty(B, np.float64), np.empty(B, np.int32)
        self._check(fn(self._h, *lead, B, _dp(init), *extra, _dp(out), _dp(fit), _dp(rmse), _ip(it)))
        return dict(transforms=out.reshape(B, 4, 4), fitness=fit, rmse=rmse, iterations=it)

    def _icp_refine(self, refine, register, lead, inits, B, radius, its, constrained):
        """Point-to-point ICP through `refine` (the z-constrained entry point, no flags argument) or `register` (with the full-rotation flag)."""
        if constrained:
            return self._icp_call(refine, lead, inits, B, (float(radius), int(its)))
        return self._icp_call(register, lead, inits, B, (float(radius), int(its), ICP_FULL_ROTATION))

    def icp_refine(self, sources, targets, inits, radius=0.1, its=30, constrained=True):
        """sources / targets: lists of [n, 3] arrays; inits: [B, 4, 4].  Returns dict(transforms, fitness, rmse, iterations).
        constrained=True: rotation about z only (with_constraint=True, alignnet_icp_refine); False: full 3-D rotation
        (with_constraint=False, alignnet_icp_register with ALIGNNET_ICP_FULL_ROTATION)."""
        p1, p2, off = _pack_pairs(sources, targets)
        return self._icp_refine(self._lib.alignnet_icp_refine, self._lib.alignnet_icp_register, (_fp(p1), _fp(p2), _lp(off)), inits, len(sources), radius,
                                its, constrained)

    def icp_refine_rows(self, rows, inits, radius=0.1, its=30, constrained=True):
        """Same on the clouds of the uploaded dataset (upload_dataset), addressed by example rows."""
        r, rp = self._rows(rows)
        return self._icp_refine(self._lib.alignnet_icp_refine_dataset, self._lib.alignnet_icp_register_dataset, (rp,), inits, r.size, radius, its,
                                constrained)

    # ---- evaluation of given transforms without ground truth (alignnet_evaluate_registration*; definition: tests/reg_eval_ref.py) ----
    def _evaluate_registration(self, call, B, sizes, transforms, threshold, centers, want_information, want_correspondences):
        """call(tf, threshold, centers, fitness, rmse, information, correspondences) -> rc with the pointers bound; sizes: the B source sizes."""
        tf = np.ascontiguousarray(transforms, np.float64).reshape(B, 16)
        cen = None if centers is None else np.ascontiguousarray(centers, np.float64).reshape(B, 3)
        fit, rmse = np.empty(B, np.float64), np.empty(B, np.float64)
        info = np.empty((B, 6, 6), np.float64) if want_information else None
        corr = np.full(max(int(np.sum(sizes)), 1), -1, np.int32) if want_correspondences else None
        self._check(call(_dp(tf), float(threshold), _dp(cen), _dp(fit), _dp(rmse), _dp(info), _ip(corr)))
        res = dict(fitness=fit, rmse=rmse)
        if want_information:
            res["information"] = info
        if want_correspondences:
            ends = np.cumsum(sizes, dtype=np.int64)
            res["correspondences"] = [corr[e - n:e].copy() for e, n in zip(ends, sizes)]
        return res

    def evaluate_registration(self, sources, targets, transforms, threshold=0.02, centers=None, want_information=False, want_correspondences=False):
        """Fitness and inlier RMSE of given transforms [B, 4, 4] on the pairs (sources[b], targets[b]) -- Open3D's evaluate_registration: ONE
        correspondence step, nearest target within `threshold` of every transformed source point -- with no ground truth involved.  Returns
        dict(fitness [B], rmse [B]); want_information adds information [B, 6, 6] (Open3D's get_information_matrix_from_point_clouds about
        `centers` [B, 3], default the origin), want_correspondences a list of int32 arrays (target index per source point, -1: no inlier).
        The search is the engine's icp_search option."""
        fn = self._register_fn("alignnet_evaluate_registration")
        B = len(sources)
        p1, p2, off = _pack_pairs(sources, targets)
        offp = _lp(off)
        return self._evaluate_registration(lambda *a: fn(self._h, _fp(p1), _fp(p2), offp, B, *a), B, np.diff(off[:, 0]), transforms, threshold, centers,
                                           want_information, want_correspondences)

    def evaluate_registration_rows(self, rows, transforms, threshold=0.02, centers=None, want_information=False, want_correspondences=False):
        """Same on the clouds of the uploaded dataset (upload_dataset), addressed by example rows; the correspondences follow `rows`."""
        fn = self._register_fn("alignnet_evaluate_registration_dataset")
        r, rp = self._rows(rows)
        sizes = np.zeros(r.size, np.int64)
        if want_correspondences:
            if self._dataset_sizes is None:
                raise EngineError("evaluate_registration_rows: want_correspondences needs the source sizes of a dataset uploaded with upload_dataset")
            sizes = self._dataset_sizes[np.clip(r, 0, len(self._dataset_sizes) - 1)]   # (a row out of range is the library's to report)
        return self._evaluate_registration(lambda *a: fn(self._h, rp, r.size, *a), r.size, sizes, transforms, threshold, centers, want_information,
                                           want_correspondences)

    def debug_icp_scan(self, source, target, T, radius=0.1, constrained=True, lds_points=0):
        """Test hook: ONE evaluation (correspondence step at the 4x4 `T`) of one pair by the ICP kernel's own scan, with what it decided per
        source point.  Returns dict(index [n1] chosen target, dist2 [n1] its fp64 squared distance, inlier [n1] bool, lanes [n1, 4] what each
        lane of the point's quad did with its slice of the LDS-resident targets (0 none / 1 single / 2 walk; lane s holds targets s, s + 4, ...),
        tail_won [n1] bool: the winner came from the fp64 tail, lds_points as used, fitness, rmse).  lds_points > 0 overrides the LDS stage's
        size (<= 4266) so that small clouds reach the tail."""
        p1, p2, Tm = _one_pair(source, target, T)
        n = max(len(p1), 1)
        idx, d2, inl, paths = np.full(n, -1, np.int32), np.zeros(n, np.float64), np.zeros(n, np.int32), np.zeros(n, np.int32)
        used, fit, rmse = np.zeros(1, np.int32), np.zeros(1, np.float64), np.zeros(1, np.float64)
        self._check(self._lib.alignnet_debug_icp_scan(self._h, _fp(p1), len(p1), _fp(p2), len(p2), _dp(Tm), float(radius),
                                                      0 if constrained else ICP_FULL_ROTATION, int(lds_points), _ip(idx), _dp(d2), _ip(inl), _ip(paths),
                                                      _ip(used), _dp(fit), _dp(rmse)))
        n1 = len(p1)
        paths = paths[:n1]
        return dict(index=idx[:n1].copy(), dist2=d2[:n1].copy(), inlier=inl[:n1] == 1, lanes=np.stack([(paths >> (2 * s)) & 3 for s in range(4)], -1),
                    tail_won=(paths & 256) != 0, lds_points=int(used[0]), fitness=float(fit[0]), rmse=float(rmse[0]))

    def debug_icp_grid(self, source, target, T, radius=0.1, constrained=True):
        """Test hook: the grid build and ONE evaluation (correspondence step at the 4x4 `T`) of one pair by the ICP kernel's grid search
        (set_option("icp_search", 1) selects it for icp_refine*; this read-back takes it whatever the option says).  Returns dict(index [n1]
        chosen target's original index, -1 without a candidate; dist2 [n1] fp64 squared distance, inf without; inlier [n1] bool; candidates
        [n1] records evaluated; cell_edge; buckets_occupied; largest_bucket; fitness; rmse)."""
        p1, p2, Tm = _one_pair(source, target, T)
        n = max(len(p1), 1)
        idx, d2, inl, cand = np.full(n, -1, np.int32), np.zeros(n, np.float64), np.zeros(n, np.int32), np.zeros(n, np.int32)
        edge, occ, big, fit, rmse = np.zeros(1, np.float64), np.zeros(1, np.int32), np.zeros(1, np.int32), np.zeros(1, np.float64), np.zeros(1, np.float64)
        self._check(self._lib.alignnet_debug_icp_grid(self._h, _fp(p1), len(p1), _fp(p2), len(p2), _dp(Tm), float(radius),
                                                      0 if constrained else ICP_FULL_ROTATION, _ip(idx), _dp(d2), _ip(inl), _ip(cand), _dp(edge), _ip(occ),
                                                      _ip(big), _dp(fit), _dp(rmse)))
        n1 = len(p1)
        return dict(index=idx[:n1].copy(), dist2=d2[:n1].copy(), inlier=inl[:n1] == 1, candidates=cand[:n1].copy(), cell_edge=float(edge[0]),
                    buckets_occupied=int(occ[0]), largest_bucket=int(big[0]), fitness=float(fit[0]), rmse=float(rmse[0]))

    # ---- point-to-plane ICP (csrc/alignnet_icp.hip: icp_plane_*; semantics: tests/icp_plane_ref.py) ----
    def _icp_surface(self, fn, lead, inits, B, radius, normal_radius, its, constrained):
        """Point-to-plane or generalized ICP through the entry point `fn`: both take (radius, normal_radius, its, flags) behind init."""
        return self._icp_call(fn, lead, inits, B, (float(radius), float(normal_radius), int(its), 0 if constrained else ICP_FULL_ROTATION))

    def icp_plane_refine(self, sources, targets, inits, radius=0.1, normal_radius=0.3, its=30, constrained=True):
        """Point-to-plane ICP: icp_refine's loop (nearest target within `radius`, same stop rule, same return dict) with the estimate that
        minimises the distances to the targets' tangent planes.  The target normals are computed once per call from ALL target points within
        `normal_radius` (fewer than 3: (0, 0, 1); orientation n_z >= 0).  constrained=True: rotation about z + translation; False: six unknowns.
        A singular system (a single plane) leaves the transform as it is.  Why 0.3 and not the search radius: the 64-ring sensor's ring spacing
        is 0.0075 x range, so at 20 m a radius of 0.1 sees only one ring and every neighbourhood is a line."""
        p1, p2, off = _pack_pairs(sources, targets)
        return self._icp_surface(self._lib.alignnet_icp_plane_register, (_fp(p1), _fp(p2), _lp(off)), inits, len(sources), radius, normal_radius, its,
                                 constrained)

    def icp_plane_refine_rows(self, rows, inits, radius=0.1, normal_radius=0.3, its=30, constrained=True):
        """Same on the clouds of the uploaded dataset (upload_dataset), addressed by example rows."""
        r, rp = self._rows(rows)
        return self._icp_surface(self._lib.alignnet_icp_plane_register_dataset, (rp,), inits, r.size, radius, normal_radius, its, constrained)

    # ---- generalized (plane-to-plane) ICP (csrc/alignnet_icp.hip: icp_generalized_*; semantics: tests/icp_generalized_ref.py) ----
    def icp_generalized_refine(self, sources, targets, inits, radius=0.1, normal_radius=0.3, its=30, constrained=True):
        """Generalized ICP (Segal, Haehnel, Thrun 2009): icp_plane_refine's loop, arguments and return dict with every correspondence weighted by
        the inverse of the sum of the two surface covariances (1e-3 along the normal, 1 across it).  Normals of BOTH clouds are computed once per
        call, each cloud on its own within `normal_radius`, the source's in its own frame.  A single plane gives a regular system."""
        p1, p2, off = _pack_pairs(sources, targets)
        return self._icp_surface(self._register_fn("alignnet_icp_generalized_register"), (_fp(p1), _fp(p2), _lp(off)), inits, len(sources), radius,
                                 normal_radius, its, constrained)

    def icp_generalized_refine_rows(self, rows, inits, radius=0.1, normal_radius=0.3, its=30, constrained=True):
        """Same on the clouds of the uploaded dataset (upload_dataset), addressed by example rows."""
        r, rp = self._rows(rows)
        return self._icp_surface(self._register_fn("alignnet_icp_generalized_register_dataset"), (rp,), inits, r.size, radius, normal_radius, its,
                                 constrained)

    # ---- multi-scale (coarse-to-fine) ICP (csrc/alignnet_multiscale.hip; definition: tests/icp_multiscale_ref.py) ----
    def _icp_multiscale(self, fn, lead, inits, B, voxel_sizes, radii, its, estimate, normal_radius, constrained):
        """One multi-scale call through `fn`: the schedule's three lists go down as arrays of L, normal_radius as a scalar or a list of L."""
        if estimate not in ("point", "plane", "generalized"):
            raise ValueError("estimate must be one of point, plane, generalized, got %r" % (estimate,))
        vs = np.ascontiguousarray(voxel_sizes, np.float64).reshape(-1)
        rd = np.ascontiguousarray(radii, np.float64).reshape(-1)
        it = np.ascontiguousarray(its, np.int32).reshape(-1)
        L = vs.size
        if rd.size != L or it.size != L:
            raise ValueError("voxel_sizes, radii and its must have one entry per level (%d, %d, %d)" % (L, rd.size, it.size))
        nr = np.ascontiguousarray(np.broadcast_to(np.asarray(normal_radius, np.float64).reshape(-1), (L,)) if L else np.zeros(0))
        init = np.ascontiguousarray(inits, np.float64).reshape(B, 16)
        out = np.empty((B, 16), np.float64)
        fit, rmse = np.empty(B, np.float64), np.empty(B, np.float64)
        iters, sizes = np.zeros((B, max(L, 1)), np.int32), np.zeros((B, max(L, 1), 2), np.int32)
        self._check(fn(self._h, *lead, B, _dp(init), L, _dp(vs), _dp(rd), _ip(it), _dp(nr), self.REFINE[estimate],
                       0 if constrained else ICP_FULL_ROTATION, _dp(out), _dp(fit), _dp(rmse), _ip(iters), _ip(sizes)))
        return dict(transforms=out.reshape(B, 4, 4), fitness=fit, rmse=rmse, iterations=iters, level_sizes=sizes)

    def icp_multiscale_refine(self, sources, targets, inits, voxel_sizes, radii, its, estimate="point", normal_radius=0.3, constrained=True):
        """Coarse-to-fine ICP (Open3D's multi_scale_icp): level l voxel-downsamples both clouds of every pair at voxel_sizes[l] (<= 0: the raw
        clouds) and runs icp_refine / icp_plane_refine / icp_generalized_refine (`estimate`) on them with radii[l] and its[l], from the
        transform of the level before (level 0: `inits`).  The level clouds and the transforms between levels stay on the device.  Returns
        dict(transforms, fitness, rmse: the last level's, on its clouds at its radius; iterations [B, L]; level_sizes [B, L, 2])."""
        p1, p2, off = _pack_pairs(sources, targets)
        return self._icp_multiscale(self._register_fn("alignnet_icp_multiscale_register"), (_fp(p1), _fp(p2), _lp(off)), inits, len(sources),
                                    voxel_sizes, radii, its, estimate, normal_radius, constrained)

    def icp_multiscale_refine_rows(self, rows, inits, voxel_sizes, radii, its, estimate="point", normal_radius=0.3, constrained=True):
        """Same on the clouds of the uploaded dataset (upload_dataset), addressed by example rows."""
        r, rp = self._rows(rows)
        return self._icp_multiscale(self._register_fn("alignnet_icp_multiscale_register_dataset"), (rp,), inits, r.size, voxel_sizes, radii, its,
                                    estimate, normal_radius, constrained)

    def debug_voxel_pyramid(self, cloud, voxel_sizes):
        """Test hook: the level clouds of one cloud as the multi-scale ICP builds them, through the shipped kernels.  Returns a list with one
        dict per level: points [m, 3] float32 (what the ICP reads), means [m, 3] float64 (before the rounding), voxels [m, 3] int32 in
        ascending (ix, iy, iz), counts [m] int32.  A level with voxel <= 0 is the raw cloud: voxels None, counts all 1."""
        p = np.ascontiguousarray(np.asarray(cloud, np.float32).reshape(-1, 3))
        vs = np.ascontiguousarray(voxel_sizes, np.float64).reshape(-1)
        n, L = len(p), vs.size
        cap = max(n, 1)
        pts, mean = np.zeros((max(L, 1), cap, 3), np.float32), np.zeros((max(L, 1), cap, 3), np.float64)
        vox, cnt, sizes = np.zeros((max(L, 1), cap, 3), np.int32), np.zeros((max(L, 1), cap), np.int32), np.zeros(max(L, 1), np.int64)
        # (the library lays the levels out [L][n]: with n = 0 nothing is written)
        self._check(self._register_fn("alignnet_debug_voxel_pyramid")(self._h, _fp(p), n, L, _dp(vs), _fp(pts), _dp(mean), _ip(vox), _ip(cnt), _lp(sizes)))
        levels = []
        for l in range(L):
            if not vs[l] > 0:
                levels.append(dict(points=p.copy(), means=p.astype(np.float64), voxels=None, counts=np.ones(n, np.int32)))
                continue
            m = int(sizes[l])
            levels.append(dict(points=pts[l, :m].copy(), means=mean[l, :m].copy(), voxels=vox[l, :m].copy(), counts=cnt[l, :m].copy()))
        return levels

    # ---- one-call registration: clouds to transforms on the device (csrc/alignnet_register.hip) ----
    REFINE = {None: 0, "point": 1, "plane": 2, "generalized": 4}   # (the option values of alignnet_register_options.refine; 3 is not assigned)

    def _register_fn(self, name):
        try:
            return getattr(self._lib, name)
        except AttributeError:
            raise EngineError("%s does not export %s: it was built from a revision before that entry point was added; rebuild it "
                              "(make -C alignnet-3d_amd/csrc)" % (_capi.library_path(), name)) from None

    def _register_bufs(self, B, refine, radius, normal_radius, its, constrained, want_net, want_loss):
        if refine not in self.REFINE:
            raise ValueError("refine = %r: expected None, 'point', 'plane' or 'generalized'" % (refine,))
        opt = _capi.RegisterOptions(self.REFINE[refine], int(its) if refine else 0, 0 if constrained else ICP_FULL_ROTATION, float(radius),
                                    float(normal_radius))
        n = max(B, 0)
        res = dict(transforms=np.empty((n, 4, 4), np.float64), network_transforms=np.empty((n, 4, 4), np.float64), angles=np.empty((n, 4), np.float64))
        out = _capi.RegisterOutputs()
        out.transforms, out.network_transforms, out.angles = _dp(res["transforms"]), _dp(res["network_transforms"]), _dp(res["angles"])
        keep = []
        if refine:
            res.update(fitness=np.empty(n, np.float64), rmse=np.empty(n, np.float64), iterations=np.empty(n, np.int32))
            out.fitness, out.rmse, out.iterations = _dp(res["fitness"]), _dp(res["rmse"]), _ip(res["iterations"])
        if want_net:
            arrs, o = self._alloc_outputs(n)
            res.update(arrs)
            keep.append(o)
            out.net = C.pointer(o)
        loss = None
        if want_loss:
            loss = np.empty(17, np.float32)
            out.loss = _fp(loss)
        return opt, out, res, loss, keep

    @staticmethod
    def _register_finish(res, loss):
        res["loss"] = None if loss is None else (float(loss[0]), dict(zip(SUMMARY_NAMES, [float(v) for v in loss[1:]])))
        return res

    def register(self, sources, targets, seed=0, streams=None, refine=None, radius=0.1, normal_radius=0.3, its=30, constrained=True, want_net=False):
        """Two raw clouds per pair in, a 4x4 per pair out, in ONE engine call: the sampler's draw, the eval forward, the fp64 yaw decode, the
        initial transform T_net and -- refine="point" | "plane" | "generalized" -- ICP on the full clouds from it, with no return to the host in between.
        sources / targets: lists of [n, 3] arrays; streams: [B] ids of the pairs' random streams (None: the pair index) -- pair b is drawn as
        register_rows would draw it were the pair example streams[b] of the dataset.  Returns dict(transforms [B, 4, 4] (refined, or T_net),
        network_transforms [B, 4, 4], angles [B, 4] = a1, a2, a_rem, pred_angle, loss=None; fitness, rmse, iterations when refining; the
        eight network arrays with want_net)."""
        fn = self._register_fn("alignnet_register")
        B = len(sources)
        if len(targets) != B:
            raise ValueError("register: %d sources and %d targets" % (B, len(targets)))
        p1, p2, off = _pack_pairs(sources, targets)
        st = None
        if streams is not None:
            st = np.ascontiguousarray(streams, np.int64).ravel()
            if st.size != B:
                raise ValueError("register: %d streams for %d pairs" % (st.size, B))
        opt, out, res, loss, keep = self._register_bufs(B, refine, radius, normal_radius, its, constrained, want_net, False)
        self._check(fn(self._h, _fp(p1), _fp(p2), _lp(off), B, int(seed), _lp(st), C.byref(opt), C.byref(out)))
        return self._register_finish(res, loss)

    def register_rows(self, rows, seed, refine=None, radius=0.1, normal_radius=0.3, its=30, constrained=True, want_net=False, want_loss=False):
        """Same on rows of the uploaded dataset (upload_dataset): the batch forward_rows(rows, seed) draws.  want_loss: loss = (loss, summaries)
        as eval_loss returns them for this batch against the dataset's labels."""
        fn = self._register_fn("alignnet_register_dataset")
        r, rp = self._rows(rows)
        opt, out, res, loss, keep = self._register_bufs(r.size, refine, radius, normal_radius, its, constrained, want_net, want_loss)
        self._check(fn(self._h, rp, r.size, int(seed), C.byref(opt), C.byref(out)))
        return self._register_finish(res, loss)

    def debug_icp_plane(self, source, target, T, radius=0.1, normal_radius=0.3, constrained=True):
        """Test hook: one pair through the point-to-plane kernels' own source -- the target's normals and neighbour counts, ONE evaluation at the
        4x4 `T` and the estimate that follows.  Returns dict(normals [n2, 3], neighbours [n2], index [n1] (-1 without a candidate), dist2 [n1]
        (inf without), inlier [n1] bool, residual [n1] (0 for outliers), sums [29] (count, sum dist2, upper triangle of J^T J, J^T r; 16 used
        by the z-constrained estimate), update [4, 4], fitness, rmse)."""
        p1, p2, Tm = _one_pair(source, target, T)
        n, m = max(len(p1), 1), max(len(p2), 1)
        nrm, nbr = np.zeros((m, 3), np.float64), np.zeros(m, np.int32)
        idx, d2, inl, res = np.full(n, -1, np.int32), np.zeros(n, np.float64), np.zeros(n, np.int32), np.zeros(n, np.float64)
        sums, upd, fit, rmse = np.zeros(29, np.float64), np.zeros(16, np.float64), np.zeros(1, np.float64), np.zeros(1, np.float64)
        self._check(self._lib.alignnet_debug_icp_plane(self._h, _fp(p1), len(p1), _fp(p2), len(p2), _dp(Tm), float(radius), float(normal_radius),
                                                       0 if constrained else ICP_FULL_ROTATION, _dp(nrm), _ip(nbr), _ip(idx), _dp(d2), _ip(inl), _dp(res),
                                                       _dp(sums), _dp(upd), _dp(fit), _dp(rmse)))
        n1, n2 = len(p1), len(p2)
        return dict(normals=nrm[:n2].copy(), neighbours=nbr[:n2].copy(), index=idx[:n1].copy(), dist2=d2[:n1].copy(), inlier=inl[:n1] == 1,
                    residual=res[:n1].copy(), sums=sums, update=upd.reshape(4, 4), fitness=float(fit[0]), rmse=float(rmse[0]))

    def debug_icp_generalized(self, source, target, T, radius=0.1, normal_radius=0.3, constrained=True):
        """Test hook: one pair through the generalized-ICP kernels' own source -- both clouds' normals and neighbour counts, ONE evaluation at the
        4x4 `T` and the estimate that follows.  Returns dict(normals [n2, 3], neighbours [n2] (the target's), source_normals [n1, 3],
        source_neighbours [n1], index [n1] (-1 without a candidate), dist2 [n1] (inf without), inlier [n1] bool, sums [29] (count, sum dist2, upper
        triangle of J^T M J, J^T M d; 16 used by the z-constrained estimate), update [4, 4], fitness, rmse)."""
        p1, p2, Tm = _one_pair(source, target, T)
        n, m = max(len(p1), 1), max(len(p2), 1)
        nrm, nbr, snrm, snbr = np.zeros((m, 3), np.float64), np.zeros(m, np.int32), np.zeros((n, 3), np.float64), np.zeros(n, np.int32)
        idx, d2, inl = np.full(n, -1, np.int32), np.zeros(n, np.float64), np.zeros(n, np.int32)
        sums, upd, fit, rmse = np.zeros(29, np.float64), np.zeros(16, np.float64), np.zeros(1, np.float64), np.zeros(1, np.float64)
        self._check(self._lib.alignnet_debug_icp_generalized(self._h, _fp(p1), len(p1), _fp(p2), len(p2), _dp(Tm), float(radius), float(normal_radius),
                                                             0 if constrained else ICP_FULL_ROTATION, _dp(nrm), _ip(nbr), _dp(snrm), _ip(snbr), _ip(idx),
                                                             _dp(d2), _ip(inl), _dp(sums), _dp(upd), _dp(fit), _dp(rmse)))
        n1, n2 = len(p1), len(p2)
        return dict(normals=nrm[:n2].copy(), neighbours=nbr[:n2].copy(), source_normals=snrm[:n1].copy(), source_neighbours=snbr[:n1].copy(),
                    index=idx[:n1].copy(), dist2=d2[:n1].copy(), inlier=inl[:n1] == 1, sums=sums, update=upd.reshape(4, 4), fitness=float(fit[0]),
                    rmse=float(rmse[0]))

    # ---- global registration: RANSAC on FPFH feature matches (csrc/alignnet_globalreg.hip) ----
    @staticmethod
    def _global_bufs(B, streams, default_streams):
        st = np.ascontiguousarray(default_streams if streams is None else streams, np.int32).ravel()
        if st.size != B:
            raise ValueError("streams: one id per pair (%d given for %d pairs)" % (st.size, B))
        out = np.empty((B, 16), np.float64)
        fit, rmse = np.empty(B, np.float64), np.empty(B, np.float64)
        it, val = np.empty(B, np.int64), np.empty(B, np.int32)
        tail = (_dp(out), _dp(fit), _dp(rmse), _lp(it), _ip(val))
        return st, tail, lambda: dict(transforms=out.reshape(B, 4, 4), fitness=fit, rmse=rmse, iterations=it, validations=val)

    def global_register(self, sources, targets, constrained=True, seed=0, streams=None, max_iteration=4000000, max_validation=500):
        """RANSAC on FPFH feature matches of the 5 cm voxel-downsampled clouds (the reference's o3_gicp, no ICP after it).
        sources / targets: lists of [n, 3] arrays.  constrained=True: rotation about z only; False: full 3-D rotation.
        streams: one non-negative id per pair selecting its random draws under `seed` (default 0 .. B - 1); a pair's result
        depends on (seed, stream, clouds, arguments) only.  Returns dict(transforms, fitness, rmse, iterations, validations)."""
        B = len(sources)
        p1, p2, off = _pack_pairs(sources, targets)
        st, tail, result = self._global_bufs(B, streams, np.arange(B))
        self._check(self._lib.alignnet_global_register(self._h, _fp(p1), _fp(p2), _lp(off), B, 0 if constrained else ICP_FULL_ROTATION, int(seed),
                                                       _ip(st), int(max_iteration), int(max_validation), *tail))
        return result()

    def global_register_rows(self, rows, constrained=True, seed=0, streams=None, max_iteration=4000000, max_validation=500):
        """Same on the clouds of the uploaded dataset (upload_dataset), addressed by example rows; streams default to the rows."""
        r, rp = self._rows(rows)
        st, tail, result = self._global_bufs(r.size, streams, r)
        self._check(self._lib.alignnet_global_register_dataset(self._h, rp, r.size, 0 if constrained else ICP_FULL_ROTATION, int(seed), _ip(st),
                                                               int(max_iteration), int(max_validation), *tail))
        return result()

    def debug_global_stages(self, source, target, constrained=True, seed=0, stream=0, max_iteration=4000000, max_validation=500):
        """Test hook: global_register of one pair, with the stage outputs.  Returns the result dict (scalars, transform [4, 4]) plus
        per cloud (index 0 = source, 1 = target) lists points / voxels / voxel_points / normals / spfh / fpfh, `matches` (target index
        of every downsampled source point) and `winning_iteration` (-1: no hypothesis was validated)."""
        p1, p2, _ = _one_pair(source, target)
        cap = max(len(p1), len(p2), 1)
        counts = np.zeros(2, np.int32)
        pts, vox, npt = np.zeros((2, cap, 3), np.float64), np.zeros((2, cap, 3), np.int32), np.zeros((2, cap), np.int32)
        nrm, spfh, fpfh = np.zeros((2, cap, 3), np.float64), np.zeros((2, cap, 33), np.float64), np.zeros((2, cap, 33), np.float64)
        match, win = np.zeros(cap, np.int32), np.zeros(1, np.int64)
        st, tail, result = self._global_bufs(1, [stream], None)
        self._check(self._lib.alignnet_debug_global_stages(self._h, _fp(p1), len(p1), _fp(p2), len(p2), 0 if constrained else ICP_FULL_ROTATION, int(seed),
                                                           int(stream), int(max_iteration), int(max_validation), cap, _ip(counts), _dp(pts), _ip(vox), _ip(npt),
                                                           _dp(nrm), _dp(spfh), _dp(fpfh), _ip(match), _lp(win), *tail))
        res = result()
        out = dict(transform=res["transforms"][0], fitness=float(res["fitness"][0]), rmse=float(res["rmse"][0]), iterations=int(res["iterations"][0]),
                   validations=int(res["validations"][0]), winning_iteration=int(win[0]), counts=counts.copy(), matches=match[: counts[0]].copy())
        for name, arr in (("points", pts), ("voxels", vox), ("voxel_points", npt), ("normals", nrm), ("spfh", spfh), ("fpfh", fpfh)):
            out[name] = [arr[k, : counts[k]].copy() for k in range(2)]
        return out

    # ---- fast global registration on FPFH feature matches (csrc/alignnet_globalreg.hip, the fgr_* kernels) ----
    @staticmethod
    def _fgr_bufs(B, streams, default_streams, constrained, decrease_mu, division_factor, maximum_correspondence_distance, iteration_number,
                  tuple_scale, maximum_tuple_count):
        st = np.ascontiguousarray(default_streams if streams is None else streams, np.int32).ravel()
        if st.size != B:
            raise ValueError("streams: one id per pair (%d given for %d pairs)" % (st.size, B))
        out = np.empty((B, 16), np.float64)
        fit, rmse = np.empty(B, np.float64), np.empty(B, np.float64)
        corr, trials = np.empty(B, np.int32), np.empty(B, np.int64)
        flags = (0 if constrained else ICP_FULL_ROTATION) | (FGR_DECREASE_MU if decrease_mu else 0)
        options = (float(division_factor), float(maximum_correspondence_distance), int(iteration_number), float(tuple_scale), int(maximum_tuple_count))
        tail = (_dp(out), _dp(fit), _dp(rmse), _ip(corr), _lp(trials))
        return st, flags, options, tail, lambda: dict(transforms=out.reshape(B, 4, 4), fitness=fit, rmse=rmse, correspondences=corr, trials=trials)

    def fgr_register(self, sources, targets, constrained=True, decrease_mu=False, seed=0, streams=None, division_factor=1.4,
                     maximum_correspondence_distance=0.025, iteration_number=64, tuple_scale=0.95, maximum_tuple_count=1000):
        """Fast global registration on FPFH feature matches of the 5 cm voxel-downsampled clouds (the reference's o3_gicp_fast, no ICP
        after it; defined by tests/fgr_ref.py).  sources / targets: lists of [n, 3] arrays.  constrained=True: rotation about z only; False:
        full 3-D rotation.  decrease_mu: Open3D's FastGlobalRegistrationOption.decrease_mu.  streams: one non-negative id per pair selecting
        its tuple draws under `seed` (default 0 .. B - 1); a pair's result depends on (seed, stream, clouds, arguments) only.
        Returns dict(transforms, fitness, rmse, correspondences, trials)."""
        B = len(sources)
        p1, p2, off = _pack_pairs(sources, targets)
        st, flags, options, tail, result = self._fgr_bufs(B, streams, np.arange(B), constrained, decrease_mu, division_factor,
                                                          maximum_correspondence_distance, iteration_number, tuple_scale, maximum_tuple_count)
        self._check(self._lib.alignnet_fgr_register(self._h, _fp(p1), _fp(p2), _lp(off), B, flags, int(seed), _ip(st), *options, *tail))
        return result()

    def fgr_register_rows(self, rows, constrained=True, decrease_mu=False, seed=0, streams=None, division_factor=1.4,
                          maximum_correspondence_distance=0.025, iteration_number=64, tuple_scale=0.95, maximum_tuple_count=1000):
        """Same on the clouds of the uploaded dataset (upload_dataset), addressed by example rows; streams default to the rows."""
        r, rp = self._rows(rows)
        st, flags, options, tail, result = self._fgr_bufs(r.size, streams, r, constrained, decrease_mu, division_factor,
                                                          maximum_correspondence_distance, iteration_number, tuple_scale, maximum_tuple_count)
        self._check(self._lib.alignnet_fgr_register_dataset(self._h, rp, r.size, flags, int(seed), _ip(st), *options, *tail))
        return result()

    def debug_fgr_stages(self, source, target, constrained=True, decrease_mu=False, seed=0, stream=0, division_factor=1.4,
                         maximum_correspondence_distance=0.025, iteration_number=64, tuple_scale=0.95, maximum_tuple_count=1000):
        """Test hook: fgr_register of one pair, with the stage outputs.  Returns the result dict (scalars, transform [4, 4]) plus per cloud
        (index 0 = source, 1 = target) lists points / fpfh, `matches` (target index of every downsampled source point), `reverse_matches`
        (source index of every downsampled target point), `cross` (source indices of the mutual matches, ascending), `tuple_source` /
        `tuple_target` (the correspondences the tuple test kept, 3 per accepted trial, in trial order), `tuple_trials` (the trial of every
        accepted tuple), `means` [2, 3], `scale`, and `trace` [iteration_number, 4, 4]: the transform after every iteration, in the normalised
        frame, moving the target onto the source."""
        p1, p2, _ = _one_pair(source, target)
        cap = max(len(p1), len(p2), 1)
        mtc, its = max(int(maximum_tuple_count), 0), max(int(iteration_number), 0)
        counts = np.zeros(4, np.int32)
        pts, fpfh = np.zeros((2, cap, 3), np.float64), np.zeros((2, cap, 33), np.float64)
        match, rmatch, cross = np.zeros(cap, np.int32), np.zeros(cap, np.int32), np.zeros(cap, np.int32)
        ts, tt, ttr = np.zeros(3 * mtc + 1, np.int32), np.zeros(3 * mtc + 1, np.int32), np.zeros(mtc + 1, np.int64)
        norm, trace = np.zeros(7, np.float64), np.zeros((its + 1, 16), np.float64)
        st, flags, options, tail, result = self._fgr_bufs(1, [stream], None, constrained, decrease_mu, division_factor,
                                                          maximum_correspondence_distance, iteration_number, tuple_scale, maximum_tuple_count)
        self._check(self._lib.alignnet_debug_fgr_stages(self._h, _fp(p1), len(p1), _fp(p2), len(p2), flags, int(seed), int(stream), *options, cap,
                                                        _ip(counts), _dp(pts), _dp(fpfh), _ip(match), _ip(rmatch), _ip(cross), _ip(ts), _ip(tt),
                                                        _lp(ttr), _dp(norm), _dp(trace), *tail))
        res = result()
        na = int(counts[3])
        out = dict(transform=res["transforms"][0], fitness=float(res["fitness"][0]), rmse=float(res["rmse"][0]),
                   correspondences=int(res["correspondences"][0]), trials=int(res["trials"][0]), counts=counts[:2].copy(),
                   matches=match[: counts[0]].copy() if counts[1] else match[:0].copy(),
                   reverse_matches=rmatch[: counts[1]].copy() if counts[0] else rmatch[:0].copy(), cross=cross[: counts[2]].copy(),
                   tuple_source=ts[: 3 * na].copy(), tuple_target=tt[: 3 * na].copy(), tuple_trials=ttr[:na].copy(),
                   means=norm[:6].reshape(2, 3).copy(), scale=float(norm[6]), trace=trace[:its].reshape(its, 4, 4).copy())
        for name, arr in (("points", pts), ("fpfh", fpfh)):
            out[name] = [arr[k, : counts[k]].copy() for k in range(2)]
        return out

    # ---- Go-ICP: branch-and-bound over yaw and a translation box (csrc/alignnet_goicp.hip; semantics: tests/goicp_ref.py) ----
    GOICP_STATUS = ("CERTIFIED", "RESOLUTION", "OVERFLOW", "LEVELS", "EMPTY")
    GOICP_DEFAULTS = dict(yaw_half=np.pi, t_half=(2.0, 2.0, 0.25), yaw_res=np.pi / 256, t_res=0.02, trunc=0.5, mse_thresh=1e-4, max_source=256,
                          max_target=2048, max_frontier=1 << 18, max_levels=_capi.GOICP_MAX_LEVELS, starts=8, start_radius=0.5, start_its=30,
                          fitness_radius=0.10, stage_points=0)
    GOICP_REFINE_RADIUS, GOICP_REFINE_ITS = 0.10, 30   # icp.py:188-189: refine_radius=0.10; the ICP calls' 30 iterations

    @classmethod
    def _goicp_params(cls, constrained, refine, kw):
        if not constrained:
            raise NotImplementedError("goicp searches yaw and translation only (with_constraint=True): there is no full-rotation form")
        if refine not in (None, "p2p"):
            raise ValueError("goicp: refine must be None or 'p2p', got %r" % (refine,))
        unknown = sorted(set(kw) - set(cls.GOICP_DEFAULTS))
        if unknown:
            raise TypeError("goicp: unknown parameters %s" % ", ".join(unknown))
        v = dict(cls.GOICP_DEFAULTS, **kw)
        p = _capi.GoicpParams()
        p.yaw_half, p.yaw_res, p.t_res, p.trunc, p.mse_thresh, p.start_radius = (float(v[k]) for k in ("yaw_half", "yaw_res", "t_res", "trunc", "mse_thresh",
                                                                                                        "start_radius"))
        p.fitness_radius = float(v["fitness_radius"])
        th = [float(x) for x in v["t_half"]]
        if len(th) != 3:
            raise ValueError("goicp: t_half has three entries")
        for k in range(3):
            p.t_half[k] = th[k]
        for k in ("max_source", "max_target", "max_frontier", "max_levels", "starts", "start_its", "stage_points"):
            setattr(p, k, int(v[k]))
        p.flags = 0
        return p

    @staticmethod
    def _goicp_bufs(B):
        L = _capi.GOICP_MAX_LEVELS
        out, err, low, fit = np.empty((B, 16), np.float64), np.empty(B, np.float64), np.empty(B, np.float64), np.empty(B, np.float64)
        st, ev, sv = np.empty(B, np.int32), np.empty((B, L), np.int32), np.empty((B, L), np.int32)
        tail = (_dp(out), _dp(err), _dp(low), _dp(fit), _ip(st), _ip(ev), _ip(sv))
        return tail, lambda: dict(transforms=out.reshape(B, 4, 4), error=err, lower_bound=low, fitness=fit, status=st, evaluated=ev, survived=sv)

    def goicp_register(self, sources, targets, constrained=True, refine=None, **params):
        """Branch-and-bound registration over yaw and a translation box (the reference's `goicp`, which it leaves unimplemented): the pose
        with the lowest truncated nearest-neighbour error E on subsampled working sets, independent of any start, with a certificate.
        sources / targets: lists of [n, 3] arrays; params: GOICP_DEFAULTS keys.  Returns dict(transforms [B, 4, 4] about the origin, error,
        lower_bound (no pose of the domain has a smaller E), fitness (share of the source working set within
        fitness_radius of a target at the returned pose), status (index into GOICP_STATUS), evaluated / survived [B, 24] nodes per
        level).  refine="p2p": icp_refine on the FULL clouds (radius 0.10, 30 iterations) from the search's pose follows; `transforms` is
        then the refined estimate, `search_transforms` the search's, and fitness / rmse / iterations are the refinement's.
        constrained=False raises NotImplementedError before anything reaches the device."""
        p = self._goicp_params(constrained, refine, params)
        fn = self._register_fn("alignnet_goicp_register")
        B = len(sources)
        if len(targets) != B:
            raise ValueError("goicp_register: %d sources and %d targets" % (B, len(targets)))
        p1, p2, off = _pack_pairs(sources, targets)
        tail, result = self._goicp_bufs(B)
        self._check(fn(self._h, _fp(p1), _fp(p2), _lp(off), B, C.byref(p), *tail))
        res = result()
        if refine == "p2p":
            ref = self.icp_refine(sources, targets, res["transforms"], radius=self.GOICP_REFINE_RADIUS, its=self.GOICP_REFINE_ITS)
            res.update(search_transforms=res["transforms"], **ref)
        return res

    def goicp_register_rows(self, rows, constrained=True, refine=None, **params):
        """Same on the clouds of the uploaded dataset (upload_dataset), addressed by example rows."""
        p = self._goicp_params(constrained, refine, params)
        fn = self._register_fn("alignnet_goicp_register_dataset")
        r, rp = self._rows(rows)
        tail, result = self._goicp_bufs(r.size)
        self._check(fn(self._h, rp, r.size, C.byref(p), *tail))
        res = result()
        if refine == "p2p":
            ref = self.icp_refine_rows(r, res["transforms"], radius=self.GOICP_REFINE_RADIUS, its=self.GOICP_REFINE_ITS)
            res.update(search_transforms=res["transforms"], **ref)
        return res

    def debug_goicp_nodes(self, source, target, depth, coords, **params):
        """Test hook: (ub [K], lb [K]) of K nodes of one pair, given as integer coordinates coords [K, 4] at the halvings depth [4] of
        (theta, x, y, z), by the search's own evaluation kernel."""
        p = self._goicp_params(True, None, params)
        p1, p2, _ = _one_pair(source, target)
        d = np.ascontiguousarray(depth, np.int32).reshape(4)
        c = np.ascontiguousarray(coords, np.int32).reshape(-1, 4)
        ub, lb = np.empty(len(c), np.float64), np.empty(len(c), np.float64)
        self._check(self._lib.alignnet_debug_goicp_nodes(self._h, _fp(p1), len(p1), _fp(p2), len(p2), C.byref(p), _ip(d), _ip(c), len(c), _dp(ub), _dp(lb)))
        return ub, lb

    # ---- multiway registration: pose-graph optimisation (csrc/alignnet_posegraph.hip; semantics: tests/pose_graph_ref.py) ----
    POSE_GRAPH_STATUS = ("CONVERGED", "ITERATIONS", "STALLED", "EMPTY")
    POSE_GRAPH_PRUNE = 0.25   # Open3D's edge_prune_threshold

    @staticmethod
    def _pose_graph_arrays(graphs):
        """The concatenated arrays of a list of graphs; each graph is a dict(poses [n, 4, 4], i [m], j [m], T [m, 4, 4], info [m, 6, 6], c [m, 3],
        uncertain [m]).  Checks shapes, indices and finiteness: nothing wrong reaches the library."""
        node_off, edge_off = np.zeros(len(graphs) + 1, np.int64), np.zeros(len(graphs) + 1, np.int64)
        poses, edges, T, info, c, unc = [], [], [], [], [], []
        for k, g in enumerate(graphs):
            X = np.asarray(g["poses"], np.float64)
            if X.ndim != 3 or X.shape[1:] != (4, 4) or len(X) < 1:
                raise ValueError("pose graph %d: poses must be [n >= 1, 4, 4]" % k)
            n, m = len(X), len(g["i"])
            e = np.stack([np.asarray(g["i"], np.int64).reshape(m), np.asarray(g["j"], np.int64).reshape(m)], 1)
            if m and (e.min() < 0 or e.max() >= n):
                raise ValueError("pose graph %d: edge index out of range" % k)
            if m and (e[:, 0] == e[:, 1]).any():
                raise ValueError("pose graph %d: an edge joins a node to itself (i == j)" % k)
            parts = (X, np.asarray(g["T"], np.float64).reshape(m, 4, 4), np.asarray(g["info"], np.float64).reshape(m, 6, 6),
                     np.asarray(g["c"], np.float64).reshape(m, 3))
            if not all(np.isfinite(p).all() for p in parts):
                raise ValueError("pose graph %d: a non-finite entry" % k)
            node_off[k + 1], edge_off[k + 1] = node_off[k] + n, edge_off[k] + m
            poses.append(X); edges.append(e.astype(np.int32)); T.append(parts[1]); info.append(parts[2]); c.append(parts[3])
            unc.append(np.asarray(g["uncertain"]).reshape(m).astype(bool).astype(np.int32))
        cat = lambda L, shape, dt: np.ascontiguousarray(np.concatenate(L, 0), dt) if L else np.zeros(shape, dt)
        return (node_off, edge_off, cat(poses, (0, 4, 4), np.float64), cat(edges, (0, 2), np.int32), cat(T, (0, 4, 4), np.float64),
                cat(info, (0, 6, 6), np.float64), cat(c, (0, 3), np.float64), cat(unc, (0,), np.int32))

    @staticmethod
    def _pose_graph_mu(graphs, info, edge_off, mu, preference, threshold):
        """mu per graph: the given value(s), or Open3D's rule preference * threshold^2 * the mean inlier count (info[5, 5]) of the graph's edges."""
        G = len(graphs)
        if mu is None:
            out = np.ones(G)
            for k in range(G):
                count = info[edge_off[k]: edge_off[k + 1], 5, 5].mean() if edge_off[k + 1] > edge_off[k] else 0.0
                if count > 0:     # (no edge, or no inlier on any edge: every information matrix is zero, nothing is optimised and mu is not read)
                    out[k] = float(preference) * float(threshold) ** 2 * count
        else:
            out = np.broadcast_to(np.asarray(mu, np.float64), (G,)).copy()
        if not (np.isfinite(out).all() and (out > 0).all()):
            raise ValueError("pose graph: mu must be > 0 and finite (mu <= 0: no line process is defined), got %r" % (out.tolist(),))
        return np.ascontiguousarray(out, np.float64)

    def pose_graph_optimize(self, graphs, constrained=True, mu=None, preference=1.0, threshold=0.02, max_solves=100):
        """Multiway registration (Open3D's global_optimization with its line process): per graph, one pose per node from the pairwise registration
        results on its edges, Levenberg-Marquardt to the end on the device, one workgroup per graph, one call for all graphs.
        graphs: a list of dict(poses [n, 4, 4] initial, i, j [m] node numbers, T [m, 4, 4] cloud i into frame j, info [m, 6, 6] the information matrix of
        evaluate_registration about c [m, 3] (in frame j), uncertain [m] bool: loop closures under the line process).  Node 0 is never moved; nodes that
        no chain of edges joins to node 0 keep their pose.  constrained: yaw + translation per node (every transform rotates about z only).
        mu: the line process's scale (a number or one per graph); None = preference * threshold^2 * the mean inlier count info[5, 5] of the graph's edges.
        Returns a list of dict(poses, before, after (the objective), solves, status (a POSE_GRAPH_STATUS name), chi2 [m], weights [m],
        pruned [m] = uncertain & (weights < 0.25))."""
        fn = self._register_fn("alignnet_pose_graph_optimize")
        graphs = list(graphs)
        if not graphs:
            return []
        if int(max_solves) < 1:
            raise ValueError("pose_graph_optimize: max_solves must be >= 1")
        node_off, edge_off, poses, edges, T, info, c, unc = self._pose_graph_arrays(graphs)
        mus = self._pose_graph_mu(graphs, info, edge_off, mu, preference, threshold)
        G, nodes, E = len(graphs), int(node_off[-1]), int(edge_off[-1])
        out, before, after = np.empty((nodes, 4, 4), np.float64), np.empty(G, np.float64), np.empty(G, np.float64)
        solves, status, chi2, w = np.empty(G, np.int32), np.empty(G, np.int32), np.empty(E, np.float64), np.empty(E, np.float64)
        dp, ip, lp = (lambda a: a.ctypes.data_as(C.POINTER(C.c_double))), (lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))), (lambda a: a.ctypes.data_as(C.POINTER(C.c_int64)))
        self._check(fn(self._h, G, lp(node_off), lp(edge_off), dp(poses), ip(edges), dp(T), dp(info), dp(c), ip(unc), dp(mus), 0 if constrained else 1,
                       int(max_solves), dp(out), dp(before), dp(after), ip(solves), ip(status), dp(chi2), dp(w)))
        res = []
        for k in range(G):
            ns, es = slice(node_off[k], node_off[k + 1]), slice(edge_off[k], edge_off[k + 1])
            res.append(dict(poses=out[ns].copy(), before=float(before[k]), after=float(after[k]), solves=int(solves[k]),
                            status=self.POSE_GRAPH_STATUS[status[k]], chi2=chi2[es].copy(), weights=w[es].copy(), mu=float(mus[k]),
                            pruned=(unc[es] != 0) & (w[es] < self.POSE_GRAPH_PRUNE)))
        return res

    def debug_pose_graph_system(self, graph, constrained=True, mu=None, preference=1.0, threshold=0.02):
        """Test hook: the kernel's own linearisation of ONE graph at its poses, no step taken: dict(r [m, d], chi2 [m], weights [m], F, H [N, N] dense,
        b [N]), d = 4 (constrained) or 6, N = d (n - 1)."""
        fn = self._register_fn("alignnet_debug_pose_graph_system")
        node_off, edge_off, poses, edges, T, info, c, unc = self._pose_graph_arrays([graph])
        mus = self._pose_graph_mu([graph], info, edge_off, mu, preference, threshold)
        n, m, d = int(node_off[1]), int(edge_off[1]), 4 if constrained else 6
        N = d * (n - 1)
        r, chi2, w, F = np.zeros((m, d)), np.zeros(m), np.zeros(m), C.c_double(0.0)
        H, b = np.zeros((N, N)), np.zeros(N)
        dp, ip = (lambda a: a.ctypes.data_as(C.POINTER(C.c_double))), (lambda a: a.ctypes.data_as(C.POINTER(C.c_int32)))
        self._check(fn(self._h, n, m, dp(poses), ip(edges), dp(T), dp(info), dp(c), ip(unc), float(mus[0]), 0 if constrained else 1, dp(r), dp(chi2), dp(w),
                       C.byref(F), dp(H), dp(b)))
        return dict(r=r, chi2=chi2, weights=w, F=float(F.value), H=H, b=b)

    # ---- spinning-LiDAR scene generator (csrc/alignnet_scene.hip; alignnet3d/scenes.py builds the arguments) ----
    def scene_upload_meshes(self, meshes, sensor=None):
        """meshes: list of (vertices [nv, 3] float64 normalised as scenes.normalise_mesh does, faces [nf, 3] int, centroid [3]); sensor: (dir_x [4500],
        dir_y [4500], dir_z [64]) direction tables, None = scenes.sensor_tables().  Copied to the device once."""
        from . import scenes
        dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
        sx, sy, sz = (np.ascontiguousarray(a, np.float64) for a in (scenes.sensor_tables() if sensor is None else sensor))
        assert sx.shape == (scenes.HRES,) and sy.shape == (scenes.HRES,) and sz.shape == (scenes.VRES,)
        self._check(self._lib.alignnet_scene_set_sensor(self._h, dp(sx), dp(sy), dp(sz)))
        M = len(meshes)
        off = np.zeros((M + 1, 2), np.int64)
        for m, (v, f, _) in enumerate(meshes):
            off[m + 1] = off[m] + (len(v), len(f))
        cat = lambda L, dt: np.ascontiguousarray(np.concatenate([np.asarray(x, dt).reshape(-1, 3) for x in L], 0)) if L else np.zeros((0, 3), dt)
        verts, faces = cat([m[0] for m in meshes], np.float64), cat([m[1] for m in meshes], np.int32)
        cen = np.ascontiguousarray(np.asarray([m[2] for m in meshes], np.float64).reshape(M, 3))
        self._check(self._lib.alignnet_scene_upload_meshes(self._h, dp(verts), faces.ctypes.data_as(C.POINTER(C.c_int32)),
                                                           off.ctypes.data_as(C.POINTER(C.c_int64)), dp(cen), M))

    def scene_free_meshes(self):
        self._check(self._lib.alignnet_scene_free_meshes(self._h))

    def scene_generate(self, mesh, scale, poses, scene_ids=None, seed=0, sigma=0.05, clip=0.05):
        """mesh [B] library indices, scale [B], poses [B, 2, 4] = x y z angle of the two clouds, scene_ids [B] (None = 0 .. B - 1).  sigma <= 0: no
        noise.  The clouds stay on the device (scene_read / scene_install_dataset); returns the offsets table [B + 1, 2]."""
        mesh = np.ascontiguousarray(mesh, np.int32).ravel()
        B = mesh.size
        scale = np.ascontiguousarray(scale, np.float64).ravel()
        poses = np.ascontiguousarray(poses, np.float64).reshape(B, 2, 4)
        assert scale.size == B
        ids = None if scene_ids is None else np.ascontiguousarray(scene_ids, np.int64).ravel()
        assert ids is None or ids.size == B
        off = np.zeros((B + 1, 2), np.int64)
        dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
        self._check(self._lib.alignnet_scene_generate(self._h, mesh.ctypes.data_as(C.POINTER(C.c_int32)), dp(scale), dp(poses),
                                                      None if ids is None else ids.ctypes.data_as(C.POINTER(C.c_int64)), B, int(seed) & (2 ** 64 - 1),
                                                      float(sigma), float(clip), off.ctypes.data_as(C.POINTER(C.c_int64))))
        self._scene_offsets = off
        return off

    def scene_read(self, offsets=None):
        """(points1, points2) float32 [n, 3] blobs of the last scene_generate (offsets: its return value, None = remembered)."""
        off = self._scene_offsets if offsets is None and hasattr(self, "_scene_offsets") else offsets
        n1, n2 = (0, 0) if off is None else (int(off[-1, 0]), int(off[-1, 1]))
        p1, p2 = np.empty((n1, 3), np.float32), np.empty((n2, 3), np.float32)
        self._check(self._lib.alignnet_scene_read(self._h, _fp(p1), _fp(p2)))
        return p1, p2

    def scene_install_dataset(self, labels):
        """The last scene_generate becomes the HBM-resident dataset (device to device); labels [B, 12] as for upload_dataset."""
        lab = np.ascontiguousarray(labels, np.float32).reshape(-1, 12)
        assert hasattr(self, "_scene_offsets") and lab.shape[0] == self._scene_offsets.shape[0] - 1, "one label row per generated scene"
        self._check(self._lib.alignnet_scene_install_dataset(self._h, _fp(lab)))
        self._dataset_sizes = np.diff(self._scene_offsets[:, 0])

    # ---- KITTI tracklet extraction (csrc/alignnet_crop.hip; alignnet3d/tracklets.py builds the arguments) ----
    def tracklet_upload_scans(self, scans):
        """scans: list of float32 arrays [n, 3] or [n, 4] (a KITTI .bin is [n, 4]: x y z reflectance), all of one width, or a tuple (points
        [sum n, stride], offsets [F + 1]) that is concatenated already.  Copied to the device once; frame f of tracklet_extract is scans[f]."""
        if isinstance(scans, tuple):
            pts, off = np.ascontiguousarray(scans[0], np.float32), np.ascontiguousarray(scans[1], np.int64).ravel()
            stride = pts.shape[1] if pts.ndim == 2 else 0
        else:
            arrs = [np.asarray(s, np.float32) for s in scans]
            widths = {a.shape[1] if a.ndim == 2 else 0 for a in arrs}
            stride = widths.pop() if len(widths) == 1 else (3 if not arrs else 0)
            off = np.zeros(len(arrs) + 1, np.int64)
            off[1:] = np.cumsum([len(a) for a in arrs])
            pts = np.ascontiguousarray(np.concatenate(arrs, 0)) if arrs and stride else np.zeros((0, max(stride, 1)), np.float32)
        self._check(self._lib.alignnet_tracklet_upload_scans(self._h, _fp(pts), int(stride), off.ctypes.data_as(C.POINTER(C.c_int64)), off.size - 1))
        self._tracklet_frames = off.size - 1

    def tracklet_free_scans(self):
        self._check(self._lib.alignnet_tracklet_free_scans(self._h))
        self._tracklet_frames = 0

    def tracklet_extract(self, frames, boxes, dz=None):
        """frames [B, 2] indices into the uploaded scans, boxes [B, 2, 7] float64 = (x, y, z, h, w, l, ry) of the KITTI label (camera frame),
        dz [B, 2] float32 subtracted from z (None = 0).  The crops stay on the device (tracklet_read / tracklet_install_dataset); returns the
        offsets table [B + 1, 2]."""
        frames = np.ascontiguousarray(frames, np.int32).reshape(-1, 2)
        B = frames.shape[0]
        boxes = np.ascontiguousarray(boxes, np.float64).reshape(B, 2, 7)
        dz = np.zeros((B, 2), np.float32) if dz is None else np.ascontiguousarray(dz, np.float32).reshape(B, 2)
        off = np.zeros((B + 1, 2), np.int64)
        self._check(self._lib.alignnet_tracklet_extract(self._h, frames.ctypes.data_as(C.POINTER(C.c_int32)), boxes.ctypes.data_as(C.POINTER(C.c_double)),
                                                        _fp(dz), B, off.ctypes.data_as(C.POINTER(C.c_int64))))
        self._tracklet_offsets = off
        return off

    def tracklet_extract_frustum(self, frames, rects, proj, image, dz=None, clip=2.0):
        """The image-frustum crop (the reference's from_bbox2d): frames [B, 2] as for tracklet_extract, rects [B, 2, 4] float64 = (xmin, ymin,
        xmax, ymax) in pixels, proj the velodyne-to-image matrix M (tracklets.projection) as [3, 4] or [12] for all uploaded frames or [F, 3, 4]
        one per frame, image = (W, H) or [F, 2], dz [B, 2] float32 (None = 0), clip the least x kept (exclusive).  A point is kept when its
        projection lies in the image and in the rectangle, both half-open.  The result replaces, and is read and installed like, a
        tracklet_extract's; returns the offsets table [B + 1, 2]."""
        fn = self._register_fn("alignnet_tracklet_extract_frustum")
        frames = np.ascontiguousarray(frames, np.int32).reshape(-1, 2)
        B, F = frames.shape[0], getattr(self, "_tracklet_frames", 0)
        rects = np.ascontiguousarray(rects, np.float64).reshape(B, 2, 4)
        dz = np.zeros((B, 2), np.float32) if dz is None else np.ascontiguousarray(dz, np.float32).reshape(B, 2)
        proj, image = np.asarray(proj, np.float64), np.asarray(image, np.float64)
        if proj.size == 12:
            proj = np.broadcast_to(proj.reshape(1, 12), (F, 12))
        elif proj.shape != (F, 3, 4) and proj.shape != (F, 12):
            raise ValueError("proj of shape %s: expected [3, 4], [12] or [%d, 3, 4] (one per uploaded frame)" % (proj.shape, F))
        if image.size == 2 and image.ndim == 1:
            image = np.broadcast_to(image.reshape(1, 2), (F, 2))
        elif image.shape != (F, 2):
            raise ValueError("image of shape %s: expected (W, H) or [%d, 2] (one per uploaded frame)" % (image.shape, F))
        proj, image = np.ascontiguousarray(proj).reshape(F, 12), np.ascontiguousarray(image).reshape(F, 2)
        off = np.zeros((B + 1, 2), np.int64)
        dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
        self._check(fn(self._h, frames.ctypes.data_as(C.POINTER(C.c_int32)), dp(rects), _fp(dz), B, dp(proj), dp(image), float(clip),
                       off.ctypes.data_as(C.POINTER(C.c_int64))))
        self._tracklet_offsets = off
        return off

    def tracklet_read(self, offsets=None):
        """(points1, points2) float32 [n, 3] blobs of the last tracklet_extract (offsets: its return value, None = remembered)."""
        off = self._tracklet_offsets if offsets is None and hasattr(self, "_tracklet_offsets") else offsets
        n1, n2 = (0, 0) if off is None else (int(off[-1, 0]), int(off[-1, 1]))
        p1, p2 = np.empty((n1, 3), np.float32), np.empty((n2, 3), np.float32)
        self._check(self._lib.alignnet_tracklet_read(self._h, _fp(p1), _fp(p2)))
        return p1, p2

    def tracklet_install_dataset(self, labels):
        """The last tracklet_extract becomes the HBM-resident dataset (device to device); labels [B, 12] as for upload_dataset."""
        lab = np.ascontiguousarray(labels, np.float32).reshape(-1, 12)
        assert hasattr(self, "_tracklet_offsets") and lab.shape[0] == self._tracklet_offsets.shape[0] - 1, "one label row per extracted pair"
        self._check(self._lib.alignnet_tracklet_install_dataset(self._h, _fp(lab)))
        self._dataset_sizes = np.diff(self._tracklet_offsets[:, 0])

    def debug_scene_cast(self, mesh, scale, pose, lds_triangles=0, binned=False, rows=False):
        """Test hook: ONE cloud by the shipped cast kernel, no noise.  Returns dict(t [64, 4500] float64 (inf = miss), triangle [64, 4500] (-1), window =
        (first column, columns), lds_triangles as used).  lds_triangles in 1 .. 512 forces several LDS chunks on small meshes.  binned=False: the scan;
        True: the binned cast (set_option("scene_cast", 1) selects it for scene_generate; this read-back takes it whatever the option says), and the
        dict also holds tile_counts [tiles of the window] (the length of every tile's triangle list) and entries (their sum).  rows=True: the
        chosen staging with its inner loop by elevation band (set_option("scene_rows", 1) selects that for scene_generate; again whatever the option
        says): the record (t, triangle, window, lds_triangles) plus cell_counts [tiles of the window, 8] (the staged triangles per tile and band of 8
        rows whose band bit was set) and cells (their sum)."""
        pose = np.ascontiguousarray(pose, np.float64).reshape(4)
        t, tri = np.empty(64 * 4500, np.float64), np.empty(64 * 4500, np.int32)
        win, used = np.zeros(2, np.int32), np.zeros(1, np.int32)
        ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))
        args = (self._h, int(mesh), float(scale), pose.ctypes.data_as(C.POINTER(C.c_double)), int(lds_triangles),
                t.ctypes.data_as(C.POINTER(C.c_double)), ip(tri), ip(win), ip(used))
        if rows:
            cell_counts, cells = np.zeros((563, 8), np.int32), C.c_int64(0)
            self._check(self._lib.alignnet_debug_scene_cast_rows(*args[:5], int(bool(binned)), ip(win), args[5], ip(tri), ip(used), ip(cell_counts),
                                                                 C.byref(cells)))
        elif binned:
            counts, entries = np.zeros(563, np.int32), C.c_int64(0)
            self._check(self._lib.alignnet_debug_scene_cast_binned(*args, ip(counts), C.byref(entries)))
        else:
            self._check(self._lib.alignnet_debug_scene_cast(*args))
        self.__dict__.pop("_scene_offsets", None)
        out = dict(t=t.reshape(64, 4500), triangle=tri.reshape(64, 4500), window=(int(win[0]), int(win[1])), lds_triangles=int(used[0]))
        if rows:
            out.update(cell_counts=cell_counts[:(int(win[1]) + 7) // 8].copy(), cells=int(cells.value))
        elif binned:
            out.update(tile_counts=counts[:(int(win[1]) + 7) // 8].copy(), entries=int(entries.value))
        return out

    @staticmethod
    def read_device(ptr, count, dtype=np.float32):
        """Debug / test helper: copy `count` elements from a device pointer (synchronous hipMemcpy)."""
        hip = C.CDLL("libamdhip64.so")
        out = np.empty(count, dtype)
        rc = hip.hipMemcpy(C.c_void_p(out.ctypes.data), C.c_void_p(ptr), C.c_size_t(out.nbytes), C.c_int(2))
        if rc != 0:
            raise EngineError("hipMemcpy device->host failed (%d)" % rc)
        return out

    def apply_gradients(self, grad_scale=1.0):
        self._check(self._lib.alignnet_apply_gradients(self._h, float(grad_scale)))

    def get_gradient(self, name):
        shp = dict((n, s) for n, s, _ in self.variables())[name]
        a = np.empty(shp[0] * shp[1], np.float32)
        self._check(self._lib.alignnet_get_grad(self._h, name.encode(), _fp(a), a.size))
        return a.reshape(shp) if shp[0] > 1 else a

    def debug_dropout_uniforms(self, B):
        """The uniforms the device-side dropout stream draws at the current step (layout of `dropout_u`): list of five
        [B, width] arrays [s1 tower0, s2 tower0, s1 tower1, s2 tower1, pair head]."""
        o = self.cfg["model"]["options"]
        w12, w3 = int(o["s1transformer"][1][0][-1]), int(o["remaining_transform_prediction"][0][-1])
        a = np.empty(B * (4 * w12 + w3), np.float32)
        self._check(self._lib.alignnet_debug_dropout_uniforms(self._h, B, _fp(a), a.size))
        return [a[i * B * w12:(i + 1) * B * w12].reshape(B, w12) for i in range(4)] + [a[4 * B * w12:].reshape(B, w3)]

    def debug_knn_graph(self, B):
        """The k = 20 neighbour graph the last eval-mode forward (of B pairs) built, dgcnn engines only: int32
        [2, B, num_points, 20] (tower, pair, point, neighbour rank; utils/tf_util_dgcnn.py:638-676)."""
        n = self.num_points
        a = np.empty((2, B, n, 20), np.int32)
        self._check(self._lib.alignnet_debug_knn_graph(self._h, a.ctypes.data_as(C.POINTER(C.c_int32)), a.size))
        return a

    def debug_train_decisions(self, B, relu=False):
        """What the last training forward (of B pairs) decided -- the graph's discontinuous choices, for decision-pinned parity tests
        (include/alignnet_hip.h: alignnet_debug_train_decisions).  dict: "yaw" int32 [2, B]; "pool" list over the three stages of
        [2, B, C_last]; dgcnn engines also "slot" list of [2, B, N, C_edge] and "knn" [2, B, N, 20].  Tower outermost.
        relu=True adds "relu": the sign every relu of that step saw (alignnet_debug_train_relu_mask), keyed as oracle/alignnet_torch.py keys
        its layers -- "<tower>:<scope>/conv<l>" bool [B*N(*k), C] (the conv in front of a max: at the winner), "<tower>:<scope>/fc<j>" [B, C],
        "p:fc<j>" for the pair head.  Call it right after train_forward_backward (the masks of recomputed layers are rebuilt from the
        step's parameters and statistics)."""
        o, n = self.cfg["model"]["options"], self.num_points
        convs = [list(o["s1transformer"][0]), list(o["s2transformer"][0]), list(o["embedding"])]
        ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))

        def get(kind, stage, shape):
            a = np.empty(shape, np.int32)
            self._check(self._lib.alignnet_debug_train_decisions(self._h, kind, stage, ip(a), a.size))
            return a
        out = {"yaw": get(0, 0, (2, B)), "pool": [get(1, s, (2, B, convs[s][-1])) for s in range(3)]}
        if self.cfg["model"]["backbone"] == "dgcnn":
            out["slot"] = [get(2, s, (2, B, n, convs[s][-2])) for s in range(3)]
            out["knn"] = get(3, 0, (2, B, n, 20))
        if relu:
            out["relu"] = self.debug_train_relu_masks(B)
            # (with the signs: the classes of the loss's target angles, models/tp8.py:193-199 -- [2, B] per tower term, [2, B, B] for the pair term)
            out["loss_cls"] = [get(4, 0, (2, B)), get(4, 1, (2, B)), get(4, 2, (2, B, B))]
        return out

    def debug_loss(self, o2, s1c, o3, labels, num_bins, accept_inverted=True, early_stage_factor=0.5, angle_factor=1.0, want_grad=True,
                   want_classes=True):
        """The loss kernels alone on given head outputs (include/alignnet_hip.h: alignnet_debug_loss): o2 [2B, 3 + 2 nb], s1c [2B, 3], o3 [B, 3 + 2 nb],
        towers outermost; labels as for eval_loss.  Nothing of the engine's own configuration or state enters.  dict: "out" [17] (loss, 16 summaries),
        "s2c" [2B, 3], "theta" [2B], "pcls" int32 [2B]; want_classes: "cls" = [[2, B], [2, B], [2, B, B]] (tower 1, tower 2, pair); want_grad:
        "d_s1c", "d_s2c", "d_o2", "d_o3" as the loss kernels leave them, in front of the glue backward."""
        nb = int(num_bins)
        ld = 3 + 2 * nb
        o3 = np.ascontiguousarray(o3, np.float32)
        B = o3.shape[0] if o3.ndim == 2 else 0
        o2, s1c = np.ascontiguousarray(o2, np.float32), np.ascontiguousarray(s1c, np.float32)
        if B >= 1 and nb >= 1 and (o2.shape != (2 * B, ld) or s1c.shape != (2 * B, 3) or o3.shape != (B, ld)):
            raise ValueError(f"debug_loss: o2 {o2.shape}, s1c {s1c.shape}, o3 {o3.shape} do not fit B = {B}, num_bins = {nb}")
        n = max(B, 0)
        keep, L = self._labels(labels, n)
        ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))
        res = {"out": np.empty(17, np.float32), "s2c": np.empty((2 * n, 3), np.float32), "theta": np.empty(2 * n, np.float32), "pcls": np.empty(2 * n, np.int32)}
        cls = [np.empty((2, n), np.int32), np.empty((2, n), np.int32), np.empty((2, n, n), np.int32)] if want_classes else None
        grads = {k: np.empty((2 * n, w), np.float32) for k, w in (("d_s1c", 3), ("d_s2c", 3), ("d_o2", ld))} if want_grad else {}
        if want_grad:
            grads["d_o3"] = np.empty((n, ld), np.float32)
        gp = [_fp(grads[k]) if want_grad else None for k in ("d_s1c", "d_s2c", "d_o2", "d_o3")]
        cp = [ip(c) if want_classes else None for c in (cls or [None] * 3)]
        self._check(self._lib.alignnet_debug_loss(self._h, B, nb, int(bool(accept_inverted)), float(early_stage_factor), float(angle_factor), int(bool(want_grad)),
                                                  _fp(o2), _fp(s1c), _fp(o3), C.byref(L), _fp(res["out"]), _fp(res["s2c"]), _fp(res["theta"]), ip(res["pcls"]),
                                                  cp[0], cp[1], cp[2], gp[0], gp[1], gp[2], gp[3]))
        if want_classes:
            res["cls"] = cls
        res.update(grads)
        return res

    def debug_train_rounded(self, B):
        """bf16 step, fused PointNet stages: the bf16-rounded h1 / h2 the step's MFMA convs multiplied (alignnet_debug_train_rounded), keyed like the relu masks
        by the conv layer that CONSUMES them: "<tower>:<scope>/conv2" -> h1 as float32 [B*N, C1], "<tower>:<scope>/conv3" -> h2 [B*N, C2]."""
        o, n = self.cfg["model"]["options"], self.num_points
        convs = [list(o["s1transformer"][0]), list(o["s2transformer"][0]), list(o["embedding"])]
        scopes = ["transformer1/embedding", "transformer2/embedding", "embedding"]
        out = {}
        dg = self.cfg["model"]["backbone"] == "dgcnn"
        for s in range(3):
            for l in range(2):
                a = np.empty((2, B * n * (20 if dg and l == 0 else 1), convs[s][l]), np.uint16)
                self._check(self._lib.alignnet_debug_train_rounded(self._h, s, l, a.ctypes.data_as(C.POINTER(C.c_uint16)), a.size))
                f = (a.astype(np.uint32) << 16).view(np.float32)
                for t in range(2):
                    out[f"{t}:{scopes[s]}/conv{l + 2}"] = f[t]
        return out

    def debug_train_relu_masks(self, B):
        o, n = self.cfg["model"]["options"], self.num_points
        dg = self.cfg["model"]["backbone"] == "dgcnn"
        convs = [list(o["s1transformer"][0]), list(o["s2transformer"][0]), list(o["embedding"])]
        fcs = [list(o["s1transformer"][1][0]), list(o["s2transformer"][1][0]), list(o["remaining_transform_prediction"][0])]
        scopes = ["transformer1/embedding", "transformer2/embedding", "embedding"]
        heads = ["transformer1/mlp/", "transformer2/mlp/", ""]

        def get(kind, stage, layer, shape):
            a = np.empty(shape, np.uint8)
            self._check(self._lib.alignnet_debug_train_relu_mask(self._h, kind, stage, layer, a.ctypes.data_as(C.POINTER(C.c_uint8)), a.size))
            return a.astype(bool)
        out = {}
        for s in range(3):
            nl = len(convs[s])
            for l, c in enumerate(convs[s]):
                if l == nl - 1:
                    shape = (2, B, c)                 # at the winning point
                elif dg and l == nl - 2:
                    shape = (2, B * n, c)             # at the winning neighbour slot
                else:
                    shape = (2, B * n * (20 if dg else 1), c)
                m = get(0, s, l, shape)
                for t in range(2):
                    out[f"{t}:{scopes[s]}/conv{l + 1}"] = m[t]
            for j, c in enumerate(fcs[s]):
                if s < 2:
                    m = get(1, s, j, (2, B, c))
                    for t in range(2):
                        out[f"{t}:{heads[s]}fc{j + 1}"] = m[t]
                else:
                    out[f"p:fc{j + 1}"] = get(1, s, j, (B, c))
        return out

    def grad_buffer(self):
        ptr, n = C.c_void_p(), C.c_size_t()
        self._check(self._lib.alignnet_grad_buffer(self._h, C.byref(ptr), C.byref(n)))
        return ptr.value, n.value

    # ---- multi-GPU (RCCL over xGMI) ---------------------------------------------
    @staticmethod
    def comm_unique_id():
        buf = (C.c_uint8 * 128)()
        if _capi.load_library().alignnet_comm_unique_id(buf) != 0:
            raise EngineError("alignnet_comm_unique_id failed (librccl not loadable?)")
        return bytes(buf)

    @staticmethod
    def comm_loopback_id():
        """Id of a new in-process loopback group: `world` engines of this process on one device, one host thread each
        (include/alignnet_hip.h: alignnet_comm_loopback_id) -- the multi-rank paths on a 1-GPU box."""
        buf = (C.c_uint8 * 128)()
        if _capi.load_library().alignnet_comm_loopback_id(buf) != 0:
            raise EngineError("alignnet_comm_loopback_id failed")
        return bytes(buf)

    def comm_init(self, rank, world, unique_id):
        buf = (C.c_uint8 * 128).from_buffer_copy(unique_id)
        self._check(self._lib.alignnet_comm_init(self._h, rank, world, buf))

    def comm_init_grad(self, rank, world, unique_id):
        """A second communicator of the same ranks for the gradient buckets alone (include/alignnet_hip.h: alignnet_comm_init_grad)."""
        buf = (C.c_uint8 * 128).from_buffer_copy(unique_id)
        self._check(self._lib.alignnet_comm_init_grad(self._h, rank, world, buf))

    def comm_allreduce_grads(self):
        self._check(self._lib.alignnet_comm_allreduce_grads(self._h))

    def comm_average_shadows(self):
        """Average the BatchNorm EMA shadows over the ranks of the engine's communicator (one all-reduce on the device)."""
        self._check(self._lib.alignnet_comm_average_shadows(self._h))

    # ---- checkpoints (tf.train.Saver, train.py:220,252,268,281,317,321) -----------
    def save(self, path):
        self._check(self._lib.alignnet_save(self._h, str(path).encode()))

    def load(self, path, skip_step=False):
        self._check(self._lib.alignnet_load(self._h, str(path).encode(), int(skip_step)))

    # ---- state -----------------------------------------------------------------
    def state(self):
        st = _capi.State()
        self._check(self._lib.alignnet_get_state(self._h, C.byref(st)))
        return dict(step=st.step, learning_rate=st.learning_rate, bn_decay=st.bn_decay)

    def set_step(self, step):
        self._check(self._lib.alignnet_set_step(self._h, int(step)))

    # ---- profiling hook ----------------------------------------------------------
    def set_option(self, key, value):
        """Run-time options outside the reference's config surface (include/alignnet_hip.h: alignnet_set_option)."""
        self._check(self._lib.alignnet_set_option(self._h, key.encode(), int(value)))

    def get_option(self, key):
        v = C.c_int64(0)
        self._check(self._lib.alignnet_get_option(self._h, key.encode(), C.byref(v)))
        return int(v.value)

    def last_backbone_kernel(self):
        """Name of the backbone kernel instantiation the most recent eval forward launched."""
        return KERNEL_NAMES.get(self.get_option("last_backbone_kernel"), "none")

    def last_backbone_wg_waves(self):
        """Waves per workgroup of that launch: the shipped shape runs as four-wave workgroups, two per CU, on grids that fill the
        chip twice over, as eight-wave ones below (set_option("infer_wg_waves", 0 / 4 / 8)); both report the same kernel name."""
        return self.get_option("last_backbone_wg_waves")

    def profile_enable(self, on=True):
        self._check(self._lib.alignnet_profile_enable(self._h, int(on)))

    PROFILED_KERNELS = ("backbone", "knn", "train_fwd_phase2", "train_fwd_phase3", "train_gram_h2", "train_bwd_b2", "train_bwd_b1",
                        "dg_train_fwd", "dg_train_bwd_edge", "allreduce", "optimizer", "scene_window", "scene_cast", "scene_compact",
                        "icp_grid_build", "icp_grid", "scene_bin", "icp_plane_normals", "icp_plane", "scene_band",
                        "tracklet_test", "tracklet_compact", "icp_generalized_normals", "icp_generalized", "pose_graph", "icp_pyramid")

    def profile_kernels(self):
        """{kernel: (ms, launches)} accumulated since the last profile_read(reset=True); call BEFORE that reset."""
        out = {}
        for k in self.PROFILED_KERNELS:
            ms, n = C.c_double(), C.c_int64()
            self._check(self._lib.alignnet_profile_read_kernel(self._h, k.encode(), C.byref(ms), C.byref(n)))
            if n.value:
                out[k] = (ms.value, n.value)
        return out

    def profile_read(self, reset=True):
        ms, n, tot = C.c_double(), C.c_int64(), C.c_double()
        self._check(self._lib.alignnet_profile_read(self._h, C.byref(ms), C.byref(n), C.byref(tot), int(reset)))
        return dict(backbone_ms=ms.value, backbone_launches=n.value, total_ms=tot.value)
