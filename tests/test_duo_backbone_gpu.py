"""GPU: the four-wave form of the shipped-shape PointNet backbone (csrc/kernels_infer.h pointnet_fused_duo<128, 132, 16>: two independent
workgroups per CU, lift and hidden layer in place on a wave's own 32 rows, the row-serial last layer over four waves with eight pool registers)
against the eight-wave kernel pointnet_fused<128, 68, 132, 16> ("infer_wg_waves" = 4 against 8).  Per (row, column) both accumulate the same
products in ascending k from zero, the lift keeps its expression and the max runs over the same values, so all eight outputs must agree bit
for bit, on the smallest shapes at which the new kernel takes another path.  "infer_tile_points" is 128 throughout: small batches otherwise
pick the 64-point kernel and nothing would be compared.  One case goes to the fp64 oracle as well, so the old kernel is not the only witness."""
import numpy as np
import pytest

import alignnet3d
from oracle import alignnet_ref as R
from tests.helpers import oracle_params, compare_forward, compare_forward_all

pytestmark = pytest.mark.gpu

KERNEL = "pointnet_fused<64,128,k16>"
_PARAMS = {}


def _cfg(N, c3=1024):
    cfg = alignnet3d.default_model_config()
    cfg["model"]["num_points"] = N
    cfg["model"]["options"]["embedding"] = [64, 128, c3]
    return cfg


def _params(cfg):
    key = (cfg["model"]["num_points"], tuple(cfg["model"]["options"]["embedding"]))
    if key not in _PARAMS:
        _PARAMS[key] = oracle_params(cfg)
    return _PARAMS[key]


def _engine(cfg, options=()):
    spec, P32 = _params(cfg)
    eng = alignnet3d.Engine(cfg)
    eng.set_variables(P32)
    eng.set_option("infer_tile_points", 128)
    for k, v in options:
        eng.set_option(k, v)
    return eng


def _forward(cfg, d, waves, options=(), twice=False):
    eng = _engine(cfg, tuple(options) + (("infer_wg_waves", waves),))
    assert eng.get_option("infer_wg_waves") == waves
    out = eng.forward(d["pcs1"], d["pcs2"])
    assert eng.last_backbone_kernel() == KERNEL, eng.last_backbone_kernel()
    assert eng.get_option("last_backbone_wg_waves") == waves
    if twice:   # the resident weight images and the pool registers start over: the same bits again
        again = eng.forward(d["pcs1"], d["pcs2"])
        for k in out:
            np.testing.assert_array_equal(again[k], out[k], err_msg="second forward: " + k)
    eng.close()
    return out


def _same(a, b, what):
    assert len(a) == 8 and sorted(a) == sorted(b)
    for k in a:
        assert np.array_equal(a[k], b[k]), (what, k, float(np.abs(a[k].astype(np.float64) - b[k]).max()))


def _both(cfg, d, options=(), twice=False):
    new = _forward(cfg, d, 4, options, twice)
    old = _forward(cfg, d, 8, options)
    _same(new, old, "four- vs eight-wave workgroups %s" % (options,))
    return new


def test_one_tile_one_workgroup_per_cloud(gpu_required):
    """N = 128, B = 1: one tile, no reload of the last layer's image; the forward runs twice."""
    _both(_cfg(128), R.synth_pairs(1, 128, seed=3, dtype=np.float32), twice=True)


def test_tile_walk_and_one_tile_per_workgroup(gpu_required):
    """N = 256, B = 2: the workgroup walks both tiles of its cloud (both weight images re-requested across the tile boundary, the pooled maximum
    carried in registers) and, on the same clouds, one tile per workgroup (merged through atomicMax): four runs, one set of bits."""
    cfg, d = _cfg(256), R.synth_pairs(2, 256, seed=11, dtype=np.float32)
    walk = _both(cfg, d, (("ab_tiles_per_wg", 2),))
    single = _both(cfg, d, (("ab_tiles_per_wg", 1),))
    _same(walk, single, "walk vs one tile per workgroup")


def test_full_walk_fills_the_eight_pool_registers(gpu_required):
    """N = 1024, B = 2: eight tiles per workgroup, and at C3 = 1024 eight channel tiles per wave -- every pool register in use."""
    cfg, d = _cfg(1024), R.synth_pairs(2, 1024, seed=11, dtype=np.float32)
    _both(cfg, d, (("ab_tiles_per_wg", 8),))


def test_ragged_last_tile(gpu_required):
    """N = 200, B = 3: the second tile's tail rows repeat the last point."""
    cfg, d = _cfg(200), R.synth_pairs(3, 200, seed=5, dtype=np.float32)
    _same(_both(cfg, d, (("ab_tiles_per_wg", 2),)), _both(cfg, d, (("ab_tiles_per_wg", 1),)), "walk vs one tile per workgroup")


@pytest.mark.parametrize("c3", [288,     # 9 channel tiles: wave 0 owns three, the rest two
                                1000,    # masked partial last channel tile
                                1056])   # 33 channel tiles: wave 0's ninth goes through the per-tile publish path
def test_embedding_width(gpu_required, c3):
    cfg, d = _cfg(256, c3), R.synth_pairs(2, 256, seed=7, dtype=np.float32)
    _both(cfg, d, (("ab_tiles_per_wg", 2),), twice=(c3 == 1056))
    _both(cfg, d, (("ab_tiles_per_wg", 1),))


def test_shipped_config_against_the_oracle(gpu_required):
    """The three stages of the shipped config (C3 = 256 / 512 / 1024: 2 / 4 / 8 channel tiles per wave) against the fp64 oracle, at the bars of
    tests/test_last_layer_schedule_gpu.py::test_shipped_config_against_the_oracle, on the same inputs."""
    cfg, B = _cfg(256), 4
    spec, P32 = _params(cfg)
    d = R.synth_pairs(B, 256, seed=1234, dtype=np.float32)
    ep = _both(cfg, d)
    ref, _, aux = R.get_model({k: v.astype(np.float64) for k, v in P32.items()}, spec, d["pcs1"].astype(np.float64), d["pcs2"].astype(np.float64))
    worst, unstable = compare_forward(ep, ref, spec.num_bins)
    print("worst abs err", worst, "unstable pairs", unstable)
    assert unstable <= 1
    worst, pinned, left_out = compare_forward_all(ep, ref, aux, P32, spec, d["pcs1"], d["pcs2"])   # every pair, the oracle pinned to the engine's yaw class where they differ
    print("ALL %d pairs: %d pinned to the engine's yaw class, left out %s, worst abs err %s" % (B, pinned, left_out, worst))
    assert left_out == []


def _waves_after_forward(cfg, B, options=()):
    N = cfg["model"]["num_points"]
    d = R.synth_pairs(B, N, seed=2, dtype=np.float32)
    eng = _engine(cfg, options)
    eng.forward(d["pcs1"], d["pcs2"])
    assert eng.last_backbone_kernel() == KERNEL, eng.last_backbone_kernel()
    got = eng.get_option("last_backbone_wg_waves"), eng.get_option("backbone_wgs_per_cu")
    eng.close()
    return got


def test_automatic_dispatch_follows_the_grid(gpu_required):
    """N = 128: B = 256 is 512 one-tile workgroups, two for every CU -- four waves, and the runtime places two of them on a CU; B = 2 is four
    workgroups -- eight waves."""
    cfg = _cfg(128)
    assert _waves_after_forward(cfg, 256) == (4, 2)
    assert _waves_after_forward(cfg, 2)[0] == 8


@pytest.mark.parametrize("waves", [0, 4, 8])
def test_stream_schedule_keeps_eight_waves(gpu_required, waves):
    cfg = _cfg(128)
    assert _waves_after_forward(cfg, 256, (("infer_wg_waves", waves), ("ab_last_layer_stream", 1)))[0] == 8


def test_wg_waves_key_changes_nothing_else(gpu_required):
    from tests.helpers import small_cfg
    eng = alignnet3d.Engine(small_cfg())
    others = ("infer_tile_points", "ab_tiles_per_wg", "infer_matmul_bf16x3", "ab_mask", "ab_last_layer_stream", "ab_no_ld_const", "ab_infer_tile64")
    before = {k: eng.get_option(k) for k in others}
    assert before["ab_mask"] == 0 and eng.get_option("infer_wg_waves") == 0
    for v in (4, 8, 0):
        eng.set_option("infer_wg_waves", v)
        assert eng.get_option("infer_wg_waves") == v
        assert {k: eng.get_option(k) for k in others} == before
    with pytest.raises(alignnet3d.EngineError):
        eng.set_option("infer_wg_waves", 2)
    assert eng.get_option("infer_wg_waves") == 0
    eng.close()
