"""GPU: the row-serial last layer of pointnet_fused<128, 68, 132, 16> (csrc/kernels_infer.h rowserial_chain: a channel tile's row tiles one after
the other, the weight image in registers, the epilogue under the next chain) against the weight-stream schedule it replaced
("ab_last_layer_stream" = 1).  Per (row, column) both accumulate the same products in ascending k and take a max over the same values, so all
eight outputs must agree bit for bit, on the smallest shapes at which the new loop takes another path.  "infer_tile_points" is set to 128
throughout: small batches otherwise pick the 64-point kernel and nothing would be compared.  One case goes to the fp64 oracle as well, so the old
kernel is not the only witness."""
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


def _forward(cfg, d, stream, options=(), twice=False):
    spec, P32 = _params(cfg)
    eng = alignnet3d.Engine(cfg)
    eng.set_variables(P32)
    eng.set_option("infer_tile_points", 128)
    for k, v in options:
        eng.set_option(k, v)
    eng.set_option("ab_last_layer_stream", int(stream))
    assert eng.get_option("ab_last_layer_stream") == int(stream)
    out = eng.forward(d["pcs1"], d["pcs2"])
    assert eng.last_backbone_kernel() == KERNEL, eng.last_backbone_kernel()
    if twice:   # the resident weight image and the pooled registers start over: the same bits again
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
    new = _forward(cfg, d, False, options, twice)
    old = _forward(cfg, d, True, options)
    _same(new, old, "row-serial vs stream %s" % (options,))
    return new


def test_stream_key_sets_its_mask_bit_and_nothing_else(gpu_required):
    from tests.helpers import small_cfg
    eng = alignnet3d.Engine(small_cfg())
    others = ("infer_tile_points", "ab_tiles_per_wg", "infer_matmul_bf16x3", "ab_no_ld_const", "ab_infer_tile64")
    before = {k: eng.get_option(k) for k in others}
    assert eng.get_option("ab_mask") == 0 and eng.get_option("ab_last_layer_stream") == 0
    eng.set_option("ab_last_layer_stream", 1)
    assert eng.get_option("ab_mask") == 1 << 14 and eng.get_option("ab_last_layer_stream") == 1
    assert {k: eng.get_option(k) for k in others} == before
    eng.set_option("ab_last_layer_stream", 0)
    assert eng.get_option("ab_mask") == 0
    eng.close()


def test_one_tile_one_workgroup_per_cloud(gpu_required):
    """N = 128, B = 1: no next-tile reload, only the exposed final epilogue per channel tile walk."""
    _both(_cfg(128), R.synth_pairs(1, 128, seed=3, dtype=np.float32), twice=True)


@pytest.mark.parametrize("N", [256, 1024])
def test_tile_walk_and_one_tile_per_workgroup(gpu_required, N):
    """The workgroup walks all tiles of its cloud (weights reloaded across the point-tile boundary, the pooled maximum carried in registers) and,
    on the same clouds, one tile per workgroup (merged through atomicMax): four runs, one set of bits."""
    cfg, d = _cfg(N), R.synth_pairs(2, N, seed=11, dtype=np.float32)
    walk = _both(cfg, d, (("ab_tiles_per_wg", N // 128),), twice=(N == 256))
    single = _both(cfg, d, (("ab_tiles_per_wg", 1),))
    _same(walk, single, "walk vs one tile per workgroup")


def test_ragged_last_tile(gpu_required):
    """N = 200, B = 3: the second tile's tail rows repeat the last point."""
    cfg, d = _cfg(200), R.synth_pairs(3, 200, seed=5, dtype=np.float32)
    _same(_both(cfg, d, (("ab_tiles_per_wg", 2),)), _both(cfg, d, (("ab_tiles_per_wg", 1),)), "walk vs one tile per workgroup")


@pytest.mark.parametrize("c3", [288,     # 9 channel tiles: wave 0 owns two, the rest one
                                1000,    # masked partial last channel tile
                                1056])   # 33 channel tiles: wave 0's fifth goes through the per-tile publish path
def test_embedding_width(gpu_required, c3):
    cfg, d = _cfg(256, c3), R.synth_pairs(2, 256, seed=7, dtype=np.float32)
    _both(cfg, d, (("ab_tiles_per_wg", 2),), twice=(c3 == 1056))
    _both(cfg, d, (("ab_tiles_per_wg", 1),))


def test_tile_shapes_stay_bit_identical(gpu_required):
    """The 64-point kernel (untouched, weight stream) against the 128-point one, default dispatch."""
    cfg, d = _cfg(200), R.synth_pairs(3, 200, seed=5, dtype=np.float32)
    spec, P32 = _params(cfg)
    outs = {}
    for tile in (64, 128):
        eng = alignnet3d.Engine(cfg)
        eng.set_variables(P32)
        eng.set_option("infer_tile_points", tile)
        outs[tile] = eng.forward(d["pcs1"], d["pcs2"])
        eng.close()
    _same(outs[128], outs[64], "128- vs 64-point tiles")


def test_shipped_config_against_the_oracle(gpu_required):
    """The three stages of the shipped config (C3 = 256 / 512 / 1024: 1 / 2 / 4 channel tiles per wave) against the fp64 oracle, at the bar the forward
    tests use."""
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
