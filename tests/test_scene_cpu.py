"""CPU: the host side of the scene generator (alignnet3d/scenes.py, make_synth_dataset.py's writer) against the reference's recorded
draws (tests/golden/scene_vectors.*, made by tests/golden/make_scene_golden.py), and the restatement (tests/scene_ref.py) on every input
the GPU tests use: it must find no undecided ray on any of them."""
import json
import os
import re
import sys

import numpy as np
import pytest

from alignnet3d import scenes as S
from tests import scene_cases as C
from tests import scene_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "alignnet-3d_amd")
GOLD = os.path.join(ROOT, "tests", "golden")


def _golden():
    return np.load(os.path.join(GOLD, "scene_vectors.npz")), json.load(open(os.path.join(GOLD, "scene_vectors.json")))


def test_sensor_tables_match_the_reference():
    z, _ = _golden()
    got = S.ray_directions(z["ray_rows"])
    np.testing.assert_allclose(got, z["ray_directions"], rtol=1e-12, atol=1e-12 * 120)
    assert z["ray_rows"][0] == 0 and z["ray_rows"][-1] == 64 * 4500 - 1 and len(z["ray_rows"]) >= 289
    # the restatement casts the very same rays
    for a, b in zip(S.sensor_tables(), R.sensor_tables()):
        assert np.array_equal(a, b)
    assert not np.any(S.sensor_tables()[2] == 0)      # no row looks along the horizon: a face at sensor height is never edge-on to a row


def test_scene_draws_match_the_reference_bit_for_bit():
    z, meta = _golden()
    assert len(meta["scenes"]) == 120
    seen = set()
    for i, info in enumerate(meta["scenes"]):
        s = S.draw_scene(info["seed"], info["kind"], second_object_set=info["second_object_set"], cats=meta["cats"])
        t = s.transform
        assert (s.cat, s.mesh_id) == (info["cat"], info["mesh_id"]), info
        assert np.array_equal(z["scalars"][i], [s.mesh_scale, t.start_angle, t.end_angle, t.rel_angle, t.angle, t.velocity]), info
        for f in ("start_position", "end_position", "translation"):
            assert np.array_equal(z[f][i], getattr(t, f)), (info, f)
        for f in ("transform_start", "transform_end", "rel_transform"):   # (the reference builds the rotation with scipy: equal up to the last bit)
            np.testing.assert_allclose(getattr(t, f), z[f][i], rtol=0, atol=1e-15, err_msg=str(info))
        seen.add(s.cat)
    assert {"car", "person"} <= seen and seen & set(meta["cats"])
    # the draw the issue quotes
    s = S.draw_scene(3, "carspersons")
    assert (s.cat, s.mesh_id, s.mesh_scale) == ("car", 24, 6.0)
    np.testing.assert_allclose(s.transform.start_position, [-1.627, 4.172, 0], atol=1e-3)


def test_off_reader():
    text = "OFF4 2 0\n# a comment\n0 0 0\n1 0 0  # trailing\n\n1 1 0\n0 1 0.5\n4 0 1 2 3\n5 0 1 2 3 1\n"
    v, f = S.read_off(text)
    assert v.shape == (4, 3) and v[3, 2] == 0.5
    assert f.tolist() == [[0, 1, 2], [0, 2, 3], [0, 1, 2], [0, 2, 3], [0, 3, 1]]      # a quad = 2, a pentagon = 3 triangles, fans
    v2, f2 = S.read_off("OFF\n3 1 0\n0 0 0\n1 0 0\n0 1 0\n3 0 1 2\n")
    assert v2.shape == (3, 3) and f2.tolist() == [[0, 1, 2]]
    with pytest.raises(ValueError):
        S.read_off("OFF\n3 1 0\n0 0 0\n1 0 0\n0 1 0\n3 0 1 7\n")
    with pytest.raises(ValueError):
        S.read_off("PLY\n1 2 3\n")
    for cat in ("car", "person"):
        v, f = S.builtin_mesh(cat)
        rv, rf = S.read_off(S.write_off(v, f))
        assert np.array_equal(rv, v) and np.array_equal(rf, f)


def test_normalise_mesh_is_the_three_line_definition():
    rng = np.random.default_rng(4)
    v = rng.normal(size=(50, 3)) * [3, 1, 0.5] + [10, -4, 2]
    bounds = np.stack([v.min(0), v.max(0)])
    w = v - np.mean(bounds, axis=0)
    bounds = np.stack([w.min(0), w.max(0)])
    w = w * (1.0 / (np.max(np.abs(bounds)) * 2.0))
    got = S.normalise_mesh(v)
    assert np.array_equal(got, w)
    assert abs(np.abs(got).max() - 0.5) < 1e-15 and np.allclose(got.min(0) + got.max(0), 0, atol=1e-15)
    # the centroid the engine is given is the area-weighted one
    cv, cf = C.car()
    assert np.allclose(S.mesh_centroid(cv, cf), R.posed_centroid(cv, cf), atol=1e-15)
    assert np.array_equal(S.mesh_centroid(cv[:3], np.array([[0, 0, 1]])), cv[:3].mean(0))    # no area: the mean of the vertices


@pytest.mark.parametrize("name", sorted(C.CASES))
def test_restatement_finds_no_undecided_ray(name):
    """Every input of tests/test_scene_gpu.py: dilated and eroded casts agree on every ray of the window."""
    r = C.reference(name)
    assert len(r["undecided"]) == 0, (name, r["undecided"][:10])
    assert np.all(np.diff(r["rays"]) > 0)
    v, f, scale, pose = C.CASES[name]
    # the window holds every hit the whole sensor would see: cast the columns next to it as well
    first, count = r["window"]
    if 0 < count < R.HRES:
        outside = np.array([(first - 1) % R.HRES, (first - 2) % R.HRES, (first + count) % R.HRES, (first + count + 1) % R.HRES])
        assert not np.isfinite(R.cast(r["posed"], f, outside)["t_dilated"]).any()


def test_restatement_batch_inputs_have_no_undecided_ray():
    for k in range(len(C.BATCH)):
        for c in C.batch_reference(k):
            assert len(c["undecided"]) == 0, k
    assert len(C.batch_reference(2)[1]["rays"]) == 0 and C.batch_reference(2)[0]["window"][0] + C.batch_reference(2)[0]["window"][1] > R.HRES


def test_restatement_edge_semantics():
    assert len(C.reference("empty")["rays"]) == 0 and C.reference("empty")["window"] == (0, 0)
    assert len(C.reference("above")["rays"]) == 0 and C.reference("above")["window"][1] > 0
    assert C.reference("over_sensor")["window"] == (0, R.HRES) and len(C.reference("over_sensor")["rays"]) == 64 * R.HRES
    for name in ("wrap_plus180", "wrap_minus180"):
        first, count = C.reference(name)["window"]
        assert first + count > R.HRES and len(C.reference(name)["rays"]) > 1000
    # a duplicated face changes nothing but the triangle ids; the zero-area faces (ids 0, 1, 2) are never reported
    dup, zero = C.reference("duplicate"), C.reference("zero_area")
    assert np.isfinite(dup["cast"]["t"]).sum() > 5000
    tri = zero["cast"]["triangle"]
    assert tri.max() > 2 and not np.isin(tri, [0, 1, 2]).any()
    # the edge-on faces are hit by no ray along their plane; the face behind them is
    e = C.reference("edge_on")
    assert set(np.unique(e["cast"]["triangle"])) >= {-1, 2}


@pytest.mark.parametrize("cat,scale,yaw", [("car", 4.0, np.deg2rad(65.0)), ("person", 1.8, 0.3)])
def test_builtin_meshes_give_a_plausible_scan(cat, scale, yaw):
    """Built-ins at the size of a small car (4 m, end-on) and of a person (1.8 m) from 8 m: closed, not convex, some hundred triangles, 200 - 5000 hits."""
    v, f, cen = S.load_mesh("builtin", cat, 1)
    assert 100 <= len(f) <= 1000
    edges = {}
    for a, b, c in f:
        for e in ((a, b), (b, c), (c, a)):
            edges[e] = edges.get(e, 0) + 1
    assert all(edges.get((b, a), 0) == n for (a, b), n in edges.items())      # every edge is shared by two faces of opposite sense
    r = R.cloud(v, f, scale, C.polar(8.0, 25.0, yaw=yaw))
    assert 200 <= len(r["rays"]) <= 5000, len(r["rays"])
    assert len(r["undecided"]) == 0
    # not convex: some ray meets the surface more than twice
    P = r["posed"]
    N, A, Bv, c = R.triangle_setup(P, f)
    dx, dy, dz = R.sensor_tables()
    ray = r["rays"][:: max(1, len(r["rays"]) // 300)]
    d = np.stack([dx[ray % R.HRES], dy[ray % R.HRES], dz[ray // R.HRES]], 1)
    den = d @ N.T
    with np.errstate(divide="ignore", invalid="ignore"):
        u, w = (d @ A.T) / den, (d @ Bv.T) / den
    crossings = ((den != 0) & (u >= 0) & (w >= 0) & (u + w <= 1)).sum(1)
    assert crossings.max() >= 4
    assert S.builtin_mesh(cat, 1)[0].shape == S.builtin_mesh(cat, 1)[0].shape and not np.array_equal(S.builtin_mesh(cat, 1)[0], S.builtin_mesh(cat, 2)[0])


def test_writer_files_are_read_back_by_the_provider(tmp_path):
    """write_dataset's layout through provider.load_batch, and the reference's meta keys."""
    import importlib
    if PKG not in sys.path:
        sys.path.insert(0, PKG)
    for m in ("config", "provider"):
        sys.modules.pop(m, None)
    config = importlib.import_module("config")
    scenes = [S.draw_scene(seed, "carspersons") for seed in (3, 4, 5)]
    clouds = [[R.cloud(*S.load_mesh("builtin", s.cat, s.mesh_id)[:2], s.mesh_scale, list(p) + [a])["points"]
               for p, a in ((s.transform.start_position, s.transform.start_angle), (s.transform.end_position, s.transform.end_angle))] for s in scenes]
    off = np.zeros((4, 2), np.int64)
    off[1:] = np.cumsum([[len(c[0]), len(c[1])] for c in clouds], 0)
    p1, p2 = (np.concatenate([c[k] for c in clouds]) for k in (0, 1))
    root = tmp_path / "SynthTiny"
    S.write_dataset(str(root), scenes, p1, p2, off, n_train=2)
    meta = json.load(open(root / "meta" / "00000001.json"))
    assert list(meta) == ["start_position", "start_angle", "end_position", "end_angle", "translation", "rel_angle",
                          "version", "seed", "mesh_id", "mesh_scale", "cat"]
    assert open(root / "split" / "train.txt").read() == "0\n1\n" and open(root / "split" / "val.txt").read() == "2\n"
    pc = np.load(root / "pointcloud2" / "00000002.npy")
    assert pc.dtype == np.float64 and pc.shape == (len(clouds[2][1]), 3) and np.array_equal(pc, clouds[2][1].astype(np.float64))
    assert np.array_equal(np.load(root / "transform" / "00000000.npy"), scenes[0].transform.rel_transform)
    cfgp = tmp_path / "cfg.json"
    json.dump({"data": {"basepath": str(root)}, "logging": {"basedir": str(tmp_path / "logs")}, "model": {"num_points": 32}}, open(cfgp, "w"))
    config.load_config(str(cfgp))
    provider = importlib.import_module("provider")
    np.random.seed(0)
    batch = provider.load_batch([0, 2], override_batch_size=2)
    pcs1, pcs2, translations, rel_angles, pc1centers, pc2centers, pc1angles, pc2angles = batch
    assert pcs1.shape == (2, 32, 3) and pcs2.shape == (2, 32, 3)
    for k, s in enumerate((scenes[0], scenes[2])):
        t = s.transform
        assert np.array_equal(np.ravel(translations[k]), t.translation) and np.ravel(rel_angles[k])[0] == t.rel_angle
        assert np.array_equal(np.ravel(pc1centers[k]), t.start_position) and np.array_equal(np.ravel(pc2centers[k]), t.end_position)
        assert np.ravel(pc1angles[k])[0] == t.start_angle and np.ravel(pc2angles[k])[0] == t.end_angle
    # every loaded point is a point of the written cloud
    src = clouds[0][0].astype(np.float64)
    assert all((src == p).all(1).any() for p in pcs1[0][:8])


def test_scene_labels_and_meta_agree():
    s = S.draw_scene(9, "cars")
    lab = S.scene_labels(s)
    t = s.transform
    assert lab.dtype == np.float32 and lab.shape == (12,)
    np.testing.assert_allclose(lab, np.concatenate([t.translation, [t.rel_angle], t.start_position, t.end_position, [t.start_angle, t.end_angle]]), rtol=1e-7)
    assert abs((t.end_angle - t.start_angle) - t.rel_angle) < 1e-15 and np.allclose(t.end_position - t.start_position, t.translation)


def test_cast_kernel_uses_no_scratch():
    """The cast kernel (both instantiations) and the kernels around it keep everything in registers: hipcc's resource remarks next to the object."""
    path = os.path.join(PKG, "csrc", "alignnet_scene.remarks")
    if not os.path.exists(path):
        pytest.skip("no resource remarks next to the objects (library built by an older Makefile)")
    rows = re.findall(r"Function Name: (\S+).*?ScratchSize \[bytes/lane\]: (\d+).*?VGPRs Spill: (\d+)", open(path).read(), re.S)
    seen = {}
    for name, scratch, spill in rows:
        for key in ("scene_cast_kernel", "scene_window_kernel", "scene_count_kernel", "scene_scan_kernel", "scene_scatter_kernel"):
            if key in name:
                seen.setdefault(key, []).append((name, int(scratch), int(spill)))
    assert set(seen) == {"scene_cast_kernel", "scene_window_kernel", "scene_count_kernel", "scene_scan_kernel", "scene_scatter_kernel"}, sorted(seen)
    assert len(seen["scene_cast_kernel"]) == 2
    for lst in seen.values():
        for name, scratch, spill in lst:
            assert scratch == 0 and spill == 0, (name, scratch, spill)
