"""Synthetic LiDAR scenes: the host side of the GPU scene generator (csrc/alignnet_scene.hip).

Counterpart of the reference's SynthCars / SynthCarsPersons / Synth20 / Synth20others generation (tp_utils/pointcloud.py:945-971 the
sensor, :447-454 Mesh, :520-556 RandomTransform, :1055-1186 SyntheticScene / SyntheticSceneCats): a ModelNet mesh is normalised, scaled,
put at two poses and scanned by a 64 x 4500-ray spinning LiDAR at the origin; `meta/ pointcloud1/ pointcloud2/ transform/` files are
written.  Here the ray cast runs on the GPU (Engine.scene_generate); this module holds everything around it:

  sensor_tables()      the 4500 (sin, cos) and 64 tan values times 120, by NumPy in the reference's operation order
  read_off()           OFF meshes (polygons as fans, ModelNet's `OFF490 518 0` header glued onto one line)
  normalise_mesh()     Mesh.__init__: bounds midpoint to 0, longest half extent to 0.5
  draw_scene()         the np.random draws of the three reference constructors, in the reference's order (tests/golden/scene_vectors.*)
  builtin_mesh()       procedural car and person meshes (this project's own geometry), so that everything runs with no mesh files
  generate()           scenes -> clouds on the device, optionally installed as the HBM-resident dataset
  write_dataset()      the reference's on-disk layout

The noise of a generated cloud is the engine's counter stream, not np.random.randn's (include/alignnet_hip.h): datasets made here are
distributed like the reference's, not equal to them.
"""
import io
import json
import os
from collections import namedtuple

import numpy as np

VRES, VFOV, HRES, HFOV = 64, 26.9, 4500, 360.0
RAY_LENGTH = 120.0
PERSON_BLACKLIST = [1, 13, 16, 19, 26, 29, 30, 40, 41, 44, 45, 46, 51, 58, 60, 76, 77, 82, 85, 86, 92, 93, 94, 101, 106, 107, 108]
CAR_BLACKLIST = [21, 31, 46]


def sensor_tables():
    """(dir_x [4500], dir_y [4500], dir_z [64]): ray idx = vidx * 4500 + hidx has direction (dir_x[hidx], dir_y[hidx], dir_z[vidx]),
    pointcloud.py:957-971 with the loops written as arrays (same operations in the same order)."""
    vangle = -VFOV / 2.0 + VFOV / (VRES - 1) * np.arange(VRES)
    hangle = -HFOV / 2.0 + HFOV / (HRES) * np.arange(HRES)
    return (np.sin(hangle / 180. * np.pi) * RAY_LENGTH, np.cos(hangle / 180. * np.pi) * RAY_LENGTH, np.tan(vangle / 180. * np.pi) * RAY_LENGTH)


def ray_directions(rows=None):
    """[n, 3] rows of the reference's `ray_directions` table (all 288000 when rows is None)."""
    dx, dy, dz = sensor_tables()
    idx = np.arange(VRES * HRES) if rows is None else np.asarray(rows, np.int64)
    return np.stack([dx[idx % HRES], dy[idx % HRES], dz[idx // HRES]], 1)


# ---- meshes ----------------------------------------------------------------------------------------------------------------------------
def read_off(path_or_text):
    """(vertices [nv, 3] float64, faces [nf, 3] int32) of an OFF file (a path, or the text itself when it holds a newline).  Polygons
    become fans about their first vertex; `#` comments and blank lines are skipped; the counts may be glued to the magic word
    (`OFF490 518 0`, as in part of ModelNet40)."""
    text = path_or_text if "\n" in path_or_text else open(path_or_text).read()
    tokens = []
    for line in text.splitlines():
        line = line.split("#", 1)[0].strip()
        if line:
            tokens.extend(line.split())
    if not tokens or not tokens[0].upper().startswith("OFF"):
        raise ValueError("not an OFF file")
    head = tokens[0][3:]
    tokens = ([head] if head else []) + tokens[1:]
    nv, nf = int(tokens[0]), int(tokens[1])
    pos = 3
    verts = np.array(tokens[pos:pos + 3 * nv], np.float64).reshape(nv, 3)
    pos += 3 * nv
    faces = []
    for _ in range(nf):
        k = int(tokens[pos])
        idx = [int(x) for x in tokens[pos + 1:pos + 1 + k]]
        pos += 1 + k
        faces.extend([idx[0], idx[i], idx[i + 1]] for i in range(1, k - 1))
    faces = np.array(faces, np.int32).reshape(-1, 3)
    if faces.size and (faces.min() < 0 or faces.max() >= nv):
        raise ValueError("OFF face index out of range")
    return verts, faces


def write_off(vertices, faces):
    out = ["OFF", "%d %d 0" % (len(vertices), len(faces))]
    out += ["%r %r %r" % tuple(float(x) for x in v) for v in vertices]
    out += ["3 %d %d %d" % tuple(int(i) for i in f) for f in faces]
    return "\n".join(out) + "\n"


def normalise_mesh(vertices):
    """Mesh.__init__ (pointcloud.py:447-454): subtract the midpoint of the bounds, scale by 1 / (2 max |bounds|)."""
    v = np.asarray(vertices, np.float64).reshape(-1, 3)
    if not len(v):
        return v.copy()
    bounds = np.stack([v.min(0), v.max(0)])
    v = v - np.mean(bounds, axis=0)
    bounds = np.stack([v.min(0), v.max(0)])
    return v * (1.0 / (np.max(np.abs(bounds)) * 2.0))


def mesh_centroid(vertices, faces):
    """trimesh's mesh.centroid: the area-weighted mean of the triangle centroids (the mean of the vertices when the total area is 0)."""
    v = np.asarray(vertices, np.float64).reshape(-1, 3)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    if not len(v):
        return np.zeros(3)
    if len(f):
        tri = v[f]
        area = 0.5 * np.linalg.norm(np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]), axis=1)
        if area.sum() > 0:
            return (tri.mean(1) * area[:, None]).sum(0) / area.sum()
    return v.mean(0)


def _strip(x, zb, zt, half_width):
    """Closed solid between a bottom curve zb(x) and a top curve zt(x) sampled at the stations x, extruded to y = +-half_width."""
    n = len(x)
    v = []
    for side in (-half_width, half_width):
        v += [(x[i], side, zb[i]) for i in range(n)] + [(x[i], side, zt[i]) for i in range(n)]
    b0, t0, b1, t1 = 0, n, 2 * n, 3 * n
    f = []
    for i in range(n - 1):
        f += [(b0 + i, b0 + i + 1, t0 + i + 1), (b0 + i, t0 + i + 1, t0 + i)]            # side y = -w
        f += [(b1 + i, t1 + i + 1, b1 + i + 1), (b1 + i, t1 + i, t1 + i + 1)]            # side y = +w
        f += [(t0 + i, t0 + i + 1, t1 + i + 1), (t0 + i, t1 + i + 1, t1 + i)]            # top
        f += [(b0 + i, b1 + i + 1, b0 + i + 1), (b0 + i, b1 + i, b1 + i + 1)]            # bottom
    f += [(b0, t0, t1), (b0, t1, b1)]                                                      # rear end
    f += [(b0 + n - 1, t1 + n - 1, t0 + n - 1), (b0 + n - 1, b1 + n - 1, t1 + n - 1)]      # front end
    return np.array(v, np.float64), np.array(f, np.int32)


def _prism(centre, radius, half_len, axis, sides):
    """Closed regular prism (a coarse cylinder) about `axis` (0, 1 or 2)."""
    a = 2 * np.pi * (np.arange(sides) + 0.5) / sides
    ring = np.stack([np.cos(a) * radius[0], np.sin(a) * radius[1]], 1)
    other = [k for k in range(3) if k != axis]
    v = np.zeros((2 * sides + 2, 3))
    for e, s in enumerate((-half_len, half_len)):
        v[e * sides:(e + 1) * sides, other[0]] = ring[:, 0]
        v[e * sides:(e + 1) * sides, other[1]] = ring[:, 1]
        v[e * sides:(e + 1) * sides, axis] = s
        v[2 * sides + e, axis] = s
    f = []
    for i in range(sides):
        j = (i + 1) % sides
        f += [(i, j, sides + j), (i, sides + j, sides + i), (2 * sides, j, i), (2 * sides + 1, sides + i, sides + j)]
    return v + np.asarray(centre, np.float64), np.array(f, np.int32)


def _merge(parts):
    vs, fs, n = [], [], 0
    for v, f in parts:
        vs.append(v); fs.append(f + n); n += len(v)
    return np.concatenate(vs), np.concatenate(fs).astype(np.int32)


def builtin_mesh(cat, mesh_id=1):
    """Procedural stand-ins for the ModelNet meshes (metres, before normalisation): `car` -- a 4.4 m body whose side profile carries bonnet,
    windscreen, roof and boot on top and two wheel arches underneath, with four wheels standing in the arches (not convex: the arches, the
    wheels and the cabin occlude parts of the body); `person` -- torso, head, arms and legs as prisms.  mesh_id varies the proportions a
    little (a pseudo-random but fixed function of the id), so that a data set holds more than one shape.  Any other category is a car."""
    g = np.random.RandomState(1000 + int(mesh_id))   # a generator of its own: the global np.random stream belongs to the scene draws
    k = g.uniform(0.9, 1.1, 6)
    if cat == "person":
        h = 1.75 * k[0]
        parts = [_prism((0, 0, 0.58 * h + 0.14 * h), (0.17 * k[1], 0.11), 0.14 * h, 2, 8),                  # torso
                 _prism((0, 0, 0.93 * h), (0.09, 0.1), 0.07 * h, 2, 8)]                                     # head
        for s in (-1, 1):
            parts.append(_prism((0.01 * s, 0.09 * s * k[1], 0.29 * h), (0.075, 0.07), 0.29 * h, 2, 8))      # legs
            parts.append(_prism((0.02 * s, 0.235 * s * k[1], 0.62 * h), (0.05, 0.045), 0.17 * h * k[2], 2, 8))   # arms
        return _merge(parts)
    L, W, H = 2.2 * k[0], 0.88 * k[1], 1.43 * k[2]
    wheel_x, wheel_r = (-0.62 * L, 0.60 * L), 0.33 * k[3]
    arch_r, sill = wheel_r + 0.07, 0.19
    x = np.unique(np.concatenate([np.linspace(-L, L, 23), [wx + arch_r * np.cos(a) for wx in wheel_x for a in np.linspace(0, np.pi, 9)]]))
    zb = np.full_like(x, sill)
    for wx in wheel_x:
        inside = np.abs(x - wx) < arch_r
        zb[inside] = np.maximum(sill, wheel_r + np.sqrt(np.maximum(arch_r ** 2 - (x[inside] - wx) ** 2, 0.0)))
    # top profile: boot, rear window, roof, windscreen, bonnet, nose
    px = np.array([-1.0, -0.93, -0.55, -0.42, 0.12, 0.42, 0.93, 1.0]) * L
    pz = np.array([0.52, 0.64, 0.66, 1.0, 1.0, 0.62, 0.55, 0.40]) * H
    zt = np.interp(x, px, pz)
    zb = np.minimum(zb, zt - 0.05)
    parts = [_strip(x, zb, zt, W)]
    for wx in wheel_x:
        for s in (-1, 1):
            parts.append(_prism((wx, s * (W - 0.13), wheel_r), (wheel_r, wheel_r), 0.12, 1, 12))
    return _merge(parts)


def load_mesh(source, cat, mesh_id):
    """Normalised (vertices, faces, centroid) of mesh `mesh_id` of category `cat`: source "builtin", or the root of ModelNet40Aligned
    (`<cat>/train/<cat>_%04d.off`, else `<cat>/test/...`: pointcloud.py:1088-1090)."""
    if source == "builtin":
        v, f = builtin_mesh(cat, mesh_id)
    else:
        name = "%s_%s.off" % (cat, str(mesh_id).zfill(4))
        path = os.path.join(source, cat, "train", name)
        if not os.path.isfile(path):
            path = os.path.join(source, cat, "test", name)
        v, f = read_off(path)
    v = normalise_mesh(v)
    return v, f, mesh_centroid(v, f)


# ---- scene draws -----------------------------------------------------------------------------------------------------------------------
def rot_z4(translation, angle):
    """get_mat_angle(translation, angle) about the origin (pointcloud.py:279-289)."""
    c, s = np.cos(angle), np.sin(angle)
    m = np.eye(4)
    m[:2, :2] = [[c, -s], [s, c]]
    m[:3, 3] = translation
    return m


Transform = namedtuple("Transform", "angle velocity translation rel_angle start_position start_angle end_position end_angle "
                                    "transform_start rel_transform transform_end")
Scene = namedtuple("Scene", "seed version cat mesh_id mesh_scale transform")


def random_transform(polar_dist_range):
    """RandomTransform.__init__ (pointcloud.py:520-556): six uniform draws from the global np.random stream."""
    angle = np.random.uniform(-np.pi, np.pi)
    velocity = np.random.uniform(0, 1)
    translation = np.array([np.sin(angle), np.cos(angle), 0]) * velocity
    rel_angle = np.random.uniform(-np.pi, np.pi) / 2.0
    polar_angle = np.random.uniform(-np.pi, np.pi)
    polar_distance = np.random.uniform(*polar_dist_range)
    start_position = np.array([np.sin(polar_angle), np.cos(polar_angle), 0]) * polar_distance
    start_angle = np.random.uniform(-np.pi, np.pi)
    end_position = start_position + translation
    end_angle = start_angle + rel_angle
    return Transform(angle, velocity, translation, rel_angle, start_position, start_angle, end_position, end_angle,
                     rot_z4(start_position, start_angle), rot_z4(translation, rel_angle), rot_z4(end_position, end_angle))


def draw_scene(seed, kind="cars", version=1, second_object_set=False, polar_dist_range=(4, 20), person_prob=0.2, cats=None,
               obj_size_range=None):
    """np.random.seed(seed), then the draws of the reference constructor in its order:
    kind "cars":        SyntheticScene(seed, version, second_object_set)                          (SynthCars)
    kind "carspersons": SyntheticScene(..., allow_persons=True, person_prob=person_prob)          (SynthCarsPersons)
    kind "cats":        SyntheticSceneCats(seed, version, cats, second_object_set)                (Synth20 / Synth20others)
    SyntheticScene first runs Scene.__init__, whose RandomTransform([4, 20]) is drawn and discarded; SyntheticSceneCats skips it
    (`super(Scene, self).__init__()`)."""
    np.random.seed(seed)
    if kind == "cats":
        assert cats, "kind 'cats' needs the list of categories"
        tr = random_transform(polar_dist_range)
        cat = str(np.random.choice(cats))
        mesh_scale = np.random.uniform(*(obj_size_range or (1., 5.0)))
        mesh_ids = np.arange(20) + 1
        if second_object_set:
            mesh_ids = np.arange(20) + 20 + 1
    else:
        assert kind in ("cars", "carspersons"), kind
        random_transform([4, 20])
        tr = random_transform(polar_dist_range)
        cat = "car"
        if kind == "carspersons" and np.random.random() < person_prob:
            cat = "person"
        mesh_scale = np.random.uniform(*(obj_size_range or dict(car=[6, 6], person=[1.6, 2.0]))[cat])
        lo, hi = (54, 104 if cat == "car" else 105) if second_object_set else (1, 54)
        black = PERSON_BLACKLIST if cat == "person" else ([] if second_object_set else CAR_BLACKLIST)
        mesh_ids = [i for i in range(lo, hi) if i not in black]
        assert len(mesh_ids) == (50 if cat == "car" else 40)
    mesh_id = int(np.random.choice(mesh_ids))
    return Scene(seed, version, cat, mesh_id, float(mesh_scale), tr)


def scene_labels(scene):
    """The 12 label columns of alignnet3d/packed.py: translation, rel_angle, start_position, end_position, start_angle, end_angle."""
    t = scene.transform
    return np.concatenate([t.translation, [t.rel_angle], t.start_position, t.end_position, [t.start_angle, t.end_angle]]).astype(np.float32)


# ---- generation ------------------------------------------------------------------------------------------------------------------------
class MeshLibrary:
    """The distinct meshes of a list of scenes, loaded and normalised once, in first-use order."""

    def __init__(self, source="builtin"):
        self.source, self.index, self.meshes = source, {}, []

    def add(self, cat, mesh_id):
        key = (cat, int(mesh_id))
        if key not in self.index:
            self.index[key] = len(self.meshes)
            self.meshes.append(load_mesh(self.source, cat, mesh_id))
        return self.index[key]


CASTS = {"scan": 0, "binned": 1, "auto": 2}   # engine option scene_cast (include/alignnet_hip.h)


def cast_option(cast):
    """The value of the engine option "scene_cast" for a cast name; ValueError for an unknown one."""
    if cast not in CASTS:
        raise ValueError("cast = %r: expected one of %s" % (cast, ", ".join(sorted(CASTS))))
    return CASTS[cast]


def generate(engine, scenes, seed=0, meshes="builtin", noise=True, sigma=0.05, clip=0.05, install=False, cast="scan", rows=False):
    """Cast `scenes` (draw_scene results) on the GPU.  The noise key of a scene is (seed, scene.seed): a scene's clouds do not depend on
    what else is in the list.  Returns the offsets table [B + 1, 2]; the clouds stay on the device -- engine.scene_read() copies them
    out, install=True makes them the HBM-resident dataset (engine.sample_batch, train_step_rows, icp_refine_rows, ... work on it).
    cast: "scan" (every tile of a cloud's window goes through the whole mesh), "binned" (the triangles are binned to the tiles first) or
    "auto" (binned for meshes of more than 512 triangles); it sets the engine option "scene_cast", which stays set.  The clouds are the same
    bit for bit whichever is chosen; "binned" and "auto" are exact alternatives that were slower than "scan" at every mesh size measured
    (516 to 100,002 triangles: profiles/scene_cast_rate.json).
    rows: True runs the inner loop of the chosen cast by elevation band (a staged triangle is intersected only with the bands of 8 rows
    it can reach); it sets the engine option "scene_rows", which stays set, and changes no result either (profiles/scene_rows_rate.json)."""
    option = cast_option(cast)
    if not isinstance(rows, (bool, np.bool_)):
        raise ValueError("rows = %r: expected True or False" % (rows,))
    engine.set_option("scene_cast", option)
    engine.set_option("scene_rows", int(rows))
    lib = meshes if isinstance(meshes, MeshLibrary) else MeshLibrary(meshes)
    first = len(lib.meshes)
    ids = [lib.add(s.cat, s.mesh_id) for s in scenes]
    if len(lib.meshes) != first or getattr(engine, "_scene_library", None) is not lib:
        engine.scene_upload_meshes(lib.meshes)
        engine._scene_library = lib
    poses = np.array([[list(s.transform.start_position) + [s.transform.start_angle], list(s.transform.end_position) + [s.transform.end_angle]]
                      for s in scenes], np.float64).reshape(len(scenes), 2, 4)
    off = engine.scene_generate(ids, [s.mesh_scale for s in scenes], poses, scene_ids=[s.seed for s in scenes], seed=seed,
                                sigma=sigma if noise else 0.0, clip=clip)
    if install:
        engine.scene_install_dataset(np.stack([scene_labels(s) for s in scenes]))
    return off


def np_to_str(arr):
    """pointcloud.py:245-252, plaintext branch: np.savetxt into a string (provider.str_to_np reads it back)."""
    out = io.BytesIO()
    np.savetxt(out, arr)
    return out.getvalue().decode("ascii")


def scene_meta(scene):
    """Scene.save_meta + SyntheticScene.save_meta (pointcloud.py:986-997, 1140-1148): the same keys in the same order."""
    t = scene.transform
    return {"start_position": np_to_str(t.start_position), "start_angle": t.start_angle, "end_position": np_to_str(t.end_position),
            "end_angle": t.end_angle, "translation": np_to_str(t.translation), "rel_angle": t.rel_angle,
            "version": scene.version, "seed": scene.seed, "mesh_id": int(scene.mesh_id), "mesh_scale": scene.mesh_scale, "cat": scene.cat}


def write_dataset(root, scenes, points1, points2, offsets, n_train):
    """meta/%08d.json, pointcloud{1,2}/%08d.npy (float64 [n, 3]), transform/%08d.npy (rel_transform), split/{train,val}.txt: example i is
    scenes[i]; the first n_train go to the training split, the rest to validation."""
    for sub in ("meta", "pointcloud1", "pointcloud2", "transform", "split"):
        os.makedirs(os.path.join(root, sub), exist_ok=True)
    for i, s in enumerate(scenes):
        stem = str(i).zfill(8)
        with open(os.path.join(root, "meta", stem + ".json"), "w") as fh:
            json.dump(scene_meta(s), fh)
        for k, pts in enumerate((points1, points2)):
            np.save(os.path.join(root, "pointcloud%d" % (k + 1), stem), np.asarray(pts[offsets[i, k]:offsets[i + 1, k]], np.float64))
        np.save(os.path.join(root, "transform", stem), s.transform.rel_transform)
    for name, ids in (("train", range(n_train)), ("val", range(n_train, len(scenes)))):
        with open(os.path.join(root, "split", name + ".txt"), "w") as fh:
            fh.write("".join("%d\n" % i for i in ids))
