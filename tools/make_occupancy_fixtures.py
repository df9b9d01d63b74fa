#!/usr/bin/env python3
"""Writes tests/golden/occupancy_octomap.npz (+ .sha256): what the reference's OWN octomap says about a few thousand
world points -- Vector3::norm() of the offset from the sensor origin, coordToKeyChecked's verdict and key -- and, after
updateNode(key, true) on the accepted ones, getNumLeafNodes(), size() and the bytes of writeBinary.

Run by hand, never by a test:

    python tools/make_occupancy_fixtures.py --reference /path/to/U96-SLAM [--out DIR]

It compiles its driver, tools/octomap_drivers/hits.cpp (this project's text), against the octomap sources vendored in the
reference tree (src/slam/src/octomap/*.cpp, headers under src/slam/include; tools/octomap_kit.py builds them once, outside the
history), feeds it the points and keeps only inputs and recorded outputs. The points are made here from disparity planes and poses through the front half of
oracle/occupancy_ref (reprojection and the two transforms), so that the GPU tests can feed the very same cases as planes:

    scene   three 40 x 30 planes of a sloped scene (rows from 55 m down to 0.9 m, some invalid pixels) through three poses
    edge    1 x 1 planes under poses with a ZERO rotation block: the world point is the pose's translation, exactly, and the
            offset from the origin is 0. Points straddling zero on each axis, within one float ulp of voxel faces, the key
            range edge (3276.75f -> key 65535; the next voxel is rejected), values whose floor fits no int, inf and NaN; a full
            2 x 2 x 2 block, a full 4 x 4 x 4 block and a 2 x 2 x 2 block with one voxel missing
    norm    1 x 1 planes under a model whose local transform has a zero rotation block and the translation (15, 20, 0) -- norm
            exactly 25 -- through scaling and translating poses: offsets on both sides of norm 25
"""
import struct

import numpy as np

import octomap_kit as kit
from octomap_kit import down, f32, occ, up, voxel

NGROUPS = 3   # tree 0: every accepted point; tree 1: the blocks alone; tree 2: nothing


def scene():
    rng = np.random.default_rng(11)
    h, w = 30, 40
    rows, cols = np.mgrid[0:h, 0:w]
    planes = []
    for k in range(3):
        d = 14 + 30 * rows + 2 * cols + 40 * k + rng.integers(0, 3, (h, w))
        d = d.astype(np.int16)
        d[rng.random((h, w)) < 0.05] = -16           # FILTERED
        d[rng.random((h, w)) < 0.02] = 0
        planes.append(d)
    poses = []
    for k, (yaw, t) in enumerate(((0.0, (0.0, 0.0, 0.0)), (0.35, (0.8, -0.3, 0.02)), (-2.1, (-1.7, 2.4, -0.05)))):
        c, s = np.cos(yaw), np.sin(yaw)
        poses.append([c, -s, 0, t[0], s, c, 0, t[1], 0, 0, 1, t[2]])
    # camera (z forward, x right, y down) -> body (x forward, y left, z up), lifted 0.2 m
    local = [0, 0, 1, 0.05, -1, 0, 0, 0, 0, -1, 0, 0.2]
    return np.stack(planes), np.asarray(poses, np.float32), occ.model(local=local)


def zero_rotation(t):
    return [0, 0, 0, t[0], 0, 0, 0, t[1], 0, 0, 0, t[2]]


def edge_points():
    """World points (float32 triples) of the edge group and a parallel list: is the point part of the blocks-only tree."""
    pts, block = [], []
    rest = [f32(1.234), f32(-2.5), f32(0.77)]

    def axis_values(vals):
        for a in range(3):
            for v in vals:
                p = list(rest)
                p[a] = f32(v)
                pts.append(p)
                block.append(False)

    tiny = f32(1e-30)
    axis_values([f32(0.0), f32(-0.0), tiny, -tiny, f32(0.05), f32(-0.05), f32(0.1), f32(-0.1), up(0.1), down(0.1), up(-0.1),
                 down(-0.1)])
    for k in (3, 7, -5, 12, -20, 100, 4095, -4096):
        face = f32(k * 0.1)
        axis_values([face, up(face), down(face)])
    edge = f32(3276.75)
    axis_values([edge, f32(3276.8), down(3276.8), up(3276.8), f32(-3276.8), up(-3276.8), down(-3276.8), f32(3276.9), f32(-3276.9),
                 f32(2e8), f32(-2e8), f32(3e9), f32(-3e9), f32(1e10), f32(3e38), f32(np.inf), f32(-np.inf), f32(np.nan)])

    def cube(base, size, skip=None):
        for i in range(size):
            for j in range(size):
                for k in range(size):
                    if (i, j, k) == skip:
                        continue
                    pts.append([f32(voxel(base[0] + i)), f32(voxel(base[1] + j)), f32(voxel(base[2] + k))])
                    block.append(True)

    cube((1000, -2000, 400), 2)                 # collapses one level
    cube((1200, -2000, 400), 4)                 # collapses two levels
    cube((1400, -2000, 400), 2, skip=(1, 0, 1))   # must not collapse
    return np.asarray(pts, np.float32), np.asarray(block)


def norm_poses():
    eps = np.float32(2.0 ** -23)
    poses = []
    for a in (1.0, 1 + eps, 1 - eps / 2, 1 + 2 * eps, 1 - eps, 0.99999, 1.00001, 0.2, 0.24, 1.5):
        a = f32(a)
        poses.append([a, 0, 0, 0, 0, a, 0, 0, 0, 0, a, 0])
    for o in ((1, 2, 3), (-7.3, 0.2, 5.5), (0.1, 0.1, 0.1), (-15.0, -20.0, 0.0), (1e-3, -1e-3, 1e-3), (33.3, -41.7, 2.9),
              (-0.7, 0.3, -0.2), (100.1, 200.2, -300.3), (3.3, 4.4, 0.0), (-3.3, -4.4, 0.0)):
        poses.append([1, 0, 0, o[0], 0, 1, 0, o[1], 0, 0, 1, o[2]])
    return np.asarray(poses, np.float32)


def main():
    args = kit.arguments(__doc__)
    resolution, range_max, scale = 0.1, np.float32(5.0), 4

    scene_disp, scene_poses, m = scene()
    pts, origins, group = [], [], []
    for d, pose in zip(scene_disp, scene_poses):
        wpts = occ.world(d, scale, m, pose).reshape(-1, 3)
        pts.append(wpts)
        origins.append(np.tile(pose[[3, 7, 11]], (len(wpts), 1)))
        group.append(np.full(len(wpts), 1, np.uint8))
    edge_disp = np.full((1, 1), 160, np.int16)
    epts, eblock = edge_points()
    edge_poses = np.asarray([zero_rotation(p) for p in epts], np.float32)
    for pose in edge_poses:
        pts.append(occ.world(edge_disp, scale, m, pose).reshape(-1, 3))
        origins.append(pose[[3, 7, 11]][None])
    assert np.array_equal(np.concatenate(pts[3:]), epts, equal_nan=True)   # a zero rotation block hands the translation through
    group.append(np.where(eblock, 3, 1).astype(np.uint8))
    m_edge = occ.model(local=zero_rotation((15.0, 20.0, 0.0)))
    nposes = norm_poses()
    for pose in nposes:
        pts.append(occ.world(edge_disp, scale, m_edge, pose).reshape(-1, 3))
        origins.append(pose[[3, 7, 11]][None])
    group.append(np.full(len(nposes), 1, np.uint8))
    pts = np.ascontiguousarray(np.concatenate(pts), np.float32)
    origins = np.ascontiguousarray(np.concatenate(origins), np.float32)
    group = np.concatenate(group)
    n = len(pts)

    code, raw = kit.run(kit.build(args.reference, "hits"), "hits", lambda f: f.write(
        struct.pack("<dfii", resolution, float(range_max), n, NGROUPS) + np.concatenate([pts, origins], axis=1).astype(np.float32).tobytes() +
        group.tobytes()))
    assert code == 0, code
    r = kit.Reader(raw)
    rec = r.take(np.dtype([("norm", "<f8"), ("ok", "u1"), ("key", "<u2", 3)]), n)
    trees = {name: (r.one("<u4"), r.one("<u4"), r.stream()) for name in ("all", "blocks", "empty")}
    r.done()
    out = dict(resolution=np.float64(resolution), range_max=range_max, scale=np.int32(scale), model=occ.model_to_array(m),
               model_edge=occ.model_to_array(m_edge), scene_disp=scene_disp, scene_poses=scene_poses, edge_disp=edge_disp,
               edge_poses=edge_poses, norm_poses=nposes, points=pts, origins=origins, group=group, norm=rec["norm"].copy(),
               ok=rec["ok"].copy(), keys=rec["key"].copy())
    for name, (leafs, size, data) in trees.items():
        out[f"leafs_{name}"], out[f"size_{name}"], out[f"bt_{name}"] = np.uint32(leafs), np.uint32(size), data
    OUT = kit.save(args.out, "octomap", out, kit.numpy_npz)
    gate = rec["norm"] <= float(range_max * range_max)
    print(f"{OUT}: {OUT.stat().st_size} bytes, {n} points, {int(rec['ok'].sum())} keyed, {int((gate & (rec['ok'] == 1)).sum())} "
          f"accepted, norms above the gate {int((~gate & np.isfinite(rec['norm'])).sum())}; trees "
          + ", ".join(f"{k}: {v[0]} leafs / {v[1]} nodes / {len(v[2])} B" for k, v in trees.items()))


if __name__ == "__main__":
    main()
