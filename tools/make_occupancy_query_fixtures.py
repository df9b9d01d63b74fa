#!/usr/bin/env python3
"""Writes tests/golden/occupancy_query.npz (+ .sha256): what the reference's OWN octomap answers for search(point) and
castRay(origin, direction, end, ignoreUnknownCells, maxRange) on a few small trees -- per point whether a node was found, its
log-odds and isNodeOccupied, per ray the return value and the bits of `end` (set to NaN before each call, because octomap leaves
it untouched where it gives up) -- together with the trees' inputs and leaves. Beside it, tests/golden/occupancy_query_cpu.json
holds the milliseconds per ray octomap's castRay took on the scene of tools/bench_occupancy_query.py (kept out of the .npz so
that the .npz regenerates to the same bytes).

Run by hand, never by a test:

    python tools/make_occupancy_query_fixtures.py --reference /path/to/U96-SLAM [--out DIR]

It compiles its driver, tools/octomap_drivers/query.cpp (this project's text; it calls octomap's API only), against the octomap
sources vendored in the reference tree (tools/octomap_kit.py builds them once, outside the history), and keeps only inputs and
recorded outputs. Log-odds trees are built with
insertPointCloud of recorded scans, the hit tree with updateNode(key, true) over a recorded key list. The statuses beside
octomap's answers are the transcription's (tests/occupancy_query_cases.py); the generator asserts that they agree with every
recorded return value and `end`. Trees and query sets:

    box     one scan from a voxel centre to the six faces of a 2 m cube: free inside, occupied shell, unknown outside
      origin   origin cell occupied / free / unknown x ignore_unknown 0 / 1, each also with a zero direction
      axes     single rays along +-x, +-y, +-z into the shell
      ties     the origin at a voxel centre, directions (+-1, +-1, +-1) and (1, 1, 0), both ignore_unknown values
      lengths  one ray with direction lengths 1e-3, 1 and 1e3
      bounds   an origin three cells from the +x and from the -x edge of the key space, cast outward
      odd      NaN / infinite origin and direction components, float overflow and underflow of the direction's squared norm
    wall2   a 5 x 5 wall 2 m ahead
      range    max_range just inside, exactly on and just outside the wall cell's squared distance, and 0 and -1
    gap     a free corridor, an unknown gap, then a wall
      gap      the ray along it under both ignore_unknown values
    thres   occupancy_thres == clamp_max, one voxel driven to the clamp: occupied under >=, free under >
    scene / scene_hits   the three 40 x 30 planes of tools/make_occupancy_fixtures.py as log-odds scans (max_range 6) and as
            a hit-mode tree
      view     a 40 x 30 view from pose 0
      random   1024 random rays with max_range 6
      search   512 points, every second on a voxel face
"""
import functools
import struct

import numpy as np

import octomap_kit as kit
from octomap_kit import BENCH_PLANES, BENCH_RANGE, PROBS, RESOLUTION, bench, occ, rc
import occupancy_query_cases as qc

F = np.float32
voxel = functools.partial(kit.voxel, dtype=np.float32)


def rays(rows):
    """rows: (origin, direction, ignore_unknown, max_range) -> a query set"""
    return dict(points=np.zeros((0, 3), np.float32), rays=np.array([list(o) + list(d) for o, d, _, _ in rows], np.float32).reshape(-1, 6),
                ignore=np.array([i for _, _, i, _ in rows], np.int32), max_range=np.array([r for _, _, _, r in rows], np.float64))


def view_rays_numpy(width, height, scale, m, pose):
    """The header's view formula in vectorised numpy, written apart from occupancy_query_cases.view_rays."""
    rows, cols = np.mgrid[0:height, 0:width]
    q = np.stack([((cols * scale).astype(np.float64) - m.cx_l) / m.fx_l, ((rows * scale).astype(np.float64) - m.cy_l) / m.fy_l,
                  np.ones((height, width))], -1).astype(np.float32).reshape(-1, 3)

    def apply(p, t):
        t = np.asarray(t, np.float32).reshape(3, 4)
        return np.stack([(t[r, 0] * p[:, 0] + t[r, 1] * p[:, 1]) + t[r, 2] * p[:, 2] + t[r, 3] for r in range(3)], -1).astype(np.float32)

    def T(p):
        return apply(apply(p, list(m.local)) if m.has_local else p, pose)

    o = T(np.zeros((1, 3), np.float32))
    return np.broadcast_to(o, q.shape).copy(), T(q) - o


def scene_sets(hits):
    disp, poses, m = kit.scene("query")
    rng = np.random.default_rng(23)
    o, d = view_rays_numpy(40, 30, 4, m, poses[0])
    qo, qd = qc.view_rays(40, 30, 4, m, poses[0])
    assert np.array_equal(o.view(np.uint32), qo.view(np.uint32)) and np.array_equal(d.view(np.uint32), qd.view(np.uint32))
    n = len(o)
    sets = {"view": dict(points=np.zeros((0, 3), np.float32), rays=np.concatenate([o, d], 1), ignore=np.ones(n, np.int32),
                         max_range=np.full(n, 6.0))}
    cloud = np.concatenate([rc.plane_points(dd, 4, m, p) for dd, p in zip(disp, poses)])
    jitter = np.where(np.arange(1024)[:, None] % 4 == 3, 0.3, 0.02)           # every fourth origin strays from its sensor
    ro = (poses[rng.integers(0, 3, 1024)][:, [3, 7, 11]] + jitter * rng.uniform(-1, 1, (1024, 3))).astype(np.float32)
    rd = rng.normal(size=(1024, 3))
    rd[:, 2] *= 0.3                                   # the scene lies around the sensors' height
    aim = np.arange(1024) % 8 < 5                     # five rays of eight aim at a point of the scans, give or take 5 cm
    rd[aim] = (cloud[rng.integers(0, len(cloud), 1024)] + rng.uniform(-0.05, 0.05, (1024, 3)) - ro)[aim]
    rd = (rd * rng.uniform(0.1, 10, (1024, 1))).astype(np.float32)
    ignore = (np.arange(1024) & 1).astype(np.int32) if not hits else np.ones(1024, np.int32)
    sets["random"] = dict(points=np.zeros((0, 3), np.float32), rays=np.concatenate([ro, rd], 1), ignore=ignore,
                          max_range=np.full(1024, 6.0))
    pts = cloud[rng.integers(0, len(cloud), 512)] * rng.uniform(0.2, 1.1, (512, 1))     # along the rays and a little beyond
    snap = rng.integers(0, 3, 512)
    for i in range(1, 512, 2):
        pts[i, snap[i]] = np.round(pts[i, snap[i]] / RESOLUTION) * RESOLUTION
    sets["search"] = dict(points=pts.astype(np.float32), rays=np.zeros((0, 6), np.float32), ignore=np.zeros(0, np.int32),
                          max_range=np.zeros(0))
    return sets


def make_trees():
    trees = {}
    c = voxel((0, 0, 0))
    g = np.arange(-10, 11) * 0.1
    a, b = np.meshgrid(g, g, indexing="ij")
    a, b, one = a.reshape(-1), b.reshape(-1), np.ones(a.size)
    faces = np.concatenate([np.stack(f, 1) for f in ((one, a, b), (-one, a, b), (a, one, b), (a, -one, b), (a, b, one), (a, b, -one))])
    box = dict(params=rc.RayParams(), scans=[(c, -1.0, (c + faces).astype(np.float32))], sets={})
    wall_cell = voxel((10, 0, 0))
    outside = voxel((30, 0, 0))
    rows = []
    for start, d in ((wall_cell + F(0.01), (1, 0, 0)), (c + F(0.02), (1, 0, 0)), (outside, (-1, 0, 0))):
        for ignore in (0, 1):
            rows += [(start, d, ignore, -1.0), (start, (0, 0, 0), ignore, -1.0)]
    box["sets"]["origin"] = rays(rows)
    o = c + np.float32([0.02, -0.03, 0.04])
    box["sets"]["axes"] = rays([(o, d, 0, -1.0) for d in ((1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1))])
    dirs = [(sx, sy, sz) for sx in (1, -1) for sy in (1, -1) for sz in (1, -1)] + [(1, 1, 0)]
    box["sets"]["ties"] = rays([(c, d, ignore, -1.0) for d in dirs for ignore in (0, 1)])
    box["sets"]["lengths"] = rays([(o, np.float32([0.3, -0.2, 0.1]) * F(s), 1, -1.0) for s in (1e-3, 1.0, 1e3)])
    hi, lo = voxel((65532 - 32768, 3, -2)), voxel((3 - 32768, 3, -2))
    box["sets"]["bounds"] = rays([(hi, (1, 0, 0), 1, -1.0), (lo, (-1, 0, 0), 1, -1.0), (hi, (1, 0, 0), 0, -1.0), (hi, (2, 1e-4, 0), 1, 0.0),
                                  (lo, (-1, -1e-5, 1e-5), 1, -5.0)])
    nan, inf = np.nan, np.inf
    odd = [((nan, 0, 0), (1, 0, 0)), ((inf, 0, 0), (1, 0, 0)), ((0, -inf, 0), (1, 0, 0)), ((0, 0, 4000.0), (0, 0, -1)),
           (o, (nan, 0, 0)), (o, (nan, 1, 0)), (o, (nan, nan, nan)), (o, (inf, 0, 0)), (o, (inf, 1, 0)), (o, (-inf, -inf, 0)),
           (o, (1e30, 0, 0)), (o, (1e30, 1e30, 1)), (o, (1e-30, 0, 0)), (o, (0, -1e-30, 1e-30)), (o, (1e-45, 0, 0)), (o, (-0.0, 0.0, -0.0))]
    box["sets"]["odd"] = rays([(a_, b_, 1, -1.0) for a_, b_ in odd])
    edge = [(3276.75, 0, 0), (3276.85, 0, 0), (-3276.8, 0, 0), (-3276.81, 0, 0), (nan, 0, 0), (0, inf, 0), (0.1, 0.2, 0.3),
            (1.0, 0.0, 0.0), (1.1, 0.0, 0.0), (1.05, 0.05, 0.05), (5.0, 5.0, 5.0)]
    box["sets"]["search"] = dict(points=np.array(edge, np.float32), rays=np.zeros((0, 6), np.float32), ignore=np.zeros(0, np.int32),
                                 max_range=np.zeros(0))
    trees["box"] = box

    w = np.array([(2.0, y, z) for y in g[8:13] for z in g[8:13]])
    wall = dict(params=rc.RayParams(), scans=[(c, -1.0, (c + w).astype(np.float32))], sets={})
    cell = qc.centre(rc.key3(c + np.float32([2.0, 0, 0]), 1 / RESOLUTION), RESOLUTION)
    dist = sum(float((cell[j] - c[j]) * (cell[j] - c[j])) for j in range(3))
    r = float(np.sqrt(dist))
    for _ in range(4):
        if r * r == dist:
            break
        r = float(np.nextafter(r, np.inf if r * r < dist else 0.0))
    assert r * r == dist, "range: no double squares to the wall cell's distance"
    inside, outside_r = float(np.nextafter(r, np.inf)), float(np.nextafter(r, 0.0))
    assert inside * inside > dist > outside_r * outside_r
    wall["sets"]["range"] = rays([(c, (1, 0, 0), 0, mr) for mr in (inside, r, outside_r, 0.0, -1.0, 1.0)])
    wall["range_values"] = (inside, r, outside_r)
    trees["wall2"] = wall

    far = c + np.float32([3.0, 0, 0])
    near = voxel((29, 0, 0))
    gap = dict(params=rc.RayParams(), scans=[(c, 1.0, far[None]), (near, -1.0, far[None])], sets={})
    gap["sets"]["gap"] = rays([(c, (1, 0, 0), ignore, mr) for ignore in (0, 1) for mr in (-1.0, 2.0)])
    trees["gap"] = gap

    p = c + np.float32([1.0, 0, 0])
    thres = dict(params=rc.RayParams(occupancy_thres=0.971), scans=[(c, -1.0, p[None])] * 8 + [(c, -1.0, (c + np.float32([0, 0.5, 0]))[None])],
                 sets={})
    thres["sets"]["clamp"] = rays([(c, (1, 0, 0), 0, -1.0), (c, (0, 1, 0), 0, -1.0)])
    thres["sets"]["search"] = dict(points=np.stack([p, c + np.float32([0, 0.5, 0]), c]), rays=np.zeros((0, 6), np.float32),
                                   ignore=np.zeros(0, np.int32), max_range=np.zeros(0))
    trees["thres"] = thres

    disp, poses, m = kit.scene("query")
    trees["scene"] = dict(params=rc.RayParams(), scans=[(pose[[3, 7, 11]], 6.0, rc.plane_points(d, 4, m, pose)) for d, pose in zip(disp, poses)],
                          sets=scene_sets(False))
    keys, counts = occ.insert(disp, 4, m, poses)
    trees["scene_hits"] = dict(params=rc.RayParams(), hit_keys=keys, hit_counts=counts, sets=scene_sets(True))

    _, bposes = bench.synth_planes(BENCH_PLANES)
    o, d = view_rays_numpy(bench.W, bench.H, bench.SCALE, bench.synth_model(), bposes[0])
    timing = dict(points=np.zeros((0, 3), np.float32), rays=np.concatenate([o, d], 1), ignore=np.ones(len(o), np.int32),
                  max_range=np.full(len(o), BENCH_RANGE), timing=True)
    trees["bench"] = dict(params=rc.RayParams(), timing=True, sets={"view": timing}, scans=kit.bench_scans())
    return trees


def restated_map(tree, constants):
    """The transcription's map of a tree, built by the insert transcription (or from the key list)."""
    if "hit_keys" in tree:
        return qc.Map({int(k): int(n) for k, n in zip(tree["hit_keys"], tree["hit_counts"])}, qc.HITS, 0.0, RESOLUTION)
    t = rc.Tree(tree["params"], RESOLUTION)
    for o, mr, p in tree["scans"]:
        t.rp.max_range = mr
        t.insert(p, o)
    return qc.Map(dict(t.v), qc.LOGODDS, constants[4], RESOLUTION)


def main():
    args = kit.arguments(__doc__)
    trees = make_trees()

    def write(f):
        f.write(kit.ints(len(trees)))
        for t in trees.values():
            hits = "hit_keys" in t
            f.write(kit.head(t["params"]) + kit.ints(hits) + (kit.hits(t["hit_keys"]) if hits else kit.scans(t["scans"])))   # each key once
            f.write(kit.ints(len(t["sets"])))
            for s in t["sets"].values():
                f.write(kit.ints(s.get("timing", False)) + kit.points(s["points"]) + kit.ints(len(s["rays"])))
                for r, ig, mr in zip(s["rays"], s["ignore"], s["max_range"]):
                    f.write(r.astype(np.float32).tobytes() + struct.pack("<id", int(ig), float(mr)))

    code, raw = kit.run(kit.build(args.reference, "query"), "query", write)
    assert code == 0, code
    r = kit.Reader(raw)
    out = dict(resolution=np.float64(RESOLUTION), trees=np.array([n for n, t in trees.items() if not t.get("timing")]))
    report, cpu, seen = [], {}, set()
    for name, t in trees.items():
        consts = r.take("<f4", 5).copy()
        n = r.one("<u4")
        keys, values = r.voxels(n)
        if t.get("timing"):
            s = t["sets"]["view"]
            ms = r.one("<f8")
            cpu = dict(scene="tools/bench_occupancy_rays.py synth_planes", planes=BENCH_PLANES, insert_max_range=BENCH_RANGE,
                       view=[bench.W, bench.H, bench.SCALE], ignore_unknown=1, max_range=BENCH_RANGE, rays=len(s["rays"]), leaves=int(n),
                       octomap_ms_per_ray=ms / len(s["rays"]),
                       note="octomap's castRay, one thread, -O1, on the CPU of the machine that made the fixture")
            report.append(f"{name}: {n} leaves, {ms / len(s['rays']) * 1e3:.2f} us per ray")
            continue
        hits = "hit_keys" in t
        m = restated_map(t, consts)
        assert np.array_equal(keys, np.array(sorted(m.v), np.uint64)), (name, "keys")
        if hits:
            out[f"{name}_counts"] = np.asarray(t["hit_counts"], np.uint32)
        else:
            assert np.array_equal(values.view(np.uint32), np.array([m.v[int(q)] for q in keys], np.float32).view(np.uint32)), (name, "values")
            out[f"{name}_logodds"] = values
            out[f"{name}_origins"] = np.stack([o for o, _, _ in t["scans"]]).astype(np.float32)
            out[f"{name}_scan_range"] = np.array([mr for _, mr, _ in t["scans"]], np.float64)
            out[f"{name}_points"] = np.concatenate([p for _, _, p in t["scans"]]).astype(np.float32)
            out[f"{name}_npoints"] = np.array([len(p) for _, _, p in t["scans"]], np.int32)
        out[f"{name}_hits"] = np.int32(hits)
        out[f"{name}_params"] = np.array([getattr(t["params"], q) for q in PROBS], np.float64)
        out[f"{name}_constants"] = consts
        out[f"{name}_keys"] = keys
        out[f"{name}_sets"] = np.array(list(t["sets"]))
        for sname, s in t["sets"].items():
            tag = f"{name}_{sname}"
            npts, nr = len(s["points"]), len(s["rays"])
            rec = r.take("<u4", 3 * npts).reshape(npts, 3)
            ret = r.take("<i4", nr).copy()
            end = r.take("<f4", 3 * nr).reshape(nr, 3).copy()
            if npts:
                state, value = m.search_all(s["points"])
                found, occupied = rec[:, 0].astype(bool), rec[:, 1].astype(bool)
                assert np.array_equal(found, state > 0) and np.array_equal(occupied, state == qc.CELL_OCCUPIED), (tag, "search")
                if not hits:
                    assert np.array_equal(rec[found, 2], value[found]), (tag, "log-odds")
                out[f"{tag}_points"] = s["points"].astype(np.float32)
                out[f"{tag}_found"] = found.astype(np.uint8)
                out[f"{tag}_occupied"] = occupied.astype(np.uint8)
                out[f"{tag}_value"] = value          # the 4-byte words: the bits of octomap's log-odds (NaN: no node), or hit counts
                out[f"{tag}_state"] = state
            if nr:
                status = np.empty(nr, np.int32)
                for i, (ray, ig, mr) in enumerate(zip(s["rays"], s["ignore"], s["max_range"])):
                    status[i], e = m.cast_ray(ray[:3], ray[3:], bool(ig), float(mr))
                    assert (status[i] == qc.RAY_HIT) == bool(ret[i]), (tag, i, "return value")
                    assert (status[i] == qc.RAY_NONE) == bool(np.isnan(end[i]).all()), (tag, i, "untouched end")
                    assert status[i] == qc.RAY_NONE or np.array_equal(e.view(np.uint32), end[i].view(np.uint32)), (tag, i, "end")
                seen.update(int(x) for x in status)
                out[f"{tag}_rays"] = s["rays"].astype(np.float32)
                out[f"{tag}_ignore"] = s["ignore"].astype(np.int32)
                out[f"{tag}_max_range"] = s["max_range"].astype(np.float64)
                out[f"{tag}_ret"] = ret.astype(np.uint8)
                out[f"{tag}_end"] = end
                out[f"{tag}_status"] = status
                report.append(f"{tag}: {nr} rays, statuses {np.bincount(status, minlength=5).tolist()}")
            else:
                report.append(f"{tag}: {npts} points, states {np.bincount(state + 1, minlength=4).tolist()}")
    r.done()
    assert seen == {0, 1, 2, 3, 4}, seen
    c = out["thres_constants"]
    assert c[3] == c[4], "thres: the threshold is not the clamp"
    key = rc.pack3(rc.key3(voxel((10, 0, 0)), 1 / RESOLUTION))
    assert out["thres_logodds"][list(out["thres_keys"]).index(key)] == c[3], "thres: the voxel is not at the clamp"
    assert out["wall2_range_status"].tolist() == [1, 1, 2, 1, 1, 2], out["wall2_range_status"]
    out["wall2_range_values"] = np.array(trees["wall2"]["range_values"], np.float64)
    assert out["gap_gap_status"].tolist() == [3, 3, 1, 2], out["gap_gap_status"]
    disp, poses, m = kit.scene("query")
    out["scene_disp"], out["scene_poses"], out["scene_model"], out["scene_scale"] = disp, poses, occ.model_to_array(m), np.int32(4)
    OUT = kit.save(args.out, "query", out, cpu=cpu)
    print(f"{OUT}: {OUT.stat().st_size} bytes\n  " + "\n  ".join(report))


if __name__ == "__main__":
    main()
