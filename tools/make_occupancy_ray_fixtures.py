#!/usr/bin/env python3
"""Writes tests/golden/occupancy_rays.npz (+ .sha256): what the reference's OWN octomap answers for
insertPointCloud(scan, origin, maxrange) on a few small scans -- after every scan the depth-16 leaves (key, float log-odds) of
the expanded tree, and at the end size() and the bytes of writeBinary -- together with the five log-odds constants of each
tree and the milliseconds octomap took for one plane of the benchmark's synthetic scan (tools/bench_occupancy_rays.py).

Run by hand, never by a test:

    python tools/make_occupancy_ray_fixtures.py --reference /path/to/U96-SLAM [--out DIR]

It compiles its driver, tools/octomap_drivers/rays.cpp (this project's text; it calls octomap's API only), against the octomap
sources vendored in the reference tree (tools/octomap_kit.py builds them once, outside the history), feeds it the scans and keeps
only inputs and recorded outputs. The cases:

    axes    single rays along +-x, +-y, +-z, one per scan: two steps are 0 and their tMax is the double maximum
    ties    origin at a voxel centre, ends along (+-1, +-1, +-1) * k * 0.1 and (1, 1, 0) * k * 0.1: equal tMax on two and three
            axes
    short   an end in the origin's cell; an end in a face-adjacent cell
    range   offsets (15, 20, 0) scaled to norms one float step either side of 25 and at 25 with max_range 25; a truncated ray
    rangeneg  the truncated ray's point with max_range < 0
    bounds  ends beyond +-3276.8 m; a scan whose origin is out of range; points that are not finite
    scene   the three 40 x 30 planes of tools/make_occupancy_fixtures.py through their poses, max_range 6
    clamp   eight scans of an 8 x 8 wall, then eight with the wall 1 m further back
    order_ab / order_ba   two scans in both orders, under a clamp_max below one hit, so that the results differ
    random  1024 rays from one origin, lengths 0 - 6 m, every second end on a voxel face; the seed is the first whose census has a ray that ends on the length test
    block / mixed   a full 2 x 2 x 2 block of free voxels under a far wall; the same with one voxel hit instead
"""
import numpy as np

import octomap_kit as kit
from octomap_kit import PROBS, RESOLUTION, bench, f32, occ, rc, up, voxel


def pts(*rows):
    return np.asarray(rows, np.float32).reshape(-1, 3)


def case(scans, timing=False, **probs):
    """scans: [(origin, points)]; probs: RayParams keywords."""
    return dict(params=rc.RayParams(**probs), timing=timing,
                scans=[(np.asarray(o, np.float32), np.asarray(p, np.float32).reshape(-1, 3)) for o, p in scans])


def clamp_planes():
    """Sixteen 8 x 8 planes at scale 40: a wall 2 m ahead eight times, then 3 m ahead eight times, through poses a few
    millimetres apart. The local transform only rotates, so a pixel's two rays are collinear and the second crosses the first's
    end point. -> (planes, poses, model, scale)"""
    rng = np.random.default_rng(5)
    planes = np.stack([np.full((8, 8), 16 * 24 if k < 8 else 16 * 16, np.int16) for k in range(16)])
    poses = np.tile(np.asarray(occ.pose_rows([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0])), (16, 1))
    poses[:, [3, 7, 11]] = rng.uniform(-0.004, 0.004, (16, 3)).astype(np.float32) + np.float32([0.01, 0.02, 0.03])
    return planes, poses, occ.model(cx=140.0, cy=140.0, local=[0, 0, 1, 0, -1, 0, 0, 0, 0, -1, 0, 0]), 40


def make_cases():
    cases = {}
    o = (0.02, -0.03, 0.04)
    cases["axes"] = case([(o, pts(np.add(o, np.multiply(d, 1.37)))) for d in
                          ((1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1))])
    c = voxel((3, -2, 5))
    ends = [np.add(c, np.multiply((sx, sy, sz), k * 0.1)) for k in (1, 2, 5) for sx in (1, -1) for sy in (1, -1) for sz in (1, -1)]
    ends += [np.add(c, np.multiply((1, 1, 0), k * 0.1)) for k in (1, 2, 5)]
    cases["ties"] = case([(c, pts(e)) for e in ends])
    cases["short"] = case([(c, pts(np.add(c, (0.02, -0.03, 0.01)))), (c, pts(np.add(c, (0.0, 0.1, 0.0))))])
    base = np.array([15, 20, 0], np.float32)
    eps = f32(2.0 ** -23)
    o = np.array([0.3, -0.2, 0.1], np.float32)
    far = [o + base * f32(a) for a in (1.0, 1 + eps, 1 - eps / 2, 1 + 2 * eps, 1 - eps)] + [base * f32(a) for a in (1.0, 1 + eps, 1 - eps / 2)]
    cases["range"] = case([(o, pts(p)) for p in far[:5]] + [((0, 0, 0), pts(p)) for p in far[5:]] + [(o, pts(o + base * f32(2)))],
                          max_range=25.0)
    cases["rangeneg"] = case([(o, pts(o + base * f32(2)))], max_range=-1.0)
    inside = pts((1.0, 0.5, -0.3))
    odd = pts((3300.0, 1.0, 0.0), (0.0, -3276.9, 2.0), (1.0, 2.0, up(3276.8)), (np.nan, 0, 0), (0, np.inf, 0), (1, 1, -np.inf))
    cases["bounds"] = case([((0, 0, 0), np.concatenate([odd, inside])), ((4000.0, 0, 0), np.concatenate([inside, pts((2.0, 0.1, 0.1))])),
                            ((0.5, 0.5, 0.5), np.concatenate([inside, odd]))])
    cases["bounds_range"] = case([((0, 0, 0), np.concatenate([odd[:3], inside]))], max_range=3.0)
    disp, poses, m = kit.scene("rays")
    cases["scene"] = case([(pose[[3, 7, 11]], rc.plane_points(d, 4, m, pose)) for d, pose in zip(disp, poses)], max_range=6.0)
    disp, poses, m, scale = clamp_planes()
    cases["clamp"] = case([(pose[[3, 7, 11]], rc.plane_points(d, scale, m, pose)) for d, pose in zip(disp, poses)])
    a = (c, pts(np.add(c, (0.8, 0.3, 0.1)), np.add(c, (0.5, -0.4, 0.2))))
    b = (c, pts(np.add(c, (1.6, 0.6, 0.2)), np.add(c, (1.0, -0.8, 0.4)), np.add(c, (0.4, 0.4, 0.4))))
    cases["order_ab"] = case([a, b], clamp_max=0.6)
    cases["order_ba"] = case([b, a], clamp_max=0.6)
    for seed in range(100):
        rng = np.random.default_rng(seed)
        d = rng.normal(size=(1024, 3))
        d /= np.linalg.norm(d, axis=1, keepdims=True)
        o = np.array([0.013, -0.027, 0.041], np.float32)
        p = o + d * rng.uniform(0, 6, (1024, 1))
        snap = rng.integers(0, 3, 1024)           # every second end lies on a voxel face of one axis, as nearly as a float can:
        for i in range(1, 1024, 2):               # there the float direction decides which of the two stops ends the ray
            p[i, snap[i]] = np.round(p[i, snap[i]] / RESOLUTION) * RESOLUTION
        p = p.astype(np.float32)
        census = {}
        rc.scan_sets(p, o, -1.0, RESOLUTION, census)
        if census.get(rc.LENGTH, 0) >= 1:
            break
    else:
        raise AssertionError("no seed gives a ray that ends on the length test")
    cases["random"] = case([(o, p)])
    cases["random"]["seed"], cases["random"]["census"] = seed, census
    # eight free voxels that are siblings (keys 32768 + {40, 41} on every axis), each crossed by a ray to a wall further on
    centre = voxel((-3, 40, 40))
    block = np.array([voxel((40 + i, 40 + j, 40 + k)) for i in (0, 1) for j in (0, 1) for k in (0, 1)])
    beyond = (centre + (block - centre) * 1.8).astype(np.float32)
    cases["block"] = case([(centre, beyond)])
    mixed = beyond.copy()
    mixed[5] = block[5]
    cases["mixed"] = case([(centre, mixed)])
    for r in bench.RANGES:
        cases[f"bench_{int(r)}"] = case([(o, p) for o, _, p in kit.bench_scans(1, r)], timing=True, max_range=r)
    return cases


def check_cases(cases):
    """What the cases claim about themselves, by the restatement."""
    def leaves(name):
        t = rc.Tree(cases[name]["params"], RESOLUTION)
        for o, p in cases[name]["scans"]:
            t.insert(p, o)
        return t.leaves()

    ab, ba = leaves("order_ab"), leaves("order_ba")
    assert np.array_equal(ab[0], ba[0]) and not np.array_equal(ab[1].view(np.uint32), ba[1].view(np.uint32)), "order: AB equals BA"
    _, v = leaves("clamp")
    t = rc.Tree()
    assert (v == t.cmin).any() and (v == t.cmax).any(), "clamp: a clamp is not reached"
    rays, ends = set(), set()
    for o, p in cases["scene"]["scans"]:
        f, e = rc.scan_sets(p, o, 6.0, RESOLUTION)
        raw = set()
        for q in p:
            r, _ = rc.ray_keys(o, q, RESOLUTION) if rc.norm(rc.sub3(q, o)) <= 6.0 else (None, None)
            raw.update(rc.pack3(k) for k in r or [])
        assert raw & e, "scene: no cell is free for one ray and the end point of another"
    k, v = leaves("block")
    want = {rc.pack3((32768 + 40 + i, 32768 + 40 + j, 32768 + 40 + kk)) for i in (0, 1) for j in (0, 1) for kk in (0, 1)}
    assert want <= {int(x) for x in k[v < 0]}, "block: the eight siblings are not all free"
    k, v = leaves("mixed")
    assert len(want & {int(x) for x in k[v > 0]}) == 1 and len(want & {int(x) for x in k[v < 0]}) == 7, "mixed: not 7 free + 1 occupied"


def main():
    args = kit.arguments(__doc__)
    cases = make_cases()
    check_cases(cases)

    def write(f):
        f.write(kit.ints(len(cases)))
        for c in cases.values():
            f.write(kit.head(c["params"]) + kit.ints(c["timing"]) + kit.scans([(o, c["params"].max_range, p) for o, p in c["scans"]]))

    code, raw = kit.run(kit.build(args.reference, "rays"), "rays", write)
    assert code == 0, code
    r = kit.Reader(raw)
    out = dict(resolution=np.float64(RESOLUTION), names=np.array([n for n, c in cases.items() if not c["timing"]]))
    report = []
    for name, c in cases.items():
        consts = r.take("<f4", 5).copy()
        counts, keys, values = [], [], []
        for _ in c["scans"]:
            n = r.one("<u4")
            counts.append(n)
            if c["timing"]:
                ms = r.one("<f8")
                out[f"{name.replace('bench_', 'bench_cpu_ms_')}"] = np.float64(ms)
                out[f"{name.replace('bench_', 'bench_leaves_')}"] = np.uint32(n)
                continue
            k, v = r.voxels(n)
            keys.append(k)
            values.append(v)
        size, bt = r.one("<u4"), r.stream()
        if c["timing"]:
            report.append(f"{name}: {ms:.1f} ms, {counts[0]} leaves")
            continue
        rp = c["params"]
        out[f"{name}_params"] = np.array([getattr(rp, k) for k in PROBS] + [rp.max_range], np.float64)
        out[f"{name}_constants"] = consts
        out[f"{name}_origins"] = np.stack([o for o, _ in c["scans"]]).astype(np.float32)
        out[f"{name}_points"] = np.concatenate([p for _, p in c["scans"]]).astype(np.float32)
        out[f"{name}_npoints"] = np.array([len(p) for _, p in c["scans"]], np.int32)
        out[f"{name}_nleaves"] = np.array(counts, np.uint32)
        out[f"{name}_keys"] = np.concatenate(keys)
        out[f"{name}_logodds"] = np.concatenate(values)
        out[f"{name}_size"] = np.uint32(size)
        out[f"{name}_bt"] = bt
        report.append(f"{name}: {len(c['scans'])} scans, {counts[-1]} leaves, {size} nodes, {len(bt)} B")
    r.done()
    out["random_seed"] = np.int32(cases["random"]["seed"])
    out["random_length_stops"] = np.int32(cases["random"]["census"][rc.LENGTH])
    disp, poses, m = kit.scene("rays")
    out["scene_disp"], out["scene_poses"], out["scene_model"], out["scene_scale"] = disp, poses, occ.model_to_array(m), np.int32(4)
    disp, poses, m, scale = clamp_planes()
    out["clamp_disp"], out["clamp_poses"], out["clamp_model"], out["clamp_scale"] = disp, poses, occ.model_to_array(m), np.int32(scale)
    OUT = kit.save(args.out, "rays", out, kit.numpy_npz)
    print(f"{OUT}: {OUT.stat().st_size} bytes\n  " + "\n  ".join(report))


if __name__ == "__main__":
    main()
