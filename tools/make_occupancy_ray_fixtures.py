#!/usr/bin/env python3
"""Writes tests/golden/occupancy_rays.npz (+ .sha256): what the reference's OWN octomap answers for
insertPointCloud(scan, origin, maxrange) on a few small scans -- after every scan the depth-16 leaves (key, float log-odds) of
the expanded tree, and at the end size() and the bytes of writeBinary -- together with the five log-odds constants of each
tree and the milliseconds octomap took for one plane of the benchmark's synthetic scan (tools/bench_occupancy_rays.py).

Run by hand, never by a test:

    python tools/make_occupancy_ray_fixtures.py --reference /path/to/U96-SLAM

It compiles the driver below (this project's text; it calls octomap's API only) against the octomap sources vendored in the
reference tree into a temporary directory, feeds it the scans and keeps only inputs and recorded outputs. The cases:

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
import argparse
import hashlib
import pathlib
import struct
import subprocess
import sys
import tempfile

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "oracle"))
sys.path.insert(0, str(ROOT / "tests"))
sys.path.insert(0, str(ROOT / "tools"))
import bench_occupancy_rays as bench  # noqa: E402
import make_occupancy_fixtures as hitfix  # noqa: E402
import occupancy_ray_cases as rc  # noqa: E402

OUT = ROOT / "tests" / "golden" / "occupancy_rays.npz"
RESOLUTION = 0.1
PROBS = ("prob_hit", "prob_miss", "clamp_min", "clamp_max", "occupancy_thres")

DRIVER = r"""
// Driver of tools/make_occupancy_ray_fixtures.py: insertPointCloud on recorded scans, the leaves after every scan.
#include <octomap/octomap.h>
#include <chrono>
#include <cstdio>
#include <cstdint>
#include <sstream>
#include <vector>

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* in = fopen(argv[1], "rb");
  FILE* out = fopen(argv[2], "wb");
  if (!in || !out) return 2;
  int32_t ncases;
  if (fread(&ncases, 4, 1, in) != 1) return 3;
  for (int c = 0; c < ncases; c++) {
    double prob[5], max_range, resolution;
    int32_t nscans, timing;
    if (fread(prob, 8, 5, in) != 5 || fread(&max_range, 8, 1, in) != 1 || fread(&resolution, 8, 1, in) != 1 ||
        fread(&nscans, 4, 1, in) != 1 || fread(&timing, 4, 1, in) != 1)
      return 3;
    octomap::OcTree tree(resolution);
    tree.setProbHit(prob[0]);
    tree.setProbMiss(prob[1]);
    tree.setClampingThresMin(prob[2]);
    tree.setClampingThresMax(prob[3]);
    tree.setOccupancyThres(prob[4]);
    float constants[5] = {tree.getProbHitLog(), tree.getProbMissLog(), tree.getClampingThresMinLog(), tree.getClampingThresMaxLog(),
                          tree.getOccupancyThresLog()};
    fwrite(constants, 4, 5, out);
    for (int s = 0; s < nscans; s++) {
      float o[3];
      int32_t n;
      if (fread(o, 4, 3, in) != 3 || fread(&n, 4, 1, in) != 1) return 3;
      std::vector<float> pts(3 * (size_t)n);
      if (fread(pts.data(), 4, pts.size(), in) != pts.size()) return 3;
      octomap::Pointcloud scan;
      for (int i = 0; i < n; i++) scan.push_back(pts[3 * i], pts[3 * i + 1], pts[3 * i + 2]);
      octomap::point3d origin(o[0], o[1], o[2]);
      auto t0 = std::chrono::steady_clock::now();
      tree.insertPointCloud(scan, origin, max_range);
      double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
      octomap::OcTree copy(tree);
      copy.expand();
      std::vector<uint16_t> keys;
      std::vector<float> values;
      for (octomap::OcTree::leaf_iterator it = copy.begin_leafs(), end = copy.end_leafs(); it != end; ++it) {
        if (it.getDepth() != 16) return 4;
        octomap::OcTreeKey k = it.getKey();
        keys.push_back(k[0]);
        keys.push_back(k[1]);
        keys.push_back(k[2]);
        values.push_back(it->getLogOdds());
      }
      uint32_t leaves = (uint32_t)values.size();
      fwrite(&leaves, 4, 1, out);
      if (timing) {
        fwrite(&ms, 8, 1, out);
      } else {
        fwrite(keys.data(), 2, keys.size(), out);
        fwrite(values.data(), 4, values.size(), out);
      }
    }
    std::ostringstream s;
    tree.writeBinary(s);
    std::string b = s.str();
    uint32_t size = (uint32_t)tree.size(), len = timing ? 0 : (uint32_t)b.size();
    fwrite(&size, 4, 1, out);
    fwrite(&len, 4, 1, out);
    fwrite(b.data(), 1, len, out);
  }
  fclose(out);
  return 0;
}
"""


def f32(v):
    return np.float32(v)


def pts(*rows):
    return np.asarray(rows, np.float32).reshape(-1, 3)


def case(scans, timing=False, **probs):
    """scans: [(origin, points)]; probs: RayParams keywords."""
    return dict(params=rc.RayParams(**probs), timing=timing,
                scans=[(np.asarray(o, np.float32), np.asarray(p, np.float32).reshape(-1, 3)) for o, p in scans])


def up(v):
    return np.nextafter(f32(v), f32(np.inf))


def clamp_planes():
    """Sixteen 8 x 8 planes at scale 40: a wall 2 m ahead eight times, then 3 m ahead eight times, through poses a few
    millimetres apart. The local transform only rotates, so a pixel's two rays are collinear and the second crosses the first's
    end point. -> (planes, poses, model, scale)"""
    rng = np.random.default_rng(5)
    planes = np.stack([np.full((8, 8), 16 * 24 if k < 8 else 16 * 16, np.int16) for k in range(16)])
    poses = np.tile(np.asarray(hitfix.occ.pose_rows([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0])), (16, 1))
    poses[:, [3, 7, 11]] = rng.uniform(-0.004, 0.004, (16, 3)).astype(np.float32) + np.float32([0.01, 0.02, 0.03])
    return planes, poses, hitfix.occ.model(cx=140.0, cy=140.0, local=[0, 0, 1, 0, -1, 0, 0, 0, 0, -1, 0, 0]), 40


def voxel(j):
    return (np.asarray(j, np.float64) + 0.5) * RESOLUTION


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
    disp, poses, m = hitfix.scene()
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
    planes, bposes = bench.synth_planes(1)
    cloud = rc.plane_points(planes[0], bench.SCALE, bench.synth_model(), bposes[0])
    for r in bench.RANGES:
        cases[f"bench_{int(r)}"] = case([(bposes[0][[3, 7, 11]], cloud)], timing=True, max_range=r)
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
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reference", required=True, help="checkout of the reference project (read only)")
    args = ap.parse_args()
    ref = pathlib.Path(args.reference) / "src" / "slam"
    cases = make_cases()
    check_cases(cases)
    with tempfile.TemporaryDirectory() as tmp:
        tmp = pathlib.Path(tmp)
        (tmp / "driver.cpp").write_text(DRIVER)
        srcs = sorted(str(p) for p in (ref / "src" / "octomap").glob("*.cpp"))
        subprocess.run(["g++", "-O1", "-std=c++11", "-I", str(ref / "include"), "-I", str(ref / "include" / "octomap"), "-o",
                        str(tmp / "driver"), str(tmp / "driver.cpp")] + srcs, check=True)
        with open(tmp / "in.bin", "wb") as f:
            f.write(struct.pack("<i", len(cases)))
            for c in cases.values():
                rp = c["params"]
                f.write(struct.pack("<7dii", *[getattr(rp, k) for k in PROBS], rp.max_range, RESOLUTION, len(c["scans"]), int(c["timing"])))
                for o, p in c["scans"]:
                    f.write(o.astype(np.float32).tobytes() + struct.pack("<i", len(p)) + p.astype(np.float32).tobytes())
        subprocess.run([str(tmp / "driver"), str(tmp / "in.bin"), str(tmp / "out.bin")], check=True, stderr=subprocess.DEVNULL)
        raw = (tmp / "out.bin").read_bytes()
    out = dict(resolution=np.float64(RESOLUTION), names=np.array([n for n, c in cases.items() if not c["timing"]]))
    off = 0
    report = []
    for name, c in cases.items():
        consts = np.frombuffer(raw, np.float32, 5, off).copy()
        off += 20
        counts, keys, values = [], [], []
        for _ in c["scans"]:
            (n,) = struct.unpack_from("<I", raw, off)
            off += 4
            counts.append(n)
            if c["timing"]:
                (ms,) = struct.unpack_from("<d", raw, off)
                off += 8
                out[f"{name.replace('bench_', 'bench_cpu_ms_')}"] = np.float64(ms)
                out[f"{name.replace('bench_', 'bench_leaves_')}"] = np.uint32(n)
                continue
            k = np.frombuffer(raw, np.uint16, 3 * n, off).reshape(n, 3).astype(np.uint64)
            off += 6 * n
            v = np.frombuffer(raw, np.float32, n, off)
            off += 4 * n
            packed = (k[:, 0] << np.uint64(32)) | (k[:, 1] << np.uint64(16)) | k[:, 2]
            order = np.argsort(packed)
            keys.append(packed[order])
            values.append(v[order])
        size, length = struct.unpack_from("<II", raw, off)
        off += 8
        bt = np.frombuffer(raw, np.uint8, length, off).copy()
        off += length
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
        report.append(f"{name}: {len(c['scans'])} scans, {counts[-1]} leaves, {size} nodes, {length} B")
    assert off == len(raw)
    out["random_seed"] = np.int32(cases["random"]["seed"])
    out["random_length_stops"] = np.int32(cases["random"]["census"][rc.LENGTH])
    disp, poses, m = hitfix.scene()
    out["scene_disp"], out["scene_poses"], out["scene_model"], out["scene_scale"] = disp, poses, hitfix.occ.model_to_array(m), np.int32(4)
    disp, poses, m, scale = clamp_planes()
    out["clamp_disp"], out["clamp_poses"], out["clamp_model"], out["clamp_scale"] = disp, poses, hitfix.occ.model_to_array(m), np.int32(scale)
    np.savez_compressed(OUT, **out)
    OUT.with_suffix(".sha256").write_text(hashlib.sha256(OUT.read_bytes()).hexdigest() + "  " + OUT.name + "\n")
    print(f"{OUT}: {OUT.stat().st_size} bytes\n  " + "\n  ".join(report))


if __name__ == "__main__":
    main()
