#!/usr/bin/env python3
"""Writes tests/golden/occupancy_tree.npz (+ .sha256): what the reference's OWN octomap holds above the voxels of a few small
trees -- every node of begin_tree(), begin_leafs(maxDepth) for maxDepth 0, 15, 14, 12, 8 and 1, calcNumNodes() and
getNumLeafNodes(), and search(point, depth) for depths 0, 16, 15, 14, 12, 8 and 1 -- once after updateInnerOccupancy(); prune();
(the LOGODDS reading) and once after toMaxLikelihood(); prune(); (the MAXLIKELIHOOD reading), there with the writeBinary stream.
Beside it, tests/golden/occupancy_tree_cpu.json holds octomap's milliseconds for updateInnerOccupancy + prune + writeBinary to
memory and for one full leaf iteration on the scene of tools/bench_occupancy_rays.py (kept out of the .npz so that the .npz
regenerates to the same bytes).

Run by hand, never by a test:

    python tools/make_occupancy_tree_fixtures.py --reference /path/to/U96-SLAM

It compiles the driver below (this project's text; it calls octomap's API only) against the octomap sources vendored in the
reference tree into a temporary directory, and keeps only inputs and recorded outputs. The generator asserts that the
transcription tests/occupancy_tree_cases.py reproduces every recorded value before it writes the file.

A scan whose origin has no key -- (1e6, 1e6, 1e6) at 0.1 m -- casts no ray, and every point of it still marks its own voxel as
occupied: that is how exact voxel sets are laid down, in octomap and through insert_cloud. Trees (log-odds, insertPointCloud,
unless said otherwise):

    one          a single voxel
    sib8         eight siblings hit once each: they collapse to depth 15
    sib8_mixed   the same eight, one of them hit twice: no collapse under LOGODDS, a collapse under MAXLIKELIHOOD
    cube64       a full depth-14 cube: collapses twice
    cube63       the same cube with one voxel missing
    straddle     the 2 x 2 x 2 voxels around key (32768, 32768, 32768): adjacent, not siblings; eight root children
    corners      the voxels at keys 0 and 65535 on every axis combination
    shift_k      k = 0..7: k lone voxels low in Morton order, then 640 complete sibling groups -- together a sibling-group
                 boundary at every position modulo 8
    box, scene   the scans of the same names in tests/golden/occupancy_query.npz: free leaves and mixed pruned blocks
    scene_hits   the hit-mode scene, recorded after toMaxLikelihood only
"""
import argparse
import hashlib
import json
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
import occupancy_ray_cases as rc  # noqa: E402
import occupancy_tree_cases as tc  # noqa: E402
from make_occupancy_query_fixtures import write_npz  # noqa: E402

OUT = ROOT / "tests" / "golden" / "occupancy_tree.npz"
CPU = ROOT / "tests" / "golden" / "occupancy_tree_cpu.json"
QUERY = ROOT / "tests" / "golden" / "occupancy_query.npz"
RESOLUTION = 0.1
PROBS = ("prob_hit", "prob_miss", "clamp_min", "clamp_max", "occupancy_thres")
MAX_DEPTHS = (0, 15, 14, 12, 8, 1)
SEARCH_DEPTHS = (0, 16, 15, 14, 12, 8, 1)
FAR = np.float32([1e6, 1e6, 1e6])           # an origin without a key
BENCH_PLANES, BENCH_RANGE = 4, 25.0
SHIFT_GROUPS, SHIFT_FIRST = 640, 1000       # complete sibling groups of a shift tree, and the first one's depth-15 Morton prefix

DRIVER = r"""
// Driver of tools/make_occupancy_tree_fixtures.py: trees from recorded scans or key lists, then what octomap holds above them.
#include <octomap/octomap.h>
#include <chrono>
#include <cstdio>
#include <cstdint>
#include <map>
#include <sstream>
#include <vector>

template <class T> static bool rd(FILE* f, T* p, size_t n) { return fread(p, sizeof(T), n, f) == n; }
template <class T> static void wr(FILE* f, const T& v) { fwrite(&v, sizeof(T), 1, f); }

static void node_out(FILE* out, const octomap::OcTreeKey& k, unsigned depth, float value) {
  uint16_t w[4] = {k[0], k[1], k[2], (uint16_t)depth};
  fwrite(w, 2, 4, out);
  wr(out, value);
}

static void record(octomap::OcTree& tree, const std::vector<float>& pts, FILE* out) {
  std::map<const octomap::OcTreeNode*, int> depth_of;
  std::vector<uint8_t> leaf;
  uint32_t n = 0;
  for (octomap::OcTree::tree_iterator it = tree.begin_tree(), end = tree.end_tree(); it != end; ++it) n++;
  wr(out, n);
  for (octomap::OcTree::tree_iterator it = tree.begin_tree(), end = tree.end_tree(); it != end; ++it) {
    node_out(out, it.getKey(), it.getDepth(), it->getLogOdds());
    leaf.push_back(it.isLeaf() ? 1 : 0);
    depth_of[&(*it)] = (int)it.getDepth();
  }
  fwrite(leaf.data(), 1, leaf.size(), out);
  const int max_depths[6] = {0, 15, 14, 12, 8, 1};
  for (int md : max_depths) {
    n = 0;
    for (octomap::OcTree::leaf_iterator it = tree.begin_leafs(md), end = tree.end_leafs(); it != end; ++it) n++;
    wr(out, n);
    for (octomap::OcTree::leaf_iterator it = tree.begin_leafs(md), end = tree.end_leafs(); it != end; ++it)
      node_out(out, it.getKey(), it.getDepth(), it->getLogOdds());
  }
  wr(out, (uint64_t)tree.calcNumNodes());
  wr(out, (uint64_t)tree.getNumLeafNodes());
  const int depths[7] = {0, 16, 15, 14, 12, 8, 1};
  for (int d : depths)
    for (size_t i = 0; i < pts.size() / 3; i++) {
      octomap::OcTreeNode* node = tree.search(octomap::point3d(pts[3 * i], pts[3 * i + 1], pts[3 * i + 2]), d);
      int32_t found = node ? 1 : 0, depth = node ? depth_of.at(node) : -1;
      float value = node ? node->getLogOdds() : 0.f;
      wr(out, found);
      wr(out, value);
      wr(out, depth);
    }
}

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* in = fopen(argv[1], "rb");
  FILE* out = fopen(argv[2], "wb");
  if (!in || !out) return 2;
  int32_t ntrees;
  if (!rd(in, &ntrees, 1)) return 3;
  for (int t = 0; t < ntrees; t++) {
    double prob[5], resolution;
    int32_t hits, nscans, timing, npoints;
    if (!rd(in, prob, 5) || !rd(in, &resolution, 1) || !rd(in, &hits, 1) || !rd(in, &timing, 1) || !rd(in, &nscans, 1)) return 3;
    octomap::OcTree tree(resolution);
    tree.setProbHit(prob[0]);
    tree.setProbMiss(prob[1]);
    tree.setClampingThresMin(prob[2]);
    tree.setClampingThresMax(prob[3]);
    tree.setOccupancyThres(prob[4]);
    float constants[5] = {tree.getProbHitLog(), tree.getProbMissLog(), tree.getClampingThresMinLog(), tree.getClampingThresMaxLog(),
                          tree.getOccupancyThresLog()};
    fwrite(constants, 4, 5, out);
    if (hits) {       // nscans counts keys, each with its number of hits
      std::vector<uint16_t> k(3 * (size_t)nscans);
      std::vector<uint32_t> c(nscans);
      if (!rd(in, k.data(), k.size()) || !rd(in, c.data(), c.size())) return 3;
      for (int i = 0; i < nscans; i++)
        for (uint32_t j = 0; j < c[i]; j++) tree.updateNode(octomap::OcTreeKey(k[3 * i], k[3 * i + 1], k[3 * i + 2]), true);
    } else {
      for (int s = 0; s < nscans; s++) {
        float o[3];
        double max_range;
        int32_t n;
        if (!rd(in, o, 3) || !rd(in, &max_range, 1) || !rd(in, &n, 1)) return 3;
        std::vector<float> pts(3 * (size_t)n);
        if (!rd(in, pts.data(), pts.size())) return 3;
        octomap::Pointcloud scan;
        for (int i = 0; i < n; i++) scan.push_back(pts[3 * i], pts[3 * i + 1], pts[3 * i + 2]);
        tree.insertPointCloud(scan, octomap::point3d(o[0], o[1], o[2]), max_range);
      }
    }
    if (!rd(in, &npoints, 1)) return 3;
    std::vector<float> pts(3 * (size_t)npoints);
    if (!rd(in, pts.data(), pts.size())) return 3;
    if (timing) {     // octomap's own time for what the device tree replaces
      tree.expand();  // from the voxels, as the device starts
      auto t0 = std::chrono::steady_clock::now();
      tree.updateInnerOccupancy();
      tree.prune();
      std::ostringstream s;
      tree.writeBinary(s);
      double write_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
      t0 = std::chrono::steady_clock::now();
      uint64_t leaves = 0;
      for (octomap::OcTree::leaf_iterator it = tree.begin_leafs(), end = tree.end_leafs(); it != end; ++it) leaves++;
      double iterate_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
      uint64_t voxels = 0;
      tree.expand();
      for (octomap::OcTree::leaf_iterator it = tree.begin_leafs(), end = tree.end_leafs(); it != end; ++it) voxels++;
      wr(out, write_ms);
      wr(out, iterate_ms);
      wr(out, leaves);
      wr(out, voxels);
      wr(out, (uint64_t)s.str().size());
      continue;
    }
    {                 // the voxels: the leaves of an expanded copy
      octomap::OcTree copy(tree);
      copy.expand();
      uint32_t n = 0;
      for (octomap::OcTree::leaf_iterator it = copy.begin_leafs(), end = copy.end_leafs(); it != end; ++it) n++;
      wr(out, n);
      for (octomap::OcTree::leaf_iterator it = copy.begin_leafs(), end = copy.end_leafs(); it != end; ++it) {
        if (it.getDepth() != 16) return 4;
        node_out(out, it.getKey(), 16, it->getLogOdds());
      }
    }
    if (!hits) {
      tree.updateInnerOccupancy();
      tree.prune();
      record(tree, pts, out);
    }
    tree.toMaxLikelihood();
    tree.prune();
    record(tree, pts, out);
    std::ostringstream s;
    tree.writeBinaryConst(s);
    const std::string bt = s.str();
    wr(out, (uint32_t)bt.size());
    fwrite(bt.data(), 1, bt.size(), out);
  }
  fclose(out);
  return 0;
}
"""


def centres(keys):
    """keyToCoord of (n, 3) keys as float32 points"""
    return ((np.asarray(keys, np.float64) - 32768 + 0.5) * RESOLUTION).astype(np.float32)


def unmorton_keys(codes):
    return np.array([tc.unmorton(int(c)) for c in codes], np.int64).reshape(-1, 3)


def key_scans(*key_lists):
    return [(FAR, -1.0, centres(k)) for k in key_lists]


def probe_points(keys, rng):
    """A small search set for a tree laid down from keys: voxel centres, their neighbours, points nowhere near, no key"""
    keys = np.asarray(keys, np.int64).reshape(-1, 3)
    take = keys[np.unique(np.linspace(0, len(keys) - 1, 24).astype(int))]
    near = np.clip(take + rng.integers(-2, 3, take.shape), 0, 65535)
    far = np.array([[32768, 32768, 32768], [0, 0, 0], [65535, 65535, 65535], [100, 40000, 7], [32767, 32768, 32769]])
    pts = centres(np.concatenate([take, near, far]))
    odd = np.float32([[np.nan, 0, 0], [0, np.inf, 0], [3276.85, 0, 0], [0, 0, -3276.81]])
    return np.concatenate([pts, odd]).astype(np.float32)


def make_trees():
    rng = np.random.default_rng(41)
    q = dict(np.load(QUERY))
    trees = {}

    def add(name, *key_lists):
        trees[name] = dict(params=rc.RayParams(), scans=key_scans(*key_lists), scan_keys=[np.asarray(k, np.uint16) for k in key_lists],
                           points=probe_points(np.concatenate(key_lists), rng))

    sib = np.array([(32770 + x, 32772 + y, 32774 + z) for z in (0, 1) for y in (0, 1) for x in (0, 1)])
    cube = np.array([(33000 + x, 32500 + y, 32900 + z) for z in range(4) for y in range(4) for x in range(4)])
    add("one", [(32773, 32765, 32775)])
    add("sib8", sib)
    add("sib8_mixed", sib, sib[5:6])
    add("cube64", cube)
    add("cube63", np.delete(cube, 37, axis=0))
    add("straddle", [(32767 + x, 32767 + y, 32767 + z) for z in (0, 1) for y in (0, 1) for x in (0, 1)])
    add("corners", [(x, y, z) for z in (0, 65535) for y in (0, 65535) for x in (0, 65535)])
    groups = unmorton_keys(np.arange(8 * SHIFT_FIRST, 8 * (SHIFT_FIRST + SHIFT_GROUPS)))
    for k in range(8):
        add(f"shift_{k}", np.concatenate([unmorton_keys(8 * np.arange(k)), groups]))
    for name in ("box", "scene"):
        n = q[f"{name}_npoints"]
        ends = np.cumsum(n)
        scans = [(q[f"{name}_origins"][i], float(q[f"{name}_scan_range"][i]), q[f"{name}_points"][e - k:e]) for i, (k, e) in enumerate(zip(n, ends))]
        trees[name] = dict(params=rc.RayParams(*[float(v) for v in q[f"{name}_params"]]), scans=scans, points=q[f"{name}_search_points"])
    trees["scene_hits"] = dict(params=rc.RayParams(), hit_keys=q["scene_hits_keys"], hit_counts=q["scene_hits_counts"],
                               points=q["scene_hits_search_points"])
    planes, poses = bench.synth_planes(BENCH_PLANES)
    bm = bench.synth_model()
    trees["bench"] = dict(params=rc.RayParams(), timing=True, points=np.zeros((0, 3), np.float32),
                          scans=[(pose[[3, 7, 11]], BENCH_RANGE, rc.plane_points(pl, bench.SCALE, bm, pose)) for pl, pose in zip(planes, poses)])
    return trees


class Reader:
    def __init__(self, raw):
        self.raw, self.off = raw, 0

    def take(self, dtype, n=1):
        a = np.frombuffer(self.raw, dtype, n, self.off)
        self.off += a.nbytes
        return a

    def nodes(self, n):
        rec = self.take(np.dtype([("k", "<u2", 3), ("depth", "<u2"), ("value", "<f4")]), n)
        k = rec["k"].astype(np.uint64).reshape(-1, 3)
        return (k[:, 0] << np.uint64(32)) | (k[:, 1] << np.uint64(16)) | k[:, 2], rec["depth"].astype(np.int32), rec["value"].copy()

    def stage(self, npoints):
        """what record() wrote -> dict of arrays"""
        out = {}
        n = int(self.take("<u4")[0])
        out["tree_key"], out["tree_depth"], out["tree_value"] = self.nodes(n)
        out["tree_leaf"] = self.take(np.uint8, n).copy()
        for md in MAX_DEPTHS:
            n = int(self.take("<u4")[0])
            out[f"leafs{md}_key"], out[f"leafs{md}_depth"], out[f"leafs{md}_value"] = self.nodes(n)
        out["num_nodes"], out["num_leaves"] = (np.uint64(v) for v in self.take("<u8", 2))
        for d in SEARCH_DEPTHS:
            rec = self.take(np.dtype([("found", "<i4"), ("value", "<u4"), ("depth", "<i4")]), npoints)
            out[f"search{d}_found"] = rec["found"].astype(np.uint8)
            out[f"search{d}_value"] = rec["value"].copy()
            out[f"search{d}_depth"] = rec["depth"].astype(np.int8)
        return out


def pack_stage(rec):
    """One reading's records as few arrays: the six leaf lists end to end with their lengths, the seven searches as rows.
    tests/occupancy_tree_cases.py unpack_stage is the inverse."""
    out = {k: rec[k] for k in ("tree_key", "tree_value", "tree_leaf", "num_nodes", "num_leaves")}
    out["tree_depth"] = rec["tree_depth"].astype(np.uint8)
    out["leafs_n"] = np.array([len(rec[f"leafs{md}_key"]) for md in MAX_DEPTHS], np.int32)
    for k, dt in (("key", np.uint64), ("depth", np.uint8), ("value", np.float32)):
        out[f"leafs_{k}"] = np.concatenate([rec[f"leafs{md}_{k}"] for md in MAX_DEPTHS]).astype(dt)
    for k in ("found", "value", "depth"):
        out[f"search_{k}"] = np.stack([rec[f"search{d}_{k}"] for d in SEARCH_DEPTHS])
    return out


def check_stage(name, rec, tree, points, thres):
    """The transcription reproduces everything octomap recorded for one reading"""
    keys, depth, value, leaf = tree.all_nodes()
    same = lambda a, b: np.array_equal(np.asarray(a), np.asarray(b))   # noqa: E731
    assert same(keys, rec["tree_key"]) and same(depth, rec["tree_depth"]) and same(leaf, rec["tree_leaf"]), (name, "begin_tree")
    assert same(value.view(np.uint32), rec["tree_value"].view(np.uint32)), (name, "begin_tree values")
    assert tree.size == int(rec["num_nodes"]) and tree.num_leaves == int(rec["num_leaves"]), (name, "counts")
    for md in MAX_DEPTHS:
        k, d, v = tree.leaves(md)
        assert same(k, rec[f"leafs{md}_key"]) and same(d, rec[f"leafs{md}_depth"]), (name, "begin_leafs", md)
        assert same(v.view(np.uint32), rec[f"leafs{md}_value"].view(np.uint32)), (name, "begin_leafs values", md)
    for sd in SEARCH_DEPTHS:
        state, bits, found = tree.search_all(points, sd, thres)
        hit = rec[f"search{sd}_found"].astype(bool)
        assert same(state > 0, hit), (name, "search found", sd)
        assert same(bits[hit], rec[f"search{sd}_value"][hit]) and same(found, rec[f"search{sd}_depth"]), (name, "search", sd)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reference", required=True, help="checkout of the reference project (read only)")
    args = ap.parse_args()
    ref = pathlib.Path(args.reference) / "src" / "slam"
    trees = make_trees()
    q_fixture = dict(np.load(QUERY))
    with tempfile.TemporaryDirectory() as tmp:
        tmp = pathlib.Path(tmp)
        (tmp / "driver.cpp").write_text(DRIVER)
        srcs = sorted(str(p) for p in (ref / "src" / "octomap").glob("*.cpp"))
        subprocess.run(["g++", "-O1", "-std=c++11", "-I", str(ref / "include"), "-I", str(ref / "include" / "octomap"), "-o",
                        str(tmp / "driver"), str(tmp / "driver.cpp")] + srcs, check=True)
        with open(tmp / "in.bin", "wb") as f:
            f.write(struct.pack("<i", len(trees)))
            for t in trees.values():
                rp = t["params"]
                hits = "hit_keys" in t
                f.write(struct.pack("<6diii", *[getattr(rp, k) for k in PROBS], RESOLUTION, int(hits), int(t.get("timing", False)),
                                    len(t["hit_keys"] if hits else t["scans"])))
                if hits:
                    k = np.asarray(t["hit_keys"], np.uint64)
                    k3 = np.stack([(k >> np.uint64(32)) & np.uint64(0xFFFF), (k >> np.uint64(16)) & np.uint64(0xFFFF), k & np.uint64(0xFFFF)], 1)
                    f.write(k3.astype(np.uint16).tobytes() + np.asarray(t["hit_counts"], np.uint32).tobytes())
                else:
                    for o, mr, p in t["scans"]:
                        f.write(np.asarray(o, np.float32).tobytes() + struct.pack("<di", mr, len(p)) + np.asarray(p, np.float32).tobytes())
                f.write(struct.pack("<i", len(t["points"])) + np.asarray(t["points"], np.float32).tobytes())
        subprocess.run([str(tmp / "driver"), str(tmp / "in.bin"), str(tmp / "out.bin")], check=True, stderr=subprocess.DEVNULL)
        raw = (tmp / "out.bin").read_bytes()
    out = dict(resolution=np.float64(RESOLUTION), trees=np.array([n for n, t in trees.items() if not t.get("timing")]),
               max_depths=np.array(MAX_DEPTHS, np.int32), search_depths=np.array(SEARCH_DEPTHS, np.int32), far_origin=FAR)
    r, report, cpu = Reader(raw), [], {}
    for name, t in trees.items():
        consts = r.take("<f4", 5).copy()
        if t.get("timing"):
            write_ms, iterate_ms = (float(v) for v in r.take("<f8", 2))
            leaves, voxels, nbytes = (int(v) for v in r.take("<u8", 3))
            cpu = dict(scene="tools/bench_occupancy_rays.py synth_planes", planes=BENCH_PLANES, insert_max_range=BENCH_RANGE, voxels=voxels,
                       pruned_leaves=leaves, bt_bytes=nbytes, octomap_inner_prune_write_ms=write_ms, octomap_leaf_iteration_ms=iterate_ms,
                       note="octomap's updateInnerOccupancy + prune + writeBinary to memory from the expanded tree, and one "
                            "begin_leafs() pass over the pruned tree; one thread, -O1, on the CPU of the machine that made the fixture")
            report.append(f"{name}: {voxels} voxels, {write_ms:.1f} ms to the stream, {iterate_ms:.1f} ms per leaf iteration")
            continue
        hits = "hit_keys" in t
        n = int(r.take("<u4")[0])
        vk, _, vv = r.nodes(n)
        order = np.argsort(vk)
        vk, vv = vk[order], vv[order]
        if hits:
            voxels = {int(k): int(c) for k, c in zip(t["hit_keys"], t["hit_counts"])}
            assert np.array_equal(vk, np.array(sorted(voxels), np.uint64)), (name, "keys")
        else:
            m = rc.Tree(t["params"], RESOLUTION)
            for o, mr, p in t["scans"]:
                m.rp.max_range = mr
                m.insert(p, o)
            voxels = dict(m.v)
            assert np.array_equal(vk, np.array(sorted(voxels), np.uint64)), (name, "keys")
            assert np.array_equal(vv.view(np.uint32), np.array([voxels[int(k)] for k in vk], np.float32).view(np.uint32)), (name, "values")
            out[f"{name}_logodds"] = vv
        out[f"{name}_keys"] = vk
        out[f"{name}_hits"] = np.int32(hits)
        out[f"{name}_params"] = np.array([getattr(t["params"], k) for k in PROBS], np.float64)
        out[f"{name}_constants"] = consts
        out[f"{name}_points"] = np.asarray(t["points"], np.float32)
        if "scan_keys" in t and len(t["scan_keys"]) > 1:      # a tree of one key-less-origin scan is laid down from its keys
            out[f"{name}_scan_keys"] = np.concatenate(t["scan_keys"]).astype(np.uint16)
            out[f"{name}_scan_n"] = np.array([len(k) for k in t["scan_keys"]], np.int32)
        npts = len(t["points"])
        readings = ([] if hits else [("lo", tc.Tree({k: v for k, v in voxels.items()}, RESOLUTION))]) + \
                   [("ml", tc.Tree(tc.max_likelihood(voxels, tc.HITS if hits else tc.LOGODDS_MODE, consts), RESOLUTION))]
        for tag, tree in readings:
            rec = r.stage(npts)
            check_stage((name, tag), rec, tree, t["points"], consts[4])
            back = tc.unpack_stage({f"{name}_{tag}_{k}": v for k, v in pack_stage(rec).items()}, name, tag, MAX_DEPTHS, SEARCH_DEPTHS)
            assert all(np.array_equal(back[k], v) for k, v in rec.items()), (name, tag, "packing")
            for k, v in pack_stage(rec).items():
                out[f"{name}_{tag}_{k}"] = v
        nbt = int(r.take("<u4")[0])
        bt = r.take(np.uint8, nbt).copy()
        assert readings[-1][1].stream(consts[3]) == bt.tobytes(), (name, "writeBinary")
        out[f"{name}_bt"] = bt
        ml = readings[-1][1]
        report.append(f"{name}: {len(vk)} voxels, {ml.size} nodes / {ml.num_leaves} leaves after toMaxLikelihood" +
                      ("" if hits else f", {readings[0][1].size} / {readings[0][1].num_leaves} before"))
    assert r.off == len(raw)
    assert int(out["sib8_lo_num_nodes"]) == 16 and int(out["sib8_mixed_lo_num_nodes"]) == 24 and int(out["sib8_mixed_ml_num_nodes"]) == 16
    assert int(out["cube64_lo_num_leaves"]) == 1 and out["cube64_lo_tree_depth"].max() == 14
    for name in ("box", "scene"):          # the voxels are those of the query fixture, which the tests build the maps from
        assert np.array_equal(out.pop(f"{name}_keys"), q_fixture[f"{name}_keys"])
        assert np.array_equal(out.pop(f"{name}_logodds").view(np.uint32), q_fixture[f"{name}_logodds"].view(np.uint32))
    assert np.array_equal(out.pop("scene_hits_keys"), q_fixture["scene_hits_keys"])
    assert int(out["straddle_lo_num_nodes"]) == 1 + 8 * 16
    write_npz(OUT, out)
    OUT.with_suffix(".sha256").write_text(hashlib.sha256(OUT.read_bytes()).hexdigest() + "  " + OUT.name + "\n")
    CPU.write_text(json.dumps(cpu, indent=1) + "\n")
    print(f"{OUT}: {OUT.stat().st_size} bytes\n  " + "\n  ".join(report))


if __name__ == "__main__":
    main()
