#!/usr/bin/env python3
"""Writes tests/golden/occupancy_load.npz (+ .sha256): what the reference's OWN octomap holds after readBinary of every .bt stream
the other occupancy fixtures recorded (the 18 of occupancy_tree.npz, the 14 of occupancy_rays.npz, the 3 of
occupancy_octomap.npz), of a size-1 stream, and of the malformed streams of tests/occupancy_load_cases.py -- readBinary's return
value, size() and calcNumNodes(), every leaf of begin_leafs() (centre key, depth, value bits), search(point) for the points
recorded beside a tree, and for three trees the leaves again after one more insertPointCloud scan on the loaded tree. Beside it,
tests/golden/occupancy_load_cpu.json holds octomap's milliseconds for readBinary on the scene of tools/bench_occupancy_tree.py
(kept out of the .npz so that the .npz regenerates to the same bytes).

Run by hand, never by a test:

    python tools/make_occupancy_load_fixtures.py --reference /path/to/U96-SLAM

It compiles the driver below (this project's text; it calls octomap's API only) against the octomap sources vendored in the
reference tree into a temporary directory, and keeps only inputs and recorded outputs. The input streams themselves are not stored
again: a stream is named by the fixture and member that holds it. The generator asserts that the transcription
tests/occupancy_load_cases.py reproduces every recorded value before it writes the file.

octomap's verdict on a malformed stream is recorded, not required: it reads an OcTree whatever the id says, reads the legacy
header, does not bound the depth, and past the end of a stream reads two bytes it never set. Every malformed stream runs in a
process of its own; -1 stands for a run that ended without a verdict.
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
import occupancy_load_cases as lc  # noqa: E402
import occupancy_ray_cases as rc  # noqa: E402
from make_occupancy_query_fixtures import write_npz  # noqa: E402

GOLDEN = ROOT / "tests" / "golden"
OUT = GOLDEN / "occupancy_load.npz"
CPU = GOLDEN / "occupancy_load_cpu.json"
RESOLUTION = 0.1
POST = {"tree_scene": 1, "tree_box": 0, "rays_clamp": 2}     # the scan of occupancy_rays.npz "scene" inserted after the load
NO_FILE = 0xFFFFFFFF

DRIVER = r"""
// Driver of tools/make_occupancy_load_fixtures.py: readBinary of recorded streams, then what octomap holds.
#include <octomap/octomap.h>
#include <chrono>
#include <cstdio>
#include <cstdint>
#include <sstream>
#include <string>
#include <vector>

template <class T> static bool rd(FILE* f, T* p, size_t n) { return fread(p, sizeof(T), n, f) == n; }
template <class T> static void wr(FILE* f, const T& v) { fwrite(&v, sizeof(T), 1, f); }

static void leaves_out(octomap::OcTree& tree, FILE* out) {
  uint32_t n = 0;
  for (octomap::OcTree::leaf_iterator it = tree.begin_leafs(), end = tree.end_leafs(); it != end; ++it) n++;
  wr(out, n);
  for (octomap::OcTree::leaf_iterator it = tree.begin_leafs(), end = tree.end_leafs(); it != end; ++it) {
    const octomap::OcTreeKey k = it.getKey();
    uint16_t w[4] = {k[0], k[1], k[2], (uint16_t)it.getDepth()};
    fwrite(w, 2, 4, out);
    wr(out, (float)it->getLogOdds());
  }
}

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* in = fopen(argv[1], "rb");
  FILE* out = fopen(argv[2], "wb");
  if (!in || !out) return 2;
  int32_t nstreams;
  if (!rd(in, &nstreams, 1)) return 3;
  for (int t = 0; t < nstreams; t++) {
    double prob[5], resolution;
    uint32_t nbytes;
    int32_t timing, npoints, post;
    if (!rd(in, prob, 5) || !rd(in, &resolution, 1) || !rd(in, &timing, 1) || !rd(in, &nbytes, 1)) return 3;
    octomap::OcTree tree(resolution);
    tree.setProbHit(prob[0]);
    tree.setProbMiss(prob[1]);
    tree.setClampingThresMin(prob[2]);
    tree.setClampingThresMax(prob[3]);
    tree.setOccupancyThres(prob[4]);
    if (timing) {       // nbytes counts scans: build the scene, write it, and time reading it back
      for (uint32_t s = 0; s < nbytes; s++) {
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
      std::ostringstream s;
      tree.writeBinary(s);
      const std::string bt = s.str();
      double best = 1e300;
      uint64_t nodes = 0, voxels = 0;
      for (int rep = 0; rep < 5; rep++) {
        octomap::OcTree back(resolution);
        std::istringstream is(bt);
        auto t0 = std::chrono::steady_clock::now();
        const bool ok = back.readBinary(is);
        const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        if (!ok) return 5;
        if (ms < best) best = ms;
        nodes = back.size();
      }
      tree.expand();
      for (octomap::OcTree::leaf_iterator it = tree.begin_leafs(), end = tree.end_leafs(); it != end; ++it) voxels++;
      wr(out, best);
      wr(out, nodes);
      wr(out, voxels);
      wr(out, (uint64_t)bt.size());
      continue;
    }
    bool ok;
    if (nbytes == 0xFFFFFFFFu) {
      ok = tree.readBinary(std::string(argv[2]) + ".does-not-exist");
    } else {
      std::string bt(nbytes, '\0');
      if (nbytes && !rd(in, &bt[0], nbytes)) return 3;
      std::istringstream is(bt);
      ok = tree.readBinary(is);
    }
    if (!rd(in, &npoints, 1)) return 3;
    std::vector<float> pts(3 * (size_t)npoints);
    if (!rd(in, pts.data(), pts.size())) return 3;
    if (!rd(in, &post, 1)) return 3;
    wr(out, (int32_t)(ok ? 1 : 0));
    wr(out, (uint64_t)tree.size());
    wr(out, (uint64_t)tree.calcNumNodes());
    if (ok) {
      leaves_out(tree, out);
      for (int i = 0; i < npoints; i++) {
        octomap::OcTreeNode* node = tree.search(octomap::point3d(pts[3 * i], pts[3 * i + 1], pts[3 * i + 2]));
        wr(out, (int32_t)(node ? 1 : 0));
        wr(out, (float)(node ? node->getLogOdds() : 0.f));
      }
    }
    if (post) {
      float o[3];
      double max_range;
      int32_t n;
      if (!rd(in, o, 3) || !rd(in, &max_range, 1) || !rd(in, &n, 1)) return 3;
      std::vector<float> sp(3 * (size_t)n);
      if (!rd(in, sp.data(), sp.size())) return 3;
      octomap::Pointcloud scan;
      for (int i = 0; i < n; i++) scan.push_back(sp[3 * i], sp[3 * i + 1], sp[3 * i + 2]);
      tree.insertPointCloud(scan, octomap::point3d(o[0], o[1], o[2]), max_range);
      leaves_out(tree, out);
    }
  }
  fclose(out);
  return 0;
}
"""


def sources():
    """{stream id: (bytes, five probabilities, search points)} of the 35 recorded streams, in a fixed order"""
    tree, rays, octo = (dict(np.load(GOLDEN / f"occupancy_{n}.npz")) for n in ("tree", "rays", "octomap"))
    default = [getattr(rc.RayParams(), k) for k in ("prob_hit", "prob_miss", "clamp_min", "clamp_max", "occupancy_thres")]
    out = {}
    for name in (str(n) for n in tree["trees"]):
        out[f"tree_{name}"] = (tree[f"{name}_bt"].tobytes(), [float(v) for v in tree[f"{name}_params"][:5]], tree[f"{name}_points"])
    for name in (str(n) for n in rays["names"]):
        out[f"rays_{name}"] = (rays[f"{name}_bt"].tobytes(), [float(v) for v in rays[f"{name}_params"][:5]], np.zeros((0, 3), np.float32))
    for name in ("all", "blocks", "empty"):
        out[f"octomap_{name}"] = (octo[f"bt_{name}"].tobytes(), default, np.zeros((0, 3), np.float32))
    assert len(out) == 35
    return out, rays


def scan_of(rays, index):
    n = rays["scene_npoints"]
    ends = np.cumsum(n)
    return rays["scene_origins"][index], float(rays["scene_params"][5]), rays["scene_points"][ends[index] - n[index]:ends[index]]


def record(f, probs, data, points, post=None, timing=None):
    f.write(struct.pack("<6di", *probs, RESOLUTION, int(timing is not None)))
    if timing is not None:
        f.write(struct.pack("<I", len(timing)))
        for o, mr, p in timing:
            f.write(np.asarray(o, np.float32).tobytes() + struct.pack("<di", mr, len(p)) + np.asarray(p, np.float32).tobytes())
        return
    f.write(struct.pack("<I", NO_FILE if data is None else len(data)) + (data or b""))
    f.write(struct.pack("<i", len(points)) + np.asarray(points, np.float32).tobytes())
    f.write(struct.pack("<i", int(post is not None)))
    if post is not None:
        o, mr, p = post
        f.write(np.asarray(o, np.float32).tobytes() + struct.pack("<di", mr, len(p)) + np.asarray(p, np.float32).tobytes())


class Reader:
    def __init__(self, raw):
        self.raw, self.off = raw, 0

    def take(self, dtype, n=1):
        a = np.frombuffer(self.raw, dtype, n, self.off)
        self.off += a.nbytes
        return a

    def leaves(self):
        rec = self.take(np.dtype([("k", "<u2", 3), ("depth", "<u2"), ("value", "<f4")]), int(self.take("<u4")[0]))
        k = rec["k"].astype(np.uint64).reshape(-1, 3)
        return (k[:, 0] << np.uint64(32)) | (k[:, 1] << np.uint64(16)) | k[:, 2], rec["depth"].astype(np.uint8), rec["value"].copy()


def run(driver, tmp, tag, write):
    with open(tmp / f"{tag}.in", "wb") as f:
        write(f)
    r = subprocess.run([str(driver), str(tmp / f"{tag}.in"), str(tmp / f"{tag}.out")], stderr=subprocess.DEVNULL, timeout=600)
    return r.returncode, (tmp / f"{tag}.out").read_bytes()


def bits(a):
    return np.asarray(a, np.float32).view(np.uint32)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reference", required=True, help="checkout of the reference project (read only)")
    args = ap.parse_args()
    ref = pathlib.Path(args.reference) / "src" / "slam"
    good, rays = sources()
    default = good["octomap_all"][1]
    good["size1"] = (lc.stream(1, bytes((0, 0))), default, np.float32([[0.05, 0.05, 0.05], [-300.0, 12.0, 7.0], [np.nan, 0, 0]]))
    bad = lc.malformed(good["tree_scene"][0])
    import make_occupancy_tree_fixtures as tree_tool
    bench = tree_tool.make_trees()["bench"]
    with tempfile.TemporaryDirectory() as tmp:
        tmp = pathlib.Path(tmp)
        (tmp / "driver.cpp").write_text(DRIVER)
        srcs = sorted(str(p) for p in (ref / "src" / "octomap").glob("*.cpp"))
        subprocess.run(["g++", "-O1", "-std=c++11", "-I", str(ref / "include"), "-I", str(ref / "include" / "octomap"), "-o",
                        str(tmp / "driver"), str(tmp / "driver.cpp")] + srcs, check=True)

        def write_good(f):
            f.write(struct.pack("<i", len(good) + 1))
            for name, (data, probs, points) in good.items():
                record(f, probs, data, points, scan_of(rays, POST[name]) if name in POST else None)
            record(f, default, None, None, timing=bench["scans"])

        code, raw = run(tmp / "driver", tmp, "good", write_good)
        assert code == 0, code
        verdicts = {}
        for name, (data, _) in list(bad.items()) + [("no_file", (None, lc.UNSUPPORTED))]:
            code, out = run(tmp / "driver", tmp, name, lambda f: (f.write(struct.pack("<i", 1)), record(f, default, data, np.zeros((0, 3)))))
            verdicts[name] = int(np.frombuffer(out, "<i4", 1)[0]) if code == 0 and len(out) >= 4 else -1
    out = dict(resolution=np.float64(RESOLUTION), streams=np.array(list(good)), malformed=np.array(list(bad)),
               post_scan=np.array([f"{k}:{v}" for k, v in POST.items()]))
    r, report = Reader(raw), []
    for name, (data, probs, points) in good.items():
        ret, size, nodes = int(r.take("<i4")[0]), int(r.take("<u8")[0]), int(r.take("<u8")[0])
        keys, depth, value = r.leaves()
        search = r.take(np.dtype([("found", "<i4"), ("value", "<u4")]), len(points))
        consts = rc.constants(rc.RayParams(*probs))
        p = lc.parse(data)
        assert ret == 1 and p.status == lc.OK and p.size == p.nodes == size == nodes, (name, ret, p.status, p.size, p.nodes, size, nodes)
        ck, cd = lc.centre_leaves(p)
        assert np.array_equal(ck, keys) and np.array_equal(cd, depth), (name, "begin_leafs")
        want = np.where(lc.leaf_arrays(p)[2] > 0, rc.F(consts[3]), rc.F(consts[2])).astype(np.float32)
        assert np.array_equal(bits(want), bits(value)), (name, "values")
        vk, vv = lc.expand(p, consts[2], consts[3]) if p.voxels <= 1 << 20 else (None, None)
        if len(points):
            voxels = dict(zip(vk.tolist(), vv)) if vk is not None else None
            for i, pt in enumerate(points):
                key = rc.key3([rc.F(c) for c in pt], 1.0 / RESOLUTION) if name != "size1" else None
                if name == "size1":          # one leaf holds the whole key space
                    hit = all(np.isfinite(pt)) and all(-3276.8 <= float(c) < 3276.8 for c in pt)
                    assert bool(search["found"][i]) == hit and (not hit or search["value"][i] == bits(consts[3])), (name, i)
                    continue
                v = voxels.get(rc.pack3(key)) if key is not None else None
                assert bool(search["found"][i]) == (v is not None), (name, "search", i)
                assert v is None or search["value"][i] == bits(v), (name, "search value", i)
            out[f"{name}_search_found"] = search["found"].astype(np.uint8)
            out[f"{name}_search_value"] = search["value"].copy()
        out[f"{name}_ret"], out[f"{name}_size"], out[f"{name}_num_nodes"] = np.uint8(ret), np.uint64(size), np.uint64(nodes)
        out[f"{name}_leaf_key"], out[f"{name}_leaf_depth"], out[f"{name}_leaf_value"] = keys, depth, value
        line = f"{name}: size {size}, {len(keys)} leaves, {p.voxels} voxels, shallowest depth {int(depth.min()) if len(depth) else '-'}"
        if name in POST:
            pk, pd, pv = r.leaves()
            o, mr, pts = scan_of(rays, POST[name])
            t = rc.Tree(rc.RayParams(*probs, max_range=mr), RESOLUTION)
            t.v = dict(zip(vk.tolist(), (rc.F(x) for x in vv)))
            t.insert(pts, o)
            wk, wv = t.leaves()
            gk, gv = lc.expand_centres(pk, pd, pv)
            assert np.array_equal(gk, wk) and np.array_equal(bits(gv), bits(wv)), (name, "post scan")
            out[f"{name}_post_key"], out[f"{name}_post_depth"], out[f"{name}_post_value"] = pk, pd, pv
            line += f"; after scan {POST[name]}: {len(pk)} leaves, {len(gk)} voxels"
        report.append(line)
    ms = float(r.take("<f8")[0])
    nodes, voxels, nbytes = (int(v) for v in r.take("<u8", 3))
    assert r.off == len(raw)
    for name, (data, code) in bad.items():
        assert lc.parse(data).status == code, (name, lc.parse(data).status, code)
        out[f"bad_{name}"] = np.frombuffer(data, np.uint8)
        out[f"bad_{name}_code"] = np.int32(code)
        out[f"bad_{name}_octomap"] = np.int32(verdicts[name])
        report.append(f"bad {name}: {len(data)} bytes, status {code}, octomap's verdict {verdicts[name]}")
    out["bad_no_file_octomap"] = np.int32(verdicts["no_file"])
    assert verdicts["no_file"] == 0
    write_npz(OUT, out)
    OUT.with_suffix(".sha256").write_text(hashlib.sha256(OUT.read_bytes()).hexdigest() + "  " + OUT.name + "\n")
    cpu = dict(scene="tools/bench_occupancy_rays.py synth_planes", planes=tree_tool.BENCH_PLANES, insert_max_range=tree_tool.BENCH_RANGE,
               voxels=voxels, nodes=nodes, bt_bytes=nbytes, octomap_read_binary_ms=ms,
               note="octomap's readBinary from memory of the stream it wrote for the scene (best of 5; the tree stays pruned, as octomap "
                    "keeps it); one thread, -O1, on the CPU of the machine that made the fixture")
    CPU.write_text(json.dumps(cpu, indent=1) + "\n")
    print(f"{OUT}: {OUT.stat().st_size} bytes\n  " + "\n  ".join(report) + f"\n  bench: readBinary {ms:.2f} ms for {voxels} voxels")


if __name__ == "__main__":
    main()
