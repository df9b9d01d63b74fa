#!/usr/bin/env python3
"""Writes tests/golden/occupancy_ot.npz (+ .sha256): what the reference's OWN octomap writes with AbstractOcTree::write and holds
after AbstractOcTree::read.

  per-scan streams   for every scene of tests/golden/occupancy_rays.npz, after each recorded insertPointCloud scan, the bytes of
                     tree.write(); the driver also writes after updateInnerOccupancy(); prune(); and reports whether the bytes
                     are the same (the generator asserts that they are)
  read-back records  for each of those streams what read() leaves: size(), calcNumNodes(), every leaf of begin_leafs() (centre
                     key, depth, value bits), search(point) on the points beside the scene
  resume records     for three scenes (the one whose values reach the clamps among them) the leaves after read() of the stream
                     written after scan k followed by the remaining scans; the generator asserts that they equal the leaves of
                     the uninterrupted tree
  hand-built / malformed streams of tests/occupancy_ot_cases.py: read-back records of the first, octomap's verdict on the second
                     (each in a process of its own; -1: the run ended without a verdict)

Run by hand, never by a test:

    python tools/make_occupancy_ot_fixtures.py --reference /path/to/U96-SLAM

It compiles the driver below (this project's text; it calls octomap's API only) against the octomap sources vendored in the
reference tree into a temporary directory, and keeps only inputs and recorded outputs. The generator asserts that the transcription
tests/occupancy_ot_cases.py reproduces every recorded value before it writes the file.
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
import occupancy_ot_cases as oc  # noqa: E402
import occupancy_ray_cases as rc  # noqa: E402
from make_occupancy_load_fixtures import Reader, bits, run  # noqa: E402
from make_occupancy_query_fixtures import write_npz  # noqa: E402

GOLDEN = ROOT / "tests" / "golden"
OUT = GOLDEN / "occupancy_ot.npz"
RESOLUTION = 0.1
RESUME = {"scene": 1, "clamp": 7, "ties": 13}      # scene: the scans after which the stream is written and read back
POINTS = np.float32([[0.05, 0.05, 0.05], [0.35, -0.15, 0.25], [1.05, 0.05, 0.05], [-0.45, 0.95, 0.15], [2.0, 2.0, 2.0],
                     [-300.0, 12.0, 7.0], [4000.0, 0.0, 0.0], [np.nan, 0, 0]])

DRIVER = r"""
// Driver of tools/make_occupancy_ot_fixtures.py: AbstractOcTree::write / read of octomap::OcTree.
#include <octomap/octomap.h>
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
static void stream_out(const std::string& s, FILE* out) {
  wr(out, (uint32_t)s.size());
  fwrite(s.data(), 1, s.size(), out);
}
static void set_params(octomap::OcTree& tree, const double* prob) {
  tree.setProbHit(prob[0]);
  tree.setProbMiss(prob[1]);
  tree.setClampingThresMin(prob[2]);
  tree.setClampingThresMax(prob[3]);
  tree.setOccupancyThres(prob[4]);
}
static bool scan_in(FILE* in, octomap::OcTree& tree) {
  float o[3];
  double max_range;
  int32_t n;
  if (!rd(in, o, 3) || !rd(in, &max_range, 1) || !rd(in, &n, 1)) return false;
  std::vector<float> pts(3 * (size_t)n);
  if (n && !rd(in, pts.data(), pts.size())) return false;
  octomap::Pointcloud scan;
  for (int i = 0; i < n; i++) scan.push_back(pts[3 * i], pts[3 * i + 1], pts[3 * i + 2]);
  tree.insertPointCloud(scan, octomap::point3d(o[0], o[1], o[2]), max_range);
  return true;
}
// read() of a stream -> ok, size, calcNumNodes, leaves, search(points)
static octomap::OcTree* read_back(const std::string& s, const double* prob, const std::vector<float>& pts, FILE* out) {
  std::istringstream is(s);
  octomap::AbstractOcTree* any = octomap::AbstractOcTree::read(is);
  octomap::OcTree* tree = dynamic_cast<octomap::OcTree*>(any);
  wr(out, (int32_t)(tree ? 1 : any ? 2 : 0));
  if (!tree) return 0;
  set_params(*tree, prob);
  wr(out, (uint64_t)tree->size());
  wr(out, (uint64_t)tree->calcNumNodes());
  leaves_out(*tree, out);
  for (size_t i = 0; i < pts.size() / 3; i++) {
    octomap::OcTreeNode* node = tree->search(octomap::point3d(pts[3 * i], pts[3 * i + 1], pts[3 * i + 2]));
    wr(out, (int32_t)(node ? 1 : 0));
    wr(out, (float)(node ? node->getLogOdds() : 0.f));
  }
  return tree;
}

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* in = fopen(argv[1], "rb");
  FILE* out = fopen(argv[2], "wb");
  if (!in || !out) return 2;
  int32_t njobs;
  if (!rd(in, &njobs, 1)) return 3;
  for (int t = 0; t < njobs; t++) {
    double prob[5], resolution;
    int32_t kind, npoints;
    if (!rd(in, prob, 5) || !rd(in, &resolution, 1) || !rd(in, &kind, 1) || !rd(in, &npoints, 1)) return 3;
    std::vector<float> pts(3 * (size_t)npoints);
    if (npoints && !rd(in, pts.data(), pts.size())) return 3;
    if (kind == 0) {          // a scene: scans, a stream after each, its read-back; `resume` >= 0: read that stream and go on
      int32_t nscans, resume;
      if (!rd(in, &nscans, 1) || !rd(in, &resume, 1)) return 3;
      octomap::OcTree tree(resolution);
      set_params(tree, prob);
      octomap::OcTree* resumed = 0;
      for (int s = 0; s < nscans; s++) {
        const long at = ftell(in);
        if (!scan_in(in, tree)) return 3;
        if (resumed) {
          fseek(in, at, SEEK_SET);
          if (!scan_in(in, *resumed)) return 3;
        }
        std::ostringstream a, b;
        tree.write(a);
        octomap::OcTree copy(tree);
        copy.updateInnerOccupancy();
        copy.prune();
        copy.write(b);
        stream_out(a.str(), out);
        wr(out, (int32_t)(a.str() == b.str() ? 1 : 0));
        if (a.str() != b.str()) stream_out(b.str(), out);
        octomap::OcTree* back = read_back(a.str(), prob, pts, out);
        if (s == resume) resumed = back;
        else delete back;
      }
      if (resume >= 0) {
        if (!resumed) return 5;
        leaves_out(*resumed, out);
        tree.expand();
        resumed->expand();
        leaves_out(tree, out);
        leaves_out(*resumed, out);
        delete resumed;
      }
    } else {                  // a stream given: its read-back
      uint32_t nbytes;
      if (!rd(in, &nbytes, 1)) return 3;
      std::string s(nbytes, '\0');
      if (nbytes && !rd(in, &s[0], nbytes)) return 3;
      delete read_back(s, prob, pts, out);
      fflush(out);
    }
  }
  fclose(out);
  return 0;
}
"""


def job_head(f, probs, kind, points):
    f.write(struct.pack("<6dii", *probs, RESOLUTION, kind, len(points)) + np.asarray(points, np.float32).tobytes())


def scans_of(rays, name):
    n = rays[f"{name}_npoints"]
    ends = np.cumsum(n)
    mr = float(rays[f"{name}_params"][5])
    return [(rays[f"{name}_origins"][i], mr, rays[f"{name}_points"][ends[i] - n[i]:ends[i]]) for i in range(len(n))]


def take_readback(r, npoints):
    ret = int(r.take("<i4")[0])
    if ret != 1:
        return ret, None
    size, nodes = int(r.take("<u8")[0]), int(r.take("<u8")[0])
    keys, depth, value = r.leaves()
    search = r.take(np.dtype([("found", "<i4"), ("value", "<u4")]), npoints)
    return ret, (size, nodes, keys, depth, value, search)


def check_readback(tag, data, rec, points):
    """the transcription's parse of `data` against what octomap's read() left"""
    size, nodes, keys, depth, value, search = rec
    p = oc.parse(data)
    assert p.status == oc.OK and p.size == p.nodes == nodes, (tag, p.status, p.size, p.nodes, size, nodes)
    ck, cd = oc.centre_leaves(p)
    assert np.array_equal(ck, keys) and np.array_equal(cd, depth), (tag, "begin_leafs")
    assert np.array_equal(oc.leaf_arrays(p)[2], bits(value)), (tag, "values")
    from occupancy_tree_cases import unmorton
    for i, pt in enumerate(points):
        key = rc.key3([rc.F(c) for c in pt], 1.0 / RESOLUTION)
        hit = None
        if key is not None:
            for code, d, v in p.leaves:
                lo = unmorton(code)
                if all(lo[a] <= key[a] < lo[a] + (1 << (16 - d)) for a in range(3)):
                    hit = v
        assert bool(search["found"][i]) == (hit is not None), (tag, "search", i)
        assert hit is None or search["value"][i] == hit, (tag, "search value", i)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reference", required=True, help="checkout of the reference project (read only)")
    args = ap.parse_args()
    ref = pathlib.Path(args.reference) / "src" / "slam"
    rays = dict(np.load(GOLDEN / "occupancy_rays.npz"))
    names = [str(n) for n in rays["names"]]
    default = [getattr(rc.RayParams(), k) for k in ("prob_hit", "prob_miss", "clamp_min", "clamp_max", "occupancy_thres")]
    hand = oc.hand_built()
    with tempfile.TemporaryDirectory() as tmp:
        tmp = pathlib.Path(tmp)
        (tmp / "driver.cpp").write_text(DRIVER)
        srcs = sorted(str(p) for p in (ref / "src" / "octomap").glob("*.cpp"))
        subprocess.run(["g++", "-O1", "-std=c++11", "-I", str(ref / "include"), "-I", str(ref / "include" / "octomap"), "-o",
                        str(tmp / "driver"), str(tmp / "driver.cpp")] + srcs, check=True)

        def write_good(f):
            f.write(struct.pack("<i", len(names) + len(hand)))
            for name in names:
                scans = scans_of(rays, name)
                job_head(f, [float(v) for v in rays[f"{name}_params"][:5]], 0, POINTS)
                f.write(struct.pack("<ii", len(scans), RESUME.get(name, -1)))
                for o, mr, p in scans:
                    f.write(np.asarray(o, np.float32).tobytes() + struct.pack("<di", mr, len(p)) + np.asarray(p, np.float32).tobytes())
            for data in hand.values():
                job_head(f, default, 1, POINTS)
                f.write(struct.pack("<I", len(data)) + data)

        code, raw = run(tmp / "driver", tmp, "good", write_good)
        assert code == 0, code
        r, report = Reader(raw), []
        out = dict(resolution=np.float64(RESOLUTION), names=np.array(names), points=POINTS, hand_built=np.array(list(hand)),
                   resume=np.array([f"{k}:{v}" for k, v in RESUME.items()]))
        good = None
        for name in names:
            probs = [float(v) for v in rays[f"{name}_params"][:5]]
            mr = float(rays[f"{name}_params"][5])
            scans = scans_of(rays, name)
            tree = rc.Tree(rc.RayParams(*probs, max_range=mr), RESOLUTION)
            found, value = [], []
            for s, (o, _, pts) in enumerate(scans):
                data = r.take(np.uint8, int(r.take("<u4")[0])).tobytes()
                same = int(r.take("<i4")[0])
                assert same == 1, (name, s, "write() differs after updateInnerOccupancy(); prune()")
                ret, rec = take_readback(r, len(POINTS))
                assert ret == 1, (name, s, ret)
                check_readback((name, s), data, rec, POINTS)
                tree.insert(pts, o)
                k, v = tree.leaves()
                assert oc.write(dict(zip(k.tolist(), v)), RESOLUTION) == data, (name, s, "the transcription's write")
                out[f"{name}_ot_{s}"] = np.frombuffer(data, np.uint8)
                out[f"{name}_size_{s}"], out[f"{name}_num_nodes_{s}"] = np.uint64(rec[0]), np.uint64(rec[1])
                out[f"{name}_leaf_key_{s}"], out[f"{name}_leaf_depth_{s}"], out[f"{name}_leaf_value_{s}"] = rec[2], rec[3], rec[4]
                found.append(rec[5]["found"].astype(np.uint8))
                value.append(rec[5]["value"].copy())
                if name == "scene" and s == 0:
                    good = data
            out[f"{name}_search_found"], out[f"{name}_search_value"] = np.stack(found), np.stack(value)
            line = f"{name}: {len(scans)} scans, last stream {len(data)} bytes, size {rec[0]}"
            if name in RESUME:
                rk, rd_, rv = r.leaves()
                uk, ud, uv = r.leaves()          # expanded: the uninterrupted tree, then the resumed one
                ek, ed, ev = r.leaves()
                assert np.array_equal(uk, ek) and np.array_equal(ud, ed) and np.array_equal(bits(uv), bits(ev)), (name, "resume")
                k, v = tree.leaves()
                gk, gv = oc.expand_leaves(*_codes(ek, ed), ev)
                assert np.array_equal(gk, k) and np.array_equal(bits(gv), bits(v)), (name, "resume against the transcription")
                out[f"{name}_resume_key"], out[f"{name}_resume_depth"], out[f"{name}_resume_value"] = rk, rd_, rv
                line += f"; resumed after scan {RESUME[name]}: {len(rk)} leaves, {len(ek)} voxels, equal to the uninterrupted tree"
            report.append(line)
        for name, data in hand.items():
            ret, rec = take_readback(r, len(POINTS))
            assert ret == 1, (name, ret)
            check_readback(name, data, rec, POINTS)
            out[f"hand_{name}"] = np.frombuffer(data, np.uint8)
            out[f"hand_{name}_size"], out[f"hand_{name}_num_nodes"] = np.uint64(rec[0]), np.uint64(rec[1])
            out[f"hand_{name}_leaf_key"], out[f"hand_{name}_leaf_depth"], out[f"hand_{name}_leaf_value"] = rec[2], rec[3], rec[4]
            out[f"hand_{name}_search_found"], out[f"hand_{name}_search_value"] = rec[5]["found"].astype(np.uint8), rec[5]["value"].copy()
            report.append(f"hand {name}: {len(data)} bytes, size() {rec[0]}, calcNumNodes {rec[1]}, {len(rec[2])} leaves")
        assert r.off == len(raw)
        bad = oc.malformed(good)
        out["malformed"] = np.array(list(bad))
        for name, (data, code) in bad.items():
            rcode, o = run(tmp / "driver", tmp, name, lambda f: (f.write(struct.pack("<i", 1)), job_head(f, default, 1, np.zeros((0, 3))),
                                                                 f.write(struct.pack("<I", len(data)) + data)))
            verdict = int(np.frombuffer(o, "<i4", 1)[0]) if rcode == 0 and len(o) >= 4 else -1
            assert oc.parse(data).status == code, (name, oc.parse(data).status, code)
            out[f"bad_{name}"] = np.frombuffer(data, np.uint8)
            out[f"bad_{name}_code"] = np.int32(code)
            out[f"bad_{name}_octomap"] = np.int32(verdict)
            report.append(f"bad {name}: {len(data)} bytes, status {code}, octomap's verdict {verdict}")
    write_npz(OUT, out)
    OUT.with_suffix(".sha256").write_text(hashlib.sha256(OUT.read_bytes()).hexdigest() + "  " + OUT.name + "\n")
    print(f"{OUT}: {OUT.stat().st_size} bytes\n  " + "\n  ".join(report))


def _codes(keys, depths):
    """centre keys of begin_leafs -> (first Morton codes, depths)"""
    codes = [rc.morton(int(k)) >> (3 * (16 - int(d))) << (3 * (16 - int(d))) for k, d in zip(keys, depths)]
    return codes, depths


if __name__ == "__main__":
    main()
