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

    python tools/make_occupancy_ot_fixtures.py --reference /path/to/U96-SLAM [--out DIR]

It compiles its driver, tools/octomap_drivers/ot.cpp (this project's text; it calls octomap's API only), against the octomap
sources vendored in the reference tree (tools/octomap_kit.py builds them once, outside the history), and keeps only inputs and
recorded outputs. The generator asserts that the transcription
tests/occupancy_ot_cases.py reproduces every recorded value before it writes the file.
"""
import numpy as np

import octomap_kit as kit
from octomap_kit import RESOLUTION, bits, rc
import occupancy_ot_cases as oc

RESUME = {"scene": 1, "clamp": 7, "ties": 13}      # scene: the scans after which the stream is written and read back
POINTS = np.float32([[0.05, 0.05, 0.05], [0.35, -0.15, 0.25], [1.05, 0.05, 0.05], [-0.45, 0.95, 0.15], [2.0, 2.0, 2.0],
                     [-300.0, 12.0, 7.0], [4000.0, 0.0, 0.0], [np.nan, 0, 0]])


def stream_job(probs, points, data):
    """kind 1: a stream given, its read-back"""
    return kit.head(probs) + kit.ints(1) + kit.points(points) + kit.stream(data)


def take_readback(r, npoints):
    ret = r.one("<i4")
    if ret != 1:
        return ret, None
    size, nodes = r.one("<u8"), r.one("<u8")
    keys, depth, value = r.leaves()
    search = r.take(kit.FOUND_VALUE, npoints)
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
    args = kit.arguments(__doc__)
    rays = kit.load("rays", "ot")
    names = [str(n) for n in rays["names"]]
    default = kit.DEFAULT_PROBS
    hand = oc.hand_built()
    driver = kit.build(args.reference, "ot")

    def write_good(f):
        f.write(kit.ints(len(names) + len(hand)))
        for name in names:       # kind 0: a scene's scans
            f.write(kit.head([float(v) for v in rays[f"{name}_params"][:5]]) + kit.ints(0) + kit.points(POINTS) +
                    kit.ints(RESUME.get(name, -1)) + kit.scans(kit.scans_of(rays, name)))
        for data in hand.values():
            f.write(stream_job(default, POINTS, data))

    code, raw = kit.run(driver, "good", write_good)
    assert code == 0, code
    r, report = kit.Reader(raw), []
    out = dict(resolution=np.float64(RESOLUTION), names=np.array(names), points=POINTS, hand_built=np.array(list(hand)),
               resume=np.array([f"{k}:{v}" for k, v in RESUME.items()]))
    good = None
    for name in names:
        probs = [float(v) for v in rays[f"{name}_params"][:5]]
        mr = float(rays[f"{name}_params"][5])
        scans = kit.scans_of(rays, name)
        tree = rc.Tree(rc.RayParams(*probs, max_range=mr), RESOLUTION)
        found, value = [], []
        for s, (o, _, pts) in enumerate(scans):
            data = r.stream().tobytes()
            same = r.one("<i4")
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
    r.done()
    bad = oc.malformed(good)
    out["malformed"] = np.array(list(bad))
    for name, (data, code) in bad.items():
        rcode, o = kit.run(driver, name, lambda f: f.write(kit.ints(1) + stream_job(default, np.zeros((0, 3)), data)))
        verdict = int(np.frombuffer(o, "<i4", 1)[0]) if rcode == 0 and len(o) >= 4 else -1
        assert oc.parse(data).status == code, (name, oc.parse(data).status, code)
        out[f"bad_{name}"] = np.frombuffer(data, np.uint8)
        out[f"bad_{name}_code"] = np.int32(code)
        out[f"bad_{name}_octomap"] = np.int32(verdict)
        report.append(f"bad {name}: {len(data)} bytes, status {code}, octomap's verdict {verdict}")
    OUT = kit.save(args.out, "ot", out)
    print(f"{OUT}: {OUT.stat().st_size} bytes\n  " + "\n  ".join(report))


def _codes(keys, depths):
    """centre keys of begin_leafs -> (first Morton codes, depths)"""
    codes = [rc.morton(int(k)) >> (3 * (16 - int(d))) << (3 * (16 - int(d))) for k, d in zip(keys, depths)]
    return codes, depths


if __name__ == "__main__":
    main()
