#!/usr/bin/env python3
"""Writes tests/golden/occupancy_load.npz (+ .sha256): what the reference's OWN octomap holds after readBinary of every .bt stream
the other occupancy fixtures recorded (the 18 of occupancy_tree.npz, the 14 of occupancy_rays.npz, the 3 of
occupancy_octomap.npz), of a size-1 stream, and of the malformed streams of tests/occupancy_load_cases.py -- readBinary's return
value, size() and calcNumNodes(), every leaf of begin_leafs() (centre key, depth, value bits), search(point) for the points
recorded beside a tree, and for three trees the leaves again after one more insertPointCloud scan on the loaded tree. Beside it,
tests/golden/occupancy_load_cpu.json holds octomap's milliseconds for readBinary on the scene of tools/bench_occupancy_tree.py
(kept out of the .npz so that the .npz regenerates to the same bytes).

Run by hand, never by a test:

    python tools/make_occupancy_load_fixtures.py --reference /path/to/U96-SLAM [--out DIR]

It compiles its driver, tools/octomap_drivers/load.cpp (this project's text; it calls octomap's API only), against the octomap
sources vendored in the reference tree (tools/octomap_kit.py builds them once, outside the history), and keeps only inputs and
recorded outputs. The input streams themselves are not stored
again: a stream is named by the fixture and member that holds it. The generator asserts that the transcription
tests/occupancy_load_cases.py reproduces every recorded value before it writes the file.

octomap's verdict on a malformed stream is recorded, not required: it reads an OcTree whatever the id says, reads the legacy
header, does not bound the depth, and past the end of a stream reads two bytes it never set. Every malformed stream runs in a
process of its own; -1 stands for a run that ended without a verdict.
"""
import numpy as np

import octomap_kit as kit
from octomap_kit import BENCH_PLANES, BENCH_RANGE, RESOLUTION, bits, rc
import occupancy_load_cases as lc

POST = {"tree_scene": 1, "tree_box": 0, "rays_clamp": 2}     # the scan of occupancy_rays.npz "scene" inserted after the load


def sources():
    """{stream id: (bytes, five probabilities, search points)} of the 35 recorded streams, in a fixed order"""
    tree, rays, octo = (kit.load(n, "load") for n in ("tree", "rays", "octomap"))
    out = {}
    for name in (str(n) for n in tree["trees"]):
        out[f"tree_{name}"] = (tree[f"{name}_bt"].tobytes(), [float(v) for v in tree[f"{name}_params"][:5]], tree[f"{name}_points"])
    for name in (str(n) for n in rays["names"]):
        out[f"rays_{name}"] = (rays[f"{name}_bt"].tobytes(), [float(v) for v in rays[f"{name}_params"][:5]], np.zeros((0, 3), np.float32))
    for name in ("all", "blocks", "empty"):
        out[f"octomap_{name}"] = (octo[f"bt_{name}"].tobytes(), kit.DEFAULT_PROBS, np.zeros((0, 3), np.float32))
    assert len(out) == 35
    return out, rays


def record(probs, data, points, post=None):
    """One stream's record: data None stands for a file that is not there; post: a scan to insert after the load"""
    return (kit.head(probs) + kit.ints(False, data is not None) + (kit.stream(data) if data is not None else b"") + kit.points(points) +
            kit.ints(post is not None) + (kit.scan(*post) if post is not None else b""))


def main():
    args = kit.arguments(__doc__)
    good, rays = sources()
    default = good["octomap_all"][1]
    good["size1"] = (lc.stream(1, bytes((0, 0))), default, np.float32([[0.05, 0.05, 0.05], [-300.0, 12.0, 7.0], [np.nan, 0, 0]]))
    bad = lc.malformed(good["tree_scene"][0])
    scene_scans = kit.scans_of(rays, "scene")
    driver = kit.build(args.reference, "load")

    def write_good(f):
        f.write(kit.ints(len(good) + 1))
        for name, (data, probs, points) in good.items():
            f.write(record(probs, data, points, scene_scans[POST[name]] if name in POST else None))
        f.write(kit.head(default) + kit.ints(True) + kit.scans(kit.bench_scans()))      # timed: build the scene, write it, read it back

    code, raw = kit.run(driver, "good", write_good)
    assert code == 0, code
    verdicts = {}
    for name, (data, _) in list(bad.items()) + [("no_file", (None, lc.UNSUPPORTED))]:
        code, out = kit.run(driver, name, lambda f: f.write(kit.ints(1) + record(default, data, np.zeros((0, 3)))))
        verdicts[name] = int(np.frombuffer(out, "<i4", 1)[0]) if code == 0 and len(out) >= 4 else -1
    out = dict(resolution=np.float64(RESOLUTION), streams=np.array(list(good)), malformed=np.array(list(bad)),
               post_scan=np.array([f"{k}:{v}" for k, v in POST.items()]))
    r, report = kit.Reader(raw), []
    for name, (data, probs, points) in good.items():
        ret, size, nodes = r.one("<i4"), r.one("<u8"), r.one("<u8")
        keys, depth, value = r.leaves()
        search = r.take(kit.FOUND_VALUE, len(points))
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
            o, mr, pts = scene_scans[POST[name]]
            t = rc.Tree(rc.RayParams(*probs, max_range=mr), RESOLUTION)
            t.v = dict(zip(vk.tolist(), (rc.F(x) for x in vv)))
            t.insert(pts, o)
            wk, wv = t.leaves()
            gk, gv = lc.expand_centres(pk, pd, pv)
            assert np.array_equal(gk, wk) and np.array_equal(bits(gv), bits(wv)), (name, "post scan")
            out[f"{name}_post_key"], out[f"{name}_post_depth"], out[f"{name}_post_value"] = pk, pd, pv
            line += f"; after scan {POST[name]}: {len(pk)} leaves, {len(gk)} voxels"
        report.append(line)
    ms = r.one("<f8")
    nodes, voxels, nbytes = (int(v) for v in r.take("<u8", 3))
    r.done()
    for name, (data, code) in bad.items():
        assert lc.parse(data).status == code, (name, lc.parse(data).status, code)
        out[f"bad_{name}"] = np.frombuffer(data, np.uint8)
        out[f"bad_{name}_code"] = np.int32(code)
        out[f"bad_{name}_octomap"] = np.int32(verdicts[name])
        report.append(f"bad {name}: {len(data)} bytes, status {code}, octomap's verdict {verdicts[name]}")
    out["bad_no_file_octomap"] = np.int32(verdicts["no_file"])
    assert verdicts["no_file"] == 0
    cpu = dict(scene="tools/bench_occupancy_rays.py synth_planes", planes=BENCH_PLANES, insert_max_range=BENCH_RANGE,
               voxels=voxels, nodes=nodes, bt_bytes=nbytes, octomap_read_binary_ms=ms,
               note="octomap's readBinary from memory of the stream it wrote for the scene (best of 5; the tree stays pruned, as octomap "
                    "keeps it); one thread, -O1, on the CPU of the machine that made the fixture")
    OUT = kit.save(args.out, "load", out, cpu=cpu)
    print(f"{OUT}: {OUT.stat().st_size} bytes\n  " + "\n  ".join(report) + f"\n  bench: readBinary {ms:.2f} ms for {voxels} voxels")


if __name__ == "__main__":
    main()
