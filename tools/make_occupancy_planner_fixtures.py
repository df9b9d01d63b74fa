#!/usr/bin/env python3
"""Writes tests/golden/occupancy_planner.npz (+ .sha256) and tests/golden/occupancy_planner_cpu.json: what the reference's OWN
octomap answers on its read side for planners -- begin_leafs_bbx(min, max, maxDepth) by keys and by points,
getUnknownLeafCenters(centres, pmin, pmax, depth), getMetricMin / getMetricMax (the const forms and calcMinMax) with volume(), and
getRayIntersection(origin, direction, centre, intersection, delta) -- and octomap's CPU time for the calls
tools/bench_occupancy_planner.py times.

Run by hand, never by a test:

    python tools/make_occupancy_planner_fixtures.py --reference /path/to/U96-SLAM [--out DIR]

It compiles its driver, tools/octomap_drivers/planner.cpp (this project's text; it calls octomap's API only), against the octomap
sources vendored in the reference tree (tools/octomap_kit.py builds them once, outside the history), and keeps only inputs and
recorded outputs. The trees are those of tests/golden/occupancy_tree.npz (its own key lists, the cube and the three 40 x 30 planes
of the query fixture, log-odds and hit mode) and the empty tree; every one has its metric bounds recorded expanded and pruned.
Through the restatement tests/occupancy_planner_cases.py the generator asserts equality with octomap everywhere, and the coverage
the cases claim:

    box iterator   a box of one voxel; a box equal to a collapsed cube; one that cuts it; one whose minimum is the cube's
                   one-past-end key (the loose upper side visits it: the exact-overlap answer differs); min > max (nothing at
                   depth 16; a collapsed node whose loose interval holds both is still visited, as octomap does); a box over
                   everything (equals leaves(max_depth)) at max_depth 1, 8, 15 and 0; the point form with a corner outside the key
                   space and a NaN corner; the empty tree. Every case equals the per-node decision (a node's own test implies its
                   ancestors').
    unknown cells  depth 16 and depth 14; pmin == pmax; zero steps on one axis; a box fully known, one fully unknown, one that
                   straddles; grids of 1 x 1 x 1, 1 x 1 x 65 and 5 x 4 x 3 cells and one of 12 x 12 x 12 away from zero; some
                   reported float differs in bits from its cell's keyToCoord centre; the cell at pmin is absent although unknown.
    ray entry      the six axis rays; parallel to two axes; grazing within and beyond 1e-6 of an edge; a miss; an origin inside
                   (a negative d wins); zero, NaN and infinite directions; delta 0 and +-1e-3; un-normalised directions; castRay's
                   recorded end points of the query fixture as centres.
"""
import struct

import numpy as np

import octomap_kit as kit
from octomap_kit import PROBS, RESOLUTION, centres, rc
import occupancy_planner_cases as pc
import occupancy_tree_cases as tc

FAR = np.float32([1e6, 1e6, 1e6])
ALL = ((0, 0, 0), (65535, 65535, 65535))
BBX_TREES = ("one", "sib8", "sib8_mixed", "cube64", "cube63", "straddle", "corners", "shift_3", "box", "scene", "scene_hits", "empty")
BENCH_BOX, BENCH_UNKNOWN, BENCH_RAYS = 64, 128, 1 << 20
NAN, INF = float("nan"), float("inf")


def unpack(keys):
    return kit.occ.unpack(np.asarray(keys, np.uint64)).astype(np.int64)


def tree_inputs(T, q):
    """name -> dict(params, hits, scans | hit_keys + hit_counts, keys (n, 3))"""
    out = {}
    for name in [str(t) for t in T["trees"]]:
        hits = bool(int(T[f"{name}_hits"]))
        params = rc.RayParams(*[float(v) for v in T[f"{name}_params"]])
        if hits:
            out[name] = dict(params=params, hits=True, hit_keys=q["scene_hits_keys"], hit_counts=q["scene_hits_counts"], keys=unpack(q["scene_hits_keys"]))
            continue
        keys = T[f"{name}_keys"] if f"{name}_keys" in T else q[f"{name}_keys"]
        if f"{name}_npoints" in q:
            scans = kit.scans_of(q, name)
        elif f"{name}_scan_keys" in T:
            ends = np.cumsum(T[f"{name}_scan_n"])
            scans = [(FAR, -1.0, centres(T[f"{name}_scan_keys"][e - n:e])) for n, e in zip(T[f"{name}_scan_n"], ends)]
        else:
            scans = [(FAR, -1.0, centres(unpack(keys)))]
        out[name] = dict(params=params, hits=False, scans=scans, keys=unpack(keys))
    out["empty"] = dict(params=rc.RayParams(), hits=False, scans=[], keys=np.zeros((0, 3), np.int64))
    return out


def grid(end_key, want, depth=16):
    """A depth-16 box that ends at voxel `end_key` and has exactly want[a] steps on axis a: the step count is a floor of a float
    quotient of two rounded centres, so a span of n voxels gives n or n - 1 steps, and the span is chosen by the restatement"""
    lo, hi = [], []
    for a in range(3):
        for end, span in [(end_key[a] + e, want[a] + s) for e in sorted(range(-16, 96), key=abs) for s in (0, 1)]:
            if end - span < 0 or end > 65535:
                continue
            k, top = list(end_key), list(end_key)
            k[a], top[a] = end - span, end
            st, _, _, steps = pc.unknown_plan(RESOLUTION, centres(np.array([k]))[0], centres(np.array([top]))[0], depth)
            if st == 0 and steps[a] == want[a]:
                lo.append(k[a]), hi.append(end)
                break
        else:
            raise AssertionError((end_key, want, a))
    return centres(np.array([lo]))[0], centres(np.array([hi]))[0], depth


def make_cases(name, keys):
    """-> (key boxes [(min, max, depth)], point boxes, unknown boxes)"""
    boxes, pboxes, unknown = [], [], []
    if name not in BBX_TREES:
        return boxes, pboxes, unknown
    big = name == "box"
    if not big:
        boxes += [ALL + (d,) for d in (0, 1, 8, 15)]
    lo, hi = (keys.min(axis=0), keys.max(axis=0)) if len(keys) else (np.array([32768] * 3), np.array([32768] * 3))
    k = tuple(int(v) for v in keys[len(keys) // 2]) if len(keys) else (32768, 32768, 32768)
    boxes += [(k, k, 0), (k, k, 15), (k, k, 3)]                                        # one voxel
    boxes += [((k[0] + 1, k[1], k[2]), k, 0), ((k[0] + 1, k[1], k[2]), k, 15), (k, (k[0], k[1], k[2] - 1), 0)]     # min > max
    mid = tuple(int(v) for v in (lo + hi) // 2)
    boxes += [(tuple(int(v) for v in lo), mid, d) for d in (0, 14)] + [(mid, tuple(int(v) for v in hi), d) for d in (0, 12)]
    boxes += [((0, 0, 0), mid, 0), (mid, (65535, 65535, 65535), 2)]
    cube = {"sib8": ((32770, 32772, 32774), 2), "sib8_mixed": ((32770, 32772, 32774), 2), "cube64": ((33000, 32500, 32900), 4),
            "cube63": ((33000, 32500, 32900), 4)}.get(name)
    if cube:
        c, s = cube
        end = tuple(v + s for v in c)
        boxes += [(c, tuple(v - 1 for v in end), d) for d in (0, 15, 14, 13)]                      # equal to the cube
        boxes += [(tuple(v + 1 for v in c), tuple(v + 1 for v in c), 0), ((c[0] + 1, c[1], c[2]), (c[0] + s - 2 + 1, end[1], end[2]), 0)]   # cuts it
        boxes += [(end, tuple(v + 6 for v in end), d) for d in (0, 15)]                           # the one-past-end key: loose
        boxes += [((end[0], c[1], c[2]), (end[0] + 3, end[1] - 1, end[2] - 1), 0)]
        boxes += [((end[0] + 1, c[1], c[2]), (end[0] + 3, end[1] - 1, end[2] - 1), 0)]            # one further: not visited
        boxes += [((c[0] + s // 2, c[1], c[2]), (c[0] + s // 2 - 1, end[1], end[2]), 0)]          # min > max inside the loose interval
        boxes += [((0, 0, 0), tuple(v - 1 for v in c), 0), ((0, 0, 0), c, 0)]                     # the lower side is exact
    boxes = [(tuple(min(max(int(v), 0), 65535) for v in a), tuple(min(max(int(v), 0), 65535) for v in b), d) for a, b, d in boxes]
    p = lambda key: centres(np.array([key]))[0]                                                   # noqa: E731
    pboxes += [(p(lo), p(hi), 0), (p(lo) - np.float32(0.04), p(mid) + np.float32(0.04), 15), (p(mid), p(hi), 8)]
    pboxes += [(np.float32([3276.85, 0, 0]), p(hi), 0), (p(lo), np.float32([0, -3276.81, 0]), 0), (np.float32([NAN, 0, 0]), p(hi), 0),
               (p(lo), np.float32([0, 0, INF]), 0), (np.float32([-3276.8, -3276.8, -3276.8]), np.float32([3276.75, 3276.75, 3276.75]), 1 if big else 0)]
    # unknown cells
    step = np.float32(RESOLUTION)
    unknown += [(p(k), p(k), 0), (p(k), p(k), 14)]                                                # pmin == pmax
    unknown += [grid(k, (1, 1, 1)), grid(k, (1, 1, 65)), grid(k, (5, 4, 3)), grid(k, (3, 0, 2))]     # the last: zero steps on y
    unknown += [(p(k) + np.float32([40, -35, 20]), p(k) + np.float32([40, -35, 20]) + step * 6, 16)]      # nothing known there
    unknown += [(p(lo) - step * 2, p(lo) + step * 10, 16), (p(lo) - step * 8, p(lo) + step * 16, 14), (p(mid) - step * 9, p(mid) + step * 8, 15)]
    if cube:
        c, s = cube
        unknown += [(p(c), p(tuple(v + s - 1 for v in c)), 16)]                                   # inside the cube: fully known
        unknown += [(p(tuple(v - 1 for v in c)), p(tuple(v + s - 1 for v in c)), 16)]             # the whole cube: fully known
        unknown += [grid(tuple(v + 5 for v in c), (12, 12, 12))]                                  # 12 x 12 x 12, straddles
        unknown += [(p(tuple(v - 8 for v in c)), p(tuple(v + 8 for v in c)), 14), (p(tuple(v - 8 for v in c)), p(tuple(v + 8 for v in c)), 15)]
    return boxes, pboxes, [u for u in unknown if defined(*u)]


def defined(pmin, pmax, depth):
    """octomap's getUnknownLeafCenters is defined for this box: both corners have keys and no step count is negative (its
    cast of a negative count to unsigned is not)"""
    for a in range(3):
        lo, hi = (pc.coord_to_key(np.float32(p[a]), depth or 16, 1.0 / RESOLUTION) for p in (pmin, pmax))
        if lo is None or hi is None or not 0 <= lo <= hi <= 65535:
            return False
    return True


def ray_cases(q):
    """(origin, direction, centre, delta) rows as float64 (n, 10)"""
    c = centres(np.array([[32768 + 12, 32768 - 7, 32768 + 3]]))[0].astype(np.float64)      # a voxel centre away from zero
    h, rows = 0.05, []

    def add(o, d, centre=c, delta=0.0):
        rows.append(list(np.float32(o).astype(np.float64)) + list(np.float32(d).astype(np.float64)) + list(np.float32(centre).astype(np.float64)) + [delta])

    for a in range(3):                                       # the six axis rays, normalised and not
        for s in (1.0, -1.0):
            d = np.zeros(3)
            d[a] = s
            for scale in (1.0, 3.5, 0.01):
                for delta in (0.0, 1e-3, -1e-3):
                    add(c - 2.0 * d + np.array([0.01, -0.02, 0.015]) * (1 - np.abs(d)), d * scale, delta=delta)
    add(c + [-1.0, -1.0, 0.02], [1.0, 1.0, 0.0])             # parallel to one axis; the x and y planes tie
    add(c + [-1.0, 0.01, 0.02], [2.0, 0.0, 0.0])             # parallel to two axes
    for eps in (0.0, 5e-7, 9e-7, 2e-6, 1e-5, -5e-7):         # grazing an edge: within and beyond 1e-6
        add(c + [-1.0, h + eps, 0.0], [1.0, 0.0, 0.0])
        add(c + [0.0, -1.0, -h - eps], [0.0, 1.0, 0.0])
        add(c + [-1.0, h + eps - 0.5, 0.0], [1.0, 0.5, 0.0])
    add(c + [-1.0, 0.3, 0.0], [1.0, 0.0, 0.0])               # misses
    add(c + [-1.0, 0.0, 0.0], [1.0, 1.0, 1.0])
    add(c + [-1.0, 0.0, 0.0], [-1.0, 0.0, 0.0])              # points away: the line still meets the planes, d < 0
    for delta in (0.0, 1e-3, -1e-3):                         # origin inside: the negative d wins
        add(c + [0.01, 0.02, -0.03], [0.3, -0.5, 0.8], delta=delta)
        add(c, [1.0, 0.0, 0.0], delta=delta)
    add(c + [-1.0, 0.0, 0.0], [0.0, 0.0, 0.0])               # zero, NaN and infinite directions
    add(c + [-1.0, 0.0, 0.0], [-0.0, 0.0, 0.0])
    add(c + [-1.0, 0.0, 0.0], [NAN, 0.0, 0.0])
    add(c + [-1.0, 0.0, 0.0], [1.0, NAN, 0.0])
    add(c + [-1.0, 0.0, 0.0], [NAN, NAN, NAN])
    add(c + [-1.0, 0.0, 0.0], [INF, 0.0, 0.0])
    add(c + [-1.0, 0.0, 0.0], [1.0, -INF, 0.0])
    add(c + [-1.0, 0.0, 0.0], [INF, INF, INF])
    add([NAN, 0.0, 0.0], [1.0, 0.0, 0.0])
    add(c + [-1.0, 0.0, 0.0], [1.0, 0.0, 0.0], centre=[INF, 0.0, 0.0])
    add(c + [-1.0, 0.0, 0.0], [1e-30, 0.0, 0.0])             # d overflows float
    add(c + [-1.0, 0.0, 0.0], [1.0, 1e-20, 0.0], delta=1e300)
    for name in ("box_axes", "box_origin", "box_ties", "scene_random"):      # castRay's own end points as centres
        rays, end = q[f"{name}_rays"][:96], q[f"{name}_end"][:96]
        for r, e in zip(rays, end):
            if np.isfinite(e).all():
                add(r[:3], r[3:], centre=e, delta=1e-3 if len(rows) % 3 == 0 else 0.0)
    return np.array(rows, np.float64)


def bench_inputs():
    """The boxes tools/bench_occupancy_planner.py asks: 64^3 keys and 128^3 cells around the last pose of the four key frames"""
    scans = kit.bench_scans()
    key = np.array(rc.key3([np.float32(v) for v in scans[-1][0]], 1.0 / RESOLUTION))
    lo, hi = key - BENCH_BOX // 2, key + BENCH_BOX // 2 - 1
    c = centres(np.array([key]))[0]
    half = np.float32(RESOLUTION * BENCH_UNKNOWN / 2)
    return scans, (lo, hi), (c - half, c + half)


def main():
    args = kit.arguments(__doc__)
    T, q = kit.load("tree", "planner"), kit.load("query", "planner")
    trees = tree_inputs(T, q)
    cases = {name: make_cases(name, t["keys"]) for name, t in trees.items()}
    rays = ray_cases(q)
    scans, bbox, ubox = bench_inputs()

    def write(f):
        f.write(kit.ints(len(trees)))
        for name, t in trees.items():
            f.write(kit.head(t["params"]) + kit.ints(t["hits"], t["hits"]))
            f.write(kit.hits(t["hit_keys"], t["hit_counts"]) if t["hits"] else kit.scans(t["scans"]))
            boxes, pboxes, unknown = cases[name]
            f.write(kit.ints(len(boxes)) + b"".join(np.array(list(lo) + list(hi), np.uint16).tobytes() + kit.ints(d) for lo, hi, d in boxes))
            for group in (pboxes, unknown):
                f.write(kit.ints(len(group)) + b"".join(np.float32(list(lo) + list(hi)).tobytes() + kit.ints(d) for lo, hi, d in group))
        f.write(struct.pack("<d", RESOLUTION) + kit.ints(len(rays)))
        for r in rays:
            f.write(np.float32(r[:9]).tobytes() + struct.pack("<d", r[9]))
        f.write(kit.ints(1) + kit.head(rc.RayParams()) + kit.scans(scans))
        f.write(np.array(list(bbox[0]) + list(bbox[1]), np.uint16).tobytes() + np.float32(list(ubox[0]) + list(ubox[1])).tobytes())
        f.write(kit.ints(max(1, BENCH_RAYS // len(rays))))

    code, raw = kit.run(kit.build(args.reference, "planner"), "planner", write)
    assert code == 0, code
    r = kit.Reader(raw)
    out = dict(resolution=np.float64(RESOLUTION), trees=np.array(list(trees)), far_origin=FAR)
    report, seen = [], dict(loose=0, grids=set(), drift=0, pmin_absent=0, known=0, unknown=0, straddle=0, minmax_visit=0, differ=0, no_key=0)
    same = lambda a, b: np.array_equal(np.asarray(a), np.asarray(b))   # noqa: E731
    for name, t in trees.items():
        m = np.array(r.take("<f8", 25))
        if t["hits"]:
            voxels = tc.max_likelihood({int(k): 0 for k in t["hit_keys"]}, tc.HITS, rc.constants(t["params"]))
        else:
            tree = rc.Tree(t["params"], RESOLUTION)
            for o, mr, p in t["scans"]:
                tree.rp.max_range = mr
                tree.insert(p, o)
            voxels = dict(tree.v)
        mine = tc.Tree(voxels, RESOLUTION)
        want = [pc.metric(mine, False), pc.metric_calc(mine, False), pc.metric(mine, True), pc.metric_calc(mine, True)]
        flat = np.array([v for lo, hi in want for v in lo + hi], np.float64)
        assert same(flat.view(np.uint64), m[:24].view(np.uint64)), (name, "metric")
        assert np.float64(pc.volume(*want[3])).view(np.uint64) == m[24:].view(np.uint64)[0], (name, "volume")
        seen["differ"] += int(not same(m[:6].view(np.uint64), m[12:18].view(np.uint64)))
        out[f"{name}_metric"] = m
        out[f"{name}_hits"] = np.int32(t["hits"])
        boxes, pboxes, unknown = cases[name]
        rec = dict(n=[], key=[], depth=[], value=[])
        for i, (lo, hi, d) in enumerate(boxes + pboxes):
            k, dd, v = r.leaves(np.int32)
            got = pc.leaves_bbx(mine, lo, hi, d) if i < len(boxes) else pc.leaves_bbx_points(mine, lo, hi, d, octomap=True)
            assert same(k, got[0]) and same(dd, got[1]) and same(kit.bits(v), kit.bits(got[2])), (name, "bbx", i)
            if i >= len(boxes) and not pc.corners_have_keys(mine, lo, hi):      # the divergence: octomap's loop visits the root once
                assert len(k) == (1 if len(t["keys"]) else 0) and (dd == 0).all() and len(pc.leaves_bbx_points(mine, lo, hi, d)[0]) == 0
                seen["no_key"] += len(k)
            if i < len(boxes):
                node = pc.leaves_bbx_by_node(mine, lo, hi, d)
                assert same(k, node[0]) and same(dd, node[1]), (name, "a node's own test implies its ancestors'", i)
                exact = [j for j in range(len(k)) if all(lo[a] <= int(x) + (32768 >> int(dd[j])) - (1 if dd[j] < 16 else 0) and
                                                         hi[a] >= int(x) - (32768 >> int(dd[j])) for a, x in enumerate(unpack(k[j:j + 1])[0]))]
                seen["loose"] += int(len(exact) != len(k))
                seen["minmax_visit"] += int(any(lo[a] > hi[a] for a in range(3)) and len(k) > 0)
                if any(lo[a] > hi[a] for a in range(3)):
                    assert (dd < 16).all(), (name, "min > max visits no voxel")
                if (lo, hi) == ALL:
                    full = mine.leaves(d)
                    assert same(k, full[0]) and same(dd, full[1]), (name, "the box over everything")
            for key, val in zip(("n", "key", "depth", "value"), (len(k), k, dd.astype(np.uint8), v)):
                rec[key].append(val)
        out[f"{name}_bbx_boxes"] = np.array([list(lo) + list(hi) + [d] for lo, hi, d in boxes], np.int32).reshape(-1, 7)
        out[f"{name}_bbx_point_boxes"] = np.array([list(lo) + list(hi) for lo, hi, _ in pboxes], np.float32).reshape(-1, 6)
        out[f"{name}_bbx_point_depths"] = np.array([d for _, _, d in pboxes], np.int32)
        out[f"{name}_bbx_n"] = np.array(rec["n"], np.int32)
        out[f"{name}_bbx_key"] = np.concatenate(rec["key"] + [np.zeros(0, np.uint64)]).astype(np.uint64)
        out[f"{name}_bbx_depth"] = np.concatenate(rec["depth"] + [np.zeros(0, np.uint8)]).astype(np.uint8)
        out[f"{name}_bbx_value"] = np.concatenate(rec["value"] + [np.zeros(0, np.float32)]).astype(np.float32)
        un, uxyz, usteps = [], [], []
        for i, (lo, hi, d) in enumerate(unknown):
            n = r.one("<u4")
            xyz = r.take("<f4", 3 * n).reshape(-1, 3).copy()
            st, got, steps = pc.unknown_centers(mine, lo, hi, d)
            assert st == 0 and same(kit.bits(xyz), kit.bits(got)), (name, "unknown", i)
            cells = steps[0] * steps[1] * steps[2]
            seen["grids"].add(tuple(steps))
            seen["known"] += int(cells > 0 and n == 0)
            seen["unknown"] += int(cells > 0 and n == cells)
            seen["straddle"] += int(0 < n < cells)
            if n:
                depth = d or 16
                closed = np.array([[np.float32(pc.key_to_coord(pc.coord_to_key(c, depth, 1.0 / RESOLUTION), depth, RESOLUTION)) for c in p] for p in xyz])
                seen["drift"] += int((kit.bits(closed) != kit.bits(xyz)).any())
            _, plo, _, _ = pc.unknown_plan(RESOLUTION, lo, hi, d)
            if cells and mine.search(plo, d)[0] == tc.CELL_UNKNOWN:
                assert not (kit.bits(xyz) == kit.bits(plo)).all(axis=1).any(), (name, "the cell at pmin is never asked", i)
                seen["pmin_absent"] += 1
            un.append(n), uxyz.append(xyz), usteps.append(steps)
        out[f"{name}_unknown_boxes"] = np.array([list(lo) + list(hi) for lo, hi, _ in unknown], np.float32).reshape(-1, 6)
        out[f"{name}_unknown_depths"] = np.array([d for _, _, d in unknown], np.int32)
        out[f"{name}_unknown_steps"] = np.array(usteps, np.int32).reshape(-1, 3)
        out[f"{name}_unknown_n"] = np.array(un, np.int32)
        out[f"{name}_unknown_xyz"] = np.concatenate(uxyz + [np.zeros((0, 3), np.float32)]).astype(np.float32)
        report.append(f"{name}: {len(boxes)} + {len(pboxes)} boxes -> {sum(rec['n'])} entries, {len(unknown)} unknown-cell boxes -> {sum(un)} centres")
    rec = r.take(np.dtype([("found", "<i4"), ("xyz", "<f4", 3)]), len(rays))
    for i, (row, got) in enumerate(zip(rays, rec)):
        found, xyz = pc.ray_intersection(RESOLUTION, row[:3], row[3:6], row[6:9], row[9])
        assert found == bool(got["found"]) and same(kit.bits(xyz), kit.bits(got["xyz"])), ("ray", i, row, xyz, got)
    out["ray_cases"], out["ray_found"], out["ray_xyz"] = rays, rec["found"].astype(np.uint8), rec["xyz"].copy()
    found = rec["found"].astype(bool)
    assert found.any() and (~found).any() and np.isnan(rec["xyz"][~found]).all()
    names = ("leaves", "leaves_bbx", "unknown_16", "unknown_14", "metric", "ray_intersections")
    cpu = {}
    for key in names:
        count, ms = r.one("<u8"), r.one("<f8")
        cpu[key] = dict(count=int(count), ms=round(ms, 3))
    cpu["ray_intersections"]["found"] = int(r.one("<u8"))
    r.done()
    # the coverage the cases claim
    assert seen["loose"] >= 2, "no recorded box shows the loose upper side"
    assert seen["minmax_visit"] >= 1, "no min > max box visits a collapsed node"
    assert {(1, 1, 1), (1, 1, 65), (5, 4, 3), (12, 12, 12)} <= seen["grids"] and any(0 in g and max(g) > 0 for g in seen["grids"]), seen["grids"]
    assert seen["drift"] and seen["pmin_absent"] and seen["known"] and seen["unknown"] and seen["straddle"], seen
    cpu_note = dict(what="octomap's own begin_leafs / begin_leafs_bbx loops, getUnknownLeafCenters at depth 16 and 14, the const getMetricMin + "
                         "getMetricMax and a getRayIntersection loop on the pruned map of the benchmark's four key frames",
                    build=" ".join(kit.CXX), threads=1, bbx_keys=[int(v) for v in list(bbox[0]) + list(bbox[1])],
                    unknown_box=[float(v) for v in list(ubox[0]) + list(ubox[1])], calls=cpu)
    OUT = kit.save(args.out, "planner", out, cpu=cpu_note)
    print(f"{OUT}: {OUT.stat().st_size} bytes\n  " + "\n  ".join(report) + f"\n  expanded and pruned bounds differ in bits for {seen['differ']} trees"
          f"\n  rays: {len(rays)}, {int(found.sum())} found\n  cpu: {cpu}")
    assert OUT.stat().st_size <= (kit.GOLDEN / "occupancy_ot.npz").stat().st_size, "larger than the largest occupancy fixture"


if __name__ == "__main__":
    main()
