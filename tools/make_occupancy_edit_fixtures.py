#!/usr/bin/env python3
"""Writes tests/golden/occupancy_edit.npz (+ .sha256) and tests/golden/occupancy_edit_cpu.json: what the reference's OWN octomap
answers for updateNode(key | point, float | bool), setNodeValue, deleteNode at any depth and the box-delete loop its users
write -- after every step the depth-16 leaves (key, float log-odds) of the expanded tree, the changed keys with their flags, and
search() of a few probe keys -- and octomap's CPU time for the calls tools/bench_occupancy_edit.py times.

Run by hand, never by a test:

    python tools/make_occupancy_edit_fixtures.py --reference /path/to/U96-SLAM [--out DIR]

It compiles its driver, tools/octomap_drivers/edit.cpp (this project's text; it calls octomap's API only), against the octomap
sources vendored in the reference tree (tools/octomap_kit.py builds them once, outside the history), feeds it the steps and keeps
only inputs and recorded outputs. Through the restatement tests/occupancy_edit_cases.py it asserts what each case claims, and
equality with octomap everywhere but in the two divergences include/sbm.h names, where it asserts the exact difference. The cases:

    clamps            hits up to clamp max and on (the early abort: nothing happens), misses down to clamp min and on, in one call
                      and call by call
    zero_update       u = 0 on an absent voxel (created at 0), on a present one, on voxels at either clamp
    set_beyond        setNodeValue beyond both clamps and inside them
    set_update_order  set then update, and update then set, on one voxel each in ONE call: the two results differ
    delete_then_update   delete then update in one call: created again from 0
    delete_depths     deleteNode at depths 16, 13 and 1
    delete_in_pruned  a voxel inside a pruned block of eight: its seven siblings stay
    delete_absent     deleteNode of keys that are not there, at depths 16 and 12
    delete_last_voxel the DIVERGENCE: octomap keeps a childless root, which search returns for every key
    points            the point forms, with points that have no key
    nan               a NaN update and a NaN set, and what later items make of them
    box_delete        the box loop inside and outside, bounds on voxels that exist, and the empty box
    detect            edits under change detection: created, flipped, flipped back, created-then-flipped stays created
    delete_change_record   the DIVERGENCE: octomap keeps a deleted voxel's key in changed_keys, and does not overwrite it when
                      the voxel is created again
    bool              updateNode(key, bool): equals updateNode(key, float) with the formed log-odds
    scene_edits       the three 40 x 30 planes of tools/make_occupancy_fixtures.py with edits between the scans, under detection
"""
import struct

import numpy as np

import octomap_kit as kit
from octomap_kit import PROBS, RESOLUTION, rc

import bench_occupancy_edit as be
import occupancy_edit_cases as ec
from occupancy_edit_cases import DELETE, DELETE_BOX, DELETE_KEYS, EDIT, HIT, MISS, SCAN, SET, UPDATE

NAN = float("nan")
BOX_LO, BOX_HI = (32768 + 105, 32768 + 100, 32768 + 110), (32768 + 125, 32768 + 130, 32768 + 139)     # of box_delete


def K(i, j, k):
    return rc.pack3((32768 + i, 32768 + j, 32768 + k))


def edit(items, detect=False, reset_changes=False):
    """items: (key, op, value)"""
    return dict(kind=EDIT, form=0, keys=np.array([i[0] for i in items], np.uint64), ops=np.array([i[1] for i in items], np.uint8),
                values=np.array([i[2] for i in items], np.float32), detect=detect, reset_changes=reset_changes)


def edit_points(items, detect=False):
    """items: (point, op, value)"""
    return dict(kind=EDIT, form=1, points=np.array([i[0] for i in items], np.float32).reshape(-1, 3),
                ops=np.array([i[1] for i in items], np.uint8), values=np.array([i[2] for i in items], np.float32), detect=detect,
                reset_changes=False)


def delete(keys, depth=0, detect=False):
    return dict(kind=DELETE_KEYS, keys=np.array(keys, np.uint64), depth=depth, detect=detect, reset_changes=False)


def box(kmin, kmax, outside=False, detect=False):
    return dict(kind=DELETE_BOX, box=np.array(list(kmin) + list(kmax), np.uint16), outside=outside, detect=detect, reset_changes=False)


def scan(origin, points, detect=False):
    return dict(kind=SCAN, origin=np.asarray(origin, np.float32), points=np.asarray(points, np.float32).reshape(-1, 3), detect=detect,
                reset_changes=False)


def case(steps, probes=(), **probs):
    for s in steps:      # every step holds every field, empty where its kind has none
        n = len(s.get("keys", s.get("points", ())))
        s.setdefault("form", 0), s.setdefault("depth", 0), s.setdefault("outside", False)
        s.setdefault("keys", np.zeros(n, np.uint64)), s.setdefault("points", np.zeros((n, 3), np.float32))
        s.setdefault("ops", np.zeros(n, np.uint8)), s.setdefault("values", np.zeros(n, np.float32))
        s.setdefault("origin", np.zeros(3, np.float32)), s.setdefault("box", np.zeros(6, np.uint16))
    return dict(params=rc.RayParams(**probs), steps=steps, probes=np.array(probes, np.uint64))


def seed(*keys, value=1.0):
    """far-apart voxels that keep the tree from ever being a bare root"""
    return [(k, SET, value) for k in keys]


def make_cases():
    cases = {}
    far = [K(900, -700, 300), K(-800, 650, -200)]
    a, b, c, d = K(3, -2, 5), K(-40, 17, 9), K(120, 121, -122), K(7, 7, 7)
    hit, miss = float(rc.logodds(0.7)), float(rc.logodds(0.4))
    cases["clamps"] = case([edit(seed(*far) + [(a, UPDATE, hit)] * 8 + [(b, UPDATE, miss)] * 9), edit([(b, UPDATE, miss)]),
                            edit([(a, UPDATE, hit), (b, UPDATE, miss)] * 2), edit([(a, UPDATE, miss), (b, UPDATE, hit)])])
    cases["zero_update"] = case([edit(seed(*far) + [(a, SET, 9.0), (b, SET, -9.0), (c, SET, 0.5)]),
                                 edit([(a, UPDATE, 0.0), (b, UPDATE, 0.0), (c, UPDATE, 0.0), (d, UPDATE, 0.0), (a, UPDATE, -0.0)])])
    cases["set_beyond"] = case([edit(seed(*far) + [(a, SET, 100.0), (b, SET, -100.0), (c, SET, 1.25), (d, SET, -1.5)]),
                                edit([(a, SET, -0.25), (d, SET, 3.5)])])
    cases["set_update_order"] = case([edit(seed(*far) + [(a, SET, 3.0), (a, UPDATE, hit), (b, UPDATE, hit), (b, SET, 3.0)])])
    cases["delete_then_update"] = case([edit(seed(*far) + [(a, SET, 2.0), (b, SET, 2.0)]),
                                        edit([(a, DELETE, 0), (a, UPDATE, hit), (b, UPDATE, hit), (c, UPDATE, hit), (c, DELETE, 0),
                                              (d, DELETE, 0), (d, SET, -1.0), (d, DELETE, 0), (d, UPDATE, miss)])])
    rng = np.random.default_rng(27)
    # distinct voxels whose key components all have the top bit set, three of them in one 8 x 8 x 8 block, and forty in the other
    # half of x, which a depth of 1 tells apart
    cloud = [K(104, 104, 104), K(111, 111, 111), K(105, 110, 107)]
    cloud += [K(int(i), int(j), int(k)) for i, j, k in rng.integers(100, 140, (300, 3))]
    cloud += [K(int(i) - 9000, int(j), int(k)) for i, j, k in rng.integers(100, 140, (40, 3))]
    cloud = list(dict.fromkeys(cloud))
    values = rng.uniform(-2.5, 4.0, len(cloud))
    base = edit([(k, SET, float(v)) for k, v in zip(cloud, values)])
    cases["delete_depths"] = case([base, delete([cloud[5], cloud[6], cloud[5]], 16), delete([K(106, 106, 106), cloud[7]], 13),
                                   delete([cloud[8]], 1)])
    block = [K(64 + i, -32 + j, 16 + k) for i in (0, 1) for j in (0, 1) for k in (0, 1)]
    cases["delete_in_pruned"] = case([edit(seed(*far) + [(k, SET, 0.75) for k in block]), delete([block[5]]),
                                      edit([(block[2], DELETE, 0)])])
    cases["delete_absent"] = case([base, delete([K(500, 500, 500), K(-3000, 2, 2)], 16), delete([K(500, 500, 500), K(-3000, 2, 2)], 12),
                                   edit([(K(501, 500, 500), DELETE, 0)])])
    cases["delete_last_voxel"] = case([edit([(a, UPDATE, hit)]), delete([a])], probes=[a, b])
    ok = np.float32([0.31, -0.22, 0.57])
    cases["points"] = case([edit_points([(ok, UPDATE, hit), ((4000.0, 0, 0), UPDATE, hit), ((0.1, NAN, 0.2), SET, 1.0), (ok + 0.01, UPDATE, hit),
                                         ((0.5, 0.5, float("inf")), UPDATE, hit), ((-3276.75, 3276.75, 0.05), SET, -1.0), ((1.0, 1.0, 3276.8), SET, 1.0),
                                         ((-1.25, 2.5, 0.35), SET, 2.0)]),
                            edit_points([((-1.21, 2.55, 0.31), DELETE, 0), ((9000.0, 0, 0), DELETE, 0), (ok, UPDATE, miss)])])
    cases["nan"] = case([edit(seed(*far) + [(a, SET, 1.0), (a, UPDATE, NAN), (b, SET, NAN), (c, UPDATE, NAN), (d, SET, 1.0)]),
                         edit([(a, UPDATE, hit), (b, UPDATE, hit), (c, SET, 0.5), (d, UPDATE, NAN), (d, SET, 2.0)])])
    lo, hi = BOX_LO, BOX_HI
    on_bounds = [rc.pack3(lo), rc.pack3(hi), rc.pack3((lo[0], hi[1], 32768)), rc.pack3((lo[0] - 1, hi[1], 32768)),
                 rc.pack3((hi[0], hi[1] + 1, 32768))]
    grid = edit([(k, SET, float(v)) for k, v in zip(cloud, values)] + [(k, SET, 0.5) for k in on_bounds])
    cases["box_delete"] = case([grid, box(lo, hi), grid, box(lo, hi, outside=True), box((32768, 32768, 32768), (32767, 40000, 40000)),   # min > max on x: the empty box
                                box((0, 0, 0), (65535, 65535, 65535), outside=True)])
    # default probabilities: thres 0; x goes 0.85 (created), then three misses flip it at the third, a hit flips it back
    cases["detect"] = case([edit(seed(*far)), edit([(a, UPDATE, hit), (b, UPDATE, miss)], detect=True),
                            edit([(a, UPDATE, miss)] * 3 + [(c, SET, 1.0), (c, SET, -1.0)], detect=True),
                            edit([(far[0], SET, -1.0), (far[1], UPDATE, miss), (far[1], UPDATE, miss), (far[1], UPDATE, miss)], detect=True,
                                 reset_changes=True),
                            edit([(far[0], UPDATE, hit), (far[0], UPDATE, hit), (far[1], UPDATE, miss)], detect=True),
                            edit([(d, UPDATE, hit)], detect=False), edit([(d, SET, -1.0)], detect=True)])
    cases["delete_change_record"] = case([edit(seed(*far) + [(a, SET, 1.0)]), edit([(a, SET, -1.0), (b, SET, 1.0)], detect=True),
                                          delete([a, b], detect=True), edit([(a, SET, 1.0), (b, SET, 1.0)], detect=True)])
    cases["bool"] = case([edit(seed(*far) + [(a, HIT, 0), (a, HIT, 0), (b, MISS, 0), (a, MISS, 0), (b, HIT, 0)] + [(c, HIT, 0)] * 7 +
                               [(d, MISS, 0)] * 7)], prob_hit=0.8, prob_miss=0.3)
    disp, poses, m = kit.scene("edit")
    pts = [rc.plane_points(dd, 4, m, pose) for dd, pose in zip(disp, poses)]
    mid = [rc.pack3(rc.key3(p, 10.0)) for p in pts[0][::37][:12]]
    cases["scene_edits"] = case([scan(poses[0][[3, 7, 11]], pts[0]),
                                 edit([(k, SET, -2.0) for k in mid[:6]] + [(k, DELETE, 0) for k in mid[6:]] + [(mid[0], UPDATE, hit)], detect=True),
                                 scan(poses[1][[3, 7, 11]], pts[1], detect=True),
                                 # the records are reset before the deletes: a deleted voxel that held one is the divergence
                                 dict(delete(mid[:3], 14, detect=True), reset_changes=True),
                                 box((32768 - 10, 32768 - 10, 32768 - 2), (32768 + 10, 32768 + 10, 32768 + 6), detect=True),
                                 scan(poses[2][[3, 7, 11]], pts[2], detect=True)], max_range=6.0)
    return cases


def check_cases(cases):
    """What the cases claim about themselves, by the restatement."""
    run = {name: ec.run_case(c, RESOLUTION) for name, c in cases.items()}
    a, b, c, d = K(3, -2, 5), K(-40, 17, 9), K(120, 121, -122), K(7, 7, 7)
    cmin, cmax = rc.logodds(0.1192), rc.logodds(0.971)

    def value(r, key):
        keys, lo = r[0], r[1]
        i = list(map(int, keys)).index(key)
        return lo[i]

    def state(r, key):
        return dict(zip(map(int, r[2]), r[3])).get(key)

    r = run["clamps"]
    assert kit.bits(value(r[0], a)) == kit.bits(cmax) and kit.bits(value(r[0], b)) == kit.bits(cmin)
    t = ec.Tree()
    for _ in range(4):
        t.update_node(a, t.hit)
    assert t.v[a] < cmax, "clamps: the clamp is reached by the fifth hit, the others are early aborts"
    assert kit.bits(value(r[2], a)) == kit.bits(cmax) and value(r[3], a) < cmax and value(r[3], b) > cmin
    r = run["zero_update"][1]
    assert kit.bits(value(r, d)) == kit.bits(np.float32(0)) and kit.bits(value(r, a)) == kit.bits(cmax) and kit.bits(value(r, b)) == kit.bits(cmin)
    r = run["set_beyond"]
    assert kit.bits(value(r[0], a)) == kit.bits(cmax) and kit.bits(value(r[0], b)) == kit.bits(cmin) and value(r[1], d) == np.float32(3.5)
    r = run["set_update_order"][0]
    assert kit.bits(value(r, a)) == kit.bits(cmax) and value(r, b) == np.float32(3.0), "set_update_order: the order does not show"
    r = run["delete_then_update"][1]
    assert kit.bits(value(r, a)) == kit.bits(rc.logodds(0.7)) and value(r, b) > 2.5 and c not in map(int, r[0])
    assert kit.bits(value(r, d)) == kit.bits(rc.logodds(0.4))
    r = run["delete_depths"]
    n = [len(x[0]) for x in r]
    far_half = sum(1 for k in map(int, r[0][0]) if k >> 47 == 0)
    assert n[0] - n[1] == 2 and n[1] - n[2] >= 4 and n[3] == far_half and 30 < far_half <= 40 and n[2] > 250, n
    r = run["delete_in_pruned"]
    assert len(r[0][0]) == 10 and len(r[1][0]) == 9 and len(r[2][0]) == 8
    r = run["delete_absent"]
    assert all(np.array_equal(x[0], r[0][0]) for x in r)
    assert len(run["delete_last_voxel"][1][0]) == 0
    r = run["points"]
    assert len(r[0][0]) == 3 and len(r[1][0]) == 2, [len(x[0]) for x in r]
    r = run["nan"]
    assert np.isnan(value(r[0], a)) and np.isnan(value(r[0], b)) and np.isnan(value(r[0], c))
    assert np.isnan(value(r[1], a)) and np.isnan(value(r[1], b)) and value(r[1], c) == 0.5 and value(r[1], d) == 2.0
    r = run["box_delete"]
    assert 0 < len(r[1][0]) < len(r[0][0]) and len(r[1][0]) + len(r[3][0]) == len(r[0][0]) and np.array_equal(r[4][0], r[3][0])
    lo, hi = BOX_LO, BOX_HI
    assert {rc.pack3(lo), rc.pack3(hi)} <= set(map(int, r[3][0])) and rc.pack3((lo[0] - 1, hi[1], 32768)) in map(int, r[1][0])
    assert len(r[5][0]) == len(r[3][0])
    r = run["detect"]
    far = [K(900, -700, 300), K(-800, 650, -200)]
    assert state(r[1], a) == 1 and state(r[1], b) == 1 and state(r[2], a) == 1 and value(r[2], a) < 0, "created-then-flipped stays created"
    assert state(r[2], c) == 1 and state(r[3], far[0]) == 0 and state(r[3], far[1]) == 0 and state(r[3], a) is None
    assert state(r[4], far[0]) is None and state(r[4], far[1]) == 0, "flipped back erases; an update that crosses no threshold keeps"
    assert state(r[5], d) is None and state(r[6], d) == 0
    r = run["delete_change_record"]
    assert state(r[1], a) == 0 and state(r[1], b) == 1 and state(r[2], a) is None and state(r[3], a) == 1 and state(r[3], b) == 1
    r = run["scene_edits"]
    assert len(r[3][0]) < len(r[2][0]) and len(r[4][0]) < len(r[3][0]) and 0 < r[2][3].sum() < len(r[2][3]) and r[5][3].sum() > 0
    return run


def step_bytes(s, max_range):
    sw = kit.ints(s["kind"], int(s["detect"]) | int(s["reset_changes"]) << 1)
    if s["kind"] == SCAN:
        return sw + kit.scan(s["origin"], max_range, s["points"])
    if s["kind"] == EDIT:
        items = s["points"].astype(np.float32).tobytes() if s["form"] else kit.occ.unpack(s["keys"]).tobytes()
        return sw + kit.ints(s["form"], len(s["ops"])) + items + s["ops"].tobytes() + s["values"].astype(np.float32).tobytes()
    if s["kind"] == DELETE_KEYS:
        return sw + kit.ints(s["depth"], len(s["keys"])) + kit.occ.unpack(s["keys"]).tobytes()
    return sw + s["box"].astype(np.uint16).tobytes() + kit.ints(int(s["outside"]))


def case_bytes(c, record=True):
    return (kit.head(c["params"]) + kit.ints(int(record), len(c["probes"])) + kit.occ.unpack(c["probes"]).tobytes() + kit.ints(len(c["steps"])) +
            b"".join(step_bytes(s, c["params"].max_range) for s in c["steps"]))


def timed_cases():
    """The calls of tools/bench_occupancy_edit.py on the map of its four key frames -> {name: case}"""
    scans = [scan(o, p) for o, _, p in kit.bench_scans()]
    out = {}
    for name in be.BATCHES:
        keys, values = be.batch(name)
        out[name] = case(scans + [dict(kind=EDIT, form=0, keys=keys, ops=np.zeros(len(keys), np.uint8), values=values, detect=False,
                                       reset_changes=False)], max_range=kit.BENCH_RANGE)
    lo, hi = be.half_box()
    out["box_delete_half"] = case(scans + [box(lo, hi)], max_range=kit.BENCH_RANGE)
    return out


def main():
    args = kit.arguments(__doc__)
    cases = make_cases()
    run = check_cases(cases)
    timed = timed_cases()

    def write(f):
        f.write(kit.ints(len(cases) + len(timed)))
        for c in cases.values():
            f.write(case_bytes(c))
        for c in timed.values():
            f.write(case_bytes(c, record=False))

    # octomap's deleteNode needs a release build: deleteNodeRecurs deletes a node that lost its last child while the node still
    # holds its (empty) child array, which the node's destructor asserts against (OcTreeDataNode.hxx:69; without the assert the
    # array leaks and the tree is right)
    code, raw = kit.run(kit.build(args.reference, "edit", extra=["-DNDEBUG"]), "edit", write)
    assert code == 0, code
    r = kit.Reader(raw)
    out = dict(resolution=np.float64(RESOLUTION), names=np.array(list(cases)))
    report = []
    for name, c in cases.items():
        out[f"{name}_constants"] = r.take("<f4", 5).copy()
        rec = dict(leaf_keys=[], leaf_values=[], changed_keys=[], changed_created=[], nleaves=[], nchanges=[], root_only=[], root_value=[],
                   probe_found=[], probe_value=[])
        for i, s in enumerate(c["steps"]):
            bare, root = r.one("<u4"), r.one("<f4")
            n = r.one("<u4")
            k, v = r.voxels(n)
            m = r.one("<u4")
            ck, cf = kit.occ.pack(r.take("<u2", 3 * m)), r.take("u1", m)
            order = np.argsort(ck)
            ck, cf = ck[order].astype(np.uint64), cf[order].astype(np.uint8)
            probe = r.take(kit.FOUND_VALUE, len(c["probes"]))
            for key, val in zip(rec, (k, v, ck, cf, n, m, bare, root, probe["found"].copy(), probe["value"].copy())):
                rec[key].append(val)
            mine = run[name][i]
            same = np.array_equal(mine[0], k) and np.array_equal(kit.bits(mine[1]), kit.bits(v))
            same_changes = np.array_equal(mine[2], ck) and np.array_equal(mine[3], cf)
            if name == ec.LAST_VOXEL and i == 1:
                # octomap: a bare root that every search returns; here: an empty map
                assert bare and n == 0 and len(mine[0]) == 0 and probe["found"].all() and (probe["value"] == np.float32(root).view(np.uint32)).all()
            elif name == ec.CHANGE_RECORD and i >= 2:
                # octomap keeps the deleted voxels' keys, and its insert does not overwrite a's `flipped` when a is created again
                assert same and not bare
                a, b = (int(x) for x in c["steps"][2]["keys"])
                theirs, ours = dict(zip(map(int, ck), cf)), dict(zip(map(int, mine[2]), mine[3]))
                assert theirs == {a: 0, b: 1} and ours == ({} if i == 2 else {a: 1, b: 1}), (theirs, ours)
            else:
                assert same and same_changes and not bare, f"{name}: step {i} differs from octomap"
        st = c["steps"]
        rp = c["params"]
        out[f"{name}_params"] = np.array([getattr(rp, k) for k in PROBS] + [rp.max_range], np.float64)
        out[f"{name}_probes"] = c["probes"]
        out[f"{name}_steps"] = np.array([[s["kind"], s["detect"], s["reset_changes"], len(s["ops"]) if s["kind"] != DELETE_KEYS else len(s["keys"]),
                                          s["depth"] if s["kind"] == DELETE_KEYS else int(s["outside"]), s["form"]] for s in st], np.int32)
        out[f"{name}_keys"] = np.concatenate([s["keys"] for s in st]).astype(np.uint64)
        out[f"{name}_points"] = np.concatenate([s["points"] for s in st]).astype(np.float32).reshape(-1, 3)
        out[f"{name}_ops"] = np.concatenate([s["ops"] if s["kind"] != DELETE_KEYS else np.full(len(s["keys"]), DELETE, np.uint8) for s in st])
        out[f"{name}_values"] = np.concatenate([s["values"] if s["kind"] != DELETE_KEYS else np.zeros(len(s["keys"]), np.float32) for s in st])
        out[f"{name}_origins"] = np.stack([s["origin"] for s in st])
        out[f"{name}_boxes"] = np.stack([s["box"] for s in st])
        for key in ("leaf_keys", "leaf_values", "changed_keys", "changed_created"):
            out[f"{name}_{key}"] = np.concatenate(rec[key])
        out[f"{name}_nleaves"], out[f"{name}_nchanges"] = np.array(rec["nleaves"], np.uint32), np.array(rec["nchanges"], np.uint32)
        out[f"{name}_root_only"], out[f"{name}_root_value"] = np.array(rec["root_only"], np.uint8), np.array(rec["root_value"], np.float32)
        out[f"{name}_probe_found"] = np.array(rec["probe_found"], np.int32).reshape(len(st), -1)
        out[f"{name}_probe_value"] = np.array(rec["probe_value"], np.uint32).reshape(len(st), -1)
        report.append(f"{name}: {len(st)} steps, {rec['nleaves'][-1]} leaves, {rec['nchanges'][-1]} changes")
    cpu = {}
    for name in timed:
        r.take("<f4", 5)
        cpu[name] = dict(ms=round(struct.unpack("<d", r.take(np.uint8, 8).tobytes())[0], 3))
    r.done()
    disp, poses, m = kit.scene("edit")
    out["scene_disp"], out["scene_poses"], out["scene_model"], out["scene_scale"] = disp, poses, kit.occ.model_to_array(m), np.int32(4)
    cpu_note = dict(what="octomap's own updateNode(key, float) loop and box-delete loop on the map of the benchmark's four key frames",
                    build=" ".join(kit.CXX), threads=1, calls=cpu)
    OUT = kit.save(args.out, "edit", out, cpu=cpu_note)
    print(f"{OUT}: {OUT.stat().st_size} bytes\n  " + "\n  ".join(report) + f"\n  cpu: {cpu}")


if __name__ == "__main__":
    main()
