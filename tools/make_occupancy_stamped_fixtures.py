#!/usr/bin/env python3
"""Writes tests/golden/occupancy_stamped.npz (+ .sha256) and tests/golden/occupancy_stamped_cpu.json: what the reference's OWN
octomap (OcTreeStamped) answers for the stamps insertPointCloud, updateNode, setNodeValue and deleteNode leave, for
degradeOutdatedNodes, and for forgetting by age as a leaf loop plus deleteNode -- and octomap's CPU time for the calls
tools/bench_occupancy_stamped.py times.

Run by hand, never by a test:

    python tools/make_occupancy_stamped_fixtures.py --reference /path/to/U96-SLAM [--out DIR]

It compiles its driver, tools/octomap_drivers/stamped.cpp (this project's text; it calls octomap's API only), against the octomap
sources vendored in the reference tree (tools/octomap_kit.py builds them once, outside the history), feeds it the steps and keeps
only inputs and recorded outputs. octomap takes its clock from time(NULL); the driver defines time() itself and answers what a
step scripts. octomap is driven with lazy_eval = true inserts and edits, so that it never prunes while it inserts: the divergence
include/sbm.h states. Through the restatement tests/occupancy_stamped_cases.py the generator asserts what each case claims, and
equality with octomap in every recorded integer and float bit. The cases:

    scans            four scans of the 40 x 30 planes of tools/make_occupancy_fixtures.py at clocks 1000..1030 that share cells: a
                     wall saturates at its second hit and keeps that hit's stamp through the third (the early return), free space
                     saturates at clamp min likewise
    scans_discrete, scans_box, scans_detect   the first three scans with discretize, with the bounding box, with change detection
    degrade          the scans, voxels set by value (stamp 0), then degradeOutdatedNodes at several (clock, threshold) pairs: a
                     threshold above every age, threshold 0, a clock BELOW the stamps (the 32-bit wrap makes a huge age), repeated
                     until the voxels fall below the occupancy threshold and stop degrading; then one scan that stamps again
    edits            one batch, run at two clocks: updateNode by bool and by float, zero updates, setNodeValue on a new and on an
                     existing voxel, delete followed by re-create, items of one voxel at its clamp
    blocks           for the tree, values beyond clamp max so that every stored value is clamp max: eight siblings with equal stamps
                     (collapse), the same with one stamp different (no collapse), 64 voxels that collapse two levels, 64 where one
                     group of eight has another stamp, eight with the odd stamp in child 0 and eight with it in child 7; a snapshot
                     in both readings (nodes in pre-order with depth, value and stamp, the root's stamp, the .ot and the .bt bytes),
                     then the odd stamps made equal and a second snapshot
    resume           scans and a block, a snapshot, the stamped .ot written and read back (stamps 0), one more scan, a snapshot
    older            the scans and voxels of stamp 0, then forgetting by age at two thresholds and once with a clock below the
                     stamps; the youngest voxels stay (octomap keeps a root when its last voxel goes, which is not recorded)
"""
import struct

import numpy as np

import octomap_kit as kit
from octomap_kit import PROBS, RESOLUTION, rc

import occupancy_stamped_cases as sc
from occupancy_stamped_cases import DEGRADE, DETECT, DISCRETIZE, EDIT, FORGET, RESUME, SCAN, SNAPSHOT, USE_BOX, ec

PROB = dict(prob_hit=0.9, prob_miss=0.2)       # two hits reach clamp max, two misses clamp min: the third is the early return
RANGE = 3.0


def K(i, j, k):
    return rc.pack3((32768 + i, 32768 + j, 32768 + k))


def _step(kind, clock, n, **kw):
    s = dict(kind=kind, clock=clock, flags=0, thres=0, keys=np.zeros(n, np.uint64), points=np.zeros((n, 3), np.float32),
             values=np.zeros(n, np.float32), ops=np.zeros(n, np.uint8), origin=np.zeros(3, np.float32), box=np.zeros(6, np.float32))
    s.update(kw)
    return s


def scan(clock, origin, points, flags=0, box=None):
    p = np.asarray(points, np.float32).reshape(-1, 3)
    return _step(SCAN, clock, len(p), points=p, origin=np.asarray(origin, np.float32), flags=flags,
                 box=np.zeros(6, np.float32) if box is None else np.asarray(box, np.float32))


def edit(clock, items):
    """items: (key, ec.UPDATE | SET | DELETE | HIT | MISS, value)"""
    return _step(EDIT, clock, len(items), keys=np.array([i[0] for i in items], np.uint64), ops=np.array([i[1] for i in items], np.uint8),
                 values=np.array([i[2] for i in items], np.float32))


def degrade(clock, thres):
    return _step(DEGRADE, clock, 0, thres=thres)


def forget(clock, thres):
    return _step(FORGET, clock, 0, thres=thres)


def snapshot(clock):
    return _step(SNAPSHOT, clock, 0)


def resume(clock):
    return _step(RESUME, clock, 0)


def block(corner, side=2):
    return [K(corner[0] + i, corner[1] + j, corner[2] + k) for k in range(side) for j in range(side) for i in range(side)]


B_EQUAL, B_ODD, B_64, B_64_ODD, B_CHILD0, B_CHILD7 = (64, -32, 16), (-20, 40, 8), (128, 64, 32), (-64, -64, -64), (200, 200, 200), (-200, 100, 50)


def case(steps, **probs):
    return dict(params=rc.RayParams(**dict(PROB, **probs)), steps=steps)


def the_scans(flags=0, box=None, count=4):
    disp, poses, m = kit.scene("stamped")
    pts = [rc.plane_points(dd, 4, m, pose) for dd, pose in zip(disp, poses)]
    o = [pose[[3, 7, 11]] for pose in poses]
    return [scan(1000, o[0], pts[0][::5], flags, box), scan(1010, o[0], pts[0][2::5], flags, box), scan(1020, o[0], pts[0][::4], flags, box),
            scan(1030, o[1], pts[1][::5], flags, box)][:count]


SET_KEYS = [K(400 + i, -300, 20 + i) for i in range(6)]


def batch():
    a, b, c, d, e, f, g, h = [K(10 + i, -20 - i, 5 * i) for i in range(8)]
    return [(a, ec.HIT, 0.0), (a, ec.HIT, 0.0), (a, ec.HIT, 0.0),                       # a: the third hit finds it at clamp max
            (b, ec.MISS, 0.0), (b, ec.UPDATE, 0.0), (b, ec.MISS, 0.0), (b, ec.MISS, 0.0),   # b: a zero update between misses, then clamp min
            (c, ec.SET, 0.5), (d, ec.SET, 100.0), (d, ec.UPDATE, 0.0),                      # c, d: set; d at clamp max, a zero update returns early
            (e, ec.UPDATE, 1.5), (e, ec.DELETE, 0.0), (e, ec.SET, 0.25),                    # e: deleted, created again by a set: stamp 0
            (f, ec.UPDATE, -0.5), (f, ec.DELETE, 0.0), (f, ec.UPDATE, 0.75),                # f: deleted, created again by an update: the clock
            (g, ec.UPDATE, 5.0), (g, ec.UPDATE, 5.0),                                       # g: two items of one voxel at its clamp
            (h, ec.UPDATE, 0.0), (h, ec.DELETE, 0.0)]                                       # h: created by a zero update, ends absent


def make_cases():
    cases = {}
    cases["scans"] = case(the_scans(), max_range=RANGE)
    lo, hi = [-0.5, -1.0, -0.4], [2.5, 1.2, 1.0]
    cases["scans_discrete"] = case(the_scans(DISCRETIZE, count=3), max_range=RANGE)
    cases["scans_box"] = case(the_scans(USE_BOX, lo + hi, count=3), max_range=RANGE)
    cases["scans_detect"] = case(the_scans(DETECT, count=3), max_range=RANGE)
    sets = edit(1035, [(k, ec.SET, 1.0 + 0.5 * i) for i, k in enumerate(SET_KEYS)])
    again = the_scans()[0]
    cases["degrade"] = case(the_scans() + [sets, degrade(1040, 2000), degrade(1040, 15), degrade(1040, 0), degrade(500, 1000), degrade(1041, 0),
                                           degrade(1042, 0), degrade(1043, 0), dict(again, clock=1050), degrade(1050, 0), degrade(1060, 5)], max_range=RANGE)
    b = batch()
    cases["edits"] = case([edit(2000, b), edit(2500, b), edit(2600, [(b[0][0], ec.MISS, 0.0), (b[10][0], ec.SET, -9.0)])])
    hits = lambda keys: [(k, ec.UPDATE, 100.0) for k in keys]   # noqa: E731  a new voxel: clamp max, stamped with the clock
    e8, o8, b64, o64, c0, c7 = block(B_EQUAL), block(B_ODD), block(B_64, 4), block(B_64_ODD, 4), block(B_CHILD0), block(B_CHILD7)
    odd64 = [k for n, k in enumerate(o64) if (n % 4 // 2, n // 4 % 4 // 2, n // 16 // 2) == (1, 0, 1)]
    assert len(odd64) == 8
    late = [o8[3]] + odd64 + [c0[0], c7[7]]
    first = [k for k in e8 + o8 + b64 + o64 + c0 + c7 if k not in late]
    cases["blocks"] = case([edit(3000, hits(first)), edit(3001, hits(late)), snapshot(3010),
                            edit(3000, [(k, ec.DELETE, 0.0) for k in late] + hits(late)), snapshot(3020)])
    cases["resume"] = case(the_scans(count=2) + [edit(1015, hits(e8) + hits(o8[:7])), edit(1016, hits(o8[7:])), snapshot(1018), resume(1019),
                                                 the_scans()[2], snapshot(1025)], max_range=RANGE)
    cases["older"] = case(the_scans() + [sets, forget(1040, 35), forget(1040, 25), forget(900, (1 << 32) - 125)], max_range=RANGE)
    return cases


def check_cases(cases):
    """What the cases claim about themselves, by the restatement."""
    run = {name: sc.run_case(c, RESOLUTION) for name, c in cases.items()}
    r = run["scans"]
    keys, lo, stamps, _ = r[2]
    m = sc.Map(cases["scans"]["params"])
    assert ((lo == m.cmax) & (stamps == 1010)).sum() > 20, "scans: a wall hit three times keeps the stamp of the saturating hit"
    assert ((lo == m.cmin) & (stamps == 1010)).sum() > 100, "scans: free space saturates at clamp min and keeps that stamp"
    assert (stamps == 1020).sum() > 50 and set(np.unique(r[3][2])) == {1000, 1010, 1020, 1030}
    for name in ("scans_discrete", "scans_box", "scans_detect"):
        assert len(run[name][2][0]) > 100 and ((run[name][2][2] == 1010) & (run[name][2][1] == m.cmax)).sum() > 5, name
    assert len(run["scans_box"][2][0]) < len(r[2][0]) and not np.array_equal(run["scans_discrete"][2][0], r[2][0])
    r = run["degrade"]
    n = [s[3] for s in r[5:]]
    assert n[0] == 0 and 0 < n[1] < n[2] and n[3] > 0, f"degrade: nothing is old enough, some are, all are, the wrap makes all old: {n}"
    assert n[3] >= n[4] > 0 and n[6] == 0, f"degrade: repeated until nothing is occupied: {n}"
    assert np.array_equal(r[6][2], r[4][2]), "degrade: the stamps are untouched"
    assert (r[4][2] == 0).sum() == len(SET_KEYS) and n[8] == 0 and n[9] > 0, f"degrade: stamp 0 voxels; a hit stamps again, and ten ticks later it degrades again: {n}"
    r = run["edits"]
    a, b, c, d, e, f, g, h = [K(10 + i, -20 - i, 5 * i) for i in range(8)]
    at = dict(zip(map(int, r[0][0]), map(int, r[0][2])))
    assert at == {a: 2000, b: 2000, c: 0, d: 0, e: 0, f: 2000, g: 2000}, at
    at = dict(zip(map(int, r[1][0]), map(int, r[1][2])))
    assert at == {a: 2000, b: 2000, c: 0, d: 0, e: 0, f: 2500, g: 2000}, f"edits: at the clamps nothing is stamped the second time: {at}"
    at = dict(zip(map(int, r[2][0]), map(int, r[2][2])))
    assert at[a] == 2600 and at[e] == 0
    r = run["blocks"]
    (nodes1, root1, ot1), (ml1, mroot1, bt1) = r[2][4]
    (nodes2, root2, _), _ = r[4][4]
    at1 = {(int(k), int(d)): (int(st), int(lf)) for k, d, _, st, lf in zip(*nodes1)}
    at2 = {(int(k), int(d)): (int(st), int(lf)) for k, d, _, st, lf in zip(*nodes2)}
    centre = lambda corner, level: K(*[(c >> level << level) + (1 << (level - 1)) for c in corner])   # noqa: E731
    assert at1[(centre(B_EQUAL, 1), 15)] == (3000, 1), "blocks: equal stamps collapse to the common stamp"
    for b in (B_ODD, B_CHILD0, B_CHILD7):
        assert at1[(centre(b, 1), 15)] == (3010, 0) and at2[(centre(b, 1), 15)] == (3000, 1), "blocks: one odd stamp keeps eight leaves; made equal, they collapse"
    assert at1[(centre(B_64, 2), 14)] == (3000, 1) and at1[(centre(B_64_ODD, 2), 14)] == (3010, 0) and at2[(centre(B_64_ODD, 2), 14)] == (3000, 1)
    assert root1 == mroot1 == 3010 and root2 == 3020 and len(nodes1[0]) > len(nodes2[0]) and b"id OcTreeStamped" in ot1
    assert len(ml1[0]) == len(nodes1[0]), "blocks: every value is clamp max, so both readings have one structure"
    r = run["resume"]
    assert not r[5][2].any() and (r[6][2] == 1020).sum() > 0 and (r[6][2] == 0).sum() > 0, "resume: the loaded map has stamp 0, the next scan stamps"
    r = run["older"]
    n = [s[3] for s in r[5:]]
    assert 0 < n[0] and 0 < n[1] and n[2] > 0, f"older: every call forgets something, the last by the wrap: {n}"
    assert len(SET_KEYS) <= n[0] and len(r[-1][0]) > 0 and set(np.unique(r[-1][2])) == {1030}, "older: the stamp 0 voxels go first, and the youngest stay"
    return run


def step_bytes(s, max_range):
    head = kit.ints(s["kind"]) + struct.pack("<I", s["clock"])
    if s["kind"] == SCAN:
        box = np.asarray(s["box"], np.float32).tobytes() if s["flags"] & USE_BOX else b""
        return head + kit.ints(s["flags"]) + box + kit.scan(s["origin"], max_range, s["points"])
    if s["kind"] == EDIT:
        return head + kit.ints(len(s["keys"])) + kit.occ.unpack(s["keys"]).tobytes() + s["ops"].astype(np.uint8).tobytes() + s["values"].astype(np.float32).tobytes()
    if s["kind"] in (SNAPSHOT, RESUME):
        return head
    return head + struct.pack("<I", s["thres"])


def case_bytes(c, record=True):
    return kit.head(c["params"]) + kit.ints(int(record), len(c["steps"])) + b"".join(step_bytes(s, c["params"].max_range) for s in c["steps"])


def timed_cases():
    """The calls of tools/bench_occupancy_stamped.py on the map of its key frames -> {name: case}"""
    scans = kit.bench_scans()
    steps = [scan(1000 + 10 * i, o, p) for i, (o, _, p) in enumerate(scans)]
    return {"frames": dict(params=rc.RayParams(max_range=kit.BENCH_RANGE), steps=steps + [snapshot(1100), degrade(1100, 75), forget(1100, 85)])}


def take_voxels(r):
    n = r.one("<u4")
    k, v, s = kit.occ.pack(r.take("<u2", 3 * n)), r.take("<f4", n), r.take("<u4", n)
    order = np.argsort(k)
    return k[order].astype(np.uint64), v[order].copy(), s[order].copy()


NODE = np.dtype([("k", "<u2", 3), ("depth", "<u2"), ("value", "<f4"), ("stamp", "<u4")])


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

    code, raw = kit.run(kit.build(args.reference, "stamped", extra=["-DNDEBUG"]), "stamped", write)
    assert code == 0, code
    r = kit.Reader(raw)
    out = dict(resolution=np.float64(RESOLUTION), names=np.array(list(cases)))
    report = []
    for name, c in cases.items():
        out[f"{name}_constants"] = r.take("<f4", 5).copy()
        rec = dict(voxel_keys=[], voxel_values=[], voxel_stamps=[], nvoxels=[], counts=[], node_keys=[], node_depths=[], node_values=[],
                   node_stamps=[], node_leaf=[], nnodes=[], root_stamps=[], streams=[], nstream=[])
        for i, s in enumerate(c["steps"]):
            count = r.one("<u4") if s["kind"] in (DEGRADE, FORGET) else 0
            snap = []
            for _ in range(2 if s["kind"] == SNAPSHOT else 0):
                n = r.one("<u4")
                nd = r.take(NODE, n)
                leaf = r.take("u1", n).copy()
                root = r.one("<u4")
                data = r.stream().tobytes()
                snap.append(((kit.occ.pack(nd["k"]).astype(np.uint64), nd["depth"].astype(np.int32), nd["value"].copy(), nd["stamp"].copy(), leaf), root, data))
                rec["node_keys"].append(snap[-1][0][0]), rec["node_depths"].append(nd["depth"].astype(np.uint8)), rec["node_values"].append(nd["value"].copy())
                rec["node_stamps"].append(nd["stamp"].copy()), rec["node_leaf"].append(leaf), rec["nnodes"].append(n), rec["root_stamps"].append(root)
                rec["streams"].append(np.frombuffer(data, np.uint8)), rec["nstream"].append(len(data))
            vox = take_voxels(r)
            rec["voxel_keys"].append(vox[0]), rec["voxel_values"].append(vox[1]), rec["voxel_stamps"].append(vox[2])
            rec["nvoxels"].append(len(vox[0])), rec["counts"].append(count)
            assert sc.same(run[name][i], vox + (count,) + ((snap,) if snap else ())), f"{name}: step {i} differs from octomap"
        rp, st = c["params"], c["steps"]
        out[f"{name}_params"] = np.array([getattr(rp, k) for k in PROBS] + [rp.max_range], np.float64)
        out[f"{name}_steps"] = np.array([[s["kind"], s["clock"], len(s["keys"]), s["flags"], s["thres"]] for s in st], np.int64)
        out[f"{name}_keys"] = np.concatenate([s["keys"] for s in st]).astype(np.uint64)
        out[f"{name}_points"] = np.concatenate([s["points"] for s in st]).astype(np.float32).reshape(-1, 3)
        out[f"{name}_values"] = np.concatenate([s["values"] for s in st]).astype(np.float32)
        out[f"{name}_ops"] = np.concatenate([s["ops"] for s in st]).astype(np.uint8)
        out[f"{name}_origins"] = np.stack([s["origin"] for s in st])
        out[f"{name}_boxes"] = np.stack([s["box"] for s in st])
        for key, dt in (("voxel_keys", np.uint64), ("voxel_values", np.float32), ("voxel_stamps", np.uint32)):
            out[f"{name}_{key}"] = np.concatenate(rec[key]).astype(dt)
        for key, dt in (("node_keys", np.uint64), ("node_depths", np.uint8), ("node_values", np.float32), ("node_stamps", np.uint32), ("node_leaf", np.uint8),
                        ("streams", np.uint8)):
            out[f"{name}_{key}"] = np.concatenate(rec[key]).astype(dt) if rec[key] else np.zeros(0, dt)
        for key in ("nvoxels", "counts", "nnodes", "root_stamps", "nstream"):
            out[f"{name}_{key}"] = np.array(rec[key], np.uint32)
        report.append(f"{name}: {len(st)} steps, voxels {rec['nvoxels']}, counts {rec['counts']}")
    cpu = {}
    for name, c in timed.items():
        r.take("<f4", 5)
        ms = list(struct.unpack(f"<{len(c['steps'])}d", r.take(np.uint8, 8 * len(c["steps"])).tobytes()))
        cpu[name] = dict(insert_ms=[round(v, 3) for v in ms[:-3]], prune_update_ms=round(ms[-3], 3), degrade_ms=round(ms[-2], 3), forget_ms=round(ms[-1], 3))
    r.done()
    cpu_note = dict(what="octomap's own OcTreeStamped on the benchmark's key frames: insertPointCloud (lazy_eval) per frame, "
                         "degradeOutdatedNodes, and the leaf loop plus deleteNode that forgets by age; a figure across two machines "
                         "when set beside profiles/occupancy_stamped_bench_synth.json", build=" ".join(kit.CXX), threads=1, calls=cpu)
    OUT = kit.save(args.out, "stamped", out, cpu=cpu_note)
    print(f"{OUT}: {OUT.stat().st_size} bytes\n  " + "\n  ".join(report) + f"\n  cpu: {cpu}")


if __name__ == "__main__":
    main()
