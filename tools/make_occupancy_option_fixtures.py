#!/usr/bin/env python3
"""Writes tests/golden/occupancy_options.npz (+ .sha256): what the reference's OWN octomap answers for insertPointCloud with its
three insert switches -- discretize, the bounding box (setBBXMin / setBBXMax / useBBXLimit) and change detection
(enableChangeDetection / resetChangeDetection / changedKeys) -- after every scan the depth-16 leaves (key, float log-odds) of the
expanded tree and the changed keys with their flags (1: created, 0: occupancy flipped).

Run by hand, never by a test:

    python tools/make_occupancy_option_fixtures.py --reference /path/to/U96-SLAM [--out DIR]

It compiles its driver, tools/octomap_drivers/options.cpp (this project's text; it calls octomap's API only), against the
octomap sources vendored in the reference tree (tools/octomap_kit.py builds them once, outside the history), feeds it the scans
and keeps only inputs and recorded outputs. The driver is never fed a point whose floor fits no int. The cases:

    box_inside        256 rays of the ray fixture's `random` inside a box that holds them all: the result without a box
    box_exit          rays that end outside the box: free cells up to the face, nothing occupied
    origin_outside    the origin outside, the end inside: one occupied voxel and no free cell
    box_face          bounds that are no voxel boundaries; ends on max exactly, one float step beyond it, inside the max key's
                      voxel beyond the float bound, and one voxel further
    box_range         a point inside the box beyond max_range
    box_empty         min > max on one axis
    box_nokey_origin  the end in the box, the origin without a key
    created           a first scan under detection: free voxels are created too
    toggle            default probabilities: a hit, reset, three misses (flipped after the third), a hit (the entry is gone)
    created_then_flipped   a voxel created occupied and then freed stays created
    clamp_noop        a hit on a voxel already at clamp_max, after a reset
    enable_late / disabled / reset_between   the switch and the reset between two scans
    same_voxel        300 distinct points of one voxel, discretised: one ray
    wrap              x = 3300 discretised under a small max_range: the key wraps to 232
    disc_range        a point within range whose voxel centre is beyond it, and the reverse
    disc_duplicates_order / _perm   points with duplicates, and the same points permuted
    scene_all         the three 40 x 30 planes of tools/make_occupancy_fixtures.py discretised inside a box, detection on from
                      the second plane: created, flipped and unchanged voxels
"""
import numpy as np

import octomap_kit as kit
from octomap_kit import PROBS, RESOLUTION, f32, rc, up, voxel

import occupancy_option_cases as oc


def pts(*rows):
    return np.asarray(rows, np.float32).reshape(-1, 3)


def scan(origin, points, box=None, use_box=False, detect=False, discretize=False, reset_changes=False):
    return dict(origin=np.asarray(origin, np.float32), points=np.asarray(points, np.float32).reshape(-1, 3),
                box=None if box is None else (np.asarray(box[0], np.float32), np.asarray(box[1], np.float32)), use_box=use_box,
                detect=detect, discretize=discretize, reset_changes=reset_changes)


def case(scans, **probs):
    return dict(params=rc.RayParams(**probs), scans=scans)


def make_cases():
    cases = {}
    rays = kit.load("rays", "options")
    o, p = kit.scans_of(rays, "random")[0][0], kit.scans_of(rays, "random")[0][2][:256]
    cases["box_inside"] = case([scan(o, p, box=((-7, -7, -7), (7, 7, 7)), use_box=True)])
    o = (0.02, -0.03, 0.04)
    unit = ((-1, -1, -1), (1, 1, 1))
    dirs = pts((1, 0.2, 0.1), (-1, 0.3, -0.2), (0.1, 1, 0.3), (0.2, -1, 0.1), (0.3, 0.1, 1), (-0.2, 0.3, -1), (1, 1, 1), (-1, 1, -1))
    cases["box_exit"] = case([scan(o, np.add(o, dirs * f32(2.2)), box=unit, use_box=True)])
    cases["origin_outside"] = case([scan((2.0, 0.03, 0.04), pts((0.5, 0.1, 0.1)), box=unit, use_box=True)])
    hi = f32(0.57)
    face = pts((hi, 0.11, 0.12), (up(hi), 0.21, 0.12), (0.59, 0.31, 0.12), (0.75, -0.21, 0.12), (0.12, hi, 0.33), (0.12, 0.33, up(hi)))
    cases["box_face"] = case([scan(o, face, box=((-1.03, -1.03, -1.03), (hi, hi, hi)), use_box=True)])
    cases["box_range"] = case([scan(o, pts((3.0, 0.5, 0.2), (1.0, 0.5, 0.2)), box=((-5, -5, -5), (5, 5, 5)), use_box=True)], max_range=2.0)
    cases["box_empty"] = case([scan(o, pts((0.5, 0.1, 0.1), (-0.5, 0.2, 0.3)), box=((1, -1, -1), (-1, 1, 1)), use_box=True)])
    cases["box_nokey_origin"] = case([scan((4000.0, 0, 0), pts((0.5, 0.1, 0.1)), box=unit, use_box=True)])

    c = voxel((3, -2, 5))
    x = np.add(c, (0.8, 0.3, 0.1))                      # the voxel the toggles are about
    beyond = np.add(c, (1.6, 0.6, 0.2))                 # the same direction, twice as far: its ray crosses x
    cases["created"] = case([scan(c, pts(x, np.add(c, (0.5, -0.4, 0.2))), detect=True)])
    cases["toggle"] = case([scan(c, pts(x), detect=True)] + [scan(c, pts(beyond), detect=True, reset_changes=(k == 0)) for k in range(3)] +
                           [scan(c, pts(x), detect=True)])
    cases["created_then_flipped"] = case([scan(c, pts(x), detect=True), scan(c, pts(beyond), detect=True)], prob_miss=0.2)
    cases["clamp_noop"] = case([scan(c, pts(x), detect=True), scan(c, pts(x), detect=True),
                                scan(c, pts(x), detect=True, reset_changes=True)], clamp_max=0.75)
    other = pts(np.add(c, (0.5, -0.4, 0.2)), beyond)
    cases["enable_late"] = case([scan(c, pts(x)), scan(c, other, detect=True)], prob_miss=0.2)
    cases["disabled"] = case([scan(c, pts(x), detect=True), scan(c, other)], prob_miss=0.2)
    cases["reset_between"] = case([scan(c, pts(x), detect=True), scan(c, other, detect=True, reset_changes=True)], prob_miss=0.2)

    rng = np.random.default_rng(11)
    lo = voxel((30, 12, -7)) - 0.05
    same = (lo + rng.uniform(0.002, 0.098, (300, 3))).astype(np.float32)
    cases["same_voxel"] = case([scan(o, same, discretize=True)])
    cases["wrap"] = case([scan((0, 0, 0), pts((3300.0, 0.02, 0.03)), discretize=True)], max_range=2.0)
    cases["disc_range"] = case([scan((0, 0.03, 0), pts((0.91, 0.03, 0.0), (0.0, 0.99, 0.0)), discretize=True)], max_range=0.93)
    dup = (np.float32([0.3, -0.2, 0.1]) + rng.uniform(-1.5, 1.5, (40, 3))).astype(np.float32)
    dup = np.concatenate([dup, dup[::3], dup[5:9] + f32(0.001)])
    cases["disc_duplicates_order"] = case([scan(o, dup, discretize=True)])
    cases["disc_duplicates_order_perm"] = case([scan(o, dup[rng.permutation(len(dup))], discretize=True)])

    disp, poses, m = kit.scene("options")
    cases["scene_all"] = case([scan(pose[[3, 7, 11]], rc.plane_points(d, 4, m, pose), box=((-1.53, -2.07, -0.33), (3.47, 3.03, 2.52)),
                                    use_box=True, detect=i > 0, discretize=True) for i, (d, pose) in enumerate(zip(disp, poses))], max_range=6.0)
    return cases


def check_cases(cases):
    """What the cases claim about themselves, by the restatement."""
    run = {name: oc.run_case(c, RESOLUTION) for name, c in cases.items()}
    res = RESOLUTION

    def sets(name, s=0, box=True, disc=None):
        c, sc = cases[name], cases[name]["scans"][s]
        b = oc.Box(res)
        if sc["box"] is not None:
            assert b.set(*sc["box"])
        p = sc["points"]
        if sc["discretize"] if disc is None else disc:
            p = oc.discretize(p, res)
        return oc.scan_sets(p, sc["origin"], c["params"].max_range, res, b if box and sc["use_box"] else None)

    def vox(p):
        return rc.pack3(rc.key3(np.float32(p), 1.0 / res))

    s = cases["box_inside"]["scans"][0]
    plain = rc.Tree().insert(s["points"], s["origin"]).leaves()
    assert np.array_equal(run["box_inside"][0][0], plain[0]) and np.array_equal(kit.bits(run["box_inside"][0][1]), kit.bits(plain[1]))
    free, occ = sets("box_exit")
    assert not occ and {k >> 32 for k in free} >= {32768 - 10, 32768 + 10} and max(k >> 32 for k in free) == 32768 + 10
    assert len(free) < len(sets("box_exit", box=False)[0])
    assert sets("origin_outside") == (set(), {vox((0.5, 0.1, 0.1))})
    free, occ = sets("box_face")
    face = cases["box_face"]["scans"][0]["points"]
    assert occ == {vox(face[0]), vox(face[4])}, "box_face: only the ends on max are occupied"
    assert all(k >> 32 <= 32768 + 5 for k in free), "box_face: a free cell beyond the max key"
    assert any(k >> 32 == 32768 + 5 for k in free), "box_face: no free cell in the max key's voxel"
    free, occ = sets("box_range")
    assert occ == {vox((1.0, 0.5, 0.2))} and vox((3.0, 0.5, 0.2)) not in free and len(free) > 20
    assert sets("box_empty") == (set(), set())
    assert sets("box_nokey_origin") == (set(), {vox((0.5, 0.1, 0.1))})

    xk = vox(cases["toggle"]["scans"][0]["points"][0])
    keys, lo, ck, cf = run["created"][0]
    assert np.array_equal(keys, ck) and cf.all() and (lo < 0).any(), "created: not every voxel, free ones included, is created"
    t = run["toggle"]
    value = [float(lo[list(k).index(xk)]) for k, lo, _, _ in t]
    assert [round(v, 2) for v in value] == [0.85, 0.44, 0.04, -0.37, 0.48], value        # 0.8473 - k * 0.4055, then + 0.8473
    state = [dict(zip(map(int, ck), cf)).get(xk) for _, _, ck, cf in t]
    assert state == [1, None, None, 0, None], state
    assert all(len(ck) for _, _, ck, _ in t[1:]), "toggle: the far end point is created after the reset"
    a, b = run["created_then_flipped"]
    assert dict(zip(map(int, b[2]), b[3]))[xk] == 1 and b[1][list(b[0]).index(xk)] < 0
    n = run["clamp_noop"]
    assert len(n[2][2]) == 0 and kit.bits(n[2][1][list(n[2][0]).index(xk)]) == kit.bits(rc.logodds(0.75))
    late = run["enable_late"][1]
    assert dict(zip(map(int, late[2]), late[3]))[xk] == 0 and late[3].sum() > 0 and len(late[2]) < len(late[0])
    d0, d1 = run["disabled"]
    assert np.array_equal(d0[2], d1[2]) and np.array_equal(d0[3], d1[3]) and len(d1[0]) > len(d0[0])
    r0, r1 = run["reset_between"]
    assert not set(map(int, r1[2])) & (set(map(int, r0[2])) - {xk}) and dict(zip(map(int, r1[2]), r1[3]))[xk] == 0

    sc = cases["same_voxel"]["scans"][0]
    assert len(oc.discretize(sc["points"], res)) == 1 and len(np.unique(sc["points"], axis=0)) == 300
    assert sets("same_voxel")[1] == sets("same_voxel", disc=False)[1] and sets("same_voxel")[0] != sets("same_voxel", disc=False)[0]
    w = oc.discretize(cases["wrap"]["scans"][0]["points"], res)
    assert oc.wrapped_key(3300.0, 10.0) == 232 and kit.bits(w[0][0]) == kit.bits(np.float32(-3253.55))
    free, occ = sets("wrap")
    assert not occ and min(k >> 32 for k in free) < 32768 - 15 and max(k >> 32 for k in free) == 32768
    sc = cases["disc_range"]["scans"][0]
    d = oc.discretize(sc["points"], res)
    dist = [rc.norm(rc.sub3(q, sc["origin"])) for q in list(sc["points"]) + list(d)]
    assert dist[0] <= 0.93 < dist[2] and dist[3] <= 0.93 < dist[1], dist
    assert sets("disc_range")[1] == {vox(sc["points"][1])} and sets("disc_range", disc=False)[1] == {vox(sc["points"][0])}
    a, b = run["disc_duplicates_order"][0], run["disc_duplicates_order_perm"][0]
    assert np.array_equal(a[0], b[0]) and np.array_equal(kit.bits(a[1]), kit.bits(b[1]))
    assert not np.array_equal(cases["disc_duplicates_order"]["scans"][0]["points"], cases["disc_duplicates_order_perm"]["scans"][0]["points"])
    last = run["scene_all"][-1]
    assert 0 < last[3].sum() < len(last[3]) and len(last[2]) < len(last[0]), "scene_all: no mix of created, flipped and unchanged"
    return run


def main():
    args = kit.arguments(__doc__)
    cases = make_cases()
    check_cases(cases)

    def write(f):
        f.write(kit.ints(len(cases)))
        for c in cases.values():
            f.write(kit.head(c["params"]) + kit.ints(len(c["scans"])))
            for s in c["scans"]:
                sw = s["use_box"] | s["detect"] << 1 | s["discretize"] << 2 | s["reset_changes"] << 3 | (s["box"] is not None) << 4
                f.write(kit.ints(sw))
                if s["box"] is not None:
                    f.write(s["box"][0].tobytes() + s["box"][1].tobytes())
                f.write(kit.scan(s["origin"], c["params"].max_range, s["points"]))

    code, raw = kit.run(kit.build(args.reference, "options"), "options", write)
    assert code == 0, code
    r = kit.Reader(raw)
    out = dict(resolution=np.float64(RESOLUTION), names=np.array(list(cases)))
    report = []
    for name, c in cases.items():
        out[f"{name}_constants"] = r.take("<f4", 5).copy()
        keys, values, ckeys, cflags, nleaves, nchanges = [], [], [], [], [], []
        for _ in c["scans"]:
            n = r.one("<u4")
            k, v = r.voxels(n)
            m = r.one("<u4")
            ck, cf = kit.occ.pack(r.take("<u2", 3 * m)), r.take("u1", m)
            order = np.argsort(ck)
            keys.append(k), values.append(v), ckeys.append(ck[order]), cflags.append(cf[order]), nleaves.append(n), nchanges.append(m)
        rp, scans = c["params"], c["scans"]
        out[f"{name}_params"] = np.array([getattr(rp, k) for k in PROBS] + [rp.max_range], np.float64)
        out[f"{name}_origins"] = np.stack([s["origin"] for s in scans])
        out[f"{name}_points"] = np.concatenate([s["points"] for s in scans])
        out[f"{name}_npoints"] = np.array([len(s["points"]) for s in scans], np.int32)
        # per scan: use_box, detect, discretize, reset_changes, a box is set
        out[f"{name}_switches"] = np.array([[s["use_box"], s["detect"], s["discretize"], s["reset_changes"], s["box"] is not None]
                                            for s in scans], np.uint8)
        out[f"{name}_boxes"] = np.stack([np.concatenate(s["box"]) if s["box"] is not None else np.zeros(6, np.float32) for s in scans])
        out[f"{name}_nleaves"] = np.array(nleaves, np.uint32)
        out[f"{name}_keys"] = np.concatenate(keys)
        out[f"{name}_logodds"] = np.concatenate(values)
        out[f"{name}_nchanges"] = np.array(nchanges, np.uint32)
        out[f"{name}_changed_keys"] = np.concatenate(ckeys).astype(np.uint64)
        out[f"{name}_changed_created"] = np.concatenate(cflags).astype(np.uint8)
        report.append(f"{name}: {len(scans)} scans, {nleaves[-1]} leaves, {nchanges[-1]} changes")
    r.done()
    disp, poses, m = kit.scene("options")
    out["scene_disp"], out["scene_poses"], out["scene_model"], out["scene_scale"] = disp, poses, kit.occ.model_to_array(m), np.int32(4)
    OUT = kit.save(args.out, "options", out)
    print(f"{OUT}: {OUT.stat().st_size} bytes\n  " + "\n  ".join(report))


if __name__ == "__main__":
    main()
