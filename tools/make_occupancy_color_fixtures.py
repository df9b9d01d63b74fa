#!/usr/bin/env python3
"""Writes tests/golden/occupancy_color.npz (+ .sha256) and tests/golden/occupancy_color_cpu.json: what the reference's OWN octomap
(ColorOcTree) answers for setNodeColor and averageNodeColor by key and by point in item order, for the colours of the tree
after prune(); updateInnerOccupancy(); (begin_leafs at maxDepth 16, 15, 12 and 0), for AbstractOcTree::write of that tree and what
read() makes of the stream, and for a run resumed from its own stream -- and octomap's CPU time for the calls
tools/bench_occupancy_color.py times.

Run by hand, never by a test:

    python tools/make_occupancy_color_fixtures.py --reference /path/to/U96-SLAM [--out DIR]

It compiles its driver, tools/octomap_drivers/color.cpp (this project's text; it calls octomap's API only), against the octomap
sources vendored in the reference tree (tools/octomap_kit.py builds them once, outside the history), feeds it the steps and keeps
only inputs and recorded outputs. octomap is driven with lazy_eval = true inserts and edits, so that it never prunes while it
inserts, and is coloured by key on the unpruned tree: the divergence include/sbm.h states. Through the restatement
tests/occupancy_color_cases.py the generator asserts what each case claims, and equality with octomap in every recorded integer,
float bit and byte. The cases:

    scans      three scans of the 40 x 30 planes of tools/make_occupancy_fixtures.py; between them AVERAGE by the scan's own points
               (with points outside the key space and points of unknown voxels), SET by key after AVERAGE, AVERAGE after SET
    run300     300 items of one voxel in one call, interleaved with two other voxels' items, white given as a colour in mid-chain,
               unknown keys, a key with a bit above 47; then SET after AVERAGE and AVERAGE after SET across calls
    blocks     designed blocks at clamp max: a 2^3 block whose child 0 is white and whose siblings are coloured (collapses to
               white), one whose child 0 is set with white siblings (the average over the set ones), a 4^3 block collapsing over two
               levels, and a block that does not collapse (the inner average)
    reborn     coloured voxels deleted and created again inside ONE edit batch (delete then set, delete then update, set delete set),
               beside ones that keep their colour and one that ends absent; then colours on the new voxels
    resume     a scan and a block, colours, then write / read / expand(), one more scan and one more colour batch
"""
import struct

import numpy as np

import octomap_kit as kit
from octomap_kit import PROBS, RESOLUTION, rc

import occupancy_color_cases as cc
from occupancy_color_cases import AVERAGE, COLOR, EDIT, RESUME, SCAN, SET, SET_VALUES, SNAPSHOT, WHITE, ec


def K(i, j, k):
    return rc.pack3((32768 + i, 32768 + j, 32768 + k))


def _step(kind, n, **kw):
    s = dict(kind=kind, form=0, op=0, keys=np.zeros(n, np.uint64), points=np.zeros((n, 3), np.float32), words=np.zeros(n, np.uint32),
             values=np.zeros(n, np.float32), ops=np.zeros(n, np.uint8), origin=np.zeros(3, np.float32))
    s.update(kw)
    return s


def scan(origin, points):
    p = np.asarray(points, np.float32).reshape(-1, 3)
    return _step(SCAN, len(p), points=p, origin=np.asarray(origin, np.float32))


def color(items, op):
    """items: (key, word)"""
    return _step(COLOR, len(items), op=op, keys=np.array([i[0] for i in items], np.uint64), words=np.array([i[1] for i in items], np.uint32))


def color_points(points, words, op):
    p = np.asarray(points, np.float32).reshape(-1, 3)
    return _step(COLOR, len(p), form=1, op=op, points=p, words=np.asarray(words, np.uint32))


def set_values(items):
    """items: (key, value)"""
    return _step(SET_VALUES, len(items), keys=np.array([i[0] for i in items], np.uint64), values=np.array([i[1] for i in items], np.float32))


def edit(items):
    """items: (key, ec.UPDATE | ec.SET | ec.DELETE, value)"""
    return _step(EDIT, len(items), keys=np.array([i[0] for i in items], np.uint64), ops=np.array([i[1] for i in items], np.uint8),
                 values=np.array([i[2] for i in items], np.float32))


def snapshot():
    return _step(SNAPSHOT, 0)


def resume():
    return _step(RESUME, 0)


def case(steps, **probs):
    return dict(params=rc.RayParams(**probs), steps=steps)


BLOCK_WHITE0, BLOCK_SET0, BLOCK_64, BLOCK_OPEN = (64, -32, 16), (-20, 40, 8), (128, 64, 32), (-64, -64, -64)


def block(corner, side=2):
    return [K(corner[0] + i, corner[1] + j, corner[2] + k) for k in range(side) for j in range(side) for i in range(side)]


def make_cases():
    cases = {}
    rng = np.random.default_rng(29)
    disp, poses, m = kit.scene("color")
    pts = [rc.plane_points(dd, 4, m, pose) for dd, pose in zip(disp, poses)]
    words = [rng.integers(0, 1 << 24, len(p)).astype(np.uint32) for p in pts]
    outside = np.float32([[4000.0, 0, 0], [0.1, np.nan, 0.2], [0.5, 0.5, np.inf], [1.0, 1.0, 3276.8]])
    unknown = np.float32([[30.05, 30.05, 30.05], [-30.05, 1.0, 2.0]])
    first = np.concatenate([pts[0][:700], outside, unknown, pts[0][::-1][:400]])
    mid = [rc.pack3(rc.key3(p, 10.0)) for p in pts[0][::37][:12]]
    cases["scans"] = case([scan(poses[0][[3, 7, 11]], pts[0]),
                           color_points(first, rng.integers(0, 1 << 24, len(first)).astype(np.uint32), AVERAGE),
                           scan(poses[1][[3, 7, 11]], pts[1]),
                           color([(k, int(w)) for k, w in zip(mid, rng.integers(0, 1 << 24, len(mid)))], SET),
                           color_points(pts[1], words[1], AVERAGE),
                           scan(poses[2][[3, 7, 11]], pts[2]),
                           color_points(pts[2][::3], words[2][::3] | np.uint32(0xFF000000), AVERAGE),      # the top byte is ignored
                           snapshot()], max_range=6.0)
    a, b, c, far = K(3, -2, 5), K(-40, 17, 9), K(7, 7, 7), K(900, -700, 300)
    chain = []
    for i in range(300):
        chain.append((a, WHITE if i == 150 else int(rng.integers(0, 1 << 24))))
        if i % 3 == 0:
            chain.append((b, int(rng.integers(0, 1 << 24))))
        if i % 50 == 0:
            chain += [(K(500, 500, 500), 0x123456), (a | 1 << 48, 0x654321), (c, int(rng.integers(0, 1 << 24)))]
    assert sum(1 for k, _ in chain if k == a) == 300
    cases["run300"] = case([set_values([(a, 0.5), (b, -0.5), (c, 1.5), (far, 1.0)]), color(chain, AVERAGE),
                            color([(a, 0x102030), (b, WHITE)], SET), color([(a, 0x506070), (b, 0x0A0B0C), (far, 0x010203)], AVERAGE),
                            color([(far, 0x0000FF), (far, 0x00FF00), (c, 0x111111)], SET), snapshot()])
    # every value is beyond clamp max, so every stored value IS clamp max and the full blocks collapse
    w0, s0, big, opened = block(BLOCK_WHITE0), block(BLOCK_SET0), block(BLOCK_64, 4), block(BLOCK_OPEN)
    values = [(k, 100.0) for k in w0 + s0 + big + opened[:-1]] + [(opened[-1], 0.25)]
    paint = [(k, int(rng.integers(0, 0xFFFFFF))) for k in w0[1:]]                               # child 0 stays white
    paint += [(s0[0], 0x0A141E)] + [(k, int(rng.integers(0, 0xFFFFFF))) for k in s0[1:5]]     # children 5, 6, 7 stay white
    # the 4^3 block: sub-blocks with child 0 white, with every child white, and fully painted ones
    for n, k in enumerate(big):
        i, j, kk = n % 4, n // 4 % 4, n // 16
        sub = (i // 2, j // 2, kk // 2)
        first_child = (i % 2, j % 2, kk % 2) == (0, 0, 0)
        if sub == (1, 1, 1) or (sub == (1, 0, 0) and first_child):
            continue
        paint.append((k, int(rng.integers(0, 0xFFFFFF))))
    paint += [(k, int(rng.integers(0, 0xFFFFFF))) for k in opened[2:]]
    cases["blocks"] = case([set_values(values), color(paint, SET), snapshot()])
    ks = [K(i, -i, 2 * i) for i in range(1, 9)]
    kw = [(k, int(rng.integers(0, 0xFFFFFF))) for k in ks]
    a, b, c, d, e, f = ks[:6]
    cases["reborn"] = case([set_values([(k, 0.5 + 0.1 * i) for i, k in enumerate(ks)] + [(far, 1.0)]), color(kw, SET),
                            edit([(a, ec.DELETE, 0.0), (a, ec.SET, 1.25), (b, ec.DELETE, 0.0), (b, ec.UPDATE, 0.75), (c, ec.SET, 2.0), (c, ec.DELETE, 0.0),
                                  (c, ec.SET, -1.0), (d, ec.SET, 0.25), (d, ec.UPDATE, 0.5), (e, ec.DELETE, 0.0), (f, ec.UPDATE, 0.1), (a, ec.UPDATE, 0.5)]),
                            color([(a, 0x111111), (e, 0x222222), (d, 0x333333)], AVERAGE), snapshot()])
    few = pts[0][::2]
    cases["resume"] = case([scan(poses[0][[3, 7, 11]], few), set_values([(k, 100.0) for k in s0 + w0]),
                            color_points(few, words[0][::2], AVERAGE), color(paint[:12], SET), snapshot(), resume(),
                            scan(poses[1][[3, 7, 11]], pts[1][::2]), color_points(pts[1][::2], words[1][::2], AVERAGE),
                            color([(s0[3], 0x334455), (w0[0], 0x010101)], AVERAGE), snapshot()], max_range=6.0)
    return cases


def check_cases(cases):
    """What the cases claim about themselves, by the restatement."""
    run = {name: cc.run_case(c, RESOLUTION) for name, c in cases.items()}
    r = run["scans"]
    assert cases["scans"]["steps"][1]["points"].shape[0] - r[1][3] >= 6 and 0 < r[1][3], "scans: items outside and unknown are not found"
    assert (r[6][2] != WHITE).sum() > 500 and (r[6][2] == WHITE).sum() > 0 and (r[6][2] >> 24).max() == 0
    lists = r[7][0]
    assert len(lists[0][0]) > len(lists[1][0]) > len(lists[2][0]) > 1 and len(lists[3][0]) == len(lists[0][0]), "maxDepth 0 means 16"
    r = run["run300"]
    a, b = K(3, -2, 5), K(-40, 17, 9)
    col = dict(zip(map(int, r[1][0]), map(int, r[1][2])))
    t = WHITE
    for k, w in [(k, w) for k, w in zip(cases["run300"]["steps"][1]["keys"], cases["run300"]["steps"][1]["words"]) if int(k) == a][151:]:
        t = cc.step_color(t, w, AVERAGE)
    assert col[a] == t and t != WHITE, "run300: the chain starts over after white"
    assert r[1][3] == 300 + 100 + 6, r[1][3]
    col = dict(zip(map(int, r[2][0]), map(int, r[2][2])))
    assert col[a] == 0x102030 and col[b] == WHITE
    col = dict(zip(map(int, r[3][0]), map(int, r[3][2])))
    assert col[a] == 0x304050 and col[b] == 0x0A0B0C, "run300: AVERAGE after SET, and from white the colour itself"
    r = run["blocks"]
    keys, depth, _, words = r[2][0][0]
    at = {(int(k), int(d)): int(w) for k, d, w in zip(keys, depth, words)}
    centre = lambda corner, level: K(*[(c >> level << level) + (1 << (level - 1)) for c in corner])   # noqa: E731
    assert at[(centre(BLOCK_WHITE0, 1), 15)] == WHITE, "blocks: child 0 white collapses to white"
    got = at[(centre(BLOCK_SET0, 1), 15)]
    assert got != WHITE and got == cc.average_child_color([w for w in r[1][2][np.isin(r[1][0], block(BLOCK_SET0))]]), "blocks: the average over the set ones"
    assert (centre(BLOCK_64, 2), 14) in at and (centre(BLOCK_OPEN, 1), 15) not in at, "blocks: two levels collapse, the open block does not"
    k15 = r[2][0][1]
    assert (centre(BLOCK_OPEN, 1), 15) in {(int(k), int(d)) for k, d in zip(k15[0], k15[1])}, "blocks: the inner node shows at maxDepth 15"
    r = run["reborn"]
    ks = [K(i, -i, 2 * i) for i in range(1, 9)]
    col = dict(zip(map(int, r[2][0]), map(int, r[2][2])))
    before = dict(zip(map(int, r[1][0]), map(int, r[1][2])))
    assert col[ks[0]] == col[ks[1]] == col[ks[2]] == WHITE and col[ks[3]] == before[ks[3]] != WHITE and ks[4] not in col, "reborn: created again is white"
    assert r[3][3] == 2 and dict(zip(map(int, r[3][0]), map(int, r[3][2])))[ks[0]] == 0x111111
    r = run["resume"]
    assert not np.array_equal(r[4][2][2], r[3][2]) and np.array_equal(r[5][2], r[4][2][2]), "resume: the loaded map holds the collapsed colours"
    return run


def step_bytes(s, max_range):
    head = kit.ints(s["kind"])
    if s["kind"] == SCAN:
        return head + kit.scan(s["origin"], max_range, s["points"])
    if s["kind"] == COLOR:
        items = s["points"].astype(np.float32).tobytes() if s["form"] else kit.occ.unpack(s["keys"]).tobytes()
        w = s["words"].astype(np.uint32)
        rgb = np.stack([w & 255, w >> 8 & 255, w >> 16 & 255], axis=1).astype(np.uint8)
        return head + kit.ints(s["form"], s["op"], len(w)) + items + rgb.tobytes()
    if s["kind"] == SET_VALUES:
        return head + kit.ints(len(s["keys"])) + kit.occ.unpack(s["keys"]).tobytes() + s["values"].astype(np.float32).tobytes()
    if s["kind"] == EDIT:
        return head + kit.ints(len(s["keys"])) + kit.occ.unpack(s["keys"]).tobytes() + s["ops"].astype(np.uint8).tobytes() + s["values"].astype(np.float32).tobytes()
    return head


def for_octomap(c):
    """The case as octomap can take it: an item whose key has a bit above 47 has no OcTreeKey, so it is left out (the device skips it)"""
    steps = []
    for s in c["steps"]:
        if s["kind"] == COLOR and not s["form"]:
            ok = (s["keys"] >> np.uint64(48)) == 0
            s = dict(s, keys=s["keys"][ok], words=s["words"][ok])
        steps.append(s)
    return dict(c, steps=steps)


def case_bytes(c, record=True):
    c = for_octomap(c)
    return kit.head(c["params"]) + kit.ints(int(record), len(c["steps"])) + b"".join(step_bytes(s, c["params"].max_range) for s in c["steps"])


def timed_cases():
    """The calls of tools/bench_occupancy_color.py on the map of its key frames -> {name: case}"""
    import bench_occupancy_color as bc
    scans = kit.bench_scans()
    pts, words = bc.frame_batch()
    return {"frame_average": case([scan(o, p) for o, _, p in scans] + [color_points(pts, words, AVERAGE), snapshot()], max_range=kit.BENCH_RANGE)}


def take_voxels(r):
    n = r.one("<u4")
    k, v, rgb = kit.occ.pack(r.take("<u2", 3 * n)), r.take("<f4", n), r.take("u1", 3 * n).reshape(-1, 3).astype(np.uint32)
    order = np.argsort(k)
    return k[order].astype(np.uint64), v[order].copy(), (rgb[:, 0] | rgb[:, 1] << 8 | rgb[:, 2] << 16).astype(np.uint32)[order]


LEAF = np.dtype([("k", "<u2", 3), ("depth", "<u2"), ("value", "<f4"), ("rgb", "u1", 4)])


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

    code, raw = kit.run(kit.build(args.reference, "color", extra=["-DNDEBUG"]), "color", write)
    assert code == 0, code
    r = kit.Reader(raw)
    out = dict(resolution=np.float64(RESOLUTION), names=np.array(list(cases)))
    report = []
    for name, c in cases.items():
        out[f"{name}_constants"] = r.take("<f4", 5).copy()
        rec = dict(voxel_keys=[], voxel_values=[], voxel_words=[], nvoxels=[], found=[], leaf_keys=[], leaf_depths=[], leaf_values=[],
                   leaf_words=[], nleaves=[], streams=[], nstream=[])
        for i, s in enumerate(c["steps"]):
            found = 0
            if s["kind"] == SNAPSHOT:
                lists = []
                for _ in cc.DEPTHS:
                    n = r.one("<u4")
                    lf = r.take(LEAF, n)
                    w = lf["rgb"].astype(np.uint32)
                    lists.append((kit.occ.pack(lf["k"]).astype(np.uint64), lf["depth"].astype(np.int32), lf["value"].copy(),
                                  (w[:, 0] | w[:, 1] << 8 | w[:, 2] << 16).astype(np.uint32)))
                data = r.stream().tobytes()
                assert r.one("<i4") == 1, f"{name}: octomap does not read its own stream back"
                vox = take_voxels(r)
                theirs = (lists, data, vox)
                for ls in lists:
                    rec["leaf_keys"].append(ls[0]), rec["leaf_depths"].append(ls[1].astype(np.uint8)), rec["leaf_values"].append(ls[2])
                    rec["leaf_words"].append(ls[3]), rec["nleaves"].append(len(ls[0]))
                rec["streams"].append(np.frombuffer(data, np.uint8)), rec["nstream"].append(len(data))
            else:
                if s["kind"] == COLOR:
                    found = r.one("<u4")
                vox = take_voxels(r)
                theirs = vox + (found,)
            rec["voxel_keys"].append(vox[0]), rec["voxel_values"].append(vox[1]), rec["voxel_words"].append(vox[2])
            rec["nvoxels"].append(len(vox[0])), rec["found"].append(found)
            assert cc.same(run[name][i], theirs), f"{name}: step {i} differs from octomap"
        rp = c["params"]
        st = c["steps"]
        out[f"{name}_params"] = np.array([getattr(rp, k) for k in PROBS] + [rp.max_range], np.float64)
        out[f"{name}_steps"] = np.array([[s["kind"], len(s["keys"]), s["form"], s["op"]] for s in st], np.int32)
        out[f"{name}_keys"] = np.concatenate([s["keys"] for s in st]).astype(np.uint64)
        out[f"{name}_points"] = np.concatenate([s["points"] for s in st]).astype(np.float32).reshape(-1, 3)
        out[f"{name}_words"] = np.concatenate([s["words"] for s in st]).astype(np.uint32)
        out[f"{name}_values"] = np.concatenate([s["values"] for s in st]).astype(np.float32)
        out[f"{name}_ops"] = np.concatenate([s["ops"] for s in st]).astype(np.uint8)
        out[f"{name}_origins"] = np.stack([s["origin"] for s in st])
        for key, dt in (("voxel_keys", np.uint64), ("voxel_values", np.float32), ("voxel_words", np.uint32), ("leaf_keys", np.uint64),
                        ("leaf_depths", np.uint8), ("leaf_values", np.float32), ("leaf_words", np.uint32), ("streams", np.uint8)):
            out[f"{name}_{key}"] = np.concatenate(rec[key]).astype(dt) if rec[key] else np.zeros(0, dt)
        for key in ("nvoxels", "found", "nleaves", "nstream"):
            out[f"{name}_{key}"] = np.array(rec[key], np.uint32)
        report.append(f"{name}: {len(st)} steps, {rec['nvoxels'][-1]} voxels, streams {rec['nstream']}")
    cpu = {}
    for name, c in timed.items():
        r.take("<f4", 5)
        ms = []
        for s in c["steps"]:
            if s["kind"] in (COLOR, SNAPSHOT):
                n = 1 if s["kind"] == COLOR else 3
                ms += list(struct.unpack(f"<{n}d", r.take(np.uint8, 8 * n).tobytes()))
        cpu[name] = dict(color_batch_ms=round(ms[0], 3), prune_update_ms=round(ms[1], 3), write_ms=round(ms[2], 3), read_ms=round(ms[3], 3))
    r.done()
    cpu_note = dict(what="octomap's own averageNodeColor loop over one 640 x 480 frame's points on the map of the benchmark's key frames, "
                         "its prune() + updateInnerOccupancy(), write() and read() of that tree; a figure across two machines when set "
                         "beside profiles/occupancy_color_bench_synth.json", build=" ".join(kit.CXX), threads=1, calls=cpu)
    OUT = kit.save(args.out, "color", out, cpu=cpu_note)
    print(f"{OUT}: {OUT.stat().st_size} bytes\n  " + "\n  ".join(report) + f"\n  cpu: {cpu}")


if __name__ == "__main__":
    main()
