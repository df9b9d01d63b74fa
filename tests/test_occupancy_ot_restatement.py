"""The transcription tests/occupancy_ot_cases.py against what the reference's octomap wrote and read
(tests/golden/occupancy_ot.npz), and against itself: no GPU, no library.

write: for every recorded scene after every scan, the transcription's stream of the recorded voxels equals octomap's bytes.
parse: the leaves octomap's read() left; parse o write is the identity on random trees; the device parse's formulas (include/sbm.h,
"Device") give the same leaves as the recursive parser."""
import hashlib
import pathlib
import sys

import numpy as np
import pytest

ROOT = pathlib.Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "tests"))
import occupancy_ot_cases as oc  # noqa: E402
import occupancy_ray_cases as rc  # noqa: E402

FX = oc.fixture()
RAYS = dict(np.load(ROOT / "tests" / "golden" / "occupancy_rays.npz"))
NAMES = [str(n) for n in FX["names"]]


def bits(a):
    return np.asarray(a, np.float32).view(np.uint32)


def scan_voxels(name):
    """per scan {packed key: float32} of the recorded scene: the rays fixture holds octomap's leaves after every scan"""
    ends = np.cumsum(RAYS[f"{name}_nleaves"])
    for s, e in enumerate(ends):
        b = e - RAYS[f"{name}_nleaves"][s]
        yield s, dict(zip(RAYS[f"{name}_keys"][b:e].tolist(), RAYS[f"{name}_logodds"][b:e]))


def test_fixture_is_what_the_generator_wrote():
    path = ROOT / "tests" / "golden" / "occupancy_ot.npz"
    assert path.stat().st_size < 512 * 1024
    assert hashlib.sha256(path.read_bytes()).hexdigest() == path.with_suffix(".sha256").read_text().split()[0]
    assert NAMES == [str(n) for n in RAYS["names"]]
    assert sorted(oc.hand_built()) == sorted(str(n) for n in FX["hand_built"])
    for name, data in oc.hand_built().items():
        assert bytes(FX[f"hand_{name}"]) == data, name
    for name, (data, code) in oc.malformed(bytes(FX["scene_ot_0"])).items():
        assert bytes(FX[f"bad_{name}"]) == data and int(FX[f"bad_{name}_code"]) == code, name


@pytest.mark.parametrize("name", NAMES)
def test_write_against_octomap(name):
    for s, voxels in scan_voxels(name):
        assert oc.write(voxels, 0.1) == bytes(FX[f"{name}_ot_{s}"]), (name, s)
    assert s + 1 == len(FX[f"{name}_search_found"])


@pytest.mark.parametrize("name", NAMES)
def test_parse_against_octomap(name):
    for s, voxels in scan_voxels(name):
        p = oc.parse(bytes(FX[f"{name}_ot_{s}"]), 0.1)
        assert p.status == oc.OK and p.size == p.nodes == int(FX[f"{name}_num_nodes_{s}"]) == int(FX[f"{name}_size_{s}"])
        ck, cd = oc.centre_leaves(p)
        assert np.array_equal(ck, FX[f"{name}_leaf_key_{s}"]) and np.array_equal(cd, FX[f"{name}_leaf_depth_{s}"])
        assert np.array_equal(oc.leaf_arrays(p)[2], bits(FX[f"{name}_leaf_value_{s}"]))
        if p.voxels <= 4096:
            k, v = oc.expand(p)
            want = sorted(voxels)
            assert k.tolist() == want and np.array_equal(bits(v), bits([voxels[x] for x in want])), (name, s)


def test_hand_built_streams_against_octomap():
    for name in (str(n) for n in FX["hand_built"]):
        p = oc.parse(bytes(FX[f"hand_{name}"]))
        assert p.status == oc.OK and p.size == int(FX[f"hand_{name}_num_nodes"]), name
        ck, cd = oc.centre_leaves(p)
        assert np.array_equal(ck, FX[f"hand_{name}_leaf_key"]) and np.array_equal(cd, FX[f"hand_{name}_leaf_depth"]), name
        assert np.array_equal(oc.leaf_arrays(p)[2], bits(FX[f"hand_{name}_leaf_value"])), name
    a, b = oc.parse(bytes(FX["hand_inner_right"])), oc.parse(bytes(FX["hand_inner_wrong"]))
    assert a.leaves == b.leaves and bytes(FX["hand_inner_right"]) != bytes(FX["hand_inner_wrong"])      # inner values are not kept
    k, v = oc.expand(a)
    assert oc.write(dict(zip(k.tolist(), v)), 0.1) == bytes(FX["hand_inner_right"])


def test_resume_records():
    """octomap's own leaves after read() of the stream of scan k and the remaining scans: those of the uninterrupted run, which
    the rays fixture holds, and what the transcription gives from the parsed stream"""
    for name, k in ((t.split(":")[0], int(t.split(":")[1])) for t in (str(x) for x in FX["resume"])):
        last = dict(list(scan_voxels(name))[-1][1])
        codes = [rc.morton(int(key)) >> (3 * (16 - int(d))) << (3 * (16 - int(d))) for key, d in
                 zip(FX[f"{name}_resume_key"], FX[f"{name}_resume_depth"])]
        gk, gv = oc.expand_leaves(codes, FX[f"{name}_resume_depth"], FX[f"{name}_resume_value"])
        want = sorted(last)
        assert gk.tolist() == want and np.array_equal(bits(gv), bits([last[x] for x in want])), name
        p = oc.parse(bytes(FX[f"{name}_ot_{k}"]), 0.1)
        ek, ev = oc.expand(p)
        params = [float(v) for v in RAYS[f"{name}_params"]]
        tree = rc.Tree(rc.RayParams(*params[:5], max_range=params[5]), 0.1)
        tree.v = dict(zip(ek.tolist(), (rc.F(x) for x in ev)))
        n = RAYS[f"{name}_npoints"]
        ends = np.cumsum(n)
        for s in range(k + 1, len(n)):
            tree.insert(RAYS[f"{name}_points"][ends[s] - n[s]:ends[s]], RAYS[f"{name}_origins"][s])
        tk, tv = tree.leaves()
        assert tk.tolist() == want and np.array_equal(bits(tv), bits([last[x] for x in want])), name


def device_parse(data):
    """The device parse of include/sbm.h on the body of a well-formed header: D by a scan, the parent as the previous
    smaller-or-equal D, the child index from mask[parent] -> (status, leaves)"""
    body = data[data.index(b"data\n") + 5:]
    n = oc.parse(data).size
    mask = [body[5 * i + 4] for i in range(n)]
    c = [bin(m).count("1") for m in mask]
    D = [1]
    for i in range(n):
        D.append(D[-1] + c[i] - 1)
    if any(d < 1 for d in D[:n]) or D[n] != 0:
        return oc.SIZE, []
    leaves = []
    for i in range(n):
        if c[i]:
            continue
        cur, code, depth = i, 0, 0
        while cur:
            if depth == 16:
                return oc.SIZE, []
            p = max(j for j in range(cur) if D[j] <= D[cur])
            r = D[p] + c[p] - 1 - D[cur]
            assert 0 <= r < c[p]
            code |= [b for b in range(8) if mask[p] >> b & 1][r] << (3 * depth)
            cur, depth = p, depth + 1
        leaves.append((code << (3 * (16 - depth)), depth, int.from_bytes(body[5 * i:5 * i + 4], "little")))
    return oc.OK, leaves


def test_parse_of_write_is_the_identity_and_the_device_formulas_agree():
    rng = np.random.default_rng(20)
    for t in range(300):
        tree = oc.random_tree(rng, p_child=0.22 + 0.01 * (t % 10), max_depth=4 + t % 5)
        data = oc.of_records(tree)
        p = oc.parse(data)
        assert p.status == oc.OK and p.size == oc.count(tree)
        st, leaves = device_parse(data)
        assert st == oc.OK and leaves == p.leaves, t
        if p.voxels <= 4096:                  # what a map would hold, written again: the same leaves (prune may merge none here:
            k, v = oc.expand(p)               # random values differ), so the second stream parses to the same voxels
            again = oc.parse(oc.write(dict(zip(k.tolist(), v)), 0.1))
            k2, v2 = oc.expand(again)
            assert np.array_equal(k, k2) and np.array_equal(bits(v), bits(v2)), t
    for name in ("chain16", "outside_clamps", "inner_wrong"):
        data = bytes(FX[f"hand_{name}"])
        assert device_parse(data) == (oc.OK, oc.parse(data).leaves), name
    for name in ("depth17", "complete_early", "size_minus_one", "size_plus_one"):
        data = bytes(FX[f"bad_{name}"])
        assert device_parse(data)[0] == oc.parse(data).status == oc.SIZE, name
    codes = np.unique(rng.integers(0, 1 << 48, 300, dtype=np.uint64))          # the numpy builder against the recursive one
    values = rng.normal(size=len(codes)).astype(np.float32)
    from occupancy_load_cases import _unmorton_array
    assert oc.unpruned(codes, values) == oc.of_records(oc.of_voxels(dict(zip(_unmorton_array(codes).tolist(), values))))
    comb = oc.of_records(oc.comb(40))
    assert device_parse(comb) == (oc.OK, oc.parse(comb).leaves)
