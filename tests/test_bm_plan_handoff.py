"""The interior SAD kernel's row-segment plan where later segments take their vertical sums over (fast_linked_plan,
csrc/sbm_sad_fast.hip), through the plan query of tests/test_bm_plan.py; no device.

SBM_FAST_HANDOFF=0 and =2 keep the plan every segment primes with: its segment counts and rows for five shapes are recorded here
(the values before the linked plan existed). In the default mode a launch whose dispatch order has a stride D below its segment count
gets lengths BY DISPATCH POSITION that rise over the first round (positions 0 .. D-2), then fall to the last position, and
hand-off scratch for the linked segments only (sbm_debug_handoff_bytes)."""
import ctypes

import pytest

import test_bm_plan as plan

CAP = 1 << 30          # kHandoffMaxBytes
# name -> (W, H, pairs, nd, w), the plan of SBM_FAST_HANDOFF=0: (nseg, segrow), and whether the default mode links segments
SHAPES = {
    "kitti_x64": ((1242, 375, 64, 128, 15), (8, [7, 63, 118, 174, 229, 285, 326, 354, 368]), True),
    "ref640_x64": ((640, 480, 64, 64, 21), (12, [10, 54, 98, 141, 185, 229, 273, 317, 360, 404, 437, 459, 470]), True),
    "kitti_nd64_x64": ((1242, 375, 64, 64, 15), (9, [7, 55, 103, 151, 200, 248, 296, 332, 356, 368]), True),
    "kitti_x1": ((1242, 375, 1, 128, 15),
                 (45, [7, 15, 24, 32, 40, 48, 57, 65, 73, 82, 90, 98, 107, 115, 123, 131, 140, 148, 156, 165, 173, 181, 190, 198, 206, 214,
                       223, 231, 239, 248, 256, 264, 273, 281, 289, 297, 306, 314, 322, 331, 339, 347, 356, 362, 366, 368]), False),
    "kitti_x8": ((1242, 375, 8, 128, 15),
                 (33, [7, 18, 30, 41, 53, 64, 76, 87, 99, 110, 122, 133, 145, 156, 167, 179, 190, 202, 213, 225, 236, 248, 259, 271, 282,
                       294, 305, 316, 328, 339, 351, 359, 365, 368]), True),
}


def case(W, H, n, nd, w):
    return dict(W=W, H=H, n=n, nd=nd, w=w, mind=0, roi=None, inplace=1, env={}, cap=31, uniq=10, tex=10, d12=1, spk_win=50, spk_range=32)


def query(pkg, monkeypatch, mode, c):
    """The plan and (hand-off bytes, flag bytes) of a case under SBM_FAST_HANDOFF=mode."""
    monkeypatch.setenv("SBM_FAST_HANDOFF", str(mode))
    st, pl = plan.query(pkg, c)
    assert st == plan.OK and pl.fast
    fn = pkg.load_library().sbm_debug_handoff_bytes
    fn.restype = ctypes.c_int
    fn.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_uint64)]
    out = (ctypes.c_uint64 * 2)()
    assert fn(ctypes.byref(plan.make_params(pkg, c)), c["n"], c["W"], c["H"], 1, out) == plan.OK
    return pl, int(out[0]), int(out[1])


def order(nseg, per_seg, nd):
    """fast_segment_order: (stride D, segment at each dispatch position)."""
    slots = 4096 if nd <= 64 else 3072
    D = plan.cdiv(slots, per_seg) + 1
    if D >= nseg:
        return nseg, list(range(nseg))
    at, base = [0] * nseg, 0
    for r in range(D):
        for p in range(r, nseg, D):
            at[p] = base
            base += 1
    return D, at


def scratch(linked_sets, per_seg, nd):
    slots = linked_sets * per_seg
    flags = (2 * slots * 4 + 255) & ~255
    return flags + slots * (nd // 4 * 512 + 256), flags


@pytest.mark.parametrize("mode", [0, 2])
@pytest.mark.parametrize("name", list(SHAPES))
def test_priming_and_separate_launches_keep_their_plan(pkg, monkeypatch, name, mode):
    dims, (nseg, segrow), _ = SHAPES[name]
    pl, nbytes, flags = query(pkg, monkeypatch, mode, case(*dims))
    assert (pl.f.nseg, list(pl.f.segrow[:nseg + 1])) == (nseg, segrow)
    plan.check_plan(case(*dims), pl)
    lone = pl.f.NWAVES == 1 and bool(pl.f.exact)
    if mode == 0 or not lone:
        assert (nbytes, flags) == (0, 0)
    else:                                                  # every later segment is linked and holds a slot
        assert (nbytes, flags) == scratch(nseg - 1, dims[2] * pl.f.strips, dims[3]) and nbytes <= CAP


@pytest.mark.parametrize("name", list(SHAPES))
def test_linked_plan(pkg, monkeypatch, name):
    dims, (nseg0, segrow0), linked = SHAPES[name]
    W, H, n, nd, w = dims
    pl, nbytes, flags = query(pkg, monkeypatch, 1, case(*dims))
    plan.check_plan(case(*dims), pl)                       # the fixed points: count, rising rows, grid, split
    f = pl.f
    per_seg = n * f.strips
    D, at = order(f.nseg, per_seg, nd)
    if not linked:                                         # one pair: cooperating wavefronts, nothing is linked, nothing changes
        assert D >= f.nseg or f.NWAVES > 1
        assert (f.nseg, list(f.segrow[:f.nseg + 1])) == (nseg0, segrow0) and (nbytes, flags) == (0, 0)
        return
    assert f.NWAVES == 1 and f.exact and D < f.nseg and f.nseg >= nseg0
    rows = [f.segrow[k + 1] - f.segrow[k] for k in range(f.nseg)]
    assert min(rows) > 0 and sum(rows) == pl.g.row1 - pl.g.row0
    by_pos = [rows[at[p]] for p in range(f.nseg)]
    print(name, "stride", D, "rows by dispatch position", by_pos)
    # every position at or above the stride holds a segment, and those are the linked ones
    takers = sorted(at[p] for p in range(D, f.nseg))
    assert len(set(takers)) == f.nseg - D and takers[0] >= 1
    first = by_pos[:D - 1]
    assert all(a <= b for a, b in zip(first, first[1:])), first
    assert by_pos[-1] == min(by_pos), by_pos
    assert (nbytes, flags) == scratch(f.nseg - D, per_seg, nd)
    assert 0 < nbytes <= CAP


def test_the_cap_limits_the_count(pkg, monkeypatch):
    """64 pairs of 8192 x 2160 at 128 disparities: a set of slots is 140 MB, and the linked plan takes only as many segments as fit the
    cap (never fewer than the priming plan's)."""
    c = case(8192, 2160, 64, 128, 15)
    pl0, _, _ = query(pkg, monkeypatch, 0, c)
    pl, nbytes, flags = query(pkg, monkeypatch, 1, c)
    per_seg = 64 * pl.f.strips
    D, _ = order(pl.f.nseg, per_seg, 128)
    assert D < pl.f.nseg and pl.f.nseg >= pl0.f.nseg
    assert (nbytes, flags) == scratch(pl.f.nseg - D, per_seg, 128) and 0 < nbytes <= CAP
    assert scratch(pl.f.nseg - D + 1, per_seg, 128)[0] > CAP or pl.f.nseg == pl0.f.nseg or pl.f.nseg == 64
