"""The FPGA-flavour matcher's launch plan (FpgaPlan, csrc/sbm_fpga.hip), queried through sbm_fpga_debug_plan without a device and
held to the invariants its launches rely on, over the whole envelope of sbm_fpga_params_validate. Properties only: no recorded
table of tuning outputs, so a retune that keeps the invariants keeps this file green. Also the validation itself against the
oracle's (oracle.fpga_check) over the same grid, invalid windows and disparity counts included."""
import ctypes

import pytest

WINDOWS = list(range(3, 32, 2))
NDS = list(range(32, 257, 32))
PAIRS = [1, 3, 64, 65535]


def sizes(wsz, nd):
    """(W, H) of a spread of frames for one window and range: the smallest legal frame, one sample more each way, the strip
    boundaries of the first strips, a few ordinary frames, the largest frame."""
    hw = wsz // 2
    w0, h0 = nd + 1 + 2 * hw + 1, 2 * hw + 1                 # sad_wdt = sad_hgt = 1
    nv = 64 - 2 * hw
    ws = {w0, w0 + 1, w0 + nv - 2, w0 + nv - 1, w0 + nv, w0 + 2 * nv - 1, w0 + 2 * nv, nd + 200, 640, 1000, 1023}
    hs = {h0, h0 + 1, h0 + 2 * wsz - 1, h0 + 4 * wsz - 2, h0 + 4 * wsz - 1, h0 + 4 * wsz, 45, 150, 240, 480, 511}
    return sorted(w for w in ws if w0 <= w <= 1023), sorted(h for h in hs if h0 <= h <= 511)


def test_plan_invariants_over_the_envelope(pkg):
    seen_groups, cases = set(), 0
    for wsz in WINDOWS:
        hw = wsz // 2
        for nd in NDS:
            if pkg.fpga_validate(pkg.fpga_params(1023, 511, wsz, nd)) != 0:
                continue
            ws, hs = sizes(wsz, nd)
            for W in ws:
                for H in hs:
                    for n in PAIRS:
                        for uni in (0, 1):
                            p = pkg.fpga_params(W, H, wsz, nd, uni, 0, 0x200)
                            assert pkg.fpga_validate(p) == 0, (W, H, wsz, nd)
                            pl = pkg.fpga_plan(p, n)
                            where = (W, H, wsz, nd, n, uni)
                            cases += 1
                            # geometry (bm.v:249-255)
                            assert (pl.hwsz, pl.hsad_wdt, pl.sad_wdt, pl.sad_hgt) == (hw, W - nd - 1, W - nd - 1 - 2 * hw, H - 2 * hw), where
                            # launches: groups of 1, 2 or 4 consecutive phases that cover the range once, in order
                            groups = pl.groups
                            assert 1 <= pl.nlaunch <= 8 and set(groups) <= {1, 2, 4} and sum(groups) == nd // 32 == pl.nphase, where
                            assert [pl.launch[i].phase0 for i in range(pl.nlaunch)] == [sum(groups[:i]) for i in range(pl.nlaunch)], where
                            seen_groups.add(tuple(groups))
                            # lean: exactly one launch and the filter off
                            for i in range(pl.nlaunch):
                                assert pl.launch[i].lean == int(pl.nlaunch == 1 and not uni), where
                            # strips cover the samples, none is empty; lanes 0 .. 63 + 2 hwsz of a prefix row fit its LDS row
                            assert pl.nv == 64 - 2 * hw and pl.nv >= 1, where
                            assert pl.strips * pl.nv >= pl.sad_wdt > (pl.strips - 1) * pl.nv, where
                            assert 1 + 63 + 2 * hw < pl.xs, where
                            assert pl.lds >= (18 * pl.xs + 2 * 256) * 4 and pl.lds <= 65536, where
                            # segments cover the rows, none is empty, and every one of them earns its wsz - 1 priming rows
                            assert pl.nseg >= 1 and pl.seg >= 1 and 1 <= pl.grid_y <= pl.nseg, where
                            assert pl.seg * pl.grid_y >= pl.sad_hgt > pl.seg * (pl.grid_y - 1), where
                            if pl.nseg > 1:
                                assert pl.seg >= 2 * wsz, where
                            # saturation: the flag is tracked exactly when a column sum can pass the limiter, the exact pass
                            # exists exactly when segments could then be wrong
                            assert pl.track_sat == int(wsz * 63 > 1023), where
                            assert pl.exact == int(pl.track_sat and pl.nseg > 1), where
                            # the grid HIP accepts
                            assert pl.strips <= 65535 and pl.grid_y <= 65535, where
    assert cases > 50000
    assert seen_groups == {(1,), (2,), (2, 1), (4,), (4, 1), (4, 2), (4, 2, 1), (4, 4)}


def test_plan_does_not_depend_on_the_filter_beyond_lean_or_on_mode_and_threshold(pkg):
    for wsz, nd, W, H, n in ((5, 96, 300, 200, 2), (21, 128, 640, 480, 1), (31, 256, 1023, 511, 3)):
        ref = pkg.fpga_plan(pkg.fpga_params(W, H, wsz, nd, 1, 0, 0), n)
        for uni in ((0, 0, 0), (1, 1, 0x3ff), (0, 1, 5)):
            pl = pkg.fpga_plan(pkg.fpga_params(W, H, wsz, nd, *uni), n)
            for k, _ in pl._fields_[:-1]:
                assert getattr(pl, k) == getattr(ref, k), (k, uni)
            assert pl.groups == ref.groups


def test_more_pairs_never_mean_more_segments(pkg):
    """The segment count only serves to fill the chip: it falls (weakly) with the batch, down to one."""
    for wsz, nd, W, H in ((5, 96, 163, 200), (21, 64, 260, 150), (3, 32, 1023, 511), (31, 256, 1023, 511)):
        last = None
        for n in (1, 2, 4, 16, 64, 256, 1024, 4096, 65535):
            pl = pkg.fpga_plan(pkg.fpga_params(W, H, wsz, nd), n)
            assert last is None or pl.nseg <= last
            last = pl.nseg
        assert last == 1


def test_export_status_codes(pkg):
    from u96_slam_amd import stereobm

    L = pkg.load_library()
    p = pkg.fpga_params(640, 480, 21, 64)
    pl = stereobm.FpgaPlan()
    size = ctypes.sizeof(pl)
    assert size == 4 * (15 + 3 * 8)
    for bad in (size - 4, size + 4, 0):
        assert L.sbm_fpga_debug_plan(ctypes.byref(p), 1, ctypes.byref(pl), bad) == -2
    assert L.sbm_fpga_debug_plan(None, 1, ctypes.byref(pl), size) == -1
    assert L.sbm_fpga_debug_plan(ctypes.byref(p), 1, None, size) == -1
    assert L.sbm_fpga_debug_plan(ctypes.byref(p), 0, ctypes.byref(pl), size) == -24
    assert L.sbm_fpga_debug_plan(ctypes.byref(p), 65536, ctypes.byref(pl), size) == -23
    assert L.sbm_fpga_debug_plan(ctypes.byref(p), 65535, ctypes.byref(pl), size) == 0
    for kw, code in ((dict(block_size=20), -6), (dict(num_disparities=48), -7), (dict(width=1024), -2), (dict(height=42), 0),
                     (dict(height=20), -2), (dict(width=64 + 1 + 20), -2), (dict(width=64 + 1 + 20 + 1), 0)):
        q = pkg.fpga_params(**{**dict(width=640, height=480, block_size=21, num_disparities=64), **kw})
        assert L.sbm_fpga_debug_plan(ctypes.byref(q), 1, ctypes.byref(pl), size) == code, kw
    with pytest.raises(pkg.StereoBMError) as e:
        pkg.fpga_plan(pkg.fpga_params(640, 480, 22, 64))
    assert e.value.code == -6


def test_validate_equals_the_oracle_check_and_never_refuses_a_legal_geometry(pkg, oracle):
    """sbm_fpga_params_validate against oracle.fpga_check over the grid of the plan test, with even and out-of-range windows,
    disparity counts that are no multiple of 32 or out of range, and frames one sample too small or too large. Status -23
    (bm_obuf2.v:239 would never leave state 6: (nd + hwsz + 1) & 31 == 0) cannot occur: nd & 31 == 0 and 2 <= hwsz + 1 <= 16.
    The check stays in both as a guard of that arithmetic."""
    codes = {}
    for wsz in [0, 1, 2] + list(range(3, 34)) + [63]:
        for nd in [0, 16, 31] + NDS + [33, 48, 255, 257, 288, 512]:
            hw = max(wsz, 0) // 2
            w0, h0 = nd + 1 + 2 * hw + 1, 2 * hw + 1
            for W in (0, 1, w0 - 1, w0, w0 + 1, 640, 1023, 1024):
                for H in (0, 1, h0 - 1, h0, h0 + 1, 480, 511, 512):
                    got = pkg.fpga_validate(pkg.fpga_params(W, H, wsz, nd))
                    ref = oracle.fpga_check(W, H, wsz, nd)
                    assert got == ref, (W, H, wsz, nd, got, ref)
                    assert got != -23, (W, H, wsz, nd)
                    codes[got] = codes.get(got, 0) + 1
    assert set(codes) == {0, -2, -6, -7} and min(codes.values()) > 100
    for wsz in WINDOWS:
        for nd in NDS:
            assert (nd + wsz // 2 + 1) & 31
