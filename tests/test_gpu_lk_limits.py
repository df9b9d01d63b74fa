"""GPU LK stereo (u96-slam_amd/csrc/sbm_lk.hip) on the host and launch paths that tests/test_gpu_lk.py does not reach, exact
against the sequential C restatement (oracle/lk_stereo_ref): a batch one pair longer than a scratch chunk (both scratch layouts),
frames that keep the deepest level the engine holds and max_level beyond it, the documented limit of 65 535 pairs per call, counts
above cap -- and the device against the reference's own tracker (oracle/_ref/liblk_reference.so) without the restatement between.
Floats are compared as uint32; no mismatch is allowed."""
import pathlib
import sys

import numpy as np
import pytest

ROOT = pathlib.Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "tests"))
import lk_reference  # noqa: E402
import lk_stereo_ref as ref  # noqa: E402
from gpu_support import bm, dev  # noqa: E402,F401
from lk_cases import (DEEP_SIZES, bits, bound_points, deep_pair, edge_points, grid_points, noise_frame, small_pair,  # noqa: E402
                      small_points)

pytestmark = pytest.mark.gpu
CHUNK_BYTES = 256 << 20          # include/sbm.h: "a call works through its pairs in chunks of at most 256 MiB" of scratch
RP0, ST0, ER0 = -7.25, 77, -3.5  # what the outputs hold before the call


def gpu_params(pkg, p):
    return pkg.lk_params(p.win_width, p.win_height, p.max_level, p.max_count, p.epsilon, p.flags, p.min_eig_threshold,
                         p.min_disparity, p.max_disparity)


def chunk_pairs(w, h, p):
    """Pairs per chunk by the documented rule: per pair, 1 B per pixel of the levels above 0 of both images and 4 B per pixel of
    every left level."""
    sizes = ref.level_sizes(w, h, p)
    every = sum(a * b for a, b in sizes)
    per_pair = 2 * (every - w * h) + 4 * every
    return CHUNK_BYTES // per_pair, per_pair


def run_batch(bm, pkg, lefts, rights, kpts, counts, p):
    """(n, H, W) pairs, (n, cap, 2) points, n counts -> numpy (right_pts, status, err), preset to the sentinels."""
    import torch

    n, cap = kpts.shape[:2]
    rp = torch.full((n, cap, 2), RP0, dtype=torch.float32, device="cuda:0")
    st = torch.full((n, cap), ST0, dtype=torch.uint8, device="cuda:0")
    er = torch.full((n, cap), ER0, dtype=torch.float32, device="cuda:0")
    bm.lk_stereo(dev(lefts), dev(rights), dev(kpts), dev(np.asarray(counts, np.int32)), gpu_params(pkg, p), right_pts=rp, status=st, err=er)
    return rp.cpu().numpy(), st.cpu().numpy(), er.cpu().numpy()


def check_chunked(bm, pkg, distinct, w, h, p, grid, what):
    """chunk + 1 pairs cycling through `distinct`; slot i tracks its own 8-point slice of grid, count i % 9, cap 8."""
    chunk, per_pair = chunk_pairs(w, h, p)
    n, cap = chunk + 1, 8
    assert 1 <= chunk < n, (chunk, per_pair)
    want = [ref.correspondences(l, r, grid, p) for l, r in distinct]          # points share nothing: a slice of it is the slot's answer
    which = np.arange(n) % len(distinct)
    start = (8 * np.arange(n)) % (len(grid) - cap)
    counts = np.arange(n) % (cap + 1)
    assert len({(int(a), int(b)) for a, b in zip(which, start)}) == n and chunk % len(distinct) != 0
    kpts = np.stack([grid[s:s + cap] for s in start]).astype(np.float32)
    lefts = np.stack([distinct[k][0] for k in which])
    rights = np.stack([distinct[k][1] for k in which])
    rp, st, er = run_batch(bm, pkg, lefts, rights, kpts, counts, p)
    bad = []
    for i in range(n):
        k, s, d = int(counts[i]), int(start[i]), int(which[i])
        wo, ws, we = (a[s:s + k] for a in want[d])
        ok = np.array_equal(bits(rp[i, :k]), bits(wo)) and np.array_equal(st[i, :k], ws) and np.array_equal(bits(er[i, :k]), bits(we))
        ok = ok and (rp[i, k:] == RP0).all() and (st[i, k:] == ST0).all() and (er[i, k:] == ER0).all()
        if not ok:
            bad.append(i)
    named = {"last of chunk 0": chunk - 1, "first of chunk 1": chunk, "last": n - 1}
    assert not bad, (what, f"{len(bad)} of {n} pairs differ (chunk = {chunk} pairs of {per_pair} B)", bad[:12],
                     {k: ("differs" if v in bad else "equal") for k, v in named.items()})
    assert st[counts[:, None] > np.arange(cap)[None]].sum() >= 20          # something was tracked


def test_chunk_boundary_with_upper_levels(bm, pkg, golden):
    """640 x 480 at the default five levels: 1 842 600 B of scratch per pair, 145 pairs per chunk, 146 pairs."""
    L, R = golden["rect_l"], golden["rect_r"]
    p = ref.params()
    assert chunk_pairs(640, 480, p) == (145, 1842600)
    check_chunked(bm, pkg, [(L, R), (R, L), (noise_frame(640, 480, 31), noise_frame(640, 480, 32))], 640, 480, p, grid_points(), "640x480")


def test_chunk_boundary_level_0_only(bm, pkg):
    """1024 x 1024 with max_level 0: no pyramid scratch, 4 MiB of derivatives per pair, 64 pairs per chunk, 65 pairs."""
    p = ref.params(max_level=0, max_disparity=-1.0)
    assert chunk_pairs(1024, 1024, p) == (64, 4 << 20)
    a, b = deep_pair(1024, 1024, 5)
    c, d = noise_frame(1024, 1024, 41), noise_frame(1024, 1024, 42)
    grid = (grid_points() * np.array([1.6, 2.1], np.float32)).astype(np.float32)
    check_chunked(bm, pkg, [(a, b), (b, a), (c, d)], 1024, 1024, p, grid, "1024x1024 level 0")


@pytest.mark.parametrize("w,h,last", DEEP_SIZES)
def test_deep_pyramids(bm, pkg, w, h, last):
    """max_level 7, 9 and 100 on 2048 and 2047 columns: the count rule ends 40 and 33 rows at level 3 and keeps level 7, the
    engine's last, for 512 and 385 rows; a max_level above 7 changes nothing."""
    left, right = deep_pair(w, h)
    pts = np.concatenate([edge_points(w, h, last), bound_points(w, h, last)])
    for max_level in (7, 9, 100):
        p = ref.params(max_level=max_level, max_disparity=-1.0)
        sizes = ref.level_sizes(w, h, p)
        assert len(sizes) - 1 == last and (last != 7 or sizes[-1] == (16, 4))
        lv, dv = bm.lk_pyramid(dev(np.stack([left, right])), gpu_params(pkg, p))
        assert len(lv) == len(dv) == last + 1 and tuple(lv[-1].shape) == (2, sizes[-1][1], sizes[-1][0])
        for i, im in enumerate((left, right)):
            wl, wd = ref.pyramid(im, p)
            for k in range(last + 1):
                assert np.array_equal(lv[k][i].cpu().numpy(), wl[k]), (max_level, i, k, "level")
                assert np.array_equal(dv[k][i].cpu().numpy(), wd[k]), (max_level, i, k, "deriv")
        rp, st, er = run_batch(bm, pkg, left[None], right[None], pts[None], [len(pts)], p)
        wo, ws, we = ref.correspondences(left, right, pts, p)
        assert np.array_equal(bits(rp[0]), bits(wo)) and np.array_equal(st[0], ws) and np.array_equal(bits(er[0]), bits(we)), max_level
        assert ws.any() and not ws.all()


def test_deepest_square_frame_every_plane(bm, pkg):
    img = deep_pair(2048, 2048, 3)[0]
    p = ref.params(max_level=9)
    lv, dv = bm.lk_pyramid(dev(img), gpu_params(pkg, p))
    wl, wd = ref.pyramid(img, p)
    assert len(lv) == len(wl) == 8 and tuple(lv[7].shape) == (1, 16, 16)
    for k in range(8):
        assert np.array_equal(lv[k][0].cpu().numpy(), wl[k]), (k, "level")
        assert np.array_equal(dv[k][0].cpu().numpy(), wd[k]), (k, "deriv")


@pytest.fixture(scope="module")
def tiny():
    """Five distinct 32 x 8 pairs (level 1 is 16 x 4) x seven points, one point per pair: the restatement's answer per combination."""
    p = ref.params(min_eig_threshold=1e-7, max_disparity=-1.0)
    pairs = [small_pair(32, 8), small_pair(32, 8)[::-1], (noise_frame(32, 8, 1), noise_frame(32, 8, 2)),
             (noise_frame(32, 8, 3), noise_frame(32, 8, 3)), deep_pair(32, 8, 2)]
    pts = np.array([(16.0, 4.0), (3.25, 1.5), (28.5, 6.75), (0.0, 0.0), (31.0, 7.0), (40.0, 3.0), (12.125, 3.0)], np.float32)
    assert ref.level_sizes(32, 8, p) == [(32, 8), (16, 4)]
    out = np.zeros((5, 7, 2), np.float32)
    st = np.zeros((5, 7), np.uint8)
    err = np.zeros((5, 7), np.float32)
    for k, (l, r) in enumerate(pairs):
        out[k], st[k], err[k] = ref.correspondences(l, r, pts, p)
    assert st.any() and not st.all()
    return {"p": p, "L": np.stack([a for a, _ in pairs]), "R": np.stack([b for _, b in pairs]), "pts": pts, "out": out, "st": st, "err": err}


@pytest.mark.parametrize("n", [32767, 32768, 65535])
def test_pair_count_up_to_the_documented_limit(bm, pkg, tiny, n):
    """One pyrDown launch takes both images of every pair of a chunk: above 32 767 pairs a call has to split even where the
    scratch would hold them all."""
    t = tiny
    i = np.arange(n)
    k, q = i % 5, (i // 5) % 7
    rp, st, er = run_batch(bm, pkg, t["L"][k], t["R"][k], t["pts"][q][:, None, :], np.ones(n, np.int32), t["p"])
    bad = (bits(rp[:, 0]) != bits(t["out"][k, q])).any(axis=1) | (st[:, 0] != t["st"][k, q]) | (bits(er[:, 0]) != bits(t["err"][k, q]))
    assert not bad.any(), (n, int(bad.sum()), "pairs differ; first", np.nonzero(bad)[0][:8], "last", np.nonzero(bad)[0][-1])
    if n == 65535:
        lv, dv = bm.lk_pyramid(dev(t["L"][k]), gpu_params(pkg, t["p"]))
        w1 = np.stack([ref.pyramid(a, t["p"])[0][1] for a in t["L"]])
        d1 = np.stack([ref.pyramid(a, t["p"])[1][1] for a in t["L"]])
        assert np.array_equal(lv[1].cpu().numpy(), w1[k]) and np.array_equal(dv[1].cpu().numpy(), d1[k])


def test_pair_count_above_the_limit_is_refused(bm, pkg, tiny):
    t = tiny
    n = 65536
    k = np.arange(n) % 5
    with pytest.raises(pkg.StereoBMError) as e:
        run_batch(bm, pkg, t["L"][k], t["R"][k], t["pts"][k % 7][:, None, :], np.ones(n, np.int32), t["p"])
    assert e.value.code == -23          # SBM_ERR_UNSUPPORTED


def test_count_above_cap_reads_as_cap(bm, pkg, golden):
    L, R = golden["rect_l"], golden["rect_r"]
    cap = 8
    grid = grid_points()
    kpts = np.stack([grid[100:108], grid[200:208], grid[300:308]])
    counts = [cap + 1, 2 ** 31 - 1, 3]
    p = ref.params()
    rp, st, er = run_batch(bm, pkg, np.stack([L, R, L]), np.stack([R, L, R]), kpts, counts, p)
    for i, (l, r) in enumerate(((L, R), (R, L), (L, R))):
        k = min(counts[i], cap)
        wo, ws, we = ref.correspondences(l, r, kpts[i, :k], p)
        assert np.array_equal(bits(rp[i, :k]), bits(wo)) and np.array_equal(st[i, :k], ws) and np.array_equal(bits(er[i, :k]), bits(we)), i
        assert (rp[i, k:] == RP0).all() and (st[i, k:] == ST0).all() and (er[i, k:] == ER0).all(), i


@pytest.fixture(scope="module")
def reference():
    """oracle/_ref/liblk_reference.so as it was built where the reference tree is; this module never reads that tree."""
    ok, why = lk_reference.available()
    if not ok:
        pytest.skip(why)
    lk_reference.lib()
    return lk_reference


def against_reference(bm, pkg, reference, left, right, pts, p, what):
    rp, st, er = run_batch(bm, pkg, left[None], right[None], pts[None], [len(pts)], p)
    wo, ws, we = reference.track(left, right, pts, p)
    bad = (bits(rp[0]) != bits(wo)).any(axis=1) | (st[0] != ws) | (bits(er[0]) != bits(we))
    assert not bad.any(), (what, int(bad.sum()), "points differ; first", np.nonzero(bad)[0][:8])
    return ws


def test_device_against_the_reference_build_golden_grid(bm, pkg, reference, golden):
    ws = against_reference(bm, pkg, reference, golden["rect_l"], golden["rect_r"], grid_points(), ref.params(max_disparity=-1.0), "golden")
    assert ws.sum() >= 100 and (ws == 0).sum() >= 100


@pytest.mark.parametrize("w,h", [(16, 4), (37, 11)])
def test_device_against_the_reference_build_small_frames(bm, pkg, reference, w, h):
    left, right = small_pair(w, h)
    pts = small_points(w, h)
    for thr in (1e-4, 1e-7):
        ws = against_reference(bm, pkg, reference, left, right, pts, ref.params(min_eig_threshold=thr, max_disparity=-1.0), (w, h, thr))
    assert ws.any() and not ws.all()
    against_reference(bm, pkg, reference, noise_frame(w, h, 5), noise_frame(w, h, 6), pts,
                      ref.params(min_eig_threshold=0.0, max_disparity=-1.0), "noise")
