"""The small HIP kernels in front of and behind the matcher -- decimate, reproject, keypoints3d, to_float (sbm_consume.hip,
sbm_consume_math.h), rect_map, rect_remap (sbm_rectify.hip), gftt_eig (sbm_gftt.hip) -- against the restatements of
tests/frontend_cases.py, on the inputs that tests/test_frontend_cases_restatement.py holds to the C oracle on the CPU.
Tolerance 0 everywhere: the float outputs are compared as uint32 with NaN at the same places (the kernels keep the reference's
type per operation and never contract a multiply-add), the integer outputs are equal. A failure prints the first differing
indices and the disparity, keypoint or pixel behind them."""
import ctypes

import numpy as np
import pytest

import frontend_cases as fc
from gpu_support import bm, dev, torch_cuda  # noqa: F401

pytestmark = pytest.mark.gpu

MODELS = fc.models()
PLANES = fc.disparity_planes()


def gmodel(pkg, m):
    return fc.fill_model(pkg.StereoModel(), m)


def assert_same(got, ref, what, behind=None):
    if not fc.same_floats(got, ref):
        d = fc.first_diffs(got, ref)
        lines = [f"{i}: got {np.asarray(got)[i]!r} expected {np.asarray(ref)[i]!r}" + (f" <- {behind(i)}" if behind else "") for i in d]
        pytest.fail(f"{what}: first differences\n  " + "\n  ".join(lines))


def assert_equal(got, ref, what, behind=None):
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    if not np.array_equal(got, ref):
        d = [tuple(int(v) for v in i) for i in np.argwhere(got != ref)[:5]]
        lines = [f"{i}: got {got[i]} expected {ref[i]}" + (f" <- {behind(i)}" if behind else "") for i in d]
        pytest.fail(f"{what}: {int((got != ref).sum())} differ, first\n  " + "\n  ".join(lines))


# ---------------------------------------------------------------------------------------------------------- consumers ---------
@pytest.mark.parametrize("name", list(MODELS))
def test_reproject_every_disparity(torch_cuda, pkg, bm, name):
    """Every int16 disparity under one camera model: scales 1, 4, 7, the local transform on and off, a batch of three planes
    (the batch index is blockIdx.y)."""
    m, g = MODELS[name], gmodel(pkg, MODELS[name])
    d = dev(PLANES)
    for scale in fc.REPROJECT_SCALES:
        for apply_local in ((True, False) if m["local"] is not None else (True,)):
            got = bm.reproject(d, g, scale=scale, apply_local=apply_local).cpu().numpy()
            for i in range(3):
                assert_same(got[i], fc.reproject(PLANES[i], scale, m, apply_local), f"{name} scale {scale} local {apply_local} plane {i}",
                            lambda j: f"disparity {int(PLANES[i][j[0], j[1]])} at column {j[1]} row {j[0]}")
    one = bm.reproject(d[1], g, scale=1).cpu().numpy()
    assert_same(one, fc.reproject(PLANES[1], 1, m), f"{name} single plane")


@pytest.mark.parametrize("name", list(MODELS))
def test_keypoints3d_edges_and_gates(torch_cuda, pkg, bm, name):
    """Keypoints on and beyond every edge, non-finite and huge ones, every gate pair, depth gates hit exactly; nk 1, 255, 256,
    257 through the mirror."""
    m, g = MODELS[name], gmodel(pkg, MODELS[name])
    kp, disp = fc.keypoints(), PLANES[0]
    d, k = dev(disp), dev(kp)
    for lo, hi in fc.depth_gates(disp, kp, m):
        got = bm.keypoints3d(d, k, g, lo, hi).cpu().numpy()
        assert_same(got, fc.keypoints3d(disp, kp, m, lo, hi), f"{name} gates ({lo!r}, {hi!r})", lambda j: f"keypoint {kp[j[0]].tolist()}")
    for nk in fc.KEYPOINT_COUNTS:
        if nk:
            got = bm.keypoints3d(d, k[:nk], g, 2.0, 30.0).cpu().numpy()
            assert_same(got, fc.keypoints3d(disp, kp[:nk], m, 2.0, 30.0), f"{name} nk {nk}", lambda j: f"keypoint {kp[j[0]].tolist()}")


def test_keypoints3d_zero_count_writes_nothing(torch_cuda, pkg, bm):
    """nk = 0 through the C ABI: status 0, the output buffer untouched (with and without pointers)."""
    torch = torch_cuda
    g = gmodel(pkg, MODELS["kitti"])
    d, k = dev(PLANES[0]), dev(fc.keypoints())
    out = torch.full((16, 3), 7.5, dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()
    assert bm._L.sbm_keypoints3d_device(bm._h, d.data_ptr(), fc.PW, fc.PH, k.data_ptr(), 0, ctypes.byref(g), 0.0, 0.0, out.data_ptr(), 1) == 0
    assert bm._L.sbm_keypoints3d_device(bm._h, d.data_ptr(), fc.PW, fc.PH, None, 0, ctypes.byref(g), 0.0, 0.0, None, 1) == 0
    assert (out.cpu().numpy() == 7.5).all()


@pytest.mark.parametrize("scale", fc.DECIMATE_SCALES)
def test_decimate_scales(torch_cuda, bm, scale):
    for planes in fc.decimate_planes():
        got = bm.decimate(dev(planes), scale).cpu().numpy()
        assert_equal(got, fc.decimate(planes, scale), f"scale {scale} of {planes.shape}")
    one = bm.decimate(dev(PLANES[2]), scale).cpu().numpy()
    assert_equal(one, fc.decimate(PLANES[2], scale), f"scale {scale}, single plane")


def test_decimate_scale_beyond_the_frame_writes_nothing(torch_cuda, bm):
    """A scale larger than the width or the height leaves no output pixel: status 0 and a marker-filled buffer untouched."""
    torch = torch_cuda
    planes = fc.decimate_planes()[0]                        # 3 x 37 x 53
    d = dev(planes)
    for scale in (38, 54, 1000):                            # > height only (53 // 38 == 1 column would remain), > both
        out = torch.full((3 * 37 * 53,), -12345, dtype=torch.int16, device="cuda:0")
        torch.cuda.synchronize()
        assert bm._L.sbm_decimate_device(bm._h, 3, d.data_ptr(), 53, 37, scale, out.data_ptr(), 1) == 0
        assert (out.cpu().numpy() == -12345).all(), scale
    wide = dev(np.ascontiguousarray(planes.transpose(0, 2, 1)))   # 3 x 53 x 37: a scale beyond the width only
    out = torch.full((3 * 37 * 53,), -12345, dtype=torch.int16, device="cuda:0")
    torch.cuda.synchronize()
    assert bm._L.sbm_decimate_device(bm._h, 3, wide.data_ptr(), 37, 53, 38, out.data_ptr(), 1) == 0
    assert (out.cpu().numpy() == -12345).all()


def test_to_float_every_value_and_the_tail(torch_cuda, bm):
    for d in fc.to_float_inputs():
        got = bm.to_float(dev(d)).cpu().numpy()
        assert got.dtype == np.float32
        assert_same(got, fc.to_float(d), f"{d.shape}", lambda j: f"value {int(d[j])}")


# ---------------------------------------------------------------------------------------------------------- rectifier ---------
@pytest.mark.parametrize("name", list(fc.rect_cams()))
def test_rect_map_calibrations(torch_cuda, pkg, bm, name):
    """lw negative (its conversion to unsigned), lw == 0 (the den == 0 branch), lw == -1, int32 extremes."""
    cam = fc.rect_cams()[name]
    ref, lw, over = fc.rect_map(cam)
    assert not over.any()
    got = bm.rect_map(pkg.make_rect_cam(**cam), fc.RW, fc.RH).cpu().numpy()
    assert_equal(got, ref, name, lambda j: f"pixel ({j[1]}, {j[0]}) lw {lw[j[0], j[1]]}")


@pytest.mark.parametrize("name", list(fc.remap_cases()))
def test_rect_remap_fast_path_boundary(torch_cuda, bm, name):
    src, maps = fc.remap_cases()[name]
    h, w = src.shape[-2:]
    s = dev(src)
    for k, m in enumerate(maps):
        got = bm.rect_remap(s, dev(m)).cpu().numpy()
        ref = fc.rect_remap(src, m)
        assert_equal(got, ref, f"{name} map {k}", lambda j: f"map entry {m[j[-2], j[-1]].tolist()} = (xi, yi) "
                     f"{(int(m[j[-2], j[-1], 0]) >> 5, int(m[j[-2], j[-1], 1]) >> 5)} of a {w} x {h} frame")
        if name.endswith("all255"):
            assert (got[fc.fully_inside(m, w, h)] == 255).all()


# ---------------------------------------------------------------------------------------------------------- GFTT --------------
def gftt_check(bm, frames, what, names=None):
    """frames (n, H, W) uint8 through the kernel; map and Max word of every frame against the restatement."""
    eig, mx = bm.gftt_eig(dev(frames))
    eig, mx = eig.cpu().numpy(), mx.cpu().numpy()
    for i, im in enumerate(frames):
        g = fc.gftt_eig(im)

        def behind(j, g=g):
            y, x = j
            if 2 <= y < im.shape[0] - 2:
                return "a %d c %d b %d s %d r %d" % tuple(int(g[k][y - 2, x]) for k in ("a", "c", "b", "s", "r"))
            return "border row"
        name = names[i] if names else f"frame {i}"
        assert_equal(eig[i], g["eig"].astype(np.int64), f"{what} {name}", behind)
        assert int(mx[i]) == g["max"], (what, name, int(mx[i]), g["max"])


@pytest.mark.parametrize("W,H", fc.GFTT_SIZES)
def test_gftt_structured_images(torch_cuda, bm, W, H):
    """Constants, ramps, steps, checkerboards, stripes, a dot, a quadrant, the two searched images: radicands of 0, below 1024,
    perfect squares, at the cap; a, c, b at their limiters; a negative a + c - r; output 65535 (the CPU test asserts that the
    set reaches each). 126, 127, 253, 254 columns put a strip boundary of the two-column kernel inside the structure."""
    imgs = fc.gftt_images(W, H)
    gftt_check(bm, np.stack(list(imgs.values())), f"{W} x {H}", list(imgs))


@pytest.mark.parametrize("W,H", fc.GFTT_NARROW)
def test_gftt_one_column_kernel_widths(torch_cuda, bm, W, H):
    """W = 4, 5, 6: the one-column kernel's 4-byte loads with the last Sobel column's shift."""
    rng = np.random.default_rng(W * 10 + H)
    frames = np.stack([rng.integers(0, 256, (H, W), dtype=np.uint8), (rng.integers(0, 2, (H, W)) * 255).astype(np.uint8),
                       fc.gftt_images(W, H)["diag_step"]])
    gftt_check(bm, frames, f"{W} x {H}")


@pytest.mark.parametrize("W,H,n,seg", fc.GFTT_BATCHES)
def test_gftt_batches_with_long_segments(torch_cuda, bm, W, H, n, seg):
    """launch_gftt_eig starts at 64 rows per wavefront and doubles that while seg < 256 and strips * ceil(H / (2 seg)) * n >=
    4096 (W >= 8; one strip at W = 9). 9 x 300, n = 1400: 3 * 1400 >= 4096, then 2 * 1400 < 4096 -> 128. 9 x 300, n = 4096:
    3 * 4096, 2 * 4096 >= 4096 -> 256. 9 x 511, n = 4096: -> 256, the last segment 255 rows. Eight distinct frames repeated;
    every one of the n maps and Max words is compared, so a wrong segment shows whichever wavefront took it."""
    torch = torch_cuda
    assert fc.gftt_launch_seg(W, H, n) == seg
    frames = fc.gftt_batch_frames(W, H)
    refs = [fc.gftt_eig(im) for im in frames]
    batch = dev(frames).repeat((n + 7) // 8, 1, 1)[:n].contiguous()
    eig, mx = bm.gftt_eig(batch)
    ref = dev(np.stack([r["eig"].astype(np.int32) for r in refs])).repeat((n + 7) // 8, 1, 1)[:n]
    rmx = dev(np.array([r["max"] for r in refs], np.int32)).repeat((n + 7) // 8)[:n]
    bad = (eig != ref).flatten(1).any(1) | (mx != rmx)
    if bool(bad.any()):
        i = int(torch.nonzero(bad)[0])
        assert_equal(eig[i].cpu().numpy(), refs[i % 8]["eig"].astype(np.int64), f"map {i} of {n} (frame {i % 8}), {int(bad.sum())} maps differ")
        assert int(mx[i]) == refs[i % 8]["max"], (i, int(mx[i]), refs[i % 8]["max"])
