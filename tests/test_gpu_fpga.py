"""GPU parity of the FPGA-flavour matcher (u96-slam_amd/csrc/sbm_fpga.hip, through the C-ABI) against the CPU
restatement of the RTL (oracle/sbm_oracle_fpga.c). Integer path: bit-exact. The oracle itself is parity-unpinned for
this stage (no RTL output in the reference, no simulator): see tests/test_oracle_fpga.py."""
import numpy as np
import pytest

from gpu_support import dev

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def bm(pkg):
    import torch

    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a visible MI355X")
    return pkg.StereoBM.create(64, 21)


def test_reference_stimulus_firmware_registers(pkg, bm, oracle, golden):
    """data/ref_xsbl_{l,r} = the RTL's own BM stimulus (sim_dvp.v:460-490), configured through the register words the
    firmware writes (fpga.c:155,158)."""
    p = pkg.fpga_params_from_regs((480 << 16) + 640, 0x00150040, 0)
    assert (p.width, p.height, p.block_size, p.num_disparities, p.uni_enable) == (640, 480, 21, 64, 0)
    got = bm.fpga_bm(dev(golden["xsbl_l"]), dev(golden["xsbl_r"]), p).cpu().numpy()
    ref = oracle.fpga_bm(golden["xsbl_l"], golden["xsbl_r"], 21, 64)
    assert np.array_equal(got, ref), int((got != ref).sum())
    # whole PL pipeline from the rectified pair: xsbl2 prefilter on the device, then the matcher
    got2 = bm.fpga_compute(dev(golden["rect_l"]), dev(golden["rect_r"]), p).cpu().numpy()
    assert np.array_equal(got2, ref)


@pytest.mark.parametrize("W,H,wsz,nd", [(200, 60, 9, 64), (333, 71, 21, 32), (400, 90, 15, 128), (700, 64, 5, 256),
                                        (161, 40, 31, 96), (640, 480, 21, 128)])
def test_random_frames_and_uniqueness_filter(pkg, bm, oracle, W, H, wsz, nd):
    rng = np.random.default_rng(W + wsz)
    n = 3
    xr = rng.integers(0, 64, (n, H, W)).astype(np.uint8)
    xl = np.stack([np.roll(xr[i], 5 + 11 * i, axis=1) for i in range(n)])
    xl = np.clip(xl.astype(int) + rng.integers(-4, 5, xl.shape), 0, 63).astype(np.uint8)
    for uni in ((0, 0, 0), (1, 0, 0x2c0), (1, 1, 0x100)):
        p = pkg.fpga_params(W, H, wsz, nd, *uni)
        got = bm.fpga_bm(dev(xl), dev(xr), p).cpu().numpy()
        for i in range(n):
            ref = oracle.fpga_bm(xl[i], xr[i], wsz, nd, *uni)
            assert np.array_equal(got[i], ref), (i, uni, int((got[i] != ref).sum()))


def test_saturating_column_sums_take_the_exact_pass(pkg, bm, oracle):
    """Only 0 / 63 inputs with wsz 21: column sums pass 1023, HSAD becomes history dependent (bm_calc_sad.v:103-125), the
    segmented launch flags the pair and the top-to-bottom launch must reproduce the RTL's clamped arithmetic."""
    rng = np.random.default_rng(5)
    H, W = 300, 260
    xl = (rng.integers(0, 2, (2, H, W)) * 63).astype(np.uint8)
    xr = (rng.integers(0, 2, (2, H, W)) * 63).astype(np.uint8)
    xr[:, :, ::3] = 63 - xl[:, :, ::3]
    xl[1] = rng.integers(0, 64, (H, W))          # pair 1 never saturates: stays on the segmented result
    xr[1] = np.roll(xl[1], -9, axis=1)
    p = pkg.fpga_params(W, H, 21, 64)
    got = bm.fpga_bm(dev(xl), dev(xr), p).cpu().numpy()
    for i in range(2):
        ref = oracle.fpga_bm(xl[i], xr[i], 21, 64)
        assert np.array_equal(got[i], ref), (i, int((got[i] != ref).sum()))
    # the unclamped sums really differ here, i.e. the case is not vacuous
    assert (got[0] != -1).any()


def test_limits_are_status_codes(pkg, bm):
    import torch

    z = torch.zeros((64, 200), dtype=torch.uint8, device="cuda:0")
    for kw, code in ((dict(block_size=20), -6), (dict(num_disparities=48), -7), (dict(num_disparities=288), -7)):
        p = pkg.fpga_params(200, 64, **{**dict(block_size=9, num_disparities=64), **kw})
        assert pkg.fpga_validate(p) == code
        with pytest.raises(pkg.StereoBMError) as e:
            bm.fpga_bm(z, z, p)
        assert e.value.code == code


def test_host_entry_points_of_the_pl_blocks(pkg, bm, oracle, golden):
    """sbm_fpga_compute / sbm_gftt_eig on host images with a row stride (cv::Mat::step), the shapes FPGA.cpp:270-291 hands out."""
    p = pkg.fpga_params_from_regs((480 << 16) + 640, 0x00150040, 0)
    wide_l = np.zeros((480, 700), np.uint8); wide_l[:, :640] = golden["rect_l"]
    wide_r = np.zeros((480, 700), np.uint8); wide_r[:, :640] = golden["rect_r"]
    got = bm.fpga_compute_host(wide_l[:, :640], wide_r[:, :640], p)
    assert np.array_equal(got, oracle.fpga_compute(golden["rect_l"], golden["rect_r"], 21, 64))
    eig, mx = bm.gftt_eig_host(wide_l[:, :640])
    ref, rmax = oracle.gftt_eig(golden["rect_l"])
    assert np.array_equal(eig, ref) and mx == rmax


@pytest.mark.parametrize("W,H,wsz,nd,amp,n", [(66, 26, 5, 32, 2, 3), (423, 25, 5, 192, 2, 2), (335, 104, 15, 96, 64, 1), (97, 40, 9, 64, 2, 3),
                                              (115, 46, 3, 96, 64, 2), (181, 150, 31, 64, 64, 3), (168, 125, 5, 96, 64, 1)])
def test_first_and_last_samples_of_a_batch(pkg, bm, oracle, W, H, wsz, nd, amp, n):
    """The two places where a window piece straddles the range-checked descriptor: sample (row 0, column 0) of every frame
    (HSAD column 0 of the last phase starts one byte in front of its row) and the last samples of the last row of the LAST
    frame (the piece ends a few bytes behind the batch). The hardware zeroes a whole 16-byte load that straddles, so those
    pieces are re-fetched dword / byte wise. Found by tools/soak.py: 1 wrong pixel per frame in 6 % (head) / 0.8 % (tail) of
    random configurations."""
    rng = np.random.default_rng(W * 7 + wsz)
    xr = (rng.integers(0, amp, (n, H, W)) * (63 if amp == 2 else 1)).astype(np.uint8)
    xl = np.stack([np.roll(xr[i], int(rng.integers(0, nd)), axis=1) for i in range(n)])
    p = pkg.fpga_params(W, H, wsz, nd, 0, 0, 0)
    got = bm.fpga_bm(dev(xl), dev(xr), p).cpu().numpy()
    for i in range(n):
        ref = oracle.fpga_bm(xl[i], xr[i], wsz, nd, 0, 0, 0)
        assert np.array_equal(got[i], ref), (i, int((got[i] != ref).sum()), np.argwhere(got[i] != ref)[:3].tolist())
