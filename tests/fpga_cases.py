"""Input makers of the FPGA-flavour matcher's tests, shared by tests/test_oracle_fpga.py (the C oracle against its numpy
restatement, CPU) and tests/test_gpu_fpga_paths.py (the device against the C oracle). x-Sobel planes are uint8 with 6
significant bits. TEST INFRASTRUCTURE ONLY."""
import numpy as np

# the three settings of the uniqueness filter every family of cases is run under: off (the firmware's), on with the
# masked value 0x00 and a lenient threshold, on with the masked value 0xFF and a strict one
UNI = ((0, 0, 0), (1, 0, 0x300), (1, 1, 0x100))

# shifts that put the winner on the first / last lanes of a 32-disparity phase (lane j of phase k = disparity 32k + j - 1):
# its neighbour sums then come from the guard lanes 0 and 33, disparity -1 and disparity nd included
PHASE_END_SHIFTS = (0, 1, 31, 32, 33, 63, 64, 65, 95)


def shifted(rng, H, W, shift, amp=64):
    """xl = roll(xr, shift) of random amp-level data: SAD 0 at disparity `shift`, nowhere else (but by accident)."""
    xr = rng.integers(0, amp, (H, W)).astype(np.uint8)
    return np.roll(xr, shift, axis=1), xr


def noisy_shift(rng, H, W, shift, noise=4, amp=64):
    xl, xr = shifted(rng, H, W, shift, amp)
    xl = np.clip(xl.astype(int) + rng.integers(-noise, noise + 1, xl.shape), 0, amp - 1).astype(np.uint8)
    return xl, xr


def two_level(rng, H, W, hi=3):
    """Random 0 / hi on both planes: a handful of distinct SAD values, so minima tie within and across phases."""
    xl = (rng.integers(0, 2, (H, W)) * hi).astype(np.uint8)
    xr = (rng.integers(0, 2, (H, W)) * hi).astype(np.uint8)
    return xl, xr


def periodic8(rng, H, W, roll=3):
    """Every row an 8-column periodic pattern, the left plane the same pattern `roll` columns on: equal SADs (0) at
    disparities roll, roll + 8, roll + 16, ... across every phase boundary."""
    pat = rng.integers(0, 64, (H, 8)).astype(np.uint8)
    x = np.arange(W)
    return pat[:, (x - roll) % 8], pat[:, x % 8]


def zeros(H, W):
    return np.zeros((H, W), np.uint8), np.zeros((H, W), np.uint8)


def constant(H, W, left, right):
    return np.full((H, W), left, np.uint8), np.full((H, W), right, np.uint8)


def saturating(rng, H, W):
    """Only 0 / 63, every third column of the right plane the complement of the left: column sums of 17 or more rows pass the
    10-bit limiter (bm_calc_sad.v:103-113) and HSAD becomes history dependent."""
    xl = (rng.integers(0, 2, (H, W)) * 63).astype(np.uint8)
    xr = (rng.integers(0, 2, (H, W)) * 63).astype(np.uint8)
    xr[:, ::3] = 63 - xl[:, ::3]
    return xl, xr


def bounded(rng, H, W, wsz, shift, noise=2):
    """A noisy shift whose amplitude keeps wsz * max|L - R| <= 1023: no column sum can reach the limiter."""
    amp = min(64, 1023 // wsz + 1)
    return noisy_shift(rng, H, W, shift, noise, amp)


def near_limit(rng, H, W, wsz, spread=2):
    """Left plane 63, right plane random within `spread` of 63 - 1023 / wsz: the sum of wsz abs-diffs sits within a few units
    of the limiter, above it in some columns and below it in others. All lanes nearly tie, and which one wins depends on what
    the limiter cut off rows earlier: the map depends on the rows above (unlike `saturating` at window 17, whose saturated
    lanes are never winners). Windows of 17 rows and more."""
    lo = max(0, round(63 - 1023 / wsz) - spread)
    return np.full((H, W), 63, np.uint8), rng.integers(lo, lo + 2 * spread + 1, (H, W)).astype(np.uint8)


def between(rng, H, W, shift, noise=1):
    """The left plane half way between the right plane `shift` - 1 and `shift` columns on: two adjacent disparities with
    nearly equal, small SADs -- on either side of a phase boundary when shift is a multiple of 32 (bm_calc_upd.v's adjacency
    rule, ddisp1 == disp1 + 1)."""
    xr = rng.integers(0, 64, (H, W)).astype(int)
    xl = (np.roll(xr, shift - 1, axis=1) + np.roll(xr, shift, axis=1) + rng.integers(0, 2, (H, W))) // 2
    xl = np.clip(xl + rng.integers(-noise, noise + 1, (H, W)), 0, 63)
    return xl.astype(np.uint8), xr.astype(np.uint8)


def column_sums(xl, xr, wsz, nd):
    """[r][c]: the largest UNCLAMPED sum of abs-diffs over rows r .. r + wsz - 1 of HSAD column c (image column nd + c), over
    every lane's disparity D in [-1, nd]: what the column sums of output row r would be without the 10-bit limiter."""
    H, W = xl.shape
    L = (xl & 63).astype(np.int32)
    R = (xr & 63).astype(np.int32)
    x = np.arange(nd, W - 1)
    best = np.zeros((H - wsz + 1, x.size), np.int32)
    for D in range(-1, nd + 1):
        cs = np.cumsum(np.abs(R[:, x - D] - L[:, x]), axis=0)
        win = cs[wsz - 1:].copy()
        win[1:] -= cs[:-wsz]
        np.maximum(best, win, out=best)
    return best


def saturates(xl, xr, wsz, nd):
    """The largest unclamped column sum the matcher forms on this frame (column_sums). At most 1023: the limiter never acts
    and row segments are exact; above: at least one column sum saturates (the first one to pass 1023 does so with an
    unclamped history)."""
    return int(column_sums(xl, xr, wsz, nd).max())
