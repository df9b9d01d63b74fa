"""The small kernels in front of and behind the matcher, restated, and the inputs their edge tests share.

Restatements (numpy and Python integers only), each written from the reference source its kernel cites, not from oracle/sbm_oracle.c:
  project / reproject / keypoints3d   Stereo.cpp:53-117,157-199 and main.cpp:522-553, the type of every operation explicit
  decimate                            SensorData.cpp:50-58
  to_float                            cv convertTo(CV_32F, 1. / 16)
  rect_map                            fpga.c:303-366 in Python integers (py_rect_point of tests/test_frontend.py, extended to report
                                      lw and whether any intermediate leaves the int64 range)
  rect_remap                          rect_intp.v:285-404 (py_remap_point of tests/test_frontend.py, and the same vectorised)
  gftt_eig                            gftt_sbl.v, gftt_eig.v, gftt_box.v, gftt_obuf.v in int64, with the intermediates a, c, b, s, e
tests/test_frontend_cases_restatement.py holds them to the oracle on the CPU, tests/test_gpu_frontend_edges.py holds the HIP kernels
to them on the GPU; both read the inputs below, so that the two comparisons are over the same cases.

Rectifier calibrations that overflow int64. The firmware's C (fpga.c:303-366) multiplies in `long long`; a product that leaves
its range is undefined behaviour there, so such a calibration has no defined map and is not a case. rot[2][2] = 1 (the integer,
not 1.0 in s1.24) with the other two entries of the column 0 is one: lw == 1 on every pixel, 2^48 / lw == 2^48, and lx * 2^48
overflows wherever |lx| >= 2^15. The test asserts from rect_point's flag that no pixel of any case below overflows.

GFTT regimes. Besides the regimes the structured images reach by construction, two were searched for:
  b at its limiter      reached, narrowly: `diag_blobs`. Diagonal steps and stripes of period 2 to 8 stop at 54 864 (period 3). An
                        exhaustive search over the 2^25 0/255 patches of 5 x 5 pixels gives 69 088 > 65 535 as the largest 3 x 3 box
                        sum of |dx dy| >> 6, for the seven-pixel anti-diagonal blob (.XX / XXX / XX.); hill climbing over all
                        grey levels from there finds nothing larger. The image tiles that blob every 9 columns and 8 rows.
  a + c - r < 0         reached: `step75_noise4` (a vertical step of 75 grey levels under noise over four grey levels). There
                        |dx| is about 300 and |dy| below 8, so dy^2 >> 6 is 0 while |dx dy| >> 6 is not: c == 0, b > 0 and
                        r = floor(sqrt((a^2 >> 10 << 10) + 4 b^2 ...)) exceeds a. The truncations break b^2 <= a c.
"""
import functools

import numpy as np

from test_frontend import CAM_L, py_rect_point, py_remap_point, scaled_cam

F32, F64, I64 = np.float32, np.float64, np.int64


# ================================================================================================= consumers: restatements ====
LOCAL = (0, 0, 1, 0.1, -1, 0, 0, 0.2, 0, -1, 0, 0.3)


def make_model(fx=718.856, fy=718.856, cx=607.1928, cy=185.2157, baseline=0.537, cx_r=None, local=None):
    """The fields of sbm_stereo_model for a rectified pair, P1 = [f 0 cx_r -f b; ...], as a dict (doubles; local 12 floats)."""
    return dict(fx_l=fx, fy_l=fy, cx_l=cx, cy_l=cy, Tx_l=0.0, fx_r=fx, fy_r=fy, cx_r=cx if cx_r is None else cx_r,
                Tx_r=-fx * baseline, local=None if local is None else tuple(float(v) for v in local))


def fill_model(struct, m):
    """m into a ctypes mirror of sbm_stereo_model (the oracle's or the package's) -> struct."""
    for k in ("fx_l", "fy_l", "cx_l", "cy_l", "Tx_l", "fx_r", "fy_r", "cx_r", "Tx_r"):
        setattr(struct, k, m[k])
    struct.has_local = 0 if m["local"] is None else 1
    struct.local[:] = [0.0] * 12 if m["local"] is None else list(m["local"])
    return struct


def project(px, py, disp, m):
    """projectDisparityTo3D (Stereo.cpp:157-182) of float32 arrays -> (x, y, z) float32, NaN where not disp > 0."""
    px, py, disp = (np.asarray(v, F32) for v in (px, py, disp))
    with np.errstate(all="ignore"):
        c = F32(F64(m["cx_r"]) - F64(m["cx_l"]))                            # float c = (float)(cx_r - cx_l)
        dc = (disp + c).astype(F64)                                         # disp + c in float, promoted by the division
        Wx = ((F64(m["Tx_l"]) / F64(m["fx_l"]) - F64(m["Tx_r"]) / F64(m["fx_r"])) / dc).astype(F32)
        Wy = ((F64(m["Tx_l"]) / F64(m["fy_l"]) - F64(m["Tx_r"]) / F64(m["fy_r"])) / dc).astype(F32)
        x = ((px.astype(F64) - F64(m["cx_l"])) * Wx.astype(F64)).astype(F32)
        y = ((py.astype(F64) - F64(m["cy_l"])) * Wy.astype(F64)).astype(F32)
        z = (F64(m["fx_l"]) * Wx.astype(F64)).astype(F32)
        bad = ~(disp > 0)
    nan = F32(np.nan)
    return np.where(bad, nan, x), np.where(bad, nan, y), np.where(bad, nan, z)


def transform(x, y, z, t):
    """transformPoint (Stereo.cpp:189-199): float32, summed left to right."""
    t = [F32(v) for v in t]
    with np.errstate(all="ignore"):
        return (t[0] * x + t[1] * y + t[2] * z + t[3], t[4] * x + t[5] * y + t[6] * z + t[7], t[8] * x + t[9] * y + t[10] * z + t[11])


def reproject(disp, scale, m, apply_local=True):
    """main.cpp:522-553 up to the local transform: int16 (H, W) -> float32 (H, W, 3), NaN where d <= 0 or the point is not finite."""
    H, W = disp.shape
    d = disp.astype(F32) / F32(16)
    col, row = np.meshgrid((np.arange(W) * scale).astype(F32), (np.arange(H) * scale).astype(F32))
    x, y, z = project(col, row, d, m)
    ok = (d > 0) & np.isfinite(x) & np.isfinite(y) & np.isfinite(z)
    if apply_local and m["local"] is not None:
        x, y, z = transform(x, y, z, m["local"])
    out = np.stack([x, y, z], -1).astype(F32)
    out[~ok] = np.nan
    return out


def keypoints3d(disp, kp, m, min_depth=0.0, max_depth=0.0):
    """generateKeypoints3DStereo, dense-map branch (Stereo.cpp:53-117): int16 (H, W), float32 (nk, 2) -> float32 (nk, 3)."""
    H, W = disp.shape
    kp = np.asarray(kp, F32).reshape(-1, 2)
    kx, ky = kp[:, 0], kp[:, 1]
    lim = F32(2.0 ** 31)
    with np.errstate(all="ignore"):
        conv = np.isfinite(kx) & np.isfinite(ky) & (np.abs(kx) < lim) & (np.abs(ky) < lim)   # (int) of anything else: no pixel
    ix = np.where(conv, np.trunc(np.where(conv, kx, 0)), -1).astype(I64)                     # (int) truncates toward zero
    iy = np.where(conv, np.trunc(np.where(conv, ky, 0)), -1).astype(I64)
    inside = conv & (ix >= 0) & (ix < W) & (iy >= 0) & (iy < H)
    d = disp[np.where(inside, iy, 0), np.where(inside, ix, 0)].astype(F32) / F32(16)
    d = np.where(d < 0, F32(0), d)
    x, y, z = project(kx, ky, d, m)
    lo, hi = F32(min_depth), F32(max_depth)
    with np.errstate(all="ignore"):
        ok = inside & (d != 0) & np.isfinite(x) & np.isfinite(y) & np.isfinite(z)
        ok &= (z > lo) if not lo < 0 else True
        ok &= (z <= hi) if not hi <= 0 else True
    if m["local"] is not None:
        x, y, z = transform(x, y, z, m["local"])
    out = np.stack([x, y, z], -1).astype(F32)
    out[~ok] = np.nan
    return out


def decimate(disp, s):
    H, W = disp.shape[-2:]
    return np.ascontiguousarray(disp[..., ::s, ::s][..., :H // s, :W // s])


def to_float(disp):
    return (disp.astype(F64) / 16).astype(F32)


def same_floats(a, b):
    """Bit-identical float32 arrays, NaN at the same places (payloads aside)."""
    a, b = np.ascontiguousarray(a, F32), np.ascontiguousarray(b, F32)
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(na, nb) and np.array_equal(a.view(np.uint32)[~na], b.view(np.uint32)[~nb])


def first_diffs(a, b, k=5):
    """Indices of the first k elements at which two float32 arrays differ in bits or in NaN-ness."""
    a, b = np.ascontiguousarray(a, F32), np.ascontiguousarray(b, F32)
    na, nb = np.isnan(a), np.isnan(b)
    bad = (na != nb) | (~na & ~nb & (a.view(np.uint32) != b.view(np.uint32)))
    return [tuple(int(v) for v in i) for i in np.argwhere(bad)[:k]]


# ================================================================================================= consumers: inputs ==========
PW = PH = 256


def disparity_planes():
    """int16 (3, 256, 256): every int16 value once per plane. The positive values fill the plane from its border inwards (ring
    by ring, shuffled among themselves), so every border pixel and every pixel near (0, 0) holds one; planes 1 and 2 are
    plane 0 rolled along its rows and its columns (batch index)."""
    rng = np.random.default_rng(20261019)
    r, c = np.meshgrid(np.arange(PH), np.arange(PW), indexing="ij")
    ring = np.minimum(np.minimum(r, c), np.minimum(PH - 1 - r, PW - 1 - c)).ravel()
    order = np.argsort(ring, kind="stable")
    vals = np.concatenate([rng.permutation(np.arange(1, 32768)), rng.permutation(np.arange(-32768, 1))]).astype(np.int16)
    p = np.empty(PW * PH, np.int16)
    p[order] = vals
    p = p.reshape(PH, PW)
    return np.stack([p, np.roll(p, 77, axis=1), np.roll(p, -31, axis=0)])


def models():
    """name -> model. See the issue's list: each arithmetic regime of projectDisparityTo3D, with a local transform where one
    changes what is computed."""
    out = {}

    def both(name, **kw):
        out[name] = make_model(**kw)
        out[name + "+local"] = make_model(local=LOCAL, **kw)

    both("kitti")
    both("cxr_gt", cx_r=615.25)
    both("cxr_lt_exact", cx=607.25, cx_r=601.0)           # c = -6.25 = -100/16: disp + c == 0 at disparity value 100, < 0 below
    both("subnormal", baseline=1e-42)                     # Wx, Wy, z in the float32 subnormal range
    out["overflow_1e38"] = make_model(baseline=1e38)      # Wx overflows float32 for the small disparities, fx Wx for more
    out["overflow_1e36+local"] = make_model(baseline=1e36, local=LOCAL)
    both("baseline0", baseline=0.0)
    both("fx_ne_fy_cy_neg", fx=700.0, fy=350.5, cx=300.25, cy=-12.5)
    return out


REPROJECT_SCALES = (1, 4, 7)


def keypoints(W=PW, H=PH, n_random=400):
    """float32 (nk, 2): random keypoints over (-3, W + 3) x (-3, H + 3) after the fixed edge list."""
    y, x = 100.25, 90.75
    inf, nan = np.inf, np.nan
    fixed = [(-0.5, y), (-0.999, -0.999), (-1.0, y), (W - 0.001, H - 0.001), (W, y), (x, H),
             (nan, y), (x, nan), (nan, nan), (inf, y), (x, inf), (-inf, y), (x, -inf),
             (3e9, y), (x, 3e9), (-3e9, y), (x, -3e9), (2.0 ** 31, y), (x, 2.0 ** 31), (-2.0 ** 31, y),
             (0.0, 0.0), (W - 1.0, H - 1.0), (x, -0.5), (0.999, 0.999)]
    rng = np.random.default_rng(4)
    rnd = np.stack([rng.uniform(-3, W + 3, n_random), rng.uniform(-3, H + 3, n_random)], 1)
    return np.concatenate([np.array(fixed), rnd]).astype(F32)


def depth_gates(disp, kp, m):
    """(min_depth, max_depth) pairs: the fixed ones, and gates equal to one reprojected keypoint's z, from the restatement of
    the ungated call: max_depth == z (kept by <=), the float32 just below z (dropped), min_depth == z (dropped by >)."""
    gates = [(0.0, 0.0), (2.0, 30.0), (-1.0, 8.0)]
    zs = keypoints3d(disp, kp, dict(m, local=None), 0.0, 0.0)[:, 2]        # the gates see z before the local transform
    zs = zs[np.isfinite(zs) & (zs > 0)]
    if len(zs):
        z = F32(np.sort(zs)[len(zs) // 2])
        gates += [(0.0, float(z)), (0.0, float(np.nextafter(z, F32(0)))), (float(z), 0.0)]
    return gates


KEYPOINT_COUNTS = (1, 255, 256, 257, 0)

DECIMATE_SCALES = (1, 2, 3, 4, 5, 8, 16)


def decimate_planes():
    rng = np.random.default_rng(53)
    return [rng.integers(-32768, 32768, (3, 37, 53)).astype(np.int16), disparity_planes()]


def to_float_inputs():
    """int16 tensors: all 65 536 values as a plane (vector path only), 65 537 elements as a 65 537 x 1 plane (scalar tail), and
    1, 2, 3 elements."""
    allv = np.arange(-32768, 32768).astype(np.int16)
    return [allv.reshape(256, 256), np.concatenate([allv, allv[-7:-6]]).reshape(65537, 1), allv[5:6].reshape(1, 1),
            allv[::40000].reshape(1, 2), allv[::30000].reshape(3, 1)]


# ================================================================================================= rectifier ==================
RW, RH = 67, 45
_I64_MIN, _I64_MAX = -(1 << 63), (1 << 63) - 1


def rect_point(cam, xd, yd):
    """py_rect_point (tests/test_frontend.py) with lw and an overflow flag: ([x, y], lw, any intermediate outside int64)."""
    over = False

    def chk(v):
        nonlocal over
        if not _I64_MIN <= v <= _I64_MAX:
            over = True
        return v

    xn = chk((chk(xd * cam["f2inv"][0]) >> 8) - cam["c2_f2"][0])
    yn = chk((chk(yd * cam["f2inv"][1]) >> 8) - cam["c2_f2"][1])
    r = cam["rot"]
    l = [chk(chk((chk(r[0][k] * xn) >> 24) + (chk(r[1][k] * yn) >> 24)) + r[2][k]) for k in range(3)]
    den = l[2] % (1 << 64)                                  # conversion to unsigned long long
    inv = ((1 << 48) // den) if den else 0
    out = []
    for num, f, c in ((l[0], cam["f"][0], cam["c"][0]), (l[1], cam["f"][1], cam["c"][1])):
        v = chk((chk((chk(num * inv) >> 24) * f) >> 34) + (c << 6))
        v = chk(v + 1) >> 1
        v &= 0xFFFF
        out.append(v - 0x10000 if v & 0x8000 else v)
    return out, l[2], over


def rect_map(cam, W=RW, H=RH):
    """-> (int16 (H, W, 2) map, int64 (H, W) lw, bool (H, W) overflow)."""
    m, lw, ov = np.empty((H, W, 2), np.int16), np.empty((H, W), object), np.empty((H, W), bool)
    for y in range(H):
        for x in range(W):
            m[y, x], lw[y, x], ov[y, x] = rect_point(cam, x, y)
    return m, lw, ov


def _fix(v):
    return int(round(v * (1 << 24)))


def rect_cams():
    """name -> calibration on the 67 x 45 sensor: the firmware's left camera scaled, its rotation replaced."""
    base = scaled_cam(CAM_L, RW, RH)
    out = {}

    def put(name, rot, **kw):
        out[name] = dict(base, rot=[[int(v) for v in row] for row in rot], **kw)

    for deg in (0, 5, 30, 60, 89, 90, 120, 180, -45):
        c, s = np.cos(np.deg2rad(deg)), np.sin(np.deg2rad(deg))
        rx = [[1, 0, 0], [0, c, -s], [0, s, c]]
        ry = [[c, 0, s], [0, 1, 0], [-s, 0, c]]
        rz = [[c, -s, 0], [s, c, 0], [0, 0, 1]]
        for ax, R in (("x", rx), ("y", ry), ("z", rz)):
            put(f"rot{ax}{deg}", [[_fix(v) for v in row] for row in R])
    one = 1 << 24
    put("lw_zero", [[one, 0, 0], [0, one, 0], [1000, -2000, 0]])                 # rot[*][2] = 0: lw == 0 everywhere, den == 0
    put("lw_is_xn", [[one, 0, one], [0, one, 0], [0, 0, 0]])                     # lw == xn: changes sign along every row
    put("lw_minus1", [[one, 0, 0], [0, one, 0], [0, 0, -1]])                     # lw == -1: den == 2^64 - 1
    imax, imin = (1 << 31) - 1, -(1 << 31)
    put("rot_int32_extremes", [[imax, imin, imax], [imin, imax, imin], [imax, imin, imax]])
    put("f_int32_extremes", base["rot"], f=(imax, imin))
    return out


# ================================================================================================= resampler ==================
def rect_remap(src, rmap):
    """rect_intp.v:285-404 vectorised: uint8 (h, w) or (n, h, w) through an int16 (h, w, 2) map; taps outside the frame read 0."""
    src = np.asarray(src)
    if src.ndim == 3:
        return np.stack([rect_remap(s, rmap) for s in src])
    h, w = src.shape
    mx, my = rmap[..., 0].astype(I64), rmap[..., 1].astype(I64)
    xi, yi, xf, yf = mx >> 5, my >> 5, mx & 31, my & 31

    def tap(x, y):
        ok = (x >= 0) & (x < w) & (y >= 0) & (y < h)
        return np.where(ok, src[np.where(ok, y, 0), np.where(ok, x, 0)].astype(I64), 0)

    acc = (tap(xi, yi) * (32 - xf) * (32 - yf) + tap(xi + 1, yi) * xf * (32 - yf) + tap(xi, yi + 1) * (32 - xf) * yf
           + tap(xi + 1, yi + 1) * xf * yf)
    return (((acc >> 9) + 1) >> 1).astype(np.uint8)


def rect_remap_points(src, rmap):
    """The same, one py_remap_point call per pixel."""
    h, w = src.shape
    return np.array([[py_remap_point(src, int(rmap[y, x, 0]), int(rmap[y, x, 1])) for x in range(w)] for y in range(h)], np.uint8)


def remap_maps(w, h, fracs=tuple(range(32))):
    """Maps for a w x h frame, built rather than drawn: every (xi, yi) of {-2, -1, 0, w-2, w-1, w} x {-2, -1, 0, h-2, h-1, h}
    times every (xf, yf) of fracs^2 -- each side of the resampler's fast-path boundary at every fraction -- then the int16
    extremes in either coordinate; laid out over as many (h, w, 2) planes as that takes, the last one wrapping round."""
    xs, ys = sorted({-2, -1, 0, w - 2, w - 1, w}), sorted({-2, -1, 0, h - 2, h - 1, h})
    ent = [(xi * 32 + xf, yi * 32 + yf) for yi in ys for xi in xs for yf in fracs for xf in fracs]
    mid = (((w - 1) // 2) * 32 + 13, ((h - 1) // 2) * 32 + 7)
    for e in (-32768, 32767):
        ent += [(e, mid[1]), (mid[0], e), (e, e), (e, -e - 1), (e, 0), (0, e)]
    ent = np.array(ent, np.int16)
    per = w * h
    planes = -(-len(ent) // per)
    idx = np.arange(planes * per) % len(ent)
    return [ent[idx[i * per:(i + 1) * per]].reshape(h, w, 2) for i in range(planes)]


def remap_cases():
    """name -> (uint8 source (h, w) or (n, h, w), list of maps). The kernel resamples a frame onto a frame of the same size, so
    the boundary {-2, -1, 0, W-2, W-1, W} is that of the frame a map belongs to: the full construction is laid over a 192 x 192
    frame (two planes) and over a 40 x 30 one (31 planes); the tiny sources take a few fractions only."""
    rng = np.random.default_rng(192)
    few = (0, 1, 16, 31)
    out = {
        "192x192_random": (rng.integers(0, 256, (192, 192), dtype=np.uint8), remap_maps(192, 192)),
        "192x192_all255": (np.full((192, 192), 255, np.uint8), remap_maps(192, 192)),
        "40x30_random": (rng.integers(0, 256, (30, 40), dtype=np.uint8), remap_maps(40, 30)),
        "40x30_all255": (np.full((30, 40), 255, np.uint8), remap_maps(40, 30)),
        "width1": (rng.integers(1, 256, (30, 1), dtype=np.uint8), remap_maps(1, 30, few)),
        "1x1": (np.array([[201]], np.uint8), remap_maps(1, 1, few)),
        "3x1": (np.array([[7, 255, 130]], np.uint8), remap_maps(3, 1, few)),           # W * H < 4: the tail loop only
        "41x29_batch3": (rng.integers(0, 256, (3, 29, 41), dtype=np.uint8), remap_maps(41, 29)),   # W * H odd
    }
    return out


def fully_inside(rmap, w, h):
    """Pixels whose four taps all lie inside a w x h frame."""
    xi, yi = rmap[..., 0].astype(I64) >> 5, rmap[..., 1].astype(I64) >> 5
    return (xi >= 0) & (xi + 1 < w) & (yi >= 0) & (yi + 1 < h)


# ================================================================================================= GFTT =======================
def _isqrt(n):
    r = np.floor(np.sqrt(n.astype(F64))).astype(I64)
    r -= (r * r > n)
    r += ((r + 1) * (r + 1) <= n)
    assert ((r * r <= n) & ((r + 1) * (r + 1) > n)).all()
    return r


def gftt_eig(img):
    """uint8 (H, W) -> dict: eig uint16 (H, W) (rows 2..H-3 written, 0 elsewhere), max, and for the written rows the int64
    (H - 4, W) intermediates a, c, b (after their limiters), a_raw, c_raw, b_raw (before), s (the 22-bit radicand, capped),
    s_raw, r and e = a + c - r before its clamp."""
    p = np.asarray(img).astype(I64)
    H, W = p.shape
    dx, dy = np.zeros((H, W), I64), np.zeros((H, W), I64)
    # gftt_sbl.v: rows 1..H-2, the first and the last column forced to 0
    dx[1:-1, 1:-1] = (p[:-2, 2:] - p[:-2, :-2]) + 2 * (p[1:-1, 2:] - p[1:-1, :-2]) + (p[2:, 2:] - p[2:, :-2])
    dy[1:-1, 1:-1] = (p[2:, :-2] - p[:-2, :-2]) + 2 * (p[2:, 1:-1] - p[:-2, 1:-1]) + (p[2:, 2:] - p[:-2, 2:])
    ax, ay = np.abs(dx), np.abs(dy)

    def box(v):                                             # gftt_box.v: 3-sum along the row, 0 in the edge columns; 3 rows
        hs = np.zeros((H, W), I64)
        hs[:, 1:-1] = v[:, :-2] + v[:, 1:-1] + v[:, 2:]
        return hs[1:-3] + hs[2:-2] + hs[3:-1]               # rows 2..H-3

    raw = [box((ax * ax) >> 6), box((ay * ay) >> 6), box((ax * ay) >> 6)]
    a, c, b = (np.minimum(v, 0xffff) for v in raw)
    s_raw = (((a - c) * (a - c)) >> 10) + ((b * b) >> 8)
    s = np.minimum(s_raw, 0x3fffff)
    r = _isqrt(s << 10)
    e = a + c - r
    eig = np.zeros((H, W), np.uint16)
    eig[2:H - 2] = np.clip(e, 0, 0xffff)
    return dict(eig=eig, max=int(eig.max()), a=a, c=c, b=b, a_raw=raw[0], c_raw=raw[1], b_raw=raw[2], s=s, s_raw=s_raw, r=r, e=e)


@functools.lru_cache(maxsize=None)
def sqrt_tables():
    """Over all 2^22 radicands s, rad = s << 10, r = floor(sqrt(rad)): (where r (r + 2) == rad, that is (r + 1)^2 == rad + 1, so
    that a `<=` in the kernel's one comparison would step past the root; where float32 sqrt(s) * 32, correctly rounded, truncates
    to r + 1, so that the root must be taken low before it is floored). The second is a CPU stand-in: the device's own square
    root instruction decides which radicands those are there."""
    s = np.arange(1 << 22, dtype=I64)
    rad = s << 10
    r = _isqrt(rad)
    return r * (r + 2) == rad, (np.sqrt(s.astype(F32)) * F32(32)).astype(I64) > r


def gftt_regimes(g):
    """Which regimes the interior columns of the written rows of one gftt_eig result reach -> dict name -> pixel count."""
    i = (slice(None), slice(1, -1))
    s, r = g["s"][i], g["r"][i]
    root = np.floor(np.sqrt(s.astype(F64))).astype(I64)
    edge, high = sqrt_tables()
    shows = (g["e"][i] >= 1) & (g["e"][i] <= 0xffff)        # a root one too large changes the clamped output
    return {"s == 0": int((s == 0).sum()), "0 < s < 1024": int(((s > 0) & (s < 1024)).sum()),
            "s a non-zero perfect square": int(((s > 0) & (root * root == s)).sum()),
            "s == 0x3fffff": int((s == 0x3fffff).sum()),
            "a at its limiter": int((g["a_raw"][i] > 0xffff).sum()), "c at its limiter": int((g["c_raw"][i] > 0xffff).sum()),
            "b at its limiter": int((g["b_raw"][i] > 0xffff).sum()), "a + c - r < 0": int((g["e"][i] < 0).sum()),
            "output 65535": int((g["eig"][2:-2][i] == 0xffff).sum()), "r == 65535": int((r == 65535).sum()),
            "r (r + 2) == rad, showing": int((edge[s] & shows).sum()),
            "float32 sqrt(s) * 32 truncates above the root, showing": int((high[s] & shows).sum())}


GFTT_REGIMES = ("s == 0", "0 < s < 1024", "s a non-zero perfect square", "s == 0x3fffff", "a at its limiter", "c at its limiter",
                "b at its limiter", "a + c - r < 0", "output 65535", "r == 65535", "r (r + 2) == rad, showing",
                "float32 sqrt(s) * 32 truncates above the root, showing")
GFTT_SIZES = ((130, 60), (126, 24), (127, 24), (253, 24), (254, 24))


def gftt_images(W, H):
    """name -> uint8 (H, W) structured image."""
    y, x = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    rng = np.random.default_rng(W * 1000 + H)
    u8 = lambda v: np.ascontiguousarray(v).astype(np.uint8)
    out = {"const0": u8(0 * x), "const255": u8(0 * x + 255), "ramp_x": u8(x % 256), "ramp_y": u8(y * 4 % 256),
           "ramp_diag": u8((x + y) % 256), "noise4": u8(rng.integers(0, 4, (H, W))), "noise256": u8(rng.integers(0, 256, (H, W))),
           "step_v": u8(255 * (x >= W // 2)), "step_h": u8(255 * (y >= H // 2)), "diag_step": u8(255 * (x - W // 2 >= y - H // 2)),
           "dot": u8(255 * ((x == W // 2) & (y == H // 2))), "quadrant": u8(255 * ((x >= W // 2) & (y >= H // 2))),
           "step75_noise4": u8(75 * (x >= W // 2) + rng.integers(0, 4, (H, W)))}
    cell = np.zeros((8, 9), I64)
    cell[:3, :3] = [[0, 1, 1], [1, 1, 1], [1, 1, 0]]
    out["diag_blobs"] = u8(255 * cell[y % 8, x % 9])
    for p in (1, 2, 4):
        out[f"checker{p}"] = u8(255 * (((x // p) + (y // p)) & 1))
    for p in (1, 2):
        out[f"stripes_x{p}"] = u8(255 * ((x // p) & 1))
        out[f"stripes_y{p}"] = u8(255 * ((y // p) & 1))
    for p in (3, 5):
        out[f"stripes_diag{p}"] = u8(255 * (((x + y) // p) & 1))
    return out


GFTT_NARROW = tuple((w, h) for w in (4, 5, 6) for h in (5, 6, 7, 8))

# (W, H, n, seg): launch_gftt_eig starts at seg = 64 rows per wavefront and doubles it while seg < 256 and
# strips * ceil(H / (2 seg)) * n >= 4096 (two-column kernel, W >= 8; strips = ceil(W / 126) = 1 at W = 9):
#   9 x 300, n = 1400: seg 64: ceil(300/128) = 3, 4200 >= 4096 -> 128; seg 128: ceil(300/256) = 2, 2800 < 4096          -> 128
#   9 x 300, n = 4096: seg 64: 12288 -> 128; seg 128: 8192 -> 256                                                         -> 256
#   9 x 511, n = 4096: seg 64: ceil(511/128) = 4, 16384 -> 128; seg 128: 2 * 4096 -> 256; segments of 256 and 255 rows      -> 256
GFTT_BATCHES = ((9, 300, 1400, 128), (9, 300, 4096, 256), (9, 511, 4096, 256))


def gftt_launch_seg(W, H, n):
    """The launcher's rule restated (sbm_gftt.hip, launch_gftt_eig)."""
    two = W >= 8
    strips = -(-W // (126 if two else 62))
    seg = 64
    while seg < 256 and strips * -(-H // (2 * seg)) * n >= (4096 if two else 8192):
        seg *= 2
    return seg


def gftt_batch_frames(W, H):
    """uint8 (8, H, W): four noise frames and four structured ones; a batch repeats them."""
    rng = np.random.default_rng(H)
    g = gftt_images(W, H)
    return np.stack([rng.integers(0, 256, (H, W), dtype=np.uint8) for _ in range(3)] + [(rng.integers(0, 2, (H, W)) * 255).astype(np.uint8)]
                    + [g["checker2"], g["diag_step"], g["step75_noise4"], g["ramp_x"]])
