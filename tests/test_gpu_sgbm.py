"""The semi-global matcher on the GPU against the CPU restatement (oracle/sgbm_ref.c), bit for bit: the reference's call on the golden
pair (Python mirror and the C++ call-site program), C and S stage by stage, a seeded fuzz over the parameter space, batches,
host/device/asynchronous entry points, and every documented limit with the first value past it."""
import pathlib
import subprocess

import numpy as np
import pytest

import sgbm_ref
from gpu_support import build_callsite

ROOT = pathlib.Path(__file__).resolve().parents[1]

pytestmark = pytest.mark.gpu
HH, SG = sgbm_ref.MODE_HH, sgbm_ref.MODE_SGBM
UNSUPPORTED = -23
# main.cpp:219-230, positionally
REF_ARGS = (-64, 128, 11, 100, 1000, 32, 0, 15, 1000, 16, HH)


@pytest.fixture(scope="module")
def torch():
    import torch as t

    assert t.cuda.is_available()
    return t


def _pair(rng, H, W, kind="noise"):
    if kind == "flat":
        L = np.full((H, W), 90, np.uint8)
        L[:, W // 3:] = 91
        return L, np.roll(L, -2, axis=1)
    if kind == "smooth":
        base = (np.cumsum(rng.integers(-5, 6, (H, W + 64)), axis=1) % 256).astype(np.uint8)
    else:
        base = rng.integers(0, 256, (H, W + 64)).astype(np.uint8)
    s = int(rng.integers(0, 24))
    L = np.ascontiguousarray(base[:, 32:32 + W])
    R = np.clip(base[:, 32 + s:32 + s + W].astype(int) + rng.integers(-2, 3, (H, W)), 0, 255).astype(np.uint8)
    return L, R


def _device(torch, sg, Ls, Rs, **kw):
    dl = torch.from_numpy(np.ascontiguousarray(np.stack(Ls))).cuda()
    dr = torch.from_numpy(np.ascontiguousarray(np.stack(Rs))).cuda()
    return sg.compute(dl, dr, **kw)


def test_reference_call_on_golden_pair(pkg, golden):
    L, R = golden["rect_l"], golden["rect_r"]
    sg = pkg.StereoSGBM.create(*REF_ARGS)
    got = sg.compute(L, R)
    want = sgbm_ref.compute(sgbm_ref.make_params(*REF_ARGS), L, R)
    np.testing.assert_array_equal(got, want)
    assert (want > -65 * 16).mean() > 0.3   # a real map, not an all-invalid one


def _build_callsite(tmp_path, extra=()):
    exe, r = build_callsite(tmp_path, "sgbm_callsite_main.cpp", extra, exe="sgbm_callsite")
    assert r.returncode == 0, r.stderr
    return exe


@pytest.mark.parametrize("extra", [(), ("-DSBM_TEST_WITH_OPENCV", "-I", str(ROOT / "tests" / "cpp" / "mock_opencv"))],
                         ids=["raw", "mock_opencv"])
def test_callsite_program_matches_restatement(tmp_path, golden, extra):
    exe = _build_callsite(tmp_path, extra)
    L, R = golden["rect_l"], golden["rect_r"]
    (tmp_path / "l.raw").write_bytes(np.ascontiguousarray(L).tobytes())
    (tmp_path / "r.raw").write_bytes(np.ascontiguousarray(R).tobytes())
    out = tmp_path / "d.raw"
    r = subprocess.run([str(exe), str(tmp_path / "l.raw"), str(tmp_path / "r.raw"), str(L.shape[1]), str(L.shape[0]), str(out)],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    got = np.frombuffer(out.read_bytes(), np.int16).reshape(L.shape)
    np.testing.assert_array_equal(got, sgbm_ref.compute(sgbm_ref.make_params(*REF_ARGS), L, R))


@pytest.mark.parametrize("mode", [HH, SG])
def test_stages_C_S_and_premedian(pkg, torch, mode):
    rng = np.random.default_rng(7 + mode)
    L, R = _pair(rng, 23, 90, "smooth")
    args = (-5, 32, 7, 9, 70, 2, 20, 10, 0, 0, mode)
    p = sgbm_ref.make_params(*args)
    want, st = sgbm_ref.compute(p, L, R, stages=True)
    sg = pkg.StereoSGBM.create(*args)
    got = _device(torch, sg, [L], [R]).cpu().numpy()[0]
    shape = (1,) + st["C"].shape
    np.testing.assert_array_equal(sg.debug_fetch(4, shape)[0], st["C"])
    np.testing.assert_array_equal(sg.debug_fetch(5, shape)[0], st["S"])
    np.testing.assert_array_equal(sg.debug_fetch(6, (1, 23, 90))[0], st["pre"])
    np.testing.assert_array_equal(got, want)


def _fuzz_cases():
    rng = np.random.default_rng(2026)
    cases = []
    for i in range(36):
        nd = int(rng.choice([16, 32, 48, 64, 80, 128, 160, 256]))
        minD = int(rng.choice([-nd - 3, -17, -1, 0, 1, 2, 5, 30]))
        bs = int(rng.choice([-1, 0, 1, 3, 4, 5, 7, 9, 11]))
        cap = int(rng.choice([0, 15, 31, 63]))
        P1 = int(rng.choice([0, 4, 8, 100]))
        P2 = int(rng.choice([0, 32, 300, 1000, 6000]))
        kind = ["noise", "smooth", "flat"][i % 3]
        H = int(rng.integers(4, 40))
        w1 = int(rng.choice([1, 2, 7, 60, 150]))
        W = max(w1 + max(minD + nd, 0) - min(minD, 0), 3)
        p = sgbm_ref.make_params(minD, nd, bs, P1, P2, int(rng.choice([-1, 0, 1, 32])), cap, int(rng.choice([0, 5, 15, -1])),
                                 int(rng.choice([0, 0, 20])), int(rng.choice([0, 1, 4])), int(rng.choice([HH, SG])))
        if sgbm_ref.envelope(p) > 32767:
            p.p2 = 0
        if sgbm_ref.envelope(p) > 32767:
            p.block_size = 3
        cases.append((p, H, W, kind, int(rng.choice([0, 32, 64, 96]))))
    # saturation-heavy noise inside the envelope: 9 x 9 at cap 63, P2 near the edge
    cases.append((sgbm_ref.make_params(0, 64, 9, 50, 14000, 1, 63, 0, 0, 0, HH), 30, 120, "noise", 0))
    cases.append((sgbm_ref.make_params(0, 64, 9, 50, 14000, 1, 63, 0, 0, 0, SG), 30, 120, "noise", 0))
    return cases


def test_seeded_fuzz(pkg, torch, monkeypatch):
    rng = np.random.default_rng(11)
    for i, (p, H, W, kind, reading) in enumerate(_fuzz_cases()):
        Ls, Rs = zip(*[_pair(rng, H, W, kind) for _ in range(2)])
        monkeypatch.setenv("SBM_CV_READING", str(reading))
        sg = pkg.StereoSGBM.create(*[getattr(p, f) for f, _ in sgbm_ref.SgbmParams._fields_])
        got = _device(torch, sg, Ls, Rs).cpu().numpy()
        sg.close()
        for k in range(2):
            want = sgbm_ref.compute(p, Ls[k], Rs[k], reading=reading)
            assert np.array_equal(got[k], want), (i, k, [getattr(p, f) for f, _ in p._fields_], H, W, kind, reading,
                                                   int((got[k] != want).sum()))


def test_batch_host_device_async_agree(pkg, torch):
    rng = np.random.default_rng(5)
    Ls, Rs = zip(*[_pair(rng, 40, 200, "smooth") for _ in range(5)])
    args = (-8, 64, 5, 10, 120, 1, 0, 15, 50, 2, HH)
    p = sgbm_ref.make_params(*args)
    sg = pkg.StereoSGBM.create(*args)
    batch = _device(torch, sg, Ls, Rs).cpu().numpy()
    for k in range(5):
        single = _device(torch, sg, [Ls[k]], [Rs[k]]).cpu().numpy()[0]
        host = sg.compute(Ls[k], Rs[k])
        np.testing.assert_array_equal(batch[k], single)
        np.testing.assert_array_equal(host, single)
        np.testing.assert_array_equal(host, sgbm_ref.compute(p, Ls[k], Rs[k]))
    # strided host buffers (cv::Mat::step), as at main.cpp:233
    Lw = np.zeros((40, 256), np.uint8); Lw[:, :200] = Ls[0]
    Rw = np.zeros((40, 256), np.uint8); Rw[:, :200] = Rs[0]
    out = np.zeros((40, 300), np.int16)
    sg.compute(Lw[:, :200], Rw[:, :200], out[:, :200])
    np.testing.assert_array_equal(out[:, :200], batch[0])
    assert not out[:, 200:].any()
    d = _device(torch, sg, Ls, Rs, sync=False)
    sg.synchronize()
    np.testing.assert_array_equal(d.cpu().numpy(), batch)


def _check_limit(pkg, torch, args, H, W, n=1, ok=True, sample=None):
    p = sgbm_ref.make_params(*args)
    # (the pair count is a limit of the compute call, not of the parameters)
    assert pkg.sgbm_validate(pkg.sgbm_params(*args), W, H) == (0 if ok or n > 1 else UNSUPPORTED)
    if not ok:
        sg = pkg.StereoSGBM.create(*args)
        with pytest.raises(pkg.StereoBMError) as e:
            sg.compute(torch.zeros((n, H, W), dtype=torch.uint8, device="cuda"), torch.zeros((n, H, W), dtype=torch.uint8, device="cuda"))
        assert e.value.code == UNSUPPORTED
        return
    rng = np.random.default_rng(H * 7 + W)
    L = rng.integers(0, 256, (n, H, W)).astype(np.uint8)
    R = np.roll(L, -3, axis=2)
    sg = pkg.StereoSGBM.create(*args)
    got = sg.compute(torch.from_numpy(L).cuda(), torch.from_numpy(R).cuda()).cpu().numpy()
    idx = range(n) if sample is None else sorted(set(np.random.default_rng(1).integers(0, n, sample).tolist()) | {0, n - 1})
    for k in idx:
        np.testing.assert_array_equal(got[k], sgbm_ref.compute(p, L[k], R[k]))
    sg.close()


@pytest.mark.parametrize("W,ok", [(8192, True), (8193, False)])
def test_limit_width(pkg, torch, W, ok):
    _check_limit(pkg, torch, (0, 16, 3, 0, 0, 0, 0, 0, 0, 0, HH), 6, W, ok=ok)


@pytest.mark.parametrize("nd,ok", [(512, True), (528, False)])
def test_limit_disparities(pkg, torch, nd, ok):
    _check_limit(pkg, torch, (-nd // 2, nd, 3, 0, 0, 1, 0, 10, 0, 0, HH), 12, nd + 60, ok=ok)


@pytest.mark.parametrize("H,ok", [(65535, True), (65536, False)])
def test_limit_height(pkg, torch, H, ok):
    _check_limit(pkg, torch, (0, 16, 3, 0, 0, 0, 0, 0, 0, 0, SG), H, 24, ok=ok)


@pytest.mark.parametrize("n,ok", [(32767, True), (32768, False)])
def test_limit_pairs(pkg, torch, n, ok):
    _check_limit(pkg, torch, (0, 16, 3, 0, 0, 0, 0, 0, 0, 0, SG), 4, 22, n=n, ok=ok, sample=48)


@pytest.mark.parametrize("P2,ok", [(32767 - 121 * 189, True), (32768 - 121 * 189, False)])
def test_limit_envelope(pkg, torch, P2, ok):
    # blockSize 11 at cap 63: 121 * (2 * 63 + 63) = 22 869; the edge is P2 = 9898
    _check_limit(pkg, torch, (0, 32, 11, 100, P2, 1, 63, 5, 0, 0, HH), 20, 80, ok=ok)


@pytest.mark.parametrize("minD,ok", [(-2047, True), (-2048, False)])
def test_limit_min_disparity(pkg, torch, minD, ok):
    _check_limit(pkg, torch, (minD, 16, 3, 0, 0, 0, 0, 0, 0, 0, SG), 4, 2080, ok=ok)


@pytest.mark.parametrize("minD,ok", [(2031, True), (2032, False)])
def test_limit_max_disparity(pkg, torch, minD, ok):
    _check_limit(pkg, torch, (minD, 16, 3, 0, 0, 0, 0, 0, 0, 0, SG), 4, 2080, ok=ok)


@pytest.mark.parametrize("cap,uniq,ok", [(63, 65535, True), (64, 15, False), (31, 65536, False)])
def test_limit_cap_and_uniqueness(pkg, torch, cap, uniq, ok):
    _check_limit(pkg, torch, (0, 16, 3, 0, 0, 0, cap, uniq, 0, 0, SG), 8, 40, ok=ok)


@pytest.mark.parametrize("sr,ok", [(0, True), (-1, False)])
def test_limit_speckle_range(pkg, torch, sr, ok):
    _check_limit(pkg, torch, (0, 16, 3, 0, 0, 0, 0, 0, 10, sr, SG), 8, 40, ok=ok)


def test_chunked_batch_and_profile(pkg, torch):
    # 20 pairs of 640 x 360 at 256 disparities with the speckle filter on: C and S of 71 MB each, the pre-median map and the
    # speckle scratch make ~148 MB per pair -> chunks of 14 pairs within 2 GiB; every stage runs per chunk, and sampled pairs of
    # both chunks equal the restatement
    rng = np.random.default_rng(3)
    n, H, W = 20, 360, 640
    args = (0, 256, 3, 8, 64, 1, 0, 10, 100, 2, SG)
    base = (np.cumsum(rng.integers(-7, 8, (n, H, W + 16)), axis=2) % 256).astype(np.uint8)
    L, R = base[:, :, 16:].copy(), base[:, :, 10:10 + W].copy()
    sg = pkg.StereoSGBM.create(*args)
    sg.set_profiling(1)
    got = sg.compute(torch.from_numpy(L).cuda(), torch.from_numpy(R).cuda()).cpu().numpy()
    assert sg.profile("sgbm_aggregate") > 0 and sg.profile("sgbm_total") >= sg.profile("sgbm_cost")
    for which, shape in ((4, (n, H, W - 256, 256)), (6, (n, H, W))):
        with pytest.raises(pkg.StereoBMError):
            sg.debug_fetch(which, shape)   # more than one chunk: the stages are not kept for every pair
    p = sgbm_ref.make_params(*args)
    for k in (0, 7, 13, 14, 19):
        want = sgbm_ref.compute(p, L[k], R[k])
        np.testing.assert_array_equal(got[k], want)
    assert (got[:, :, 256:] > 0).any()   # a real map, not an all-invalid one


@pytest.mark.parametrize("mode", [HH, SG])
def test_all_saturated_pixels_have_no_winner(pkg, torch, mode):
    # high-contrast uncorrelated pairs, 11 x 11 at cap 63, P2 near the envelope's edge (121 * 189 + 9000 = 31 869), uniqueness 0:
    # S saturates at every disparity of some pixels, where OpenCV's winner loop finds no disparity and the pixel stays invalid
    rng = np.random.default_rng(40 + mode)
    Ls = [(rng.integers(0, 2, (20, 120)) * 255).astype(np.uint8) for _ in range(3)]
    Rs = [(rng.integers(0, 2, (20, 120)) * 255).astype(np.uint8) for _ in range(3)]
    for minD in (0, -3):
        args = (minD, 32, 11, 50, 9000, 1, 63, 0, 0, 0, mode)
        p = sgbm_ref.make_params(*args)
        sg = pkg.StereoSGBM.create(*args)
        got = _device(torch, sg, Ls, Rs).cpu().numpy()
        saturated = 0
        for k in range(3):
            want, st = sgbm_ref.compute(p, Ls[k], Rs[k], stages=True)
            saturated += int((st["S"] == 32767).all(axis=2).sum())
            np.testing.assert_array_equal(got[k], want)
        assert saturated > 0
        sg.close()


def test_profile_of_a_reused_handle_starts_at_zero(pkg, torch):
    rng = np.random.default_rng(9)
    L, R = _pair(rng, 30, 120, "smooth")
    sg = pkg.StereoSGBM.create(0, 32, 5)
    sg.set_profiling(1)
    _device(torch, sg, [L], [R])
    assert sg.profile("sgbm_total") > 0
    sg.close()                                  # parked for re-use
    sg2 = pkg.StereoSGBM.create(0, 32, 5)       # re-armed from the parked handles
    assert sg2.profile("sgbm_total") == 0.0
