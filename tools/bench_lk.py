"""Measure the pyramidal LK stereo path (computeCorrespondences at the reference's constants: 15 x 3, 5 levels, 30 iterations,
0.01, 1e-4, 0.5 < d <= 128) on the keypoints of the OpenCV-flavour detector (up to 1500 per frame) and print one JSON line:

  pyramid_ms / track_ms / stereo_ms   device time per sbm_lk_stereo_device call on --n pairs: the stage clock's "lk_pyramid" and
                                      "lk_track" (median over --steps profiled calls) and the whole call between two events on the
                                      engine's stream without profiling (median over --steps)
  single_*                            the same three for one pair
  depth3d_ms                          sbm_keypoints3d_lk_device on the call's outputs
  dense_compute_ms / dense_kp3d_ms    the dense route on the same pairs, same run: sbm_compute_device (64 disparities, block 21) and
                                      sbm_keypoints3d_device for every frame's keypoints
  sparse_route_ms / dense_route_ms    stereo_ms + depth3d_ms against dense_compute_ms + dense_kp3d_ms
  iterations_hist                     [level][iterations] point counts of the restatement over the first 4 pairs
  points_per_frame / tracked_per_frame   from the device counts and statuses
  restatement_1core_ms                oracle/lk_stereo_ref (sequential C) per pair on one core
  restatement_16proc_ms               --n pairs over 16 host processes, wall time
  bit_exact_first_4                   the device outputs of the first 4 pairs equal the restatement's

  python tools/bench_lk.py --frames golden|synth|kitti [--n 64] [--steps 20] [--warmup 3] [--out FILE]

golden: the 640 x 480 pair repeated; synth: 640 x 480 synthetic pairs; kitti: 1242 x 375 synthetic pairs.
"""
import argparse
import ctypes
import json
import multiprocessing
import pathlib
import statistics
import sys
import time

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "oracle"))


def pairs(kind, n):
    if kind == "golden":
        g = np.load(ROOT / "tests" / "golden" / "ref_pair_640x480.npz")
        return np.stack([g["rect_l"]] * n), np.stack([g["rect_r"]] * n)
    import _pkg

    _pkg.load()
    from u96_slam_amd import synth

    w, h = (1242, 375) if kind == "kitti" else (640, 480)
    L, R = synth.make_batch(0, n, w, h, 64)
    return np.ascontiguousarray(L), np.ascontiguousarray(R)


def _host_track(job):
    import lk_stereo_ref

    left, right, pts = job
    return int(lk_stereo_ref.correspondences(left, right, pts)[1].sum())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", choices=("golden", "synth", "kitti"), default="golden")
    ap.add_argument("--n", type=int, default=64)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out")
    a = ap.parse_args()

    import gftt_cv_ref
    import lk_stereo_ref

    Ls, Rs = pairs(a.frames, a.n)
    n, H, W = Ls.shape
    res = {"tool": "bench_lk", "frames": a.frames, "n": n, "width": W, "height": H}
    # the host legs first: the pool forks before this process opens the GPU
    lk_stereo_ref.lib()
    host_pts = [gftt_cv_ref.detect(Ls[i])[0] for i in range(min(n, 4))]
    t0 = time.perf_counter()
    hist = None
    for i, pts in enumerate(host_pts):
        lk_stereo_ref.correspondences(Ls[i], Rs[i], pts)
    res["restatement_1core_ms"] = (time.perf_counter() - t0) / len(host_pts) * 1e3
    for i, pts in enumerate(host_pts):
        hh = lk_stereo_ref.track(Ls[i], Rs[i], pts)[4]
        hist = hh if hist is None else hist + hh
    res["iterations_hist"] = hist[:, :32].tolist()
    jobs = [(Ls[i], Rs[i], host_pts[i % len(host_pts)]) for i in range(n)]
    with multiprocessing.Pool(16) as pool:
        pool.map(_host_track, jobs[:16])
        t0 = time.perf_counter()
        pool.map(_host_track, jobs)
        res["restatement_16proc_ms"] = (time.perf_counter() - t0) * 1e3

    import torch

    import _pkg

    pkg = _pkg.load()
    bm = pkg.StereoBM.create(64, 21)
    L, h = bm._L, bm._h
    p = pkg.lk_params()
    gp = pkg.gftt_cv_params()
    cap = gp.max_features
    dl, dr = torch.from_numpy(Ls).to("cuda:0"), torch.from_numpy(Rs).to("cuda:0")
    kp, cn = bm.gftt_cv_detect(dl, gp, maps=False)
    rp = torch.zeros((n, cap, 2), dtype=torch.float32, device="cuda:0")
    st = torch.zeros((n, cap), dtype=torch.uint8, device="cuda:0")
    er = torch.zeros((n, cap), dtype=torch.float32, device="cuda:0")
    xyz = torch.zeros((n, cap, 3), dtype=torch.float32, device="cuda:0")
    disp = torch.zeros((n, H, W), dtype=torch.int16, device="cuda:0")
    model = pkg.StereoModel()
    model.fx_l = model.fx_r = 700.0
    model.fy_l = model.fy_r = 700.0
    model.cx_l = model.cx_r = W / 2
    model.cy_l = H / 2
    model.Tx_r = -84.0
    torch.cuda.synchronize()
    stream = torch.cuda.ExternalStream(L.sbm_stream(h), device="cuda:0")

    def check(s):
        if s != 0:
            raise RuntimeError(f"status {s}")

    def kp3d_dense(k):
        for i in range(k):
            check(L.sbm_keypoints3d_device(h, disp[i].data_ptr(), W, H, kp[i].data_ptr(), cap, ctypes.byref(model), 0.0, 0.0,
                                           xyz[i].data_ptr(), 0))

    calls = {
        "stereo": lambda k: check(L.sbm_lk_stereo_device(h, k, dl.data_ptr(), dr.data_ptr(), W, H, kp.data_ptr(), cn.data_ptr(), cap,
                                                         ctypes.byref(p), rp.data_ptr(), st.data_ptr(), er.data_ptr(), 0)),
        "depth3d": lambda k: check(L.sbm_keypoints3d_lk_device(h, k, kp.data_ptr(), rp.data_ptr(), st.data_ptr(), cn.data_ptr(), cap,
                                                               ctypes.byref(model), 0.0, 0.0, xyz.data_ptr(), 0)),
        "dense_compute": lambda k: check(L.sbm_compute_device(h, k, dl.data_ptr(), dr.data_ptr(), W, H, disp.data_ptr(), 0)),
        "dense_kp3d": kp3d_dense,
    }

    def timed(name, k):
        for _ in range(a.warmup):
            calls[name](k)
        check(L.sbm_synchronize(h))
        ts = []
        for _ in range(a.steps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            calls[name](k)
            e1.record(stream)
            e1.synchronize()
            ts.append(e0.elapsed_time(e1))
        return statistics.median(ts)

    def staged(k):
        bm.set_profiling(1)
        try:
            rows = []
            for _ in range(a.steps):
                calls["stereo"](k)
                rows.append(bm.lk_profile())
        finally:
            bm.set_profiling(0)
        return statistics.median(r["lk_pyramid"] for r in rows), statistics.median(r["lk_track"] for r in rows)

    for tag, k in (("", n), ("single_", 1)):
        res[tag + "stereo_ms"] = timed("stereo", k)
        res[tag + "pyramid_ms"], res[tag + "track_ms"] = staged(k)
        res[tag + "depth3d_ms"] = timed("depth3d", k)
        res[tag + "dense_compute_ms"] = timed("dense_compute", k)
        res[tag + "dense_kp3d_ms"] = timed("dense_kp3d", k)
        res[tag + "sparse_route_ms"] = res[tag + "stereo_ms"] + res[tag + "depth3d_ms"]
        res[tag + "dense_route_ms"] = res[tag + "dense_compute_ms"] + res[tag + "dense_kp3d_ms"]
    calls["stereo"](n)
    check(L.sbm_synchronize(h))
    counts, kps = cn.cpu().numpy(), kp.cpu().numpy()
    rps, sts, ers = rp.cpu().numpy(), st.cpu().numpy(), er.cpu().numpy()
    exact = True
    for i in range(min(n, 4)):
        k = int(counts[i])
        wo, ws, we = lk_stereo_ref.correspondences(Ls[i], Rs[i], kps[i, :k])
        exact &= bool(np.array_equal(rps[i, :k].view(np.uint32), wo.view(np.uint32))) and bool(np.array_equal(sts[i, :k], ws)) and \
            bool(np.array_equal(ers[i, :k].view(np.uint32), we.view(np.uint32)))
    res["bit_exact_first_4"] = exact
    res["points_per_frame"] = float(np.mean(counts))
    res["tracked_per_frame"] = float(np.mean([sts[i, :counts[i]].sum() for i in range(n)]))
    line = json.dumps(res)
    print(line)
    if a.out:
        pathlib.Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        pathlib.Path(a.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
