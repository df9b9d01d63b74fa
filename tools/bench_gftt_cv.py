"""Measure the OpenCV-flavour keypoint detector (generateKeypoints at the reference's constants: 1500, 0.01, 7.0, 3) and print one
JSON line:

  eig_ms / select_ms / detect_ms   device time per call on --n frames (events on the engine's stream, median over --steps) of
                                   sbm_gftt_cv_eig_device alone, sbm_gftt_cv_select_device alone (on those maps) and
                                   sbm_gftt_cv_detect_device (both, one call, maps kept)
  eig_gbps / eig_hbm_share         the map kernel's traffic at 5 B per pixel (1 read, 4 written) over its time, and that as a
                                   share of --hbm-gbps (8000: the MI355X's nominal HBM3E bandwidth)
  single_*                         the same three for one frame
  candidates_per_frame / points_per_frame   from the restatement on the first 8 frames / from the device counts
  restatement_1core_ms             oracle/gftt_cv_ref (sequential C) per frame on one core
  restatement_16proc_ms            --n frames over 16 host processes, wall time
  fpga_flavour_detect_ms           sbm_gftt_detect_device (the PL's uint16 map + generateKeypoints2) on the same frames, same run;
                                   null where the frames exceed that map's limits (width 1023, height 511)

  python tools/bench_gftt_cv.py --frames golden|synth|kitti [--n 64] [--steps 20] [--warmup 3] [--out FILE]

golden: the 640 x 480 pair repeated; synth: 640 x 480 synthetic frames; kitti: 1242 x 375 synthetic frames.
--step-only runs the timed --n frame detect calls and nothing else, for a kernel trace.
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


def frames(kind, n):
    if kind == "golden":
        g = np.load(ROOT / "tests" / "golden" / "ref_pair_640x480.npz")
        two = [g["rect_l"], g["rect_r"]]
        return np.stack([two[i % 2] for i in range(n)])
    import _pkg

    _pkg.load()
    from u96_slam_amd import synth

    w, h = (1242, 375) if kind == "kitti" else (640, 480)
    L, _ = synth.make_batch(0, n, w, h, 64)
    return np.ascontiguousarray(L)


def _host_detect(img):
    import gftt_cv_ref

    return len(gftt_cv_ref.detect(img)[0])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", choices=("golden", "synth", "kitti"), default="golden")
    ap.add_argument("--n", type=int, default=64)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--hbm-gbps", type=float, default=8000.0)
    ap.add_argument("--step-only", action="store_true")
    ap.add_argument("--out")
    a = ap.parse_args()

    imgs = frames(a.frames, a.n)
    n, H, W = imgs.shape
    res = {"tool": "bench_gftt_cv", "frames": a.frames, "n": n, "width": W, "height": H}
    if not a.step_only:   # the host legs first: the pool forks before this process opens the GPU
        import gftt_cv_ref

        gftt_cv_ref.lib()
        t0 = time.perf_counter()
        for i in range(min(n, 4)):
            gftt_cv_ref.detect(imgs[i])
        res["restatement_1core_ms"] = (time.perf_counter() - t0) / min(n, 4) * 1e3
        with multiprocessing.Pool(16) as pool:
            pool.map(_host_detect, list(imgs[:16]))
            t0 = time.perf_counter()
            pool.map(_host_detect, list(imgs))
            res["restatement_16proc_ms"] = (time.perf_counter() - t0) * 1e3

    import torch

    import _pkg

    pkg = _pkg.load()
    bm = pkg.StereoBM.create(64, 21)
    L, h = bm._L, bm._h
    p = pkg.gftt_cv_params()
    ps = pkg.gftt_select_params()
    cap = p.max_features
    res["params"] = {"max_features": p.max_features, "quality_level": p.quality_level, "min_distance": p.min_distance}
    d_img = torch.from_numpy(imgs).to("cuda:0")
    eig = torch.empty((n, H, W), dtype=torch.float32, device="cuda:0")
    mx = torch.empty((n,), dtype=torch.float32, device="cuda:0")
    eig16 = torch.empty((n, H, W), dtype=torch.int16, device="cuda:0")
    mx16 = torch.empty((n,), dtype=torch.int32, device="cuda:0")
    kp = torch.empty((n, cap, 2), dtype=torch.float32, device="cuda:0")
    cn = torch.empty((n,), dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    stream = torch.cuda.ExternalStream(L.sbm_stream(h), device="cuda:0")

    def check(st):
        if st != 0:
            raise RuntimeError(f"status {st}")

    calls = {
        "eig": lambda k: check(L.sbm_gftt_cv_eig_device(h, k, d_img.data_ptr(), W, H, eig.data_ptr(), mx.data_ptr(), 0)),
        "select": lambda k: check(L.sbm_gftt_cv_select_device(h, k, eig.data_ptr(), mx.data_ptr(), W, H, ctypes.byref(p),
                                                              kp.data_ptr(), cn.data_ptr(), 0)),
        "detect": lambda k: check(L.sbm_gftt_cv_detect_device(h, k, d_img.data_ptr(), W, H, ctypes.byref(p), eig.data_ptr(),
                                                              mx.data_ptr(), kp.data_ptr(), cn.data_ptr(), 0)),
        "fpga": lambda k: check(L.sbm_gftt_detect_device(h, k, d_img.data_ptr(), W, H, ctypes.byref(ps), eig16.data_ptr(),
                                                         mx16.data_ptr(), kp.data_ptr(), cn.data_ptr(), 0)),
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

    if a.step_only:
        timed("detect", n)
        return
    for tag, k in (("", n), ("single_", 1)):
        res[tag + "eig_ms"] = timed("eig", k)
        res[tag + "select_ms"] = timed("select", k)
        res[tag + "detect_ms"] = timed("detect", k)
        gbps = 5.0 * k * W * H / (res[tag + "eig_ms"] * 1e-3) / 1e9
        res[tag + "eig_gbps"] = gbps
        res[tag + "eig_hbm_share"] = gbps / a.hbm_gbps
    fits = W <= 1023 and H <= 511
    res["fpga_flavour_detect_ms"] = timed("fpga", n) if fits else None
    res["single_fpga_flavour_detect_ms"] = timed("fpga", 1) if fits else None
    calls["detect"](n)
    check(L.sbm_synchronize(h))
    counts = cn.cpu().numpy()
    kps = kp.cpu().numpy()
    maps = eig.cpu().numpy()
    import gftt_cv_ref

    ncand = []
    exact = True
    for i in range(min(n, 8)):
        pts, e_ref, m_ref, nc = gftt_cv_ref.detect(imgs[i])
        exact &= bool(np.array_equal(kps[i, :counts[i]], pts)) and bool(np.array_equal(maps[i].view(np.uint32), e_ref.view(np.uint32)))
        ncand.append(nc)
    res["bit_exact_first_8"] = exact
    res["candidates_per_frame"] = float(np.mean(ncand))
    res["points_per_frame"] = float(np.mean(counts))
    line = json.dumps(res)
    print(line)
    if a.out:
        pathlib.Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        pathlib.Path(a.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
