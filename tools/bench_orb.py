"""Measure the ORB descriptors (computeDescriptor at the reference's values, the reference's pattern) on 640 x 480 frames and
print one JSON line:

  describe_ms / single_describe_ms   device time per sbm_orb_describe_device call (events on the engine's stream, median over
                                     --steps) on --n frames and on one frame, keypoints from sbm_gftt_detect_device
  features_ms / single_features_ms   the same for sbm_orb_features_device (detection + descriptors, one call)
  kept_per_frame                     keypoints left after the border rule (mean)
  bit_exact_first_8                  descriptors and kept points of the first 8 frames equal the CPU restatement's
  restatement_host_ms                the CPU restatement (oracle/orb_ref.c, single-threaded C) on one frame: for scale only

  python tools/bench_orb.py --frames golden|synth [--n 64] [--steps 20] [--warmup 3] [--out FILE]

--step-only runs the timed --n-frame describe calls and nothing else, for a kernel trace.
"""
import argparse
import ctypes
import json
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
    from u96_slam_amd import synth

    L, _ = synth.make_batch(0, n, 640, 480, 64)
    return np.ascontiguousarray(L)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", choices=("golden", "synth"), default="golden")
    ap.add_argument("--n", type=int, default=64)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--step-only", action="store_true")
    ap.add_argument("--out")
    a = ap.parse_args()

    import torch

    import _pkg
    import gftt_select_ref
    import orb_ref
    import sbm_oracle

    pkg = _pkg.load()
    bm = pkg.StereoBM.create(64, 21)
    L, h = bm._L, bm._h
    imgs = frames(a.frames, a.n)
    n, H, W = imgs.shape
    gp = pkg.gftt_select_params()
    op = pkg.orb_params()
    pat = np.ascontiguousarray(np.load(ROOT / "tests" / "golden" / "orb_pattern.npz")["pattern"], np.int32).reshape(-1)
    cap = pkg.gftt_select_capacity(gp, W, H)
    d_img = torch.from_numpy(imgs).to("cuda:0")
    eig = torch.empty((n, H, W), dtype=torch.int16, device="cuda:0")
    mx = torch.empty((n,), dtype=torch.int32, device="cuda:0")
    kp = torch.empty((n, cap, 2), dtype=torch.float32, device="cuda:0")
    cn = torch.empty((n,), dtype=torch.int32, device="cuda:0")
    kp2 = torch.empty_like(kp)
    cn2 = torch.empty_like(cn)
    desc = torch.zeros((n, cap, 32), dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    stream = torch.cuda.ExternalStream(L.sbm_stream(h), device="cuda:0")

    def check(st):
        if st != 0:
            raise RuntimeError(f"status {st}")

    check(L.sbm_gftt_detect_device(h, n, d_img.data_ptr(), W, H, ctypes.byref(gp), eig.data_ptr(), mx.data_ptr(), kp.data_ptr(),
                                   cn.data_ptr(), 1))
    calls = {
        "describe": lambda k: check(L.sbm_orb_describe_device(h, k, d_img.data_ptr(), W, H, cap, kp.data_ptr(), cn.data_ptr(),
                                                              pat.ctypes.data, ctypes.byref(op), kp2.data_ptr(), cn2.data_ptr(),
                                                              desc.data_ptr(), None, 0)),
        "features": lambda k: check(L.sbm_orb_features_device(h, k, d_img.data_ptr(), W, H, ctypes.byref(gp), pat.ctypes.data,
                                                              ctypes.byref(op), eig.data_ptr(), mx.data_ptr(), kp2.data_ptr(),
                                                              cn2.data_ptr(), desc.data_ptr(), None, 0)),
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
        timed("describe", n)
        return
    res = {"tool": "bench_orb", "frames": a.frames, "n": n, "width": W, "height": H, "cap": cap}
    res["describe_ms"] = timed("describe", n)
    res["single_describe_ms"] = timed("describe", 1)
    res["features_ms"] = timed("features", n)
    res["single_features_ms"] = timed("features", 1)
    calls["describe"](n)
    check(L.sbm_synchronize(h))
    counts, kps, ds = cn2.cpu().numpy(), kp2.cpu().numpy(), desc.cpu().numpy()
    exact = True
    for i in range(min(n, 8)):
        e_ref, m_ref = sbm_oracle.gftt_eig(imgs[i])
        pts = gftt_select_ref.select(e_ref, m_ref)
        wk, wd, _ = orb_ref.describe(imgs[i], pts, pat)
        exact &= bool(np.array_equal(kps[i, :counts[i]], wk)) and bool(np.array_equal(ds[i, :counts[i]], wd))
    res["bit_exact_first_8"] = exact
    res["kept_per_frame"] = float(np.mean(counts))
    e_ref, m_ref = sbm_oracle.gftt_eig(imgs[0])
    pts = gftt_select_ref.select(e_ref, m_ref)
    t0 = time.perf_counter()
    for _ in range(5):
        orb_ref.describe(imgs[0], pts, pat)
    res["restatement_host_ms"] = (time.perf_counter() - t0) / 5 * 1e3
    line = json.dumps(res)
    print(line)
    if a.out:
        pathlib.Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        pathlib.Path(a.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
