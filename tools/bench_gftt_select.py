"""Measure the GFTT keypoint selection (generateKeypoints2 at the reference's constants: 1500, 0.01, 7.0) on 640 x 480 frames
and print one JSON line:

  eig_ms / select_ms / detect_ms   device time per call on 64 frames (events on the engine's stream, median over --steps) of
                                   sbm_gftt_eig_device alone, sbm_gftt_select_device alone (on those maps) and
                                   sbm_gftt_detect_device (both, one call)
  single_detect_ms                 the same for one frame
  candidates_per_frame             interior pixels over the threshold (mean over the frames)
  scanned_per_frame                candidates taken in order until the last accepted point (mean): what the trim must see
  points_per_frame                 accepted points (mean)
  restatement_host_ms              the CPU restatement (oracle/gftt_select_ref.c, single-threaded C) on one frame: for scale only

  python tools/bench_gftt_select.py --frames golden|synth [--n 64] [--steps 20] [--warmup 3] [--out FILE]

--step-only runs the timed 64-frame select calls and nothing else, for a kernel trace.
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


def scanned(eig, mx, pts, q=0.01):
    """1 + the position, in the (value desc, index desc) order, of the last accepted point (all candidates when none)."""
    H, W = eig.shape
    sub = eig[1:-1, 1:-1]
    ys, xs = np.nonzero(sub.astype(np.float64) >= (mx & 0xffff) * q)
    v = sub[ys, xs].astype(np.int64)
    idx = (ys + 1) * W + xs + 1
    order = np.lexsort((-idx, -v))
    if len(pts) == 0:
        return len(order)
    last = int(pts[-1][1]) * W + int(pts[-1][0])
    return int(np.nonzero(idx[order] == last)[0][0]) + 1


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
    import sbm_oracle

    pkg = _pkg.load()
    bm = pkg.StereoBM.create(64, 21)
    L, h = bm._L, bm._h
    imgs = frames(a.frames, a.n)
    n, H, W = imgs.shape
    p = pkg.gftt_select_params()
    cap = pkg.gftt_select_capacity(p, W, H)
    d_img = torch.from_numpy(imgs).to("cuda:0")
    eig = torch.empty((n, H, W), dtype=torch.int16, device="cuda:0")
    mx = torch.empty((n,), dtype=torch.int32, device="cuda:0")
    kp = torch.empty((n, cap, 2), dtype=torch.float32, device="cuda:0")
    cn = torch.empty((n,), dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    stream = torch.cuda.ExternalStream(L.sbm_stream(h), device="cuda:0")

    def check(st):
        if st != 0:
            raise RuntimeError(f"status {st}")

    calls = {
        "eig": lambda k: check(L.sbm_gftt_eig_device(h, k, d_img.data_ptr(), W, H, eig.data_ptr(), mx.data_ptr(), 0)),
        "select": lambda k: check(L.sbm_gftt_select_device(h, k, eig.data_ptr(), mx.data_ptr(), W, H, ctypes.byref(p), kp.data_ptr(),
                                                           cn.data_ptr(), 0)),
        "detect": lambda k: check(L.sbm_gftt_detect_device(h, k, d_img.data_ptr(), W, H, ctypes.byref(p), eig.data_ptr(),
                                                           mx.data_ptr(), kp.data_ptr(), cn.data_ptr(), 0)),
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

    calls["eig"](n)
    check(L.sbm_synchronize(h))
    if a.step_only:
        timed("select", n)
        return
    res = {"tool": "bench_gftt_select", "frames": a.frames, "n": n, "width": W, "height": H,
           "params": {"max_features": p.max_features, "quality_level": p.quality_level, "min_distance": p.min_distance}}
    res["eig_ms"] = timed("eig", n)
    res["select_ms"] = timed("select", n)
    res["detect_ms"] = timed("detect", n)
    res["single_detect_ms"] = timed("detect", 1)
    calls["detect"](n)
    check(L.sbm_synchronize(h))
    counts = cn.cpu().numpy()
    kps = kp.cpu().numpy()
    maps = (eig.cpu().numpy().view(np.uint16))
    mxs = mx.cpu().numpy()
    ncand, nscan = [], []
    exact = True
    for i in range(min(n, 8)):
        e_ref, m_ref = sbm_oracle.gftt_eig(imgs[i])
        pts = gftt_select_ref.select(e_ref, m_ref)
        exact &= bool(np.array_equal(kps[i, :counts[i]], pts)) and bool(np.array_equal(maps[i], e_ref))
        ncand.append(gftt_select_ref.candidates(e_ref, m_ref))
        nscan.append(scanned(e_ref, int(m_ref), pts))
    res["bit_exact_first_8"] = exact
    res["candidates_per_frame"] = float(np.mean(ncand))
    res["scanned_per_frame"] = float(np.mean(nscan))
    res["points_per_frame"] = float(np.mean(counts))
    e_ref, m_ref = sbm_oracle.gftt_eig(imgs[0])
    t0 = time.perf_counter()
    for _ in range(5):
        gftt_select_ref.select(e_ref, m_ref)
    res["restatement_host_ms"] = (time.perf_counter() - t0) / 5 * 1e3
    line = json.dumps(res)
    print(line)
    if a.out:
        pathlib.Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        pathlib.Path(a.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
