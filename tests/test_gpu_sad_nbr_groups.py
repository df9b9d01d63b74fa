"""The neighbour look-up of the interior SAD kernel's lone wavefronts (fast_neighbours_grouped, csrc/sbm_sad_fast_core.h): the sums
S[mind - 1] and S[mind + 1] are selected only in the groups of 32 buffer indices that a live lane of the wavefront-row needs, and in
the full tree when more than half of the groups are needed or SBM_FAST_NBR=0 says so. Same integers either way, so every case is
held twice: bit-exact against the CPU oracle (map, map before the LR check, cost plane -- with disp12MaxDiff 1 the cost plane also
goes through the LR stage) and byte-equal against SBM_FAST_NBR=0 on the same engine.

Content is DESIGNED: the left image is smoothed noise and the right image repeats it, column zone by column zone, moved by the
disparity that puts the winner at a chosen buffer index (index d <-> disparity nd - 1 - d). A stride-3 wavefront covers every
third column of its triple, so the zones of a pair are the groups its wavefront-rows need: one, two (adjacent or not), three, four.
Uniform pairs put the winner at the group edges, where mind - 1 and mind + 1 lie in different groups, and at the mirrored ends.
What the case claims is checked on the oracle's map: the winners are where they were put, and some wavefront-row has exactly that
many groups among its valid pixels (pixels that uniqueness rejects are live as well and do not show in the map: the claim is as
good as the CPU can tell). Pairs differ, rows of one pair do not (10 valid rows), except at ten row segments, where the patterns
rotate every 24 rows.

Shapes are the smallest that reach the path: one stride-3 triple and a last strip of 21 columns (folded at 128 disparities and
window 15, a plain strip elsewhere and under SBM_FAST_FOLD=0), 256 pairs because fewer are split over cooperating wavefronts, which
keep the tree. A plain strip of 21 columns is also the halo case: its lanes 21..63 and the lanes 60..63 of every stride-3 strip
produce nothing; they compute on the frame's padding or on exchange entries nobody wrote, so their winners are garbage that the
CPU cannot predict -- the live lanes of those rows sit in one group, and the maps say whether the garbage got a say.
Window 9 plans scaled planes (pfshift 2) like window 15; the untagged search is window 27 (pfshift 0), and window 9 with
SBM_FAST_PFSHIFT=0, which the library reads once per process: that case runs in a child process."""
import importlib.util
import os
import pathlib
import subprocess
import sys

import numpy as np
import pytest

ROOT = pathlib.Path(__file__).resolve().parents[1]
KW = dict(prefilter_cap=31, texture_threshold=10, uniqueness_ratio=10, disp12_max_diff=1, speckle_window_size=50, speckle_range=32)

# winners at the group edges and the mirrored ends (uniform pairs), 128 disparities
EDGES128 = [(k,) for k in (0, 1, 30, 31, 32, 33, 62, 63, 64, 65, 94, 95, 96, 97, 126, 127)]
# zones -> groups a stride-3 wavefront-row needs: one; two adjacent, two apart; three; four (the last two: through edge indices)
GROUPS128 = [(12,), (12, 20), (12, 44), (44, 76), (12, 108), (12, 44, 76), (12, 76, 108), (12, 44, 76, 108), (108, 76, 44, 12), (31, 97), (31, 95)]
NGROUPS128 = [1, 1, 2, 2, 2, 3, 3, 4, 4, 3, 4]
EDGES64 = [(0,), (31,), (32,), (63,), (12,), (44,), (12, 44), (44, 12)]
NGROUPS64 = [1, 2, 2, 1, 1, 1, 2, 2]

# name -> nd, w, W, H, pairs, content, what the content claims, parameter overrides, environment, hand-off mode
CASES = {
    "main_edges": (128, 15, 342, 24, 256, EDGES128, None, {}, {}, 0),
    "main_groups": (128, 15, 342, 24, 256, GROUPS128, NGROUPS128, {}, {}, 0),
    "main_groups_uniq60": (128, 15, 342, 24, 256, GROUPS128, NGROUPS128, dict(uniqueness_ratio=60), {}, 0),
    "main_groups_plain_last_strip": (128, 15, 342, 24, 256, GROUPS128, NGROUPS128, {}, dict(SBM_FAST_FOLD=0), 0),   # (the halo case)
    "main_edges_plain_last_strip": (128, 15, 342, 24, 256, EDGES128, None, {}, dict(SBM_FAST_FOLD=0), 0),
    "main_no_live_lane": (128, 15, 342, 24, 256, "constant", None, {}, {}, 0),
    "main_all_tied": (128, 15, 342, 24, 256, "constant", None, dict(texture_threshold=0, uniqueness_ratio=0), {}, 0),
    "main_synth_uniq10": (128, 15, 342, 24, 256, "synth", None, {}, {}, 0),
    "main_synth_uniq60": (128, 15, 342, 24, 256, "synth", None, dict(uniqueness_ratio=60), {}, 0),
    "segments_every_one_primes": (128, 15, 342, 96, 48, GROUPS128, None, {}, {}, 0),
    "segments_every_handoff_taken": (128, 15, 342, 96, 48, GROUPS128, None, {}, {}, 2),
    "nd64_w21": (64, 21, 278, 30, 256, EDGES64, NGROUPS64, {}, {}, 0),
    "nd64_w15": (64, 15, 278, 24, 256, EDGES64, NGROUPS64, {}, {}, 0),
    "nd112_masked": (112, 15, 326, 24, 256, [(0,), (111,), (110,), (95,), (96,), (12, 100), (12, 44, 76, 108), (111, 12)], None, {}, {}, 0),
    "nd96_masked": (96, 15, 310, 24, 256, [(0,), (95,), (94,), (63,), (64,), (12, 80), (12, 44, 76), (95, 12)], None, {}, {}, 0),
    "w9": (128, 9, 342, 18, 256, EDGES128[2:6] + GROUPS128, None, {}, {}, 0),
    "w27_untagged": (128, 27, 342, 36, 256, EDGES128[2:6] + GROUPS128, None, {}, {}, 0),
}
# (nd, w) -> the instantiation; the planes' scaling follows the window -- and the uniqueness ratio: at 60 the window-15 sums no longer
# fit scaled, so those cases run the untagged search as well
KERNEL = {(128, 15): "<128,1,5,3,true,true>", (64, 21): "<64,1,7,3,true,true>", (64, 15): "<64,1,5,3,true,true>",
          (112, 15): "<128,1,5,3,false,true>", (96, 15): "<128,1,5,3,false,true>", (128, 9): "<128,1,3,3,true,true>",
          (128, 27): "<128,1,9,3,true,true>"}
PFSHIFT = {9: 2, 15: 2, 21: 1, 27: 0}


def kernel_name(name):
    nd, w = CASES[name][:2]
    uniq = CASES[name][7].get("uniqueness_ratio", KW["uniqueness_ratio"])
    return f"{KERNEL[(nd, w)]} pfshift={0 if uniq > 10 else PFSHIFT[w]}"


CHILD = "w9_pfshift0"      # window 9 on unscaled planes: SBM_FAST_PFSHIFT=0 in a process of its own
CHILD_KERNEL = "<128,1,3,3,true,true> pfshift=0"


def _load(name):
    spec = importlib.util.spec_from_file_location("_nbr_" + name, ROOT / "tests" / (name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def designed(patterns, W, H, nd, x0, x1, rotate):
    """One pair per pattern: left = smoothed noise, right = noise with the left image's column zones (equal parts of the image
    columns [x0, x1), the outer ones out to the frame's edges) copied in at the zone's disparity. rotate: rows per pattern, 0 = all."""
    from u96_slam_amd import synth

    rng = np.random.default_rng(23)
    n = len(patterns)
    L = np.stack([synth.box3(rng.integers(0, 256, (H, W), dtype=np.uint8)) for _ in range(n)])
    R = np.stack([synth.box3(rng.integers(0, 256, (H, W), dtype=np.uint8)) for _ in range(n)])
    for i in range(n):
        for y0 in range(0, H, rotate or H):
            zones = patterns[(i + (y0 // rotate if rotate else 0)) % n]
            rows = slice(y0, min(H, y0 + (rotate or H)))
            edges = np.linspace(x0, x1, len(zones) + 1).astype(int)
            edges[0], edges[-1] = 0, W
            for z, k in enumerate(zones):
                D = nd - 1 - k
                a, b = max(int(edges[z]), D), int(edges[z + 1])
                if b > a:
                    R[i, rows, a - D:b - D] = L[i, rows, a:b]
    return L, R


def images(content, W, H, nd, x0, x1, rotate):
    from u96_slam_amd import synth

    if content == "constant":
        L = np.full((1, H, W), 100, np.uint8)
        return L, L.copy()
    if content == "synth":
        return synth.make_batch(0, 4, W, H, nd)
    return designed(content, W, H, nd, x0, x1, rotate)


def geometry(pkg, nd, w, W, H, n, kw, env):
    """The case's plan and the image columns of its stride-3 triple (x0, x1) and of its last strip (x1, x2)."""
    import test_bm_plan as plan
    import test_bm_plan_fold as foldplan

    c = dict(foldplan.case(W, H, n, nd, w, **{k: v for k, v in env.items() if k in plan.SWITCHES}), uniq=kw["uniqueness_ratio"], tex=kw["texture_threshold"])
    st, pl = plan.query(pkg, c)
    assert st == plan.OK and pl.fast
    f = pl.f
    assert (f.strips3, f.strips, f.NWAVES) == (3, 4, 1), (f.strips3, f.strips, f.NWAVES)   # one triple + one strip, lone wavefronts
    nv3 = 64 - (f.NTERM - 1)
    x0 = pl.g.lofs + f.xc0
    assert pl.g.lofs + f.xc1 - (x0 + 3 * nv3) == 21
    return pl, x0, x0 + 3 * nv3, pl.g.lofs + f.xc1


def reference(oracle, pkg, name):
    """Images (distinct pairs repeated up to n), the oracle's stages, the plan; and the check that the content is what it claims."""
    nd, w, W, H, n, content, claims, override, env, mode = CASES[name]
    kw = dict(KW, **override)
    pl, x0, x1, x2 = geometry(pkg, nd, w, W, H, n, kw, env)
    rotate = 24 if H > 60 else 0
    L, R = images(content, W, H, nd, x0, x1, rotate)
    distinct = len(L)
    p = oracle.make_params(num_disparities=nd, block_size=w, **kw)
    refs = [oracle.compute(p, L[i], R[i], stages=True)[1] for i in range(distinct)]
    pick = np.arange(n) % distinct
    ref = {k: np.stack([refs[i][k] for i in range(distinct)])[pick] for k in refs[0]}
    rows = slice(pl.g.row0, pl.g.row1)
    pre = np.stack([refs[i]["pre_lr"] for i in range(distinct)])[:, rows].astype(int)
    valid = pre >= 0
    mind = nd - 1 - ((pre + 8) >> 4)
    if content == "constant":
        tied = kw["texture_threshold"] == 0
        assert (pre[:, :, x0:x2] == ((nd - 1) * 16 if tied else -16)).all()      # index 0 wins every tie / every lane fails texture
    elif content != "synth" and not rotate:
        for i, zones in enumerate(content):
            if len(zones) == 1:          # the winner sits where it was put (the sub-pixel step moves the map by at most 8 / 16)
                at_k = np.abs(pre[i][:, x0:x2] - (nd - 1 - zones[0]) * 16) <= 8
                assert at_k.mean() > 0.9, (name, zones, float(at_k.mean()))
            if claims:                   # some wavefront-row (a row of one stride-3 phase) needs exactly that many groups
                counts = set()
                for ph in range(3):
                    m, v = mind[i][:, x0 + ph:x1:3], valid[i][:, x0 + ph:x1:3]
                    lo, hi = np.where(m > 0, m - 1, 1), np.where(m < nd - 1, m + 1, nd - 2)
                    for y in range(m.shape[0]):
                        counts.add(len(set((lo[y][v[y]] >> 5).tolist()) | set((hi[y][v[y]] >> 5).tolist())))
                assert claims[i] in counts, (name, zones, claims[i], sorted(counts))
    return dict(L=np.ascontiguousarray(L[pick]), R=np.ascontiguousarray(R[pick]), ref=ref, pl=pl, kw=kw, cols=(x0, x1, x2))


def run(pkg, parity, case, name, setenv, kernel):
    """The engine on the case, grouped look-up and SBM_FAST_NBR=0: both bit-exact to the oracle, byte-equal to each other."""
    import torch

    nd, w, W, H, n, content, claims, override, env, mode = CASES[name]
    pl, kw, ref = case["pl"], case["kw"], case["ref"]
    setenv("SBM_FAST_HANDOFF", str(mode))
    setenv("SBM_FAST_FOLD", str(env.get("SBM_FAST_FOLD", 1)))
    assert pl.kernel.decode() == "sad_fast_kernel" + kernel, pl.kernel.decode()
    assert pl.f.uniq_plain == (kw["uniqueness_ratio"] <= 10)
    assert (pl.f.nseg >= 3) if H > 60 else (pl.f.nseg == 1), pl.f.nseg
    later = (pl.f.nseg - 1) * n * pl.f.strips
    bm = pkg.StereoBM.create(nd, w, device=0)
    bm.setPreFilterCap(kw["prefilter_cap"]); bm.setTextureThreshold(kw["texture_threshold"]); bm.setUniquenessRatio(kw["uniqueness_ratio"])
    bm.setDisp12MaxDiff(kw["disp12_max_diff"]); bm.setSpeckleWindowSize(kw["speckle_window_size"]); bm.setSpeckleRange(kw["speckle_range"])
    dl, dr = torch.from_numpy(case["L"]).cuda(), torch.from_numpy(case["R"]).cuda()
    outs = {}
    for nbr in ("1", "0"):
        setenv("SBM_FAST_NBR", nbr)
        d = bm.compute_device(dl, dr).cpu().numpy()
        assert bm.last_kernel() == pl.kernel.decode()
        outs[nbr] = dict(disp=d, pre_lr=bm.debug_fetch(3, n, H, W), cost=bm.debug_fetch(2, n, H, W))
        taken, could = bm.debug_fetch(7).tolist()
        assert (taken, could) == ((0, 0) if mode == 0 else (later, later))
        parity.assert_stages_equal(outs[nbr], ref, dict(kw, num_disparities=nd, block_size=w))
    for k in ("disp", "pre_lr", "cost"):
        assert outs["1"][k].tobytes() == outs["0"][k].tobytes(), k
    if name == "main_no_live_lane":       # FILTERED with cost 0xffff, whatever the look-up returned
        x0, x1, x2 = case["cols"]
        rows = slice(pl.g.row0, pl.g.row1)
        assert (outs["1"]["pre_lr"][:, rows, x0:x2] == -16).all() and (outs["1"]["cost"][:, rows, x0:x2] == 0xffff).all()


@pytest.fixture(scope="module")
def ctx(pkg, oracle):
    import torch

    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    return dict(pkg=pkg, oracle=oracle, parity=_load("test_gpu_parity"))


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_grouped_lookup_matches_the_oracle_and_the_tree(ctx, monkeypatch, name):
    run(ctx["pkg"], ctx["parity"], reference(ctx["oracle"], ctx["pkg"], name), name, monkeypatch.setenv, kernel_name(name))


@pytest.mark.gpu
def test_window_9_on_unscaled_planes_in_a_process_of_its_own(ctx):
    """SBM_FAST_PFSHIFT is read once per process, so the untagged search at window 9 needs a fresh one."""
    env = dict(os.environ, SBM_FAST_PFSHIFT="0")
    r = subprocess.run([sys.executable, str(pathlib.Path(__file__).resolve()), CHILD], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "child ok" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]


def _child():
    sys.path[:0] = [str(ROOT), str(ROOT / "oracle"), str(ROOT / "tests")]
    import _pkg
    import sbm_oracle

    sbm_oracle.lib()
    pkg = _pkg.load()
    CASES[CHILD] = CASES["w9"]
    run(pkg, _load("test_gpu_parity"), reference(sbm_oracle, pkg, CHILD), CHILD, os.environ.__setitem__, CHILD_KERNEL)
    print("child ok")


if __name__ == "__main__" and sys.argv[1:] == [CHILD]:
    _child()
