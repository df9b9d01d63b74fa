"""estimate_motion on the MI355X against the independent statement of its arithmetic (tests/pnp_independent.py), not against the
restatement that shares the kernels' header: the hypotheses read through d_hyp, the counts, the inlier list, the refined pose,
the transform and the covariance scales. The scenes, the checks and every bound are those of
tests/test_pnp_math_independent.py, where the same checks run on the CPU restatement and the seeds are shown to need no
exemption at the gate. This module changes no kernel and reads the device's outputs only."""
import numpy as np
import pytest

import test_pnp_math_independent as cpu
from gpu_support import bm, dev  # noqa: F401
from test_gpu_pnp import K, model

pytestmark = pytest.mark.gpu


def run(bm, pkg, st, jobs, pairs, npairs, params, local=None):
    res, inl, hyp = bm.estimate_motion(dev(st.xyz), dev(st.kpts), dev(st.count), dev(pairs), dev(npairs), jobs, K, model(pkg, local),
                                       params, hyp=True)
    return pkg.pnp_records(res), inl.cpu().numpy(), pkg.pnp_records(hyp, pkg.PNP_HYP_DTYPE)


@pytest.mark.parametrize("iterations", cpu.ITERATIONS)
def test_hypotheses_of_noise_free_jobs_are_the_true_pose(bm, pkg, iterations):
    st, jobs, pairs, npairs = cpu.device_store("clean", iterations)
    recs, inl, hy = run(bm, pkg, st, jobs, pairs, npairs, cpu.params_for(iterations))
    assert hy.shape == (len(jobs), iterations)
    cpu.check_clean_hypotheses(hy, st)
    cpu.check_true_poses(recs, st)


@pytest.mark.parametrize("iterations", cpu.ITERATIONS)
def test_counts_are_the_independent_inlier_counts(bm, pkg, iterations):
    st, jobs, pairs, npairs = cpu.device_store("noisy", iterations)
    recs, inl, hy = run(bm, pkg, st, jobs, pairs, npairs, cpu.params_for(iterations))
    assert cpu.check_counts(hy, st) == 0
    if iterations == 300:
        assert cpu.check_inlier_lists(recs, inl, hy, st) == 0
        cpu.check_refined_poses(recs, inl, hy, st)


def test_poses_turned_about_the_optical_axis(bm, pkg):
    st, jobs, pairs, npairs = cpu.device_store("axis")
    recs, inl, hy = run(bm, pkg, st, jobs, pairs, npairs, cpu.params_for())
    cpu.check_true_poses(recs, st)


@pytest.mark.parametrize("name", [None] + list(cpu.LOCALS))
def test_transform_is_the_inverse_of_local_times_pnp(bm, pkg, name):
    lo = None if name is None else cpu.LOCALS[name].astype(np.float32)
    st, jobs, pairs, npairs = cpu.device_store("noisy", 64)
    recs, _, _ = run(bm, pkg, st, jobs[3:5], pairs[3:5], npairs[3:5], cpu.params_for(64), None if lo is None else lo.ravel())
    for r in recs:
        cpu.check_transform(r, lo)


@pytest.mark.parametrize("local", [None, "3 rad about y"])
@pytest.mark.parametrize("kind", list(cpu.COV_CASES))
def test_covariance_scales_are_the_upper_medians(bm, pkg, kind, local):
    lo = None if local is None else cpu.LOCALS[local].astype(np.float32)
    st, pairs, to, inl_ref = cpu.cov_scene(kind, lo)
    st.xyz[1, :65] = to
    recs, inl, _ = run(bm, pkg, st, [(0, 1)], pairs[None].copy(), np.array([65], np.int32), cpu.params_for(),
                       None if lo is None else lo.ravel())
    cpu.check_cov(recs[0], inl[0, :recs[0]["num_inliers"]], st, to, lo, kind, local)
