"""Sparse local bundle adjustment (vo_sba_solve; sparse_bundle_adjustment.cpp:150-643) against the CPU
restatement: double precision, so the bar is a relative 1e-9 on every pose entry and landmark coordinate
after MAX_ITER = 10 iterations (the summation order of the pose blocks differs: strided partial sums on the
device, landmark order on the CPU), and the per-iteration average errors to 1e-10."""
import numpy as np
import pytest

from visual_odometry_ros_amd import synthetic as S
from visual_odometry_ros_amd.api import SparseBundleAdjustmentSolver
from util import RIG_KITTI, sba_converged
from util import sba_run as _run  # device next to oracle.sba_solve at the bar of the docstring above

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("stereo", [False, True])
def test_sba_matches_oracle_kitti_window(ctx, oracle, stereo):
    """The reference's window: 9 keyframes (kitti_00_stereo.yaml:83), the first two fixed
    (motion_estimator.cpp:1127), ~1500 landmarks."""
    p = S.ba_window(n_kf=9, n_points=1800, stereo=stereo, seed=11)
    assert p["X"].shape[0] > 1000
    ok, T, X, err = _run(ctx, oracle, p)
    assert ok and err[0] > 1.0 and err[-1] < 0.6  # 0.3 px pixel noise -> ~0.42 px RMS floor
    # closer to the ground truth than the start
    assert np.abs(T - p["T_jw_true"]).max() < 0.3 * np.abs(p["T_jw"] - p["T_jw_true"]).max()
    # a second solve through the same context (arena reuse) gives the same bits
    sol = SparseBundleAdjustmentSolver(ctx, stereo)
    (sol.setStereoCameras(p["K"], p["K"], p["T_lr"]) if stereo else sol.setCamera(p["K"]))
    sol.setHuberThreshold(0.5)
    ok2, T2, X2, err2 = sol.solveForFiniteIterations(10, p["T_jw"], p["opt_index"], p["X"], p["obs_ptr"], p["obs_frame"],
                                                     p["obs_right"], p["obs_px"])
    assert np.array_equal(T2, T) and np.array_equal(X2, X) and np.array_equal(err2, err)


def test_sba_quirks_and_edges(ctx, oracle, vo):
    # rotated (unrectified) stereo rig + different right intrinsics: calc_Qij_t_Qij_weight's zero entries matter
    w = np.array([0.02, -0.015, 0.01])
    th = np.linalg.norm(w)
    k = w / th
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    T_lr = np.eye(4)
    T_lr[:3, :3] = np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * Kx @ Kx
    T_lr[:3, 3] = [0.537, 0.004, -0.003]
    p = S.ba_window(n_kf=6, n_points=400, stereo=True, seed=2, T_lr=T_lr)
    _run(ctx, oracle, p)
    # the same rig with two different cameras (fx != fy in both): right observations projected with K_r, which the
    # solver is given as well — K_l read for K_r, or fx for fy, leaves several pixels of error and fails both checks
    p = S.ba_window(n_kf=6, n_points=400, stereo=True, seed=2, T_lr=T_lr, K=RIG_KITTI["K_l"], Kr=RIG_KITTI["K_r"])
    assert not np.array_equal(p["Kr"], p["K"])
    ok, T, X, err = _run(ctx, oracle, p, label="rotated rig, K_r != K_l")
    assert ok and sba_converged(err)
    # landmarks seen only in the right image of some keyframes (skipped by the Schur loops)
    p = S.ba_window(n_kf=6, n_points=400, stereo=True, seed=3, right_only_frac=0.3)
    _run(ctx, oracle, p)
    # observation lists in reverse keyframe order: blocks accumulate below the diagonal and are overwritten
    p = S.ba_window(n_kf=6, n_points=300, stereo=False, seed=4)
    q = dict(p)
    for name in ("obs_frame", "obs_right", "obs_px"):
        q[name] = p[name].copy()
    for i in range(0, p["X"].shape[0], 2):
        a, b = p["obs_ptr"][i], p["obs_ptr"][i + 1]
        for name in ("obs_frame", "obs_right", "obs_px"):
            q[name][a:b] = p[name][a:b][::-1]
    _run(ctx, oracle, q)
    # every pose fixed: structure-only refinement, empty reduced system
    r = dict(p)
    r["opt_index"] = np.full_like(p["opt_index"], -1)
    ok, T, X, err = _run(ctx, oracle, r)
    assert np.array_equal(T, p["T_jw"])
    # one iteration, zero iterations
    _run(ctx, oracle, p, iters=1)
    sol = SparseBundleAdjustmentSolver(ctx, False)
    sol.setCamera(p["K"])
    sol.setHuberThreshold(0.5)
    ok, T, X, err = sol.solveForFiniteIterations(0, p["T_jw"], p["opt_index"], p["X"], p["obs_ptr"], p["obs_frame"],
                                                 p["obs_right"], p["obs_px"])
    assert ok and np.array_equal(T, p["T_jw"]) and np.array_equal(X, p["X"])
    # malformed lists are rejected on the host
    bad = p["obs_frame"].copy()
    bad[5] = 99
    with pytest.raises(vo.VoError):
        sol.solveForFiniteIterations(2, p["T_jw"], p["opt_index"], p["X"], p["obs_ptr"], bad, p["obs_right"], p["obs_px"])
    with pytest.raises(vo.VoError):
        SparseBundleAdjustmentSolver(ctx, True).setCamera(p["K"])
    # a landmark behind a camera makes the solve go NaN-free but wild; a NaN input must raise as the reference throws
    Xn = p["X"].copy()
    Xn[3] = np.nan
    with pytest.raises(vo.VoError):
        sol.solveForFiniteIterations(2, p["T_jw"], p["opt_index"], Xn, p["obs_ptr"], p["obs_frame"], p["obs_right"],
                                     p["obs_px"])
