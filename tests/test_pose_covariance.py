"""CPU suite of the pose covariance: the yardstick's Jacobians against finite differences, the two host mirrors
(propagate_pose_covariance, pose_covariance_ros) against numerical linearisations of what they claim, and the new kernel's
resources."""
import os

import numpy as np
import pytest

import pose_covariance_restatement as PR
from visual_odometry_ros_amd import build as B


def _fd_rows(d, T10, right, h=1e-6):
    """Central differences of the projection (left or right camera) under T10 <- exp(delta) T10: (n, 2, 6)."""
    K = (d["Kr"] if right else d["Kl"]).astype(np.float64)
    T_rl = PR.inv_se3(d["T_lr"].astype(np.float64))
    X = d["X"].astype(np.float64)

    def proj(T):
        Xc = X @ T[:3, :3].T + T[:3, 3]
        if right:
            Xc = Xc @ T_rl[:3, :3].T + T_rl[:3, 3]
        return PR.project(K, Xc)

    J = np.zeros((X.shape[0], 2, 6))
    for k in range(6):
        e = np.zeros(6)
        e[k] = h
        J[:, :, k] = (proj(PR.se3_exp(e) @ T10) - proj(PR.se3_exp(-e) @ T10)) / (2 * h)
    return J


def _jacobian_case(rotated=False):
    kw = {}
    if rotated:
        T_lr = (PR.stereo_T_lr().astype(np.float64) @ PR.se3_exp([0, 0, 0, 0.004, -0.006, 0.003])).astype(np.float32)
        kw = dict(T_lr=T_lr, Kr=np.array([700.0, 705.0, 600.0, 180.0], np.float32))
    d = PR.two_view(40, np.random.default_rng(0), 0.3, **kw)
    T10 = PR.se3_exp(PR.XI_TRUE * 0.9)
    _, J = PR.rows(d["X"], d["pts_l"], d["pts_r"], d["Kl"], d["Kr"], d["T_lr"], T10)
    return d, T10, J


def test_restatement_jacobians_left_rows_equal_finite_differences():
    """The yardstick, not the feature: the left camera's rows, all six columns, relative 1e-6 (of the row's largest entry) at
    step 1e-6."""
    d, T10, J = _jacobian_case()
    Jl, fd = J[:, :2], _fd_rows(d, T10, right=False)
    err = np.abs(Jl - fd).max(2) / np.abs(fd).max(2)
    print("left rows: max relative difference", err.max())
    assert err.max() <= 1e-6


@pytest.mark.parametrize("rotated", [False, True], ids=["rectified", "rotated"])
def test_restatement_jacobians_right_rows_equal_finite_differences(rotated):
    """The right camera's rows, all six columns, relative 1e-6 at step 1e-6: a rectified rig (T_lr a pure baseline) and, beyond
    that, a rotated rig with unequal cameras. The rows are the derivative of the right projection under T10 <- exp(delta) T10.
    (The reference's own right rows — the left-frame formula evaluated at Xr — are not: with Xr = Xl + t_rl their rotation columns
    hold xr where the derivative has xl, and they miss this bound by 4.7e-2 (x rows) and 8.4e-2 (y rows) on the rectified case.)"""
    d, T10, J = _jacobian_case(rotated)
    Jr, fd = J[:, 2:], _fd_rows(d, T10, right=True)
    err = np.abs(Jr - fd).max(2) / np.abs(fd).max(2)
    print("right rows: max relative difference, x rows", err[:, 0].max(), "y rows", err[:, 1].max())
    assert err.max() <= 1e-6
    if not rotated:  # where R_rl = I the translation columns and column 3 are the reference's own right rows
        ref = PR._jac(d["Kr"].astype(np.float64), _right_points(d, T10))
        assert np.abs(Jr[:, :, :4] - ref[:, :, :4]).max() <= 1e-12 * np.abs(ref[:, :, :4]).max()  # (up to the order of operations)


def _right_points(d, T10):
    T_rl = PR.inv_se3(d["T_lr"].astype(np.float64))
    Xl = d["X"].astype(np.float64) @ T10[:3, :3].T + T10[:3, 3]
    return Xl @ T_rl[:3, :3].T + T_rl[:3, 3]


def _chain_case(seed):
    rng = np.random.default_rng(seed)
    T_prev = PR.se3_exp(rng.normal(0, 1, 6) * [3, 1, 5, 0.2, 0.4, 0.1])
    T01 = PR.se3_exp([0.03, -0.05, 0.9, 0.01, -0.03, 0.004])
    A = rng.normal(0, 1, (6, 6))
    B = rng.normal(0, 1, (6, 6))
    scale = np.diag([1e-2, 1e-2, 3e-2, 1e-3, 1e-3, 2e-3])
    return T_prev, T01, scale @ A @ A.T @ scale, 0.1 * scale @ B @ B.T @ scale


@pytest.mark.parametrize("seed", [0, 1])
def test_propagate_pose_covariance_is_the_linearised_chain(vo, seed):
    """e_k = -log(T_wc_est^-1 T_wc_true) with T_wc_true,k-1 = T_wc_est,k-1 exp(-e_k-1) and T10_true = exp(eps) T10_est, linearised
    numerically (central differences, 1e-6): P_k = Je P Je^T + Jeps Sigma Jeps^T against propagate_pose_covariance, 1e-4."""
    T_prev, T01, P, Sigma = _chain_case(seed)
    T10 = PR.inv_se3(T01)
    T_est = T_prev @ T01

    def e_k(e_prev, eps):
        T_true = T_prev @ PR.se3_exp(-e_prev) @ PR.inv_se3(PR.se3_exp(eps) @ T10)
        return -PR.se3_log(PR.inv_se3(T_est) @ T_true)

    h, z = 1e-6, np.zeros(6)
    Je, Jeps = np.zeros((6, 6)), np.zeros((6, 6))
    for k in range(6):
        d = np.zeros(6)
        d[k] = h
        Je[:, k] = (e_k(d, z) - e_k(-d, z)) / (2 * h)
        Jeps[:, k] = (e_k(z, d) - e_k(z, -d)) / (2 * h)
    want = Je @ P @ Je.T + Jeps @ Sigma @ Jeps.T
    got = vo.propagate_pose_covariance(P, T10, Sigma)
    assert np.abs(got - want).max() <= 1e-4 * np.abs(want).max()
    assert np.array_equal(got, got.T) and (np.diag(got) >= 0).all()
    carried = vo.propagate_pose_covariance(P, T10, None)
    assert np.abs(carried - Je @ P @ Je.T).max() <= 1e-4 * np.abs(want).max()
    assert np.abs(vo.se3_adjoint(T10) - PR.adjoint(T10)).max() == 0


@pytest.mark.parametrize("seed", [0, 1])
def test_pose_covariance_ros_is_position_and_world_axis_rotation(vo, seed):
    """T_wc_true = T_wc_est exp(-e): the position error and the world-axis rotation error (log of R_true R_est^T), linearised
    numerically in e, give C = G P G^T; pose_covariance_ros must return it (1e-4: central differences at 1e-6), symmetric, with
    a non-negative diagonal, 36 doubles in the order (x, y, z, rot x, rot y, rot z)."""
    T_prev, T01, P, _ = _chain_case(seed)
    T_wc = T_prev @ T01

    def world_error(e):
        T_true = T_wc @ PR.se3_exp(-e)
        Rd = np.eye(4)
        Rd[:3, :3] = T_true[:3, :3] @ T_wc[:3, :3].T
        return np.concatenate([T_true[:3, 3] - T_wc[:3, 3], PR.se3_log(Rd)[3:]])

    h, G = 1e-6, np.zeros((6, 6))
    for k in range(6):
        d = np.zeros(6)
        d[k] = h
        G[:, k] = (world_error(d) - world_error(-d)) / (2 * h)
    want = G @ P @ G.T
    got = vo.pose_covariance_ros(P, T_wc)
    assert got.shape == (36,) and got.dtype == np.float64
    C = got.reshape(6, 6)
    assert np.abs(C - want).max() <= 1e-4 * np.abs(want).max()
    assert np.array_equal(C, C.T) and (np.diag(C) >= 0).all()


def test_restatement_information_is_what_it_says():
    """H, s2 and Sigma of the restatement on a small stereo and mono set: loops over points and rows, written out."""
    d = PR.two_view(7, np.random.default_rng(2), 0.3, outlier_frac=0.3)
    T01 = PR.inv_se3(PR.se3_exp(PR.XI_TRUE)).astype(np.float32)
    for pr in (d["pts_r"], None):
        o = PR.information(d["X"], d["pts_l"], pr, d["Kl"], d["Kr"], d["T_lr"], T01)
        r, J = PR.rows(d["X"], d["pts_l"], pr, d["Kl"], d["Kr"], d["T_lr"], PR.inv_se3(T01.astype(np.float64)))
        H, swr, sw = np.zeros((6, 6)), 0.0, 0.0
        for i in range(7):
            a = np.abs(r[i]).sum() * (0.5 if pr is not None else 1.0)
            w = 1.0 if a < 0.5 else 0.5 / a
            for q in range(r.shape[1]):
                H += w * np.outer(J[i, q], J[i, q])
            swr += w * (r[i] ** 2).sum()
            sw += w
        s2 = swr / (r.shape[1] * sw - 6)
        assert o["valid"] and np.allclose(o["H"], H, rtol=1e-13) and np.isclose(o["s2"], s2, rtol=1e-13)
        assert np.allclose(o["Sigma"] @ H, s2 * np.eye(6), atol=1e-9 * s2)
        assert (o["a"] >= 0.5).any() and (o["a"] < 0.5).any()  # both Huber branches


@pytest.mark.skipif(not os.path.exists(B.HIPCC), reason="no hipcc")
def test_pose_covariance_kernel_resources():
    """No scratch, no spills, and the placement rule of tests/test_kernel_resources.py for a kernel that runs while a replay
    pool may be resident: (lanes / 256) x VGPRs (in units of 8) <= 236. 256 lanes."""
    from test_kernel_resources import _usage
    res = _usage("pose_covariance.hip")
    hit = {n: v for n, v in res.items() if "pose_cov_kernel" in n}
    assert len(hit) == 2, sorted(res)  # stereo and mono
    for n, v in hit.items():
        assert v["ScratchSize [bytes/lane]"] == 0 and v["VGPRs Spill"] == 0, (n, v)
        assert (256 // 256) * ((v["VGPRs"] + 7) // 8 * 8) <= 236, (n, v)
