"""numpy float64 restatement of the pose covariance's definitions (include/vo_hip.h:
vo_gn_pose_information_stereo / _mono, vo_svo_set_pose_covariance), written from the reference's lines
core/visual_odometry/motion_estimator.cpp:976-981, :993-998 (stereo, left rows; :1009-1014, :1026-1031 are the right rows there,
see rows()) and :755-760, :784-789 (mono).
Everything is evaluated in float64 from the float32 inputs; the order of a twist is xi = [rho; phi] of se3Exp_f."""
import numpy as np


def hat(w):
    return np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])


def se3_exp(xi):
    xi = np.asarray(xi, np.float64)
    v, w = xi[:3], xi[3:]
    th = np.linalg.norm(w)
    W = hat(w)
    if th < 1e-9:
        a, b, c = 1.0 - th * th / 6, 0.5 - th * th / 24, 1.0 / 6 - th * th / 120
    else:
        a, b, c = np.sin(th) / th, (1 - np.cos(th)) / th ** 2, (th - np.sin(th)) / th ** 3
    T = np.eye(4)
    T[:3, :3] = np.eye(3) + a * W + b * W @ W
    T[:3, 3] = (np.eye(3) + b * W + c * W @ W) @ v
    return T


def se3_log(T):
    R, t = T[:3, :3], T[:3, 3]
    c = min(1.0, max(-1.0, (np.trace(R) - 1) / 2))
    th = np.arccos(c)
    A = 0.5 * (R - R.T)
    w = np.array([A[2, 1], A[0, 2], A[1, 0]])
    if th > 1e-9:
        w = w * th / np.sin(th)
    th = np.linalg.norm(w)
    W = hat(w)
    if th < 1e-9:
        b, c2 = 0.5, 1.0 / 6
    else:
        b, c2 = (1 - np.cos(th)) / th ** 2, (th - np.sin(th)) / th ** 3
    V = np.eye(3) + b * W + c2 * W @ W
    return np.concatenate([np.linalg.solve(V, t), w])


def inv_se3(T):
    T = np.asarray(T, np.float64).reshape(4, 4)
    Ti = np.eye(4)
    Ti[:3, :3] = T[:3, :3].T
    Ti[:3, 3] = -T[:3, :3].T @ T[:3, 3]
    return Ti


def project(K, X):
    return np.stack([K[0] * X[:, 0] / X[:, 2] + K[2], K[1] * X[:, 1] / X[:, 2] + K[3]], 1)


def _jac(K, X):
    """The reference's two rows at camera-frame points X: (n, 2, 6)."""
    f_x, f_y = K[0], K[1]
    iz = 1.0 / X[:, 2]
    xiz, yiz = X[:, 0] * iz, X[:, 1] * iz
    fxxiz, fyyiz = f_x * xiz, f_y * yiz
    z = np.zeros_like(iz)
    Jx = np.stack([f_x * iz, z, -fxxiz * iz, -fxxiz * yiz, f_x * (1.0 + xiz * xiz), -f_x * yiz], 1)
    Jy = np.stack([z, f_y * iz, -fyyiz * iz, -f_y * (1.0 + yiz * yiz), fyyiz * xiz, f_y * xiz], 1)
    return np.stack([Jx, Jy], 1)


def rows(X, pts_l, pts_r, Kl, Kr, T_lr, T10):
    """Residuals (n, rows) and Jacobian rows (n, rows, 6) at T10; pts_r None: mono (two rows), else four
    (left x, left y, right x, right y). The right camera's rows are the derivative of the right projection under
    T10 <- exp(delta) T10: Xr = R_rl Xl + t_rl moves as R_rl [I | -[Xl]x] delta. (The reference's own right rows, :1009-1014 and
    :1026-1031, put Xr into the rotation columns; that is not the derivative, not even for a rectified rig.)"""
    X = np.asarray(X, np.float32).astype(np.float64).reshape(-1, 3)
    pl = np.asarray(pts_l, np.float32).astype(np.float64).reshape(-1, 2)
    Kl = np.asarray(Kl, np.float32).astype(np.float64)
    T10 = np.asarray(T10, np.float64).reshape(4, 4)
    Xl = X @ T10[:3, :3].T + T10[:3, 3]
    r, J = project(Kl, Xl) - pl, _jac(Kl, Xl)
    if pts_r is None:
        return r, J
    pr = np.asarray(pts_r, np.float32).astype(np.float64).reshape(-1, 2)
    Kr = np.asarray(Kr, np.float32).astype(np.float64)
    T_rl = inv_se3(np.asarray(T_lr, np.float32).astype(np.float64))
    Xr = Xl @ T_rl[:3, :3].T + T_rl[:3, 3]
    iz = 1.0 / Xr[:, 2]
    z = np.zeros_like(iz)
    dp = np.stack([np.stack([Kr[0] * iz, z, -Kr[0] * Xr[:, 0] * iz * iz], 1),
                   np.stack([z, Kr[1] * iz, -Kr[1] * Xr[:, 1] * iz * iz], 1)], 1)   # d proj / d Xr: (n, 2, 3)
    a = dp @ T_rl[:3, :3]
    rot = np.cross(Xl[:, None, :], a)   # a (-[Xl]x) = Xl x a
    return np.concatenate([r, project(Kr, Xr) - pr], 1), np.concatenate([J, np.concatenate([a, rot], 2)], 1)


def huber_weight(r):
    """The estimator's own weight: a = 0.5 * sum |r| (stereo, four rows) or |rx| + |ry| (mono); w = 1 if a < 0.5 else 0.5 / a."""
    a = np.abs(r).sum(1) * (0.5 if r.shape[1] == 4 else 1.0)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(a < 0.5, 1.0, 0.5 / a), a


def information(X, pts_l, pts_r, Kl, Kr, T_lr, T01, sigma_px=0.0):
    """dict(H, s2, Sigma, valid, a): T10 = the SE(3) inverse of the float32 T01, taken in float64."""
    T10 = inv_se3(np.asarray(T01, np.float32).astype(np.float64))
    X = np.asarray(X, np.float32).reshape(-1, 3)
    n = X.shape[0]
    out = dict(H=np.zeros((6, 6)), s2=0.0, Sigma=np.zeros((6, 6)), valid=False, a=np.zeros(0))
    if n == 0:
        return out
    with np.errstate(all="ignore"):
        r, J = rows(X, pts_l, pts_r, Kl, Kr, T_lr, T10)
        w, a = huber_weight(r)
        H = np.einsum("n,nri,nrj->ij", w, J, J)
        den = r.shape[1] * w.sum() - 6.0
        s2 = (w * (r * r).sum(1)).sum() / den if den != 0 else np.inf
    out.update(H=H, a=a)
    if n < 3 or not den > 0 or not np.isfinite(H).all() or not np.isfinite(s2) or not np.isfinite(a).all():
        return out
    d = np.diag(H)
    if not (d > 0).all():
        return out
    S = 1.0 / np.sqrt(d)
    A = H * S[:, None] * S[None, :]
    try:
        L = np.linalg.cholesky(A)
    except np.linalg.LinAlgError:
        return out
    Li = np.linalg.inv(L)
    Hinv = (Li.T @ Li) * S[:, None] * S[None, :]
    scale = sigma_px ** 2 if sigma_px > 0 else s2
    out.update(s2=s2, Sigma=scale * Hinv, valid=True)
    return out


def adjoint(T):
    T = np.asarray(T, np.float64).reshape(4, 4)
    A = np.zeros((6, 6))
    A[:3, :3] = A[3:, 3:] = T[:3, :3]
    A[:3, 3:] = hat(T[:3, 3]) @ T[:3, :3]
    return A


# ---- the geometry of BASELINE configs[0], as the issue sets it for the operator tests ----
K0 = np.array([718.856, 718.856, 607.1928, 185.2157], np.float32)
BASELINE_M = 0.5371657189
XI_TRUE = np.array([0.05, -0.02, 0.8, 0.004, -0.01, 0.002])


def stereo_T_lr():
    T = np.eye(4, dtype=np.float32)
    T[0, 3] = BASELINE_M
    return T


def two_view(n, rng, noise_px, outlier_frac=0.0, outlier_px=20.0, T_lr=None, Kr=None):
    """n points X ~ U([-10,10] x [-4,4] x [4,40]) in the previous left camera's frame, their pixels in the current pair under
    the true motion T10 = exp(XI_TRUE), Gaussian pixel noise and a fraction of +-outlier_px outliers. float32 arrays."""
    T_lr = stereo_T_lr() if T_lr is None else np.asarray(T_lr, np.float32)
    Kr = K0 if Kr is None else np.asarray(Kr, np.float32)
    X = np.stack([rng.uniform(-10, 10, n), rng.uniform(-4, 4, n), rng.uniform(4, 40, n)], 1).astype(np.float32)
    T10 = se3_exp(XI_TRUE)
    Xl = X.astype(np.float64) @ T10[:3, :3].T + T10[:3, 3]
    T_rl = inv_se3(T_lr.astype(np.float64))
    Xr = Xl @ T_rl[:3, :3].T + T_rl[:3, 3]
    pl, pr = project(K0.astype(np.float64), Xl), project(Kr.astype(np.float64), Xr)
    pl = pl + rng.normal(0, noise_px, pl.shape)
    pr = pr + rng.normal(0, noise_px, pr.shape)
    n_out = int(round(outlier_frac * n))
    if n_out:
        idx = rng.choice(n, n_out, replace=False)
        pl[idx] += rng.choice([-outlier_px, outlier_px], (n_out, 2))
        pr[idx] += rng.choice([-outlier_px, outlier_px], (n_out, 2))
    return dict(X=X, pts_l=pl.astype(np.float32), pts_r=pr.astype(np.float32), Kl=K0, Kr=Kr, T_lr=T_lr, T10_true=T10)
