"""numpy float32 restatement of what MonoVO's steady-state debug image is drawn from (include/vo_hip.h: vo_mvo_set_debug_image;
csrc/mono_debug_device.hpp): membership, inverseSE3_f of the frame's pose and projectToPixel, every operation rounded to float
on its own (numpy evaluates one ufunc per operation: no contraction). Shared by tests/test_mono_debug_image.py (against the
header's text compiled by g++) and tests/test_mono_debug_image_gpu.py (against the driver)."""
import numpy as np

F = np.float32


def inverse_se3(T):
    """geometry::inverseSE3_f: R10 = R01^T, t10_i = ((-R10[i,0] t0) + (-R10[i,1] t1)) + (-R10[i,2] t2)."""
    T = np.asarray(T, F).reshape(4, 4)
    R = T[:3, :3].T.copy()
    t = T[:3, 3]
    out = np.eye(4, dtype=F)
    out[:3, :3] = R
    for i in range(3):
        out[i, 3] = F(F(F(-R[i, 0]) * t[0]) + F(F(-R[i, 1]) * t[1])) + F(F(-R[i, 2]) * t[2])
    return out


def transform(T, X):
    """((T[r,0] X0 + T[r,1] X1) + T[r,2] X2) + T[r,3] per row r, for (n, 3) points."""
    T, X = np.asarray(T, F), np.asarray(X, F).reshape(-1, 3)
    with np.errstate(all="ignore"):
        return np.stack([((T[r, 0] * X[:, 0] + T[r, 1] * X[:, 1]) + T[r, 2] * X[:, 2]) + T[r, 3] for r in range(3)], axis=1).astype(F)


def project(dT01, K, Xp):
    """pts1_proj_ba: projectToPixel(dR10 Xp + dt10), dT10 = inverseSE3_f(dT01)."""
    Xc = transform(inverse_se3(dT01), Xp)
    K = np.asarray(K, F)
    with np.errstate(all="ignore"):
        invz = F(1.0) / Xc[:, 2]
        u = (K[0] * Xc[:, 0]) * invz + K[2]
        v = (K[1] * Xc[:, 1]) * invz + K[3]
    return np.stack([u, v], axis=1).astype(F)


def members(stage, ba_ok):
    return (np.asarray(stage) >= 2) & (np.asarray(ba_ok) != 0)


def ba_sets(stage, ba_ok, pts1, Xp, dT01, K):
    """(pts1_ba, pts1_proj_ba), compacted in feature order."""
    m = members(stage, ba_ok)
    return np.asarray(pts1, F).reshape(-1, 2)[m], project(dT01, K, np.asarray(Xp, F).reshape(-1, 3)[m])


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)
