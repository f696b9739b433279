"""The direct image alignment on the semi-dense map (include/vo_hip.h, "Semi-dense alignment"), restated in numpy
from the definition and independent of the kernel: the map's pixels as arrays, every float operation a float32 numpy operation of
its own in the order the header states, the Jacobian entries, weights and residuals as integers, the sums exact per block of 1024
raster indices, the blocks added in float64 in block order, the solve and the pose update scalar by scalar."""
import math

import numpy as np

from semidense_temporal_restatement import _in, _q, _sample

DEFAULTS = dict(min_obs=1, huber=10.0, max_iters=10, eps=1e-4, min_pixels=100)
F, D = np.float32, np.float64
BLOCK = 1024
FRONT = F(0.1)
QMAX = F(4194304.0)  # 2^22
PIVOT = D(2.0 ** -20)
STATUS = {0: "converged", 1: "max_iters reached", 2: "too few pixels", 3: "singular system", 4: "no result (keyframe frame)"}
PAIRS = [(i, j) for i in range(6) for j in range(i, 6)]  # the 21 entries of H, row by row


def se3_exp(xi):
    """geometry::se3Exp_f as the pose-only BA's kernel evaluates it (float32; the coefficients through float64, by the Taylor
    series below 0.25 rad)"""
    xi = np.asarray(xi, F)
    v, w = xi[:3], xi[3:]
    theta = np.sqrt((w[0] * w[0] + w[1] * w[1]) + w[2] * w[2])
    z = F(0)
    wx = np.array([z, -w[2], w[1], w[2], z, -w[0], -w[1], w[0], z], F)
    wx2 = np.zeros(9, F)
    for i in range(3):
        for j in range(3):
            s = F(0)
            for k in range(3):
                s = s + wx[i * 3 + k] * wx[k * 3 + j]
            wx2[i * 3 + j] = s
    if D(theta) < 1e-7:
        a, b, c = F(1), F(0.5), F(0.33333333333333333333333333)
    else:
        th = D(theta)
        if th < 0.25:
            t2 = th * th
            sn = th * (D(1) + t2 * (D(-1.0 / 6) + t2 * (D(1.0 / 120) + t2 * (D(-1.0 / 5040) + t2 * (D(1.0 / 362880) + t2 * (
                D(-1.0 / 39916800) + t2 * D(1.0 / 6227020800.0)))))))
            cs1 = t2 * (D(0.5) + t2 * (D(-1.0 / 24) + t2 * (D(1.0 / 720) + t2 * (D(-1.0 / 40320) + t2 * (D(1.0 / 3628800) + t2 * D(
                -1.0 / 479001600.0))))))
        else:
            sn, cs1 = D(math.sin(th)), D(1) - D(math.cos(th))
        a = F(sn / th)
        b = F(cs1 / D(theta * theta))
        c = F((th - sn) / D(theta * theta * theta))
    T = np.zeros((4, 4), F)
    V = np.zeros(9, F)
    for i in range(9):
        I = F(1 if i in (0, 4, 8) else 0)
        T[i // 3, i % 3] = (I + a * wx[i]) + b * wx2[i]
        V[i] = (I + b * wx[i]) + c * wx2[i]
    for i in range(3):
        T[i, 3] = (V[i * 3] * v[0] + V[i * 3 + 1] * v[1]) + V[i * 3 + 2] * v[2]
    T[3, 3] = 1
    return T


def mul44(A, B):
    out = np.zeros((4, 4), F)
    for i in range(4):
        for j in range(4):
            r = A[i, 0] * B[0, j]
            for k in range(1, 4):
                r = A[i, k] * B[k, j] + r
            out[i, j] = r
    return out


def constants(key, m, K, min_obs=1):
    """the pixel set and its per-pixel constants: dict(idx raster indices (ascending), xs, ys, q [n, 6] int64, X, Y, Z float32)"""
    fx, fy, cx, cy = (F(v) for v in K)
    Lk = key.astype(np.int64)
    H, W = Lk.shape
    sel = (m["n_obs"] >= min_obs) & (m["sigma"] > 0) & (m["invd"] > 0)
    sel[0, :] = sel[-1, :] = False
    sel[:, 0] = sel[:, -1] = False
    ys, xs = np.nonzero(sel)
    gx = (Lk[ys, xs + 1] - Lk[ys, xs - 1]).astype(F)
    gy = (Lk[ys + 1, xs] - Lk[ys - 1, xs]).astype(F)
    with np.errstate(all="ignore"):
        invd = m["invd"][ys, xs].astype(F)
        Z = F(1) / invd
        u, v = (xs.astype(F) - cx) / fx, (ys.astype(F) - cy) / fy
        X, Y = u * Z, v * Z
        fu, fv = fx * u, fy * v
        zero = np.zeros(len(ys), F)
        Ju = [fx * invd + zero, zero, -(fu * invd), -(fu * v), fx + fu * u, -(fx * v)]
        Jv = [zero, fy * invd + zero, -(fv * invd), -(fy + fv * v), fv * u, fy * u]
        J16 = np.stack([F(16) * (F(0.5) * (gx * Ju[i] + gy * Jv[i])) for i in range(6)], 1).reshape(-1, 6)
        ok = (np.isfinite(J16) & (np.abs(J16) < QMAX)).all(1) & np.isfinite(X) & np.isfinite(Y) & np.isfinite(Z)
        q = np.where(ok[:, None], np.floor(J16 + F(0.5)), 0).astype(np.int64)
    k = np.nonzero(ok)[0]
    return dict(idx=(ys * W + xs)[k], xs=xs[k], ys=ys[k], q=q[k], X=X[k], Y=Y[k], Z=Z[k], key16=16 * Lk[ys[k], xs[k]], n_blocks=(H * W + BLOCK - 1) // BLOCK)


def residuals(c, cur, K, T, huber):
    """one iteration's per-pixel terms at the pose T: valid, r, w (int64)"""
    fx, fy, cx, cy = (F(v) for v in K)
    T = np.asarray(T, F).reshape(4, 4)
    Lc = cur.astype(np.int64)
    H, W = Lc.shape
    X, Y, Z = c["X"], c["Y"], c["Z"]
    with np.errstate(all="ignore"):
        Xc, Yc, Zc = (((T[i, 0] * X + T[i, 1] * Y) + T[i, 2] * Z) + T[i, 3] for i in range(3))
        front = Zc > FRONT
        px, py = fx * (Xc / Zc) + cx, fy * (Yc / Zc) + cy
        QX, QY = _q(px.astype(F)), _q(py.astype(F))
    valid = front & _in(QX, QY, W, H)
    r = _sample(Lc, QX, QY) - c["key16"]
    kq = int(np.floor(F(16) * F(huber) + F(0.5)))
    ar = np.abs(r)
    w = np.where(ar <= kq, 256, (256 * kq) // np.maximum(ar, 1))
    return valid, np.where(valid, r, 0), np.where(valid, w, 0)


def block_sums(c, valid, r, w, order=None):
    """the 30 integer sums per block [n_blocks, 30] int64: 21 H, 6 b, sum w r^2, sum w, count. order: a permutation of the pixels
    (the sums do not depend on it)"""
    q = c["q"]
    terms = np.stack([w * q[:, i] * q[:, j] for i, j in PAIRS] + [w * q[:, i] * r for i in range(6)] + [w * r * r, w, valid.astype(np.int64)], 1)
    terms = terms.reshape(-1, 30)
    blk = c["idx"] // BLOCK
    if order is not None:
        terms, blk = terms[order], blk[order]
    out = np.zeros((c["n_blocks"], 30), np.int64)
    np.add.at(out, blk, terms)
    return out


def reduce_blocks(bs):
    """the blocks' sums converted to float64 and added in block order, block 0 first; then the exact scales"""
    s = np.zeros(30, D)
    for b in range(bs.shape[0]):
        s = s + bs[b].astype(D)
    Hs = s[:21] * D(2.0 ** -16)
    bv = s[21:27] * D(2.0 ** -16)
    return Hs, bv, s[27], s[28], int(bs[:, 29].sum())


def solve(Hs, bv):
    """LDL^T in float64 in the header's order: (ok, xi)"""
    A = np.zeros((6, 6), D)
    for n, (i, j) in enumerate(PAIRS):
        A[i, j] = A[j, i] = Hs[n]
    L, Dg = np.zeros((6, 6), D), np.zeros(6, D)
    with np.errstate(all="ignore"):
        for j in range(6):
            d = A[j, j]
            for k in range(j):
                d = d - (L[j, k] * L[j, k]) * Dg[k]
            if not (d > 0) or not (d > A[j, j] * PIVOT) or not np.isfinite(d):
                return False, np.zeros(6, D)
            Dg[j] = d
            for i in range(j + 1, 6):
                s = A[i, j]
                for k in range(j):
                    s = s - (L[i, k] * L[j, k]) * Dg[k]
                L[i, j] = s / d
        y = np.zeros(6, D)
        for i in range(6):
            s = bv[i]
            for k in range(i):
                s = s - L[i, k] * y[k]
            y[i] = s
        x = np.zeros(6, D)
        for i in range(5, -1, -1):
            s = y[i] / Dg[i]
            for k in range(i + 1, 6):
                s = s - L[k, i] * x[k]
            x[i] = s
    if not np.isfinite(x).all():
        return False, np.zeros(6, D)
    return True, x


def align(key, cur, K, T_ck, m, **params):
    """the operator: dict(T_ck [4, 4] float32, status, iters, count, rms, H [21], b [6] float64)"""
    p = dict(DEFAULTS, **params)
    c = constants(key, m, K, p["min_obs"])
    T = np.asarray(T_ck, F).reshape(4, 4).copy()
    T[3] = (0, 0, 0, 1)
    out = dict(status=1, iters=0, count=0, rms=0.0, H=np.zeros(21, D), b=np.zeros(6, D))
    for it in range(p["max_iters"]):
        valid, r, w = residuals(c, cur, K, T, p["huber"])
        Hs, bv, swrr, sw, count = reduce_blocks(block_sums(c, valid, r, w))
        out.update(iters=it + 1, count=count, H=Hs, b=bv, rms=float(np.sqrt(swrr / sw) / D(16)) if sw > 0 else 0.0)
        if count < p["min_pixels"]:
            out["status"] = 2
            break
        ok, xi = solve(Hs, bv)
        if not ok:
            out["status"] = 3
            break
        nrm2 = ((((xi[0] * xi[0] + xi[1] * xi[1]) + xi[2] * xi[2]) + xi[3] * xi[3]) + xi[4] * xi[4]) + xi[5] * xi[5]
        T = mul44(T, se3_exp(-xi.astype(F)))
        if nrm2 < D(F(p["eps"])) * D(F(p["eps"])):  # (the square of a float32 is exact in float64)
            out["status"] = 0
            break
    out["T_ck"] = T
    return out
