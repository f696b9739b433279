"""The propagation of a keyframe's semi-dense map to the next keyframe (include/vo_hip.h, "Semi-dense propagation"),
restated in numpy from the definition and independent of the kernels: sources as arrays, every float operation a float32 numpy
operation of its own in the order the header states, the occlusion winner by a sort over (target, invd_b, source index) — no key
word, no atomic."""
import numpy as np

DEFAULTS = dict(min_obs=1, max_diff=30, chi=3.0, sigma_add=0.01)
F = np.float32
FRONT, FMAX = F(0.1), np.finfo(np.float32).max
ORIGIN = {0: "nothing", 1: "static only", 2: "propagated only", 3: "fused", 4: "static replaces an inconsistent propagated value"}


def _warp(idx, invd, sigma, W, K, T_ba, sigma_add):
    """the sources idx (raster indices) in the new camera: ok, invd_b, sigma_b, p_x, p_y"""
    fx, fy, cx, cy = (F(v) for v in K)
    T = np.asarray(T_ba, F).reshape(4, 4)
    R, t = T[:3, :3], T[:3, 3]
    x, y = (idx % W).astype(F), (idx // W).astype(F)
    r, sg = invd[idx], sigma[idx]
    with np.errstate(all="ignore"):
        xc, yc = x - cx, y - cy
        u, v = xc / fx, yc / fy
        a0, a1, a2 = ((R[i, 0] * u + R[i, 1] * v) + R[i, 2] for i in range(3))
        D = a2 + r * t[2]
        ok = D > FRONT
        invd_b = r / D
        px = fx * ((a0 + r * t[0]) / D) + cx
        py = fy * ((a1 + r * t[1]) / D) + cy
        sw = (sg * np.abs(a2)) / (D * D)
        sa = F(sigma_add)
        sigma_b = np.sqrt(sw * sw + sa * sa)
        ok = ok & (invd_b > 0) & (invd_b <= FMAX) & (sigma_b > 0) & (sigma_b <= FMAX)
    return ok, invd_b.astype(F), sigma_b.astype(F), px.astype(F), py.astype(F)


def _pix(p):
    with np.errstate(all="ignore"):
        t = np.floor(p + F(0.5))
        ok = (t >= F(-1048576)) & (t <= F(4194304))
    return np.where(ok, t, F(-1048576)).astype(np.int64)


def propagate(m, La, Lb, stat, bf, K, T_ba, mask=None, **params):
    """the old map m (dict invd, sigma, n_obs; not modified) of the key plane La -> the new keyframe's map: dict(invd, sigma, n_obs,
    tstatus, origin, src) and counts = dict(sources, kept, collisions, ties). stat: dict(disparity, sigma_invd, status) of the
    new pair; mask: the new keyframe's ignore mask (0 = ignore) or None."""
    p = dict(DEFAULTS, **params)
    H, W = La.shape
    n = H * W
    invd, sigma, n_obs = (np.ascontiguousarray(m[k]).reshape(-1) for k in ("invd", "sigma", "n_obs"))
    idx = np.nonzero((n_obs.astype(np.int64) >= p["min_obs"]) & (sigma > 0) & (invd > 0))[0]
    ok, invd_b, sigma_b, px, py = _warp(idx, invd, sigma, W, K, T_ba, p["sigma_add"])
    X, Y = _pix(px), _pix(py)
    ok &= (X >= 1) & (X <= W - 2) & (Y >= 1) & (Y <= H - 2)
    Xc, Yc = np.clip(X, 0, W - 1), np.clip(Y, 0, H - 1)
    if mask is not None:
        ok &= mask[Yc, Xc] != 0
    ok &= np.abs(La.reshape(-1)[idx].astype(np.int64) - Lb[Yc, Xc].astype(np.int64)) <= p["max_diff"]
    counts = dict(sources=int(len(idx)), kept=int(ok.sum()))
    idx, invd_b, sigma_b, tgt = idx[ok], invd_b[ok], sigma_b[ok], (Yc * W + Xc)[ok]
    # occlusion: per target the largest invd_b, then the smallest source index
    order = np.lexsort((idx, -invd_b.astype(np.float64), tgt))
    idx, invd_b, sigma_b, tgt = idx[order], invd_b[order], sigma_b[order], tgt[order]
    first = np.ones(len(tgt), bool)
    first[1:] = tgt[1:] != tgt[:-1]
    group = np.cumsum(first) - 1
    counts["collisions"] = int(len(tgt) - first.sum())
    counts["ties"] = int((~first & (invd_b == invd_b[first][group])).sum()) if len(tgt) else 0
    win = np.full(n, -1, np.int64)
    w_invd, w_sig, w_no = np.zeros(n, F), np.zeros(n, F), np.zeros(n, np.int64)
    win[tgt[first]] = idx[first]
    w_invd[tgt[first]], w_sig[tgt[first]], w_no[tgt[first]] = invd_b[first], sigma_b[first], n_obs[idx[first]]
    has = win >= 0
    # resolve
    s_ok = stat["status"].reshape(-1) == 1
    with np.errstate(all="ignore"):
        rho_s = stat["disparity"].reshape(-1).astype(F) / F(bf)
        sig_s = stat["sigma_invd"].reshape(-1).astype(F)
        dd = w_invd - rho_s
        s2, m2 = w_sig * w_sig, sig_s * sig_s
        sm = s2 + m2
        chi = F(p["chi"])
        cons = (sm > 0) & (dd * dd <= (chi * chi) * sm)
        f_invd = (w_invd * m2 + rho_s * s2) / sm
        f_sig = np.sqrt((s2 * m2) / sm)
    origin = np.zeros(n, np.uint8)
    origin[s_ok & ~has] = 1
    origin[~s_ok & has] = 2
    origin[s_ok & has & cons] = 3
    origin[s_ok & has & ~cons] = 4
    static = (origin == 1) | (origin == 4)
    out_invd = np.where(static, rho_s, np.where(origin == 2, w_invd, np.where(origin == 3, f_invd, F(0)))).astype(F)
    out_sig = np.where(static, sig_s, np.where(origin == 2, w_sig, np.where(origin == 3, f_sig, F(0)))).astype(F)
    out_no = np.where(static, 1, np.where(origin == 2, w_no, np.where(origin == 3, np.minimum(w_no + 1, 255), 0))).astype(np.uint8)
    return dict(invd=out_invd.reshape(H, W), sigma=out_sig.reshape(H, W), n_obs=out_no.reshape(H, W), tstatus=np.zeros((H, W), np.uint8),
                origin=origin.reshape(H, W), src=win.astype(np.int32).reshape(H, W), counts=counts)
