"""The temporal semi-dense search and its fusion (include/vo_hip.h, "Semi-dense temporal"), restated in numpy from
the definition and independent of the kernel: candidates as arrays, every float operation a float32 numpy operation of its own in
the order the header states, the sample values and the five sums as integers (no summation order enters)."""
import numpy as np

DEFAULTS = dict(hw=4, hh=1, g_min=20, thres_best=0.95, thres_peak=0.9, peak_px=5, edge_px=2, eps_edge=0.5, eps_epi=1.0,
                z_min=3.0, z_max=100.0, max_search=128, j_min=16.0, eps_scale=3.0)
F = np.float32
EPS_DK2, FRONT, OUTSIDE = F(1e-6), F(0.1), F(-3.0)
STATUS = {0: "no candidate", 1: "accepted", 2: "best score too low", 3: "second peak", 4: "best at the end of the run",
          5: "too few positions", 6: "range too long", 7: "no parallax", 8: "range or depth refused"}


def seed(disparity, sigma_invd, status, bf):
    """the map of a static result: dict(invd, sigma float32; n_obs, tstatus uint8)"""
    ok = status == 1
    with np.errstate(divide="ignore", invalid="ignore"):
        invd = np.where(ok, disparity.astype(F) / F(bf), F(0)).astype(F)
    return dict(invd=invd, sigma=np.where(ok, sigma_invd, F(0)).astype(F), n_obs=ok.astype(np.uint8), tstatus=np.zeros(status.shape, np.uint8))


def empty_map(shape):
    return dict(invd=np.zeros(shape, F), sigma=np.zeros(shape, F), n_obs=np.zeros(shape, np.uint8), tstatus=np.zeros(shape, np.uint8))


def _q(p):
    t = np.floor(F(32) * p + F(0.5))
    ok = (t >= F(-1048576)) & (t <= F(4194304))
    return np.where(ok, t, F(-1048576)).astype(np.int64)


def _in(X, Y, W, H):
    cx, cy = X >> 5, Y >> 5
    return (cx >= 0) & (cx <= W - 2) & (cy >= 0) & (cy <= H - 2)


def _sample(img, X, Y):
    H, W = img.shape
    cx, cy = np.clip(X >> 5, 0, W - 2), np.clip(Y >> 5, 0, H - 2)
    wx, wy = X & 31, Y & 31
    top = (32 - wx) * img[cy, cx] + wx * img[cy, cx + 1]
    bot = (32 - wx) * img[cy + 1, cx] + wx * img[cy + 1, cx + 1]
    return ((32 - wy) * top + wy * bot + 32) >> 6


def pose_parts(T_ck):
    T = np.asarray(T_ck, F).reshape(4, 4)
    R, t = T[:3, :3], T[:3, 3]
    C = np.array([-((R[0, i] * t[0] + R[1, i] * t[1]) + R[2, i] * t[2]) for i in range(3)], F)
    return R, t, C


def pose_ck(T_wc, T_wk):
    """T_ck = inverseSE3(T_wc) * T_wk as the driver forms it on the host, in float32 and in the header's order"""
    A, B = np.asarray(T_wc, F).reshape(4, 4), np.asarray(T_wk, F).reshape(4, 4)
    Ti = np.zeros((4, 4), F)
    Ti[:3, :3] = A[:3, :3].T
    for i in range(3):
        Ti[i, 3] = ((-Ti[i, 0]) * A[0, 3] + (-Ti[i, 1]) * A[1, 3]) + (-Ti[i, 2]) * A[2, 3]
    Ti[3, 3] = 1
    out = np.zeros((4, 4), F)
    for i in range(4):
        for j in range(4):
            r = Ti[i, 0] * B[0, j]
            for k in range(1, 4):
                r = Ti[i, k] * B[k, j] + r
            out[i, j] = r
    return out


def temporal(key, cur, K, T_ck, m, mask=None, chunk=20000, **params):
    """one launch: the map m (not modified) -> dict(invd, sigma, n_obs, tstatus, score)"""
    p = dict(DEFAULTS, **params)
    hw, hh, edge, peak, max_search = p["hw"], p["hh"], p["edge_px"], p["peak_px"], p["max_search"]
    width, n = 2 * hw + 1, (2 * hw + 1) * (2 * hh + 1)
    fx, fy, cx, cy = (F(v) for v in K)
    R, t, C = pose_parts(T_ck)
    r_min, r_max, j_min = F(1) / F(p["z_max"]), F(1) / F(p["z_min"]), F(p["j_min"])
    ee, ep, es, tb, tp = F(p["eps_edge"]), F(p["eps_epi"]), F(p["eps_scale"]), F(p["thres_best"]), F(p["thres_peak"])
    Lk, Lc = key.astype(np.int64), cur.astype(np.int64)
    H, W = Lk.shape
    out = dict(invd=m["invd"].copy(), sigma=m["sigma"].copy(), n_obs=m["n_obs"].copy(), tstatus=np.zeros((H, W), np.uint8),
               score=np.zeros((H, W), F))
    gx, gy = np.zeros_like(Lk), np.zeros_like(Lk)
    gx[:, 1:-1] = Lk[:, 2:] - Lk[:, :-2]
    gy[1:-1, :] = Lk[2:, :] - Lk[:-2, :]
    cand = np.zeros((H, W), bool)
    cand[1:H - 1, 1:W - 1] = True
    cand &= gx * gx + gy * gy >= p["g_min"] ** 2
    if mask is not None:
        cand &= mask != 0
    ys, xs = np.nonzero(cand)
    if not len(ys):
        return out
    gxa, gya = gx[ys, xs], gy[ys, xs]
    st = np.zeros(len(ys), np.int64)
    kk = np.tile(np.arange(-hw, hw + 1), 2 * hh + 1).astype(F)
    vv = np.repeat(np.arange(-hh, hh + 1), width).astype(F)
    with np.errstate(all="ignore"):
        xc, yc = xs.astype(F) - cx, ys.astype(F) - cy
        u, v = xc / fx, yc / fy
        a0, a1, a2 = ((R[i, 0] * u + R[i, 1] * v) + R[i, 2] for i in range(3))
        dkx, dky = fx * C[0] - xc * C[2], fy * C[1] - yc * C[2]
        dk2 = dkx * dkx + dky * dky
        epi = dk2 < EPS_DK2
        st[epi] = 7
        dot = gxa.astype(F) * dkx + gya.astype(F) * dky
        g2 = (gxa * gxa + gya * gya).astype(F)
        live = ~epi & ~((F(4) * dot) * dot < g2 * dk2)
        dkl = np.sqrt(dk2)
        ux, uy = dkx / dkl, dky / dkl
        # the key patch inside the image
        for i0 in range(0, len(ys), chunk):
            s = slice(i0, i0 + chunk)
            tx = (xs[s].astype(F)[:, None] + kk[None] * ux[s, None]) + vv[None] * (-uy[s])[:, None]
            ty = (ys[s].astype(F)[:, None] + kk[None] * uy[s, None]) + vv[None] * ux[s, None]
            live[s] &= _in(_q(tx), _q(ty), W, H).all(1)
        invd, sig = m["invd"][ys, xs], m["sigma"][ys, xs]
        prior = sig > 0
        two = F(2) * sig
        lo = np.where(prior, np.maximum(invd - two, r_min), r_min).astype(F)
        hi = np.where(prior, np.minimum(invd + two, r_max), r_max).astype(F)
        Dlo, Dhi = a2 + lo * t[2], a2 + hi * t[2]
        bad = live & (~(lo < hi) | ~((Dlo > FRONT) & (Dhi > FRONT)))
        st[bad] = 8
        live &= ~bad
        N0, N1 = a0 + lo * t[0], a1 + lo * t[1]
        P0x, P0y = fx * (N0 / Dlo) + cx, fy * (N1 / Dlo) + cy
        P1x, P1y = fx * ((a0 + hi * t[0]) / Dhi) + cx, fy * ((a1 + hi * t[1]) / Dhi) + cy
        ex, ey = P1x - P0x, P1y - P0y
        ln = np.sqrt(ex * ex + ey * ey)
        J = ln / (hi - lo)
        bad = live & ~(J >= j_min)
        st[bad] = 7
        live &= ~bad
        lx, ly = ex / ln, ey / ln
        tl = np.floor(ln + F(0.5))
        too_long = ~(tl <= F(max_search))
        npos = np.where(too_long | ~live, 0, tl).astype(np.int64) + 2 * edge + 3
        bad = live & (too_long | (npos > max_search))
        st[bad] = 6
        live &= ~bad
        bx, by = ux / fx, uy / fy
        b0, b1, b2 = (R[i, 0] * bx + R[i, 1] * by for i in range(3))
        wx, wy = fx * (b0 * Dlo - N0 * b2), fy * (b1 * Dlo - N1 * b2)
        pos = lx * wx + ly * wy >= 0
        dhx, dhy = np.where(pos, ux, -ux).astype(F), np.where(pos, uy, -uy).astype(F)
        j0 = -(edge + 1)
        Dp = a2 + invd * t[2]
        qx, qy = fx * ((a0 + invd * t[0]) / Dp) + cx, fy * ((a1 + invd * t[1]) / Dp) + cy
        tj = np.floor(((qx - P0x) * lx + (qy - P0y) * ly) + F(0.5))
        has_jp = prior & (Dp > FRONT) & (tj >= F(j0)) & (tj <= (j0 + npos - 1).astype(F))
        jp = np.where(has_jp, tj, j0 - 1).astype(np.int64) - j0  # (-1: none)
    out["tstatus"][ys, xs] = st.astype(np.uint8)
    idx = np.nonzero(live)[0]
    if not len(idx):
        return out
    # ---- the searched candidates: key patches, scores ----
    nc = len(idx)
    npos_s = npos[idx]
    maxpos = int(npos_s.max())
    S = np.full((nc, maxpos), OUTSIDE, F)
    A = np.zeros(nc, np.int64)
    keyp = np.zeros((nc, n), np.int64)
    with np.errstate(all="ignore"):
        for i0 in range(0, nc, chunk):
            ii = idx[i0:i0 + chunk]
            tx = (xs[ii].astype(F)[:, None] + kk[None] * dhx[ii, None]) + vv[None] * (-dhy[ii])[:, None]
            ty = (ys[ii].astype(F)[:, None] + kk[None] * dhy[ii, None]) + vv[None] * dhx[ii, None]
            keyp[i0:i0 + chunk] = _sample(Lk, _q(tx), _q(ty))
        Sk, Skk = keyp.sum(1), (keyp * keyp).sum(1)
        A = n * Skk - Sk * Sk
        item_c = np.repeat(np.arange(nc), npos_s)
        item_p = np.arange(len(item_c)) - np.repeat(np.cumsum(npos_s) - npos_s, npos_s)
        for i0 in range(0, len(item_c), chunk):
            c, pp = item_c[i0:i0 + chunk], item_p[i0:i0 + chunk]
            ii = idx[c]
            jf = (pp + j0).astype(F)
            pjx, pjy = P0x[ii] + jf * lx[ii], P0y[ii] + jf * ly[ii]
            X = _q((pjx[:, None] + kk[None] * lx[ii, None]) + vv[None] * (-ly[ii])[:, None])
            Y = _q((pjy[:, None] + kk[None] * ly[ii, None]) + vv[None] * lx[ii, None])
            ins = _in(X, Y, W, H).all(1)
            cv, kv = _sample(Lc, X, Y), keyp[c]
            Sc, Scc, Skc = cv.sum(1), (cv * cv).sum(1), (kv * cv).sum(1)
            B = n * Scc - Sc * Sc
            num = n * Skc - Sk[c] * Sc
            s = num.astype(F) / np.sqrt(A[c].astype(F) * B.astype(F))
            s = np.where((A[c] != 0) & (B != 0), s, F(-1)).astype(F)
            S[c, pp] = np.where(ins, s, OUTSIDE)
    out["counts"] = dict(candidates=int(len(ys)), searched=int(nc), positions=int(npos_s.sum()))  # (for the cost measurement)
    # ---- the decision ----
    ar = np.arange(nc)
    inside = S > F(-2.5)
    jps = jp[idx]
    at_prior = (jps >= 0) & inside[ar, np.maximum(jps, 0)]
    start = np.where(at_prior, jps, inside.argmax(1))
    brk = np.cumsum(~inside, 1)
    run = inside & (brk == brk[ar, start][:, None]) & inside.any(1)[:, None]
    r0, r1 = run.argmax(1), maxpos - 1 - run[:, ::-1].argmax(1)
    cnt = run.sum(1)
    Sm = np.where(run, S, F(-np.inf))
    best = Sm.argmax(1)
    best_s = Sm[ar, best]
    pk = run & (S > tp)
    lo_p, hi_p = pk.argmax(1), maxpos - 1 - pk[:, ::-1].argmax(1)
    st5 = (cnt < 2 * edge + 3) | (A == 0)
    rest = ~st5
    st2 = rest & (best_s <= tb)
    rest &= ~st2
    st3 = rest & pk.any(1) & ((lo_p < best - peak) | (hi_p > best + peak))
    rest &= ~st3
    st4 = rest & ~((r0 + edge < best) & (best < r1 - edge))
    rest &= ~st4
    sts = np.zeros(nc, np.int64)
    sts[st5], sts[st2], sts[st3], sts[st4] = 5, 2, 3, 4
    score = np.where(st5, F(0), best_s).astype(F)
    acc = np.nonzero(rest)[0]
    with np.errstate(all="ignore"):
        b = best[acc]
        ii = idx[acc]
        s0, sm, sp = S[acc, b], S[acc, np.maximum(b - 1, 0)], S[acc, np.minimum(b + 1, maxpos - 1)]
        den = (sm + sp) - (s0 + s0)
        off = np.where(den != 0, (F(0.5) * (sm - sp)) / den, F(0)).astype(F)
        js = (b + j0).astype(F) + off
        ux_ = ((P0x[ii] + js * lx[ii]) - cx) / fx
        uy_ = ((P0y[ii] + js * ly[ii]) - cy) / fy
        rx = (a0[ii] - ux_ * a2[ii]) / (ux_ * t[2] - t[0])
        ry = (a1[ii] - uy_ * a2[ii]) / (uy_ * t[2] - t[1])
        rho = np.where(np.abs(lx[ii]) >= np.abs(ly[ii]), rx, ry).astype(F)
        Ds = a2[ii] + rho * t[2]
        good = (rho >= r_min) & (rho <= r_max) & (Ds > FRONT)
        sts[acc] = np.where(good, 1, 8)
        g = np.sqrt(g2[ii])
        cs = dot[ii] / (g * np.sqrt(dk2[ii]))
        sn2 = np.maximum(F(1) - cs * cs, F(0))
        stretch = (es * F(hw)) * np.abs(F(1) - F(1) / Ds)
        sg_new = (np.sqrt((ee * ee + (ep * ep) * sn2) + stretch * stretch) / np.abs(cs)) / J[ii]
        # fusion
        s2, m2 = sig[ii] * sig[ii], sg_new * sg_new
        sm_ = s2 + m2
        f_invd = (invd[ii] * m2 + rho * s2) / sm_
        f_sig = np.sqrt((s2 * m2) / sm_)
        pr = prior[ii]
        new_invd = np.where(pr, f_invd, rho).astype(F)
        new_sig = np.where(pr, f_sig, sg_new).astype(F)
        no = m["n_obs"][ys[ii], xs[ii]].astype(np.int64)
        new_no = np.where(pr, np.minimum(no + 1, 255), 1).astype(np.uint8)
    a = acc[good]
    ia = idx[a]
    out["invd"][ys[ia], xs[ia]] = new_invd[good]
    out["sigma"][ys[ia], xs[ia]] = new_sig[good]
    out["n_obs"][ys[ia], xs[ia]] = new_no[good]
    out["meas_invd"], out["meas_sigma"] = np.zeros((H, W), F), np.zeros((H, W), F)  # (this launch's rho*, sigma*: not planes of the operator)
    out["meas_invd"][ys[ia], xs[ia]] = rho[good]
    out["meas_sigma"][ys[ia], xs[ia]] = sg_new[good].astype(F)
    out["tstatus"][ys[idx], xs[idx]] = sts.astype(np.uint8)
    out["score"][ys[idx], xs[idx]] = score
    return out


def map_points(invd, sigma, n_obs, K, T=None, min_obs=1):
    """the pixels with n_obs >= min_obs in raster order: xyz [n, 3] float32 (z = 1 / invd), sigma [n], pixel [n, 2] uint16"""
    fx, fy, cx, cy = (F(v) for v in K)
    ys, xs = np.nonzero(n_obs >= min_obs)
    with np.errstate(divide="ignore", invalid="ignore"):
        z = F(1) / invd[ys, xs]
        X = (xs.astype(F) - cx) / fx * z
        Y = (ys.astype(F) - cy) / fy * z
        if T is not None:
            T = np.asarray(T, F).reshape(4, 4)
            X, Y, z = ((T[r, 0] * X + (T[r, 1] * Y + T[r, 2] * z)) + T[r, 3] for r in range(3))
    xyz = np.stack([X, Y, z], 1).astype(F).reshape(-1, 3)
    return xyz, sigma[ys, xs].astype(F), np.stack([xs, ys], 1).astype(np.uint16).reshape(-1, 2)
