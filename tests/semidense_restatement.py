"""Semi-dense stereo depth (include/vo_hip.h, "Semi-dense stereo"), restated in numpy from the definition and
independent of the kernel: whole planes at a time, the five window sums by exact int64 box sums (all taps sit at integer pixels,
so the sums are integers and no summation order enters), every float operation a float32 numpy operation of its own."""
import math

import numpy as np

DEFAULTS = dict(hw=8, hh=1, d_min=0, d_max=64, g_min=20, thres_best=0.95, thres_peak=0.9, peak_px=5, edge_px=2, eps_edge=0.5,
                eps_epi=1.0, bf=1.0)
F = np.float32


def disparity_range(bf, z_min, z_max=math.inf):
    """(d_min, d_max) of a depth range [z_min, z_max] in metres: floor(bf / z_max), ceil(bf / z_min)"""
    return (0 if math.isinf(z_max) else int(math.floor(bf / z_max))), int(math.ceil(bf / z_min))


def _box(a, hw, hh):
    """sums of a (int64, H x W) over the (2hw+1) x (2hh+1) window centred at every pixel; 0 where the window leaves the plane"""
    H, W = a.shape
    c = np.zeros((H + 1, W + 1), np.int64)
    c[1:, 1:] = a.cumsum(0).cumsum(1)
    out = np.zeros((H, W), np.int64)
    if H < 2 * hh + 1 or W < 2 * hw + 1:
        return out
    y0, y1, x0, x1 = hh, H - hh, hw, W - hw
    out[y0:y1, x0:x1] = (c[2 * hh + 1:, 2 * hw + 1:] - c[:H - 2 * hh, 2 * hw + 1:] - c[2 * hh + 1:, :W - 2 * hw] + c[:H - 2 * hh, :W - 2 * hw])
    return out


def candidates(left, mask=None, **params):
    """the candidate plane (bool), gx, gy (int64 planes)"""
    p = dict(DEFAULTS, **params)
    L = left.astype(np.int64)
    H, W = L.shape
    gx = np.zeros_like(L)
    gy = np.zeros_like(L)
    gx[:, 1:-1] = L[:, 2:] - L[:, :-2]
    gy[1:-1, :] = L[2:, :] - L[:-2, :]
    mx, my = max(p["hw"], 1), max(p["hh"], 1)
    inside = np.zeros((H, W), bool)
    if W > 2 * mx and H > 2 * my:
        inside[my:H - my, mx:W - mx] = True
    cand = inside & (gx * gx + gy * gy >= p["g_min"] ** 2) & (3 * gx * gx >= gy * gy)
    if mask is not None:
        cand &= mask != 0
    return cand, gx, gy


def semidense(left, right, mask=None, **params):
    """dict(disparity, score, sigma_invd: float32 H x W; status: uint8 H x W) of the u8 planes left, right"""
    p = dict(DEFAULTS, **params)
    hw, hh, d_min, d_max, edge, peak = p["hw"], p["hh"], p["d_min"], p["d_max"], p["edge_px"], p["peak_px"]
    n = (2 * hw + 1) * (2 * hh + 1)
    L, R = left.astype(np.int64), right.astype(np.int64)
    H, W = L.shape
    cand, gx, gy = candidates(left, mask, **p)
    xs = np.arange(W)[None, :].repeat(H, 0)
    d_last = np.minimum(d_max, xs - hw)
    S_l, S_ll = _box(L, hw, hh), _box(L * L, hw, hh)
    Sr, Srr = _box(R, hw, hh), _box(R * R, hw, hh)
    A = n * S_ll - S_l * S_l
    D = d_max - d_min + 1
    s = np.full((D, H, W), -np.inf, F)
    for i, d in enumerate(range(d_min, d_max + 1)):
        if d >= W:
            break
        Rs = np.zeros_like(R)
        Rs[:, d:] = R[:, :W - d]
        S_lr = _box(L * Rs, hw, hh)
        S_r, S_rr = np.zeros_like(Sr), np.zeros_like(Srr)
        S_r[:, d:] = Sr[:, :W - d]
        S_rr[:, d:] = Srr[:, :W - d]
        B = n * S_rr - S_r * S_r
        num = n * S_lr - S_l * S_r
        ok = (A != 0) & (B != 0)
        with np.errstate(divide="ignore", invalid="ignore"):
            v = num.astype(F) / np.sqrt(A.astype(F) * B.astype(F))
        v = np.where(ok, v, F(-1.0)).astype(F)
        s[i] = np.where(cand & (d <= d_last), v, F(-np.inf))
    status = np.zeros((H, W), np.uint8)
    best = s.argmax(0)  # (the first maximum: the smallest d)
    d_best = best + d_min
    s0 = np.take_along_axis(s, best[None], 0)[0]
    pk = s > F(p["thres_peak"])
    any_pk = pk.any(0)
    lo = pk.argmax(0) + d_min
    hi = (D - 1 - pk[::-1].argmax(0)) + d_min
    st5 = cand & ((d_last - d_min + 1 < 2 * edge + 3) | (A == 0))
    rest = cand & ~st5
    st2 = rest & (s0 <= F(p["thres_best"]))
    rest &= ~st2
    st3 = rest & any_pk & ((lo < d_best - peak) | (hi > d_best + peak))
    rest &= ~st3
    st4 = rest & ~((d_min + edge < d_best) & (d_best < d_last - edge))
    rest &= ~st4
    status[st5], status[st2], status[st3], status[st4], status[rest] = 5, 2, 3, 4, 1
    score = np.where(cand & ~st5, s0, F(0)).astype(F)
    # accepted pixels
    disparity = np.zeros((H, W), F)
    sigma = np.zeros((H, W), F)
    ys_a, xs_a = np.nonzero(rest)
    if len(ys_a):
        b = best[ys_a, xs_a]
        c0, cm, cp = s[b, ys_a, xs_a], s[b - 1, ys_a, xs_a], s[b + 1, ys_a, xs_a]
        den = (cm + cp) - (c0 + c0)
        with np.errstate(divide="ignore", invalid="ignore"):
            off = np.where(den != 0, (F(0.5) * (cm - cp)) / den, F(0)).astype(F)
        disparity[ys_a, xs_a] = (b + d_min).astype(F) + off
        gxa, gya = gx[ys_a, xs_a], gy[ys_a, xs_a]
        g = np.sqrt((gxa * gxa + gya * gya).astype(F))
        du, dv = gxa.astype(F) / g, gya.astype(F) / g
        ee, ep = F(p["eps_edge"]), F(p["eps_epi"])
        sigma[ys_a, xs_a] = (np.sqrt(ee * ee + (ep * dv) * (ep * dv)) / np.abs(du)) / F(p["bf"])
    return dict(disparity=disparity, score=score, sigma_invd=sigma, status=status, candidates=cand)


def points(disparity, sigma_invd, status, K, bf, T=None):
    """the accepted pixels in raster order: xyz [n, 3] float32, sigma_invd [n], pixel [n, 2] uint16"""
    fx, fy, cx, cy = (F(v) for v in K)
    ys, xs = np.nonzero(status == 1)  # (raster order)
    z = F(bf) / disparity[ys, xs]
    X = (xs.astype(F) - cx) / fx * z
    Y = (ys.astype(F) - cy) / fy * z
    if T is not None:
        T = np.asarray(T, F).reshape(4, 4)
        X, Y, z = ((T[r, 0] * X + (T[r, 1] * Y + T[r, 2] * z)) + T[r, 3] for r in range(3))
    xyz = np.stack([X, Y, z], 1).astype(F).reshape(-1, 3)
    return xyz, sigma_invd[ys, xs].astype(F), np.stack([xs, ys], 1).astype(np.uint16).reshape(-1, 2)
