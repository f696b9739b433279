"""The coarse-to-fine alignment on a map pyramid (include/vo_hip.h, "Semi-dense alignment on a map pyramid"), restated
in numpy from the definition and independent of the kernels: the map pyramid float32 operation by operation, the level loop composed
from the level-0 restatement (tests/semidense_align_restatement.py: align) applied verbatim to each level's planes. The image levels
are the caller's (the oracle's pyr_down, which the slots' pyramids equal)."""
import numpy as np

import semidense_align_restatement as AR

F = np.float32
MAX_LEVELS = 6
DEFAULTS = dict(AR.DEFAULTS, levels=4, max_iters_level=(0,) * MAX_LEVELS)  # max_iters_level[l] = 0: max_iters


def level_size(w, h, l):
    """the slot pyramid's rule: w <- (w + 1) / 2, h <- (h + 1) / 2 per level"""
    for _ in range(l):
        w, h = (w + 1) // 2, (h + 1) // 2
    return w, h


def image_pyramid(img, levels, pyr_down):
    out = [np.ascontiguousarray(img, np.uint8)]
    for _ in range(levels - 1):
        out.append(pyr_down(out[-1]))
    return out


def map_pyramid_level(m):
    """one level up: dict(invd, sigma float32, n_obs uint8) of ((h + 1) / 2, (w + 1) / 2). The children of (X, Y) are the 3 x 3 finer
    cells around (2 X, 2 Y) inside the plane, visited dy = -1, 0, 1 outer and dx = -1, 0, 1 inner."""
    invd, sigma, n_obs = np.asarray(m["invd"], F), np.asarray(m["sigma"], F), np.asarray(m["n_obs"], np.uint8)
    h, w = invd.shape
    hc, wc = (h + 1) // 2, (w + 1) // 2
    Y, X = np.meshgrid(np.arange(hc), np.arange(wc), indexing="ij")
    S, N = np.zeros((hc, wc), F), np.zeros((hc, wc), F)
    n, top = np.zeros((hc, wc), np.int64), np.zeros((hc, wc), np.uint8)
    with np.errstate(all="ignore"):
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                y, x = 2 * Y + dy, 2 * X + dx
                inside = (y >= 0) & (y < h) & (x >= 0) & (x < w)
                yc, xc = np.clip(y, 0, h - 1), np.clip(x, 0, w - 1)
                sg, iv, no = sigma[yc, xc], invd[yc, xc], n_obs[yc, xc]
                counted = inside & (no >= 1) & (sg > 0) & (iv > 0) & np.isfinite(sg) & np.isfinite(iv)
                wt = F(1) / (sg * sg)
                S = np.where(counted, S + wt, S).astype(F)
                N = np.where(counted, N + wt * iv, N).astype(F)
                n += counted
                top = np.where(counted, np.maximum(top, no), top).astype(np.uint8)
        ok = (n > 0) & np.isfinite(S) & (S > 0)
        out_invd = np.where(ok, N / S, F(0)).astype(F)
        out_sigma = np.where(ok, np.sqrt(n.astype(F) / S), F(0)).astype(F)
    return dict(invd=out_invd, sigma=out_sigma, n_obs=np.where(ok, top, 0).astype(np.uint8))


def map_pyramid(m, levels):
    """levels 0 .. levels - 1; level l + 1 is formed from level l's result"""
    out = [dict(invd=np.asarray(m["invd"], F), sigma=np.asarray(m["sigma"], F), n_obs=np.asarray(m["n_obs"], np.uint8))]
    for _ in range(levels - 1):
        out.append(map_pyramid_level(out[-1]))
    return out


def level_K(K, l):
    s = F(2.0 ** -l)
    return tuple(F(v) * s for v in K)  # (a power of two: exact)


def level_iters(p):
    mil = tuple(p["max_iters_level"]) + (0,) * MAX_LEVELS
    return [int(mil[l]) if int(mil[l]) > 0 else int(p["max_iters"]) for l in range(p["levels"])]


def align_pyr(key_levels, cur_levels, K, T_ck, m, **params):
    """the operator: level 0's dict (as align returns it) with levels=[per level dict(status, iters, count, rms)], index = level"""
    p = dict(DEFAULTS, **params)
    L = int(p["levels"])
    iters = level_iters(p)
    base = {k: p[k] for k in ("min_obs", "huber", "eps", "min_pixels")}
    maps = map_pyramid(m, L)
    T = np.asarray(T_ck, F).reshape(4, 4).copy()
    per = [None] * L
    out = None
    for l in range(L - 1, -1, -1):
        out = AR.align(key_levels[l], cur_levels[l], level_K(K, l), T, maps[l], max_iters=iters[l], **base)
        per[l] = {k: out[k] for k in ("status", "iters", "count", "rms")}
        T = out["T_ck"]  # (after status 2 or 3: the pose it was met at)
    out = dict(out)
    out["levels"] = per
    return out
