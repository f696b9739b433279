"""The semi-dense map merge (include/vo_hip.h, "Semi-dense map merge"), restated in numpy from the definition and
independent of the kernel: every pixel at once as arrays, every float operation a float32 numpy operation of its own in the order the
header states, the counts as integers."""
import numpy as np

from semidense_temporal_restatement import seed

DEFAULTS = dict(chi=3.0, keep_obs=2)
F = np.float32
ORIGIN = {0: "nothing", 1: "the map's", 2: "the result's", 3: "fused", 4: "inconsistent: the map kept", 5: "inconsistent: dropped"}


def merge(m, disparity, sigma_invd, status, bf, **params):
    """m: dict(invd, sigma, n_obs) or None; the disparity result's three planes; -> dict(invd, sigma float32; n_obs, origin uint8;
    counts uint64 [6])"""
    p = dict(DEFAULTS, **params)
    chi2 = F(p["chi"]) * F(p["chi"])
    keep = int(p["keep_obs"])
    d = seed(np.asarray(disparity, F), np.asarray(sigma_invd, F), np.asarray(status, np.uint8), bf)
    rho, sig, nd = d["invd"], d["sigma"], d["n_obs"]
    shape = rho.shape
    if m is None:
        mi, ms, mn = np.zeros(shape, F), np.zeros(shape, F), np.zeros(shape, np.uint8)
    else:
        mi, ms, mn = np.asarray(m["invd"], F), np.asarray(m["sigma"], F), np.asarray(m["n_obs"], np.uint8)
    has_m, has_s = mn >= 1, nd >= 1
    with np.errstate(all="ignore"):
        dd = mi - rho
        s2, m2 = ms * ms, sig * sig
        tot = s2 + m2
        agree = (tot > F(0)) & (dd * dd <= chi2 * tot)  # (a NaN compares false)
        f_invd = (mi * m2 + rho * s2) / tot
        f_sigma = np.sqrt((s2 * m2) / tot)
    both = has_m & has_s
    fused = both & agree
    kept = both & ~agree & (mn.astype(np.int64) >= keep)
    dropped = both & ~agree & ~kept
    only_m, only_s = has_m & ~has_s, has_s & ~has_m
    origin = np.zeros(shape, np.uint8)
    for k, sel in ((1, only_m), (2, only_s), (3, fused), (4, kept), (5, dropped)):
        origin[sel] = k
    from_map = only_m | kept
    invd, sigma, n_obs = np.zeros(shape, F), np.zeros(shape, F), np.zeros(shape, np.uint8)
    # bits, not values: a NaN's payload and a negative zero survive
    iv, sv = invd.view(np.uint32), sigma.view(np.uint32)
    iv[from_map], sv[from_map], n_obs[from_map] = mi.view(np.uint32)[from_map], ms.view(np.uint32)[from_map], mn[from_map]
    iv[only_s], sv[only_s], n_obs[only_s] = rho.view(np.uint32)[only_s], sig.view(np.uint32)[only_s], nd[only_s]
    iv[fused], sv[fused] = f_invd.astype(F).view(np.uint32)[fused], f_sigma.astype(F).view(np.uint32)[fused]
    n_obs[fused] = np.minimum(mn[fused].astype(np.int64) + 1, 255).astype(np.uint8)
    counts = np.bincount(origin.reshape(-1), minlength=6).astype(np.uint64)
    return dict(invd=invd, sigma=sigma, n_obs=n_obs, origin=origin, counts=counts)
