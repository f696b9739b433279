"""The regularisation of a semi-dense map (include/vo_hip.h, "Semi-dense regularisation"), restated in numpy from the
definition and independent of the kernel: whole planes shifted by (dy, dx) in the definition's neighbour order (dy outer, dx inner),
every float operation a float32 numpy operation of its own in the order the header states, a neighbour that does not count left out
of the sums by np.where — no tile, no halo, no shared memory."""
import numpy as np

DEFAULTS = dict(radius=2, chi=2.0, dist_sigma=0.01, min_support=1, fill_min=8, g_min=20)
F = np.float32
FMAX = np.finfo(np.float32).max
RSTATUS = {0: "nothing", 1: "kept and smoothed", 2: "an entry removed", 3: "filled and kept"}


def _shift(a, dy, dx, r):
    """plane a padded by r (with zeros: no entry) -> the plane of every pixel's neighbour at (dy, dx)"""
    H, W = a.shape[0] - 2 * r, a.shape[1] - 2 * r
    return a[r + dy:r + dy + H, r + dx:r + dx + W]


def entries(m):
    with np.errstate(all="ignore"):
        return (m["n_obs"] >= 1) & (m["sigma"] > 0) & (m["sigma"] <= FMAX) & (m["invd"] > 0) & (m["invd"] <= FMAX)


def gradient2(Lk):
    """gx^2 + gy^2 of the static block, integers; 0 on the border"""
    L = Lk.astype(np.int64)
    g2 = np.zeros(L.shape, np.int64)
    gx, gy = L[1:-1, 2:] - L[1:-1, :-2], L[2:, 1:-1] - L[:-2, 1:-1]
    g2[1:-1, 1:-1] = gx * gx + gy * gy
    return g2


def regularize(m, Lk, mask=None, **params):
    """the map m (dict invd, sigma, n_obs; not modified) of the key plane Lk -> dict(invd, sigma, n_obs, rstatus) and the diagnostic
    planes filled (stage A's fills, kept or not), support, conflict. mask: the keyframe's ignore mask (0 = ignore) or None."""
    p = dict(DEFAULTS, **params)
    r = int(p["radius"])
    H, W = Lk.shape
    invd, sigma, n_obs = (np.ascontiguousarray(m[k]) for k in ("invd", "sigma", "n_obs"))
    ent = entries(dict(invd=invd, sigma=sigma, n_obs=n_obs))
    with np.errstate(all="ignore"):
        invd = np.where(ent, invd, F(0)).astype(F)
        var = np.where(ent, sigma * sigma, F(0)).astype(F)
    pad = lambda a: np.pad(a, r)
    offs = [(dy, dx) for dy in range(-r, r + 1) for dx in range(-r, r + 1)]
    chi = F(p["chi"])
    chi2 = chi * chi
    ds = F(p["dist_sigma"])
    ds2 = ds * ds

    # stage A, fill
    cand = np.zeros((H, W), bool)
    if p["fill_min"] > 0:
        cand[1:-1, 1:-1] = True
        cand &= ~ent & (gradient2(Lk) >= int(p["g_min"]) ** 2)
        if mask is not None:
            cand &= mask != 0
    P_ent, P_invd, P_var = pad(ent), pad(invd), pad(var)
    S, Wt, V, cnt = np.zeros((H, W), F), np.zeros((H, W), F), np.zeros((H, W), F), np.zeros((H, W), np.int64)
    with np.errstate(all="ignore"):
        for dy, dx in offs:
            e, i_n, v_n = _shift(P_ent, dy, dx, r), _shift(P_invd, dy, dx, r), _shift(P_var, dy, dx, r)
            w = F(1) / v_n
            S = np.where(e, S + i_n * w, S)
            Wt = np.where(e, Wt + w, Wt)
            V = np.where(e, V + v_n, V)
            cnt = cnt + e
        mean = S / Wt
        vmean = V / cnt.astype(F)
        every = np.ones((H, W), bool)
        for dy, dx in offs:
            e, i_n, v_n = _shift(P_ent, dy, dx, r), _shift(P_invd, dy, dx, r), _shift(P_var, dy, dx, r)
            dd = i_n - mean
            every &= ~e | (dd * dd <= chi2 * (v_n + vmean))
    filled = cand & (cnt >= p["fill_min"]) & every
    a_invd = np.where(filled, mean, invd).astype(F)
    a_var = np.where(filled, vmean, var).astype(F)
    a_in = ent | filled

    # stage B, support, conflict and smoothing over map A
    P_in, P_invd, P_var = pad(a_in), pad(a_invd), pad(a_var)
    S, Wt = np.zeros((H, W), F), np.zeros((H, W), F)
    support, conflict = np.zeros((H, W), np.int64), np.zeros((H, W), np.int64)
    with np.errstate(all="ignore"):
        for dy, dx in offs:
            e, o = _shift(P_in, dy, dx, r), _shift(P_ent, dy, dx, r)
            i_n, v_n = _shift(P_invd, dy, dx, r), _shift(P_var, dy, dx, r)
            dd = i_n - a_invd
            cons = e & (dd * dd <= chi2 * (a_var + v_n))
            w = F(1) / (v_n + ds2 * F(dx * dx + dy * dy))
            S = np.where(cons, S + i_n * w, S)
            Wt = np.where(cons, Wt + w, Wt)
            if (dy, dx) != (0, 0):
                support = support + (o & cons)
                conflict = conflict + (o & ~cons)
        smooth = S / Wt
        own_sigma = np.sqrt(a_var)
    keep = a_in & (support >= p["min_support"]) & (conflict <= support)
    rstatus = np.zeros((H, W), np.uint8)
    rstatus[keep & ent] = 1
    rstatus[~keep & ent] = 2
    rstatus[keep & filled] = 3
    return dict(invd=np.where(keep, smooth, F(0)).astype(F), sigma=np.where(keep, own_sigma, F(0)).astype(F),
                n_obs=np.where(keep, np.where(ent, n_obs, 1), 0).astype(np.uint8), rstatus=rstatus, filled=filled, support=support,
                conflict=conflict)
