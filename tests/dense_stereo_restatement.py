"""Dense stereo disparity (include/vo_hip.h, "Dense stereo"), restated in numpy from the definition and from nothing
else: census 9 x 7, Hamming cost, semi-global aggregation along 4 or 8 paths, winner-take-all, uniqueness and left-right checks,
parabola. Every quantity up to the decision is an integer; the parabola is float32 with every operation rounded on its own."""
import numpy as np

DEFAULTS = dict(d_min=0, n_disp=64, paths=8, p1=8, p2=64, uniqueness=10, lr_max=1, eps_d=0.5, bf=1.0)
CENSUS_BITS = 62
# the directions in the order of the definition: the first four are `paths = 4`
DIRECTIONS = ((1, 0), (-1, 0), (0, 1), (0, -1), (1, 1), (-1, -1), (1, -1), (-1, 1))

_POP8 = np.array([bin(i).count("1") for i in range(256)], np.uint8)


def census(img):
    """u64 per pixel: tap t = (v + 3) * 9 + (k + 4) for v = -3..3 (rows, outer), k = -4..4 (columns, inner), the centre left out
    and the taps after it moved down by one; bit t is I(x + k, y + v) < I(x, y), coordinates clamped to the image."""
    img = np.asarray(img, np.uint8)
    h, w = img.shape
    ys, xs = np.arange(h), np.arange(w)
    out = np.zeros((h, w), np.uint64)
    bit = 0
    for v in range(-3, 4):
        yy = np.clip(ys + v, 0, h - 1)
        for k in range(-4, 5):
            if v == 0 and k == 0:
                continue
            xx = np.clip(xs + k, 0, w - 1)
            tap = img[yy][:, xx]
            out |= (tap < img).astype(np.uint64) << np.uint64(bit)
            bit += 1
    assert bit == CENSUS_BITS
    return out


def popcount64(a):
    return _POP8[np.ascontiguousarray(a).view(np.uint8).reshape(a.shape + (8,))].sum(axis=-1, dtype=np.int32)


def cost_volume(cl, cr, d_min, n_disp):
    """C[y, x, d] = popcount(cl(x, y) ^ cr(x - d_min - d, y)), 62 where the right pixel lies left of the image"""
    h, w = cl.shape
    C = np.full((h, w, n_disp), CENSUS_BITS, np.int32)
    for d in range(n_disp):
        s = d_min + d
        if s < w:
            C[:, s:, d] = popcount64(cl[:, s:] ^ cr[:, :w - s])
    return C


def _starts(w, h, dx, dy):
    """the pixels whose predecessor along (dx, dy) lies outside the image, each once"""
    pts = []
    if dx != 0:
        x0 = 0 if dx > 0 else w - 1
        pts += [(x0, y) for y in range(h)]
        if dy != 0:
            y0 = 0 if dy > 0 else h - 1
            pts += [(x, y0) for x in range(w) if x != x0]
    else:
        y0 = 0 if dy > 0 else h - 1
        pts += [(x, y0) for x in range(w)]
    return np.array(pts, np.int64)


def aggregate(C, dx, dy, p1, p2):
    """L_r of one direction: all paths advance together, one pixel per step"""
    h, w, n = C.shape
    L = np.zeros_like(C)
    st = _starts(w, h, dx, dy)
    x, y = st[:, 0].copy(), st[:, 1].copy()
    prev = C[y, x, :].copy()
    L[y, x, :] = prev
    big = np.int32(1 << 20)
    while True:
        x, y = x + dx, y + dy
        keep = (x >= 0) & (x < w) & (y >= 0) & (y < h)
        if not keep.any():
            break
        x, y, prev = x[keep], y[keep], prev[keep]
        mn = prev.min(axis=1, keepdims=True)
        lo = np.concatenate([np.full((len(x), 1), big, np.int32), prev[:, :-1]], axis=1)
        hi = np.concatenate([prev[:, 1:], np.full((len(x), 1), big, np.int32)], axis=1)
        best = np.minimum(np.minimum(prev, np.minimum(lo, hi) + p1), mn + p2)
        prev = C[y, x, :] + best - mn
        L[y, x, :] = prev
    return L


def dense_stereo(left, right, mask=None, **params):
    """-> dict of (h, w) planes disparity f32, cost u16, sigma_invd f32, status u8, and the summed volume S (h, w, n_disp) int32"""
    p = dict(DEFAULTS, **params)
    d_min, n, paths = int(p["d_min"]), int(p["n_disp"]), int(p["paths"])
    p1, p2, uniq, lr_max = int(p["p1"]), int(p["p2"]), int(p["uniqueness"]), int(p["lr_max"])
    assert n in (64, 128, 192, 256) and paths in (4, 8) and 0 <= p1 < p2 and 0 <= uniq <= 99 and lr_max >= -1 and d_min >= 0
    left, right = np.asarray(left, np.uint8), np.asarray(right, np.uint8)
    h, w = left.shape
    C = cost_volume(census(left), census(right), d_min, n)
    S = np.zeros_like(C)
    for dx, dy in DIRECTIONS[:paths]:
        S += aggregate(C, dx, dy, p1, p2)
    d_best = S.argmin(axis=2)  # (the first of equal minima)
    ys, xs = np.mgrid[0:h, 0:w]
    s0 = S[ys, xs, d_best]
    dd = np.arange(n)[None, None, :]
    s2 = np.where(np.abs(dd - d_best[:, :, None]) > 1, S, np.int32(1 << 30)).min(axis=2)
    # the right view's disparity from the same volume: d_R(x_r) = argmin_d S(x_r + d_min + d, y, d) over the d inside the image
    xl = xs[:, :, None] + d_min + dd
    inside = xl < w
    diag = np.where(inside, S[ys[:, :, None], np.minimum(xl, w - 1), dd], np.int32(1 << 30))
    d_right = diag.argmin(axis=2)
    status = np.ones((h, w), np.uint8)
    if lr_max >= 0:
        xr = xs - d_min - d_best
        bad = xr < 0
        bad |= np.abs(d_right[ys, np.maximum(xr, 0)] - d_best) > lr_max
        status[bad] = 3
    status[s2.astype(np.int64) * (100 - uniq) < s0.astype(np.int64) * 100] = 2
    status[(d_best == 0) | (d_best == n - 1)] = 4
    if mask is not None:
        status[np.asarray(mask) == 0] = 0
    ok = status == 1
    dm, dp = np.clip(d_best - 1, 0, n - 1), np.clip(d_best + 1, 0, n - 1)
    sm, sp, sc = S[ys, xs, dm].astype(np.float32), S[ys, xs, dp].astype(np.float32), s0.astype(np.float32)
    den = (sm + sp) - (sc + sc)
    with np.errstate(divide="ignore", invalid="ignore"):
        off = np.where(den != 0, (np.float32(0.5) * (sm - sp)) / den, np.float32(0)).astype(np.float32)
    disparity = np.where(ok, (d_min + d_best).astype(np.float32) + off, np.float32(0)).astype(np.float32)
    sigma = np.where(ok, np.float32(p["eps_d"]) / np.float32(p["bf"]), np.float32(0)).astype(np.float32)
    cost = np.where(status != 0, s0, 0).astype(np.uint16)
    return dict(disparity=disparity, cost=cost, sigma_invd=sigma, status=status, S=S, n_accepted=int(ok.sum()))
