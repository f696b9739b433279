"""The alignment with affine brightness (include/vo_hip.h, "Semi-dense alignment with affine brightness"), restated in
numpy from the definition and independent of the kernel. Everything the block leaves unchanged is the level-0 restatement's
(tests/semidense_align_restatement.py: the pixel set and its constants, the warp and the sample, the exponential and the product)
and the pyramid restatement's (tests/semidense_align_pyr_restatement.py: the map pyramid, the levels' K and iterations); what
differs is written here: the integer state G, O, the residual against the mapped key grey level, the two further columns, the 47
sums per block, the 8 x 8 solve, the update of G and O with its range status."""
import numpy as np

import semidense_align_pyr_restatement as PR
import semidense_align_restatement as AR
from semidense_temporal_restatement import _in, _q, _sample

F, D = np.float32, np.float64
DEFAULTS = dict(AR.DEFAULTS, gain0=1.0, offset0=0.0)
PYR_DEFAULTS = dict(PR.DEFAULTS, gain0=1.0, offset0=0.0)
STATUS = {**AR.STATUS, 5: "gain or offset left its range"}
RANGE = 5
NSUM = 47
PAIRS = [(i, j) for i in range(8) for j in range(i, 8)]  # the 36 entries of H, row by row
G_MIN, G_MAX, O_MAX = 1 << 13, 1 << 19, 4080


def start_GO(gain0=1.0, offset0=0.0):
    """G0 = (int)floorf(65536 gain0 + 0.5f), O0 = (int)floorf(16 offset0 + 0.5f)"""
    return int(np.floor(F(65536) * F(gain0) + F(0.5))), int(np.floor(F(16) * F(offset0) + F(0.5)))


def residuals(c, cur, K, T, G, O, huber):
    """one iteration's per-pixel terms at the pose T and the brightness G, O: valid, r, w (int64)"""
    fx, fy, cx, cy = (F(v) for v in K)
    T = np.asarray(T, F).reshape(4, 4)
    Lc = cur.astype(np.int64)
    H, W = Lc.shape
    X, Y, Z = c["X"], c["Y"], c["Z"]
    with np.errstate(all="ignore"):
        Xc, Yc, Zc = (((T[i, 0] * X + T[i, 1] * Y) + T[i, 2] * Z) + T[i, 3] for i in range(3))
        front = Zc > AR.FRONT
        px, py = fx * (Xc / Zc) + cx, fy * (Yc / Zc) + cy
        QX, QY = _q(px.astype(F)), _q(py.astype(F))
    valid = front & _in(QX, QY, W, H)
    model = ((np.int64(G) * c["key16"].astype(np.int64) + np.int64(1 << 15)) >> 16) + np.int64(O)
    r = _sample(Lc, QX, QY) - model
    kq = int(np.floor(F(16) * F(huber) + F(0.5)))
    ar = np.abs(r)
    w = np.where(ar <= kq, 256, (256 * kq) // np.maximum(ar, 1))
    return valid, np.where(valid, r, 0), np.where(valid, w, 0)


def block_sums(c, valid, r, w, order=None):
    """the 47 integer sums per block [n_blocks, 47] int64: 36 H, 8 b, sum w r^2, sum w, count"""
    n = len(c["idx"])
    q = np.concatenate([c["q"].reshape(n, 6), c["key16"].reshape(n, 1).astype(np.int64), np.full((n, 1), 16, np.int64)], 1)
    terms = np.stack([w * q[:, i] * q[:, j] for i, j in PAIRS] + [w * q[:, i] * r for i in range(8)] + [w * r * r, w, valid.astype(np.int64)], 1)
    terms = terms.reshape(-1, NSUM)
    blk = c["idx"] // AR.BLOCK
    if order is not None:
        terms, blk = terms[order], blk[order]
    out = np.zeros((c["n_blocks"], NSUM), np.int64)
    np.add.at(out, blk, terms)
    return out


def reduce_blocks(bs):
    """the blocks' sums converted to float64 and added in block order, block 0 first; then the exact scales"""
    s = np.zeros(NSUM, D)
    for b in range(bs.shape[0]):
        s = s + bs[b].astype(D)
    return s[:36] * D(2.0 ** -16), s[36:44] * D(2.0 ** -16), s[44], s[45], int(bs[:, 46].sum())


def solve(Hs, bv):
    """LDL^T in float64 in the header's order over j = 0..7: (ok, x)"""
    A = np.zeros((8, 8), D)
    for n, (i, j) in enumerate(PAIRS):
        A[i, j] = A[j, i] = Hs[n]
    L, Dg = np.zeros((8, 8), D), np.zeros(8, D)
    with np.errstate(all="ignore"):
        for j in range(8):
            d = A[j, j]
            for k in range(j):
                d = d - (L[j, k] * L[j, k]) * Dg[k]
            if not (d > 0) or not (d > A[j, j] * AR.PIVOT) or not np.isfinite(d):
                return False, np.zeros(8, D)
            Dg[j] = d
            for i in range(j + 1, 8):
                s = A[i, j]
                for k in range(j):
                    s = s - (L[i, k] * L[j, k]) * Dg[k]
                L[i, j] = s / d
        y = np.zeros(8, D)
        for i in range(8):
            s = bv[i]
            for k in range(i):
                s = s - L[i, k] * y[k]
            y[i] = s
        x = np.zeros(8, D)
        for i in range(7, -1, -1):
            s = y[i] / Dg[i]
            for k in range(i + 1, 8):
                s = s - L[k, i] * x[k]
            x[i] = s
    if not np.isfinite(x).all():
        return False, np.zeros(8, D)
    return True, x


def align_state(key, cur, K, T_ck, G, O, m, **params):
    """the iteration from the state (T_ck, G, O): dict(T_ck, G, O, status, iters, count, rms, H [36], b [8], gain, offset,
    first_sums: the first iteration's [n_blocks, 47] integer sums)"""
    p = dict(DEFAULTS, **params)
    c = AR.constants(key, m, K, p["min_obs"])
    T = np.asarray(T_ck, F).reshape(4, 4).copy()
    T[3] = (0, 0, 0, 1)
    G, O = int(G), int(O)
    out = dict(status=1, iters=0, count=0, rms=0.0, H=np.zeros(36, D), b=np.zeros(8, D), first_sums=None)
    for it in range(p["max_iters"]):
        valid, r, w = residuals(c, cur, K, T, G, O, p["huber"])
        bs = block_sums(c, valid, r, w)
        if it == 0:
            out["first_sums"] = bs
        Hs, bv, swrr, sw, count = reduce_blocks(bs)
        out.update(iters=it + 1, count=count, H=Hs, b=bv, rms=float(np.sqrt(swrr / sw) / D(16)) if sw > 0 else 0.0)
        if count < p["min_pixels"]:
            out["status"] = 2
            break
        ok, x = solve(Hs, bv)
        if not ok:
            out["status"] = 3
            break
        with np.errstate(all="ignore"):
            Gn = D(G) + np.floor(D(65536) * x[6] + D(0.5))
            On = D(O) + np.floor(D(16) * x[7] + D(0.5))
        if not (Gn >= G_MIN and Gn <= G_MAX and On >= -O_MAX and On <= O_MAX):
            out["status"] = RANGE
            break
        nrm2 = ((((x[0] * x[0] + x[1] * x[1]) + x[2] * x[2]) + x[3] * x[3]) + x[4] * x[4]) + x[5] * x[5]
        T = AR.mul44(T, AR.se3_exp(-x[:6].astype(F)))
        G, O = int(Gn), int(On)
        if nrm2 < D(F(p["eps"])) * D(F(p["eps"])):
            out["status"] = 0
            break
    out.update(T_ck=T, G=G, O=O, gain=G / 65536.0, offset=O / 16.0)
    return out


def align(key, cur, K, T_ck, m, **params):
    """the level-0 operator: the state starts at (T_ck, G0, O0)"""
    p = dict(DEFAULTS, **params)
    G0, O0 = start_GO(p.pop("gain0"), p.pop("offset0"))
    return align_state(key, cur, K, T_ck, G0, O0, m, **p)


def align_pyr(key_levels, cur_levels, K, T_ck, m, G=None, O=None, **params):
    """the pyramid operator: level 0's dict with levels=[per level dict(status, iters, count, rms, G, O, T_ck: the state the level left)],
    index = level, and top_first_sums (the top level's first iteration). G, O: a start other than gain0 / offset0 (StereoVO's start =
    previous)"""
    p = dict(PYR_DEFAULTS, **params)
    L = int(p["levels"])
    iters = PR.level_iters(p)
    base = {k: p[k] for k in ("min_obs", "huber", "eps", "min_pixels")}
    maps = PR.map_pyramid(m, L)
    T = np.asarray(T_ck, F).reshape(4, 4).copy()
    G0, O0 = start_GO(p["gain0"], p["offset0"])
    G, O = (G0 if G is None else int(G)), (O0 if O is None else int(O))
    per = [None] * L
    out = None
    for l in range(L - 1, -1, -1):
        out = align_state(key_levels[l], cur_levels[l], PR.level_K(K, l), T, G, O, maps[l], max_iters=iters[l], **base)
        per[l] = {k: out[k] for k in ("status", "iters", "count", "rms", "G", "O", "T_ck")}
        T, G, O = out["T_ck"], out["G"], out["O"]  # (after status 2, 3 or 5: the state it was met at)
        if l == L - 1:
            top_sums = out["first_sums"]
    out = dict(out)
    out["levels"] = per
    out["top_first_sums"] = top_sums
    return out


def map_image(img, g, o):
    """an exposure change: clip(round(g I + o)) as u8"""
    return np.clip(np.rint(np.float64(g) * img.astype(np.float64) + np.float64(o)), 0, 255).astype(np.uint8)
