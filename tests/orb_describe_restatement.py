"""cv::ORB::compute as include/vo_hip.h ("ORB orientation and descriptors") states it, written from that text in numpy and
vectorised over the keypoints of a level: what tests/test_orb_describe.py and tests/test_orb_describe_gpu.py measure the
emulated and the real kernel against. Shares no code with the library."""
import numpy as np

M64 = (1 << 64) - 1
UMAX = (15, 15, 15, 15, 14, 14, 14, 13, 13, 12, 11, 10, 9, 8, 6, 3)
KER = (18, 34, 49, 54, 49, 34, 18)
BORDER = 32  # >= 22 + 3: the farthest tap of a blurred sample


def _mix(z):
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def seeded_pattern(seed=0x4F52423331):
    """step 5 of the header; the default table is seed 0x4F52423331"""
    out = np.zeros(1024, np.int8)
    for k in range(1024):
        z = _mix((seed + (k + 1) * 0x9E3779B97F4A7C15) & M64)
        out[k] = int(((z >> 32) * 31) >> 32) - 15
    return out.reshape(512, 2)


def reflect101(p, n):
    p = np.array(p, np.int64)
    while True:
        bad = (p < 0) | (p >= n)
        if not bad.any():
            return p
        p = np.where(p < 0, -p, np.where(p >= n, 2 * n - 2 - p, p))


def fast_atan2(y, x):
    f = np.float32
    y, x = np.asarray(y, f), np.asarray(x, f)
    K = f(180.0 / np.pi)
    p1, p3, p5, p7 = f(0.9997878412794807) * K, f(-0.3258083974640975) * K, f(0.1555786518463281) * K, f(-0.04432655554792128) * K
    eps = f(2.220446049250313e-16)
    ax, ay = np.abs(x), np.abs(y)
    swap = ~(ax >= ay)
    num, den = np.where(swap, ax, ay), np.where(swap, ay, ax)
    c = num / (den + eps)
    c2 = c * c
    a = (((p7 * c2 + p5) * c2 + p3) * c2 + p1) * c
    a = np.where(swap, f(90.0) - a, a)
    a = np.where(x < 0, f(180.0) - a, a)
    a = np.where(y < 0, f(360.0) - a, a)
    assert a.dtype == f
    return a


def describe(levels, scales, xy, octave, pattern, edge=31, steer=True):
    """levels: the ORB pyramid (uint8 images); scales: the float scale of each; -> (angle, desc [n, 32], valid)"""
    f = np.float32
    xy, octave = np.asarray(xy, f).reshape(-1, 2), np.asarray(octave, np.int64).reshape(-1)
    n = xy.shape[0]
    ang, desc, valid = np.zeros(n, f), np.zeros((n, 32), np.uint8), np.zeros(n, bool)
    pat = np.asarray(pattern).reshape(512, 2)
    px, py = pat[:, 0].astype(f), pat[:, 1].astype(f)
    for L, img in enumerate(levels):
        idx = np.nonzero(octave == L)[0]
        if idx.size == 0:
            continue
        h, w = img.shape
        inv = f(1.0) / f(scales[L])
        with np.errstate(invalid="ignore"):
            xf, yf = np.rint(xy[idx, 0] * inv), np.rint(xy[idx, 1] * inv)
            ok = (xf >= f(edge)) & (xf < f(w - edge)) & (yf >= f(edge)) & (yf < f(h - edge))
        idx = idx[ok]
        if idx.size == 0:
            continue
        valid[idx] = True
        cx, cy = xf[ok].astype(np.int64) + BORDER, yf[ok].astype(np.int64) + BORDER
        E = img[np.ix_(reflect101(np.arange(-BORDER, h + BORDER), h), reflect101(np.arange(-BORDER, w + BORDER), w))].astype(np.int64)
        a_deg = np.zeros(idx.size, f)
        if steer:
            m10, m01 = np.zeros(idx.size, np.int64), np.zeros(idx.size, np.int64)
            for v in range(-15, 16):
                for u in range(-UMAX[abs(v)], UMAX[abs(v)] + 1):
                    I = E[cy + v, cx + u]
                    m10 += u * I
                    m01 += v * I
            a_deg = fast_atan2(m01.astype(f), m10.astype(f))
        ang[idx] = a_deg
        # B at every position of E that has its 7 x 7 taps: rows / columns 3 .. size - 4
        hp = sum(KER[i] * E[:, i: E.shape[1] - 6 + i] for i in range(7))
        vp = sum(KER[j] * hp[j: hp.shape[0] - 6 + j, :] for j in range(7))
        B = (vp + (1 << 15)) >> 16
        r = (a_deg * f(np.pi / 180.0)).astype(np.float64)
        a, b = np.cos(r).astype(f)[:, None], np.sin(r).astype(f)[:, None]
        ix = np.rint(px[None, :] * a - py[None, :] * b).astype(np.int64)
        iy = np.rint(px[None, :] * b + py[None, :] * a).astype(np.int64)
        vals = B[cy[:, None] + iy - 3, cx[:, None] + ix - 3]
        bits = (vals[:, 0::2] < vals[:, 1::2]).astype(np.uint8)
        desc[idx] = np.packbits(bits.reshape(-1, 32, 8), axis=2, bitorder="little")[:, :, 0]
    return ang, desc, valid
