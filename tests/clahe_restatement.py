"""cv::CLAHE::apply for 8-bit images (OpenCV 4.x imgproc/src/clahe.cpp) restated in numpy, from the arithmetic written down in
include/vo_hip.h (vo_set_equalize). Restated from knowledge of upstream, NOT pinned against an OpenCV build. Integer maths for the
extension, the histograms, the clipping and the running sum; explicit float32 steps and np.rint (round half to even) for the two
saturate casts. What the kernels (csrc/clahe_device.hpp) are compared with, on CPU threads and on the GPU."""
import numpy as np

f32 = np.float32


def extension(w, h, tiles_x, tiles_y):
    """(w_ext, h_ext, tw, th): both amounts apply whenever either remainder is non-zero."""
    if w % tiles_x == 0 and h % tiles_y == 0:
        we, he = w, h
    else:
        we, he = w + (tiles_x - w % tiles_x), h + (tiles_y - h % tiles_y)
    return we, he, we // tiles_x, he // tiles_y


def _reflect101(n, n_ext):
    i = np.arange(n_ext)
    return np.where(i < n, i, 2 * (n - 1) - i)


def clip_limit_int(clip, total):
    """None: no clipping."""
    if not clip > 0:
        return None
    lim = float(clip) * float(total) / 256.0  # product and quotient in double
    if lim >= total:  # no bin holds more than `total`: nothing is cut (and (int) of a huge double is not asked for)
        return None
    return max(int(lim), 1)


def tile_luts(img, clip=40.0, tiles=(8, 8)):
    """uint8 [tiles_y, tiles_x, 256]"""
    img = np.ascontiguousarray(img, np.uint8)
    h, w = img.shape
    tx, ty = tiles
    assert w > tx and h > ty
    we, he, tw, th = extension(w, h, tx, ty)
    ext = img[_reflect101(h, he)][:, _reflect101(w, we)]
    total = tw * th
    limit = clip_limit_int(clip, total)
    scale = f32(255) / f32(total)
    luts = np.zeros((ty, tx, 256), np.uint8)
    for j in range(ty):
        for i in range(tx):
            hist = np.bincount(ext[j * th:(j + 1) * th, i * tw:(i + 1) * tw].ravel(), minlength=256).astype(np.int64)
            if limit is not None:
                clipped = int(np.maximum(hist - limit, 0).sum())
                hist = np.minimum(hist, limit)
                batch = clipped // 256
                residual = clipped - 256 * batch
                hist += batch
                if residual != 0:
                    step = max(256 // residual, 1)
                    k = 0
                    while k < 256 and residual > 0:
                        hist[k] += 1
                        k += step
                        residual -= 1
            s = np.cumsum(hist)
            v = np.rint(s.astype(f32) * scale)  # one float32 product, then round half to even
            luts[j, i] = np.clip(v, 0, 255).astype(np.uint8)
    return luts


def _cells(n, t, n_tiles):
    p = np.arange(n).astype(f32)
    inv = f32(1.0) / f32(t)
    tf = (p * inv).astype(f32) - f32(0.5)
    t1 = np.floor(tf).astype(np.int64)
    a = (tf - t1.astype(f32)).astype(f32)
    a1 = (f32(1.0) - a).astype(f32)
    t2 = np.minimum(t1 + 1, n_tiles - 1)
    t1 = np.maximum(t1, 0)
    return t1, t2, a, a1


def clahe(img, clip=40.0, tiles=(8, 8)):
    """(out uint8 [h, w], luts uint8 [tiles_y, tiles_x, 256])"""
    img = np.ascontiguousarray(img, np.uint8)
    h, w = img.shape
    tx, ty = tiles
    luts = tile_luts(img, clip, tiles)
    _, _, tw, th = extension(w, h, tx, ty)
    x1, x2, xa, xa1 = _cells(w, tw, tx)
    y1, y2, ya, ya1 = _cells(h, th, ty)
    L = luts.astype(f32)
    v = img.astype(np.int64)
    Y1, Y2, X1, X2 = y1[:, None], y2[:, None], x1[None, :], x2[None, :]
    XA, XA1, YA, YA1 = xa[None, :], xa1[None, :], ya[:, None], ya1[:, None]
    # every product and every sum is a float32 operation of its own
    top = ((L[Y1, X1, v] * XA1).astype(f32) + (L[Y1, X2, v] * XA).astype(f32)).astype(f32)
    bot = ((L[Y2, X1, v] * XA1).astype(f32) + (L[Y2, X2, v] * XA).astype(f32)).astype(f32)
    res = ((top * YA1).astype(f32) + (bot * YA).astype(f32)).astype(f32)
    return np.clip(np.rint(res), 0, 255).astype(np.uint8), luts
