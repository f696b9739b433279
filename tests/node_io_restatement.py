"""numpy restatement of what include/vo_hip.h states for the nodes' image encodings (vo_set_input_format: the gray
conversion, the float remap and its convertTo) and for the debug image (vo_draw_tracking, vo_draw_tracking_ba: centres,
stamps, lines, overlap order). Written from the header's text; used by tests/test_node_io.py (against the kernels' own
text on CPU threads) and tests/test_node_io_gpu.py (against the device)."""
import numpy as np

FORMATS = {"mono8": 0, "rgb8": 1, "bgr8": 2, "mono16u": 3, "mono16s": 4, "f32": 5}
DTYPES = {"mono8": np.uint8, "rgb8": np.uint8, "bgr8": np.uint8, "mono16u": np.uint16, "mono16s": np.int16, "f32": np.float32}


# ---- ingestion -------------------------------------------------------------------------------------------------
def gray(img, bgr=False):
    """(H, W, 3) uint8 -> (H, W) uint8: (c0*9798 + c1*19235 + c2*3735 + 16384) >> 15, c0 and c2 exchanged for bgr"""
    c = img.astype(np.int64)
    c0, c1, c2 = (c[..., 2], c[..., 1], c[..., 0]) if bgr else (c[..., 0], c[..., 1], c[..., 2])
    return ((c0 * 9798 + c1 * 19235 + c2 * 3735 + 16384) >> 15).astype(np.uint8)


def _quantise(m):
    """cvRound(m * 32) -> (integer part, 1/32 fraction); NaN and |.| >= 2^31 are far outside"""
    with np.errstate(invalid="ignore", over="ignore"):
        r = np.rint(np.asarray(m, np.float32) * np.float32(32.0))
    far = ~np.isfinite(r) | (np.abs(r) >= 2.0 ** 31)
    q = np.where(far, -2.0 ** 31, r).astype(np.int64)
    return q >> 5, q & 31


def _taps(src, mu, mv):
    h, w = src.shape
    sx, ax = _quantise(mu)
    sy, ay = _quantise(mv)

    def tap(dy, dx):
        y, x = sy + dy, sx + dx
        ok = (x >= 0) & (x < w) & (y >= 0) & (y < h)
        return np.where(ok, src[np.clip(y, 0, h - 1), np.clip(x, 0, w - 1)], src.dtype.type(0))
    return tap(0, 0), tap(0, 1), tap(1, 0), tap(1, 1), ax, ay


def remap_u8(src, mu, mv):
    """u8 samples: the integer form (every product and the sum are exact), round half to even of sum / 1024"""
    v00, v01, v10, v11, ax, ay = _taps(src.astype(np.int64), mu, mv)
    s = v00 * ((32 - ay) * (32 - ax)) + v01 * ((32 - ay) * ax) + v10 * (ay * (32 - ax)) + v11 * (ay * ax)
    return ((s + 511 + ((s >> 10) & 1)) >> 10).astype(np.uint8)


def float_to_u8(s):
    """convertTo(CV_8UC1): NaN -> 0, |s| >= 2^31 -> 0, else round half to even, clamped to [0, 255]"""
    s = np.asarray(s, np.float32)
    with np.errstate(invalid="ignore"):
        zero = np.isnan(s) | ~(np.abs(s) < np.float32(2.0 ** 31))
        r = np.clip(np.rint(np.where(zero, np.float32(0), s)), 0, 255)
    return r.astype(np.uint8)


def remap_float(src, mu, mv):
    """float samples: ((v00*w00 + v01*w01) + v10*w10) + v11*w11, every product and every sum rounded to float32"""
    v00, v01, v10, v11, ax, ay = _taps(src.astype(np.float32), mu, mv)
    k = np.float32(1.0 / 1024.0)
    w00, w01 = ((32 - ay) * (32 - ax)).astype(np.float32) * k, ((32 - ay) * ax).astype(np.float32) * k
    w10, w11 = (ay * (32 - ax)).astype(np.float32) * k, (ay * ax).astype(np.float32) * k
    with np.errstate(invalid="ignore", over="ignore"):
        s = ((v00 * w00 + v01 * w01) + v10 * w10) + v11 * w11
    assert s.dtype == np.float32
    return float_to_u8(s)


def ingest(img, fmt, mu, mv):
    """level 0 of an image of format `fmt` through the maps"""
    if fmt == "mono8":
        return remap_u8(img, mu, mv)
    if fmt in ("rgb8", "bgr8"):
        return remap_u8(gray(img, fmt == "bgr8"), mu, mv)
    return remap_float(img, mu, mv)


# ---- debug image -----------------------------------------------------------------------------------------------
def centre(p):
    """(rint(x), rint(y)) half to even, or None for a NaN coordinate or |coordinate| >= 2^30"""
    x, y = np.float32(p[0]), np.float32(p[1])
    if np.isnan(x) or np.isnan(y) or not (abs(x) < 2.0 ** 30) or not (abs(y) < 2.0 ** 30):
        return None
    return int(np.rint(x)), int(np.rint(y))


def circle_covers(dx, dy, r, t):
    d = 4 * (dx * dx + dy * dy)
    return max(0, 2 * r - t) ** 2 <= d <= (2 * r + t) ** 2


def rect_covers(dx, dy, h, t):
    return 2 * h - t <= 2 * max(abs(dx), abs(dy)) <= 2 * h + t


def line_pixels(a, b, w, h):
    """the pixels of a -> b that lie in a w x h image (python integers: no overflow at any length)"""
    (ax, ay), (bx, by) = a, b
    dx, dy = bx - ax, by - ay
    n = max(abs(dx), abs(dy))
    if n == 0:
        return [(ax, ay)] if 0 <= ax < w and 0 <= ay < h else []
    # along the major axis the coordinate is a + sign * k exactly: only those k can be inside
    if abs(dx) == n:
        a0, s, lim = ax, (1 if dx > 0 else -1), w
    else:
        a0, s, lim = ay, (1 if dy > 0 else -1), h
    k0, k1 = (-a0, lim - 1 - a0) if s > 0 else (a0 - (lim - 1), a0)
    out = []
    for k in range(max(k0, 0), min(k1, n) + 1):
        x, y = ax + (2 * k * dx + n) // (2 * n), ay + (2 * k * dy + n) // (2 * n)
        if 0 <= x < w and 0 <= y < h:
            out.append((x, y))
    return out


def _stamp(out, c, covers, reach, colour):
    if c is None:
        return
    h, w = out.shape[:2]
    for dy in range(-reach, reach + 1):
        for dx in range(-reach, reach + 1):
            x, y = c[0] + dx, c[1] + dy
            if 0 <= x < w and 0 <= y < h and covers(dx, dy):
                out[y, x] = colour


def _circle(out, p, r, t, colour):
    _stamp(out, centre(p), lambda dx, dy: circle_covers(dx, dy, r, t), (2 * r + t) // 2 + 1, colour)


def _rect(out, p, hh, t, colour):
    _stamp(out, centre(p), lambda dx, dy: rect_covers(dx, dy, hh, t), (2 * hh + t) // 2 + 1, colour)


def draw_tracking(gray_img, pts0, pts1, pts_new):
    """showTracking: painting in order = the highest-numbered primitive wins"""
    out = np.repeat(gray_img[:, :, None], 3, axis=2).copy()
    h, w = gray_img.shape
    for i in range(len(pts1)):
        a, b = centre(pts0[i]), centre(pts1[i])
        if a is not None and b is not None:
            for x, y in line_pixels(a, b, w, h):
                out[y, x] = (0, 255, 255)
    for pts, col in ((pts0, (255, 0, 255)), (pts1, (0, 255, 0)), (pts_new, (255, 0, 0))):
        for p in pts:
            _circle(out, p, 3, 2, (0, 0, 0))
            _circle(out, p, 2, 1, col)
    return out


def draw_tracking_ba(gray_img, pts, pts_proj):
    out = np.repeat(gray_img[:, :, None], 3, axis=2).copy()
    for p in pts:
        _circle(out, p, 1, 4, (0, 0, 255))
    for p in pts_proj:
        _rect(out, p, 6, 2, (0, 255, 0))
    return out


# ---- inputs shared by the CPU and the GPU tests ----------------------------------------------------------------------
def edge_case_maps(w, h, seed=5):
    """maps over a w x h image (w >= 33, h >= 5) with cv::remap's corner cases, as tests/test_rectify_gpu.py builds them: halves of
    the 1/32 grid, taps straddling every border, coordinates far outside, NaN"""
    rng = np.random.default_rng(seed)
    mu = rng.uniform(-3, w + 2, (h, w)).astype(np.float32)
    mv = rng.uniform(-3, h + 2, (h, w)).astype(np.float32)
    mu[0, :32] = (np.arange(32) + 0.5) / 32.0 + 5.0
    mv[0, :32] = 7.0 + 1.0 / 64.0
    mu[1, :8] = [-1.0, -0.5, -1.0 - 1 / 64, w - 1, w - 0.5, w, 1e9, -1e9]
    mv[1, :8] = [3.25] * 8
    mv[2, :8] = [-1.0, -0.5, -1.0 - 1 / 64, h - 1, h - 0.5, h, 3e9, -3e9]
    mu[2, :8] = [10.75] * 8
    mu[3, :2] = np.nan
    mv[3, 2:4] = np.nan
    mu[4, :2], mv[4, :2] = 20.5, [20.0, 21.0]  # (with the values below: interpolated sums of exactly 10.5 and 11.5)
    # integer coordinates: one tap with weight 1, the special samples below reach the conversion unmixed
    mu[5:7, :16] = np.arange(16, dtype=np.float32)[None, :]
    mv[5:7, :16] = np.array([[0.0], [1.0]], np.float32)
    return mu, mv


F32_SPECIALS = [np.nan, np.inf, -np.inf, 3e9, -7.0, 254.5, 255.5, 300.5, 0.5, 1.5, 2147483648.0, -2147483648.0, 2147483520.0]
U16_SPECIALS = [0, 255, 256, 65535, 254, 1000]
S16_SPECIALS = [0, 255, 256, 32767, -32768, -1]


def make_image(fmt, w, h, seed=0, small=False):
    """a random image of format `fmt` with the special samples in rows 0 and 1 (which edge_case_maps samples unmixed) and the .5
    pair at (20..21, 20..21). small: every value an integer in [0, 255] (comparable with the mono8 path)."""
    rng = np.random.default_rng(seed)
    if fmt in ("rgb8", "bgr8"):
        return rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    base = rng.integers(0, 256, (h, w))
    base[20, 20:22], base[21, 20:22] = [10, 11], [11, 12]
    if fmt == "mono8" or small:
        return base.astype(DTYPES[fmt])
    if fmt == "f32":
        img = (base + rng.uniform(-40, 40, (h, w))).astype(np.float32)
        img[20:22, 20:22] = base[20:22, 20:22]
        sp = F32_SPECIALS
    else:
        info = np.iinfo(DTYPES[fmt])
        img = rng.integers(max(info.min, -600), 600, (h, w)).astype(DTYPES[fmt])
        img[20:22, 20:22] = base[20:22, 20:22]
        sp = U16_SPECIALS if fmt == "mono16u" else S16_SPECIALS
    img[0, :len(sp)] = np.array(sp, DTYPES[fmt])
    img[1, 1:len(sp) + 1] = np.array(sp, DTYPES[fmt])  # (next to other values: taps of a mixed sample as well)
    return img


def strided(img, extra):
    """a view of `img` in a buffer whose rows are `extra` bytes longer (any number: rows need not stay aligned)"""
    h = img.shape[0]
    row = img[0].nbytes
    buf = np.zeros(h * (row + extra) + 8, np.uint8)
    rows = np.lib.stride_tricks.as_strided(buf, (h, row), (row + extra, 1))
    rows[:] = img.reshape(h, -1).view(np.uint8)
    return buf, row + extra
