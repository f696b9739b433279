"""image_processing::calcZNCC (core/util/image_processing.cpp:195-266) with interpImage (:28-77), restated in numpy float32 from the
arithmetic written down in include/vo_hip.h ("ZNCC") — not from the kernel. Every operation is one float32 numpy operation (each
rounded on its own, no FMA); both summation orders of the definition. What the kernel (csrc/zncc_device.hpp) is compared with, on
CPU threads and on the GPU.

Below it: the CPU loops with the gate composed into their frame() hook, in the manner of tests/mask_ref.py —
  frame()   stage 4 -> 3 where a ZNCC the gate asks for is not > thres (NaN fails)
`gate` is an attribute: None or dict(thres=, win=15, pattern="centered", pairs=("temporal",)). The counters say how often the
gate bit, so that a test whose gate never bites cannot pass."""
import numpy as np

f32 = np.float32
PATTERNS = ("reference", "centered")


def interp(img, u, v):
    """interpImage at float32 coordinates u, v (any shape): float32 values, -2 at an invalid tap. (int) truncates toward zero;
    valid iff 0 <= u0 < W - 1 and 0 <= v0 < H - 1; a NaN coordinate, and one beyond the int range, is invalid."""
    h, w = img.shape
    u, v = np.asarray(u, f32), np.asarray(v, f32)
    with np.errstate(invalid="ignore"):
        fin = np.isfinite(u) & np.isfinite(v) & (np.abs(u) < f32(2.0 ** 31)) & (np.abs(v) < f32(2.0 ** 31))
        u0 = np.where(fin, np.trunc(np.where(fin, u, 0)), -1).astype(np.int64)
        v0 = np.where(fin, np.trunc(np.where(fin, v, 0)), -1).astype(np.int64)
    valid = fin & (u0 >= 0) & (u0 < w - 1) & (v0 >= 0) & (v0 < h - 1)
    uc, vc = np.where(valid, u0, 0), np.where(valid, v0, 0)
    us, vs = np.where(valid, u, f32(0)).astype(f32), np.where(valid, v, f32(0)).astype(f32)
    ax, ay = us - uc.astype(f32), vs - vc.astype(f32)
    axay = ax * ay
    F = img.astype(f32)
    I1, I2, I3, I4 = F[vc, uc], F[vc, uc + 1], F[vc + 1, uc], F[vc + 1, uc + 1]
    val = ((axay * (((I1 - I2) - I3) + I4) + ax * (-I1 + I2)) + ay * (-I1 + I3)) + I1
    assert val.dtype == f32
    return np.where(valid, val, f32(-2.0)).astype(f32)


def offsets(win, pattern):
    """tap k = i * win + j -> (i - o, j - o) in (x, y); o = win (the reference's text) or win // 2 (centred)"""
    o = win if pattern == "reference" else win // 2
    k = np.arange(win * win)
    return (k // win - o).astype(f32), (k % win - o).astype(f32)


def _sum(terms, order):
    """sum along the last axis of float32 [n, n_elem] in the definition's order"""
    n, m = terms.shape
    if order == "reference":
        s = np.zeros(n, f32)
        for k in range(m):
            s = s + terms[:, k]
        return s
    P = 64
    while P < m:
        P *= 2
    t = np.zeros((n, P), f32)
    t[:, :m] = terms
    stride = P // 2
    while stride >= 1:
        t[:, :stride] = t[:, :stride] + t[:, stride:2 * stride]
        stride //= 2
    return t[:, 0].copy()


def zncc(img0, img1, pts0, pts1, win=15, pattern="reference", sum_order="tree"):
    """float32 [n]"""
    assert win % 2 == 1 and 3 <= win <= 31 and pattern in PATTERNS and sum_order in ("tree", "reference")
    assert img0.shape == img1.shape and img0.dtype == np.uint8 and img1.dtype == np.uint8
    p0, p1 = np.asarray(pts0, f32).reshape(-1, 2), np.asarray(pts1, f32).reshape(-1, 2)
    if len(p0) == 0:
        return np.zeros(0, f32)
    ox, oy = offsets(win, pattern)
    A = interp(img0, p0[:, :1] + ox[None, :], p0[:, 1:] + oy[None, :])
    B = interp(img1, p1[:, :1] + ox[None, :], p1[:, 1:] + oy[None, :])
    ne = f32(win * win)
    mean_l, mean_r = _sum(A, sum_order) / ne, _sum(B, sum_order) / ne
    dl, dr = A - mean_l[:, None], B - mean_r[:, None]
    numer, denom_l, denom_r = _sum(dl * dr, sum_order), _sum(dl * dl, sum_order), _sum(dr * dr, sum_order)
    with np.errstate(invalid="ignore", divide="ignore"):
        out = numer / np.sqrt(denom_l * denom_r)
    assert out.dtype == f32
    return out


# ---- the gated CPU loops ---------------------------------------------------------------------------------------------------------
from oracle.mono_vo import MonoVORef  # noqa: E402
from oracle.stereo_vo import StereoVORef  # noqa: E402


def passes(z, thres):
    with np.errstate(invalid="ignore"):
        return z > f32(thres)  # (NaN: False)


class _Gated:
    gate = None
    zncc_order = "tree"
    n_demoted = 0      # features kept at stage 3 (with tests/mask_ref.py's mask composed in: by either)
    n_zncc_demoted = 0  # ... by this gate
    last = None        # the last frame's values: dict(temporal=, stereo=) over the input features

    def _values(self, I0, I1, R, p0, pl1, pr1):
        g = self.gate
        kw = dict(win=g.get("win", 15), pattern=g.get("pattern", "centered"), sum_order=self.zncc_order)
        pairs = g.get("pairs", ("temporal",))
        out = dict(temporal=None, stereo=None)
        if "temporal" in pairs:
            out["temporal"] = zncc(I0, I1, p0, pl1, **kw)
        if "stereo" in pairs:
            out["stereo"] = zncc(I1, R, pl1, pr1, **kw)
        return out

    def _zncc_gate(self, o, vals):
        self.last = vals
        ok = np.ones(len(o["stage"]), bool)
        for z in vals.values():
            if z is not None:
                ok &= passes(z, self.gate["thres"])
        dem = (o["stage"] == 4) & ~ok
        o["stage"][dem] = 3
        self.n_demoted += int(dem.sum())
        self.n_zncc_demoted += int(dem.sum())
        return o


class GatedStereoVORef(_Gated, StereoVORef):
    def frame(self, L, R, sum_mode=None, tree_width=None):
        o = super().frame(L, R, sum_mode, tree_width)
        if self.gate is None:
            return o
        return self._zncc_gate(o, self._values(self.I0, L, R, self.pts_l, o["pts_l1"], o["pts_r1"]))


class GatedMonoVORef(_Gated, MonoVORef):
    def frame(self, I1, f, sum_mode=None, tree_width=None):
        o, op = super().frame(I1, f, sum_mode, tree_width)
        if self.gate is None or o["counts"].need_five_point:  # (a fallback frame promotes nothing on the device: no gate)
            return o, op
        return self._zncc_gate(o, self._values(self.I0, I1, None, self.pts, o["pts1"], None)), op


def with_mask(base):
    """the gate AND tests/mask_ref.py's mask on one loop: the mask's detection hook, and its lookup behind the gated frame()"""
    from mask_ref import _Masked

    class Both(_Masked, base):
        def frame(self, *a, **k):
            r = super().frame(*a, **k)
            o = r[0] if isinstance(r, tuple) else r
            self._gate(o, o["pts_l1"] if "pts_l1" in o else o["pts1"])  # (_Masked._gate: the lookup at the current pixel)
            return r
    return Both
