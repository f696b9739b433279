"""The ignore mask (include/vo_hip.h, "Ignore mask") on the CPU loops, for tests/test_mask*.py: the two hooks of
oracle/stereo_vo.py and oracle/mono_vo.py composed with the lookup —
  _detect_bucket   orb_detect -> drop the keypoints whose lookup is 0 -> bucket_argmax    ("detect, drop, then bucket")
  frame()          stage 4 -> 3 where the lookup at the feature's current (left) pixel is 0   (the track gate)
`mask` is an attribute: the test sets the mask of frame k before track() of frame k; None = no mask (the parent's loop).
The counters say how often the mask bit, so that a test whose mask never bites cannot pass."""
import numpy as np

from oracle import oracle as O
from oracle.mono_vo import MonoVORef
from oracle.stereo_vo import StereoVORef


def lookup(mask, pts):
    """mask[(int)(y + 0.5f)][(int)(x + 0.5f)] != 0 in float32; outside the plane: False. Written out here on its own (not the
    package's mask_lookup, which tests/test_mask.py checks against this one)."""
    pts = np.asarray(pts, np.float32).reshape(-1, 2)
    h, w = mask.shape
    out = np.zeros(len(pts), bool)
    for i, (x, y) in enumerate(pts):
        fx, fy = np.float32(x) + np.float32(0.5), np.float32(y) + np.float32(0.5)
        if not (fx > -1.0 and fy > -1.0 and fx < w and fy < h):  # (NaN: False)
            continue
        out[i] = mask[int(fy), int(fx)] != 0  # int() truncates toward zero, as the C cast
    return out


def masked_table(img, mask, iu, iv, nu, nv, thres_fast=15, weight=None):
    """The per-bin candidate table of `img` under `mask`: (xy [bins, 2], has [bins], n_detected, unmasked winners on masked
    pixels). weight = None: every bin."""
    d = O.orb_detect(img, thres_fast)
    xy, resp = d["xy"], d["response"]
    w = np.ones(nu * nv, np.int32) if weight is None else weight
    keep = lookup(mask, xy) if mask is not None else np.ones(len(xy), bool)
    pts, _ = O.bucket_argmax(xy[keep], resp[keep], iu, iv, nu, nv, w)
    pts0, _ = O.bucket_argmax(xy, resp, iu, iv, nu, nv, w)
    displaced = int((~lookup(mask, pts0)).sum()) if mask is not None else 0
    tab = np.zeros((nu * nv, 2), np.float32)
    has = np.zeros(nu * nv, np.uint8)
    for p in pts:
        b = int(np.floor(np.float32(p[1]) * np.float32(iv))) * nu + int(np.floor(np.float32(p[0]) * np.float32(iu)))
        tab[b], has[b] = p, 1
    return tab, has, len(xy), displaced, pts


class _Masked:
    mask = None
    n_demoted = 0      # features the gate kept at stage 3
    n_displaced = 0    # winners of the unmasked buckets that lie on masked pixels (summed over the detections)

    def _detect_bucket(self, img, weight):
        if self.mask is None:
            return super()._detect_bucket(img, weight)
        d = O.orb_detect(img, self.thres_fast)
        keep = lookup(self.mask, d["xy"])
        pts0, _ = O.bucket_argmax(d["xy"], d["response"], self.iu, self.iv, self.nu, self.nv, weight)
        self.n_displaced += int((~lookup(self.mask, pts0)).sum())
        pts, _ = O.bucket_argmax(d["xy"][keep], d["response"][keep], self.iu, self.iv, self.nu, self.nv, weight)
        return pts

    def _gate(self, o, pts):
        if self.mask is not None:
            dem = (o["stage"] == 4) & ~lookup(self.mask, pts)
            o["stage"][dem] = 3
            self.n_demoted += int(dem.sum())
        return o


class MaskedStereoVORef(_Masked, StereoVORef):
    def frame(self, L, R, sum_mode=None, tree_width=None):
        o = super().frame(L, R, sum_mode, tree_width)
        return self._gate(o, o["pts_l1"])


class MaskedMonoVORef(_Masked, MonoVORef):
    def frame(self, I1, f, sum_mode=None, tree_width=None):
        o, op = super().frame(I1, f, sum_mode, tree_width)
        return self._gate(o, o["pts1"]), op
