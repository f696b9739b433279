"""Inputs that take the dense stereo operator (include/vo_hip.h, "Dense stereo") to its edges, shared by
tests/test_dense_stereo_edges.py (the cases are what they claim), tests/test_dense_stereo_edges_emu.py (the kernels' text on CPU
threads) and tests/test_dense_stereo_edges_gpu.py (the device). A plain module: EDGE_CASES maps a name to (left, right, mask or
None, parameters, row padding); restated(name) is the numpy restatement of a case, computed once, shared and never changed.

* sat_*: the penalties at their upper limit on random pairs large enough for the summed volume to pass 32767 (the u16 the volume is
  stored in holds up to 8 (62 + 8129) = 65528; the defaults never pass 1008).
* ties*: a pattern of period 8 along the rows, so that the smallest S is attained at disparities 8 apart, with a random patch that
  has one true match pasted over a quadrant; with uniqueness = 0 the choice among equal minima shows in the disparity plane.
* the penalties and the two checks at the ends of their ranges, d_min at and beyond the width, unrelated noise, a two-level pair.
* shapes below the census window (9 x 7), below a wavefront's 8 pixels of the decision, one pixel, one row, one column, two rows
  and two columns (the diagonals' start enumeration)."""
import numpy as np

from dense_stereo_restatement import dense_stereo


def random_pair(w, h, d, seed, hi=256):
    """a random pair of constant disparity d: the right image is the left one moved by d columns"""
    wide = np.random.default_rng(seed).integers(0, hi, (h, w + d), np.uint8)
    return np.ascontiguousarray(wide[:, :w]), np.ascontiguousarray(wide[:, d:])


def periodic_pair(w=150, h=30, period=8, shift=5, patch_d=20, seed=3):
    """every row a pattern of `period` columns, the right image that pattern moved by `shift`: the disparities shift, shift + period,
    .. match equally well. The lower right quadrant is random texture of the one disparity patch_d."""
    rng = np.random.default_rng(seed)
    pat = rng.integers(0, 256, (h, period), np.uint8)
    xs = np.arange(w + patch_d)
    left, right = pat[:, xs[:w] % period].copy(), pat[:, (xs[:w] + shift) % period].copy()
    tex = rng.integers(0, 256, (h, w + patch_d), np.uint8)
    y0, x0 = h // 2, w // 2
    left[y0:, x0:] = tex[y0:, x0:w]
    right[y0:, x0 - patch_d:w - patch_d] = tex[y0:, x0:w]
    return np.ascontiguousarray(left), np.ascontiguousarray(right)


def _two_level(w, h, d, seed):
    left, right = random_pair(w, h, d, seed, hi=2)
    return left * np.uint8(255), right * np.uint8(255)


def _mask(w, h):
    m = np.ones((h, w), np.uint8)
    m[:, w // 3] = 0
    m[h // 2, :] = 0
    m[h - 1, w - 1] = 0
    return m


SAT = dict(paths=8, p1=8128, p2=8129)
TINY_SHAPES = ((1, 1), (9, 1), (1, 9), (5, 3), (8, 6), (64, 2), (2, 64), (13, 7))  # (width, height)

EDGE_CASES = {}


def _add(name, pair, prm, mask=None, pad=0):
    left, right = pair
    for a in (left, right) + ((mask,) if mask is not None else ()):
        a.setflags(write=False)
    EDGE_CASES[name] = (left, right, mask, dict(prm), pad)


# ---- the u16 volume above 32767 --------------------------------------------------------------------------------------------------
_add("sat_n64", random_pair(288, 288, 10, 1), dict(SAT, n_disp=64))
_add("sat_n128", random_pair(288, 288, 70, 1), dict(SAT, n_disp=128))  # two disparities a lane: the lane-edge exchange carries them
_add("sat_p1_0", random_pair(288, 288, 10, 1), dict(n_disp=64, paths=8, p1=0, p2=8129))
_add("paths4_p2_8129", random_pair(97, 21, 10, 2), dict(n_disp=64, paths=4, p1=8128, p2=8129))  # (4 paths stay below 4 * 8191)
# ---- ties ------------------------------------------------------------------------------------------------------------------------
_add("ties", periodic_pair(), dict(n_disp=64, d_min=2))
_add("ties_uniq0", periodic_pair(), dict(n_disp=64, d_min=2, uniqueness=0))
# ---- the penalties and the checks at the ends of their ranges --------------------------------------------------------------------
for _name, _prm in (("p1_0_p2_1", dict(p1=0, p2=1)), ("p1_63_p2_64", dict(p1=63, p2=64)), ("uniq_0", dict(uniqueness=0)),
                    ("uniq_99", dict(uniqueness=99)), ("lr_0", dict(lr_max=0)), ("lr_64", dict(lr_max=64))):
    _add(_name, random_pair(97, 21, 10, 2), dict(_prm, n_disp=64))
_add("d_min_39", random_pair(40, 21, 10, 4), dict(n_disp=64, d_min=39))  # one column has a right pixel, at d = 0 alone
_add("d_min_40", random_pair(40, 21, 10, 4), dict(n_disp=64, d_min=40))  # none has
_add("unrelated_noise", (random_pair(97, 21, 0, 5)[0], random_pair(97, 21, 0, 6)[0]), dict(n_disp=64))
_add("two_level", _two_level(97, 21, 10, 7), dict(n_disp=64))
_add("grey_0_127", random_pair(97, 21, 10, 8, hi=128), dict(n_disp=64))  # (the monotone remap v -> 2 v + 1 starts from this one)
# ---- tiny shapes -----------------------------------------------------------------------------------------------------------------
for _w, _h in TINY_SHAPES:
    _add(f"tiny_{_w}x{_h}", random_pair(_w, _h, 2, 10 + _w + 64 * _h), dict(n_disp=64))
_add("tiny_13x7_mask", random_pair(13, 7, 2, 10 + 13 + 64 * 7), dict(n_disp=64), mask=_mask(13, 7))
_add("tiny_5x3_stride", random_pair(5, 3, 2, 10 + 5 + 64 * 3), dict(n_disp=64), pad=11)

TINY = tuple(k for k in EDGE_CASES if k.startswith("tiny_"))
SATURATED = ("sat_n64", "sat_n128", "sat_p1_0")
FLIP_CASES = ("tiny_13x7", "tiny_2x64", "uniq_0")  # 13 x 7, 2 x 64 and 97 x 21: their pairs, with the defaults and 4 or 8 paths


def far_ties(S):
    """the pixels whose smallest S is attained at two disparities more than 1 apart"""
    at_min = S == S.min(axis=2, keepdims=True)
    n = S.shape[2]
    first, last = at_min.argmax(axis=2), n - 1 - at_min[:, :, ::-1].argmax(axis=2)
    return last - first > 1


def _large_next_to_accepted(S, status):
    """the numbers of accepted pixels whose S2 (the smallest S more than 1 away from d_best), and whose parabola's S(d_best - 1),
    lie above 32767: where a signed 16-bit step in the uniqueness test or in the parabola would show"""
    n = S.shape[2]
    d_best = S.argmin(axis=2)
    s2 = np.where(np.abs(np.arange(n)[None, None, :] - d_best[:, :, None]) > 1, S, np.int32(1 << 30)).min(axis=2)
    sm = np.take_along_axis(S, np.clip(d_best - 1, 0, n - 1)[:, :, None], axis=2)[:, :, 0]
    ok = status == 1
    return dict(s2_large_accepted=int((ok & (s2 > 32767)).sum()), sm_large_accepted=int((ok & (sm > 32767)).sum()))


_WANT = {}


def restated(name):
    """the restatement of a case, computed once and shared read-only: the four planes and n_accepted, and in place of the volume
    S what the tests ask of it: s_max, above_32767 (the share of its entries) and far_ties (a plane of booleans)"""
    if name not in _WANT:
        left, right, mask, prm, _ = EDGE_CASES[name]
        r = dense_stereo(left, right, mask, **prm)
        S = r.pop("S")
        r.update(s_max=int(S.max()), above_32767=float((S > 32767).mean()), far_ties=far_ties(S), **_large_next_to_accepted(S, r["status"]))
        for v in r.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _WANT[name] = r
    return _WANT[name]


def flipped(planes):
    """a result's planes with the rows in reverse order"""
    return {k: np.ascontiguousarray(planes[k][::-1]) for k in ("disparity", "cost", "sigma_invd", "status")}
