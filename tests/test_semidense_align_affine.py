"""The alignment with affine brightness (include/vo_hip.h, "Semi-dense alignment with affine brightness"): the definition — as
tests/semidense_align_affine_restatement.py states it — does its job on the synthetic 640 x 240 stream under an exposure change. The
setup of tests/test_semidense_align.py: the map of pose 2 fused with poses 3, 4, 5, the left image of pose 3 as the current one, the
start off by XI_START (62 mm, 0.21 degrees), max_iters = 20; the current image is mapped by clip(round(g I + o)) to u8 — saturated
pixels are part of the test — for (g, o) = (1, 0), (0.7, 25), (1.3, -20), (0.5, 60), (1, 15).
Measured once with the two restatements; t = translation distance to the stream's pose in mm:
  (g, o)        affine: iterations, rms, t, gain, offset        plain (§20): status, iterations, rms, t
  (1, 0)        6, 4.63, 0.618, 0.965, 4.5                      0, 7, 4.72, 0.661
  (0.7, 25)     9, 3.51, 0.688, 0.673, 28.4                     0, 17, 14.06, 5.241
  (1.3, -20)    8, 5.66, 0.572, 1.254, -14.1                    0, 13, 17.52, 2.906
  (0.5, 60)     12, 2.66, 0.724, 0.480, 62.6                    0, 19, 13.32, 3.763
  (1, 15)       6, 4.63, 0.620, 0.965, 19.6                     1, 20, 14.80, 8.277
The pose bound is set once from these: the geometric mean of the worst affine error and the best plain error over the four changed
images, sqrt(0.724 x 2.906) = 1.45 mm. Every affine run stays below it, every plain run on a changed image above it: the two together
show that the estimated gain and offset make the difference. On the unchanged image the affine error may exceed the plain one by at
most 0.1 mm. The estimated gain lies within 0.06 of g and the offset within 6 grey levels of o (clipping and Huber's weights bias
them: the worst here are 0.046 and 5.94).
The pyramid operator from the identity (800 mm off) with 4 levels under the same changes: t = 0.620 / 0.686 / 0.574 / 0.694 / 0.622
with gain and offset, 0.657 / 5.416 / 3.110 / 4.037 / 10.144 without; the same bound.
Exact properties: gain0 = 8 against a black image ends in status 5 with T, G, O as started; levels = 1 is the level-0 operator in
every field; G and O are handed from level to level; one iteration's 47 sums equal a direct Python-integer loop and stay below the
header's bounds. Also the parameter helper, the C defaults and the result structure. No GPU."""
import ctypes as C

import numpy as np
import pytest

import semidense_align_affine_restatement as FR
import semidense_align_pyr_restatement as PR
import semidense_align_restatement as AR
from test_semidense_align import distance
from test_semidense_align_affine_emu import same_levels, same_result
from test_semidense_align_emu import K, XI_START, perturbed, synthetic_setup

F = np.float32
I4 = np.eye(4, dtype=F)
CHANGES = [(1, 0), (0.7, 25), (1.3, -20), (0.5, 60), (1, 15)]
POSE_BOUND_MM = 1.45  # sqrt(0.724 x 2.906): see above
GAIN_BOUND, OFFSET_BOUND = 0.06, 6.0
UNCHANGED_SLACK_MM = 0.1


@pytest.fixture(scope="module")
def fr(oracle):
    d = dict(synthetic_setup())
    d["pyr2"] = PR.image_pyramid(d["L"][2], 4, oracle.pyr_down)
    d["pyr_down"] = oracle.pyr_down
    return d


@pytest.mark.parametrize("g,o", CHANGES)
def test_exposure_change_level_0(fr, g, o):
    cur = FR.map_image(fr["L"][3], g, o)
    if g * 255 + o > 255:
        assert (cur == 255).sum() > (fr["L"][3] == 255).sum()  # (clipped pixels are part of the test)
    T0 = perturbed(fr["T"][3], XI_START)
    a = FR.align(fr["L"][2], cur, K, T0, fr["map2"], max_iters=20)
    p = AR.align(fr["L"][2], cur, K, T0, fr["map2"], max_iters=20)
    ta, tp = distance(a["T_ck"], fr["T"][3])[0], distance(p["T_ck"], fr["T"][3])[0]
    print(f"(g, o) = ({g}, {o}): affine status {a['status']} after {a['iters']} iterations, rms {a['rms']:.2f}, t = {ta:.3f} mm, gain {a['gain']:.4f}, "
          f"offset {a['offset']:.2f}; plain status {p['status']} after {p['iters']} iterations, rms {p['rms']:.2f}, t = {tp:.3f} mm")
    assert a["status"] in (0, 1) and a["count"] > 10000
    assert abs(a["gain"] - g) <= GAIN_BOUND and abs(a["offset"] - o) <= OFFSET_BOUND
    assert ta < POSE_BOUND_MM
    if (g, o) == (1, 0):
        assert ta <= tp + UNCHANGED_SLACK_MM
    else:
        assert tp > POSE_BOUND_MM  # the plain alignment on the same inputs fails the bound: the feature makes the difference


@pytest.mark.parametrize("g,o", CHANGES)
def test_exposure_change_pyramid_from_the_identity(fr, g, o):
    cur = PR.image_pyramid(FR.map_image(fr["L"][3], g, o), 4, fr["pyr_down"])
    a = FR.align_pyr(fr["pyr2"], cur, K, I4, fr["map2"], levels=4)
    ta = distance(a["T_ck"], fr["T"][3])[0]
    print(f"(g, o) = ({g}, {o}): 4 levels from the identity: status {a['status']}, t = {ta:.3f} mm, gain {a['gain']:.4f}, offset {a['offset']:.2f}; "
          f"per level (0 first) {[(d['status'], d['iters'], d['G'], d['O']) for d in a['levels']]}")
    assert a["status"] in (0, 1) and ta < POSE_BOUND_MM
    assert abs(a["gain"] - g) <= GAIN_BOUND and abs(a["offset"] - o) <= OFFSET_BOUND
    if (g, o) != (1, 0):
        p = PR.align_pyr(fr["pyr2"], cur, K, I4, fr["map2"], levels=4)
        assert distance(p["T_ck"], fr["T"][3])[0] > POSE_BOUND_MM
    assert (a["G"], a["O"]) == (a["levels"][0]["G"], a["levels"][0]["O"])


def test_range_status_leaves_the_state_as_started(fr):
    T0 = perturbed(fr["T"][3], XI_START)
    black = np.zeros_like(fr["L"][3])
    a = FR.align(fr["L"][2], black, K, T0, fr["map2"], gain0=8.0)
    assert (a["status"], a["iters"]) == (FR.RANGE, 1) and (a["G"], a["O"]) == FR.start_GO(8.0, 0.0) == (1 << 19, 0)
    assert np.array_equal(a["T_ck"], T0) and a["count"] > 10000 and a["gain"] == 8.0 and a["offset"] == 0.0
    # ... at every level of the pyramid operator, which hands that state down
    cur = PR.image_pyramid(black, 3, fr["pyr_down"])
    a = FR.align_pyr(fr["pyr2"][:3], cur, K, T0, fr["map2"], levels=3, gain0=8.0)
    assert [(d["status"], d["iters"], d["G"], d["O"]) for d in a["levels"]] == [(FR.RANGE, 1, 1 << 19, 0)] * 3 and np.array_equal(a["T_ck"], T0)


def test_one_level_is_the_level_0_operator_and_the_state_is_handed_down(fr):
    cur = FR.map_image(fr["L"][3], 0.7, 25)
    T0 = perturbed(fr["T"][3], XI_START)
    for prm in (dict(), dict(min_obs=2, huber=6.0, max_iters=3, gain0=0.8, offset0=12.5)):
        want = FR.align(fr["L"][2], cur, K, T0, fr["map2"], **prm)
        got = FR.align_pyr(fr["pyr2"][:1], [cur], K, T0, fr["map2"], levels=1, **prm)
        ok, where = same_result(got, want)
        assert ok, where
        ok, where = same_levels(got["levels"], [want])
        assert ok, where
    # two levels by hand: level 0 run from the state level 1 left equals the pyramid operator
    curp = PR.image_pyramid(cur, 2, fr["pyr_down"])
    maps = PR.map_pyramid(fr["map2"], 2)
    base = dict(min_obs=1, huber=10.0, eps=1e-4, min_pixels=100, max_iters=10)
    G0, O0 = FR.start_GO()
    top = FR.align_state(fr["pyr2"][1], curp[1], PR.level_K(K, 1), T0, G0, O0, maps[1], **base)
    assert (top["G"], top["O"]) != (G0, O0)
    want = FR.align_state(fr["pyr2"][0], curp[0], K, top["T_ck"], top["G"], top["O"], maps[0], **base)
    got = FR.align_pyr(fr["pyr2"][:2], curp, K, T0, fr["map2"], levels=2)
    ok, where = same_result(got, want)
    assert ok, where
    assert (got["levels"][1]["G"], got["levels"][1]["O"]) == (top["G"], top["O"])


def test_one_iterations_sums_equal_a_python_integer_loop_within_the_bounds(fr):
    y0, x0, h, w = 60, 200, 45, 97  # (a crop: the loop below is plain Python)
    crop = lambda a: np.ascontiguousarray(a[y0:y0 + h, x0:x0 + w])
    key, cur = crop(fr["L"][2]), FR.map_image(crop(fr["L"][3]), 1.3, -20)
    m = {k: crop(fr["map2"][k]) for k in ("invd", "sigma", "n_obs")}
    Kc = (K[0], K[1], K[2] - x0, K[3] - y0)
    T = perturbed(fr["T"][3], 0.3 * np.asarray(XI_START))
    c = AR.constants(key, m, Kc)
    G, O = FR.start_GO(7.9, -250.0)  # (near the range's end: the largest residuals)
    valid, r, wt = FR.residuals(c, cur, Kc, T, G, O, 4.0)
    assert valid.sum() > 500 and np.abs(r).max() > 2 ** 14
    bs = FR.block_sums(c, valid, r, wt)
    want = [[0] * 47 for _ in range(c["n_blocks"])]
    for n in range(len(c["idx"])):
        if not valid[n]:
            continue
        lk16 = 16 * int(key[c["ys"][n], c["xs"][n]])
        rr = int(_sample_one(cur, c, Kc, T, n)) - (((G * lk16 + (1 << 15)) >> 16) + O)
        assert rr == int(r[n]) and abs(rr) < 2 ** 16
        q, ww, row = [int(v) for v in c["q"][n]] + [lk16, 16], int(wt[n]), want[int(c["idx"][n]) // AR.BLOCK]
        for s, (i, j) in enumerate(FR.PAIRS):
            row[s] += ww * q[i] * q[j]
        for i in range(8):
            row[36 + i] += ww * q[i] * rr
        row[44] += ww * rr * rr
        row[45] += ww
        row[46] += 1
    assert all(abs(v) < 2 ** 62 for row in want for v in row[:36]) and all(abs(v) < 2 ** 56 for row in want for v in row[36:44])
    assert all(row[44] < 2 ** 50 for row in want)
    assert bs.tolist() == want
    rng = np.random.default_rng(5)
    assert np.array_equal(FR.block_sums(c, valid, r, wt, rng.permutation(len(c["idx"]))), bs)


def _sample_one(cur, c, Kc, T, n):
    """the sample of pixel n alone, through the plain restatement (whose residual is sample - 16 Lk)"""
    one = {k: (v[n:n + 1] if isinstance(v, np.ndarray) else v) for k, v in c.items()}
    _, r, _ = AR.residuals(one, cur, Kc, T, 255.0)
    return int(r[0]) + int(one["key16"][0])


# ---- plumbing -------------------------------------------------------------------------------------------------------------------------
def test_parameters_and_defaults(vo):
    from visual_odometry_ros_amd import _capi, api
    lib = vo.load()
    p = _capi.SemiDenseAffineParams()
    assert lib.vo_semidense_affine_default_params(C.byref(p)) == 0 and lib.vo_semidense_affine_default_params(None) < 0
    assert (p.gain0, p.offset0) == (FR.DEFAULTS["gain0"], FR.DEFAULTS["offset0"]) == (1.0, 0.0)
    q = api._semidense_affine_params(lib, dict(gain0=0.7))
    assert q.gain0 == F(0.7) and q.offset0 == 0.0 and api._semidense_affine_params(lib, True).gain0 == 1.0
    with pytest.raises(ValueError):
        api._semidense_affine_params(lib, dict(huber=3.0))  # (a field of the alignment's own parameters)
    assert set(api.SEMIDENSE_ALIGN_AFFINE_STATUS) == set(FR.STATUS) == {0, 1, 2, 3, 4, 5} and set(api.SEMIDENSE_ALIGN_STATUS) == {0, 1, 2, 3, 4}
    # the entry points refuse a NULL context and NULL arguments before anything else
    res, ap, a = _capi.SemiDenseAlignAffineResult(), _capi.SemiDenseAlignParams(), _capi.SemiDenseAlignPyrParams()
    assert lib.vo_semidense_align_affine(None, None, 0, 0, 0, None, None, C.byref(ap), C.byref(p), None, None, None, 0, C.byref(res)) < 0
    assert lib.vo_semidense_align_pyr_affine(None, 0, 0, None, None, C.byref(a), C.byref(p), None, None, None, 0, C.byref(res)) < 0
    assert lib.vo_svo_set_semidense_align_affine(None, C.byref(p)) < 0
    assert lib.vo_svo_get_semidense_align_affine(None, C.byref(res), None, None, None) < 0
    # the result structure is the header's: 16 floats, 3 ints (+ padding), 1 + 36 + 8 + 2 doubles, 4 + 18 ints, 6 doubles, 12 ints
    assert C.sizeof(_capi.SemiDenseAlignAffineResult) == 64 + 16 + 8 * 47 + 4 * 22 + 8 * 6 + 4 * 12
    assert api.SemiDenseAligned._fields[-4:] == ("gain", "offset", "G", "O")
