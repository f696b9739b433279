"""The coarse-to-fine alignment on a map pyramid (include/vo_hip.h, "Semi-dense alignment on a map pyramid"): the definition — as
tests/semidense_align_pyr_restatement.py states it — does its job on the synthetic 640 x 240 stream: the map seeded at pose 2 and
fused with poses 3, 4, 5, the left images of poses 3, 4, 5 aligned against it FROM THE IDENTITY (800 / 1600 / 2400 mm off), where the
level-0 operator of DESIGN.md §20 does not converge and is not meant to. Both conditions are stated against that operator:
  the level-0 restatement with max_iters = 32 stays more than ten times farther from the stream's pose than the pyramid ends;
  the pyramid (the defaults: 4 levels, 10 iterations each) ends within twice the end point §20's table records for the close
      perturbed start (0.661 / 0.392 / 0.923 mm, 0.0021 / 0.0017 / 0.0039 degrees).
Measured once with the restatement, asserted with the project's margin of a quarter; t = translation distance to the
stream's pose in mm, r = rotation distance in degrees:
  from the identity: level 0 alone, 32 iterations: status 1 at t = 519.7 / 1495.0 / 2339.3 mm; the pyramid: status 0 after 2 / 3 / 3
      level-0 iterations at t = 0.657 / 0.391 / 0.939 mm, r = 0.0020 / 0.0017 / 0.0040; the levels 3, 2, 1 took 10, 4, 3 / 10, 7, 4 /
      10, 10, 4 iterations (the top level always ends with status 1) over 1948 / 7470 / 20726 / 28733 pixels at pose 3;
  from 5 x §20's perturbation (312 - 320 mm, 1.07 degrees): t = 0.663 / 0.389 / 0.935 mm, r = 0.0021 / 0.0017 / 0.0040.
Exact properties: levels = 1 is the level-0 operator bit for bit; an empty map gives status 2 at every level and the start as the
pose; a top level below min_pixels hands its pose down and the next level runs; the map pyramid of one valid pixel, and of a map
with non-finite and denormal entries, holds no NaN. Also the parameter helper and the C defaults. No GPU."""
import ctypes as C

import numpy as np
import pytest

import semidense_align_pyr_restatement as PR
import semidense_align_restatement as AR
import semidense_temporal_restatement as TR
from test_semidense_align import PERTURBED, distance
from test_semidense_align_emu import K, XI_START, perturbed, same_result, synthetic_setup

F = np.float32
MARGIN = 1.25
I4 = np.eye(4, dtype=F)
# measured with the restatement (see above): per pose 3, 4, 5 (t mm, r degrees)
FROM_IDENTITY = {3: (0.657, 0.0021), 4: (0.391, 0.0017), 5: (0.939, 0.0040)}
FROM_5X = {3: (0.663, 0.0021), 4: (0.389, 0.0017), 5: (0.935, 0.0040)}


@pytest.fixture(scope="module")
def fr(oracle):
    d = dict(synthetic_setup())
    d["pyr"] = {i: PR.image_pyramid(d["L"][i], 4, oracle.pyr_down) for i in (2, 3, 4, 5)}
    return d


@pytest.mark.parametrize("pose", [3, 4, 5])
def test_from_the_identity_the_pyramid_converges_where_level_0_cannot(fr, pose):
    T_ref = fr["T"][pose]
    t0, r0 = distance(I4, T_ref)
    lone = AR.align(fr["L"][2], fr["L"][pose], K, I4, fr["map2"], max_iters=32)
    tl, rl = distance(lone["T_ck"], T_ref)
    out = PR.align_pyr(fr["pyr"][2], fr["pyr"][pose], K, I4, fr["map2"])
    t, r = distance(out["T_ck"], T_ref)
    print(f"pose {pose}: the identity is {t0:.1f} mm, {r0:.4f} degrees off; level 0 alone: status {lone['status']} after {lone['iters']} iterations "
          f"at t = {tl:.1f} mm, r = {rl:.4f}; 4 levels: status {out['status']} at t = {t:.3f} mm, r = {r:.4f}; per level (0 first) "
          f"{[(d['status'], d['iters'], d['count']) for d in out['levels']]}")
    assert tl > 10 * t  # the level-0 operator stays more than ten times farther away than the pyramid ends
    t20, r20 = PERTURBED[1][pose]  # §20's end point from the close perturbed start
    assert t <= 2 * t20 and r <= 2 * r20
    assert out["status"] in (0, 1) and out["count"] > 10000
    assert t <= MARGIN * FROM_IDENTITY[pose][0] and r <= MARGIN * FROM_IDENTITY[pose][1]


@pytest.mark.parametrize("pose", [3, 4, 5])
def test_from_five_times_the_perturbation(fr, pose):
    T0 = perturbed(fr["T"][pose], 5 * np.asarray(XI_START))
    out = PR.align_pyr(fr["pyr"][2], fr["pyr"][pose], K, T0, fr["map2"])
    t, r = distance(out["T_ck"], fr["T"][pose])
    print(f"pose {pose}: start {distance(T0, fr['T'][pose])}; status {out['status']} after {out['iters']} level-0 iterations at t = {t:.3f} mm, r = {r:.4f}")
    assert out["status"] == 0 and out["iters"] <= 4
    assert t <= MARGIN * FROM_5X[pose][0] and r <= MARGIN * FROM_5X[pose][1]


# ---- exactness ----------------------------------------------------------------------------------------------------------------------
def test_one_level_is_the_level_0_operator_bit_for_bit(fr):
    T0 = perturbed(fr["T"][3], XI_START)
    for prm in (dict(), dict(min_obs=2, huber=6.0, max_iters=3)):
        want = AR.align(fr["L"][2], fr["L"][3], K, T0, fr["map2"], **prm)
        got = PR.align_pyr(fr["pyr"][2][:1], fr["pyr"][3][:1], K, T0, fr["map2"], levels=1, **prm)
        ok, where = same_result(got, want)
        assert ok, where
        assert got["levels"] == [{k: want[k] for k in ("status", "iters", "count", "rms")}]
        # max_iters_level[0] names level 0's iterations
        got = PR.align_pyr(fr["pyr"][2][:1], fr["pyr"][3][:1], K, T0, fr["map2"], levels=1, **dict(prm, max_iters=9, max_iters_level=(want["iters"],)))
        ok, where = same_result(got, AR.align(fr["L"][2], fr["L"][3], K, T0, fr["map2"], **dict(prm, max_iters=want["iters"])))
        assert ok, where


def test_an_empty_map_gives_status_2_at_every_level(fr):
    T0 = fr["T"][3]
    out = PR.align_pyr(fr["pyr"][2], fr["pyr"][3], K, T0, TR.empty_map(fr["L"][2].shape))
    assert [(d["status"], d["iters"], d["count"], d["rms"]) for d in out["levels"]] == [(2, 1, 0, 0.0)] * 4
    assert out["status"] == 2 and np.array_equal(out["T_ck"], T0) and not out["H"].any()


def test_a_level_with_too_few_pixels_hands_its_pose_down(fr):
    maps = PR.map_pyramid(fr["map2"], 4)
    n = [len(AR.constants(fr["pyr"][2][l], maps[l], PR.level_K(K, l))["idx"]) for l in range(4)]
    assert n[3] < n[2] < n[1] < n[0]
    T0 = perturbed(fr["T"][3], XI_START)
    out = PR.align_pyr(fr["pyr"][2], fr["pyr"][3], K, T0, fr["map2"], min_pixels=n[3] + 1)
    assert out["levels"][3]["status"] == 2 and out["levels"][3]["iters"] == 1 and 0 < out["levels"][3]["count"] <= n[3]
    assert out["levels"][2]["status"] in (0, 1) and out["levels"][2]["iters"] > 1 and out["status"] == 0
    # ... and the levels below run from the start the top level was given: the same bits as three levels
    want = PR.align_pyr(fr["pyr"][2][:3], fr["pyr"][3][:3], K, T0, fr["map2"], levels=3, min_pixels=n[3] + 1)
    ok, where = same_result(out, want)
    assert ok, where
    assert out["levels"][:3] == want["levels"]


def test_the_map_pyramid_holds_no_nan():
    h, w = 21, 34
    one = TR.empty_map((h, w))
    one["invd"][7, 12], one["sigma"][7, 12], one["n_obs"][7, 12] = F(0.25), F(0.02), 3
    lv = PR.map_pyramid(one, 4)
    assert [x["invd"].shape for x in lv] == [(21, 34), (11, 17), (6, 9), (3, 5)]
    for l in (1, 2, 3):
        assert all(np.isfinite(lv[l][k]).all() for k in ("invd", "sigma"))
    # (12, 7) is a child of the coarse pixels around (6, 3.5): x = 6 exactly, y = 3 and 4
    assert sorted(zip(*np.nonzero(lv[1]["n_obs"]))) == [(3, 6), (4, 6)] and (lv[1]["n_obs"][lv[1]["n_obs"] > 0] == 3).all()
    assert (lv[1]["invd"][lv[1]["n_obs"] > 0] == F(0.25)).all() and np.allclose(lv[1]["sigma"][lv[1]["n_obs"] > 0], 0.02, rtol=1e-6)
    assert lv[3]["n_obs"].any()
    # non-finite and extreme entries: a child with a non-finite sigma or invd does not count; a denormal sigma (1 / sigma^2 = inf)
    # leaves S infinite and the coarse pixel empty
    rng = np.random.default_rng(3)
    m = dict(invd=rng.uniform(0.05, 1.0, (h, w)).astype(F), sigma=rng.uniform(0.001, 0.1, (h, w)).astype(F), n_obs=rng.integers(0, 4, (h, w)).astype(np.uint8))
    m["sigma"][3, 3], m["sigma"][3, 4], m["sigma"][10, 20], m["invd"][5, 9], m["invd"][6, 9] = np.nan, np.inf, F(1e-42), np.inf, np.nan
    m["sigma"][15, 7], m["invd"][16, 30], m["invd"][12, 2] = F(-1.0), F(-0.5), F(3e38)
    m["n_obs"][3, 3:5] = m["n_obs"][10, 20] = m["n_obs"][5:7, 9] = m["n_obs"][15, 7] = m["n_obs"][16, 30] = m["n_obs"][12, 2] = 1
    lv = PR.map_pyramid(m, 4)
    for l in (1, 2, 3):
        assert not any(np.isnan(lv[l][k]).any() for k in ("invd", "sigma")), l
        has = lv[l]["n_obs"] > 0
        assert ((lv[l]["sigma"] > 0) == has).all() and ((lv[l]["invd"] > 0) == has).all() and np.isfinite(lv[l]["sigma"]).all()
    assert lv[1]["n_obs"][5, 10] == 0 and lv[1]["sigma"][5, 10] == 0 and lv[1]["invd"][5, 10] == 0  # (the denormal sigma's coarse pixel)
    # a direct scalar loop over one level, operation by operation
    fine, got = lv[0], lv[1]
    for Y in range(got["invd"].shape[0]):
        for X in range(got["invd"].shape[1]):
            S = N = F(0)
            n = top = 0
            with np.errstate(all="ignore"):
                for dy in (-1, 0, 1):
                    for dx in (-1, 0, 1):
                        y, x = 2 * Y + dy, 2 * X + dx
                        if not (0 <= y < h and 0 <= x < w):
                            continue
                        sg, iv, no = fine["sigma"][y, x], fine["invd"][y, x], int(fine["n_obs"][y, x])
                        if no >= 1 and sg > 0 and iv > 0 and np.isfinite(sg) and np.isfinite(iv):
                            wt = F(1) / F(sg * sg)
                            S, N, n, top = F(S + wt), F(N + F(wt * iv)), n + 1, max(top, no)
                ok = n > 0 and np.isfinite(S) and S > 0
                want = (F(N / S), F(np.sqrt(F(F(n) / S))), top) if ok else (F(0), F(0), 0)
            assert (got["invd"][Y, X].tobytes(), got["sigma"][Y, X].tobytes(), int(got["n_obs"][Y, X])) == (want[0].tobytes(), want[1].tobytes(), want[2]), (X, Y)


# ---- plumbing -------------------------------------------------------------------------------------------------------------------------
def test_parameters_and_defaults(vo):
    from visual_odometry_ros_amd import _capi, api
    lib = vo.load()
    p = _capi.SemiDenseAlignPyrParams()
    assert lib.vo_semidense_align_pyr_default_params(C.byref(p)) == 0 and lib.vo_semidense_align_pyr_default_params(None) < 0
    assert set(PR.DEFAULTS) == {f[0] for f in _capi.SemiDenseAlignPyrParams._fields_}
    for k, v in PR.DEFAULTS.items():
        got = getattr(p, k)
        assert (tuple(got) == tuple(v)) if k == "max_iters_level" else (got == (F(v) if isinstance(v, float) else v)), k
    assert PR.MAX_LEVELS == len(p.max_iters_level) == 6
    q = api._semidense_align_pyr_params(lib, dict(levels=3, huber=6.5, max_iters_level=(2, 0, 12)))
    assert (q.levels, q.max_iters, tuple(q.max_iters_level)) == (3, 10, (2, 0, 12, 0, 0, 0)) and q.huber == F(6.5)
    for bad in (dict(max_search=64), dict(max_iters_level=(1,) * 7), dict(start="previous")):  # (start is the driver's, not a field)
        with pytest.raises(ValueError):
            api._semidense_align_pyr_params(lib, bad)
    assert api.SEMIDENSE_ALIGN_START == {"odometry": 0, "previous": 1}
    n = C.c_longlong()
    assert lib.vo_semidense_map_pyramid_size(203, 61, 3, C.byref(n)) == 0 and n.value == 102 * 31 + 51 * 16
    assert lib.vo_semidense_map_pyramid_size(203, 61, 1, C.byref(n)) == 0 and n.value == 0
    assert lib.vo_semidense_map_pyramid_size(203, 61, 7, C.byref(n)) < 0 and lib.vo_semidense_map_pyramid_size(203, 61, 3, None) < 0
    # the entry points refuse a NULL context and NULL arguments before anything else
    res = _capi.SemiDenseAlignPyrResult()
    assert lib.vo_semidense_align_pyr(None, 0, 1, None, None, C.byref(p), None, None, None, 0, C.byref(res)) < 0
    assert lib.vo_semidense_map_pyramid(None, None, None, None, 8, 8, 2, None, None, None, 0) < 0
    assert lib.vo_svo_set_semidense_align_pyr(None, C.byref(p), 0) < 0
    assert lib.vo_svo_get_semidense_align_pyr(None, C.byref(res), None, None, None) < 0
    # the result structure is the header's: the level-0 result, then 2 + 18 ints and 6 doubles
    assert C.sizeof(_capi.SemiDenseAlignPyrResult) == C.sizeof(_capi.SemiDenseAlignResult) + 4 * 20 + 8 * 6
    assert _capi.SemiDenseAlignPyrResult.levels.offset == C.sizeof(_capi.SemiDenseAlignResult)
