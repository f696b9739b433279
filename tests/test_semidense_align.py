"""The direct image alignment on the semi-dense map (include/vo_hip.h, "Semi-dense alignment"): the definition — as
tests/semidense_align_restatement.py states it — does its job on the synthetic 640 x 240 stream, whose renderer knows the true depth
and whose poses are known: the map seeded at pose 2 and fused with poses 3, 4, 5 (tests/semidense_temporal_restatement.py), the left
images of poses 3, 4, 5 aligned against it with the default parameters. The bounds are the values measured once with the
restatement with the project's margin of a quarter; t = translation distance to the stream's pose in mm, r =
rotation distance in degrees:
  clean map (the renderer's depth at the map's pixels, the stream's own pose as the start): status 0 after 2 / 3 / 3 iterations,
      at t = 0.147 / 0.435 / 0.439 mm, r = 0.0005 / 0.0029 / 0.0022 from the start (what the 1/32 pixel grid, the 1/16 grey level
      and the renderer's interpolation leave);
  perturbed start (the fused map; the start off by xi = (0.03, -0.02, 0.05 m; 0.002, -0.003, 0.001 rad): t = 62.3 / 63.1 / 64.0 mm,
      r = 0.2144): status 0 after 7 / 7 / 7 iterations at t = 0.661 / 0.392 / 0.923 mm, r = 0.0021 / 0.0017 / 0.0039 — 94 / 161 /
      69 times closer in translation, 104 / 123 / 54 times in rotation (the condition: ten times);
      with min_obs = 2: status 0 after 5 / 6 / 6 iterations at t = 1.092 / 1.466 / 1.675 mm, r = 0.0040 / 0.0042 / 0.0111 — 57 / 43 /
      38 and 54 / 51 / 19 times closer.
Exact properties: one iteration's sums equal a direct Python-integer loop over the pixels; shuffling the pixels changes no bit; an
empty map gives status 2; a map of one fronto-parallel row gives status 3 or 2 and never a NaN. Also the parameter helper and the C
defaults. No GPU."""
import ctypes as C

import numpy as np
import pytest

import semidense_align_restatement as AR
import semidense_temporal_restatement as TR
from test_semidense_align_emu import K, XI_START, perturbed, synthetic_setup

F = np.float32
MARGIN = 1.25
# measured with the restatement (see above): per pose 3, 4, 5 (t mm, r degrees)
CLEAN = {3: (0.147, 0.0005), 4: (0.435, 0.0029), 5: (0.439, 0.0022)}
PERTURBED = {1: {3: (0.661, 0.0021), 4: (0.392, 0.0017), 5: (0.923, 0.0039)}, 2: {3: (1.092, 0.0040), 4: (1.466, 0.0042), 5: (1.675, 0.0111)}}


@pytest.fixture(scope="module")
def fr():
    return synthetic_setup()


def distance(T, T_ref):
    """(translation in mm, rotation in degrees) of T_ref^-1 T"""
    E = np.linalg.inv(np.asarray(T_ref, np.float64)) @ np.asarray(T, np.float64)
    R = E[:3, :3]
    s = 0.5 * np.linalg.norm([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])  # sin of the angle (small angles: no arccos)
    return 1e3 * float(np.linalg.norm(E[:3, 3])), float(np.degrees(np.arcsin(min(s, 1.0))))


@pytest.mark.parametrize("pose", [3, 4, 5])
def test_clean_map_stays_at_the_true_pose(fr, pose):
    m = fr["map2"]
    has = (m["n_obs"] >= 1) & (m["sigma"] > 0) & (m["invd"] > 0)
    clean = dict(invd=np.where(has, 1.0 / fr["depth2"], 0).astype(F), sigma=m["sigma"], n_obs=m["n_obs"])
    out = AR.align(fr["L"][2], fr["L"][pose], K, fr["T"][pose], clean)
    t, r = distance(out["T_ck"], fr["T"][pose])
    print(f"clean map, pose {pose}: status {out['status']} after {out['iters']} iterations, {out['count']} pixels, rms {out['rms']:.3f}; "
          f"from the start: t = {t:.3f} mm, r = {r:.4f} degrees")
    assert out["status"] == 0 and out["count"] > 20000
    assert t <= MARGIN * CLEAN[pose][0] and r <= MARGIN * CLEAN[pose][1]


@pytest.mark.parametrize("min_obs", [1, 2])
@pytest.mark.parametrize("pose", [3, 4, 5])
def test_perturbed_start_comes_back(fr, pose, min_obs):
    T0 = perturbed(fr["T"][pose], XI_START)
    t0, r0 = distance(T0, fr["T"][pose])
    out = AR.align(fr["L"][2], fr["L"][pose], K, T0, fr["map2"], min_obs=min_obs)
    t, r = distance(out["T_ck"], fr["T"][pose])
    print(f"perturbed start, pose {pose}, min_obs {min_obs}: start t = {t0:.1f} mm, r = {r0:.4f}; status {out['status']} after {out['iters']} "
          f"iterations, {out['count']} pixels, rms {out['rms']:.3f}: t = {t:.3f} mm, r = {r:.4f} degrees; {t0 / t:.0f} x, {r0 / r:.0f} x")
    assert out["status"] in (0, 1) and out["count"] > 10000
    assert 10 * t <= t0 and 10 * r <= r0  # the condition: ten times closer in translation and in rotation
    assert t <= MARGIN * PERTURBED[min_obs][pose][0] and r <= MARGIN * PERTURBED[min_obs][pose][1]


# ---- exactness ----------------------------------------------------------------------------------------------------------------------
def test_one_iterations_sums_equal_a_python_integer_loop_and_no_order_shows(fr):
    y0, x0, h, w = 60, 200, 45, 97  # (a crop: the loop below is plain Python)
    crop = lambda a: np.ascontiguousarray(a[y0:y0 + h, x0:x0 + w])
    key, cur = crop(fr["L"][2]), crop(fr["L"][3])
    m = {k: crop(fr["map2"][k]) for k in ("invd", "sigma", "n_obs")}
    Kc = (K[0], K[1], K[2] - x0, K[3] - y0)
    T = perturbed(fr["T"][3], 0.3 * np.asarray(XI_START))
    c = AR.constants(key, m, Kc)
    valid, r, wt = AR.residuals(c, cur, Kc, T, 4.0)
    assert valid.sum() > 500 and (wt[valid] != 256).sum() > 50
    bs = AR.block_sums(c, valid, r, wt)
    want = [[0] * 30 for _ in range(c["n_blocks"])]
    for n in range(len(c["idx"])):
        if not valid[n]:
            continue
        q, rr, ww, row = [int(v) for v in c["q"][n]], int(r[n]), int(wt[n]), want[int(c["idx"][n]) // AR.BLOCK]
        for s, (i, j) in enumerate(AR.PAIRS):
            row[s] += ww * q[i] * q[j]
        for i in range(6):
            row[21 + i] += ww * q[i] * rr
        row[27] += ww * rr * rr
        row[28] += ww
        row[29] += 1
    assert all(abs(v) < 2 ** 62 for row in want for v in row)
    assert bs.tolist() == want
    rng = np.random.default_rng(5)
    for _ in range(3):  # any order of the pixels, inside a block and across blocks: integer sums
        assert np.array_equal(AR.block_sums(c, valid, r, wt, rng.permutation(len(c["idx"]))), bs)
    # and the result after one iteration is the one these sums give
    Hs, bv, swrr, sw, count = AR.reduce_blocks(bs)
    out = AR.align(key, cur, Kc, T, m, huber=4.0, max_iters=1)
    assert np.array_equal(out["H"], Hs) and np.array_equal(out["b"], bv) and out["count"] == count == int(valid.sum())
    assert out["rms"] == float(np.sqrt(swrr / sw) / 16)


def test_empty_map_and_one_fronto_parallel_row(fr):
    key, cur = fr["L"][2], fr["L"][3]
    out = AR.align(key, cur, K, fr["T"][3], TR.empty_map(key.shape))
    assert (out["status"], out["iters"], out["count"], out["rms"]) == (2, 1, 0, 0.0) and np.array_equal(out["T_ck"], fr["T"][3])
    # one row at one depth: the rotation about x and the translation along y cannot be told apart — the relative pivot test refuses it
    m = TR.empty_map(key.shape)
    m["invd"][120, 100:540] = F(0.1)
    m["sigma"][120, 100:540] = F(0.01)
    m["n_obs"][120, 100:540] = 1
    flat = np.full_like(key, 93)
    for k_img, c_img in ((key, cur), (flat, flat)):  # (a constant image: every gradient 0, H = 0, the first pivot is refused)
        out = AR.align(k_img, c_img, K, fr["T"][3], m)
        assert out["status"] in (2, 3), out["status"]
        assert np.isfinite(out["T_ck"]).all() and np.isfinite(out["H"]).all() and np.isfinite(out["b"]).all()
    assert out["status"] == 3 and out["iters"] == 1 and np.array_equal(out["T_ck"], fr["T"][3])
    out = AR.align(key, cur, K, fr["T"][3], m, min_pixels=1000)
    assert out["status"] == 2


# ---- plumbing -------------------------------------------------------------------------------------------------------------------------
def test_parameters_and_defaults(vo):
    from visual_odometry_ros_amd import _capi, api
    lib = vo.load()
    p = _capi.SemiDenseAlignParams()
    assert lib.vo_semidense_align_default_params(C.byref(p)) == 0 and lib.vo_semidense_align_default_params(None) < 0
    assert set(AR.DEFAULTS) == {f[0] for f in _capi.SemiDenseAlignParams._fields_}
    for k, v in AR.DEFAULTS.items():
        assert getattr(p, k) == (F(v) if isinstance(v, float) else v), k
    q = api._semidense_align_params(lib, dict(min_obs=2, huber=6.5))
    assert (q.min_obs, q.max_iters, q.min_pixels) == (2, 10, 100) and q.huber == F(6.5) and q.eps == F(1e-4)
    with pytest.raises(ValueError):
        api._semidense_align_params(lib, dict(max_search=64))  # (a field of the temporal block only)
    assert set(api.SEMIDENSE_ALIGN_STATUS) == set(AR.STATUS) == {0, 1, 2, 3, 4}
    # the entry points refuse a NULL context and NULL arguments before anything else
    res = _capi.SemiDenseAlignResult()
    assert lib.vo_semidense_align(None, None, 0, 0, 0, None, None, C.byref(p), None, None, None, 0, C.byref(res)) < 0
    assert lib.vo_svo_set_semidense_align(None, C.byref(p)) < 0
    assert lib.vo_svo_get_semidense_align(None, C.byref(res), None, None, None) < 0
    # the result structure is the header's: 16 floats, 3 ints (+ padding), 1 + 21 + 6 doubles
    assert C.sizeof(_capi.SemiDenseAlignResult) == 64 + 16 + 8 * 28
