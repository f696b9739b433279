"""The temporal semi-dense search and fusion (include/vo_hip.h, "Semi-dense temporal"): the definition — as
tests/semidense_temporal_restatement.py states it — does its job on the synthetic stream, whose renderer knows the true depth: the
map seeded from the static result of pose 2 and fused with poses 3, 4, 5 under the stream's own relative poses. Errors are against
the renderer's depth and compared with the static result of the same keyframe. The bounds are the values measured once with the
restatement with a margin of a quarter:
  (a) pixels static accepted and a frame updated: 9779; median |1/invd - z| / z static 0.005664, fused 0.005294 (gain 0.000370);
  (b) pixels static refused for its 60-degree rule with n_obs >= 2: 1327, of which 0.8666 within 5 % of the true depth.
Also: an identity pose, the points list against a direct loop, the parameter helper and the C defaults. No GPU."""
import ctypes as C
import math

import numpy as np
import pytest

import semidense_restatement as SR
import semidense_temporal_restatement as TR

K = (370.72, 370.72, 319.5, 119.5)


@pytest.fixture(scope="module")
def run():
    from visual_odometry_ros_amd.synthetic import StereoStream
    st = StereoStream(width=640, height=240, K=K, seed=2)
    poses = st.poses(6)
    bf = np.float32(K[0] * st.baseline)
    Lk, Rk, depth = st.render_pair(poses[2])
    stat = SR.semidense(Lk, Rk, d_min=0, d_max=67, bf=float(bf))
    seeded = TR.seed(stat["disparity"], stat["sigma_invd"], stat["status"], bf)
    m, steps = seeded, []
    for i in (3, 4, 5):
        Lc, _, _ = st.render_pair(poses[i])
        T_ck = (np.linalg.inv(poses[i]) @ poses[2]).astype(np.float32)
        out = TR.temporal(Lk, Lc, K, T_ck, m)
        steps.append((m, out))
        m = {k: out[k] for k in ("invd", "sigma", "n_obs", "tstatus")}
    return dict(Lk=Lk, Lc=Lc, depth=depth, stat=stat, seeded=seeded, fused=m, steps=steps, bf=bf)


def rel_err(invd, z):
    return np.abs(1.0 / invd.astype(np.float64) - z) / z


def test_a_fusion_improves_what_static_accepted(run):
    sel = (run["stat"]["status"] == 1) & (run["fused"]["n_obs"] >= 2)
    z = run["depth"][sel]
    e_static, e_fused = np.median(rel_err(run["seeded"]["invd"][sel], z)), np.median(rel_err(run["fused"]["invd"][sel], z))
    print(f"(a) pixels {int(sel.sum())}; median relative depth error static {e_static:.6f}, fused {e_fused:.6f}, gain {e_static - e_fused:.6f}")
    assert sel.sum() >= 0.75 * 9779
    assert e_fused < e_static
    assert e_static - e_fused >= 0.75 * 0.000370


def test_b_pixels_static_refuses_for_its_60_degree_rule_enter_the_map(run):
    cand, gx, gy = SR.candidates(run["Lk"])  # (the static candidates: margin, gradient, 60 degrees)
    H, W = gx.shape
    inside = np.zeros((H, W), bool)
    inside[1:H - 1, 8:W - 8] = True
    refused = inside & (gx * gx + gy * gy >= 400) & ~(3 * gx * gx >= gy * gy)
    assert not (refused & cand).any() and not (run["seeded"]["n_obs"][refused] != 0).any()
    new = refused & (run["fused"]["n_obs"] >= 2)
    share = float(np.mean(rel_err(run["fused"]["invd"][new], run["depth"][new]) <= 0.05))
    print(f"(b) refused by static's 60-degree rule {int(refused.sum())}; in the map with n_obs >= 2: {int(new.sum())}; within 5 %: {share:.4f}")
    assert new.sum() >= 0.75 * 1327
    assert share >= 0.75 * 0.8666


def test_c_sigma_shrinks_on_every_updated_pixel(run):
    n = 0
    for before, after in run["steps"]:
        upd = (after["tstatus"] == 1) & (before["sigma"] > 0)
        n += int(upd.sum())
        assert (after["sigma"][upd] < before["sigma"][upd]).all()
        assert (after["n_obs"][upd] == before["n_obs"][upd] + 1).all()
        first = (after["tstatus"] == 1) & (before["sigma"] == 0)
        assert (after["n_obs"][first] == 1).all() and (after["sigma"][first] > 0).all()
        keep = after["tstatus"] != 1
        for k in ("invd", "sigma", "n_obs"):
            assert np.array_equal(after[k][keep], before[k][keep])
    assert n > 10000


def test_identity_pose_is_no_parallax_everywhere(run):
    m = run["seeded"]
    out = TR.temporal(run["Lk"], run["Lc"], K, np.eye(4, dtype=np.float32), m)
    gx, gy = SR.candidates(run["Lk"])[1:]
    H, W = gx.shape
    cand = gx * gx + gy * gy >= 400
    cand[0], cand[-1], cand[:, 0], cand[:, -1] = False, False, False, False
    assert cand.sum() > 10000 and (out["tstatus"][cand] == 7).all() and (out["tstatus"][~cand] == 0).all()
    for k in ("invd", "sigma", "n_obs"):
        assert np.array_equal(out[k].view(np.uint8), m[k].view(np.uint8))


@pytest.mark.parametrize("with_T", [False, True])
def test_map_points_equal_a_direct_loop(run, with_T):
    m = run["fused"]
    T = None
    if with_T:
        a = 0.3
        T = np.array([[math.cos(a), 0, math.sin(a), 1.5], [0, 1, 0, -0.25], [-math.sin(a), 0, math.cos(a), 7.0], [0, 0, 0, 1]], np.float32)
    xyz, sig, pix = TR.map_points(m["invd"], m["sigma"], m["n_obs"], K, T, min_obs=2)
    f = np.float32
    fx, fy, cx, cy = (f(v) for v in K)
    want_xyz, want_sig, want_pix = [], [], []
    H, W = m["n_obs"].shape
    for y in range(H):
        for x in range(W):
            if m["n_obs"][y, x] < 2:
                continue
            z = f(1) / m["invd"][y, x]
            X = [f(f(f(x) - cx) / fx) * z, f(f(f(y) - cy) / fy) * z, z]
            if T is not None:
                X = [f(f(T[k, 0] * X[0]) + f(f(T[k, 1] * X[1]) + f(T[k, 2] * X[2]))) + T[k, 3] for k in range(3)]
            want_xyz.append(X)
            want_sig.append(m["sigma"][y, x])
            want_pix.append((x, y))
    assert len(want_xyz) == len(xyz) > 1000
    assert np.array_equal(np.array(want_xyz, f).view(np.uint32), xyz.view(np.uint32))
    assert np.array_equal(np.array(want_sig, f), sig) and np.array_equal(np.array(want_pix, np.uint16), pix)


def test_parameters_and_defaults(vo):
    from visual_odometry_ros_amd import _capi, api
    lib = vo.load()
    p = _capi.SemiDenseTemporalParams()
    assert lib.vo_semidense_temporal_default_params(C.byref(p)) == 0 and lib.vo_semidense_temporal_default_params(None) < 0
    assert set(TR.DEFAULTS) == {f[0] for f in _capi.SemiDenseTemporalParams._fields_}
    for k, v in TR.DEFAULTS.items():
        assert getattr(p, k) == (np.float32(v) if isinstance(v, float) else v), k
    q = api._semidense_temporal_params(lib, dict(z_max=60.0, max_search=96))
    assert (q.hw, q.hh, q.max_search) == (4, 1, 96) and q.z_max == np.float32(60.0) and q.z_min == np.float32(3.0)
    with pytest.raises(ValueError):
        api._semidense_temporal_params(lib, dict(d_max=64))  # (a field of the static block only)
    # the entry points refuse a NULL context and NULL arguments before anything else
    assert lib.vo_semidense_temporal(None, None, 0, 0, 0, None, None, C.byref(p), None, None, None, None, None, 0) < 0
    assert lib.vo_semidense_map_seed(None, None, None, None, 4, 4, 1.0, None, None, None, None, 0) < 0
    n = C.c_int()
    assert lib.vo_semidense_map_points(None, None, None, None, 4, 4, 0, None, None, 1, 0, None, None, None, C.byref(n)) < 0
    assert lib.vo_svo_set_semidense_temporal(None, C.byref(p)) < 0
    assert lib.vo_svo_get_semidense_map_points(None, 1, 2, 0, None, None, None, C.byref(n), None) < 0
