"""The 5-point RANSAC pose on the device (include/vo_hip.h: vo_five_point_*; MotionEstimator::calcPose5PointsAlgorithm,
motion_estimator.cpp:21-123 + findCorrectRT :205-263): the minimal solver, the RANSAC on noise-free and noisy two-view data, the
documented sample stream and sequential rule restated in numpy, the reference's decomposition restated in numpy, determinism,
failures, allocations, MonoVO with the library's solver against the CPU loop fed the same solver, and the end-to-end runners."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MONO_K = (458.654, 457.296, 367.215, 248.375)
M64 = (1 << 64) - 1


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _rot(axis, ang):
    axis = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    Kx = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return np.eye(3) + np.sin(ang) * Kx + (1 - np.cos(ang)) * Kx @ Kx


def _skew(t):
    return np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]], np.float64)


def _angle(Ra, Rb):
    """Rotation angle of Ra^T Rb from the chord: ||Ra - Rb||_F = 2 sqrt(2) sin(theta / 2). (arccos((tr - 1) / 2) is
    ill-conditioned near 0: float32 rounding of R alone reads as ~1e-4 rad there.)"""
    d = np.linalg.norm(np.asarray(Ra, np.float64) - np.asarray(Rb, np.float64))
    return float(2 * np.arcsin(min(d / (2 * np.sqrt(2)), 1.0)))


def _tangle(ta, tb):
    """Angle between two directions from the chord of the unit vectors (well conditioned near 0)."""
    ta, tb = np.asarray(ta, np.float64), np.asarray(tb, np.float64)
    d = np.linalg.norm(ta / np.linalg.norm(ta) - tb / np.linalg.norm(tb))
    return float(2 * np.arcsin(min(d / 2, 1.0)))


def _sampson(E, x0, x1):
    """include/vo_hip.h §3, the same operations in the same order (float64, rounded to float32)."""
    E = np.asarray(E, np.float64).reshape(9)
    X0, Y0, X1, Y1 = x0[:, 0], x0[:, 1], x1[:, 0], x1[:, 1]
    a = (E[0] * X0 + E[1] * Y0) + E[2]
    b = (E[3] * X0 + E[4] * Y0) + E[5]
    c = (E[6] * X0 + E[7] * Y0) + E[8]
    d = (E[0] * X1 + E[3] * Y1) + E[6]
    e = (E[1] * X1 + E[4] * Y1) + E[7]
    r = (X1 * a + Y1 * b) + c
    with np.errstate(divide="ignore", invalid="ignore"):
        return ((r * r) / (((a * a + b * b) + d * d) + e * e)).astype(np.float32)


def _norm(pts, K):
    pts = np.asarray(pts, np.float32).astype(np.float64)
    fx, fy, cx, cy = (float(np.float32(k)) for k in K)
    return np.stack([(pts[:, 0] - cx) / fx, (pts[:, 1] - cy) / fy], 1)


def _thr(thres_px, K):
    fx, fy = float(np.float32(K[0])), float(np.float32(K[1]))
    t = float(np.float32(thres_px)) / ((fx + fy) / 2.0)
    return np.float32(t * t)


def _two_view(n, outlier_frac, noise_px, seed):
    from visual_odometry_ros_amd import synthetic as S
    d = S.two_view_points(n=n, seed=seed, noise_px=noise_px, outlier_frac=outlier_frac)
    K = d["K"].astype(np.float64)
    X = d["X"].astype(np.float64)
    p0 = np.stack([K[0] * X[:, 0] / X[:, 2] + K[2], K[1] * X[:, 1] / X[:, 2] + K[3]], 1).astype(np.float32)
    T10 = np.linalg.inv(d["T01_true"])
    return p0, d["pts_l"], d["K"], T10[:3, :3], T10[:3, 3], d["is_outlier"]


# ---- the documented sample stream and sequential rule (include/vo_hip.h §4, §6) ------------------------------------------
def _mix(z):
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def _subset(seed, s, n):
    out = []
    for j in range(256):
        k = s * 256 + j
        z = _mix((seed + (k + 1) * 0x9E3779B97F4A7C15) & M64)
        v = ((z >> 32) * n) >> 32
        if v not in out:
            out.append(v)
            if len(out) == 5:
                break
    return out + [-1] * (5 - len(out))


def _update_iters(p, ep, niters):
    p, ep = min(max(p, 0.0), 1.0), min(max(ep, 0.0), 1.0)
    num = max(1.0 - p, np.finfo(np.float64).tiny)
    q = 1.0 - ep
    q2 = q * q
    den = 1.0 - (q2 * q2) * q
    if den < np.finfo(np.float64).tiny:
        return 0
    num, den = np.log(num), np.log(den)
    return niters if (den >= 0 or -num >= niters * (-den)) else int(np.rint(num / den))


def _walk(counts, n, confidence, max_iters):
    """RANSACPointSetRegistrator::run's loop, model by model: counts[s][m] in solver order, -1 past the sample's models."""
    niters, best, bs, bm, it = max_iters, -1, -1, -1, 0
    while it < len(counts) and it < niters:
        for m, c in enumerate(counts[it]):
            if c < 0:
                break
            if c > max(best, 4):
                best, bs, bm = int(c), it, m
                niters = _update_iters(float(np.float32(confidence)), (n - best) / n, niters)
        it += 1
    return it, bs, bm, best


# ---- motion_estimator.cpp:64-127 + findCorrectRT restated (numpy SVD, the oracle's triangulateDLT) ---------------------
def _decompose(E10, p0, p1, K, oracle):
    U, _, Vt = np.linalg.svd(np.asarray(E10, np.float64).reshape(3, 3))
    V = Vt.T
    if np.linalg.det(U) < 0:
        U[:, 2] = -U[:, 2]
    if np.linalg.det(V) < 0:
        V[:, 2] = -V[:, 2]
    W = np.array([[0, -1, 0], [1, 0, 0], [0, 0, 1]], np.float64)
    Ra, Rb = U @ W @ V.T, U @ W.T @ V.T
    t = U[:, 2]
    cands = [(Ra, t), (Ra, -t), (Rb, t), (Rb, -t)]
    best, out = 0, None
    for R, tc in cands:
        d0, d1 = np.zeros(len(p0)), np.zeros(len(p0))
        for i in range(len(p0)):
            X0, X1 = oracle.triangulate_dlt(p0[i], p1[i], R.astype(np.float32), tc.astype(np.float32), K, K)
            d0[i], d1[i] = X0[2], X1[2]
        ch = (d0 > 0) & (d1 > 0)
        if ch.sum() > best:
            best, out = ch.sum(), (R, tc, ch, np.minimum(np.abs(d0), np.abs(d1)))
    return out


@pytest.fixture(scope="module")
def fctx(vo):
    c = vo.Context(device=0, max_width=64, max_height=64, max_points=4096, n_slots=3, max_level=1)
    yield c
    c.close()


def test_minimal_solver(vo, fctx):
    """4096 noise-free configurations (rotation up to 30 degrees, random t, points in front of both cameras): every returned E
    has unit norm and satisfies the five epipolar constraints and the cubic constraints to 1e-7; the true E is among them."""
    rng = np.random.default_rng(11)
    m = 4096
    x0, x1, Et = np.zeros((m, 5, 2)), np.zeros((m, 5, 2)), np.zeros((m, 3, 3))
    for s in range(m):
        R = _rot(rng.normal(size=3), rng.uniform(0, np.radians(30)))
        t = rng.normal(size=3)
        t /= np.linalg.norm(t)
        k = 0
        while k < 5:
            X = np.array([rng.uniform(-3, 3), rng.uniform(-3, 3), rng.uniform(2, 10)])
            X1 = R @ X + t
            if X1[2] <= 0.5:
                continue
            x0[s, k], x1[s, k] = X[:2] / X[2], X1[:2] / X1[2]
            k += 1
        E = _skew(t) @ R
        Et[s] = E / np.linalg.norm(E)
    fp = vo.FivePointRansac(fctx, MONO_K, max_iters=1000)
    E, ns = fp.minimal(x0, x1)
    fp.close()
    assert ns.min() >= 0 and ns.max() <= 10
    found = 0
    for s in range(m):
        h0 = np.concatenate([x0[s], np.ones((5, 1))], 1)
        h1 = np.concatenate([x1[s], np.ones((5, 1))], 1)
        hit = False
        for j in range(ns[s]):
            e = E[s, j]
            assert abs(np.linalg.norm(e) - 1) < 1e-7
            assert np.abs(np.einsum("ij,jk,ik->i", h1, e, h0)).max() < 1e-7
            assert abs(np.linalg.det(e)) < 1e-7
            assert np.abs(2 * e @ e.T @ e - np.trace(e @ e.T) * e).max() < 1e-7
            sg = np.sign(np.sum(e * Et[s]))
            hit |= np.abs(sg * e - Et[s]).max() < 1e-6
        found += hit
    rate = found / m
    print(f"minimal solver: true E recovered in {rate:.4%} of {m} configurations, {ns.mean():.2f} real solutions on average")
    assert rate >= 0.99


@pytest.mark.parametrize("n,frac", [(6, 0.0)] + [(n, f) for n in (100, 1000, 3000) for f in (0.0, 0.3, 0.5)])
def test_ransac_noise_free(vo, fctx, oracle, n, frac):
    """Noise-free pairs (float32 pixels: ~1e-5 px of rounding) at a 0.05 px threshold. (The RANSAC keeps the first model
    with the largest inlier count and does not refine it, as in the reference: at 1 px any model that keeps every point
    within 1 px can win, which is no test of the solver's accuracy)"""
    p0, p1, K, R_t, t_t, _ = _two_view(n, frac, 0.0, seed=100 + n + int(frac * 10))
    TH = 0.05
    fp = vo.FivePointRansac(fctx, K, thres_px=TH)
    ok, R, t, mask, info = fp.estimate(p0, p1)
    fp.close()
    assert ok
    print(f"noise-free n={n} outliers={frac:.0%}: R {_angle(R, R_t):.2e} rad, t {_tangle(t, t_t):.2e} rad")
    assert _angle(R, R_t) < 1e-4 and _tangle(t, t_t) < 1e-3, (_angle(R, R_t), _tangle(t, t_t))
    assert abs(np.linalg.norm(t) - 1) < 1e-5
    x0, x1 = _norm(p0, K), _norm(p1, K)
    thr = _thr(TH, K)
    Et = _skew(t_t) @ R_t
    err = _sampson(Et / np.linalg.norm(Et), x0, x1)
    true_in = err <= thr
    near = np.abs(err.astype(np.float64) - thr) <= 1e-4 * thr
    ch = np.zeros(n, bool)
    for i in range(n):
        X0, X1 = oracle.triangulate_dlt(p0[i], p1[i], R, t, K, K)
        ch[i] = X0[2] > 0 and X1[2] > 0
    want = true_in & ch
    assert np.all((mask == want) | near), np.flatnonzero((mask != want) & ~near)[:10]


def test_ransac_five_points(vo, fctx):
    """n == 5: the first minimal solution, all five points in mask_5p."""
    p0, p1, K, R_t, t_t, _ = _two_view(5, 0.0, 0.0, seed=3)
    fp = vo.FivePointRansac(fctx, K)
    ok, R, t, mask, info = fp.estimate(p0, p1)
    E, ns = fp.minimal(_norm(p0, K)[None], _norm(p1, K)[None])
    fp.close()
    assert ok and ns[0] >= 1
    assert info.n_inliers_5p == 5 and info.iterations == 1 and info.best_sample == 0 and info.models == ns[0]
    assert np.array_equal(np.array(info.E10, np.float32), E[0, 0].reshape(9).astype(np.float32))


NOISY = {}


@pytest.mark.parametrize("n,frac", [(n, f) for n in (500, 1500) for f in (0.1, 0.3, 0.5)])
@pytest.mark.parametrize("seed", [0, 7])
def test_ransac_noisy(vo, fctx, n, frac, seed):
    p0, p1, K, R_t, t_t, _ = _two_view(n, frac, 0.3, seed=200 + n + int(frac * 10))
    fp = vo.FivePointRansac(fctx, K, thres_px=1.0, seed=seed)
    ok, R, t, mask, info = fp.estimate(p0, p1)
    fp.close()
    assert ok
    Et = _skew(t_t) @ R_t
    n_true = int((_sampson(Et / np.linalg.norm(Et), _norm(p0, K), _norm(p1, K)) <= _thr(1.0, K)).sum())
    ra, ta = np.degrees(_angle(R, R_t)), np.degrees(_tangle(t, t_t))
    print(f"noisy n={n} outliers={frac:.0%} seed={seed}: inliers {info.n_inliers_5p} / true E {n_true}, R {ra:.4f} deg, "
          f"t {ta:.3f} deg, {info.iterations} samples")
    assert info.n_inliers_5p >= 0.9 * n_true
    assert ra < 0.5 and ta < 5.0


def test_sequential_rule_and_stream(vo, fctx):
    p0, p1, K, R_t, t_t, _ = _two_view(1000, 0.5, 0.3, seed=5)
    conf = 0.999
    fp = vo.FivePointRansac(fctx, K, thres_px=1.0, confidence=conf, max_iters=1000, seed=12345)
    ok, R, t, mask, info = fp.estimate(p0, p1)
    smp = fp.samples()
    fp.close()
    assert ok and len(smp["subsets"]) == 1000
    want = np.array([_subset(12345, s, 1000) for s in range(1000)], np.int32)
    assert np.array_equal(smp["subsets"], want)
    assert np.array_equal(smp["n_models"], (smp["counts"] >= 0).sum(1))
    assert np.array_equal(smp["best_count"], smp["counts"].max(1))
    it, bs, bm, best = _walk(smp["counts"], 1000, conf, 1000)
    assert (info.iterations, info.best_sample) == (it, bs), (info.iterations, info.best_sample, it, bs)
    assert info.models == int(smp["n_models"][:it].sum())
    err = _sampson(np.array(info.E10, np.float32).astype(np.float64), _norm(p0, K), _norm(p1, K))
    thr = _thr(1.0, K)
    near = int((np.abs(err.astype(np.float64) - thr) <= 1e-4 * thr).sum())
    assert abs(int((err <= thr).sum()) - info.n_inliers_5p) <= near


def test_decomposition_against_numpy(vo, fctx, oracle):
    for n, frac, seed in ((300, 0.3, 1), (800, 0.1, 2)):
        p0, p1, K, R_t, t_t, _ = _two_view(n, frac, 0.3, seed=seed)
        fp = vo.FivePointRansac(fctx, K, thres_px=1.0)
        ok, R, t, mask, info = fp.estimate(p0, p1)
        fp.close()
        assert ok
        E10 = np.array(info.E10, np.float32)
        Rr, tr, ch, depth = _decompose(E10, p0, p1, K, oracle)
        assert np.abs(R - Rr).max() < 1e-5 and np.abs(t - tr).max() < 1e-5
        m5 = _sampson(E10.astype(np.float64), _norm(p0, K), _norm(p1, K)) <= _thr(1.0, K)
        near = depth < 1e-4
        assert np.all((mask == (m5 & ch)) | near)


def test_determinism(vo, fctx):
    p0, p1, K, *_ = _two_view(1500, 0.3, 0.3, seed=9)
    a = vo.FivePointRansac(fctx, K, seed=4)
    b = vo.FivePointRansac(fctx, K, seed=4)
    r1 = a.estimate(p0, p1)
    r2 = a.estimate(p0, p1)
    a.estimate(p1[:700], p0[:700])  # an unrelated call in between
    r3 = a.estimate(p0, p1)
    r4 = b.estimate(p0, p1)
    for r in (r2, r3, r4):
        assert np.array_equal(_bits(r[1]), _bits(r1[1])) and np.array_equal(_bits(r[2]), _bits(r1[2]))
        assert np.array_equal(r[3], r1[3]) and np.array_equal(_bits(np.array(r[4].E10)), _bits(np.array(r1[4].E10)))
        assert (r[4].iterations, r[4].best_sample, r[4].n_inliers) == (r1[4].iterations, r1[4].best_sample, r1[4].n_inliers)
    a.close()
    b.close()


def test_motion_estimator_calc_pose_5_points(vo, fctx):
    """MotionEstimator.calcPose5PointsAlgorithm: thres_5p_ (setThres5p) and the K of the call, the same result as a
    FivePointRansac at that threshold; a new threshold rebuilds the solver, a new K does not need to."""
    p0, p1, K, R_t, t_t, _ = _two_view(800, 0.3, 0.3, seed=21)
    me = vo.MotionEstimator(fctx, False)
    assert me.thres_5p_ == 1.5
    K2 = np.float32([650.0, 640.0, 600.0, 190.0])
    for th, Kc in ((1.5, K), (0.8, K), (0.8, K2)):
        if th != me.thres_5p_:
            me.setThres5p(th)
        ok, R, t, mask = me.calcPose5PointsAlgorithm(p0, p1, Kc)
        fp = vo.FivePointRansac(fctx, Kc, thres_px=th)
        ok2, R2, t2, mask2, _ = fp.estimate(p0, p1)
        fp.close()
        assert ok and ok2
        assert np.array_equal(_bits(R), _bits(R2)) and np.array_equal(_bits(t), _bits(t2)) and np.array_equal(mask, mask2), (th, Kc)
        if Kc is K:
            assert _angle(R, R_t) < np.radians(0.5) and _tangle(t, t_t) < np.radians(5.0)


def test_failures(vo, fctx):
    fp = vo.FivePointRansac(fctx, MONO_K)
    p = np.random.default_rng(0).uniform(0, 400, (4, 2)).astype(np.float32)
    ok, *_ = fp.estimate(p, p + 1)
    assert not ok
    same = np.tile(np.float32([[100.0, 120.0]]), (50, 1))
    ok, R, t, mask, info = fp.estimate(same, same)
    assert not ok or (np.all(np.isfinite(R)) and np.all(np.isfinite(t)))
    ok, R, t, mask, info = fp.estimate(same, same + 3)
    assert not ok or (np.all(np.isfinite(R)) and np.all(np.isfinite(t)))
    fp.close()


def test_allocations(vo):
    c = vo.Context(device=0, max_width=64, max_height=64, max_points=2048, n_slots=3, max_level=1)
    try:
        n0 = c.allocation_count()
        fp = vo.FivePointRansac(c, MONO_K)
        n1 = c.allocation_count()
        assert n1 > n0
        p0, p1, K, *_ = _two_view(1200, 0.3, 0.3, seed=4)
        fp.estimate(p0, p1, K)
        n2 = c.allocation_count()
        for k in range(10):
            fp.estimate(p0[: 600 + 50 * k], p1[: 600 + 50 * k], K)
        assert c.allocation_count() == n2
        fp.close()
    finally:
        c.close()


def _mono_both(vo, oracle, n_frames, parallax_deg=1.0, five_point="object", seed=5, lba=True):
    """tests/test_mono_vo_gpu.py::_run_both with the library's solver on both sides: the device loop wired natively, the CPU loop
    calling the same solver object as its Python hook."""
    from oracle.mono_vo import MonoVORef
    from visual_odometry_ros_amd import synthetic as S
    W, H, nu, nv, win, lvl = 752, 480, 40, 25, 15, 5
    st = S.StereoStream(width=W, height=H, K=MONO_K, n_u=nu, n_v=nv, seed=seed, speed=0.25)
    poses = st.poses(n_frames)
    imgs = [st.render_pair(p)[0] for p in poses]
    c = vo.Context(device=0, max_width=W, max_height=H, max_points=2 * nu * nv + 512, n_slots=3, max_level=lvl)
    out = []
    try:
        solver = vo.FivePointRansac(c, MONO_K, thres_px=2.0)
        ref = MonoVORef(W, H, MONO_K, nu, nv, solver, thres_fast=15, win=win, max_level=lvl, thres_err=20.0, thres_bidir=1.0,
                        thres_poseba=5, thres_sampson=1.0, thres_parallax_deg=parallax_deg, kf_trans=2.5, lba=lba,
                        sum_mode=oracle.SUM_TREE, tree_width=512, ic_border=oracle.IC_REFERENCE, n_threads=8)
        fpo = solver if five_point == "object" else None
        mvo = vo.MonoVO(c, W, H, MONO_K, nu, nv, fpo, thres_fastscore=15, window_size=win, max_level=lvl, thres_error=20.0,
                        thres_bidirection=1.0, thres_poseba_error=5, thres_sampson=1.0, thres_parallax=parallax_deg, thres_translation=2.5,
                        strict_border=1, local_ba=lba)
        for k in range(n_frames):
            gi = mvo.trackImage(imgs[k])
            ri = ref.track(imgs[k])
            g = mvo.getTracks()
            where = f"frame {k}"
            assert gi.frame_id == ri["frame_id"] and bool(gi.is_keyframe) == ri["keyframe"], where
            assert np.array_equal(g["ids"], ref.ids), where
            assert np.array_equal(_bits(g["pts"]), _bits(ref.pts)), where
            assert np.array_equal(g["flags"], ref.flags()), where
            tri = (g["flags"] & 1) != 0
            assert np.array_equal(_bits(g["Xw"][tri]), _bits(ref.Xw()[tri])), where
            assert np.array_equal(_bits(np.array(gi.T_wc).reshape(4, 4)), _bits(ref.frames[k]["T_wc"])), where
            assert bool(gi.used_five_point) == ri["five_point"], where
            out.append((bool(gi.is_keyframe), bool(gi.lba_ran), bool(gi.used_five_point), np.array(gi.dT01, np.float32).reshape(4, 4),
                        np.array(gi.T_wc, np.float32).reshape(4, 4)))
        mvo.close()
        solver.close()
        return out, poses
    finally:
        c.close()


def test_mono_loop_with_the_library_solver(vo, oracle):
    log, poses = _mono_both(vo, oracle, 24)
    assert log[1][2] and sum(e[0] for e in log) >= 4 and sum(e[1] for e in log) >= 2
    # the initialisation's motion against the scene's (t up to scale)
    T10 = np.linalg.inv(poses[1]) @ poses[0]
    dT10 = np.linalg.inv(log[1][3].astype(np.float64))
    ra, ta = np.degrees(_angle(dT10[:3, :3], T10[:3, :3])), np.degrees(_tangle(dT10[:3, 3], T10[:3, 3]))
    print(f"initialisation: R {ra:.4f} deg, t {ta:.3f} deg from the scene's relative pose")
    assert ra < 0.5 and ta < 5.0


def test_mono_loop_fallback_with_the_library_solver(vo, oracle):
    log, _ = _mono_both(vo, oracle, 8, parallax_deg=80.0)
    assert all(e[2] for e in log[1:])


def test_mono_default_solver_equals_explicit(vo, oracle):
    a, _ = _mono_both(vo, oracle, 6, five_point="object")
    b, _ = _mono_both(vo, oracle, 6, five_point=None)
    for ea, eb in zip(a, b):
        assert np.array_equal(_bits(ea[4]), _bits(eb[4]))


def test_mono_init_fails_like_a_failing_hook(vo):
    """Fewer than five landmarks reach the second image: the library's solver fails (n < 5) and MonoVO's initialisation fails with
    VO_ERR_GN_FAILED, as it does for a hook that returns 0."""
    W, H = 320, 240
    img = np.full((H, W), 90, np.uint8)
    for (x, y) in ((100, 100), (180, 100), (140, 170)):  # three bright squares in three bins, clear of ORB's border: <= 3 landmarks
        img[y:y + 16, x:x + 16] = 230
    codes = []
    for hook in ("solver", lambda a, b: (False, np.eye(3), np.zeros(3), np.zeros(len(a), bool))):
        c = vo.Context(device=0, max_width=W, max_height=H, max_points=512, n_slots=3, max_level=2)
        try:
            mvo = vo.MonoVO(c, W, H, (300.0, 300.0, 160.0, 120.0), 4, 3, None if hook == "solver" else hook, window_size=15,
                            max_level=2, local_ba=False)
            i0 = mvo.trackImage(img)
            assert 1 <= i0.n_tracks_out < 5, i0.n_tracks_out
            with pytest.raises(vo.VoError) as e:
                mvo.trackImage(img)
            codes.append(e.value.code)
            mvo.close()
        finally:
            c.close()
    assert codes == [-9, -9]


def test_from_yaml_mono0(vo):
    from visual_odometry_ros_amd import config
    from visual_odometry_ros_amd import synthetic as S
    path = os.path.join(ROOT, "tests", "golden", "reference_config", "mono", "mono0.yaml")
    cfg = config.load_mono_config(path)
    cam = cfg["camera"]
    mvo = vo.MonoVO.from_yaml(path, strict_border=1)
    try:
        st = S.StereoStream(width=cam["width"], height=cam["height"], K=tuple(float(k) for k in cam["K"]), n_u=32, n_v=20, seed=3,
                            speed=0.25)
        infos = [mvo.trackImage(st.render_pair(p)[0]) for p in st.poses(12)]
        assert infos[1].is_init and infos[1].used_five_point
        assert infos[-1].n_tracks_out > 100 and np.all(np.isfinite(np.array(infos[-1].T_wc)))
    finally:
        mvo.close()


def test_run_mono_sequence_example(vo, tmp_path):
    PIL = pytest.importorskip("PIL.Image")
    from visual_odometry_ros_amd import synthetic as S
    W, H, K = 640, 240, (400.0, 400.0, 320.0, 120.0)
    st = S.StereoStream(width=W, height=H, K=K, n_u=20, n_v=8, seed=7, speed=0.3)
    d = tmp_path / "image_0"
    d.mkdir()
    n = 10
    for k, p in enumerate(st.poses(n)):
        PIL.fromarray(st.render_pair(p)[0]).save(d / f"{k:06d}.png")
    cfg = tmp_path / "mono.yaml"
    cfg.write_text("%YAML:1.0\nflagDoUndistortion: 0\n" + "".join(f"Camera.{k}: {v}\n" for k, v in (
        ("fx", K[0]), ("fy", K[1]), ("cx", K[2]), ("cy", K[3]), ("k1", 0.0), ("k2", 0.0), ("p1", 0.0), ("p2", 0.0), ("k3", 0.0),
        ("width", W), ("height", H))) +
        "feature_tracker.thres_error: 20.0\nfeature_tracker.thres_bidirection: 1.0\nfeature_tracker.thres_sampson: 1.0\n"
        "feature_tracker.window_size: 15\nfeature_tracker.max_level: 4\nmap_update.thres_parallax: 1.0\n"
        "feature_extractor.n_features: 2000\nfeature_extractor.n_bins_u: 20\nfeature_extractor.n_bins_v: 8\n"
        "feature_extractor.thres_fastscore: 15.0\nfeature_extractor.radius: 5.0\nmotion_estimator.thres_1p_error: 10.0\n"
        "motion_estimator.thres_5p_error: 2.0\nmotion_estimator.thres_poseba_error: 5.0\nkeyframe_update.thres_translation: 2.5\n"
        "keyframe_update.thres_rotation: 3.0\nkeyframe_update.thres_overlap_ratio: 0.7\nkeyframe_update.n_max_keyframes_in_window: 9\n")
    out, kf = tmp_path / "traj.txt", tmp_path / "kf.txt"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "run_mono_sequence.py"), "--config", str(cfg), "--images", str(d),
                        "--trajectory", str(out), "--keyframes", str(kf)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-1500:]
    lines = out.read_text().strip().splitlines()
    assert len(lines) == n
    assert all(len(l.split()) == 13 for l in lines)


def test_cpp_mono_vo_with_the_library_solver(vo, tmp_path):
    """tests/cpp/five_point_demo.cpp: vo::MonoVO(ctx, params) with the native solver, through the C++ surface only."""
    from visual_odometry_ros_amd import synthetic as S
    libdir = os.path.join(ROOT, "visual_odometry_ros_amd", "lib")
    exe = str(tmp_path / "five_point_demo")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I", ROOT, os.path.join(ROOT, "tests", "cpp", "five_point_demo.cpp"), "-o", exe,
                           "-L", libdir, "-lvo_hip", f"-Wl,-rpath,{libdir}", "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib", "-lamdhip64"])
    W, H, K = 640, 240, (400.0, 400.0, 320.0, 120.0)
    st = S.StereoStream(width=W, height=H, K=K, n_u=20, n_v=8, seed=7, speed=0.3)
    raw = tmp_path / "frames.u8"
    poses = st.poses(8)
    with open(raw, "wb") as f:
        for p in poses:
            f.write(np.ascontiguousarray(st.render_pair(p)[0]).tobytes())
    r = subprocess.run([exe, str(raw), str(W), str(H), str(len(poses))] + [str(k) for k in K], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-1500:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("frame")]
    assert len(lines) == len(poses)
    assert "four pairs -> 0" in r.stdout.splitlines()
    assert "init 1" in lines[1] and "five_point 1" in lines[1]
