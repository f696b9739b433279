"""The inputs of tests/test_rig_gpu.py, checked on the CPU with the oracle alone: a stereo rig of two different cameras
(K_r != K_l, fx != fy in both) whose right camera is rotated and shifted along all three axes (util.RIG_*). For each
input: the helpers that build it reproduce the plain-rig generators bit for bit when they are given the plain rig; the
oracle solves it (against a float64-generated truth where there is one); and it tells a wrong kernel from a right one —
every mistake of util.RIG_MUTANTS changes an output that the device tests compare, where on the plain rig of the older
tests three of the five change nothing at all."""
import hashlib

import numpy as np
import pytest

import util as U
from visual_odometry_ros_amd import synthetic as S

GN_SEED = U.RIG_GN_SEED  # seeds at which the TREE and the SEQ inlier masks are equal (asserted below)
FRAME_STREAM = dict(n_u=8, n_v=5, n_new=10, seed=4)  # 40 features at 320 x 200; margin 5 (strict border) or 16
LOOP_STREAM = dict(n_u=20, n_v=8, seed=5, speed=0.5)   # 640 x 240, 12 frames
# integer outputs of the pose-only BA (mask, iterations, cnt_invalid): the smallest n of RIG_GN_COUNTS from which on each
# mutant changes them. Dropping t_y, t_z moves a right pixel by fy * 0.011 / Z <= 2 px, under the 3 px inlier threshold:
# it flips a point on the threshold only where there are thousands; below that it shows in the pose (next table)
GN_SEEN_FROM = {"K_l <-> K_r": 1, "R_lr transposed": 1, "T_lr inverted": 1, "t_y = t_z = 0": 2047, "fx <-> fy right": 37}


def _digest(d):
    h = hashlib.sha256()
    for k in sorted(d):
        a = np.ascontiguousarray(d[k])
        for part in (k.encode(), str(a.dtype).encode(), str(a.shape).encode(), a.tobytes()):
            h.update(part)
    return h.hexdigest()[:16]


def _rel_frob(A, B):
    return np.linalg.norm(np.asarray(A, np.float64) - np.asarray(B, np.float64)) / np.linalg.norm(B)


def _same(a, b):
    return a.keys() == b.keys() and all(np.array_equal(a[k], b[k]) and np.asarray(a[k]).dtype == np.asarray(b[k]).dtype for k in a)


# ---- the helpers on the plain rig ---------------------------------------------------------------------------------------
def test_plain_rig_two_view_is_bit_identical():
    assert np.array_equal(U.plain_T_lr().astype(np.float32), S.stereo_T_lr())
    for n, seed, kw in ((500, 1, {}), (37, 3, {}), (3000, 4, {}), (800, 11, dict(noise_px=0.0, outlier_frac=0.0))):
        a = S.two_view_points(n=n, seed=seed, **kw)
        b = U.rig_two_view(n=n, seed=seed, K_l=S.KITTI_K, K_r=S.KITTI_K, T_lr=U.plain_T_lr(), **kw)
        assert np.array_equal(b.pop("Kr"), a["K"])
        assert _same(a, b), (n, seed)


@pytest.mark.parametrize("shape", ["small", "kitti"])
def test_plain_rig_stream_is_bit_identical(shape):
    kw = dict(width=320, height=200, K=(300.0, 300.0, 160.0, 100.0), n_u=8, n_v=5, n_new=10, seed=7, margin=5.0) if shape == "small" \
        else dict(n_u=12, n_v=5, n_new=20, seed=2, margin=4.0)  # 1241 x 376, KITTI_K, KITTI_BASELINE
    a = S.StereoStream(**kw)
    K = kw.pop("K", S.KITTI_K)
    b = U.RigStream(K, K, U.plain_T_lr(), **kw)
    assert b.Kr == a.K == b.K and np.array_equal(b.T_lr, a.T_lr) and b.T_lr.dtype == a.T_lr.dtype
    assert (b.width, b.height, b.baseline) == (a.width, a.height, a.baseline)
    poses = a.poses(3)
    assert all(np.array_equal(p, q) for p, q in zip(poses, b.poses(3)))
    for k in (0, 1):
        assert _same(a.track_set(k, poses[k], poses[k + 1]), b.track_set(k, poses[k], poses[k + 1])), k
    assert all(np.array_equal(x, y) for x, y in zip(a.render_pair(poses[1]), b.render_pair(poses[1])))


def test_ba_window_without_right_intrinsics_is_unchanged():
    """synthetic.ba_window gained the optional Kr: without it, and with Kr = K, the arrays are the ones it gave before
    (digests taken from the version without the argument)."""
    T = S.se3_exp([0.537, 0.004, -0.003, 0.02, -0.015, 0.01])
    for kw, want in ((dict(n_kf=6, n_points=300, stereo=True, seed=21), "5e8cb21052d91f20"),
                     (dict(n_kf=6, n_points=400, stereo=True, seed=3, right_only_frac=0.3), "63c78825dda29b67"),
                     (dict(n_kf=5, n_points=200, stereo=False, seed=4), "ab5e0b42ea55361f"),
                     (dict(n_kf=6, n_points=400, stereo=True, seed=2, T_lr=T), "be49f5d898e1b7ce")):
        p = S.ba_window(**kw)
        assert _digest(p) == want, kw
        q = S.ba_window(Kr=S.KITTI_K, **kw)
        assert np.array_equal(q.pop("Kr"), p["K"]) and _same(p, q), kw


def test_ba_window_projects_right_observations_with_right_intrinsics():
    p = U.rig_ba_window(n_kf=4, n_points=80, stereo=True, seed=6, px_noise=0.0)
    T_rl = U.se3_inverse64(U.rig_T_lr())
    lm = np.repeat(np.arange(len(p["obs_ptr"]) - 1), np.diff(p["obs_ptr"]))
    T_jw = p["T_jw_true"][p["obs_frame"]]
    Xc = (np.einsum("nij,nj->ni", T_jw[:, :3, :3], p["X_true"][lm]) + T_jw[:, :3, 3]) / 0.1  # back to metres
    right = p["obs_right"] == 1
    assert right.sum() > 100 and (~right).sum() > 100
    assert np.abs(U.project64(Xc[~right], np.eye(4), U.RIG_KITTI["K_l"]) - p["obs_px"][~right]).max() < 1e-9
    assert np.abs(U.project64(Xc[right], T_rl, U.RIG_KITTI["K_r"]) - p["obs_px"][right]).max() < 1e-9
    assert np.abs(U.project64(Xc[right], T_rl, U.RIG_KITTI["K_l"]) - p["obs_px"][right]).max() > 3.0  # and not with K_l


# ---- pose-only BA ----------------------------------------------------------------------------------------------------------
def _gn(oracle, d, T0, mode, rig=None):
    Kl, Kr, T_lr = (d["K"], d["Kr"], d["T_lr"]) if rig is None else rig
    return oracle.gn_pose_stereo(d["X"], d["pts_l"], d["pts_r"], Kl, Kr, np.asarray(T_lr, np.float32), 3.0, T0,
                                 mode, 512 if mode == oracle.SUM_TREE else 0)


def _gn_ints(r):
    return r[0], r[2].tolist(), r[3].iterations, r[3].cnt_invalid


@pytest.mark.parametrize("identity", [True, False])
def test_gn_noise_free_recovers_the_float64_truth(oracle, identity):
    """The truth is generated in float64, without the oracle: this pins the oracle's general-rig arithmetic."""
    d = U.rig_two_view(n=800, seed=11, noise_px=0.0, outlier_frac=0.0)
    for mode in (oracle.SUM_TREE, oracle.SUM_SEQ):
        rc, T, mask, _ = _gn(oracle, d, U.rig_gn_T0(d, identity), mode)
        dev = np.abs(T - d["T01_true"]).max()
        print(f"noise-free, T0 identity {identity}, mode {mode}: |T - T_true| max {dev:.2e}")
        assert rc == 1 and mask.all() and dev < 1e-5


@pytest.mark.parametrize("n", U.RIG_GN_COUNTS)
def test_gn_point_counts_have_one_mask_in_both_orders(oracle, n):
    d = U.rig_two_view(n=n, seed=GN_SEED[n])
    assert d["X"].shape[0] == n
    for identity in (True, False):
        T0 = U.rig_gn_T0(d, identity)
        assert identity or (np.abs(T0[:3, :3] - np.eye(3)).max() > 1e-3 and np.abs(T0[:3, 3]).max() > 0.5)
        rc_t, T_t, mask_t, info_t = _gn(oracle, d, T0, oracle.SUM_TREE)
        rc_s, T_s, mask_s, info_s = _gn(oracle, d, T0, oracle.SUM_SEQ)
        assert rc_t == rc_s == 1 and np.array_equal(mask_t, mask_s) and info_t.cnt_invalid == info_s.cnt_invalid
        if n >= 37:
            assert _rel_frob(T_t, T_s) < 1e-5 and 0.85 * n < mask_s.sum() <= n - round(0.1 * n)  # the 10 % outliers are out


@pytest.mark.parametrize("n", U.RIG_GN_COUNTS)
def test_gn_inputs_tell_the_mutants_apart(oracle, n):
    d = U.rig_two_view(n=n, seed=GN_SEED[n])
    mutants = U.rig_mutants(U.RIG_KITTI["K_l"], U.RIG_KITTI["K_r"], U.rig_T_lr())
    for identity in (True, False):
        T0 = U.rig_gn_T0(d, identity)
        base = _gn(oracle, d, T0, oracle.SUM_SEQ)
        for name, rig in mutants.items():
            r = _gn(oracle, d, T0, oracle.SUM_SEQ, rig)
            if n >= GN_SEEN_FROM[name]:
                assert _gn_ints(r) != _gn_ints(base), (name, identity)
            if n >= 37:  # and the pose leaves the 1e-4 the device is held to against this order
                assert _rel_frob(r[1], base[1]) > 1e-4, (name, identity, _rel_frob(r[1], base[1]))


def test_gn_plain_rig_cannot_see_three_of_the_mutants(oracle):
    d = S.two_view_points(n=500, seed=1)
    d["Kr"] = d["K"]
    T0 = np.eye(4, dtype=np.float32)
    base = _gn(oracle, d, T0, oracle.SUM_SEQ)
    mutants = U.rig_mutants(S.KITTI_K, S.KITTI_K, U.plain_T_lr())
    for name in U.RIG_PLAIN_NOOPS:
        r = _gn(oracle, d, T0, oracle.SUM_SEQ, mutants[name])
        assert _gn_ints(r) == _gn_ints(base) and np.array_equal(r[1].view(np.uint32), base[1].view(np.uint32)), name
    r = _gn(oracle, d, T0, oracle.SUM_SEQ, mutants["T_lr inverted"])  # (this one it does see)
    assert _gn_ints(r) != _gn_ints(base)


@pytest.mark.parametrize("n", U.MONO_GN_COUNTS)
def test_mono_gn_point_counts_have_one_mask_in_both_orders(oracle, n):
    d = S.two_view_points(n=n, seed=U.MONO_GN_SEED[n], K=U.MONO_K)
    for identity in (True, False):
        T0 = U.rig_gn_T0(d, identity)
        R0, t0 = np.ascontiguousarray(T0[:3, :3]), np.ascontiguousarray(T0[:3, 3])
        if not identity:  # float32 rounding of a rotation: R R^T is off the identity, the 4 x 4 cofactor inverse is not R^T
            assert 1e-8 < np.abs(R0.astype(np.float64) @ R0.astype(np.float64).T - np.eye(3)).max() < 1e-6
        for variant in (0, 1):
            rc_t, R_t, t_t, mask_t, _ = oracle.gn_pose_mono(d["X"], d["pts_l"], d["K"], 3, R0, t0, variant, oracle.SUM_TREE, 512)
            rc_s, R_s, t_s, mask_s, _ = oracle.gn_pose_mono(d["X"], d["pts_l"], d["K"], 3, R0, t0, variant, oracle.SUM_SEQ, 0)
            assert rc_t == rc_s == 1 and np.array_equal(mask_t, mask_s) and 0.85 * n < mask_s.sum() < n
            assert np.abs(R_s - d["T01_true"][:3, :3]).max() < 2e-3 and np.abs(t_s - d["T01_true"][:3, 3]).max() < 2e-3


# ---- stereo frame -----------------------------------------------------------------------------------------------------------
_FRAMES = {}


def _frame_inputs(stream_key, stream):
    """Per frame step of a 3-frame stream: (previous left, left, right, track set); rendered once per process."""
    if stream_key not in _FRAMES:
        poses = stream.poses(3)
        imgs = [stream.render_pair(p) for p in poses]
        _FRAMES[stream_key] = [(imgs[k - 1][0], imgs[k][0], imgs[k][1], stream.track_set(k - 1, poses[k - 1], poses[k]))
                               for k in (1, 2)]
    return _FRAMES[stream_key]


def _frames(oracle, stream_key, stream, rig, border):
    Kl, Kr, T_lr = rig
    prm = oracle.make_stereo_params(stream.width, stream.height, 21, 3, 80.0, 0.5, 3.0, Kl, Kr, np.asarray(T_lr, np.float32))
    out = []
    for Lp, L, R, ts in _frame_inputs(stream_key, stream):
        o = oracle.stereo_frame(prm, Lp, L, R, ts["pts_l0"], ts["pts_r0"], ts["Xp"], ts["dT_prior"], ts["pts_new"],
                                oracle.SUM_SEQ, 0, border, 8)
        assert o["rc"] == 0
        out.append(o)
    return out


def _frame_ints(o):
    c = o["counts"]
    return (o["stage"].tolist(), o["mask_new"].tolist(), c.n_l0l1, c.n_refine, c.n_l1r1, c.n_ba, c.n_inlier, c.n_new_ok,
            c.gn_iterations)


@pytest.mark.parametrize("strict", [False, True])
def test_frame_stream_is_healthy_and_tells_the_mutants_apart(oracle, strict):
    """At least half of the 40 features are BA inliers on both frame steps; every mutant changes the stage bytes or a
    count of every frame (K_l <-> K_r, R_lr^T and inverse(T_lr) leave no inlier at all; t_y = t_z = 0 and fx <-> fy in the
    right camera move right pixels by a fraction of a pixel at this size and show in the BA's iteration count) and
    moves dT by far more than the 1e-6 the device is held to."""
    margin = 5.0 if strict else 16.0
    border = oracle.IC_REFERENCE if strict else oracle.IC_MASKED
    stream = U.rig_stream(U.RIG_320, margin=margin, **FRAME_STREAM)
    base = _frames(oracle, ("rig", margin), stream, (stream.K, stream.Kr, stream.T_lr), border)
    for o in base:
        c = o["counts"]
        assert o["stage"].shape[0] == 40 and c.n_inlier >= 20 and c.n_l1r1 >= 30 and c.n_new_ok >= 5
    for name, rig in U.rig_mutants(stream.K, stream.Kr, U.rig_T_lr()).items():
        for k, (o, b) in enumerate(zip(_frames(oracle, ("rig", margin), stream, rig, border), base)):
            assert _frame_ints(o) != _frame_ints(b), (name, k)
            assert _rel_frob(o["dT"], b["dT"]) > 1e-4, (name, k)
            if name in ("K_l <-> K_r", "R_lr transposed", "T_lr inverted"):
                assert o["counts"].n_inlier == 0, (name, k)


def test_frame_plain_rig_cannot_see_three_of_the_mutants(oracle):
    K = (300.0, 300.0, 160.0, 100.0)
    stream = U.RigStream(K, K, U.plain_T_lr(), width=320, height=200, margin=5.0, **FRAME_STREAM)
    base = _frames(oracle, "plain", stream, (K, K, stream.T_lr), oracle.IC_REFERENCE)
    mutants = U.rig_mutants(K, K, U.plain_T_lr())
    for name in U.RIG_PLAIN_NOOPS:
        for o, b in zip(_frames(oracle, "plain", stream, mutants[name], oracle.IC_REFERENCE), base):
            assert _frame_ints(o) == _frame_ints(b) and np.array_equal(o["dT"], b["dT"]), name
            assert np.array_equal(o["pts_r1"].view(np.uint32), b["pts_r1"].view(np.uint32)), name


# ---- closed loop ------------------------------------------------------------------------------------------------------------
_LOOP_IMAGES = []


@pytest.mark.parametrize("lba,strict,kf_trans", [(True, 4, 1.0), (False, 1, 10.0)])
def test_closed_loop_on_the_rig_is_healthy(oracle, lba, strict, kf_trans):
    """The two runs of test_rig_gpu.py's closed loop, CPU side only: keyframes come, tracks grow, the local BA solves."""
    from oracle.stereo_vo import StereoVORef
    rig = U.RIG_640
    stream = U.rig_stream(rig, **LOOP_STREAM)
    poses = stream.poses(12)
    if not _LOOP_IMAGES:
        _LOOP_IMAGES.extend(stream.render_pair(p)[:2] for p in poses)
    ref = StereoVORef(rig["width"], rig["height"], stream.K, stream.Kr, stream.T_lr, 20, 8, thres_fast=15, win=21, max_level=4,
                      kf_trans=kf_trans, lba=lba, sum_mode=oracle.SUM_TREE, tree_width=512, ic_border=oracle.IC_REFERENCE, n_threads=8)
    infos = [ref.track(L, R) for L, R in _LOOP_IMAGES]
    assert sum(i["keyframe"] for i in infos) >= 2
    assert infos[0]["n_tracks"] > 80 and infos[-1]["n_tracks"] > 150
    assert np.abs(ref.T_wp - np.linalg.inv(poses[0]) @ poses[-1]).max() < 0.03
    solves = [i["lba"] for i in infos if i["lba"] is not None]
    if lba:
        assert len(solves) >= 1 and all(s["rc"] == 1 and s["err"][-1] < s["err"][0] < 1.0 for s in solves)
    else:
        assert not solves
