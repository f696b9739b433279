"""The closed loop of StereoVO::trackStereoImages (stereo_vo.cpp:392-989) on the device against its CPU restatement
(oracle/stereo_vo.py): what enters frame k+1 is what frame k left behind — survivors, new landmarks (DLT), ids, poses,
keyframes — and both sides run FREE (no state is copied from one to the other), so every frame's track set must come
out bit for bit for the comparison to hold at the end."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _stream(W, H, K, nu, nv, seed, speed, n):
    from visual_odometry_ros_amd import synthetic as S
    st = S.StereoStream(width=W, height=H, K=K, n_u=nu, n_v=nv, seed=seed, speed=speed)
    return st, [st.render_pair(p)[:2] for p in st.poses(n)]


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def test_triangulate_dlt_bit_exact(vo, oracle, ctx):
    rng = np.random.default_rng(3)
    K0 = np.array([718.856, 718.856, 607.1928, 185.2157], np.float32)
    K1 = np.array([700.0, 705.0, 600.0, 180.0], np.float32)
    from visual_odometry_ros_amd import synthetic as S
    T = S.se3_exp([-0.5371657189, 0.01, -0.02, 0.002, -0.003, 0.001]).astype(np.float32)
    n = 3000
    X = np.stack([rng.uniform(-12, 12, n), rng.uniform(-3, 3, n), rng.uniform(1.5, 80, n)], 1)
    p0 = np.stack([K0[0] * X[:, 0] / X[:, 2] + K0[2], K0[1] * X[:, 1] / X[:, 2] + K0[3]], 1)
    X1 = X @ T[:3, :3].T.astype(np.float64) + T[:3, 3]
    p1 = np.stack([K1[0] * X1[:, 0] / X1[:, 2] + K1[2], K1[1] * X1[:, 1] / X1[:, 2] + K1[3]], 1)
    p0 += rng.normal(0, 0.4, p0.shape)
    p1 += rng.normal(0, 0.4, p1.shape)
    p1[:50] = p0[:50]            # zero disparity: depth at infinity / behind
    p1[50:60, 0] += 40.0         # negative disparity
    p0, p1 = p0.astype(np.float32), p1.astype(np.float32)
    g0, g1 = vo.triangulateDLT(ctx, p0, p1, T, K0, K1)
    for i in range(n):
        o0, o1 = oracle.triangulate_dlt(p0[i], p1[i], T[:3, :3], T[:3, 3], K0, K1)
        assert np.array_equal(_bits(g0[i]), _bits(o0)) and np.array_equal(_bits(g1[i]), _bits(o1)), i
    good = slice(60, n)
    assert np.median(np.abs(g0[good, 2] - X[good, 2]) / X[good, 2]) < 0.05


def _run_both(vo, oracle, W, H, K, nu, nv, frames, win, lvl, n_frames, lba, strict, seed=5, speed=0.5, prefetch=False,
              kf_trans=10.0, kf_overlap=0.6, id_offset=0, id_jump=None, K_r=None, T_lr=None):
    """K_r, T_lr: the right camera's intrinsics and pose where the rig is not the stream's plain one (K, st.T_lr)."""
    from oracle.stereo_vo import StereoVORef
    st, imgs = frames
    K_r = K if K_r is None else K_r
    T_lr = st.T_lr if T_lr is None else T_lr
    ref = StereoVORef(W, H, K, K_r, T_lr, nu, nv, thres_fast=15, win=win, max_level=lvl, kf_trans=kf_trans, kf_overlap=kf_overlap,
                      lba=lba, sum_mode=oracle.SUM_TREE, tree_width=512, ic_border=oracle.IC_REFERENCE if strict else oracle.IC_MASKED,
                      n_threads=8)
    c = vo.Context(device=0, max_width=W, max_height=H, max_points=4096, n_slots=5, max_level=lvl)
    try:
        if id_offset:
            vo.TrackIds(c).reset(id_offset, 0)  # the stream's landmark counter starts here (the CPU loop's at 0)
        svo = vo.StereoVO(c, W, H, K, K_r, T_lr, nu, nv, thres_fastscore=15, window_size=win, max_level=lvl, strict_border=strict,
                          local_ba=lba, thres_trans=kf_trans, thres_alive_ratio=kf_overlap)
        log = []
        for k in range(n_frames):
            L, R = imgs[k]
            if id_jump and k == id_jump[0]:  # both landmark counters leap ahead: the ids are labels, the interval is not
                nl, nf = vo.TrackIds(c).peek()
                vo.TrackIds(c).reset(nl + id_jump[1], nf)
                ref.landmark_counter += id_jump[1]
            if prefetch:
                svo.enqueue(L, R)
                if k + 1 < n_frames:
                    svo.prefetch(*imgs[k + 1])
                gi = svo.result()
            else:
                gi = svo.trackStereoImages(L, R)
            ri = ref.track(L, R)
            g = svo.getTracks()
            where = f"frame {k}"
            assert gi.frame_id == ri["frame_id"], where
            assert bool(gi.is_keyframe) == ri["keyframe"], where
            assert np.array_equal(g["ids"] - id_offset, ref.ids), where
            assert np.array_equal(_bits(g["pts_l"]), _bits(ref.pts_l)) and np.array_equal(_bits(g["pts_r"]), _bits(ref.pts_r)), where
            assert np.array_equal(g["flags"], ref.flags), where
            tri = (ref.flags & 1) != 0
            assert np.array_equal(_bits(g["Xw"][tri]), _bits(ref.Xw[tri])), where
            assert np.array_equal(_bits(np.array(gi.T_wc).reshape(4, 4)), _bits(ref.T_wp)), where
            if k > 0:
                assert (gi.n_final, gi.n_new, gi.n_kf_tracked) == (ri["n_surv"], ri["n_new"], ri["n_kf_tracked"]), where
                npg = svo.getNewPoints()
                assert np.array_equal(_bits(npg["pts_l"]), _bits(ri["cand"])) and np.array_equal(npg["accept"], ri["accept"]), where
                assert np.array_equal(npg["mask_new"], ri["mask_new"]), where
            log.append((bool(gi.is_keyframe), gi.n_tracks_out, bool(gi.lba_ran), int(gi.lba_landmarks)))
            if gi.is_keyframe or k == n_frames - 1:  # stats_keyframe: every keyframe's current pose and map points
                gk, rk = svo.getKeyframes(), ref.keyframe_stats()
                assert len(gk) == len(rk), where
                for j, ((Tg, Xg), (Tr, Xr)) in enumerate(zip(gk, rk)):
                    assert np.array_equal(_bits(Tg), _bits(Tr)) and np.array_equal(_bits(Xg), _bits(Xr)), (where, j)
                T1, X1 = svo.getKeyframe(len(gk) - 1)  # (the one-keyframe getter against the all-at-once one)
                assert np.array_equal(_bits(T1), _bits(gk[-1][0])) and np.array_equal(_bits(X1), _bits(gk[-1][1])), where
        svo.close()
        return log, ref
    finally:
        c.close()


@pytest.mark.parametrize("strict,prefetch", [(4, False), (1, True), (0, True), (3, True)])
def test_closed_loop_small(vo, oracle, strict, prefetch):
    W, H, K = 640, 240, (400.0, 400.0, 320.0, 120.0)
    frames = _stream(W, H, K, 20, 8, 5, 0.5, 12)
    log, ref = _run_both(vo, oracle, W, H, K, 20, 8, frames, 21, 4, 12, lba=False, strict=strict, prefetch=prefetch)
    assert sum(1 for e in log if e[0]) >= 2  # the second frame and at least one more keyframe
    assert log[-1][1] > 100


def test_closed_loop_kitti_size(vo, oracle):
    """BASELINE configs[1]: 1241x376, 60x25 buckets, win 21, max_level 6 — 9 frames of the forward-driving stream."""
    from visual_odometry_ros_amd import synthetic as S
    W, H = S.KITTI_SIZE
    frames = _stream(W, H, S.KITTI_K, 60, 25, 2, 0.8, 9)
    log, ref = _run_both(vo, oracle, W, H, S.KITTI_K, 60, 25, frames, 21, 6, 9, lba=False, strict=4, prefetch=True, kf_overlap=0.8)
    assert log[-1][1] > 1000
    assert sum(1 for e in log if e[0]) >= 2


def test_closed_loop_kitti_size_local_ba(vo, oracle):
    """The same at full size with a keyframe every other frame: three local-BA solves over up to five keyframes and
    several thousand landmarks — the device-side problem builder beyond one workgroup's worth of ids and landmarks
    (multi-workgroup scans, gather lists with more than one landmark per lane)."""
    from visual_odometry_ros_amd import synthetic as S
    W, H = S.KITTI_SIZE
    frames = _stream(W, H, S.KITTI_K, 60, 25, 2, 0.8, 10)
    log, ref = _run_both(vo, oracle, W, H, S.KITTI_K, 60, 25, frames, 21, 6, 10, lba=True, strict=4, prefetch=True, kf_trans=1.0)
    assert sum(1 for e in log if e[2]) >= 3, log
    assert max(e[3] for e in log) >= 2048, log  # landmarks in the largest problem


def test_closed_loop_with_local_ba(vo, oracle):
    """Keyframes every few frames (low translation threshold) so that the window reaches three keyframes and the local BA
    runs several times; after each, poses and landmarks re-enter the loop. The device solver agrees with the CPU solver
    to ~1e-14 in double, so the float casts — and with them every later frame — come out identical."""
    W, H, K = 640, 240, (400.0, 400.0, 320.0, 120.0)
    frames = _stream(W, H, K, 20, 8, 5, 0.5, 14)
    log, ref = _run_both(vo, oracle, W, H, K, 20, 8, frames, 21, 4, 14, lba=True, strict=4, prefetch=True, kf_trans=1.2)
    assert sum(1 for e in log if e[2]) >= 3, log


def test_closed_loop_local_ba_sliding_window(vo, oracle):
    """A keyframe every other frame for 32 frames: the window fills up (nine keyframes, seven optimised: the 42 x 42
    register solve), then slides — keyframes leave the device-side ring, their slots are reused, the id interval of the
    landmark table moves on — and the device-built problem still leaves the loop bit for bit on the CPU loop's state."""
    W, H, K = 640, 240, (400.0, 400.0, 320.0, 120.0)
    frames = _stream(W, H, K, 20, 8, 7, 0.5, 32)
    log, ref = _run_both(vo, oracle, W, H, K, 20, 8, frames, 21, 4, 32, lba=True, strict=4, prefetch=True, kf_trans=0.9)
    assert sum(1 for e in log if e[0]) >= 13, log      # more keyframes than the window holds
    assert sum(1 for e in log if e[2]) >= 11, log


def test_closed_loop_local_ba_landmark_table_wraps(vo, oracle):
    """The device-side landmark table is addressed by id modulo its size (2^18 slots at first, doubling up to 2^24): a stream
    whose landmark counter crosses a multiple of every such size in the middle of a keyframe window (ids 2^24 - 150 ...)
    must give the same loop."""
    W, H, K = 640, 240, (400.0, 400.0, 320.0, 120.0)
    frames = _stream(W, H, K, 20, 8, 5, 0.5, 14)
    log, ref = _run_both(vo, oracle, W, H, K, 20, 8, frames, 21, 4, 14, lba=True, strict=4, prefetch=True, kf_trans=1.2,
                         id_offset=(1 << 24) - 150)
    assert sum(1 for e in log if e[2]) >= 3, log
    assert ref.ids.min() < 150 < ref.ids.max()  # live landmarks on both sides of the boundary at the end


def test_closed_loop_with_rectification(vo, oracle):
    """flagDoUndistortion (stereo_vo.cpp:414-427): raw cameras with lens distortion and a slightly rotated right camera;
    every pair goes through the stereo rectification maps on its way into the pyramids (device images and host images),
    the loop runs on the rectified camera — against the CPU loop fed with the CPU remap of the same pairs."""
    from oracle.stereo_vo import StereoVORef
    from util import DeviceBuffer
    from visual_odometry_ros_amd import synthetic as S
    W, H, K = 640, 240, (400.0, 400.0, 320.0, 120.0)
    st, imgs = _stream(W, H, K, 20, 8, 9, 0.5, 9)
    Kl = np.array(K, np.float32)
    Kr = np.array([402.0, 401.0, 318.0, 121.0], np.float32)
    Dl = np.array([-0.08, 0.02, 0.0005, -0.0004, 0.0], np.float32)
    Dr = np.array([-0.07, 0.015, -0.0003, 0.0006, 0.0], np.float32)
    T_lr = (st.T_lr.astype(np.float64) @ S.se3_exp([0, 0, 0, 0.004, -0.006, 0.003])).astype(np.float32)
    m = oracle.stereo_rectify_maps(W, H, Kl, Dl, Kr, Dr, T_lr)
    for on_device in (True, False):
        ref = StereoVORef(W, H, m["K_rect"], m["K_rect"], m["T_lr_rect"], 20, 8, thres_fast=15, win=21, max_level=4, kf_trans=1.2,
                          lba=True, sum_mode=oracle.SUM_TREE, tree_width=512, ic_border=oracle.IC_REFERENCE, n_threads=8,
                          rectify_maps=(m["left"], m["right"]))
        c = vo.Context(device=0, max_width=W, max_height=H, max_points=4096, n_slots=5, max_level=4)
        try:
            cam = vo.StereoCamera(c)
            cam.initParams(W, H, Kl, Dl, Kr, Dr)
            cam.setStereoPoseLeft2Right(T_lr)
            cam.initStereoCameraToRectify()
            assert np.array_equal(_bits(cam.K_rect), _bits(m["K_rect"])) and np.array_equal(_bits(cam.T_lr_rect), _bits(m["T_lr_rect"]))
            svo = vo.StereoVO(c, W, H, cam.K_rect, cam.K_rect, cam.T_lr_rect, 20, 8, thres_fastscore=15, window_size=21, max_level=4,
                              strict_border=4, local_ba=True, thres_trans=1.2, rectify=True)
            keep = []
            for k, (L, R) in enumerate(imgs):
                if on_device:
                    dL, dR = DeviceBuffer(L), DeviceBuffer(R)
                    keep.append((dL, dR))
                    gi = svo.trackStereoImages((dL.data_ptr(), W), (dR.data_ptr(), W))
                else:
                    gi = svo.trackStereoImages(L, R)
                ref.track(L, R)
                g = svo.getTracks()
                where = f"frame {k}, device images {on_device}"
                assert np.array_equal(g["ids"], ref.ids), where
                assert np.array_equal(_bits(g["pts_l"]), _bits(ref.pts_l)) and np.array_equal(_bits(g["pts_r"]), _bits(ref.pts_r)), where
                assert np.array_equal(_bits(np.array(gi.T_wc).reshape(4, 4)), _bits(ref.T_wp)), where
            assert len(ref.ids) > 100
            svo.close()
            for dL, dR in keep:
                dL.free()
                dR.free()
        finally:
            c.close()


def test_closed_loop_local_ba_wide_id_interval(vo, oracle):
    """The window's id interval is set by its oldest landmark still alive: a leap of 300 000 in the landmark counter in the
    middle of the run makes the interval wider than the window scratch's first allocation and than the landmark table's
    first size (2^18 slots) — both have to grow (the table re-hashed), and the builder's scans run over an interval that
    is almost empty."""
    W, H, K = 640, 240, (400.0, 400.0, 320.0, 120.0)
    frames = _stream(W, H, K, 20, 8, 5, 0.5, 14)
    log, ref = _run_both(vo, oracle, W, H, K, 20, 8, frames, 21, 4, 14, lba=True, strict=4, prefetch=True, kf_trans=1.2,
                         id_jump=(4, 300000))
    assert sum(1 for e in log if e[2]) >= 3, log
    assert ref.ids.min() < 1000 and ref.ids.max() > 300000  # landmarks from both sides of the leap are still tracked


def test_closed_loop_kitti_size_sliding_window(vo, oracle):
    """Steady state at full size: 1241x376 / 60x25 buckets with a keyframe every other frame for 24 frames — the window
    fills (nine keyframes, seven optimised: the 42 x 42 register solve on several thousand landmarks), slides, ring slots
    are reused — every frame's track set, flags, world points, pose and every keyframe's map points against the CPU loop."""
    from visual_odometry_ros_amd import synthetic as S
    W, H = S.KITTI_SIZE
    frames = _stream(W, H, S.KITTI_K, 60, 25, 2, 0.8, 24)
    log, ref = _run_both(vo, oracle, W, H, S.KITTI_K, 60, 25, frames, 21, 6, 24, lba=True, strict=4, prefetch=True, kf_trans=1.0)
    assert sum(1 for e in log if e[0]) >= 11, log          # more keyframes than the window holds
    assert sum(1 for e in log if e[2]) >= 9, log
    assert max(e[3] for e in log) >= 4000, log             # landmarks in the largest problem (nine keyframes)


# ---- the device loop against the CPU loop in the REFERENCE's summation order (north star: "bit-exact feature indices / track
# IDs; SE(3) within 1e-4 relative Frobenius") ---------------------------------------------------------------------------------
# The kernels sum trackWithScale's 264 taps as 64 lane partials + a butterfly and the pose-only BA's normal equations as 512
# partials + a tree (oracle SUM_TREE, what every other loop test compares with, bit for bit); the reference adds them one after
# the other (SUM_SEQ). Both loops run free, so the last bits of a frame's refined pixels enter the next frame's priors.
# Measured (tests/measure/seq_vs_tree.py runs the same comparison on the CPU alone, SUM_SEQ loop against SUM_TREE loop): ids,
# flags and keyframe decisions are equal for frames 0..8; at frame 9 the sets fork at the pose-only BA's inlier gate
# `0.5 (|rx_l| + |ry_l| + |rx_r| + |ry_r|) >= thres_poseba_error = 3.0` (motion_estimator.cpp:950-958): features 416 and 592 have
# 3.2767 / 3.0527 in the reference's order (outliers, stage 3) and 2.9246 / 2.7198 in the kernels' (inliers, stage 4). Not an
# ulp at a threshold: their refined pixels differ by 0.39 and 1.03 px between the two orders — two ill-conditioned patches whose
# trackWithScale runs amplify differences of 1e-6 relative that earlier frames left in the priors. Poses stay within 3.3e-5 and
# every keyframe decision equal over all 24 frames.
_SEQ_FORK_FRAME = 9


def _vs_reference_order(vo, oracle, n_frames=24):
    from oracle.stereo_vo import StereoVORef
    from visual_odometry_ros_amd import synthetic as S
    W, H = S.KITTI_SIZE
    st, imgs = _stream(W, H, S.KITTI_K, 60, 25, 2, 0.8, n_frames)
    ref = StereoVORef(W, H, S.KITTI_K, S.KITTI_K, st.T_lr, 60, 25, thres_fast=15, win=21, max_level=6, kf_trans=1.0, lba=True,
                      sum_mode=oracle.SUM_SEQ, tree_width=0, ic_border=oracle.IC_REFERENCE, n_threads=8)
    c = vo.Context(device=0, max_width=W, max_height=H, max_points=4096, n_slots=5, max_level=6)
    rep = dict(ids_equal=[], flags_equal=[], kf_equal=[], pose_rel=[], lba=0)
    try:
        svo = vo.StereoVO(c, W, H, S.KITTI_K, S.KITTI_K, st.T_lr, 60, 25, thres_fastscore=15, window_size=21, max_level=6,
                          strict_border=4, local_ba=True, thres_trans=1.0)
        for k in range(n_frames):
            svo.enqueue(*imgs[k])
            if k + 1 < n_frames:
                svo.prefetch(*imgs[k + 1])
            gi = svo.result()
            ri = ref.track(*imgs[k])
            g = svo.getTracks()
            same = np.array_equal(g["ids"], ref.ids)
            rep["ids_equal"].append(bool(same))
            rep["flags_equal"].append(bool(same and np.array_equal(g["flags"], ref.flags)))
            rep["kf_equal"].append(bool(gi.is_keyframe) == ri["keyframe"])
            Tg, Tr = np.array(gi.T_wc, np.float64).reshape(4, 4), ref.T_wp.astype(np.float64)
            rep["pose_rel"].append(float(np.linalg.norm(Tg - Tr) / np.linalg.norm(Tr)))
            rep["lba"] += int(bool(gi.lba_ran))
        svo.close()
    finally:
        c.close()
    return rep


@pytest.fixture(scope="module")
def seq_report(vo, oracle):
    return _vs_reference_order(vo, oracle)


def test_closed_loop_kitti_size_vs_reference_order(seq_report):
    """24 free-running frames at 1241x376 with the local BA (window full and sliding) against the CPU loop in the REFERENCE's
    summation order: pose within 1e-4 relative Frobenius and the same keyframe decision at EVERY frame; track ids and flags equal
    up to the measured fork (frame 9, see above) — a fork that moves EARLIER fails here."""
    r = seq_report
    assert max(r["pose_rel"]) < 1e-4, r["pose_rel"]
    assert all(r["kf_equal"]), r["kf_equal"]
    assert r["lba"] >= 9
    first = next((k for k, e in enumerate(r["ids_equal"]) if not e), len(r["ids_equal"]))
    assert first >= _SEQ_FORK_FRAME, (first, r["ids_equal"])
    assert all(r["flags_equal"][:_SEQ_FORK_FRAME])


@pytest.mark.xfail(strict=True, reason="track ids against the reference's summation order fork at frame 9 of 24 (1241x376, local BA): "
                   "pose-only BA inlier gate 0.5*sum|r| >= 3.0 px (motion_estimator.cpp:950-958) for features 416 / 592 — 3.2767 / "
                   "3.0527 in the reference's order against 2.9246 / 2.7198 in the kernels' (their trackWithScale results differ by "
                   "0.39 / 1.03 px: ill-conditioned patches amplify 1e-6-level differences of earlier frames, not an ulp at the gate); "
                   "poses stay within 3.3e-5, keyframe decisions equal")
def test_closed_loop_kitti_size_ids_vs_reference_order_every_frame(seq_report):
    assert all(seq_report["ids_equal"]), seq_report["ids_equal"]


def test_closed_loop_config5(vo, oracle):
    """BASELINE configs[4] as a closed loop, the stream bench.py --config 4 runs: 3840x2160, 100x80 buckets, win 21, 5-level
    pyramid, a third of configs[1]'s distance per frame and a third of its texture cell sizes (the same flow and detail per
    pixel), feature_tracker.thres_sampson = 120 (the reference's row-660 gate of step [7] would drop 70 % of a 2160-row image
    every frame: stereo_vo.cpp:659) — vo_svo_* on six frames against the CPU loop while the track set fills up (4000+ landmarks)."""
    from oracle.stereo_vo import StereoVORef
    from visual_odometry_ros_amd import synthetic as S
    W, H, K = 3840, 2160, (718.856 * 3.0, 718.856 * 3.0, 1920.0, 1080.0)
    st = S.StereoStream(width=W, height=H, K=K, n_u=100, n_v=80, seed=2, speed=0.8 / 3.0, tex_scale=1.0 / 3.0)
    imgs = [st.render_pair(p)[:2] for p in st.poses(6)]
    ref = StereoVORef(W, H, K, K, st.T_lr, 100, 80, thres_fast=15, win=21, max_level=4, kf_trans=0.5, lba=False,
                      sum_mode=oracle.SUM_TREE, tree_width=512, ic_border=oracle.IC_REFERENCE, n_threads=16, thres_sampson=120.0)
    c = vo.Context(device=0, max_width=W, max_height=H, max_points=2 * 8000 + 1024, n_slots=5, max_level=4)
    try:
        svo = vo.StereoVO(c, W, H, K, K, st.T_lr, 100, 80, thres_fastscore=15, window_size=21, max_level=4, strict_border=4,
                          local_ba=False, thres_trans=0.5, thres_sampson=120.0)
        n_kf = 0
        for k, (L, R) in enumerate(imgs):
            gi = svo.trackStereoImages(L, R)
            ri = ref.track(L, R)
            g = svo.getTracks()
            where = f"frame {k}"
            assert bool(gi.is_keyframe) == ri["keyframe"], where
            assert np.array_equal(g["ids"], ref.ids), where
            assert np.array_equal(_bits(g["pts_l"]), _bits(ref.pts_l)) and np.array_equal(_bits(g["pts_r"]), _bits(ref.pts_r)), where
            assert np.array_equal(g["flags"], ref.flags), where
            tri = (ref.flags & 1) != 0
            assert np.array_equal(_bits(g["Xw"][tri]), _bits(ref.Xw[tri])), where
            assert np.array_equal(_bits(np.array(gi.T_wc).reshape(4, 4)), _bits(ref.T_wp)), where
            n_kf += int(bool(gi.is_keyframe))
        print("config5 track set sizes:", len(ref.ids), "keyframes", n_kf)
        assert len(ref.ids) > 4000 and n_kf >= 2  # (six frames in; the stream settles near 6900 after ~50: bench.py --config 4)
        svo.close()
    finally:
        c.close()


def test_steady_state_frames_allocate_nothing(vo):
    """Everything a stream's keyframes need — landmark table, keyframe ring, keyframe pool, the local BA's window scratch
    and arena — is allocated by vo_svo_create: between frame 2 and frame 60 of a loop with a keyframe every other frame
    (the first keyframe, the growing window, the first solve, the full window, the sliding one) the context makes not one
    device or pinned allocation. Also: what a StereoVO holds for its keyframes at BASELINE configs[1] sizes."""
    W, H, K = 640, 240, (400.0, 400.0, 320.0, 120.0)
    st, imgs = _stream(W, H, K, 20, 8, 21, 0.5, 61)
    c = vo.Context(device=0, max_width=W, max_height=H, max_points=4096, n_slots=5, max_level=4)
    try:
        svo = vo.StereoVO(c, W, H, K, K, st.T_lr, 20, 8, thres_fastscore=15, window_size=21, max_level=4, strict_border=4,
                          local_ba=True, thres_trans=0.9)
        n_at_2, n_lba, n_kf = None, 0, 0
        for k in range(61):
            i = svo.trackStereoImages(*imgs[k])   # host images, no look-ahead: what the reference's caller does
            n_lba += int(bool(i.lba_ran))
            n_kf += int(bool(i.is_keyframe))
            if k == 2:
                n_at_2 = c.allocation_count()
        assert n_kf >= 20 and n_lba >= 18
        assert c.allocation_count() == n_at_2, (n_at_2, c.allocation_count())
        svo.close()
    finally:
        c.close()
    from visual_odometry_ros_amd import synthetic as S
    W, H = S.KITTI_SIZE
    c = vo.Context(device=0, max_width=W, max_height=H, max_points=2 * 1500 + 1024, n_slots=5, max_level=6)
    try:
        svo = vo.StereoVO(c, W, H, S.KITTI_K, S.KITTI_K, S.stereo_T_lr(), 60, 25, thres_fastscore=15, window_size=21, max_level=6,
                          strict_border=4, local_ba=True)
        assert svo.deviceBytes() <= 40 << 20, svo.deviceBytes()   # (was 310 MB: a 2^24-slot landmark table)
        svo.close()
    finally:
        c.close()


def test_closed_loop_is_deterministic(vo):
    """Sixty frames with the concurrent replay (mode 4), the DLT workers, the device-built local BA (atomics in its scatter,
    a window that fills and slides): two runs give the same bits — poses of every frame, final ids, every keyframe's pose and
    map points."""
    W, H, K = 640, 240, (400.0, 400.0, 320.0, 120.0)
    st, imgs = _stream(W, H, K, 20, 8, 21, 0.5, 60)
    runs = []
    for _ in range(2):
        c = vo.Context(device=0, max_width=W, max_height=H, max_points=4096, n_slots=5, max_level=4)
        try:
            svo = vo.StereoVO(c, W, H, K, K, st.T_lr, 20, 8, thres_fastscore=15, window_size=21, max_level=4, strict_border=4,
                              local_ba=True, thres_trans=0.9)
            Ts, n_lba = [], 0
            for k in range(60):
                svo.enqueue(*imgs[k])
                if k + 1 < 60:
                    svo.prefetch(*imgs[k + 1])
                i = svo.result()
                Ts.append(np.array(i.T_wc, np.float32))
                n_lba += int(bool(i.lba_ran))
            runs.append((np.stack(Ts), svo.getTracks()["ids"].copy(), svo.getKeyframes(), n_lba))
            svo.close()
        finally:
            c.close()
    (Ta, ia, ka, la), (Tb, ib, kb, lb) = runs
    assert la == lb >= 20
    assert np.array_equal(_bits(Ta), _bits(Tb)) and np.array_equal(ia, ib) and len(ka) == len(kb)
    for (T1, X1), (T2, X2) in zip(ka, kb):
        assert np.array_equal(_bits(T1), _bits(T2)) and np.array_equal(_bits(X1), _bits(X2))
    assert np.isfinite(Ta).all() and abs(Ta[-1][11] - 0.5 * 59) < 1.5  # (z of the last pose: 0.5 m per frame)


def test_run_sequence_equals_the_three_calls(vo):
    """vo_svo_run (the sequence loop inside the library: result(k), enqueue(k + 1), prefetch(k + 2)), called in three pieces,
    against the same sequence driven call by call from here: poses of every frame, keyframe decisions, final ids — the same
    bits (device images; local BA and the concurrent replay on)."""
    from util import DeviceBuffer
    W, H, K, n = 640, 240, (400.0, 400.0, 320.0, 120.0), 24
    st, imgs = _stream(W, H, K, 20, 8, 9, 0.5, n)
    bufs = [(DeviceBuffer(L), DeviceBuffer(R)) for L, R in imgs]
    pairs = [((a.data_ptr(), W), (b.data_ptr(), W)) for a, b in bufs]
    runs = []
    try:
        for mode in ("calls", "library"):
            c = vo.Context(device=0, max_width=W, max_height=H, max_points=4096, n_slots=5, max_level=4)
            try:
                svo = vo.StereoVO(c, W, H, K, K, st.T_lr, 20, 8, thres_fastscore=15, window_size=21, max_level=4, strict_border=4,
                                  local_ba=True, thres_trans=0.9)
                infos = []
                if mode == "calls":
                    svo.enqueue(*pairs[0])
                    svo.prefetch(*pairs[1])
                    for k in range(n):
                        infos.append(svo.result())
                        if k + 1 < n:
                            svo.enqueue(*pairs[k + 1])
                            if k + 2 < n:
                                svo.prefetch(*pairs[k + 2])
                else:
                    for a, b in ((0, 5), (5, 6), (6, n)):
                        # (a fresh list object per chunk: the address arrays must follow the list handed in, not its id())
                        out, stamps = svo.runSequence(pairs if a == 0 else list(pairs), a, b)
                        assert len(out) == b - a and (np.diff(stamps) > 0).all()
                        infos += out
                    with pytest.raises(vo.VoError):
                        svo.runSequence(pairs, 3, 4)  # nothing in flight any more
                runs.append((np.stack([np.array(i.T_wc, np.float32) for i in infos]), [int(i.is_keyframe) for i in infos],
                             [int(i.lba_ran) for i in infos], svo.getTracks()["ids"].copy()))
                svo.close()
            finally:
                c.close()
    finally:
        for a, b in bufs:
            a.free()
            b.free()
    (Ta, ka, la, ia), (Tb, kb, lb, ib) = runs
    assert np.array_equal(_bits(Ta), _bits(Tb)) and ka == kb and la == lb and np.array_equal(ia, ib)
    assert sum(la) >= 5


def test_synchronous_call_equals_the_look_ahead_loop(vo):
    """trackStereoImages(left, right) as ONE call per pair — with host images (the detector starts behind the left upload, from
    the slot's staging plane) and with device images (the detector starts from the caller's image, before the pyramids are
    queued) — against the loop that hands every pair over one frame early: poses of every frame, keyframe decisions, local-BA
    runs and the final ids, the same bits (local BA and the concurrent replay on)."""
    from util import DeviceBuffer
    W, H, K, n = 640, 240, (400.0, 400.0, 320.0, 120.0), 20
    st, imgs = _stream(W, H, K, 20, 8, 9, 0.5, n)
    bufs = [(DeviceBuffer(L), DeviceBuffer(R)) for L, R in imgs]
    pairs = [((a.data_ptr(), W), (b.data_ptr(), W)) for a, b in bufs]
    runs = {}
    try:
        for mode in ("look_ahead", "look_ahead_host", "sync_device", "sync_host"):
            c = vo.Context(device=0, max_width=W, max_height=H, max_points=4096, n_slots=5, max_level=4)
            try:
                svo = vo.StereoVO(c, W, H, K, K, st.T_lr, 20, 8, thres_fastscore=15, window_size=21, max_level=4, strict_border=4,
                                  local_ba=True, thres_trans=0.9)
                if mode == "look_ahead":
                    infos = svo.runSequence(pairs, 0, n)[0]
                elif mode == "look_ahead_host":  # (numpy images through the library's loop: uploaded one frame ahead)
                    infos = svo.runSequence(imgs, 0, 7)[0] + svo.runSequence(imgs, 7, n)[0]
                elif mode == "sync_device":
                    infos = [svo.trackStereoImages(*pairs[k]) for k in range(n)]
                else:
                    infos = [svo.trackStereoImages(*imgs[k]) for k in range(n)]
                runs[mode] = (np.stack([np.array(i.T_wc, np.float32) for i in infos]), [int(i.is_keyframe) for i in infos],
                              [int(i.lba_ran) for i in infos], svo.getTracks()["ids"].copy(), c.frame_recoveries())
                svo.close()
            finally:
                c.close()
    finally:
        for a, b in bufs:
            a.free()
            b.free()
    Ta, ka, la, ia, _ = runs["look_ahead"]
    assert sum(la) >= 4
    for mode in ("look_ahead_host", "sync_device", "sync_host"):
        Tb, kb, lb, ib, rec = runs[mode]
        assert rec == 0, mode
        assert np.array_equal(_bits(Ta), _bits(Tb)) and ka == kb and la == lb and np.array_equal(ia, ib), mode


def test_closed_loop_survives_a_join_timeout():
    """The loop in strict-border mode 3 with a device-side join that cannot be met (VO_DEBUG_FAIL_JOIN, fresh child process):
    the first steady-state frame is issued again with the stream-ordered replay — and with it the DLT workers and the
    epilogue that builds the next track set — and every frame still equals the CPU loop bit for bit."""
    import os
    import subprocess
    import sys
    env = dict(os.environ, VO_TEST_SWITCHES="1", VO_DEBUG_FAIL_JOIN="1")
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-x", "-m", "gpu", "-k",
                        "test_closed_loop_small and 3-True"], env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and " passed" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
    # the synchronous call (no prefetch): the BA launch's device-side join on the candidates' own launch cannot be met either —
    # the frame is issued again with everything in stream order
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-x", "-m", "gpu", "-k",
                        "test_closed_loop_small and 4-False"], env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and " passed" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]


def test_from_yaml_runs_the_references_configuration(vo, oracle, tmp_path):
    """StereoVO.from_yaml: a configuration file in the reference's format (OpenCV FileStorage YAML) for the small synthetic
    rig — with flagDoUndistortion = 1 and lens distortion — drives the loop; the CPU loop gets the same numbers by hand."""
    from oracle.stereo_vo import StereoVORef
    from visual_odometry_ros_amd import synthetic as S
    W, H, K = 640, 240, (400.0, 400.0, 320.0, 120.0)
    st, imgs = _stream(W, H, K, 20, 8, 11, 0.5, 7)
    Dl, Dr = [-0.05, 0.01, 0.0003, -0.0002, 0.0], [-0.04, 0.012, -0.0002, 0.0004, 0.0]
    T_lr = np.asarray(st.T_lr, np.float32)
    cam = lambda side, D: "".join(f"Camera.{side}.{k}: {v}\n" for k, v in (  # noqa: E731
        ("fx", K[0]), ("fy", K[1]), ("cx", K[2]), ("cy", K[3]), ("k1", D[0]), ("k2", D[1]), ("p1", D[2]), ("p2", D[3]), ("k3", D[4]),
        ("width", W), ("height", H)))
    text = ("%YAML:1.0\nflagDoUndistortion: 1\n" + cam("left", Dl) + cam("right", Dr) +
            "T_lr: !!opencv-matrix\n  rows: 4\n  cols: 4\n  dt: f\n  data: [" + ",".join(repr(float(v)) for v in T_lr.reshape(-1)) + "]\n"
            "feature_tracker.thres_error: 80.0\nfeature_tracker.thres_bidirection: 0.5\nfeature_tracker.thres_sampson: 60.0\n"
            "feature_tracker.window_size: 21\nfeature_tracker.max_level: 4\nmap_update.thres_parallax: 1.0\n"
            "feature_extractor.n_features: 2000\nfeature_extractor.n_bins_u: 20\nfeature_extractor.n_bins_v: 8\n"
            "feature_extractor.thres_fastscore: 15.0\nfeature_extractor.radius: 5.0\nmotion_estimator.thres_1p_error: 120.0\n"
            "motion_estimator.thres_5p_error: 1.0\nmotion_estimator.thres_poseba_error: 3.0\nkeyframe_update.thres_alive_ratio: 0.6\n"
            "keyframe_update.thres_mean_parallax: 1.0\nkeyframe_update.thres_trans: 1.2\nkeyframe_update.thres_rotation: 15.0\n"
            "keyframe_update.n_max_keyframes_in_window: 9\n")
    path = tmp_path / "rig.yaml"
    path.write_text(text)
    m = oracle.stereo_rectify_maps(W, H, np.array(K, np.float32), np.array(Dl, np.float32), np.array(K, np.float32),
                                   np.array(Dr, np.float32), T_lr)
    ref = StereoVORef(W, H, m["K_rect"], m["K_rect"], m["T_lr_rect"], 20, 8, thres_fast=15, win=21, max_level=4, kf_trans=1.2,
                      lba=True, sum_mode=oracle.SUM_TREE, tree_width=512, ic_border=oracle.IC_REFERENCE, n_threads=8,
                      rectify_maps=(m["left"], m["right"]))
    svo = vo.StereoVO.from_yaml(str(path))
    try:
        assert svo.config["flagDoUndistortion"] == 1 and svo.prm.rectify == 1 and svo.prm.kf_window == 9
        for k, (L, R) in enumerate(imgs):
            gi = svo.trackStereoImages(L, R)
            ref.track(L, R)
            g = svo.getTracks()
            assert np.array_equal(g["ids"], ref.ids) and np.array_equal(_bits(g["pts_l"]), _bits(ref.pts_l)), k
            assert np.array_equal(_bits(np.array(gi.T_wc).reshape(4, 4)), _bits(ref.T_wp)), k
    finally:
        svo.close()


def test_sequence_runner_example(vo, tmp_path):
    """examples/run_stereo_sequence.py: PNG pairs on disk + a configuration file of the reference's format -> the reference's
    trajectory file; the same bytes as the in-process loop over the same arrays."""
    import subprocess
    import sys
    PIL = pytest.importorskip("PIL.Image")
    W, H, K = 640, 240, (400.0, 400.0, 320.0, 120.0)
    st, imgs = _stream(W, H, K, 20, 8, 13, 0.5, 7)
    dl, dr = tmp_path / "image_0", tmp_path / "image_1"
    dl.mkdir()
    dr.mkdir()
    for k, (L, R) in enumerate(imgs):
        PIL.fromarray(L).save(dl / f"{k:06d}.png")
        PIL.fromarray(R).save(dr / f"{k:06d}.png")
    T_lr = np.asarray(st.T_lr, np.float32)
    cam = lambda side: "".join(f"Camera.{side}.{k}: {v}\n" for k, v in (  # noqa: E731
        ("fx", K[0]), ("fy", K[1]), ("cx", K[2]), ("cy", K[3]), ("k1", 0.0), ("k2", 0.0), ("p1", 0.0), ("p2", 0.0), ("k3", 0.0),
        ("width", W), ("height", H)))
    cfg = tmp_path / "rig.yaml"
    cfg.write_text("%YAML:1.0\nflagDoUndistortion: 0\n" + cam("left") + cam("right") +
                   "T_lr: !!opencv-matrix\n  rows: 4\n  cols: 4\n  dt: f\n  data: [" + ",".join(repr(float(v)) for v in T_lr.reshape(-1)) + "]\n"
                   "feature_tracker.thres_error: 80.0\nfeature_tracker.thres_bidirection: 0.5\nfeature_tracker.thres_sampson: 60.0\n"
                   "feature_tracker.window_size: 21\nfeature_tracker.max_level: 4\nmap_update.thres_parallax: 1.0\n"
                   "feature_extractor.n_features: 2000\nfeature_extractor.n_bins_u: 20\nfeature_extractor.n_bins_v: 8\n"
                   "feature_extractor.thres_fastscore: 15.0\nfeature_extractor.radius: 5.0\nmotion_estimator.thres_1p_error: 120.0\n"
                   "motion_estimator.thres_5p_error: 1.0\nmotion_estimator.thres_poseba_error: 3.0\nkeyframe_update.thres_alive_ratio: 0.6\n"
                   "keyframe_update.thres_mean_parallax: 1.0\nkeyframe_update.thres_trans: 1.2\nkeyframe_update.thres_rotation: 15.0\n"
                   "keyframe_update.n_max_keyframes_in_window: 9\n")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out, kf = tmp_path / "traj.txt", tmp_path / "kf.txt"
    r = subprocess.run([sys.executable, os.path.join(root, "examples", "run_stereo_sequence.py"), "--config", str(cfg), "--left", str(dl),
                        "--right", str(dr), "--trajectory", str(out), "--keyframes", str(kf)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-1500:]
    svo = vo.StereoVO.from_yaml(str(cfg))
    ids, Ts = [], []
    for L, R in imgs:
        i = svo.trackStereoImages(L, R)
        ids.append(i.frame_id)
        Ts.append(np.array(i.T_wc, np.float32).reshape(4, 4))
    kfs = svo.getKeyframes()
    svo.close()
    vo.write_trajectory(str(tmp_path / "ref.txt"), ids, np.stack(Ts))
    assert open(out, "rb").read() == open(tmp_path / "ref.txt", "rb").read()
    assert len(open(out).read().splitlines()) == 7 and len(open(kf).read().splitlines()) == len(kfs) >= 2
