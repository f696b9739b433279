"""The stereo operators on a rig of two DIFFERENT cameras whose right camera is rotated and shifted along all three
axes (util.RIG_*), the pose-only BA from an initial pose that is not the identity, and at the point counts where its
kernel changes path. The other device tests pass the same intrinsics twice and a pure x-translation, on which K_l read for
K_r, R_rl transposed, T_lr used for its inverse, t_y / t_z dropped or fx / fy swapped in the right camera change nothing;
tests/test_rig_inputs.py shows on the CPU that every input used here tells those mistakes apart. Bars are the existing
ones: bits against oracle(SUM_TREE, 512), masks / stages / counts equal to oracle(SUM_SEQ), pose within 1e-4 relative
Frobenius of oracle(SUM_SEQ), frame dT within 1e-6, local BA at the bar of util.sba_run."""
import numpy as np
import pytest

import util as U
from test_frame_gpu import _run_stream
from test_gn_gpu import mono_gn_parity, stereo_gn_parity
from test_stereo_vo_gpu import _run_both
from visual_odometry_ros_amd import synthetic as S

pytestmark = pytest.mark.gpu


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ---- pose-only BA -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("identity", [True, False])
@pytest.mark.parametrize("n", U.RIG_GN_COUNTS)
def test_stereo_gn_parity_on_the_rig(ctx, vo, oracle, n, identity):
    """vo_gn_enqueue inverts T0 on the host (inverse_se3_host) before gn_pose_kernel<true> sees it: with the identity that
    is the identity; the second T0 is the truth moved by 0.03 m / 0.004 rad, rounded to float32."""
    d = U.rig_two_view(n=n, seed=U.RIG_GN_SEED[n])
    dev = stereo_gn_parity(ctx, vo, oracle, d, d["Kr"], U.rig_gn_T0(d, identity))
    print(f"stereo GN on the rig, n {n}, T0 identity {identity}: pose bits equal TREE, rel. Frobenius vs SEQ {dev:.2e}")


@pytest.mark.parametrize("identity", [True, False])
def test_stereo_gn_noise_free_recovers_truth_on_the_rig(ctx, vo, identity):
    d = U.rig_two_view(n=800, seed=11, noise_px=0.0, outlier_frac=0.0)
    me = vo.MotionEstimator(ctx, True, d["T_lr"])
    ok, T, mask, info = me.poseOnlyBundleAdjustment_Stereo(d["X"], d["pts_l"], d["pts_r"], d["K"], d["Kr"], d["T_lr"], 3.0,
                                                          U.rig_gn_T0(d, identity))
    print(f"stereo GN noise-free on the rig, T0 identity {identity}: |T - T_true| max {np.abs(T - d['T01_true']).max():.2e}")
    assert ok and mask.all()
    assert np.abs(T - d["T01_true"]).max() < 1e-5


def test_stereo_gn_reference_order_on_the_rig(vo, oracle):
    """The reference summation order past the points kept in registers, from the perturbed T0: oracle(SUM_SEQ) bit for bit."""
    d = U.rig_two_view(n=2049, seed=U.RIG_GN_SEED[2049])
    T0 = U.rig_gn_T0(d, False)
    c = vo.Context(device=0, max_width=640, max_height=480, max_points=4096, n_slots=2, max_level=2, sum_order="reference")
    try:
        me = vo.MotionEstimator(c, True, d["T_lr"])
        ok, T, mask, info = me.poseOnlyBundleAdjustment_Stereo(d["X"], d["pts_l"], d["pts_r"], d["K"], d["Kr"], d["T_lr"], 3.0, T0)
    finally:
        c.close()
    rc, T_s, mask_s, info_s = oracle.gn_pose_stereo(d["X"], d["pts_l"], d["pts_r"], d["K"], d["Kr"], d["T_lr"], 3.0, T0,
                                                    oracle.SUM_SEQ, 0)
    assert ok == bool(rc)
    assert info.iterations == info_s.iterations and info.cnt_invalid == info_s.cnt_invalid
    assert np.array_equal(mask, mask_s)
    assert np.array_equal(_bits(T), _bits(T_s))
    assert _bits(info.err) == _bits(info_s.err) and _bits(info.delta_norm) == _bits(info_s.delta_norm)


@pytest.mark.parametrize("identity", [True, False])
@pytest.mark.parametrize("variant", [0, 1])
@pytest.mark.parametrize("n", U.MONO_GN_COUNTS)
def test_mono_gn_parity_past_the_register_points(ctx, vo, oracle, n, variant, identity):
    """More than GN_PC * GN_T = 2048 points: the mono kernel's reload loop. The second (R0, t0) is a rotation rounded to
    float32, so inverse4x4_host (the 4 x 4 cofactor inverse standing for Matrix4f::inverse()) is not handed R0^T's twin."""
    d = S.two_view_points(n=n, seed=U.MONO_GN_SEED[n], K=U.MONO_K)
    T0 = U.rig_gn_T0(d, identity)
    R0, t0 = np.ascontiguousarray(T0[:3, :3]), np.ascontiguousarray(T0[:3, 3])
    dev = mono_gn_parity(ctx, vo, oracle, d, R0, t0, variant)
    print(f"mono GN, n {n}, variant {variant}, T0 identity {identity}: pose bits equal TREE, rel. Frobenius vs SEQ {dev:.2e}")


# ---- stereo frame -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("strict", [False, True, 3, 5])
def test_stereo_frame_on_the_rig(ctx, oracle, strict):
    """stereo_prior_kernel, the prior block of frame_track_kernel and gn_pose_kernel<true> inside the frame, 40 features at
    320 x 200. The pose-against-truth bar of _run_stream is for KITTI-sized frames (the oracle itself is 3e-3 ... 1.3e-2 off
    the truth at this size, on either rig): more than half of the features must be BA inliers instead."""
    stream = U.rig_stream(U.RIG_320, n_u=8, n_v=5, n_new=10, seed=4, margin=5.0 if strict else 16.0)
    worst_t, worst_s = _run_stream(ctx, oracle, stream, 3, strict, win=21, max_level=3, sanity=False, min_inlier_frac=0.5)
    print(f"stereo frame on the rig, strict {strict}: dT rel. Frobenius vs TREE {worst_t:.2e}, vs SEQ {worst_s:.2e}")


# ---- closed loop ------------------------------------------------------------------------------------------------------------
_LOOP = {}


def _loop_frames():
    if not _LOOP:
        st = U.rig_stream(U.RIG_640, n_u=20, n_v=8, seed=5, speed=0.5)
        _LOOP["frames"] = (st, [st.render_pair(p)[:2] for p in st.poses(12)])
    return _LOOP["frames"]


@pytest.mark.parametrize("strict,prefetch,lba,kf_trans", [(4, True, True, 1.0), (1, False, False, 10.0)])
def test_closed_loop_on_the_rig(vo, oracle, strict, prefetch, lba, kf_trans):
    """svo_make_cam / the DLT workers, the keyframe reconstruction's right-camera reprojection, the new-landmark check and
    stereo_vo_lba.hip's scaled T_lr and K_r, where the two cameras are not interchangeable; the frames run in the world-frame
    mode (T_pw, the products with T_rl). Every per-frame bit assertion of _run_both."""
    rig = U.RIG_640
    frames = _loop_frames()
    st = frames[0]
    log, ref = _run_both(vo, oracle, rig["width"], rig["height"], st.K, 20, 8, frames, 21, 4, 12, lba=lba, strict=strict,
                         prefetch=prefetch, kf_trans=kf_trans, K_r=st.Kr, T_lr=st.T_lr)
    print(f"closed loop on the rig, strict {strict}, local BA {lba}: {sum(1 for e in log if e[0])} keyframes, "
          f"{sum(1 for e in log if e[2])} local-BA solves, {log[-1][1]} tracks: every frame's bits equal the CPU loop's")
    assert sum(1 for e in log if e[0]) >= 2
    assert log[-1][1] > 150
    if lba:
        assert sum(1 for e in log if e[2]) >= 1, log
