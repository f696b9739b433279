"""MonoVO's pose covariance (vo_mvo_set_pose_covariance) on the smallest stream of tests/test_mono_vo_gpu.py, made
to take the 5-point fallback: no local BA and a keyframe at every frame, so that from the sixth window keyframe on the pose-only
BA's class (bundled landmarks, mono_vo.cpp:800-826) is empty. Frames 0 (first image) and 1 (initialisation) have no BA pose,
frames 2-5 do, frames 6-7 fall back. The option changes no bit of what the loop returns and allocates only when it is set."""
import ctypes as C

import numpy as np
import pytest

import pose_covariance_restatement as PR
from test_mono_vo_gpu import MONO_K

pytestmark = pytest.mark.gpu

W, H, NU, NV, N_FRAMES = 752, 480, 40, 25, 8
HOOK_FRAMES = (1, 6, 7)  # the frames that call the 5-point hook, in order


class SequencedPoseHook:
    """The scene's true relative pose, for the frames that are known to ask for it (in that order): usable from inside the
    library's own loop, where no test code runs between frames."""

    def __init__(self, poses):
        self.poses, self.calls = poses, 0

    def __call__(self, pts0, pts1):
        k = HOOK_FRAMES[self.calls]
        self.calls += 1
        T10 = np.linalg.inv(self.poses[k]) @ self.poses[k - 1]
        return True, T10[:3, :3].astype(np.float32), T10[:3, 3].astype(np.float32), np.ones(len(pts0), bool)


@pytest.fixture(scope="module")
def stream():
    from visual_odometry_ros_amd import synthetic as S
    st = S.StereoStream(width=W, height=H, K=MONO_K, n_u=NU, n_v=NV, seed=5, speed=0.25)
    poses = st.poses(N_FRAMES)
    return poses, [st.render_pair(p)[0] for p in poses]


def _run(vo, stream, mode, cov, check=None):
    poses, imgs = stream
    hook = SequencedPoseHook(poses)
    c = vo.Context(device=0, max_width=W, max_height=H, max_points=2 * NU * NV + 512, n_slots=3, max_level=5)
    try:
        a_before = c.allocation_count()
        mvo = vo.MonoVO(c, W, H, MONO_K, NU, NV, hook, thres_fastscore=15, window_size=15, max_level=5, thres_error=20.0,
                        thres_bidirection=1.0, thres_poseba_error=5, thres_sampson=1.0, thres_parallax=1.0, thres_translation=0.4,
                        strict_border=1, local_ba=False)
        a_made = c.allocation_count()
        if cov:
            mvo.setPoseCovariance(True)
        a_set = c.allocation_count()
        infos, tracks, allocs = [], [], {}
        if mode == "sync":
            for k in range(N_FRAMES):
                i = mvo.trackImage(imgs[k])
                infos.append(i)
                g = mvo.getTracks()
                tracks.append((g["ids"].copy(), g["flags"].copy(), g["pts"].copy()))
                if check:
                    check(mvo, c, k, i)
                allocs[k] = c.allocation_count()
        else:
            infos, _ = mvo.runSequence(imgs)
            g = mvo.getTracks()
            tracks.append((g["ids"].copy(), g["flags"].copy(), g["pts"].copy()))
            if check:
                check(mvo, c, N_FRAMES - 1, infos[-1])
        a_end = c.allocation_count()
        assert hook.calls == len(HOOK_FRAMES)
        assert [bool(i.used_five_point) for i in infos] == [k in HOOK_FRAMES for k in range(N_FRAMES)]
        mvo.close()
        raw = [bytes(C.string_at(C.addressof(i), C.sizeof(i))) for i in infos]
        return raw, tracks, dict(before=a_before, made=a_made, set=a_set, frames=allocs, end=a_end)
    finally:
        c.close()


def _same(a, b):
    return len(a) == len(b) and all(all(np.array_equal(p, q) for p, q in zip(x, y)) for x, y in zip(a, b))


def test_option_changes_no_bit_and_allocates_only_when_set(vo, stream):
    off, tr_off, al_off = _run(vo, stream, "sync", False)
    on, tr_on, al_on = _run(vo, stream, "sync", True)
    assert off == on and _same(tr_off, tr_on)
    assert al_off["set"] == al_off["made"] and al_on["set"] - al_on["made"] == 2  # only at the set call
    assert all(al_on["frames"][k] - al_off["frames"][k] == 2 for k in range(N_FRAMES))  # the frames add nothing to it
    assert al_on["frames"][2] == al_on["frames"][5]  # vo_debug_allocation_count does not move over the steady-state frames
    r_off, rt_off, ar_off = _run(vo, stream, "run", False)
    r_on, rt_on, ar_on = _run(vo, stream, "run", True)
    assert r_off == r_on and _same(rt_off, rt_on)
    assert ar_on["end"] - ar_off["end"] == 2


def test_covariance_follows_the_operator_and_the_chain(vo, stream):
    state = dict(P=np.zeros((6, 6)), unknown=0, last=None, carried_nonzero=0)

    def check(mvo, c, k, info):
        cov = mvo.getPoseCovariance()
        where = f"frame {k}"
        T01 = np.array(info.dT01, np.float32).reshape(4, 4)
        T_wc = np.array(info.T_wc, np.float32).reshape(4, 4)
        if k in (0,) + HOOK_FRAMES:  # first image, initialisation, 5-point fallback: no BA pose, P is only carried
            if k == 0:
                T01 = np.eye(4, dtype=np.float32)
            state["unknown"] += 1
            state["carried_nonzero"] += int(state["P"].any())
            state["P"] = vo.propagate_pose_covariance(state["P"], PR.inv_se3(T01.astype(np.float64)), None)
            assert not cov.valid and not cov.Sigma_xi.any() and cov.s2 == 0.0, where
        else:
            inp = mvo.getPoseCovarianceInputs()
            assert len(inp["X"]) == cov.n_points == info.counts.n_ba > 10, where
            assert np.array_equal(inp["R01"].view(np.uint32), T01[:3, :3].copy().view(np.uint32)), where
            assert np.array_equal(inp["t01"].view(np.uint32), T01[:3, 3].copy().view(np.uint32)), where
            op = vo.MotionEstimator(c).poseInformation(inp["X"], inp["pts"], MONO_K, inp["R01"], inp["t01"])
            assert op.valid and cov.valid and cov.s2 == op.s2, where
            assert np.array_equal(cov.Sigma_xi.view(np.uint64), op.Sigma.view(np.uint64)), where  # bit for bit
            state["P"] = vo.propagate_pose_covariance(state["P"], PR.inv_se3(T01.astype(np.float64)), op.Sigma)
        assert cov.n_unknown_steps == state["unknown"], where
        scale = np.abs(state["P"]).max()
        assert np.abs(cov.P - state["P"]).max() <= 1e-12 * scale, where
        assert np.array_equal(cov.P, cov.P.T), where
        assert np.array_equal(mvo.getPoseCovarianceRos(), vo.pose_covariance_ros(cov.P, T_wc)), where
        state["last"] = cov

    _run(vo, stream, "sync", True, check)
    assert state["unknown"] == 1 + len(HOOK_FRAMES) and state["carried_nonzero"] == 2  # (frames 6 and 7 carry a P that is not zero)
    got = {}
    _run(vo, stream, "run", True, lambda mvo, c, k, info: got.update(cov=mvo.getPoseCovariance()))
    assert np.array_equal(got["cov"].P.view(np.uint64), state["last"].P.view(np.uint64))
    assert got["cov"].n_unknown_steps == state["last"].n_unknown_steps


def test_option_is_refused_while_a_frame_is_in_flight(vo, stream):
    poses, imgs = stream
    c = vo.Context(device=0, max_width=W, max_height=H, max_points=2 * NU * NV + 512, n_slots=3, max_level=5)
    try:
        mvo = vo.MonoVO(c, W, H, MONO_K, NU, NV, SequencedPoseHook(poses), thres_fastscore=15, window_size=15, max_level=5,
                        strict_border=1, local_ba=False)
        with pytest.raises(vo.VoError):
            mvo.getPoseCovariance()  # the option is off
        mvo.enqueue(imgs[0])
        with pytest.raises(vo.VoError):
            mvo.setPoseCovariance(True)
        mvo.result()
        mvo.setPoseCovariance(True, 0.5)
        mvo.enqueue(imgs[1])
        with pytest.raises(vo.VoError):
            mvo.getPoseCovariance()
        mvo.result()
        assert mvo.getPoseCovariance().n_unknown_steps == 1
        mvo.close()
    finally:
        c.close()
