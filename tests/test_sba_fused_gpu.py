"""The local BA's fused iteration (sba.hip: sba_solve_point_kernel — the dense solve inside the point-update launch, two
launches per iteration) next to the three-launch iteration behind DBG_SBA_SPLIT = 1. Both run the same arithmetic in the same
order, so everything is compared bit for bit: success flag, poses, landmarks and the per-iteration errors. The split leg is
the one the other suites held against the oracle before the fused path existed; the fused results of the first and the
tie test are held against the oracle here as well. Switch values >= 2 cap the fused grid (a test hook), so that a small
problem makes every workgroup stride over several landmark groups."""
import contextlib
import os
import re

import numpy as np
import pytest

import util as U

gpu = pytest.mark.gpu


def _constants():
    """SBA_LQ (lanes per landmark) and SBA_FUSED_PW (point wavefronts per workgroup) of sba_device.hpp."""
    from visual_odometry_ros_amd import build as B
    text = open(os.path.join(B.CSRC, "sba_device.hpp")).read()
    return tuple(int(re.search(r"#define\s+" + name + r"\s+(\d+)", text).group(1)) for name in ("SBA_LQ", "SBA_FUSED_PW"))


SBA_LQ, SBA_FUSED_PW = _constants()
PER_GROUP = 64 // SBA_LQ               # landmarks of one wavefront
PER_PASS = SBA_FUSED_PW * PER_GROUP    # landmarks one workgroup takes per pass
EDGE_M = (PER_PASS - 1, PER_PASS, PER_PASS + 1, PER_PASS + PER_GROUP + 1)


@contextlib.contextmanager
def _switch(ctx, value):
    ctx.debug_set(ctx.DBG_SBA_SPLIT, value)
    try:
        yield
    finally:
        ctx.debug_set(ctx.DBG_SBA_SPLIT, 0)


_SPLIT = {}


def _split(ctx, key, p, iters=10):
    """The three-launch result of problem `key`, computed once."""
    if (key, iters) not in _SPLIT:
        with _switch(ctx, 1):
            _SPLIT[(key, iters)] = U.sba_device(ctx, p, iters)
    return _SPLIT[(key, iters)]


def _same(a, b, what):
    same = bool(a[0] == b[0] and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2]) and np.array_equal(a[3], b[3]))
    print(f"sba fused vs split {what}: {same}; |dT| {np.abs(a[1] - b[1]).max():.3e} |dX| {np.abs(a[2] - b[2]).max():.3e} "
          f"|derr| {np.abs(a[3] - b[3]).max() if a[3].size else 0.0:.3e}")
    return same


def _edge_problem(m):
    p = U.sba_window(9, 600, True)
    lm_of = np.repeat(np.arange(len(p["obs_ptr"]) - 1), np.diff(p["obs_ptr"]))
    q = U.sba_select(p, lm_of < m)
    assert q["X"].shape[0] == m
    return q


@gpu
@pytest.mark.parametrize("stereo", [False, True])
@pytest.mark.parametrize("k", range(3, 11))
def test_every_instantiation(ctx, oracle, k, stereo):
    """n_kf = 3..10: sba_solve_point_kernel<6..48, false / true>."""
    p = U.sba_window(k, 600, stereo)
    fused = U.sba_run(ctx, oracle, p, label=f"fused n_kf={k} stereo={int(stereo)}")
    assert fused[0] and U.sba_converged(fused[3])
    assert _same(fused, _split(ctx, ("win", k, stereo), p), f"n_kf={k} stereo={int(stereo)}")


@gpu
@pytest.mark.parametrize("cap", [2, 3])
def test_strided_point_phase(ctx, cap):
    """Two and three workgroups for the window's ~75 landmark groups: many passes each, an uneven remainder, and workgroup 0
    (which also keeps the record) striding too."""
    p = U.sba_window(9, 600, True)
    assert -(-p["X"].shape[0] // PER_GROUP) > 3 * cap * SBA_FUSED_PW and -(-p["X"].shape[0] // PER_GROUP) % (cap * SBA_FUSED_PW) != 0
    with _switch(ctx, cap):
        got = U.sba_device(ctx, p)
    assert got[0] and _same(got, _split(ctx, ("win", 9, True), p), f"grid cap {cap}")


@pytest.mark.parametrize("m", EDGE_M)
def test_grid_edge_problems_are_solvable(oracle, m):
    """(CPU) the cut windows of test_grid_edges: the oracle solves each."""
    rc, T, X, err = U.sba_oracle(oracle, _edge_problem(m))
    assert rc and np.all(np.isfinite(err)) and np.all(np.isfinite(T)) and np.all(np.isfinite(X))


@gpu
@pytest.mark.parametrize("m", EDGE_M)
def test_grid_edges(ctx, m):
    """Seven optimised poses and M landmarks: one short of, exactly and one more than what one workgroup takes per pass (the
    second workgroup then holds one landmark group of one landmark), and one landmark past a full landmark group."""
    p = _edge_problem(m)
    got = U.sba_device(ctx, p)
    ref = _split(ctx, ("edge", m), p)
    assert got[0] == ref[0] and _same(got, ref, f"M={m}")


@gpu
@pytest.mark.parametrize("iters", [1, 2, 3, 10])
def test_iteration_counts(ctx, iters):
    """Both parities of the pose ping-pong (an odd count starts from the second buffer: the first launch copies the poses
    across); the last iteration always writes the caller's block. Fixed keyframes come back bit for bit."""
    p = U.sba_window(9, 600, True)
    got = U.sba_device(ctx, p, iters)
    assert got[3].shape == (iters,)
    assert _same(got, _split(ctx, ("win", 9, True), p, iters), f"iterations={iters}")
    fixed = p["opt_index"] < 0
    assert fixed.any() and np.array_equal(got[1][fixed], p["T_jw"][fixed])


@gpu
def test_no_iteration(ctx):
    p = U.sba_window(9, 600, True)
    ok, T, X, err = U.sba_device(ctx, p, 0)
    assert ok and np.array_equal(T, p["T_jw"]) and np.array_equal(X, p["X"])


@gpu
@pytest.mark.parametrize("k", [5, 9])
def test_exact_pivot_ties(ctx, oracle, k):
    """The sequential tie pre-pass inside the fused kernel (an optimised keyframe without observations)."""
    p, f = U.sba_tie_problem(k, True)
    fused = U.sba_run(ctx, oracle, p, label=f"fused tie n_kf={k}")
    assert fused[0] and _same(fused, _split(ctx, ("tie", k), p), f"tie n_kf={k}")


@gpu
@pytest.mark.parametrize("which", ["33 frames", "no optimised pose", "n_kf=11"])
def test_fallbacks_untouched(ctx, which):
    """More than SBA_LDS_FRAMES frames, no optimised pose, more than eight optimised poses: the old kernels with the switch at
    0 and at 1."""
    if which == "33 frames":
        p = U.sba_relabel(U.sba_window(9, 600, True), 33, seed=33)[0]
    elif which == "no optimised pose":
        p = U.sba_head(U.sba_window(9, 600, True), 9)
    else:
        p = U.sba_window(11, 600, True)
    got = U.sba_device(ctx, p)
    assert got[0] and _same(got, _split(ctx, ("fallback", which), p), which)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _stereo_loop(vo, split):
    rig = U.RIG_640
    st = U.rig_stream(rig, n_u=20, n_v=8, seed=5, speed=0.5)
    imgs = [st.render_pair(p)[:2] for p in st.poses(12)]
    c = vo.Context(device=0, max_width=rig["width"], max_height=rig["height"], max_points=4096, n_slots=5, max_level=4)
    try:
        c.debug_set(c.DBG_SBA_SPLIT, split)
        svo = vo.StereoVO(c, rig["width"], rig["height"], st.K, st.Kr, st.T_lr, 20, 8, thres_fastscore=15, window_size=21, max_level=4,
                          strict_border=4, local_ba=True, thres_trans=1.0, thres_alive_ratio=0.6)
        log = []
        for k, (L, R) in enumerate(imgs):
            svo.enqueue(L, R)
            if k + 1 < len(imgs):
                svo.prefetch(*imgs[k + 1])
            gi = svo.result()
            g = svo.getTracks()
            log.append((_bits(np.array(gi.T_wc)).copy(), g["ids"].copy(), g["flags"].copy(), _bits(g["Xw"]).copy(),
                        bool(gi.is_keyframe), bool(gi.lba_ran), int(gi.lba_landmarks)))
        svo.close()
        return log
    finally:
        c.close()


class _TruePoseHook:
    """Stands for the 5-point pose: the scene's true relative pose of frame k against k - 1, every pair an inlier."""

    def __init__(self, poses):
        self.poses, self.k = poses, 0

    def __call__(self, pts0, pts1):
        T10 = np.linalg.inv(self.poses[self.k]) @ self.poses[self.k - 1]
        return True, T10[:3, :3].astype(np.float32), T10[:3, 3].astype(np.float32), np.ones(len(pts0), bool)


def _mono_loop(vo, split):
    from visual_odometry_ros_amd import synthetic as S
    W, H, nu, nv, n_frames = 752, 480, 40, 25, 14
    st = S.StereoStream(width=W, height=H, K=U.MONO_K, n_u=nu, n_v=nv, seed=5, speed=0.25)
    poses = st.poses(n_frames)
    imgs = [st.render_pair(p)[0] for p in poses]
    hook = _TruePoseHook(poses)
    c = vo.Context(device=0, max_width=W, max_height=H, max_points=2 * nu * nv + 512, n_slots=3, max_level=5)
    try:
        c.debug_set(c.DBG_SBA_SPLIT, split)
        mvo = vo.MonoVO(c, W, H, U.MONO_K, nu, nv, hook, thres_fastscore=15, window_size=15, max_level=5, thres_error=20.0,
                        thres_bidirection=1.0, thres_poseba_error=5, thres_sampson=1.0, thres_parallax=1.0, thres_translation=2.5,
                        strict_border=4, local_ba=True)
        log = []
        for k in range(n_frames):
            hook.k = k
            mvo.enqueue(imgs[k])
            if k + 1 < n_frames:
                mvo.prefetch(imgs[k + 1])
            gi = mvo.result()
            g = mvo.getTracks()
            log.append((_bits(np.array(gi.T_wc)).copy(), g["ids"].copy(), g["flags"].copy(), _bits(g["Xw"]).copy(),
                        bool(gi.is_keyframe), bool(gi.lba_ran), int(gi.lba_landmarks)))
        mvo.close()
        return log
    finally:
        c.close()


@gpu
@pytest.mark.parametrize("loop", ["stereo", "mono"])
def test_the_loop(vo, loop):
    """The closed loop with the local BA on, fused against split: per frame the pose bits, the track ids, the flags, the world
    points, the keyframe decisions and lba_ran. Stereo: the small rig of test_rig_gpu.py, 12 frames; mono: the 14 frames of
    test_mono_vo_gpu.py's local-BA loop."""
    run = _stereo_loop if loop == "stereo" else _mono_loop
    fused, split = run(vo, 0), run(vo, 1)
    assert sum(1 for e in fused if e[5]) >= 1
    for k, (a, b) in enumerate(zip(fused, split)):
        for x, y in zip(a, b):
            assert np.array_equal(x, y), (loop, k)
