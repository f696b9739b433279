"""The local BA (sba.hip, vo_sba_solve) on the paths that the nine-keyframe windows of test_sba_gpu.py never reach:
every instantiation of the register solve, the general dense solve below and above 64 unknowns (and above 64 KiB of LDS),
the sequential pivot pre-pass behind exact ties, the point kernel's loops behind its prefetched batch, the frame-count
branches (poses read from HBM beyond 32 frames, no pre-staged exp(log(T)) beyond 64) and the host's capacity checks.
Every case is the device next to oracle.sba_solve at the bar of test_sba_gpu.py — 1e-9 on the poses, 1e-9 * max(1, |X|) on
the landmarks, 1e-10 * max(1, err) on the per-iteration errors — and has to have converged, so that parity on a problem
that never moved cannot pass. tests/test_sba_inputs.py checks the same inputs against the oracle alone: every one is
solvable and conditioned four orders of magnitude below the bar."""
import numpy as np
import pytest

import util as U

pytestmark = pytest.mark.gpu

VO_ERR_CAPACITY = -8  # include/vo_hip.h


def _group(k):
    return "reg" if k <= 10 else ("gen<=64" if k <= 12 else "gen>64")


@pytest.mark.parametrize("case", U.SBA_SOLVE_CASES)
def test_every_solve_instantiation(ctx, oracle, case):
    """n_kf = 3..10: sba_solve_reg_kernel<6..48>; 11, 12: sba_assemble_kernel + sba_solve_kernel with the ranked pivot
    order and the register sweeps; 13, 17, 22: its n > 64 path (17 and 22 with more than 64 KiB of dynamic LDS). The
    stereo windows from 13 keyframes on run the observation loop behind the prefetched 24, the windows from 11 on the
    slot loops behind the first 8 — asserted, so that a change of the generator cannot quietly take the loops out."""
    k, n_points, stereo = case
    p = U.sba_window(k, n_points, stereo)
    n_obs, n_slots = U.sba_obs_counts(p)
    if stereo and k >= 13:
        assert n_obs > 24
    if k >= 11:
        assert n_slots > 8
    ok, T, X, err = U.sba_run(ctx, oracle, p, label=f"{_group(k)} n_kf={k} M={p['X'].shape[0]} stereo={int(stereo)}")
    assert ok and U.sba_converged(err)


@pytest.mark.parametrize("stereo", [False, True])
@pytest.mark.parametrize("k", [3, 6, 9, 10])
def test_general_solve_behind_the_switch(ctx, oracle, k, stereo):
    """DBG_SBA_LDS_SOLVE sends the sizes of the register solve through the general kernel: within the bar of the oracle,
    and bit for bit what the register solve gives — both run the same operations in the same order (the pivot order
    from the original diagonal, the left-looking LDLT sums in increasing j, the L^T sweep in decreasing q)."""
    p = U.sba_window(k, 600, stereo)
    reg = U.sba_device(ctx, p)
    try:
        ctx.debug_set(ctx.DBG_SBA_LDS_SOLVE, 1)
        ok, T, X, err = U.sba_run(ctx, oracle, p, label=f"switch n_kf={k} stereo={int(stereo)}")
    finally:
        ctx.debug_set(ctx.DBG_SBA_LDS_SOLVE, 0)
    assert ok and U.sba_converged(err)
    same = bool(reg[0] == ok and np.array_equal(reg[1], T) and np.array_equal(reg[2], X) and np.array_equal(reg[3], err))
    print(f"sba bit-equality general vs register solve n_kf={k} stereo={int(stereo)}: {same}; "
          f"|dT| {np.abs(reg[1] - T).max():.3e} |dX| {np.abs(reg[2] - X).max():.3e} |derr| {np.abs(reg[3] - err).max():.3e}")
    assert same
    # the switch is off again: the same bits as before it was set
    again = U.sba_device(ctx, p)
    assert np.array_equal(again[1], reg[1]) and np.array_equal(again[2], reg[2])


@pytest.mark.parametrize("case", U.SBA_TIE_CASES)
def test_exact_pivot_ties(ctx, oracle, case):
    """An optimised keyframe without observations: its six diagonal entries are sums over nothing, a six-way exact tie
    at every iteration (and six zero pivots: the fabs(akk) > 0 and > tol ? : 0 guards). n_kf = 5, 9: the register kernel's
    sequential pre-pass; 12: the general kernel falls from the ranked order to the sequential one; 15: n > 64. Were a tie
    missed, the ranked order would not be a permutation. The unobserved pose stays put up to the exp(log(T)) round trip."""
    k, stereo = case
    p, f = U.sba_tie_problem(k, stereo)
    ok, T, X, err = U.sba_run(ctx, oracle, p, label=f"tie n_kf={k} stereo={int(stereo)}")
    assert ok and U.sba_converged(err)
    moved = np.abs(T[f] - p["T_jw"][f]).max()
    print(f"sba tie n_kf={k} stereo={int(stereo)}: the unobserved pose moved by {moved:.3e}")
    assert moved < 1e-12


@pytest.mark.parametrize("case", U.SBA_RELABEL_CASES)
def test_frame_count_branches(ctx, oracle, case):
    """The window's frames scattered among n_frames frames, the others fixed identity poses nobody observes: 33 takes
    sba_update_point_kernel<false> (poses from HBM), 65 and 100 the register solve without pre-staged exp(log(T)), 80 and
    90 the general solve. Parity with the oracle; the padding poses come back bit for bit; and the result is bit for bit
    that of the window under its own labels — no sum on the device runs in frame order."""
    k, n_frames = case
    p = U.sba_window(k, 600, True)
    q, new = U.sba_relabel(p, n_frames, seed=n_frames)
    ok, T, X, err = U.sba_run(ctx, oracle, q, label=f"relabel n_kf={k} n_frames={n_frames}")
    assert ok and U.sba_converged(err)
    pad = np.ones(n_frames, bool)
    pad[new] = False
    assert np.array_equal(T[pad], q["T_jw"][pad])
    fixed = new[p["opt_index"] < 0]
    assert np.array_equal(T[fixed], q["T_jw"][fixed])
    ok0, T0, X0, err0 = U.sba_device(ctx, p)
    same = bool(ok0 == ok and np.array_equal(T[new], T0) and np.array_equal(X, X0) and np.array_equal(err, err0))
    print(f"sba bit-equality relabelled vs own labels n_kf={k} n_frames={n_frames}: {same}; "
          f"|dT| {np.abs(T[new] - T0).max():.3e} |dX| {np.abs(X - X0).max():.3e} |derr| {np.abs(err - err0).max():.3e}")
    assert same


@pytest.mark.parametrize("m", U.SBA_HEAD_CASES)
def test_point_kernel_grid_edges(ctx, oracle, m):
    """Structure only (every pose fixed, at its true value so that the landmarks can reach the noise floor), the first
    m landmarks: one landmark in one workgroup with seven surplus lane groups, one short of a full workgroup, exactly
    one, one more, and eight workgroups and one landmark."""
    q = U.sba_head(U.sba_window(9, 600, True), m)
    ok, T, X, err = U.sba_run(ctx, oracle, q, label=f"head M={m}")
    assert ok and U.sba_converged(err)
    assert X.shape == (m, 3) and np.array_equal(T, q["T_jw"])


def test_host_rejections(ctx, oracle, vo):
    """One past each capacity: 21 optimised poses, and a landmark with 105 left observations in optimised keyframes.
    Both are refused on the host with VO_ERR_CAPACITY before anything is launched: an ordinary solve on the same
    context still matches the oracle."""
    from visual_odometry_ros_amd.api import SparseBundleAdjustmentSolver
    big = U.sba_window(23, 200, False)
    assert int(big["opt_index"].max()) + 1 == 21
    many = U.sba_repeat_observation(U.sba_window(6, 600, False), 105)
    assert U.sba_obs_counts(many)[1] == 105
    for p in (big, many):
        with pytest.raises(vo.VoError) as e:
            U.sba_device(ctx, p)
        assert e.value.code == VO_ERR_CAPACITY
    # 104 of them fit the host's table (and 20 optimised poses do: n_kf = 22 in test_every_solve_instantiation)
    fits = U.sba_repeat_observation(U.sba_window(6, 600, False), 104)
    sol = SparseBundleAdjustmentSolver(ctx, False)
    sol.setCamera(fits["K"])
    sol.setHuberThreshold(0.5)
    ok, T, X, err = sol.solveForFiniteIterations(0, *U.sba_args(fits))
    assert ok and np.array_equal(T, fits["T_jw"]) and np.array_equal(X, fits["X"])
    p = U.sba_window(6, 600, False)
    ok, T, X, err = U.sba_run(ctx, oracle, p, label="reg after rejections n_kf=6")
    assert ok and U.sba_converged(err)
