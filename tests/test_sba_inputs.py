"""The inputs of tests/test_sba_paths_gpu.py, checked on the CPU: the oracle (oracle/oracle_sba.c) solves every one of
them, each is well conditioned — so the 1e-9 / 1e-10 bar of the device test has orders of magnitude of room and a
deviation above it is the kernel's — and each really reaches the code path it is there for (observation and slot
counts, frame counts)."""
import numpy as np
import pytest

import util as U

# the point kernel's batch: SBA_NPRE = 3 rounds of SBA_LQ = 8 observations, the first SBA_LQ slots apart from the rest
# (sba.hip, sba_update_point_kernel); poses in LDS up to SBA_LDS_FRAMES = 32 frames; exp(log(T)) pre-staged up to 64
PREFETCHED_OBS, FIRST_SLOTS = 24, 8


def _solve_problem(case):
    k, n_points, stereo = case
    return U.sba_window(k, n_points, stereo)


def _relabel_problem(case):
    k, n_frames = case
    return U.sba_relabel(U.sba_window(k, 600, True), n_frames, seed=n_frames)


def _all_problems():
    for case in U.SBA_SOLVE_CASES:
        yield f"solve{case}", _solve_problem(case)
    for case in U.SBA_TIE_CASES:
        yield f"tie{case}", U.sba_tie_problem(*case)[0]
    for case in U.SBA_RELABEL_CASES:
        yield f"relabel{case}", _relabel_problem(case)[0]
    for m in U.SBA_HEAD_CASES:
        yield f"head({m})", U.sba_head(U.sba_window(9, 600, True), m)


def test_oracle_solves_every_input(oracle):
    """rc = 1, finite output, from several pixels down to the noise floor — for the windows of every solve size, the
    windows with an unobserved optimised keyframe, the relabelled windows and the structure-only heads."""
    n = 0
    for label, p in _all_problems():
        rc, T, X, err = U.sba_oracle(oracle, p)
        assert rc == 1, label
        assert np.all(np.isfinite(T)) and np.all(np.isfinite(X)), label
        assert U.sba_converged(err), (label, err[0], err[-1])
        n += 1
    assert n == len(U.SBA_SOLVE_CASES) + len(U.SBA_TIE_CASES) + len(U.SBA_RELABEL_CASES) + len(U.SBA_HEAD_CASES)


def test_inputs_are_well_conditioned(oracle):
    """One unit in the last place on every pixel and landmark coordinate, three draws: the oracle's output moves by
    less than 1e-11 (poses absolute, landmarks and errors relative to max(1, .)). A condition on the inputs: one that
    misses it is ill conditioned and has to be replaced, the device bar does not move."""
    worst = np.zeros(3)
    for label, p in _all_problems():
        ref = U.sba_oracle(oracle, p)
        for draw in range(3):
            dev = np.array(U.sba_deviation(U.sba_oracle(oracle, U.sba_ulp_perturbed(p, 100 + draw)), ref))
            assert dev.max() < 1e-11, (label, draw, dev)
            worst = np.maximum(worst, dev)
    print(f"oracle sensitivity to +-1 ulp, worst of all inputs: |dT| {worst[0]:.2e}  |dX| rel {worst[1]:.2e}  |derr| rel {worst[2]:.2e}")


@pytest.mark.parametrize("case", U.SBA_SOLVE_CASES)
def test_solve_cases_reach_the_tail_loops(case):
    """Stereo windows of 13 and more keyframes hold a landmark with more observations than the point kernel's batch
    takes, windows of 11 and more keyframes one with more slots than the first round; the sizes are the intended ones."""
    k, n_points, stereo = case
    p = _solve_problem(case)
    assert p["T_jw"].shape[0] == k and int(p["opt_index"].max()) + 1 == k - 2
    assert p["X"].shape[0] > 0.8 * n_points
    n_obs, n_slots = U.sba_obs_counts(p)
    if stereo and k >= 13:
        assert n_obs > PREFETCHED_OBS
    if k >= 11:
        assert n_slots > FIRST_SLOTS
    assert n_slots <= 2 * 20 + 64  # the host's slot table (SBA_MAX_OPT = 20)


@pytest.mark.parametrize("case", U.SBA_TIE_CASES)
def test_tie_problem_has_an_unobserved_optimised_keyframe(oracle, case):
    p, f = U.sba_tie_problem(*case)
    assert p["opt_index"][f] >= 0 and not np.any(p["obs_frame"] == f)
    assert np.diff(p["obs_ptr"]).min() >= 2 and p["obs_ptr"][-1] == len(p["obs_frame"]) == len(p["obs_px"])
    assert int(p["opt_index"].max()) + 1 == case[0] - 2  # the reduced system keeps its size: six of its rows are zero
    # the oracle leaves that pose where it was, up to the exp(log(T)) round trip of each iteration
    rc, T, X, err = U.sba_oracle(oracle, p)
    assert rc == 1 and np.abs(T[f] - p["T_jw"][f]).max() < 1e-12
    others = [g for g in range(case[0]) if p["opt_index"][g] >= 0 and g != f]
    assert all(np.abs(T[g] - p["T_jw"][g]).max() > 1e-6 for g in others)


@pytest.mark.parametrize("case", U.SBA_RELABEL_CASES)
def test_relabel_leaves_the_oracle_bit_identical(oracle, case):
    k, n_frames = case
    p = U.sba_window(k, 600, True)
    q, new = _relabel_problem(case)
    assert q["T_jw"].shape[0] == n_frames and new.max() == n_frames - 1 and len(set(new.tolist())) == k
    assert np.array_equal(q["opt_index"][new], p["opt_index"]) and (q["opt_index"] >= 0).sum() == k - 2
    assert np.array_equal(q["obs_ptr"], p["obs_ptr"]) and np.array_equal(q["obs_frame"], new[p["obs_frame"]])
    assert not np.array_equal(np.sort(new), new)  # frames are scattered, not merely shifted
    pad = np.ones(n_frames, bool)
    pad[new] = False
    assert np.all(q["opt_index"][pad] == -1) and np.all(q["T_jw"][pad] == np.eye(4))
    rc0, T0, X0, err0 = U.sba_oracle(oracle, p)
    rc1, T1, X1, err1 = U.sba_oracle(oracle, q)
    assert rc0 == rc1 == 1
    assert np.array_equal(T1[new], T0) and np.array_equal(X1, X0) and np.array_equal(err1, err0)
    assert np.array_equal(T1[pad], q["T_jw"][pad])


def test_head_and_rejection_inputs():
    p = U.sba_window(9, 600, True)
    for m in U.SBA_HEAD_CASES:
        q = U.sba_head(p, m)
        assert q["X"].shape[0] == m and q["obs_ptr"][-1] == len(q["obs_frame"]) and np.all(q["opt_index"] == -1)
    # 21 optimised poses, and a landmark with 105 left observations in optimised keyframes: one past each capacity
    assert int(U.sba_window(23, 200, False)["opt_index"].max()) + 1 == 21
    w = U.sba_window(6, 600, False)
    q = U.sba_repeat_observation(w, 105)
    assert U.sba_obs_counts(q)[1] == 105 and U.sba_obs_counts(w)[1] < 105
    assert q["obs_ptr"][-1] == len(q["obs_frame"]) == len(q["obs_px"]) > len(w["obs_frame"])
    assert q["X"].shape[0] == w["X"].shape[0] and np.all(np.diff(q["obs_ptr"]) >= 2)
