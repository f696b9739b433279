"""The one-wavefront dense solve of the local BA (sba.hip: sba_reg_solve_wave<N>, inlined by sba_solve_reg_kernel<N> and
sba_solve_point_kernel<N, LAST>) next to the general LDS solver (sba_solve_kernel behind DBG_SBA_LDS_SOLVE), which shares no
code with it: both run the same operations in the same order — the pivot order from the original diagonal, the left-looking
LDLT sums in increasing j, the L^T sweep in decreasing q — so the success flag, poses, landmarks and per-iteration errors have
to be the same bits, for every instantiation N = 6 ... 48, on the fused path and on the three-launch path (DBG_SBA_SPLIT = 1).
The register solve pairs its lane broadcasts two columns at a time and runs the L^T sweep out of a batch of registers: N = 6 and
12 have fewer columns than a pair pipeline is deep, odd and even remainders occur at every N, N = 48 has the most registers
live. A bit-equal pair of wrong answers cannot pass: every problem is solved by the oracle too (finite), and the windows are
within the bars of test_sba_paths_gpu.py of it."""
import numpy as np
import pytest

import util as U

pytestmark = pytest.mark.gpu

_ORACLE = {}  # (problem key, iterations) -> the oracle's (rc, T, X, err): solved once, shared, never written to


def _oracle(oracle, key, p, iters=10):
    if (key, iters) not in _ORACLE:
        ref = U.sba_oracle(oracle, p, iters)
        for a in ref[1:]:
            a.setflags(write=False)
        _ORACLE[(key, iters)] = ref
    return _ORACLE[(key, iters)]


def _device(ctx, p, iters, split, lds):
    try:
        ctx.debug_set(ctx.DBG_SBA_SPLIT, split)
        ctx.debug_set(ctx.DBG_SBA_LDS_SOLVE, lds)
        return U.sba_device(ctx, p, iters)
    finally:
        ctx.debug_set(ctx.DBG_SBA_LDS_SOLVE, 0)
        ctx.debug_set(ctx.DBG_SBA_SPLIT, 0)


def _pair(ctx, p, iters, split, label):
    """(register solve, general solve) of one problem; asserts that they are the same bits."""
    reg = _device(ctx, p, iters, split, 0)
    gen = _device(ctx, p, iters, split, 1)
    same = bool(reg[0] == gen[0] and np.array_equal(reg[1], gen[1]) and np.array_equal(reg[2], gen[2])
                and np.array_equal(reg[3], gen[3]))
    d_err = np.abs(reg[3] - gen[3]).max() if reg[3].size else 0.0
    print(f"sba solve wave {label} split={split} iters={iters}: same bits {same}; |dT| {np.abs(reg[1] - gen[1]).max():.3e} "
          f"|dX| {np.abs(reg[2] - gen[2]).max():.3e} |derr| {d_err:.3e}")
    assert same
    return reg, gen


def _finite(ref):
    rc, T, X, err = ref
    return bool(np.all(np.isfinite(T)) and np.all(np.isfinite(X)) and np.all(np.isfinite(err)))


@pytest.mark.parametrize("split", [0, 1])
@pytest.mark.parametrize("stereo", [False, True])
@pytest.mark.parametrize("k", [3, 4, 5, 6, 7, 8, 9, 10])
def test_every_instantiation_is_the_general_solver_bit_for_bit(ctx, oracle, k, stereo, split):
    """n_kf = 3 ... 10: sba_reg_solve_wave<6 ... 48>, inside sba_solve_point_kernel (split = 0) and sba_solve_reg_kernel
    (split = 1). Ten iterations; and within 1e-9 / 1e-9 / 1e-10 of the oracle, whose output is finite."""
    p = U.sba_window(k, 600, stereo)
    ref = _oracle(oracle, ("window", k, stereo), p)
    assert _finite(ref)
    reg, _ = _pair(ctx, p, 10, split, f"n_kf={k} stereo={int(stereo)}")
    ok, T, X, err = reg
    rc, T_o, X_o, err_o = ref
    dev = U.sba_deviation(reg, ref)
    print(f"sba solve wave n_kf={k} stereo={int(stereo)} split={split} vs oracle: |dT| {dev[0]:.3e} |dX| rel {dev[1]:.3e} "
          f"|derr| rel {dev[2]:.3e}")
    assert ok and rc == int(ok) and U.sba_converged(err)
    assert np.abs(err - err_o).max() <= 1e-10 * max(1.0, err_o.max())
    assert np.abs(T - T_o).max() < 1e-9 and np.abs(X - X_o).max() < 1e-9 * max(1.0, np.abs(X_o).max())


@pytest.mark.parametrize("split", [0, 1])
@pytest.mark.parametrize("k", [5, 9])
def test_pivot_ties_and_a_zero_pivot(ctx, oracle, k, split):
    """An optimised keyframe nobody observes: six exactly equal (zero) diagonal entries at every iteration — the sequential
    pivot pre-pass, then the factorisation and both sweeps on a permutation that is not a sort, and six columns behind the
    fabs(ajj) > 0 guard."""
    p, f = U.sba_tie_problem(k, True)
    ref = _oracle(oracle, ("tie", k), p)
    assert _finite(ref)
    reg, _ = _pair(ctx, p, 10, split, f"tie n_kf={k}")
    assert reg[0] and ref[0] == 1 and U.sba_converged(reg[3])


@pytest.mark.parametrize("split", [0, 1])
@pytest.mark.parametrize("iters", [1, 2])
def test_first_iterations(ctx, oracle, iters, split):
    """One and two iterations of the nine-keyframe stereo window: a difference is pinned where it arises, before ten
    iterations could blur it."""
    p = U.sba_window(9, 600, True)
    ref = _oracle(oracle, ("window", 9, True), p, iters)
    assert _finite(ref)
    reg, _ = _pair(ctx, p, iters, split, "n_kf=9 stereo=1")
    assert ref[0] == int(reg[0]) and reg[3].shape == ref[3].shape  # (the flag is the oracle's, whatever one iteration gives)
    assert np.abs(reg[3] - ref[3]).max() <= 1e-10 * max(1.0, ref[3].max())
