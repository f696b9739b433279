"""Shared helpers for the test-suite: seeded synthetic image pairs."""
import numpy as np
from scipy import ndimage


def texture(h, w, seed=0, sigma=1.5, contrast=60.0):
    rng = np.random.default_rng(seed)
    a = ndimage.gaussian_filter(rng.standard_normal((h, w)), sigma)
    b = ndimage.gaussian_filter(rng.standard_normal((h, w)), sigma * 4)
    t = a / a.std() + 1.5 * b / b.std()
    return np.clip(128 + contrast * t / 1.8, 0, 255)


def warp(img_f, dx=0.0, dy=0.0, scale=1.0, angle=0.0):
    """Sample img at the inverse similarity so that a point p moves to c + s R (p - c) + d."""
    h, w = img_f.shape
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    cx, cy = (w - 1) / 2.0, (h - 1) / 2.0
    ca, sa = np.cos(angle), np.sin(angle)
    x = xx - cx - dx
    y = yy - cy - dy
    xs = (ca * x + sa * y) / scale + cx
    ys = (-sa * x + ca * y) / scale + cy
    return ndimage.map_coordinates(img_f, [ys, xs], order=3, mode="reflect")


def move_points(pts, shape, dx=0.0, dy=0.0, scale=1.0, angle=0.0):
    h, w = shape
    cx, cy = (w - 1) / 2.0, (h - 1) / 2.0
    ca, sa = np.cos(angle), np.sin(angle)
    x, y = pts[:, 0] - cx, pts[:, 1] - cy
    return np.stack([scale * (ca * x - sa * y) + cx + dx, scale * (sa * x + ca * y) + cy + dy], 1)


def image_pair(h=240, w=320, seed=0, **motion):
    base = texture(h, w, seed)
    img0 = np.rint(base).astype(np.uint8)
    img1 = np.rint(np.clip(warp(base, **motion), 0, 255)).astype(np.uint8)
    return img0, img1


def grid_points(h, w, step=17, margin=12, jitter_seed=1):
    rng = np.random.default_rng(jitter_seed)
    ys, xs = np.mgrid[margin:h - margin:step, margin:w - margin:step]
    pts = np.stack([xs.ravel(), ys.ravel()], 1).astype(np.float64)
    pts += rng.uniform(-0.5, 0.5, pts.shape)
    return pts.astype(np.float32)


class DeviceBuffer:
    """A raw HIP allocation holding a copy of a numpy array (through the HIP runtime libvo_hip.so is
    already linked to — no torch, whose bundled runtime must not be initialised after it)."""

    def __init__(self, arr):
        import ctypes as C
        self._C = C
        self.hip = C.CDLL("libamdhip64.so.7")
        a = np.ascontiguousarray(arr)
        self.ptr = C.c_void_p()
        assert self.hip.hipMalloc(C.byref(self.ptr), C.c_size_t(a.nbytes)) == 0
        assert self.hip.hipMemcpy(self.ptr, a.ctypes.data_as(C.c_void_p), C.c_size_t(a.nbytes), 1) == 0  # H2D

    def data_ptr(self):
        return self.ptr.value

    def free(self):
        if self.ptr:
            self.hip.hipFree(self.ptr)
            self.ptr = self._C.c_void_p()


# ---- sparse local BA (test_sba_gpu.py, test_sba_paths_gpu.py, test_sba_inputs.py) -------------------------------------
# Input builders and the parity check against oracle.sba_solve. A problem is the dict synthetic.ba_window returns; the
# builders return new dicts (arrays they change are copies) and never touch the window they were given.
SBA_FIELDS = ("T_jw", "opt_index", "X", "obs_ptr", "obs_frame", "obs_right", "obs_px")
SBA_MEASURED = []  # (label, |dT|, |dX| / max(1, |X|), |derr| / max(1, err)) of every sba_run, for the DESIGN.md table


def sba_args(p):
    return tuple(p[k] for k in SBA_FIELDS)


def sba_oracle(oracle, p, iters=10):
    stereo = p["stereo"]
    return oracle.sba_solve(*sba_args(p), p["K"], p.get("Kr", p["K"]) if stereo else None,
                            p["T_lr"] if stereo else None, 0.5, iters)


def sba_device(ctx, p, iters=10):
    from visual_odometry_ros_amd.api import SparseBundleAdjustmentSolver
    stereo = p["stereo"]
    sol = SparseBundleAdjustmentSolver(ctx, stereo)
    if stereo:
        sol.setStereoCameras(p["K"], p.get("Kr", p["K"]), p["T_lr"])
    else:
        sol.setCamera(p["K"])
    sol.setHuberThreshold(0.5)
    return sol.solveForFiniteIterations(iters, *sba_args(p))


def sba_deviation(got, ref):
    """(max |dT|, max |dX| / max(1, max |X_ref|), max |derr| / max(1, max err_ref)): the three figures the bar is on."""
    (_, T, X, err), (_, T_o, X_o, err_o) = got, ref
    d_err = np.abs(err - err_o).max() / max(1.0, err_o.max()) if err_o.size else 0.0
    return np.abs(T - T_o).max(), np.abs(X - X_o).max() / max(1.0, np.abs(X_o).max()), d_err


def sba_run(ctx, oracle, p, iters=10, label=None):
    """The device solve next to the oracle's: same success flag, per-iteration average errors to 1e-10 * max(1, err),
    poses to 1e-9 absolute, landmarks to 1e-9 * max(1, |X|). Returns the device's (ok, T, X, err)."""
    got = sba_device(ctx, p, iters)
    ref = sba_oracle(oracle, p, iters)
    ok, T, X, err = got
    rc, T_o, X_o, err_o = ref
    dev = sba_deviation(got, ref)
    SBA_MEASURED.append((label,) + tuple(float(v) for v in dev))
    print(f"sba parity {label}: |dT| {dev[0]:.3e}  |dX| rel {dev[1]:.3e}  |derr| rel {dev[2]:.3e}")
    assert rc == int(ok)
    assert np.abs(err - err_o).max() <= 1e-10 * max(1.0, err_o.max())
    assert np.abs(T - T_o).max() < 1e-9 and np.abs(X - X_o).max() < 1e-9 * max(1.0, np.abs(X_o).max())
    return ok, T, X, err


def sba_converged(err):
    """The solve moved: from several pixels to the floor of the 0.3 px observation noise (~0.42 px RMS)."""
    return bool(np.all(np.isfinite(err)) and err[0] > 1.0 and err[-1] < 0.6)


_SBA_WINDOWS = {}


def sba_window(n_kf, n_points=600, stereo=True, seed=None):
    """synthetic.ba_window(n_kf, n_points, stereo, seed = n_kf unless given), generated once per process."""
    from visual_odometry_ros_amd import synthetic as S
    key = (n_kf, n_points, bool(stereo), n_kf if seed is None else seed)
    if key not in _SBA_WINDOWS:
        _SBA_WINDOWS[key] = S.ba_window(n_kf=key[0], n_points=key[1], stereo=key[2], seed=key[3])
    return _SBA_WINDOWS[key]


# every solve instantiation: n_kf = 3..10 are sba_solve_reg_kernel<6..48>; 11, 12 the general kernel with n <= 64;
# 13, 17, 22 (11, 15, 20 optimised poses) the general kernel with n > 64, from 15 poses on with more than 64 KiB of LDS
SBA_SOLVE_CASES = [(k, 600, s) for k in (3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 17, 22) for s in (False, True)] + [(22, 3000, True)]
SBA_TIE_CASES = [(k, s) for k in (5, 9, 12, 15) for s in (False, True)]
SBA_RELABEL_CASES = [(9, 33), (9, 65), (9, 100), (14, 80), (22, 90)]
SBA_HEAD_CASES = [1, 7, 8, 9, 65]


def sba_obs_counts(p):
    """(most observations of one landmark, most left observations in optimised keyframes — slots — of one landmark)"""
    ptr = p["obs_ptr"]
    slot = (p["opt_index"][p["obs_frame"]] >= 0) & (p["obs_right"] == 0)
    n_slot = np.add.reduceat(slot.astype(np.int64), ptr[:-1])
    return int(np.diff(ptr).max()), int(n_slot.max())


def sba_select(p, keep_obs, min_seen=2):
    """The problem with the observations of the boolean mask only; landmarks left with fewer than min_seen are dropped."""
    ptr = p["obs_ptr"]
    lm_of = np.repeat(np.arange(len(ptr) - 1), np.diff(ptr))
    cnt = np.bincount(lm_of[keep_obs], minlength=len(ptr) - 1)
    lm_keep = cnt >= min_seen
    ok = keep_obs & lm_keep[lm_of]
    q = dict(p)
    for name in ("obs_frame", "obs_right", "obs_px"):
        q[name] = p[name][ok].copy()
    q["obs_ptr"] = np.concatenate([[0], np.cumsum(cnt[lm_keep])]).astype(np.int32)
    q["X"] = p["X"][lm_keep].copy()
    q["X_true"] = p["X_true"][lm_keep].copy()
    return q


def sba_tie_problem(n_kf, stereo):
    """A window whose optimised keyframe in the middle has lost every observation: its 6 x 6 diagonal block, its
    off-diagonal blocks and its right-hand side are sums over nothing — six bit-identical (zero) diagonal entries at every
    iteration. Returns (problem, index of that frame)."""
    p = sba_window(n_kf, 600, stereo)
    f = 2 + (n_kf - 2) // 2
    assert p["opt_index"][f] >= 0
    return sba_select(p, p["obs_frame"] != f), f


def sba_relabel(p, n_frames, seed):
    """The same problem among n_frames frames: the window's frames go to distinct random indices, one of them
    n_frames - 1, every other frame is an identity pose that is fixed (opt_index -1) and that nothing observes.
    Observation lists keep their order; obs_frame is rewritten. Returns (problem, new index of every old frame)."""
    n_old = p["T_jw"].shape[0]
    assert n_frames >= n_old
    rng = np.random.default_rng(seed)
    new = np.append(rng.choice(n_frames - 1, n_old - 1, replace=False), n_frames - 1)
    new = rng.permutation(new).astype(np.int32)
    q = dict(p)
    q["T_jw"] = np.tile(np.eye(4), (n_frames, 1, 1))
    q["T_jw"][new] = p["T_jw"]
    q["T_jw_true"] = np.tile(np.eye(4), (n_frames, 1, 1))
    q["T_jw_true"][new] = p["T_jw_true"]
    q["opt_index"] = np.full(n_frames, -1, np.int32)
    q["opt_index"][new] = p["opt_index"]
    q["obs_frame"] = new[p["obs_frame"]]
    return q, new


def sba_head(p, m):
    """Structure only: the first m landmarks of the window, every pose fixed at its true value (the landmarks start
    from their perturbed positions, so the solve still has pixels to remove)."""
    q = dict(p)
    n_o = int(p["obs_ptr"][m])
    q["obs_ptr"] = p["obs_ptr"][: m + 1].copy()
    for name in ("obs_frame", "obs_right", "obs_px"):
        q[name] = p[name][:n_o].copy()
    q["X"] = p["X"][:m].copy()
    q["X_true"] = p["X_true"][:m].copy()
    q["T_jw"] = p["T_jw_true"].copy()
    q["opt_index"] = np.full_like(p["opt_index"], -1)
    return q


def sba_repeat_observation(p, n_left):
    """The first landmark with a left observation in an optimised keyframe gets that observation repeated until it has
    n_left of them."""
    ptr = p["obs_ptr"]
    slot = (p["opt_index"][p["obs_frame"]] >= 0) & (p["obs_right"] == 0)
    o = int(np.flatnonzero(slot)[0])
    i = int(np.searchsorted(ptr, o, side="right") - 1)
    have = int(slot[ptr[i]:ptr[i + 1]].sum())
    rep = np.concatenate([np.arange(ptr[i + 1]), np.full(n_left - have, o), np.arange(ptr[i + 1], ptr[-1])]).astype(np.int64)
    q = dict(p)
    for name in ("obs_frame", "obs_right", "obs_px"):
        q[name] = p[name][rep].copy()
    q["obs_ptr"] = p["obs_ptr"].copy()
    q["obs_ptr"][i + 1:] += n_left - have
    return q


def sba_ulp_perturbed(p, seed):
    """obs_px and X moved by one unit in the last place, up or down at random."""
    rng = np.random.default_rng(seed)
    q = dict(p)
    for name in ("obs_px", "X"):
        a = p[name]
        q[name] = np.where(rng.random(a.shape) < 0.5, np.nextafter(a, np.inf), np.nextafter(a, -np.inf))
    return q
