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


# ---- general stereo rig (test_rig_inputs.py, test_rig_gpu.py) ------------------------------------------------------------
# Right intrinsics 1-3 % off the left ones, fx != fy in both cameras, and a right camera that is rotated by ~0.016 rad and
# shifted in y and z as well: no two of K_l / K_r, R_lr / R_lr^T, T_lr / inverse(T_lr), fx / fy can be exchanged, and
# t_y, t_z cannot be dropped, without the result changing (test_rig_inputs.py shows that for every input built from these).
# Small enough that left -> right tracking still finds its features.
RIG_XI = (0.537, 0.011, -0.007, 0.012, -0.009, 0.004)
RIG_KITTI = dict(K_l=(718.856, 726.1, 607.1928, 185.2157), K_r=(709.4, 704.3, 615.9, 180.4))  # two-view point sets, BA windows
RIG_320 = dict(width=320, height=200, K_l=(300.0, 303.5, 160.0, 100.0), K_r=(296.0, 294.5, 166.0, 96.5))
RIG_640 = dict(width=640, height=240, K_l=(400.0, 404.0, 320.0, 120.0), K_r=(395.0, 392.5, 327.0, 116.0))
RIG_MUTANTS = ("K_l <-> K_r", "R_lr transposed", "T_lr inverted", "t_y = t_z = 0", "fx <-> fy right")
RIG_PLAIN_NOOPS = ("K_l <-> K_r", "R_lr transposed", "t_y = t_z = 0")  # what leaves K_r = K_l, R = I, t = (b, 0, 0) as it is
# pose-only BA point counts: one point, less than a wavefront's worth, around one workgroup (512), around the 2048 points
# gn_pose_kernel keeps in registers (the rest is reloaded each iteration), and well past it
RIG_GN_COUNTS = (1, 37, 511, 512, 513, 2047, 2048, 2049, 3000)
RIG_GN_SEED = {n: 100 + n for n in RIG_GN_COUNTS}  # seeds at which the TREE and SEQ inlier masks are equal (test_rig_inputs.py)
MONO_K = (458.654, 457.296, 367.215, 248.375)  # fx != fy
MONO_GN_COUNTS = (2047, 2048, 2049, 3000)     # around and past the points kept in registers: the mono reload loop
MONO_GN_SEED = {n: 200 + n for n in MONO_GN_COUNTS}
RIG_GN_T0_XI = (0.02, -0.015, 0.017, 0.003, -0.002, 0.0017)  # |v| = 0.030 m, |w| = 0.004 rad off the truth


def rig_T_lr():
    """float64 pose of the right camera in the left one's frame."""
    from visual_odometry_ros_amd import synthetic as S
    return S.se3_exp(RIG_XI)


def plain_T_lr(baseline=None):
    """float64 T_lr of the plain rig: its float32 cast is synthetic.stereo_T_lr(baseline)."""
    from visual_odometry_ros_amd import synthetic as S
    T = np.eye(4)
    T[0, 3] = S.KITTI_BASELINE if baseline is None else baseline
    return T


def se3_inverse64(T):
    T = np.asarray(T, np.float64)
    Ti = np.eye(4)
    Ti[:3, :3] = T[:3, :3].T
    Ti[:3, 3] = -(T[:3, :3].T @ T[:3, 3])
    return Ti


def project64(X, T, K):
    """Pixels of the points X (n x 3, float64) in the camera K = (fx, fy, cx, cy) whose frame T maps them to."""
    Xc = X @ T[:3, :3].T + T[:3, 3]
    fx, fy, cx, cy = K
    return np.stack([fx * Xc[:, 0] / Xc[:, 2] + cx, fy * Xc[:, 1] / Xc[:, 2] + cy], 1)


def rig_mutants(K_l, K_r, T_lr):
    """The rig as a kernel would see it after each of the mistakes of RIG_MUTANTS: name -> (K_l, K_r, T_lr)."""
    K_l, K_r, T = tuple(K_l), tuple(K_r), np.asarray(T_lr, np.float64)
    R_t, t_x = T.copy(), T.copy()
    R_t[:3, :3] = T[:3, :3].T
    t_x[1:3, 3] = 0.0
    rigs = ((K_r, K_l, T), (K_l, K_r, R_t), (K_l, K_r, se3_inverse64(T)), (K_l, K_r, t_x),
            (K_l, (K_r[1], K_r[0], K_r[2], K_r[3]), T))
    return dict(zip(RIG_MUTANTS, rigs))


def rig_two_view(n=500, seed=1, K_l=None, K_r=None, T_lr=None, noise_px=0.3, outlier_frac=0.10,
                 xi_true=(0.05, -0.02, 0.8, 0.004, -0.01, 0.002)):
    """synthetic.two_view_points for a rig of two different cameras: the same draws in the same order, the right pixels
    projected in float64 through inverse(T_lr) and K_r. Defaults: RIG_KITTI and rig_T_lr(). Returns K (left), Kr and the
    float32 T_lr the operators take."""
    from visual_odometry_ros_amd import synthetic as S
    K_l = RIG_KITTI["K_l"] if K_l is None else K_l
    K_r = RIG_KITTI["K_r"] if K_r is None else K_r
    T_lr = rig_T_lr() if T_lr is None else np.asarray(T_lr, np.float64)
    rng = np.random.default_rng(seed)
    X = np.stack([rng.uniform(-10, 10, n), rng.uniform(-4, 4, n), rng.uniform(4, 40, n)], 1)
    T01 = S.se3_exp(xi_true)
    T10 = np.linalg.inv(T01)
    X1 = X @ T10[:3, :3].T + T10[:3, 3]
    pl = project64(X1, np.eye(4), K_l)
    pr = project64(X1, se3_inverse64(T_lr), K_r)
    pl += rng.normal(0, noise_px, pl.shape)
    pr += rng.normal(0, noise_px, pr.shape)
    n_out = int(round(outlier_frac * n))
    out_idx = rng.choice(n, n_out, replace=False)
    pl[out_idx] += rng.uniform(-20, 20, (n_out, 2))
    pr[out_idx] += rng.uniform(-20, 20, (n_out, 2))
    is_outlier = np.zeros(n, bool)
    is_outlier[out_idx] = True
    return dict(X=X.astype(np.float32), pts_l=pl.astype(np.float32), pts_r=pr.astype(np.float32), T01_true=T01,
                K=np.asarray(K_l, np.float32), Kr=np.asarray(K_r, np.float32), T_lr=T_lr.astype(np.float32),
                is_outlier=is_outlier)


def rig_gn_T0(d, identity):
    """The initial pose of a pose-only BA test: the identity, or the truth moved by RIG_GN_T0_XI, rounded to float32 (a
    rotation that is orthonormal to float32 rounding only)."""
    from visual_odometry_ros_amd import synthetic as S
    if identity:
        return np.eye(4, dtype=np.float32)
    return (d["T01_true"] @ S.se3_exp(RIG_GN_T0_XI)).astype(np.float32)


class RigStream:
    """synthetic.StereoStream with two different cameras (a wrapper: scene, poses and every attribute it does not define
    are the wrapped stream's). The left image is rendered with K_l (.K), the right one with K_r (.Kr) at T_wc @ T_lr; the
    track set's right pixels are the float64 projection of the cast points through inverse(T_lr) and K_r. T_lr is given in
    float64; .T_lr is its float32 cast, which is what the operators take and (as in StereoStream) what the right image is
    rendered at. Every other array of the track set is StereoStream's."""

    def __init__(self, K_l, K_r, T_lr, **kw):
        from visual_odometry_ros_amd import synthetic as S
        self._T_lr64 = np.asarray(T_lr, np.float64)
        self._plain = S.StereoStream(K=K_l, baseline=float(self._T_lr64[0, 3]), **kw)
        self.Kr = K_r
        self.T_lr = self._T_lr64.astype(np.float32)

    def __getattr__(self, name):
        return getattr(self._plain, name)

    def render_pair(self, T_wc):
        L, depth = self.scene.render(T_wc, self.K, self.width, self.height)
        R, _ = self.scene.render(T_wc @ self.T_lr.astype(np.float64), self.Kr, self.width, self.height)
        return L, R, depth

    def track_set(self, k, T_wc_prev, T_wc_cur):
        from visual_odometry_ros_amd import synthetic as S
        ts = self._plain.track_set(k, T_wc_prev, T_wc_cur)
        rng = np.random.default_rng(self.seed * 7919 + k)  # the left pixels again, before their cast to float32
        pts = S.bucket_points(self.width, self.height, self.n_u, self.n_v, rng, self.margin)
        fx, fy, cx, cy = self.K
        z, _, _ = self.scene.cast(T_wc_prev, self.K, self.width, self.height, pix=pts)
        X = np.stack([(pts[:, 0] - cx) / fx * z, (pts[:, 1] - cy) / fy * z, z], 1)
        ts["pts_r0"] = project64(X, se3_inverse64(self._T_lr64), self.Kr).astype(np.float32)
        return ts


def rig_stream(rig, T_lr=None, **kw):
    """RigStream of one of the named rigs (RIG_320, RIG_640)."""
    return RigStream(rig["K_l"], rig["K_r"], rig_T_lr() if T_lr is None else T_lr, width=rig["width"], height=rig["height"], **kw)


def rig_ba_window(**kw):
    """synthetic.ba_window on RIG_KITTI with rig_T_lr(): right observations projected with K_r."""
    from visual_odometry_ros_amd import synthetic as S
    return S.ba_window(K=RIG_KITTI["K_l"], Kr=RIG_KITTI["K_r"], T_lr=rig_T_lr(), **kw)
