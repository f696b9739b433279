"""The pose covariance on the device: the operators vo_gn_pose_information_stereo / _mono against the float64
restatement (tests/pose_covariance_restatement.py), the inverse against the device's own H, determinism, the invalid cases, and
the one check that the matrix means what it claims: the statistical consistency of e^T Sigma^-1 e over 200 trials."""
import numpy as np
import pytest

import pose_covariance_restatement as PR

pytestmark = pytest.mark.gpu

SIZES = [3, 6, 63, 64, 65, 512, 513, 3000]
EPS = 2.0 ** -53


def _case(n, seed=7, rotated=False):
    rng = np.random.default_rng(seed)
    kw = {}
    if rotated:  # unequal cameras and a rotated rig, as tests/test_stereo_vo_gpu.py's unequal-camera cases use
        T_lr = (PR.stereo_T_lr().astype(np.float64) @ PR.se3_exp([0, 0, 0, 0.004, -0.006, 0.003])).astype(np.float32)
        kw = dict(T_lr=T_lr, Kr=np.array([700.0, 705.0, 600.0, 180.0], np.float32))
    d = PR.two_view(n, rng, 0.3, outlier_frac=0.10, outlier_px=20.0, **kw)
    # the pose the information is taken at: near the true one, as a BA would leave it
    d["T01"] = PR.inv_se3(PR.se3_exp(PR.XI_TRUE + [1e-3, -1e-3, 2e-3, 1e-4, -2e-4, 1e-4])).astype(np.float32)
    return d


def _device(vo, ctx, d, stereo, sigma_px=0.0):
    me = vo.MotionEstimator(ctx, True, d["T_lr"])
    if stereo:
        return me.poseInformation_Stereo(d["X"], d["pts_l"], d["pts_r"], d["Kl"], d["Kr"], d["T_lr"], d["T01"], sigma_px)
    return me.poseInformation(d["X"], d["pts_l"], d["Kl"], d["T01"][:3, :3], d["T01"][:3, 3], sigma_px)


def _host(d, stereo, sigma_px=0.0):
    return PR.information(d["X"], d["pts_l"], d["pts_r"] if stereo else None, d["Kl"], d["Kr"], d["T_lr"], d["T01"], sigma_px)


def _check(g, o, n, stereo):
    H, Hn = g.H, o["H"]
    sc = np.sqrt(np.outer(np.diag(Hn), np.diag(Hn)))
    dH = np.abs(H - Hn) / sc
    print(f"n={n} {'stereo' if stereo else 'mono'}: max |dH|/sqrt(HiiHjj) = {dH.max():.3e}, valid = {g.valid}/{o['valid']}")
    assert dH.max() <= 1e-10
    assert np.array_equal(H, H.T)
    assert g.valid == o["valid"]
    if not o["valid"]:
        assert g.s2 == 0.0 and not g.Sigma.any()
        return
    print(f"   s2 = {g.s2:.12g}, relative difference {abs(g.s2 - o['s2']) / o['s2']:.3e}")
    assert abs(g.s2 - o["s2"]) <= 1e-9 * o["s2"]
    # the inverse against the device's own H
    S = 1.0 / np.sqrt(np.diag(H))
    A = H * S[:, None] * S[None, :]
    B = g.Sigma / S[:, None] / S[None, :] / g.s2
    res = np.abs(A @ B - np.eye(6)).max()
    bound = 6 * 64 * EPS * np.linalg.cond(A, 2)
    print(f"   |(SHS)(S^-1 Sigma S^-1)/s2 - I|max = {res:.3e}, bound {bound:.3e}")
    assert res <= bound
    assert np.array_equal(g.Sigma, g.Sigma.T)


@pytest.mark.parametrize("stereo", [True, False], ids=["stereo", "mono"])
@pytest.mark.parametrize("n", SIZES)
def test_information_matches_the_restatement(vo, ctx, n, stereo):
    d = _case(n)
    if n >= 63:  # both Huber branches and points beyond the gate (3 px) are in it
        a = _host(d, stereo)["a"]
        assert (a < 0.5).any() and (a >= 0.5).any() and (a >= 3.0).any()
    _check(_device(vo, ctx, d, stereo), _host(d, stereo), n, stereo)


def test_information_rotated_rig_unequal_cameras(vo, ctx):
    d = _case(513, seed=11, rotated=True)
    o = _host(d, True)
    assert o["valid"]
    _check(_device(vo, ctx, d, True), o, 513, True)


@pytest.mark.parametrize("stereo", [True, False], ids=["stereo", "mono"])
def test_two_calls_give_identical_bits_and_sigma_px_only_rescales(vo, ctx, stereo):
    d = _case(3000, seed=3)
    a, b = _device(vo, ctx, d, stereo), _device(vo, ctx, d, stereo)
    assert a.valid and b.valid
    for x, y in ((a.H, b.H), (a.Sigma, b.Sigma), (np.float64(a.s2), np.float64(b.s2))):
        assert np.array_equal(np.asarray(x).view(np.uint64), np.asarray(y).view(np.uint64))
    sig = 0.7
    c = _device(vo, ctx, d, stereo, sigma_px=sig)
    assert c.valid and np.array_equal(c.H.view(np.uint64), a.H.view(np.uint64)) and c.s2 == a.s2
    want = (sig * sig / a.s2) * a.Sigma
    ulp = np.abs(c.Sigma - want) / np.spacing(np.abs(want))
    print("sigma_px form against sigma_px^2 / s2 times the a-posteriori form: max", ulp.max(), "ulp")
    assert ulp.max() <= 4


@pytest.mark.parametrize("stereo", [True, False], ids=["stereo", "mono"])
def test_invalid_cases(vo, ctx, stereo):
    """Every input is a legal array; none of these is a fault."""
    base = _case(64, seed=5)

    def cut(d, n):
        e = dict(d)
        for k in ("X", "pts_l", "pts_r"):
            e[k] = d[k][:n]
        return e

    for n in (0, 1, 2):
        g = _device(vo, ctx, cut(base, n), stereo)
        assert not g.valid and g.s2 == 0.0 and not g.Sigma.any(), n
    same = dict(base)
    for k in ("X", "pts_l", "pts_r"):
        same[k] = np.repeat(base[k][:1], 64, axis=0)  # all points identical: a singular H
    g = _device(vo, ctx, same, stereo)
    assert not g.valid and not g.Sigma.any() and np.isfinite(g.H).all()
    nan = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in base.items()}
    nan["pts_l"][17, 1] = np.nan
    g = _device(vo, ctx, nan, stereo)
    assert not g.valid and not g.Sigma.any() and g.s2 == 0.0
    g = _device(vo, ctx, base, stereo)  # (and the context is as good as before)
    assert g.valid


def _consistency(vo, ctx, stereo, sigma, trials=200, n=200):
    """mean of e^T Sigma^-1 e, e = log(T10_true T10_est^-1), the fraction of Huber-active points, whether every mask is all true"""
    rng = np.random.default_rng(1)
    me = vo.MotionEstimator(ctx, True, PR.stereo_T_lr())
    stat, n_act, all_in = [], 0, True
    for _ in range(trials):
        d = PR.two_view(n, rng, sigma)
        if stereo:
            ok, T01, mask, _ = me.poseOnlyBundleAdjustment_Stereo(d["X"], d["pts_l"], d["pts_r"], d["Kl"], d["Kr"], d["T_lr"], 3.0,
                                                                  np.eye(4, dtype=np.float32))
            g = me.poseInformation_Stereo(d["X"], d["pts_l"], d["pts_r"], d["Kl"], d["Kr"], d["T_lr"], T01)
            pr = d["pts_r"]
        else:
            ok, R01, t01, mask, _ = me.poseOnlyBundleAdjustment(d["X"], d["pts_l"], d["Kl"], 3, np.eye(3, dtype=np.float32),
                                                                np.zeros(3, np.float32))
            T01 = np.eye(4, dtype=np.float32)
            T01[:3, :3], T01[:3, 3] = R01, t01
            g = me.poseInformation(d["X"], d["pts_l"], d["Kl"], R01, t01)
            pr = None
        assert ok and g.valid
        all_in = all_in and bool(mask.all())
        T10 = PR.inv_se3(T01.astype(np.float64))
        r, _ = PR.rows(d["X"], d["pts_l"], pr, d["Kl"], d["Kr"], d["T_lr"], T10)
        n_act += int((PR.huber_weight(r)[1] >= 0.5).sum())
        e = PR.se3_log(d["T10_true"] @ PR.inv_se3(T10))
        stat.append(float(e @ np.linalg.solve(g.Sigma, e)))
    return float(np.mean(stat)), n_act / (trials * n), all_in


@pytest.mark.parametrize("stereo", [True, False], ids=["stereo", "mono"])
def test_statistical_consistency(vo, ctx, stereo, record_property):
    """200 trials (numpy.random.default_rng(1)), n = 200, the configs[0] geometry, Gaussian pixel noise 0.1 px, no outliers; the
    pose from the library's own pose-only BA started at the identity, then the operator. e^T Sigma^-1 e is chi^2(6): its mean
    over 200 trials has standard deviation sqrt(12 / 200) = 0.245, and the band [5, 7] is +-4 of them. Conditions on the inputs
    first: every inlier mask all true, Huber-active points (a >= 0.5 at the estimated pose) at most 0.2 % — the estimator is
    least squares there. At 0.3 px (Huber active for about 40 % of the points) the statistic is recorded, not asserted."""
    mean, frac, all_in = _consistency(vo, ctx, stereo, 0.1)
    print(f"{'stereo' if stereo else 'mono'} sigma 0.1 px: mean e^T Sigma^-1 e = {mean:.3f}, Huber-active {100 * frac:.3f} %, masks all true: {all_in}")
    record_property("chi2_mean_0p1", mean)
    assert all_in
    assert frac <= 0.002
    assert 5.0 <= mean <= 7.0
    mean3, frac3, _ = _consistency(vo, ctx, stereo, 0.3)
    print(f"{'stereo' if stereo else 'mono'} sigma 0.3 px (recorded only): mean = {mean3:.3f}, Huber-active {100 * frac3:.1f} %")
    record_property("chi2_mean_0p3", mean3)
