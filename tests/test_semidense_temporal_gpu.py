"""The temporal semi-dense search and fusion on the device (include/vo_hip.h, "Semi-dense temporal") against the
numpy restatement (tests/semidense_temporal_restatement.py), everything bit for bit: the operator, the seeding and the points list
on shapes of the emulation test, and StereoVO's option — the odometry unchanged by it, the map at every keyframe change and at the
end the restatement applied to the images and the returned poses of exactly the frames since the keyframe — through the look-ahead
calls, the synchronous call and runSequence."""
import ctypes as C

import numpy as np
import pytest

import semidense_restatement as SR
import semidense_temporal_restatement as TR
from test_semidense_temporal_emu import case_inputs, same_planes, synthetic_frames
from util import DeviceBuffer

pytestmark = pytest.mark.gpu

K = (370.72, 370.72, 319.5, 119.5)
PLANES = (("invd", np.float32), ("sigma", np.float32), ("n_obs", np.uint8), ("tstatus", np.uint8), ("score", np.float32))


@pytest.fixture(scope="module")
def frames():
    return synthetic_frames()


@pytest.fixture(scope="module")
def sdt_ctx(vo):
    c = vo.Context(device=0, max_width=203, max_height=61, max_points=256, n_slots=2, max_level=0)
    yield c
    c.close()


def _download(buf, dtype, shape):
    out = np.zeros(shape, dtype)
    assert buf.hip.hipMemcpy(out.ctypes.data_as(C.c_void_p), buf.ptr, C.c_size_t(out.nbytes), 2) == 0  # D2H
    return out


# ---- 1. the operator, the seeding and the points list ------------------------------------------------------------------------------
# seeded prior (forward motion, the epipole inside; sideways motion), no prior, a mask, and the identity pose
OP_CASES = ("203x61_forward_epipole", "97x45_sideways", "no_prior_max48", "mask", "identity")


@pytest.mark.parametrize("name", OP_CASES)
def test_operator_equals_restatement(vo, sdt_ctx, frames, name):
    """the map in host memory and in device memory (the key plane with it); the points with and without T; a capacity below the count"""
    ctx = sdt_ctx
    key, cur, Kc, T, m, mask, prm, _ = case_inputs(frames, "203x61_forward_epipole" if name == "identity" else name)
    if name == "identity":
        T = np.eye(4, dtype=np.float32)
    h, w = key.shape
    want = TR.temporal(key, cur, Kc, T, m, mask, **prm)
    ctx.set_image(0, cur)
    ctx.set_slot_mask(0, mask)
    got = ctx.semiDenseTemporal(key, 0, Kc, T, m, **prm)
    ok, where = same_planes(got._asdict(), want)
    assert ok, where
    if name == "identity":
        assert set(np.unique(want["tstatus"]).tolist()) == {0, 7}
        for k in ("invd", "sigma", "n_obs"):
            assert np.array_equal(getattr(got, k), m[k])
    padded = np.full((h, w + 5), 0xEE, np.uint8)  # the key plane on the device, with a padded stride
    padded[:, :w] = key
    bufs = {k: DeviceBuffer(np.ascontiguousarray(m[k]) if k in ("invd", "sigma", "n_obs") else np.full((h, w), 0x5A if dt is np.uint8 else -7, dt))
            for k, dt in PLANES}
    dkey = DeviceBuffer(padded)
    try:
        assert ctx.semiDenseTemporal(dkey.data_ptr(), 0, Kc, T, {k: b.data_ptr() for k, b in bufs.items()}, key_on_device=w + 5,
                                     map_on_device=True, **prm) is None
        dev = {k: _download(bufs[k], dt, (h, w)) for k, dt in PLANES}
        ok, where = same_planes(dev, want)
        assert ok, where
        Tm = np.array([[0.8, 0, 0.6, 1.5], [0, 1, 0, -0.25], [-0.6, 0, 0.8, 7.0], [0, 0, 0, 1]], np.float32)
        for min_obs in (1, 2):
            for Tp in (None, Tm):
                wx, ws, wp = TR.map_points(want["invd"], want["sigma"], want["n_obs"], Kc, Tp, min_obs)
                for on_device in (False, True):
                    if on_device:
                        gx, gs, gp = ctx.semiDenseMapPoints(bufs["invd"].data_ptr(), bufs["sigma"].data_ptr(), bufs["n_obs"].data_ptr(), Kc, Tp,
                                                            min_obs, on_device=(w, h))
                    else:
                        gx, gs, gp = ctx.semiDenseMapPoints(got.invd, got.sigma, got.n_obs, Kc, Tp, min_obs)
                    assert gx.shape == wx.shape and np.array_equal(gx.view(np.uint32), wx.view(np.uint32)), (name, min_obs, on_device)
                    assert np.array_equal(gs.view(np.uint32), ws.view(np.uint32)) and np.array_equal(gp, wp)
        n = int((want["n_obs"] >= 1).sum())
        if n > 3:  # capacity overflow: VO_ERR_CAPACITY, the true count
            with pytest.raises(vo.VoError) as e:
                ctx.semiDenseMapPoints(got.invd, got.sigma, got.n_obs, Kc, capacity=n - 3)
            assert e.value.code == -8 and e.value.n == n
    finally:
        dkey.free()
        for b in bufs.values():
            b.free()


def test_map_seed_equals_restatement(vo, sdt_ctx, frames):
    ctx = sdt_ctx
    key = np.ascontiguousarray(frames["Lk"][90:151, 220:423])
    right = np.ascontiguousarray(frames["Rk"][90:151, 220:423])
    s = SR.semidense(key, right, d_min=0, d_max=60, bf=float(frames["bf"]))
    want = TR.seed(s["disparity"], s["sigma_invd"], s["status"], frames["bf"])
    got = ctx.semiDenseMapSeed(s["disparity"], s["sigma_invd"], s["status"], frames["bf"])
    for k in ("invd", "sigma", "n_obs", "tstatus"):
        assert np.array_equal(getattr(got, k).view(np.uint8), want[k].view(np.uint8)), k
    assert (want["n_obs"] == 1).sum() > 500
    h, w = key.shape
    src = [DeviceBuffer(np.ascontiguousarray(s[k])) for k in ("disparity", "sigma_invd", "status")]
    out = {k: DeviceBuffer(np.full((h, w), 0x5A, np.uint8) if dt is np.uint8 else np.full((h, w), -7.0, np.float32)) for k, dt in PLANES[:4]}
    try:
        assert ctx.semiDenseMapSeed(*(b.data_ptr() for b in src), frames["bf"], out={k: b.data_ptr() for k, b in out.items()}, on_device=(w, h)) is None
        for k, dt in PLANES[:4]:
            assert np.array_equal(_download(out[k], dt, (h, w)).view(np.uint8), want[k].view(np.uint8)), k
    finally:
        for b in src + list(out.values()):
            b.free()


def test_operator_argument_errors(vo, sdt_ctx, frames):
    ctx = sdt_ctx
    key, cur, Kc, T, m, mask, prm, _ = case_inputs(frames, "97x45_sideways")
    ctx.set_image(0, cur)
    ctx.set_slot_mask(0, None)
    for bad in (dict(hw=0), dict(hw=16), dict(hh=4), dict(hh=-1), dict(g_min=0), dict(edge_px=-1), dict(peak_px=-1), dict(max_search=513),
                dict(max_search=6), dict(z_min=0.0), dict(z_min=5.0, z_max=4.0), dict(z_max=float("inf")), dict(j_min=0.0),
                dict(thres_best=float("nan")), dict(eps_epi=-1.0), dict(eps_scale=float("nan")), dict(peak_px=2 ** 31 - 1), dict(peak_px=513),
                dict(edge_px=2 ** 30)):
        with pytest.raises(vo.VoError) as e:
            ctx.semiDenseTemporal(key, 0, Kc, T, m, **dict(prm, **bad))
        assert e.value.code == -1, bad
    with pytest.raises(vo.VoError):
        ctx.semiDenseTemporal(key, 5, Kc, T, m, **prm)
    bad_T = T.copy()
    bad_T[0, 3] = np.nan
    with pytest.raises(vo.VoError):
        ctx.semiDenseTemporal(key, 0, Kc, bad_T, m, **prm)
    with pytest.raises(ValueError):
        ctx.semiDenseTemporal(key, 0, Kc, T, {k: v[:, :50] for k, v in m.items()}, **prm)  # (another size)
    n = C.c_int()
    a = np.zeros((45, 97), np.float32)
    b = np.zeros((45, 97), np.uint8)
    Ka = np.array(Kc, np.float32)
    for min_obs in (0, 256):
        assert ctx.lib.vo_semidense_map_points(ctx.handle, a.ctypes.data, a.ctypes.data, b.ctypes.data, 97, 45, 0, Ka.ctypes.data, None, min_obs, 0,
                                               None, None, None, C.byref(n)) == -1
    assert ctx.lib.vo_semidense_map_points(ctx.handle, a.ctypes.data, a.ctypes.data, b.ctypes.data, 500, 45, 0, Ka.ctypes.data, None, 1, 0, None,
                                           None, None, C.byref(n)) == -4
    assert ctx.lib.vo_semidense_map_seed(ctx.handle, a.ctypes.data, a.ctypes.data, b.ctypes.data, 97, 45, C.c_float(0.0), a.ctypes.data,
                                         a.ctypes.data, b.ctypes.data, b.ctypes.data, 0) == -1


# ---- 2. the driver --------------------------------------------------------------------------------------------------------------
SW, SH = 640, 240
N_FRAMES = 10
TPRM = dict(z_max=80.0, max_search=96)


@pytest.fixture(scope="module")
def stream():
    from visual_odometry_ros_amd import synthetic as S
    st = S.StereoStream(width=SW, height=SH, K=K, n_u=20, n_v=8, seed=2, speed=0.5)
    imgs = [st.render_pair(p)[:2] for p in st.poses(N_FRAMES)]
    bf = float(np.float32(K[0] * st.baseline))
    return st, imgs, dict(bf=bf, d_min=0, d_max=67)


def _driver(vo, st, semidense_arg=None):
    c = vo.Context(device=0, max_width=SW, max_height=SH, max_points=4096, n_slots=5, max_level=4)
    svo = vo.StereoVO(c, SW, SH, K, K, st.T_lr, 20, 8, thres_fastscore=15, window_size=21, max_level=4, strict_border=4, local_ba=True,
                      thres_trans=1.2, thres_alive_ratio=0.6, semidense=semidense_arg)
    return c, svo


def _run(vo, stream, mode, semidense_arg, check=None, n=N_FRAMES):
    """infos (bytes) per frame and the final track set; check(k, svo) after every frame (runSequence: after the last)"""
    st, imgs, _ = stream
    c, svo = _driver(vo, st, semidense_arg)
    try:
        if mode == "sequence":
            got, _ = svo.runSequence([(L, R) for L, R in imgs[:n]])
            infos = [bytes(i) for i in got]
            if check:
                check(n - 1, svo)
        else:
            infos = []
            for k in range(n):
                if mode == "lookahead":
                    svo.enqueue(*imgs[k])
                    if k + 1 < n:
                        svo.prefetch(*imgs[k + 1])
                    gi = svo.result()
                else:
                    gi = svo.trackStereoImages(*imgs[k])
                infos.append(bytes(gi))
                if check:
                    check(k, svo)
        g = svo.getTracks()
        return infos, {k: v.tobytes() for k, v in g.items()}
    finally:
        svo.close()
        c.close()


@pytest.fixture(scope="module")
def plain_runs(vo, stream):
    """the odometry with both options off, per calling mode (computed once)"""
    return {mode: _run(vo, stream, mode, None) for mode in ("lookahead", "sync", "sequence")}


@pytest.fixture(scope="module")
def restated(stream):
    """the map of keyframe kf after the frames kf + 1 .. k under the poses the driver returned, computed when first asked for and kept
    (the three calling modes return the same poses: their bits are compared with one plain run each)"""
    _, imgs, prm = stream
    cache = {}

    def get(kf, k, T_wc):
        key = (kf, k, T_wc[kf].tobytes(), T_wc[k].tobytes())
        if key not in cache:
            if k == kf:
                s = SR.semidense(imgs[kf][0], imgs[kf][1], **prm)
                cache[key] = TR.seed(s["disparity"], s["sigma_invd"], s["status"], np.float32(prm["bf"]))
            else:
                m = get(kf, k - 1, T_wc)
                out = TR.temporal(imgs[kf][0], imgs[k][0], K, TR.pose_ck(T_wc[k], T_wc[kf]), m, **TPRM)
                cache[key] = {p: out[p] for p in ("invd", "sigma", "n_obs", "tstatus")}
        return cache[key]
    return get


@pytest.mark.parametrize("mode", ["lookahead", "sync", "sequence"])
def test_driver_map(vo, stream, restated, plain_runs, mode):
    _, _, prm = stream
    plain_infos = [vo._capi.SvoFrameInfo.from_buffer_copy(b) for b in plain_runs[mode][0]]
    T_wc = [np.array(i.T_wc, np.float32).reshape(4, 4) for i in plain_infos]
    seen = {"looked": [], "fused": 0}

    def check(k, svo):
        last = k == N_FRAMES - 1
        if not last and not plain_infos[k + 1].is_keyframe:
            return
        r = svo.getSemiDenseMap()
        kfs = [j for j in range(k + 1) if plain_infos[j].is_keyframe]
        if not kfs:
            assert r is None, k
            return
        kf = kfs[-1]
        assert r is not None and r.frame_id == plain_infos[kf].frame_id and r.n_fused == k - kf, (k, kf, r.frame_id, r.n_fused)
        assert np.array_equal(r.T_wc.view(np.uint32), T_wc[kf].view(np.uint32)), k
        want = restated(kf, k, T_wc)
        for p in ("tstatus", "n_obs", "invd", "sigma"):
            a, b = getattr(r, p), want[p]
            assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), (k, kf, p, int((a != b).sum()))
        for world in (True, False):
            wx, ws, wp = TR.map_points(want["invd"], want["sigma"], want["n_obs"], K, T_wc[kf] if world else None, 2)
            pts = svo.getSemiDensePoints(world=world, fused=True, min_obs=2)
            assert pts["frame_id"] == r.frame_id and np.array_equal(pts["xyz"].view(np.uint32), wx.view(np.uint32)), (k, world)
            assert np.array_equal(pts["sigma_invd"].view(np.uint32), ws.view(np.uint32)) and np.array_equal(pts["pixel"], wp)
        seen["looked"].append(kf)
        seen["fused"] += int((want["n_obs"] >= 2).sum())

    infos, tracks = _run(vo, stream, mode, dict(prm, every="keyframe", temporal=dict(TPRM)), check)
    assert infos == plain_runs[mode][0] and tracks == plain_runs[mode][1]
    assert seen["looked"] and seen["fused"] > 1000
    if mode != "sequence":
        assert len(set(seen["looked"])) >= 2, seen


def test_driver_getters_errors_and_allocations(vo, stream):
    st, imgs, prm = stream
    c, svo = _driver(vo, st)

    def count(ctx_):
        n = C.c_longlong()
        ctx_.check(ctx_.lib.vo_debug_allocation_count(ctx_.handle, C.byref(n)))
        return n.value
    try:
        with pytest.raises(vo.VoError) as e:  # needs the static option
            svo.setSemiDenseTemporal({})
        assert e.value.code == -1
        svo.setSemiDense(dict(prm))
        with pytest.raises(vo.VoError):  # the option is off
            svo.getSemiDenseMap()
        with pytest.raises(vo.VoError):
            svo.getSemiDensePoints(fused=True)
        with pytest.raises(vo.VoError):
            svo.setSemiDenseTemporal(dict(max_search=1000))
        with pytest.raises(ValueError):
            svo.setSemiDenseTemporal(dict(bf=1.0))
        svo.setSemiDenseTemporal(dict(TPRM))
        assert svo.getSemiDenseMap() is None and svo.getSemiDensePoints(fused=True) is None  # no keyframe yet
        svo.enqueue(*imgs[0])
        for call in (lambda: svo.setSemiDenseTemporal(None), svo.getSemiDenseMap, lambda: svo.getSemiDensePoints(fused=True)):  # in flight
            with pytest.raises(vo.VoError) as e:
                call()
            assert e.value.code == -1
        svo.result()
        svo.trackStereoImages(*imgs[1])  # (the first keyframe)
        r = svo.getSemiDenseMap()
        assert r is not None and r.n_fused == 0 and (r.n_obs == 1).sum() > 1000
        n0 = count(c)
        svo.setSemiDenseTemporal(dict(TPRM, z_max=60.0))  # (a second enable allocates nothing)
        assert count(c) == n0
        svo.trackStereoImages(*imgs[2])
        r = svo.getSemiDenseMap()
        assert r.n_fused == 1 and (r.n_obs >= 2).sum() > 1000
        with pytest.raises(vo.VoError) as e:
            svo.getSemiDensePoints(fused=True, min_obs=2, capacity=10)
        assert e.value.code == -8 and e.value.n == int((r.n_obs >= 2).sum())
        assert len(svo.getSemiDensePoints(fused=True, min_obs=1)["xyz"]) == int((r.n_obs >= 1).sum())
        with pytest.raises(vo.VoError):
            svo.getSemiDensePoints(fused=True, min_obs=0)
        svo.trackStereoImages(*imgs[3])
        # over these frames and getters the allocation count moved exactly as it does for a driver without the options
        c2, plain = _driver(vo, st)
        try:
            for k in (0, 1):
                plain.trackStereoImages(*imgs[k])
            m0 = count(c2)
            for k in (2, 3):
                plain.trackStereoImages(*imgs[k])
            assert count(c) - n0 == count(c2) - m0
        finally:
            plain.close()
            c2.close()
        svo.setSemiDenseTemporal(None)
        with pytest.raises(vo.VoError):
            svo.getSemiDenseMap()
    finally:
        svo.close()
        c.close()


def test_driver_keeps_the_keyframes_mask(vo, stream):
    """The key pixels are gated by the mask the keyframe's pair carried — copied next to the key plane when the map is seeded —
    whatever setMask has made of the later pairs' mask since: mask A from the start, mask B (then none) after the keyframe."""
    st, imgs, prm = stream
    A = np.ones((SH, SW), np.uint8)  # (small regions: the odometry keeps its keyframe rhythm)
    A[40:200, 150:230] = 0
    A[220:, :] = 0
    B = np.ones((SH, SW), np.uint8)
    B[60:200, 400:480] = 0
    c, svo = _driver(vo, st, dict(prm, every="keyframe", temporal=dict(TPRM)))
    try:
        svo.setMask(A)
        infos = [svo.trackStereoImages(*imgs[k]) for k in (0, 1)]
        assert infos[1].is_keyframe
        T_wk = np.array(infos[1].T_wc, np.float32).reshape(4, 4)
        s0 = SR.semidense(imgs[1][0], imgs[1][1], A, **prm)
        m = TR.seed(s0["disparity"], s0["sigma_invd"], s0["status"], np.float32(prm["bf"]))
        for k, mask in ((2, B), (3, None)):
            svo.setMask(mask)
            gi = svo.trackStereoImages(*imgs[k])
            if gi.is_keyframe:
                break
            out = TR.temporal(imgs[1][0], imgs[k][0], K, TR.pose_ck(np.array(gi.T_wc, np.float32).reshape(4, 4), T_wk), m, A, **TPRM)
            m = {p: out[p] for p in ("invd", "sigma", "n_obs", "tstatus")}
            r = svo.getSemiDenseMap()
            assert r.n_fused == k - 1
            for p in ("tstatus", "n_obs", "invd", "sigma"):
                assert np.array_equal(getattr(r, p).view(np.uint8), m[p].view(np.uint8)), (k, p)
            assert (r.tstatus[A == 0] == 0).all() and (r.tstatus[(A != 0) & (B == 0)] == 1).sum() > 100, k
        assert svo.getSemiDenseMap().n_fused >= 1  # (at least the frame under mask B was compared)
    finally:
        svo.close()
        c.close()
