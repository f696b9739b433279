"""Semi-dense stereo depth on the device (include/vo_hip.h, "Semi-dense stereo") against the numpy restatement
(tests/semidense_restatement.py), everything bit for bit: the operator and the points list on the shapes of the emulation test,
and StereoVO's option — the odometry unchanged by it, every result the restatement of that frame's own pair (no slot was reused
under the launch), through the look-ahead calls, the synchronous call and runSequence."""
import ctypes as C

import numpy as np
import pytest

from semidense_restatement import points, semidense
from test_semidense_emu import CASES, case_inputs, same_planes, synthetic_pair
from util import DeviceBuffer

pytestmark = pytest.mark.gpu

K = (370.72, 370.72, 319.5, 119.5)


@pytest.fixture(scope="module")
def pair():
    return synthetic_pair()


@pytest.fixture(scope="module")
def sd_ctx(vo):
    c = vo.Context(device=0, max_width=203, max_height=37, max_points=256, n_slots=2, max_level=0)
    yield c
    c.close()


def _load(c, left, right, mask):
    c.set_image(0, left)
    c.set_image(1, right)
    c.set_slot_mask(0, mask)


def _download(buf, dtype, shape):
    out = np.zeros(shape, dtype)
    assert buf.hip.hipMemcpy(out.ctypes.data_as(C.c_void_p), buf.ptr, C.c_size_t(out.nbytes), 2) == 0  # D2H
    return out


# ---- 1. the operator and the points list ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(CASES))
def test_operator_equals_restatement(vo, sd_ctx, pair, name):
    """planes to host memory and to device memory; the points with and without T; a capacity below the count"""
    ctx = sd_ctx
    left, right, mask, prm, _ = case_inputs(pair, name)
    h, w = left.shape
    want = semidense(left, right, mask, **prm)
    _load(ctx, left, right, mask)
    got = ctx.semiDenseStereo(0, 1, **prm)
    ok, where = same_planes(got._asdict(), want)
    assert ok, where
    assert got.n_accepted == int((want["status"] == 1).sum())
    # device outputs (the planes are written tightly packed)
    bufs = {k: DeviceBuffer(np.full((h, w), 0x5A, np.uint8) if k == "status" else np.full((h, w), -7.0, np.float32))
            for k in ("disparity", "score", "sigma_invd", "status")}
    try:
        assert ctx.semiDenseStereo(0, 1, out={k: b.data_ptr() for k, b in bufs.items()}, **prm) is None
        dev = {k: _download(b, np.uint8 if k == "status" else np.float32, (h, w)) for k, b in bufs.items()}
        ok, where = same_planes(dev, want)
        assert ok, where
        # a NULL output is left out
        only = ctx.lib.vo_semidense_stereo(ctx.handle, 0, 1, C.byref(vo.api._semidense_params(ctx.lib, prm)), None, None, None,
                                           C.c_void_p(bufs["status"].data_ptr()), 1)
        assert only == 0
        T = np.array([[0.8, 0, 0.6, 1.5], [0, 1, 0, -0.25], [-0.6, 0, 0.8, 7.0], [0, 0, 0, 1]], np.float32)
        for Tm in (None, T):
            wx, ws, wp = points(want["disparity"], want["sigma_invd"], want["status"], K, prm["bf"], Tm)
            for on_device in (False, True):
                if on_device:
                    gx, gs, gp = ctx.semiDensePoints(bufs["disparity"].data_ptr(), bufs["sigma_invd"].data_ptr(), bufs["status"].data_ptr(),
                                                     K, prm["bf"], Tm, on_device=(w, h))
                else:
                    gx, gs, gp = ctx.semiDensePoints(got.disparity, got.sigma_invd, got.status, K, prm["bf"], Tm)
                assert gx.shape == wx.shape and np.array_equal(gx.view(np.uint32), wx.view(np.uint32)), (name, on_device)
                assert np.array_equal(gs.view(np.uint32), ws.view(np.uint32)) and np.array_equal(gp, wp)
        n = len(wx)
        if n > 3:  # capacity overflow: VO_ERR_CAPACITY, the true count, the first entries written
            with pytest.raises(vo.VoError) as e:
                ctx.semiDensePoints(got.disparity, got.sigma_invd, got.status, K, prm["bf"], capacity=n - 3)
            assert e.value.code == -8 and e.value.n == n
    finally:
        for b in bufs.values():
            b.free()


def test_operator_argument_errors(vo, sd_ctx, pair):
    ctx = sd_ctx
    left, right, mask, prm, _ = case_inputs(pair, "97x21")
    _load(ctx, left, right, None)
    for bad in (dict(hw=0), dict(hw=16), dict(hh=4), dict(hh=-1), dict(d_min=5, d_max=4), dict(d_max=1024), dict(d_min=-1), dict(g_min=0),
                dict(edge_px=-1), dict(peak_px=-1), dict(bf=0.0), dict(bf=float("nan")), dict(thres_best=float("nan")), dict(eps_epi=-1.0)):
        with pytest.raises(vo.VoError) as e:
            ctx.semiDenseStereo(0, 1, **dict(prm, **bad))
        assert e.value.code == -1, bad
    with pytest.raises(vo.VoError):
        ctx.semiDenseStereo(0, 5, **prm)
    ctx.set_image(1, np.zeros((21, 96), np.uint8))  # (another size)
    with pytest.raises(vo.VoError) as e:
        ctx.semiDenseStereo(0, 1, **prm)
    assert e.value.code == -4
    p = vo.api._semidense_params(ctx.lib, prm)
    assert ctx.lib.vo_semidense_stereo(ctx.handle, 0, 1, None, None, None, None, None, 0) == -1
    n = C.c_int()
    assert ctx.lib.vo_semidense_points(ctx.handle, None, None, None, 97, 21, 0, None, C.c_float(1.0), None, 0, None, None, None, C.byref(n)) == -1
    assert p.hw == 8


# ---- 2. the driver --------------------------------------------------------------------------------------------------------------
SW, SH = 640, 240
N_FRAMES = 10


@pytest.fixture(scope="module")
def stream():
    from visual_odometry_ros_amd import synthetic as S
    st = S.StereoStream(width=SW, height=SH, K=K, n_u=20, n_v=8, seed=2, speed=0.5)
    imgs = [st.render_pair(p)[:2] for p in st.poses(N_FRAMES)]
    bf = float(np.float32(K[0] * st.baseline))
    return st, imgs, dict(bf=bf, d_min=0, d_max=67)


@pytest.fixture(scope="module")
def restated(stream):
    """the restatement of every frame's own pair, computed when first asked for and kept"""
    _, imgs, prm = stream
    cache = {}

    def get(k):
        if k not in cache:
            cache[k] = semidense(imgs[k][0], imgs[k][1], **prm)
        return cache[k]
    return get


def _driver(vo, st, semidense_arg=None):
    c = vo.Context(device=0, max_width=SW, max_height=SH, max_points=4096, n_slots=5, max_level=4)
    svo = vo.StereoVO(c, SW, SH, K, K, st.T_lr, 20, 8, thres_fastscore=15, window_size=21, max_level=4, strict_border=4, local_ba=True,
                      thres_trans=1.2, thres_alive_ratio=0.6, semidense=semidense_arg)
    return c, svo


def _run(vo, stream, mode, semidense_arg, check=None, n=N_FRAMES):
    """infos (bytes) per frame and the final track set; check(k, info, svo) after every frame"""
    st, imgs, _ = stream
    c, svo = _driver(vo, st, semidense_arg)
    try:
        infos = []
        if mode == "sequence":
            got, _ = svo.runSequence([(L, R) for L, R in imgs[:n]])
            infos = [bytes(i) for i in got]
            if check:
                check(n - 1, got[-1], svo)
        else:
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
                    check(k, gi, svo)
        g = svo.getTracks()
        return infos, {k: v.tobytes() for k, v in g.items()}
    finally:
        svo.close()
        c.close()


@pytest.fixture(scope="module")
def plain_runs(vo, stream):
    """the odometry with the option off, per calling mode (computed once)"""
    return {mode: _run(vo, stream, mode, None) for mode in ("lookahead", "sync", "sequence")}


@pytest.mark.parametrize("mode", ["lookahead", "sync", "sequence"])
def test_driver_keyframes(vo, stream, restated, plain_runs, mode):
    """every = keyframes: the odometry's bits are those of the option off; the planes are the restatement of the last keyframe's
    own pair, frame_id and T_wc that frame's. The result is looked at after every second frame and after the last one — the getters
    wait for the launch, so a look right behind a keyframe would hide a slot reused under it; a look a frame or two later, when the
    next pairs have been ingested, does not. A non-keyframe leaves the previous result in place."""
    _, _, prm = stream
    plain_infos = [vo._capi.SvoFrameInfo.from_buffer_copy(b) for b in plain_runs[mode][0]]
    by_id = {i.frame_id: k for k, i in enumerate(plain_infos)}
    seen = {"looked": [], "late": 0}

    def check(k, gi, svo):
        if mode != "sequence" and not (k % 2 == 1 or k == N_FRAMES - 1):
            return
        r = svo.getSemiDense()
        kfs = [j for j in range(k + 1) if plain_infos[j].is_keyframe]
        if not kfs:
            assert r is None, k
            return
        kf = kfs[-1]
        assert r is not None and by_id[r.frame_id] == kf, (k, kf, r.frame_id)
        assert np.array_equal(r.T_wc.view(np.uint32), np.array(plain_infos[kf].T_wc, np.float32).reshape(4, 4).view(np.uint32)), k
        want = restated(kf)
        ok, where = same_planes(r._asdict(), want)
        assert ok, (k, kf, where)
        assert r.n_accepted == int((want["status"] == 1).sum()) > 1000
        seen["looked"].append(kf)
        seen["late"] += kf < k

    infos, tracks = _run(vo, stream, mode, dict(prm, every="keyframe"), check)
    assert infos == plain_runs[mode][0] and tracks == plain_runs[mode][1]
    assert seen["looked"]
    if mode != "sequence":
        assert len(set(seen["looked"])) >= 2 and seen["late"] >= 1, seen


def test_driver_every_frame_and_points(vo, stream, restated, plain_runs):
    """every = frames, four frames, look-ahead: a result per frame (the first pair included), the points in the world and in the
    camera frame"""
    _, _, prm = stream

    def check(k, gi, svo):
        r = svo.getSemiDense()
        assert r is not None and r.frame_id == gi.frame_id, k
        want = restated(k)
        ok, where = same_planes(r._asdict(), want)
        assert ok, (k, where)
        T = np.array(gi.T_wc, np.float32).reshape(4, 4)
        assert np.array_equal(r.T_wc.view(np.uint32), T.view(np.uint32))
        for world in (True, False):
            wx, ws, wp = points(want["disparity"], want["sigma_invd"], want["status"], K, prm["bf"], T if world else None)
            p = svo.getSemiDensePoints(world=world)
            assert p["frame_id"] == gi.frame_id and np.array_equal(p["xyz"].view(np.uint32), wx.view(np.uint32)), (k, world)
            assert np.array_equal(p["sigma_invd"].view(np.uint32), ws.view(np.uint32)) and np.array_equal(p["pixel"], wp)

    infos, _ = _run(vo, stream, "lookahead", dict(prm, every="frame"), check, n=4)
    assert infos == plain_runs["lookahead"][0][:4]


def test_driver_getters_and_errors(vo, stream):
    st, imgs, prm = stream
    c, svo = _driver(vo, st)
    try:
        with pytest.raises(vo.VoError) as e:  # the option is off
            svo.getSemiDense()
        assert e.value.code == -1
        with pytest.raises(vo.VoError):
            svo.getSemiDensePoints()
        with pytest.raises(ValueError):
            svo.setSemiDense(dict(prm), every="sometimes")
        with pytest.raises(ValueError):
            svo.setSemiDense(dict(d_max=10))  # (no bf)
        with pytest.raises(vo.VoError):
            svo.setSemiDense(dict(prm, hw=99))
        assert c.lib.vo_svo_set_semidense(svo._h, C.byref(vo.api._semidense_params(c.lib, prm)), 7) == -1
        svo.setSemiDense(dict(prm))
        assert svo.getSemiDense() is None and svo.getSemiDensePoints() is None  # no result yet
        svo.enqueue(*imgs[0])
        for call in (lambda: svo.setSemiDense(None), svo.getSemiDense, svo.getSemiDensePoints):  # a frame is in flight
            with pytest.raises(vo.VoError) as e:
                call()
            assert e.value.code == -1
        svo.result()
        svo.trackStereoImages(*imgs[1])  # (the first keyframe)
        r = svo.getSemiDense()
        assert r is not None and r.n_accepted == int((r.status == 1).sum()) > 1000
        with pytest.raises(vo.VoError) as e:
            svo.getSemiDensePoints(capacity=10)
        assert e.value.code == -8 and e.value.n == r.n_accepted
        assert len(svo.getSemiDensePoints()["xyz"]) == r.n_accepted
        # the option's only allocations were made by setSemiDense: over later frames, results and getters the context's allocation
        # count moves exactly as it does for a driver without the option
        def count(ctx_):
            n = C.c_longlong()
            ctx_.check(ctx_.lib.vo_debug_allocation_count(ctx_.handle, C.byref(n)))
            return n.value
        n0 = count(c)
        svo.setSemiDense(dict(prm), every="frame")
        for k in (2, 3):
            gi = svo.trackStereoImages(*imgs[k])
            assert svo.getSemiDense().frame_id == gi.frame_id and len(svo.getSemiDensePoints(world=False)["xyz"]) > 1000
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
        svo.setSemiDense(None)
        with pytest.raises(vo.VoError):
            svo.getSemiDense()
    finally:
        svo.close()
        c.close()
