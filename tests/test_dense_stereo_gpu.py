"""Dense stereo disparity on the device (include/vo_hip.h, "Dense stereo") against the numpy restatement
(tests/dense_stereo_restatement.py), everything bit for bit: the operator on the shapes of the emulation test; its planes through the
semi-dense chain's operators (points list, map seed, world integration) against their restatements; and StereoVO's option — the
odometry and the semi-dense option unchanged by it, every result the restatement of that frame's own pair (no slot was reused under
the launches), through the look-ahead calls, the synchronous call and runSequence. (The C call's refusal of a mono driver is not
exercised: no public call yields the vo_svo core of a MonoVO, so only the absence of the method on MonoVO is asserted.)"""
import ctypes as C

import numpy as np
import pytest

import semidense_world_restatement as WR
from dense_stereo_restatement import dense_stereo
from semidense_restatement import points, semidense
from semidense_temporal_restatement import seed
from test_dense_stereo_emu import CASES, case_inputs, restated as restated_case, same_planes
from test_semidense_emu import synthetic_pair
from test_semidense_world import same_records
from util import DeviceBuffer

pytestmark = pytest.mark.gpu

K = (370.72, 370.72, 319.5, 119.5)
PLANES = (("disparity", np.float32), ("cost", np.uint16), ("sigma_invd", np.float32), ("status", np.uint8))


@pytest.fixture(scope="module")
def pair():
    return synthetic_pair()


@pytest.fixture(scope="module")
def ds_ctx(vo):
    c = vo.Context(device=0, max_width=203, max_height=120, max_points=256, n_slots=2, max_level=0)
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


# ---- 1. the operator -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(CASES))
def test_operator_equals_restatement(vo, ds_ctx, pair, name):
    """planes to host memory and to device memory, a NULL output, a second call that reuses the workspace"""
    ctx = ds_ctx
    left, right, mask, prm, _ = case_inputs(pair, name)
    h, w = left.shape
    want = restated_case(pair, name)
    _load(ctx, left, right, mask)
    got = ctx.denseStereo(0, 1, **prm)
    ok, where = same_planes(got._asdict(), want)
    assert ok, where
    assert got.n_accepted == want["n_accepted"]
    bufs = {k: DeviceBuffer(np.full((h, w), 0x5A, np.uint8).astype(dt)) for k, dt in PLANES}
    try:
        assert ctx.denseStereo(0, 1, out={k: b.data_ptr() for k, b in bufs.items()}, **prm) is None  # (the workspace is there already)
        dev = {k: _download(bufs[k], dt, (h, w)) for k, dt in PLANES}
        ok, where = same_planes(dev, want)
        assert ok, where
        # a NULL output is left out: only the status plane is written again
        marker = DeviceBuffer(np.full((h, w), 0x5A, np.uint8))
        try:
            assert ctx.lib.vo_dense_stereo(ctx.handle, 0, 1, C.byref(vo.api._dense_stereo_params(ctx.lib, prm)), None, None, None,
                                           C.c_void_p(marker.data_ptr()), 1) == 0
            assert np.array_equal(_download(marker, np.uint8, (h, w)), want["status"])
        finally:
            marker.free()
    finally:
        for b in bufs.values():
            b.free()


def test_operator_argument_errors(vo, ds_ctx, pair):
    ctx = ds_ctx
    left, right, _, prm, _ = case_inputs(pair, "97x21")
    _load(ctx, left, right, None)
    for bad in (dict(d_min=-1), dict(n_disp=0), dict(n_disp=100), dict(n_disp=320), dict(paths=5), dict(paths=0), dict(p1=-1), dict(p1=64),
                dict(p1=70, p2=64), dict(p2=8130), dict(uniqueness=-1), dict(uniqueness=100), dict(lr_max=-2), dict(eps_d=-0.5),
                dict(eps_d=float("nan")), dict(eps_d=float("inf")), dict(bf=0.0), dict(bf=-1.0), dict(bf=float("nan")), dict(bf=float("inf"))):
        with pytest.raises(vo.VoError) as e:
            ctx.denseStereo(0, 1, **dict(prm, **bad))
        assert e.value.code == -1, bad
    with pytest.raises(ValueError):
        ctx.denseStereo(0, 1, **dict(prm, window=9))
    with pytest.raises(vo.VoError) as e:  # a bad slot
        ctx.denseStereo(0, 5, **prm)
    assert e.value.code == -1
    ctx.set_image(1, np.zeros((21, 96), np.uint8))  # (another size)
    with pytest.raises(vo.VoError) as e:
        ctx.denseStereo(0, 1, **prm)
    assert e.value.code == -4
    assert ctx.lib.vo_dense_stereo(ctx.handle, 0, 1, None, None, None, None, None, 0) == -1
    assert ctx.denseStereoWorkspace(97, 21, **prm) == 97 * 21 * (16 + 2 * 64)
    # z_min gives d_max as the semi-dense option derives it; n_disp is rounded up; d_min follows
    p = vo.api._dense_stereo_params(ctx.lib, dict(bf=386.1, z_min=3.0, n_disp=100))
    assert (p.n_disp, p.d_min) == (128, 2) and vo.semidense_disparity_range(386.1, 3.0)[1] == 129
    p = vo.api._dense_stereo_params(ctx.lib, dict(bf=386.1, z_min=10.0))
    assert (p.n_disp, p.d_min) == (64, 0)


# ---- 2. the planes plug into the semi-dense chain ----------------------------------------------------------------------------------
def test_planes_go_through_points_seed_and_world(vo, ds_ctx, pair):
    ctx = ds_ctx
    name = "203x37_n128"
    left, right, mask, prm, _ = case_inputs(pair, name)
    want = restated_case(pair, name)
    bf = prm["bf"]
    _load(ctx, left, right, mask)
    got = ctx.denseStereo(0, 1, **prm)
    T = np.array([[0.8, 0, 0.6, 1.5], [0, 1, 0, -0.25], [-0.6, 0, 0.8, 7.0], [0, 0, 0, 1]], np.float32)
    for Tm in (None, T):
        wx, ws, wp = points(want["disparity"], want["sigma_invd"], want["status"], K, bf, Tm)
        gx, gs, gp = ctx.semiDensePoints(got.disparity, got.sigma_invd, got.status, K, bf, Tm)
        assert len(wx) == want["n_accepted"] and gx.shape == wx.shape and np.array_equal(gx.view(np.uint32), wx.view(np.uint32))
        assert np.array_equal(gs.view(np.uint32), ws.view(np.uint32)) and np.array_equal(gp, wp)
    m = ctx.semiDenseMapSeed(got.disparity, got.sigma_invd, got.status, bf)
    wm_ = seed(want["disparity"], want["sigma_invd"], want["status"], bf)
    assert np.array_equal(m.invd.view(np.uint32), wm_["invd"].view(np.uint32)) and np.array_equal(m.sigma.view(np.uint32), wm_["sigma"].view(np.uint32))
    assert np.array_equal(m.n_obs, wm_["n_obs"])
    wprm = dict(voxel=0.1, capacity_log2=16, min_obs=1, z_max=40.0)
    world = WR.World(**wprm)
    assert world.integrate(wm_, K, T, left)
    with ctx.semiDenseWorld(**wprm) as wm:
        wm.integrate(m, K, T, key=left)
        ok, where = same_records(wm.points()._asdict(), world.records(), fields=("index", "sums", "count", "keyframes", "weight", "grey", "xyz"))
        assert ok, where
        assert wm.stats() == world.stats
        dense_inserted = wm.stats()["inserted"]
    # the same path from the semi-dense result of the same pair: fewer points reach the table
    sd = ctx.semiDenseStereo(0, 1, bf=bf, d_min=0, d_max=70)
    with ctx.semiDenseWorld(**wprm) as wm:
        wm.integrate(ctx.semiDenseMapSeed(sd.disparity, sd.sigma_invd, sd.status, bf), K, T, key=left)
        sd_inserted = wm.stats()["inserted"]
    assert dense_inserted > sd_inserted > 0, (dense_inserted, sd_inserted)


# ---- 3. the driver -----------------------------------------------------------------------------------------------------------------
SW, SH = 640, 240
N_FRAMES = 10


@pytest.fixture(scope="module")
def stream():
    from visual_odometry_ros_amd import synthetic as S
    st = S.StereoStream(width=SW, height=SH, K=K, n_u=20, n_v=8, seed=2, speed=0.5)
    imgs = [st.render_pair(p)[:2] for p in st.poses(N_FRAMES)]
    bf = float(np.float32(K[0] * st.baseline))
    return st, imgs, dict(bf=bf, d_min=0, n_disp=64)


@pytest.fixture(scope="module")
def restated(stream):
    """the restatement of a frame's own pair, computed when first asked for and kept"""
    _, imgs, prm = stream
    cache = {}

    def get(k):
        if k not in cache:
            r = dense_stereo(imgs[k][0], imgs[k][1], **prm)
            r.pop("S")
            cache[k] = r
        return cache[k]
    return get


def _driver(vo, st, **options):
    c = vo.Context(device=0, max_width=SW, max_height=SH, max_points=4096, n_slots=5, max_level=4)
    svo = vo.StereoVO(c, SW, SH, K, K, st.T_lr, 20, 8, thres_fastscore=15, window_size=21, max_level=4, strict_border=4, local_ba=True,
                      thres_trans=1.2, thres_alive_ratio=0.6, **options)
    return c, svo


def _run(vo, stream, mode, options, check=None, n=N_FRAMES, at_end=None):
    """infos (bytes) per frame and the final track set; check(k, info, svo) after every frame"""
    st, imgs, _ = stream
    c, svo = _driver(vo, st, **options)
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
        extra = at_end(svo) if at_end else None
        return infos, {k: v.tobytes() for k, v in g.items()}, extra
    finally:
        svo.close()
        c.close()


@pytest.fixture(scope="module")
def plain_runs(vo, stream):
    """the odometry with the option off, per calling mode (computed once)"""
    return {mode: _run(vo, stream, mode, {}) for mode in ("lookahead", "sync", "sequence")}


@pytest.mark.parametrize("mode", ["lookahead", "sync", "sequence"])
def test_driver_keyframes(vo, stream, restated, plain_runs, mode):
    """every = keyframes: the odometry's bits are those of the option off; the planes are the restatement of the last keyframe's
    own pair, frame_id and T_wc that frame's. The result is looked at after every second frame and after the last one — the getters
    wait for the launches, so a look right behind a keyframe would hide a slot reused under them; a look a frame or two later, when
    the next pairs have been ingested, does not. A non-keyframe leaves the previous result in place."""
    _, _, prm = stream
    plain_infos = [vo._capi.SvoFrameInfo.from_buffer_copy(b) for b in plain_runs[mode][0]]
    by_id = {i.frame_id: k for k, i in enumerate(plain_infos)}
    seen = {"looked": [], "late": 0}

    def check(k, gi, svo):
        if mode != "sequence" and not (k % 2 == 1 or k == N_FRAMES - 1):
            return
        r = svo.getDenseStereo()
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
        assert r.n_accepted == want["n_accepted"] > 100000
        seen["looked"].append(kf)
        seen["late"] += kf < k

    infos, tracks, _ = _run(vo, stream, mode, dict(dense=dict(prm, every="keyframe")), check)
    assert infos == plain_runs[mode][0] and tracks == plain_runs[mode][1]
    assert seen["looked"]
    if mode != "sequence":
        assert len(set(seen["looked"])) >= 2 and seen["late"] >= 1, seen


def test_driver_every_frame_points_and_semidense_next_to_it(vo, stream, restated, plain_runs):
    """every = frames, three frames, look-ahead, with the semi-dense option on at the same time: a result per frame (the first pair
    included), the points in the world and in the camera frame, the semi-dense result the bits of a run without the dense option"""
    _, _, prm = stream
    sdprm = dict(bf=prm["bf"], d_min=0, d_max=67, every="frame")

    def check(k, gi, svo):
        r = svo.getDenseStereo()
        assert r is not None and r.frame_id == gi.frame_id, k
        want = restated(k)
        ok, where = same_planes(r._asdict(), want)
        assert ok, (k, where)
        T = np.array(gi.T_wc, np.float32).reshape(4, 4)
        assert np.array_equal(r.T_wc.view(np.uint32), T.view(np.uint32))
        if k == 2:
            for world in (True, False):
                wx, ws, wp = points(want["disparity"], want["sigma_invd"], want["status"], K, prm["bf"], T if world else None)
                p = svo.getDensePoints(world=world)
                assert p["frame_id"] == gi.frame_id and np.array_equal(p["xyz"].view(np.uint32), wx.view(np.uint32)), (k, world)
                assert np.array_equal(p["sigma_invd"].view(np.uint32), ws.view(np.uint32)) and np.array_equal(p["pixel"], wp)

    last_sd = lambda svo: {k: np.asarray(v).tobytes() for k, v in svo.getSemiDense()._asdict().items() if v is not None}
    infos, _, both = _run(vo, stream, "lookahead", dict(dense=dict(prm, every="frame"), semidense=sdprm), check, n=3, at_end=last_sd)
    assert infos == plain_runs["lookahead"][0][:3]
    _, _, alone = _run(vo, stream, "lookahead", dict(semidense=sdprm), None, n=3, at_end=last_sd)
    assert both == alone and len(both) >= 6


def test_driver_getters_and_errors(vo, stream):
    st, imgs, prm = stream
    c, svo = _driver(vo, st)
    try:
        with pytest.raises(vo.VoError) as e:  # the option is off
            svo.getDenseStereo()
        assert e.value.code == -1
        with pytest.raises(vo.VoError):
            svo.getDensePoints()
        with pytest.raises(ValueError):
            svo.setDenseStereo(dict(prm), every="sometimes")
        with pytest.raises(ValueError):
            svo.setDenseStereo(dict(n_disp=64))  # (no bf)
        with pytest.raises(vo.VoError):
            svo.setDenseStereo(dict(prm, n_disp=96))
        assert c.lib.vo_svo_set_dense_stereo(svo._h, C.byref(vo.api._dense_stereo_params(c.lib, prm)), 7) == -1
        svo.setDenseStereo(dict(prm))
        assert svo.getDenseStereo() is None and svo.getDensePoints() is None  # no result yet
        svo.enqueue(*imgs[0])
        for call in (lambda: svo.setDenseStereo(None), svo.getDenseStereo, svo.getDensePoints):  # a frame is in flight
            with pytest.raises(vo.VoError) as e:
                call()
            assert e.value.code == -1
        svo.result()
        svo.trackStereoImages(*imgs[1])  # (the first keyframe)
        r = svo.getDenseStereo()
        assert r is not None and r.n_accepted == int((r.status == 1).sum()) > 100000
        with pytest.raises(vo.VoError) as e:
            svo.getDensePoints(capacity=10)
        assert e.value.code == -8 and e.value.n == r.n_accepted
        assert len(svo.getDensePoints()["xyz"]) == r.n_accepted

        # the option's only allocations were made by setDenseStereo: over later frames, results and getters the context's allocation
        # count moves exactly as it does for a driver without the option
        def count(ctx_):
            n = C.c_longlong()
            ctx_.check(ctx_.lib.vo_debug_allocation_count(ctx_.handle, C.byref(n)))
            return n.value
        n0 = count(c)
        svo.setDenseStereo(dict(prm), every="frame")
        for k in (2, 3):
            gi = svo.trackStereoImages(*imgs[k])
            assert svo.getDenseStereo().frame_id == gi.frame_id and len(svo.getDensePoints(world=False)["xyz"]) > 100000
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
        svo.setDenseStereo(None)
        with pytest.raises(vo.VoError):
            svo.getDenseStereo()
        assert not hasattr(vo.MonoVO, "setDenseStereo")  # a stereo driver's option (the C call refuses a mono driver's core)
    finally:
        svo.close()
        c.close()
