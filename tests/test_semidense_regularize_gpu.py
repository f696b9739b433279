"""The regularisation of the semi-dense map on the device (include/vo_hip.h, "Semi-dense regularisation") against the
numpy restatement (tests/semidense_regularize_restatement.py), everything bit for bit: the operator on the emulation test's cases —
host planes, device planes with a padded key stride, the device call twice in a row — its argument errors, the alignment and the
points list on a regularised map, and StereoVO's option through the look-ahead calls, the synchronous call and runSequence: the
odometry and the raw map the same bits as without it, the regularised map at every keyframe, keyframe change and at the end the
restatement applied to the chained raw map (with the propagation on as well); a mask that changes between keyframes; the option
switched off and on; the refusals and its one allocation. None of the entry points exists without the feature."""
import ctypes as C

import numpy as np
import pytest

import semidense_align_restatement as AR
import semidense_regularize_restatement as RR
import semidense_temporal_restatement as TR
from test_semidense_align_emu import case_inputs as align_inputs, same_result, synthetic_setup as align_setup
from test_semidense_propagate_gpu import PPRM, Chain
from test_semidense_regularize_emu import CASES, PLANES, restated, same_planes
from test_semidense_temporal_gpu import K, N_FRAMES, SH, SW, TPRM, _download, _driver, _run
from util import DeviceBuffer

pytestmark = pytest.mark.gpu

F = np.float32
OUT = (("invd", np.float32), ("sigma", np.float32), ("n_obs", np.uint8), ("rstatus", np.uint8))
RPRM = dict(chi=2.5, fill_min=6)  # (not the defaults: the driver must carry the caller's)


@pytest.fixture(scope="module")
def sdr_ctx(vo):
    c = vo.Context(device=0, max_width=203, max_height=61, max_points=256, n_slots=2, max_level=0)
    yield c
    c.close()


# ---- 1. the operator ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(CASES))
def test_operator_equals_restatement(vo, sdr_ctx, name):
    ctx = sdr_ctx
    c, want = restated(name)
    h, w = c["Lk"].shape
    got = ctx.semiDenseMapRegularize(c["map"], c["Lk"], c["mask"], **c["prm"])
    ok, where = same_planes(got._asdict(), want)
    assert ok, where
    assert got.frame_id is None and got.T_wc is None
    # every plane on the device, the key plane with a padded stride; twice in a row
    padded = np.full((h, w + 5), 0xEE, np.uint8)
    padded[:, :w] = c["Lk"]
    m = {k: DeviceBuffer(np.ascontiguousarray(c["map"][k])) for k in ("invd", "sigma", "n_obs")}
    out = {k: DeviceBuffer(np.full((h, w), 0x5A if dt is np.uint8 else -7, dt)) for k, dt in OUT}
    dkey = DeviceBuffer(padded)
    dmask = None if c["mask"] is None else DeviceBuffer(np.ascontiguousarray(c["mask"]))
    try:
        for rep in range(2):
            assert ctx.semiDenseMapRegularize({k: b.data_ptr() for k, b in m.items()}, dkey.data_ptr(), None if dmask is None else dmask.data_ptr(),
                                              out=dict({k: b.data_ptr() for k, b in out.items()}, size=(w, h)), key_on_device=w + 5,
                                              **c["prm"]) is None
            dev = {k: _download(out[k], dt, (h, w)) for k, dt in OUT}
            ok, where = same_planes(dev, want)
            assert ok, (rep, where)
        for k in ("invd", "sigma", "n_obs"):  # the inputs stay
            assert np.array_equal(_download(m[k], c["map"][k].dtype, (h, w)).view(np.uint8), np.ascontiguousarray(c["map"][k]).view(np.uint8)), k
    finally:
        dkey.free()
        for b in list(m.values()) + list(out.values()) + ([] if dmask is None else [dmask]):
            b.free()


def test_operator_argument_errors(vo, sdr_ctx):
    ctx = sdr_ctx
    c, _ = restated("c_97x45_step")
    call = lambda **kw: ctx.semiDenseMapRegularize(kw.pop("map", c["map"]), c["Lk"], c["mask"], **kw)
    for bad in (dict(radius=0), dict(radius=4), dict(chi=0.0), dict(chi=-1.0), dict(chi=float("nan")), dict(chi=float("inf")),
                dict(dist_sigma=-0.01), dict(dist_sigma=float("nan")), dict(dist_sigma=float("inf")), dict(min_support=-1), dict(min_support=49),
                dict(fill_min=-1), dict(fill_min=49), dict(g_min=0), dict(g_min=361)):
        with pytest.raises(vo.VoError) as e:
            call(**bad)
        assert e.value.code == -1, bad
    for good in (dict(radius=1), dict(radius=3), dict(dist_sigma=0.0), dict(min_support=0), dict(min_support=48), dict(fill_min=0),
                 dict(fill_min=48), dict(g_min=1), dict(g_min=360)):
        call(**good)
    with pytest.raises(ValueError):
        call(map={k: v[:, :50] for k, v in c["map"].items()})  # (another size than the key plane's)
    with pytest.raises(ValueError):
        call(max_search=64)
    # aliasing outputs, a bad stride, sizes
    h, w = c["Lk"].shape
    a, a2, b = np.zeros((h, w), F), np.zeros((h, w), F), np.zeros((h, w), np.uint8)
    o_invd, o_sigma, o_no, o_rs = np.zeros((h, w), F), np.zeros((h, w), F), np.zeros((h, w), np.uint8), np.zeros((h, w), np.uint8)
    key = np.ascontiguousarray(c["Lk"])
    p = vo._capi.SemiDenseRegularizeParams()
    ctx.lib.vo_semidense_regularize_default_params(C.byref(p))

    def rc(invd_r=o_invd, sigma_r=o_sigma, n_obs_r=o_no, rstatus=o_rs, stride=w, width=w, height=h, mask=None):
        return ctx.lib.vo_semidense_map_regularize(ctx.handle, a.ctypes.data, a2.ctypes.data, b.ctypes.data, key.ctypes.data, stride, 0,
                                                   None if mask is None else mask.ctypes.data, width, height, C.byref(p), invd_r.ctypes.data,
                                                   sigma_r.ctypes.data, n_obs_r.ctypes.data, rstatus.ctypes.data, 0)
    assert rc() == 0
    assert rc(invd_r=a) == -1 and rc(sigma_r=a2) == -1 and rc(invd_r=a2) == -1 and rc(n_obs_r=b) == -1 and rc(rstatus=b) == -1
    assert rc(rstatus=key) == -1 and rc(n_obs_r=o_rs) == -1 and rc(sigma_r=o_invd) == -1
    mask = np.ones((h, w), np.uint8)
    assert rc(mask=mask) == 0 and rc(mask=mask, rstatus=mask) == -1
    assert rc(stride=w - 1) == -1
    assert rc(width=204, stride=204) == -4 and rc(height=62) == -4 and rc(width=2) == -4 and rc(height=2) == -4  # VO_ERR_SIZE


def test_alignment_and_points_on_a_regularised_map(vo, sdr_ctx):
    """the operators that take a map take the regularised one: semiDenseAlign and semiDenseMapPoints equal their restatements on it"""
    ctx = sdr_ctx
    key, cur, Kc, T, m, prm, _ = align_inputs(align_setup(), "203x61_forward_epipole")
    want = RR.regularize(m, key)
    reg = ctx.semiDenseMapRegularize(m, key)
    ok, where = same_planes(reg._asdict(), want)
    assert ok, where
    assert (want["rstatus"] == 3).sum() >= 100 and (want["rstatus"] == 2).sum() >= 1
    ctx.set_image(0, cur)
    got = ctx.semiDenseAlign(key, 0, Kc, T, reg, **prm)
    d = got._asdict()
    d["H"] = np.array([d["H"][i, j] for i, j in AR.PAIRS])
    wa = AR.align(key, cur, Kc, T, {k: want[k] for k in ("invd", "sigma", "n_obs")}, **prm)
    ok, where = same_result(d, wa)
    assert ok, where
    assert wa["count"] > AR.align(key, cur, Kc, T, m, **prm)["count"]  # (the filled pixels take part)
    pyr = ctx.semiDenseMapPyramid(reg, 2)
    assert len(pyr) == 2 and np.array_equal(pyr[0]["invd"], reg.invd)
    Tm = np.array([[0.8, 0, 0.6, 1.5], [0, 1, 0, -0.25], [-0.6, 0, 0.8, 7.0], [0, 0, 0, 1]], F)
    for min_obs in (1, 2):
        wx, ws, wp = TR.map_points(want["invd"], want["sigma"], want["n_obs"], Kc, Tm, min_obs)
        gx, gs, gp = ctx.semiDenseMapPoints(reg, K=Kc, T=Tm, min_obs=min_obs)
        assert gx.shape == wx.shape and np.array_equal(gx.view(np.uint32), wx.view(np.uint32)), min_obs
        assert np.array_equal(gs.view(np.uint32), ws.view(np.uint32)) and np.array_equal(gp, wp)


# ---- 2. the driver --------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def stream():
    from visual_odometry_ros_amd import synthetic as S
    st = S.StereoStream(width=SW, height=SH, K=K, n_u=20, n_v=8, seed=2, speed=0.5)
    imgs = [st.render_pair(p)[:2] for p in st.poses(N_FRAMES)]
    bf = float(F(K[0] * st.baseline))
    return st, imgs, dict(bf=bf, d_min=0, d_max=67)


@pytest.fixture(scope="module")
def plain_runs(vo, stream):
    """the odometry with every option off, per calling mode (computed once)"""
    return {mode: _run(vo, stream, mode, None) for mode in ("lookahead", "sync", "sequence")}


@pytest.fixture(scope="module")
def chains(stream, plain_runs):
    """one chain of raw maps per distinct sequence of returned poses and per propagation setting (the three calling modes return the
    same bits: one chain serves them)"""
    _, imgs, prm = stream
    made = {}

    def get(vo, mode, propagate):
        key = (b"".join(plain_runs[mode][0]), propagate)
        if key not in made:
            made[key] = Chain(imgs, prm, [vo._capi.SvoFrameInfo.from_buffer_copy(b) for b in plain_runs[mode][0]],
                              plain=() if propagate else range(N_FRAMES))
        return made[key]
    return get


def _same_raw(svo, want, infos, k):
    r = svo.getSemiDenseMap()
    kf = want["kf"]
    assert r is not None and r.frame_id == infos[kf].frame_id and r.n_fused == k - kf, (k, kf, r.frame_id, r.n_fused)
    for p in ("tstatus", "n_obs", "invd", "sigma"):
        a, b = getattr(r, p), want["map"][p]
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), (k, kf, p, int((a != b).sum()))
    return r


def _same_regularised(svo, chain, k, prm, cache=None):
    """getSemiDenseMap(regularized=True) after frame k against the restatement applied to the chain's raw map; returns the restated"""
    want = chain.state(k)
    g = svo.getSemiDenseMap(regularized=True)
    if want is None:
        assert g is None, k
        return None
    kf = want["kf"]
    if cache is None or k not in cache:
        reg = RR.regularize(want["map"], chain.imgs[kf][0], chain.masks[kf], **prm)
        if cache is not None:
            cache[k] = reg
    else:
        reg = cache[k]
    assert g is not None and g.frame_id == chain.infos[kf].frame_id and g.n_fused == k - kf, (k, kf)
    assert np.array_equal(g.T_wc.view(np.uint32), chain.T[kf].view(np.uint32)), k
    ok, where = same_planes(g._asdict(), reg)
    assert ok, (k, kf, where)
    return reg


@pytest.mark.parametrize("mode,propagate", [("lookahead", True), ("sync", True), ("sequence", True), ("lookahead", False)])
def test_driver_regularised_map(vo, stream, chains, plain_runs, mode, propagate):
    _, _, prm = stream
    chain = chains(vo, mode, propagate)
    infos = chain.infos
    cache = chain.__dict__.setdefault("regularised", {})  # (the modes share the restated planes)
    seen = {"looked": [], "filled": 0, "removed": 0, "at_keyframe": 0}

    def check(k, svo):
        last = k == N_FRAMES - 1
        if not last and not infos[k + 1].is_keyframe and not infos[k].is_keyframe:
            return
        want = chain.state(k)
        if want is None:
            assert svo.getSemiDenseMap() is None and svo.getSemiDenseMap(regularized=True) is None, k
            assert svo.getSemiDensePoints(fused=True, regularized=True, min_obs=1) is None
            return
        _same_raw(svo, want, infos, k)  # the raw map: what the same run returns without the option
        reg = _same_regularised(svo, chain, k, RPRM, cache)
        seen["looked"].append(want["kf"])
        seen["filled"] += int((reg["rstatus"] == 3).sum())
        seen["removed"] += int((reg["rstatus"] == 2).sum())
        seen["at_keyframe"] += int(infos[k].is_keyframe)
        for world, min_obs in ((True, 1), (False, 2)):
            wx, ws, wp = TR.map_points(reg["invd"], reg["sigma"], reg["n_obs"], K, chain.T[want["kf"]] if world else None, min_obs)
            pts = svo.getSemiDensePoints(world=world, fused=True, regularized=True, min_obs=min_obs)
            assert pts["frame_id"] == infos[want["kf"]].frame_id and np.array_equal(pts["xyz"].view(np.uint32), wx.view(np.uint32)), (k, world)
            assert np.array_equal(pts["sigma_invd"].view(np.uint32), ws.view(np.uint32)) and np.array_equal(pts["pixel"], wp)

    sd = dict(prm, every="keyframe", temporal=dict(TPRM), regularize=dict(RPRM))
    if propagate:
        sd["propagate"] = dict(PPRM)
    infos_got, tracks = _run(vo, stream, mode, sd, check)
    assert infos_got == plain_runs[mode][0] and tracks == plain_runs[mode][1]
    assert seen["looked"] and seen["filled"] > 1000 and seen["removed"] > 10, seen
    if mode != "sequence":  # (runSequence is looked at after its last frame only)
        assert len(set(seen["looked"])) >= 2 and seen["at_keyframe"] >= 2, seen


def test_driver_mask_follows_the_keyframe_and_the_option_off_and_on(vo, stream):
    """Mask A from the start, mask B from frame 3 on: the fill takes the mask the keyframe's pair carried, whatever setMask has made of
    the later pairs' since. Then the option is switched off and on again between two frames: the getter refuses, then has nothing,
    then — after the next frame — the regularised map again; the raw map equals a plain driver's throughout."""
    st, imgs, prm = stream
    A = np.ones((SH, SW), np.uint8)  # (small regions: the odometry keeps its keyframe rhythm)
    A[40:200, 150:230] = 0
    A[220:, :] = 0
    B = np.ones((SH, SW), np.uint8)
    B[60:200, 400:480] = 0
    masks = [A if k < 3 else B for k in range(N_FRAMES)]
    c, svo = _driver(vo, st, dict(prm, every="keyframe", temporal=dict(TPRM), regularize=dict(RPRM)))
    c2, plain = _driver(vo, st, dict(prm, every="keyframe", temporal=dict(TPRM)))
    try:
        infos, seen, toggled_at = [], {"A": 0, "B": 0, "after_toggle": 0}, None
        chain = Chain(imgs, prm, infos, masks, plain=range(N_FRAMES))
        for k in range(N_FRAMES):
            svo.setMask(masks[k])
            plain.setMask(masks[k])
            gi = svo.trackStereoImages(*imgs[k])
            gp = plain.trackStereoImages(*imgs[k])
            assert bytes(gi) == bytes(gp), k
            infos.append(vo._capi.SvoFrameInfo.from_buffer_copy(bytes(gi)))
            chain.T = [np.array(i.T_wc, F).reshape(4, 4) for i in infos]
            want = chain.state(k)
            if want is None:
                continue
            a, b = svo.getSemiDenseMap(), plain.getSemiDenseMap()
            for p in ("tstatus", "n_obs", "invd", "sigma"):
                assert np.array_equal(getattr(a, p).view(np.uint8), getattr(b, p).view(np.uint8)), (k, p)
            reg = _same_regularised(svo, chain, k, RPRM)
            mk = masks[want["kf"]]
            assert (reg["rstatus"][mk == 0] != 3).all() and (reg["rstatus"][mk != 0] == 3).sum() > 100, k
            other = B if mk is A else A
            seen["A" if mk is A else "B"] += int((reg["rstatus"][(other == 0) & (mk != 0)] == 3).sum())
            seen["after_toggle"] += int(toggled_at == k - 1)
            if toggled_at is None and infos[k].is_keyframe and k >= 3:
                svo.setSemiDenseRegularize(None)
                with pytest.raises(vo.VoError):
                    svo.getSemiDenseMap(regularized=True)
                with pytest.raises(vo.VoError):
                    svo.getSemiDensePoints(fused=True, regularized=True)
                svo.setSemiDenseRegularize(dict(RPRM))
                assert svo.getSemiDenseMap(regularized=True) is None  # (no launch since the option came back)
                assert svo.getSemiDensePoints(fused=True, regularized=True) is None
                toggled_at = k
        # fills where only the OTHER mask ignores: under A's keyframes and under B's
        assert seen["A"] > 0 and seen["B"] > 0 and seen["after_toggle"] == 1, (seen, [i.is_keyframe for i in infos])
    finally:
        svo.close()
        c.close()
        plain.close()
        c2.close()


def test_driver_errors_and_allocations(vo, stream):
    st, imgs, prm = stream
    c, svo = _driver(vo, st)
    c2, plain = _driver(vo, st, dict(prm, every="keyframe", temporal=dict(TPRM)))

    def count(ctx_):
        n = C.c_longlong()
        ctx_.check(ctx_.lib.vo_debug_allocation_count(ctx_.handle, C.byref(n)))
        return n.value
    try:
        assert not hasattr(vo.MonoVO, "setSemiDenseRegularize")  # a stereo driver's option (the C call refuses a mono driver's core)
        svo.setSemiDense(dict(prm))
        with pytest.raises(vo.VoError) as e:  # needs the temporal option
            svo.setSemiDenseRegularize({})
        assert e.value.code == -1
        svo.setSemiDenseTemporal(dict(TPRM))
        with pytest.raises(vo.VoError):  # the option is off
            svo.getSemiDenseMap(regularized=True)
        with pytest.raises(vo.VoError):
            svo.getSemiDensePoints(fused=True, regularized=True)
        with pytest.raises(ValueError):
            svo.getSemiDensePoints(regularized=True)
        with pytest.raises(vo.VoError):
            svo.setSemiDenseRegularize(dict(radius=4))
        with pytest.raises(ValueError):
            svo.setSemiDenseRegularize(dict(bf=1.0))
        for k in (0, 1):  # the option off: the allocation count moves as a driver's that never heard of it
            svo.trackStereoImages(*imgs[k])
            plain.trackStereoImages(*imgs[k])
        n0, m0 = count(c), count(c2)
        svo.setSemiDenseRegularize(None)
        assert count(c) == n0
        svo.setSemiDenseRegularize({})
        assert count(c) == n0 + 1  # the option's only allocation
        assert svo.getSemiDenseMap(regularized=True) is None  # no launch yet
        svo.setSemiDenseRegularize(dict(RPRM))
        assert count(c) == n0 + 1  # a second enable allocates nothing
        svo.enqueue(*imgs[2])
        for call in (lambda: svo.setSemiDenseRegularize(None), lambda: svo.setSemiDenseRegularize({}),
                     lambda: svo.getSemiDenseMap(regularized=True), lambda: svo.getSemiDensePoints(fused=True, regularized=True)):  # in flight
            with pytest.raises(vo.VoError) as e:
                call()
            assert e.value.code == -1
        svo.result()
        plain.trackStereoImages(*imgs[2])
        g, r = svo.getSemiDenseMap(regularized=True), svo.getSemiDenseMap()
        assert g is not None and g.frame_id == r.frame_id and g.n_fused == r.n_fused and (g.rstatus == 3).sum() > 100
        n = int((g.n_obs >= 1).sum())
        assert len(svo.getSemiDensePoints(fused=True, regularized=True, min_obs=1)["xyz"]) == n
        assert len(plain.getSemiDensePoints(fused=True, min_obs=1)["xyz"]) == int((r.n_obs >= 1).sum())
        with pytest.raises(vo.VoError) as e:
            svo.getSemiDensePoints(fused=True, regularized=True, min_obs=1, capacity=10)
        assert e.value.code == -8 and e.value.n == n
        with pytest.raises(vo.VoError):
            svo.getSemiDensePoints(fused=True, regularized=True, min_obs=0)
        svo.trackStereoImages(*imgs[3])
        plain.trackStereoImages(*imgs[3])
        assert count(c) - n0 == count(c2) - m0 + 1  # frames and getters with the option on allocate nothing of their own
        svo.setSemiDenseTemporal(None)  # the map is gone: so is its regularised copy
        with pytest.raises(vo.VoError):
            svo.getSemiDenseMap(regularized=True)
        svo.setSemiDenseTemporal(dict(TPRM))
        assert svo.getSemiDenseMap(regularized=True) is None
    finally:
        svo.close()
        c.close()
        plain.close()
        c2.close()
