"""The speckle filter on the device (include/vo_hip.h, "Speckle filter") against the restatement
(tests/dense_speckle_restatement.py), everything bit for bit: the operator on the cases of the emulation test — host planes, device
planes in place, the optional outputs NULL, the workspace reused over growing shapes —; denseStereo(speckle=) against the operator
behind denseStereo; the filtered planes through the points list, the map seed and the world integration against their restatements;
and StereoVO's option: the odometry unchanged by it, every dense result the restatement of that frame's own pair (per keyframe and
per frame, through the look-ahead calls, the synchronous call and runSequence), the stats getter, unfiltered results with the option
off again. (The C calls' refusal of a mono driver is not exercised: no public call yields the vo_svo core of a MonoVO, so only the
absence of the methods on MonoVO is asserted.)"""
import ctypes as C

import numpy as np
import pytest

import semidense_world_restatement as WR
from dense_speckle_restatement import DEFAULTS, speckle_filter
from dense_stereo_restatement import dense_stereo
from semidense_restatement import points
from semidense_temporal_restatement import seed
from test_dense_speckle_emu import CASES, case, same_result
from test_dense_stereo_emu import case_inputs, same_planes
from test_dense_stereo_gpu import K, N_FRAMES, _download, _driver, _load, _run
from test_dense_stereo_gpu import stream  # noqa: F401  (a fixture: the 640 x 240, 10-frame stream and the dense parameters)
from test_semidense_emu import synthetic_pair
from test_semidense_world import same_records
from util import DeviceBuffer

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def spk_ctx(vo):
    c = vo.Context(device=0, max_width=203, max_height=120, max_points=256, n_slots=2, max_level=0)
    yield c
    c.close()


def _count(ctx):
    n = C.c_longlong()
    ctx.check(ctx.lib.vo_debug_allocation_count(ctx.handle, C.byref(n)))
    return n.value


def _on_device(vo, ctx, d, s, st, prm, outputs=True):
    """the operator in place on device planes -> what it left there (label and size only with `outputs`) and the two counts"""
    h, w = st.shape
    bufs = dict(disparity=DeviceBuffer(d), status=DeviceBuffer(st))
    if s is not None:
        bufs["sigma_invd"] = DeviceBuffer(s)
    if outputs:
        bufs["label"], bufs["size"] = (DeviceBuffer(np.full((h, w), 0x5A5A5A5A, np.int32)) for _ in range(2))
    try:
        p = vo.api._speckle_params(ctx.lib, prm)
        nr, nc = C.c_int(-5), C.c_int(-5)
        ptr = lambda k: C.c_void_p(bufs[k].data_ptr()) if k in bufs else None
        ctx.check(ctx.lib.vo_disparity_speckle_filter(ctx.handle, ptr("disparity"), ptr("sigma_invd"), ptr("status"), w, h, C.byref(p), ptr("label"),
                                                      ptr("size"), C.byref(nr) if outputs else None, C.byref(nc) if outputs else None, 1))
        types = dict(disparity=np.float32, sigma_invd=np.float32, status=np.uint8, label=np.int32, size=np.int32)
        got = {k: _download(b, types[k], (h, w)) for k, b in bufs.items()}
        got.setdefault("sigma_invd", None)
        if outputs:
            got.update(n_removed=nr.value, n_components=nc.value)
        return got
    finally:
        for b in bufs.values():
            b.free()


# ---- 1. the operator -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(CASES))
def test_operator_equals_restatement(vo, spk_ctx, name):
    """host planes (the caller's arrays keep their bits), device planes in place with label and size in device memory, and every
    optional output NULL"""
    ctx = spk_ctx
    d, s, st, prm, want = case(name)
    got = ctx.disparitySpeckleFilter(d, s, st, labels=True, **dict(DEFAULTS, **prm))
    assert same_result(got._asdict(), want) is None
    plain = ctx.disparitySpeckleFilter(d, s, st, **dict(DEFAULTS, **prm))
    assert plain.label is None and plain.size is None and same_result(plain._asdict(), want) is None
    assert same_result(_on_device(vo, ctx, d, s, st, prm), want) is None
    bare = _on_device(vo, ctx, d, None, st, prm, outputs=False)  # no sigma plane, no label, size or counts
    assert same_result(dict(bare, sigma_invd=None), dict(want, sigma_invd=None)) is None


def test_workspace_grows_with_the_shape_and_is_reused(vo):
    """a fresh context: the first call allocates the workspace and the host planes' copy, a larger shape both again, a smaller or
    equal one nothing; every result is right, whatever the workspace held before"""
    c = vo.Context(device=0, max_width=64, max_height=64, max_points=256, n_slots=2, max_level=0)
    try:
        moved = []
        for name in ("97x1", "1x97", "65x17", "203x37", "65x17", "serpentine", "203x37", "1x97", "full"):
            d, s, st, prm, want = case(name)
            n0 = _count(c)
            got = c.disparitySpeckleFilter(d, s, st, labels=True, **dict(DEFAULTS, **prm))
            moved.append(_count(c) - n0)
            assert same_result(got._asdict(), want) is None, name
            assert c.disparitySpeckleWorkspace(st.shape[1], st.shape[0]) == 16 + 8 * st.size
        #   97   97  1105  7511  1105  10500  7511  97  10500 pixels
        assert moved == [2, 0, 2, 2, 0, 2, 0, 0, 0], moved
        n0 = _count(c)
        d, s, st, prm, want = case("203x37")  # device planes take no copy: nothing more
        assert same_result(_on_device(vo, c, d, s, st, prm), want) is None and _count(c) == n0
    finally:
        c.close()


def test_operator_argument_errors(vo, spk_ctx):
    ctx = spk_ctx
    d, s, st, prm, want = case("65x17")
    for bad in (dict(max_size=-1), dict(max_diff=-0.5), dict(max_diff=float("nan")), dict(max_diff=float("inf"))):
        with pytest.raises(vo.VoError) as e:
            ctx.disparitySpeckleFilter(d, s, st, **dict(DEFAULTS, **dict(prm, **bad)))
        assert e.value.code == -1, bad
    with pytest.raises(ValueError):
        ctx.disparitySpeckleFilter(d, s[:, :-1], st)
    p = vo.api._speckle_params(ctx.lib, True)
    dd, ss = np.array(d), np.array(st)
    args = lambda **k: (k.get("d", dd.ctypes.data), None, k.get("st", ss.ctypes.data), k.get("w", 65), k.get("h", 17), k.get("p", C.byref(p)), None,
                        None, None, None, 0)
    for bad in (dict(d=None), dict(st=None), dict(p=None), dict(w=0), dict(h=0), dict(w=65536), dict(w=-3)):
        assert ctx.lib.vo_disparity_speckle_filter(ctx.handle, *args(**bad)) in (-1, -4), bad
    assert np.array_equal(dd.view(np.uint32), d.view(np.uint32)) and np.array_equal(ss, st)  # (nothing was touched)
    assert ctx.lib.vo_disparity_speckle_filter(ctx.handle, *args()) == 0


# ---- 2. behind the dense operator, and into the semi-dense chain -----------------------------------------------------------------------
@pytest.fixture(scope="module")
def dense_case(vo, spk_ctx):
    """the dense operator's result on the 203 x 37 crop (the device's, which test_dense_stereo_gpu.py holds to the restatement) and
    the restated filter behind it"""
    left, right, mask, prm, _ = case_inputs(synthetic_pair(), "203x37_n128")
    _load(spk_ctx, left, right, mask)
    r = spk_ctx.denseStereo(0, 1, **prm)
    sp = dict(max_size=20, max_diff=1.0)
    return left, right, mask, prm, r, sp, speckle_filter(r.disparity, r.sigma_invd, r.status, **sp)


def test_dense_stereo_with_speckle_equals_the_operator_behind_it(vo, spk_ctx, dense_case):
    ctx = spk_ctx
    left, right, mask, prm, r, sp, want = dense_case
    h, w = left.shape
    assert 0 < want["n_removed"] < r.n_accepted
    _load(ctx, left, right, mask)
    got = ctx.denseStereo(0, 1, speckle=sp, **prm)
    assert same_result(got._asdict(), want) is None and np.array_equal(got.cost, r.cost)
    assert got.n_accepted == r.n_accepted - want["n_removed"]
    by_op = ctx.disparitySpeckleFilter(r.disparity, r.sigma_invd, r.status, **sp)
    assert same_result(by_op._asdict(), want) is None and by_op.n_removed == want["n_removed"]
    for off in (None, False):  # off: the dense operator's own bits
        ok, where = same_planes(ctx.denseStereo(0, 1, speckle=off, **prm)._asdict(), r._asdict())
        assert ok, where
    planes = (("disparity", np.float32), ("cost", np.uint16), ("sigma_invd", np.float32), ("status", np.uint8))
    bufs = {k: DeviceBuffer(np.full((h, w), 0x5A, np.uint8).astype(dt)) for k, dt in planes}
    try:
        assert ctx.denseStereo(0, 1, out={k: b.data_ptr() for k, b in bufs.items()}, speckle=sp, **prm) is None
        dev = {k: _download(bufs[k], dt, (h, w)) for k, dt in planes}
        assert same_result(dev, want) is None and np.array_equal(dev["cost"], r.cost)
        with pytest.raises(ValueError):
            ctx.denseStereo(0, 1, out=dict(cost=bufs["cost"].data_ptr()), speckle=True, **prm)
    finally:
        for b in bufs.values():
            b.free()
    d2, _, st2, _, w2 = case("dense_203x37_n128")  # (the restated dense result of the same crop, without its sigma plane)
    assert same_result(ctx.disparitySpeckleFilter(d2, None, st2, max_size=20)._asdict(), dict(w2, sigma_invd=None)) is None


def test_filtered_planes_go_through_points_seed_and_world(vo, spk_ctx, dense_case):
    ctx = spk_ctx
    left, _, _, prm, r, sp, want = dense_case
    bf = prm["bf"]
    got = ctx.disparitySpeckleFilter(r.disparity, r.sigma_invd, r.status, **sp)
    T = np.array([[0.8, 0, 0.6, 1.5], [0, 1, 0, -0.25], [-0.6, 0, 0.8, 7.0], [0, 0, 0, 1]], np.float32)
    for Tm in (None, T):
        wx, ws, wp = points(want["disparity"], want["sigma_invd"], want["status"], K, bf, Tm)
        gx, gs, gp = ctx.semiDensePoints(got.disparity, got.sigma_invd, got.status, K, bf, Tm)
        assert len(wx) == r.n_accepted - want["n_removed"] and gx.shape == wx.shape and np.array_equal(gx.view(np.uint32), wx.view(np.uint32))
        assert np.array_equal(gs.view(np.uint32), ws.view(np.uint32)) and np.array_equal(gp, wp)
    m = ctx.semiDenseMapSeed(got.disparity, got.sigma_invd, got.status, bf)
    wm_ = seed(want["disparity"], want["sigma_invd"], want["status"], bf)
    assert np.array_equal(m.invd.view(np.uint32), wm_["invd"].view(np.uint32)) and np.array_equal(m.sigma.view(np.uint32), wm_["sigma"].view(np.uint32))
    assert np.array_equal(m.n_obs, wm_["n_obs"]) and int((m.n_obs > 0).sum()) == r.n_accepted - want["n_removed"]
    wprm = dict(voxel=0.1, capacity_log2=16, min_obs=1, z_max=40.0)
    world = WR.World(**wprm)
    assert world.integrate(wm_, K, T, left)
    with ctx.semiDenseWorld(**wprm) as wm:
        wm.integrate(m, K, T, key=left)
        ok, where = same_records(wm.points()._asdict(), world.records(), fields=("index", "sums", "count", "keyframes", "weight", "grey", "xyz"))
        assert ok, where
        assert wm.stats() == world.stats


# ---- 3. the driver -----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def restated(stream):
    """per frame: the restated dense result of its own pair and, per filter parameters, the restated filter behind it; computed when
    first asked for and kept"""
    _, imgs, prm = stream
    dense, filtered = {}, {}

    def get(k, sp=None):
        if k not in dense:
            r = dense_stereo(imgs[k][0], imgs[k][1], **prm)
            r.pop("S")
            dense[k] = r
        if sp is None:
            return dense[k]
        key = (k, tuple(sorted(sp.items())))
        if key not in filtered:
            r = dense[k]
            filtered[key] = dict(speckle_filter(r["disparity"], r["sigma_invd"], r["status"], **sp), cost=r["cost"])
        return filtered[key]
    return get


@pytest.fixture(scope="module")
def plain_runs(vo, stream):
    """the odometry with every option off, per calling mode (computed once)"""
    return {mode: _run(vo, stream, mode, {}) for mode in ("lookahead", "sync", "sequence")}


def _same_dense(r, want):
    """a driver's DenseStereoResult against a restated (filtered) result: None or where they differ"""
    where = same_result(r._asdict(), want)
    if where is None and not np.array_equal(r.cost, want["cost"]):
        where = ("cost",)
    return where


@pytest.mark.parametrize("mode", ["lookahead", "sync", "sequence"])
def test_driver_keyframes(vo, stream, restated, plain_runs, mode):
    """every = keyframes, the filter on with its defaults: the odometry's bits are those of every option off; the planes are the
    restated filter behind the restated dense result of the last keyframe's own pair, n_accepted what is left, the stats that
    filter's counts. Looked at after every second frame and after the last one (a look a frame or two behind a keyframe, when the
    next pairs have been ingested, would show a slot reused under the launches)."""
    _, _, prm = stream
    plain_infos = [vo._capi.SvoFrameInfo.from_buffer_copy(b) for b in plain_runs[mode][0]]
    by_id = {i.frame_id: k for k, i in enumerate(plain_infos)}
    seen = {"looked": [], "late": 0, "removed": 0}

    def check(k, gi, svo):
        if mode != "sequence" and not (k % 2 == 1 or k == N_FRAMES - 1):
            return
        r = svo.getDenseStereo()
        kfs = [j for j in range(k + 1) if plain_infos[j].is_keyframe]
        if not kfs:
            assert r is None and svo.getDenseSpeckleStats() == (0, 0), k
            return
        kf = kfs[-1]
        assert r is not None and by_id[r.frame_id] == kf, (k, kf, r.frame_id)
        want = restated(kf, DEFAULTS)
        assert _same_dense(r, want) is None, (k, kf, _same_dense(r, want))
        assert r.n_accepted == restated(kf)["n_accepted"] - want["n_removed"] == int((want["status"] == 1).sum())
        assert svo.getDenseSpeckleStats() == (want["n_removed"], want["n_components"])
        assert len(svo.getDensePoints()["xyz"]) == r.n_accepted
        seen["looked"].append(kf)
        seen["late"] += kf < k
        seen["removed"] += want["n_removed"]

    infos, tracks, _ = _run(vo, stream, mode, dict(dense=dict(prm, every="keyframe", speckle=True)), check)
    assert infos == plain_runs[mode][0] and tracks == plain_runs[mode][1]
    assert seen["looked"] and seen["removed"] > 0
    if mode != "sequence":
        assert len(set(seen["looked"])) >= 2 and seen["late"] >= 1, seen


def test_driver_every_frame_on_off_and_points(vo, stream, restated, plain_runs):
    """every = frames, four frames, look-ahead. Frames 0 and 1 with the filter at (50, 2.0): a filtered result per frame (the first
    pair included) and the points without the speckles; then off: frame 2 is the dense restatement's bits — what the driver gave
    before the option existed — and the stats are refused; then on with the defaults: frame 3 is filtered again."""
    _, _, prm = stream
    sp = dict(max_size=50, max_diff=2.0)

    def check(k, gi, svo):
        r = svo.getDenseStereo()
        assert r is not None and r.frame_id == gi.frame_id, k
        if k == 2:
            ok, where = same_planes(r._asdict(), restated(k))
            assert ok and r.n_accepted == restated(k)["n_accepted"], (k, where)
            with pytest.raises(vo.VoError) as e:
                svo.getDenseSpeckleStats()
            assert e.value.code == -1
            svo.setDenseSpeckle(True)
            assert svo.getDenseSpeckleStats() == (0, 0)  # (the last result did not go through the filter)
            return
        want = restated(k, sp if k < 2 else DEFAULTS)
        assert _same_dense(r, want) is None, (k, _same_dense(r, want))
        assert svo.getDenseSpeckleStats() == (want["n_removed"], want["n_components"]) and want["n_removed"] > 0
        T = np.array(gi.T_wc, np.float32).reshape(4, 4)
        if k == 1:
            for world in (True, False):
                wx, ws, wp = points(want["disparity"], want["sigma_invd"], want["status"], K, prm["bf"], T if world else None)
                p = svo.getDensePoints(world=world)
                assert p["frame_id"] == gi.frame_id and np.array_equal(p["xyz"].view(np.uint32), wx.view(np.uint32)), (k, world)
                assert np.array_equal(p["sigma_invd"].view(np.uint32), ws.view(np.uint32)) and np.array_equal(p["pixel"], wp)
            svo.setDenseSpeckle(None)

    infos, _, _ = _run(vo, stream, "lookahead", dict(dense=dict(prm, every="frame", speckle=sp)), check, n=4)
    assert infos == plain_runs["lookahead"][0][:4]


def test_driver_dense_without_speckle_is_unchanged(vo, stream, restated, plain_runs):
    """dense on, the filter never enabled: every result is the dense restatement's bits, as before the option existed"""
    _, _, prm = stream

    def check(k, gi, svo):
        r = svo.getDenseStereo()
        ok, where = same_planes(r._asdict(), restated(k))
        assert ok and r.frame_id == gi.frame_id and r.n_accepted == restated(k)["n_accepted"], (k, where)

    infos, _, _ = _run(vo, stream, "sync", dict(dense=dict(prm, every="frame")), check, n=3)
    assert infos == plain_runs["sync"][0][:3]


def test_driver_setter_errors_and_allocations(vo, stream):
    st, imgs, prm = stream
    c, svo = _driver(vo, st)
    try:
        with pytest.raises(vo.VoError) as e:  # needs the dense option
            svo.setDenseSpeckle(True)
        assert e.value.code == -1
        svo.setDenseSpeckle(None)  # (off is always accepted)
        with pytest.raises(vo.VoError):
            svo.getDenseSpeckleStats()
        svo.setDenseStereo(dict(prm))
        for bad in (dict(max_size=-1), dict(max_diff=-1.0), dict(max_diff=float("nan")), dict(max_diff=float("inf"))):
            with pytest.raises(vo.VoError) as e:
                svo.setDenseSpeckle(bad)
            assert e.value.code == -1, bad
        with pytest.raises(ValueError):
            svo.setDenseSpeckle(dict(size=3))
        with pytest.raises(vo.VoError):  # (none of these switched it on)
            svo.getDenseSpeckleStats()
        n0 = _count(c)
        svo.setDenseSpeckle(dict(max_size=30))
        assert _count(c) == n0 + 1  # the option's only allocation: the workspace for max_width x max_height
        assert svo.getDenseSpeckleStats() == (0, 0)
        svo.enqueue(*imgs[0])
        for call in (lambda: svo.setDenseSpeckle(None), lambda: svo.setDenseSpeckle(True), svo.getDenseSpeckleStats):  # a frame is in flight
            with pytest.raises(vo.VoError) as e:
                call()
            assert e.value.code == -1
        svo.result()
        svo.trackStereoImages(*imgs[1])  # (the first keyframe)
        r, (n_removed, n_components) = svo.getDenseStereo(), svo.getDenseSpeckleStats()
        assert int((r.status == vo.DISPARITY_SPECKLE).sum()) == n_removed > 0 and n_components > 1
        assert r.n_accepted == int((r.status == 1).sum()) and (r.disparity[r.status == 6] == 0).all() and (r.sigma_invd[r.status == 6] == 0).all()
        # over later frames, results, getters and re-enabling, the allocation count moves exactly as for a driver with the dense
        # option alone
        n0 = _count(c)
        svo.setDenseSpeckle(None)
        svo.setDenseSpeckle(True)
        for k in (2, 3):
            svo.trackStereoImages(*imgs[k])
            svo.getDenseStereo(), svo.getDenseSpeckleStats(), svo.getDensePoints()
        c2, plain = _driver(vo, st, dense=dict(prm))
        try:
            for k in (0, 1):
                plain.trackStereoImages(*imgs[k])
            plain.getDenseStereo()
            m0 = _count(c2)
            for k in (2, 3):
                plain.trackStereoImages(*imgs[k])
                plain.getDenseStereo(), plain.getDensePoints()
            assert _count(c) - n0 == _count(c2) - m0
        finally:
            plain.close()
            c2.close()
        assert not hasattr(vo.MonoVO, "setDenseSpeckle") and not hasattr(vo.MonoVO, "getDenseSpeckleStats")
    finally:
        svo.close()
        c.close()
