"""The propagation of the semi-dense map on the device (include/vo_hip.h, "Semi-dense propagation") against the numpy
restatement (tests/semidense_propagate_restatement.py), everything bit for bit: the operator on the emulation test's cases — host
planes, device planes, and the device call twice in a row, which the second passes only if the first left the plane of keys clean —
and StereoVO's option: the odometry unchanged by it, the map and origin at every keyframe change and at the end equal to the
restatements chained over the images and the returned poses (static, seed or propagation, the temporal launch per frame), through
the look-ahead calls, the synchronous call and runSequence; a mask that changes between keyframes; the option switched off and on."""
import ctypes as C

import numpy as np
import pytest

import semidense_propagate_restatement as PR
import semidense_restatement as SR
import semidense_temporal_restatement as TR
from test_semidense_propagate_emu import CASES, case_inputs, restate, same_planes, synthetic_setup
from test_semidense_temporal_gpu import K, N_FRAMES, SH, SW, TPRM, _download, _driver, _run
from util import DeviceBuffer

pytestmark = pytest.mark.gpu

F = np.float32
OUT = (("invd", np.float32), ("sigma", np.float32), ("n_obs", np.uint8), ("tstatus", np.uint8), ("origin", np.uint8), ("src", np.int32))
PPRM = dict(max_diff=25, chi=2.5)  # (not the defaults: the driver must carry the caller's)


@pytest.fixture(scope="module")
def frames():
    return synthetic_setup()


@pytest.fixture(scope="module")
def sdp_ctx(vo):
    c = vo.Context(device=0, max_width=203, max_height=61, max_points=256, n_slots=2, max_level=0)
    yield c
    c.close()


# ---- 1. the operator ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(CASES))
def test_operator_equals_restatement(vo, sdp_ctx, frames, name):
    ctx = sdp_ctx
    c = case_inputs(frames, name)
    want = restate(c)
    h, w = c["La"].shape
    ctx.set_image(0, c["Lb"])
    ctx.set_slot_mask(0, c["mask"])
    got = ctx.semiDenseMapPropagate(c["old"], c["La"], 0, c["stat"], c["bf"], c["K"], c["T"], **c["prm"])
    ok, where = same_planes(got._asdict(), want)
    assert ok, where
    # every plane on the device, the key plane with a padded stride; twice: the second call starts from the keys the first left
    padded = np.full((h, w + 5), 0xEE, np.uint8)
    padded[:, :w] = c["La"]
    old = {k: DeviceBuffer(np.ascontiguousarray(c["old"][k])) for k in ("invd", "sigma", "n_obs")}
    stat = {k: DeviceBuffer(np.ascontiguousarray(c["stat"][k])) for k in ("disparity", "sigma_invd", "status")}
    out = {k: DeviceBuffer(np.full((h, w), 0x5A if dt is np.uint8 else -7, dt)) for k, dt in OUT}
    dkey = DeviceBuffer(padded)
    try:
        for rep in range(2):
            assert ctx.semiDenseMapPropagate({k: b.data_ptr() for k, b in old.items()}, dkey.data_ptr(), 0, {k: b.data_ptr() for k, b in stat.items()},
                                             c["bf"], c["K"], c["T"], out={k: b.data_ptr() for k, b in out.items()}, key_on_device=w + 5,
                                             **c["prm"]) is None
            dev = {k: _download(out[k], dt, (h, w)) for k, dt in OUT}
            ok, where = same_planes(dev, want)
            assert ok, (rep, where)
        # origin and src are optional
        assert ctx.semiDenseMapPropagate({k: b.data_ptr() for k, b in old.items()}, dkey.data_ptr(), 0, {k: b.data_ptr() for k, b in stat.items()},
                                         c["bf"], c["K"], c["T"], out={k: out[k].data_ptr() for k in ("invd", "sigma", "n_obs", "tstatus")},
                                         key_on_device=w + 5, **c["prm"]) is None
        for k, dt in OUT[:4]:
            assert np.array_equal(_download(out[k], dt, (h, w)).view(np.uint8), np.ascontiguousarray(want[k]).view(np.uint8)), k
    finally:
        dkey.free()
        for b in list(old.values()) + list(stat.values()) + list(out.values()):
            b.free()
    # the host call once more: the context's own keys came back clean from every call above
    got = ctx.semiDenseMapPropagate(c["old"], c["La"], 0, c["stat"], c["bf"], c["K"], c["T"], **c["prm"])
    ok, where = same_planes(got._asdict(), want)
    assert ok, where


def test_operator_argument_errors(vo, sdp_ctx, frames):
    ctx = sdp_ctx
    c = case_inputs(frames, "97x45_inconsistent")
    ctx.set_image(0, c["Lb"])
    ctx.set_slot_mask(0, None)
    call = lambda **kw: ctx.semiDenseMapPropagate(kw.pop("old", c["old"]), c["La"], kw.pop("slot", 0), c["stat"], kw.pop("bf", c["bf"]), c["K"],
                                                  kw.pop("T", c["T"]), **dict(c["prm"], **kw))
    for bad in (dict(min_obs=0), dict(min_obs=256), dict(max_diff=-1), dict(max_diff=256), dict(chi=0.0), dict(chi=float("nan")),
                dict(chi=float("inf")), dict(sigma_add=-1.0), dict(sigma_add=float("nan")), dict(bf=0.0)):
        with pytest.raises(vo.VoError) as e:
            call(**bad)
        assert e.value.code == -1, bad
    with pytest.raises(vo.VoError):
        call(slot=5)
    bad_T = np.array(c["T"], F)
    bad_T[0, 3] = np.nan
    with pytest.raises(vo.VoError):
        call(T=bad_T)
    with pytest.raises(ValueError):
        call(old={k: v[:, :50] for k, v in c["old"].items()})  # (another size)
    with pytest.raises(ValueError):
        ctx.semiDenseMapPropagate(c["old"], c["La"], 0, c["stat"], c["bf"], c["K"], c["T"], max_search=64)
    # the new map's planes may not be the old map's
    h, w = c["La"].shape
    a, a2, b = np.zeros((h, w), F), np.zeros((h, w), F), np.zeros((h, w), np.uint8)
    o_invd, o_sigma, o_no, o_ts = np.zeros((h, w), F), np.zeros((h, w), F), np.zeros((h, w), np.uint8), np.zeros((h, w), np.uint8)
    p = vo._capi.SemiDensePropagateParams()
    ctx.lib.vo_semidense_propagate_default_params(C.byref(p))
    Ka, Ta = np.array(c["K"], F), np.eye(4, dtype=F)
    args = lambda invd, stride=w: (ctx.handle, a.ctypes.data, a2.ctypes.data, b.ctypes.data, c["La"].ctypes.data, stride, 0, a.ctypes.data,
                                   a.ctypes.data, b.ctypes.data, C.c_float(1.0), Ka.ctypes.data, Ta.ctypes.data, C.byref(p), invd.ctypes.data,
                                   o_sigma.ctypes.data, o_no.ctypes.data, o_ts.ctypes.data, None, None, 0)
    assert ctx.lib.vo_semidense_map_propagate(*args(a)) == -1
    assert ctx.lib.vo_semidense_map_propagate(*args(o_invd)) == 0
    assert ctx.lib.vo_semidense_map_propagate(*args(o_invd, w - 1)) == -1


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


class Chain:
    """the restatements chained over the images under the poses a run returned: state(k) = the map after frame k — dict(map, origin,
    from_id, kf) or None before a keyframe. masks[k]: the mask pair k carried (None: none). Statics and states are computed when
    first asked for and kept; plain: keyframes at which the option had just been switched on seed plainly."""

    def __init__(self, imgs, prm, infos, masks=None, plain=()):
        self.imgs, self.prm, self.infos, self.plain = imgs, prm, infos, set(plain)
        self.masks = masks or [None] * len(imgs)
        self.T = [np.array(i.T_wc, F).reshape(4, 4) for i in infos]
        self.cache = {}

    def static(self, k):
        return SR.semidense(self.imgs[k][0], self.imgs[k][1], self.masks[k], **self.prm)

    def state(self, k):
        if k < 0:
            return None
        if k not in self.cache:
            prev = self.state(k - 1)
            if self.infos[k].is_keyframe:
                s = self.static(k)
                if prev is None or k in self.plain:
                    m = TR.seed(s["disparity"], s["sigma_invd"], s["status"], F(self.prm["bf"]))
                    st = dict(map=m, origin=(s["status"] == 1).astype(np.uint8), from_id=-1, kf=k)
                else:
                    kf = prev["kf"]
                    o = PR.propagate(prev["map"], self.imgs[kf][0], self.imgs[k][0], s, F(self.prm["bf"]), K, TR.pose_ck(self.T[k], self.T[kf]),
                                     self.masks[k], **PPRM)
                    st = dict(map={p: o[p] for p in ("invd", "sigma", "n_obs", "tstatus")}, origin=o["origin"], from_id=self.infos[kf].frame_id,
                              kf=k, counts=o["counts"])
            elif prev is None:
                st = None
            else:
                kf = prev["kf"]
                out = TR.temporal(self.imgs[kf][0], self.imgs[k][0], K, TR.pose_ck(self.T[k], self.T[kf]), prev["map"], self.masks[kf], **TPRM)
                st = dict(prev, map={p: out[p] for p in ("invd", "sigma", "n_obs", "tstatus")})
            self.cache[k] = st
        return self.cache[k]


def _same_state(svo, want, infos, k):
    r = svo.getSemiDenseMap()
    if want is None:
        assert r is None and svo.getSemiDenseOrigin() is None, k
        return
    kf = want["kf"]
    assert r is not None and r.frame_id == infos[kf].frame_id and r.n_fused == k - kf, (k, kf, r.frame_id, r.n_fused)
    for p in ("tstatus", "n_obs", "invd", "sigma"):
        a, b = getattr(r, p), want["map"][p]
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), (k, kf, p, int((a != b).sum()))
    origin, from_id = svo.getSemiDenseOrigin()
    assert from_id == want["from_id"], (k, from_id, want["from_id"])
    assert np.array_equal(origin, want["origin"]), (k, int((origin != want["origin"]).sum()))


@pytest.fixture(scope="module")
def chains(stream, plain_runs):
    """one chain per distinct sequence of returned poses (the three calling modes return the same bits: one chain serves them)"""
    _, imgs, prm = stream
    made = {}

    def get(vo, mode):
        key = b"".join(plain_runs[mode][0])
        if key not in made:
            made[key] = Chain(imgs, prm, [vo._capi.SvoFrameInfo.from_buffer_copy(b) for b in plain_runs[mode][0]])
        return made[key]
    return get


@pytest.mark.parametrize("mode", ["lookahead", "sync", "sequence"])
def test_driver_map(vo, stream, chains, plain_runs, mode):
    _, _, prm = stream
    chain = chains(vo, mode)
    infos = chain.infos
    seen = {"looked": [], "propagated": 0, "twice_at_keyframe": 0}

    def check(k, svo):
        last = k == N_FRAMES - 1
        if not last and not infos[k + 1].is_keyframe and not infos[k].is_keyframe:
            return
        want = chain.state(k)
        _same_state(svo, want, infos, k)
        if want is None:
            return
        seen["looked"].append(want["kf"])
        if infos[k].is_keyframe and want["from_id"] >= 0:  # on the keyframe frame itself the fused getter has points
            seen["propagated"] += int((want["origin"] >= 2).sum())
            n2 = int((want["map"]["n_obs"] >= 2).sum())
            seen["twice_at_keyframe"] += n2
            pts = svo.getSemiDensePoints(world=True, fused=True, min_obs=2)
            wx, ws, wp = TR.map_points(want["map"]["invd"], want["map"]["sigma"], want["map"]["n_obs"], K, chain.T[k], 2)
            assert len(pts["xyz"]) == n2 and np.array_equal(pts["xyz"].view(np.uint32), wx.view(np.uint32)) and np.array_equal(pts["pixel"], wp)

    infos_got, tracks = _run(vo, stream, mode, dict(prm, every="keyframe", temporal=dict(TPRM), propagate=dict(PPRM)), check)
    assert infos_got == plain_runs[mode][0] and tracks == plain_runs[mode][1]
    assert seen["looked"]
    if mode != "sequence":  # (runSequence is looked at after its last frame only)
        assert len(set(seen["looked"])) >= 2 and seen["propagated"] > 1000 and seen["twice_at_keyframe"] > 1000, seen
    else:
        assert chain.state(N_FRAMES - 1)["from_id"] >= 0  # (the last map has a predecessor: the propagation ran inside runSequence)


def test_driver_mask_follows_the_keyframe_and_the_option_off_and_on(vo, stream):
    """Mask A from the start, mask B from frame 3 on: a keyframe's static result, the propagation's targets and the temporal search's
    key pixels take the mask that keyframe's pair carried. Then the option is switched off and on again between two frames: the
    next keyframe seeds plainly — once; the one after it propagates again."""
    st, imgs, prm = stream
    n = 24  # (at most: the loop ends with the keyframe that propagates again; frames past the stream's are rendered when reached)
    imgs, poses = list(imgs), st.poses(n)
    A = np.ones((SH, SW), np.uint8)  # (small regions: the odometry keeps its keyframe rhythm)
    A[40:200, 150:230] = 0
    A[220:, :] = 0
    B = np.ones((SH, SW), np.uint8)
    B[60:200, 400:480] = 0
    masks = [A if k < 3 else B for k in range(n)]
    c, svo = _driver(vo, st, dict(prm, every="keyframe", temporal=dict(TPRM), propagate=dict(PPRM)))
    try:
        infos, plain, toggled_at, checked = [], set(), None, {"B": 0, "plain": 0, "again": 0}
        chain = None
        for k in range(n):
            if k >= len(imgs):
                imgs.append(st.render_pair(poses[k])[:2])
            svo.setMask(masks[k])
            gi = svo.trackStereoImages(*imgs[k])
            infos.append(vo._capi.SvoFrameInfo.from_buffer_copy(bytes(gi)))
            if infos[k].is_keyframe and toggled_at is not None and not plain:
                plain.add(k)  # the first keyframe after the option came back
            chain = Chain(imgs, prm, infos, masks, plain) if chain is None else chain
            chain.infos, chain.plain = infos, plain
            chain.T = [np.array(i.T_wc, F).reshape(4, 4) for i in infos]
            if not infos[k].is_keyframe:
                continue
            want = chain.state(k)
            _same_state(svo, want, infos, k)
            if k in plain:
                assert want["from_id"] == -1 and (want["origin"] <= 1).all() and (want["map"]["n_obs"] <= 1).all()
                checked["plain"] += 1
            elif want["from_id"] >= 0 and k >= 3:
                assert (want["origin"][B == 0] == 0).all() and (want["origin"] >= 2).sum() > 1000
                checked["again" if plain else "B"] += 1
                if toggled_at is None:
                    svo.setSemiDensePropagate(None)
                    with pytest.raises(vo.VoError):
                        svo.getSemiDenseOrigin()
                    svo.setSemiDensePropagate(dict(PPRM))
                    assert svo.getSemiDenseOrigin() is None  # (no keyframe since the option came back)
                    toggled_at = k
            if checked["again"]:
                break
        assert checked["B"] >= 1 and checked["plain"] == 1 and checked["again"] >= 1, (checked, [i.is_keyframe for i in infos])
    finally:
        svo.close()
        c.close()


def test_driver_errors_and_allocations(vo, stream):
    st, imgs, prm = stream
    c, svo = _driver(vo, st)

    def count(ctx_):
        n = C.c_longlong()
        ctx_.check(ctx_.lib.vo_debug_allocation_count(ctx_.handle, C.byref(n)))
        return n.value
    try:
        svo.setSemiDense(dict(prm))
        with pytest.raises(vo.VoError) as e:  # needs the temporal option
            svo.setSemiDensePropagate({})
        assert e.value.code == -1
        svo.setSemiDenseTemporal(dict(TPRM))
        with pytest.raises(vo.VoError):  # the option is off
            svo.getSemiDenseOrigin()
        with pytest.raises(vo.VoError):
            svo.setSemiDensePropagate(dict(min_obs=0))
        with pytest.raises(ValueError):
            svo.setSemiDensePropagate(dict(bf=1.0))
        n0 = count(c)
        svo.setSemiDensePropagate({})
        assert count(c) == n0 + 1  # the option's only allocation
        assert svo.getSemiDenseOrigin() is None  # no keyframe yet
        svo.enqueue(*imgs[0])
        for call in (lambda: svo.setSemiDensePropagate(None), lambda: svo.setSemiDensePropagate({}), svo.getSemiDenseOrigin):  # in flight
            with pytest.raises(vo.VoError) as e:
                call()
            assert e.value.code == -1
        svo.result()
        svo.trackStereoImages(*imgs[1])  # (the first keyframe: seeded without a predecessor)
        origin, from_id = svo.getSemiDenseOrigin()
        r = svo.getSemiDenseMap()
        assert from_id == -1 and set(np.unique(origin).tolist()) == {0, 1} and np.array_equal(origin == 1, r.n_obs == 1)
        n1 = count(c)
        svo.setSemiDensePropagate(dict(PPRM))  # (a second enable allocates nothing, and keeps the chain)
        assert count(c) == n1 and svo.getSemiDenseOrigin()[1] == -1
    finally:
        svo.close()
        c.close()
