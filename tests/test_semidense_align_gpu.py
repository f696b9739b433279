"""The direct image alignment on the semi-dense map on the device (include/vo_hip.h, "Semi-dense alignment") against
the numpy restatement (tests/semidense_align_restatement.py), every field bit for bit: the operator on the emulation test's two
crops and its small maps — host planes, device planes with a padded key stride, each twice in a row (the second passes only if the
first left the ticket at zero and overwrote the "done" word), and max_iters = 1, where the 27 sums stand alone — and StereoVO's
option through the look-ahead calls, the synchronous call and runSequence: the odometry, the static result and the map the same
bits as without it, every frame's getSemiDenseAlign() the restatement applied to the key plane, the frame's left image, the map as
it stood before the frame's temporal launch and the returned poses; status 4 at keyframe frames; the option off and on again, the
refusals, its one allocation. None of the entry points exists without the feature."""
import ctypes as C

import numpy as np
import pytest

import semidense_align_restatement as AR
import semidense_temporal_restatement as TR
from test_semidense_align_emu import CASES, case_inputs, same_result, synthetic_setup
from test_semidense_temporal_gpu import K, N_FRAMES, TPRM, _driver
from util import DeviceBuffer

pytestmark = pytest.mark.gpu

F = np.float32
APRM = dict(huber=8.0, max_iters=6)  # (not the defaults: the driver must carry the caller's)
OP_CASES = ("203x61_forward_epipole", "97x45_sideways", "min_obs_2", "most_leave", "31x29_one_block", "64x32_whole_blocks")


@pytest.fixture(scope="module")
def frames():
    return synthetic_setup()


@pytest.fixture(scope="module")
def sda_ctx(vo):
    c = vo.Context(device=0, max_width=203, max_height=61, max_points=256, n_slots=2, max_level=0)
    yield c
    c.close()


# ---- 1. the operator ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", OP_CASES)
def test_operator_equals_restatement(vo, sda_ctx, frames, name):
    ctx = sda_ctx
    key, cur, Kc, T, m, prm, _ = case_inputs(frames, name)
    h, w = key.shape
    ctx.set_image(0, cur)
    padded = np.full((h, w + 5), 0xEE, np.uint8)  # the key plane on the device, with a padded stride
    padded[:, :w] = key
    bufs = {k: DeviceBuffer(np.ascontiguousarray(m[k])) for k in ("invd", "sigma", "n_obs")}
    dkey = DeviceBuffer(padded)
    try:
        for p in (dict(prm, max_iters=1), dict(prm)):
            want = AR.align(key, cur, Kc, T, m, **p)
            for rep in range(2):
                got = ctx.semiDenseAlign(key, 0, Kc, T, m, **p)
                dev = ctx.semiDenseAlign(dkey.data_ptr(), 0, Kc, T, {k: b.data_ptr() for k, b in bufs.items()}, key_on_device=w + 5,
                                         map_on_device=True, **p)
                for g in (got, dev):
                    d = g._asdict()
                    d["H"] = np.array([d["H"][i, j] for i, j in AR.PAIRS])
                    if p.get("max_iters") == 1:  # one iteration: the 27 sums on their own
                        assert np.array_equal(d["H"].view(np.uint64), want["H"].view(np.uint64)), (name, rep)
                        assert np.array_equal(d["b"].view(np.uint64), want["b"].view(np.uint64)), (name, rep)
                    ok, where = same_result(d, want)
                    assert ok, (name, p, rep, where)
                    assert np.array_equal(g.H, g.H.T) and g.T_wc is None and g.frame_id is None
    finally:
        dkey.free()
        for b in bufs.values():
            b.free()


def test_operator_argument_errors(vo, sda_ctx, frames):
    ctx = sda_ctx
    key, cur, Kc, T, m, prm, _ = case_inputs(frames, "97x45_sideways")
    ctx.set_image(0, cur)
    for bad in (dict(min_obs=0), dict(min_obs=256), dict(huber=0.0), dict(huber=float("nan")), dict(huber=256.0), dict(max_iters=0),
                dict(max_iters=33), dict(eps=-1.0), dict(eps=float("nan")), dict(eps=float("inf")), dict(min_pixels=5)):
        with pytest.raises(vo.VoError) as e:
            ctx.semiDenseAlign(key, 0, Kc, T, m, **dict(prm, **bad))
        assert e.value.code == -1, bad
    with pytest.raises(vo.VoError):
        ctx.semiDenseAlign(key, 5, Kc, T, m, **prm)
    bad_T = T.copy()
    bad_T[0, 3] = np.nan
    with pytest.raises(vo.VoError):
        ctx.semiDenseAlign(key, 0, Kc, bad_T, m, **prm)
    with pytest.raises(vo.VoError):
        ctx.semiDenseAlign(key, 0, (0.0, Kc[1], Kc[2], Kc[3]), T, m, **prm)
    with pytest.raises(ValueError):
        ctx.semiDenseAlign(key, 0, Kc, T, {k: v[:, :50] for k, v in m.items()}, **prm)  # (another size)
    with pytest.raises(ValueError):
        ctx.semiDenseAlign(key, 0, Kc, T, m, max_search=64)
    # an empty map: status 2, the pose is the start
    empty = TR.empty_map(key.shape)
    r = ctx.semiDenseAlign(key, 0, Kc, T, empty)
    assert (r.status, r.iters, r.count, r.rms) == (2, 1, 0, 0.0) and np.array_equal(r.T_ck[:3], T[:3]) and not r.H.any()


# ---- 2. the driver --------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def stream():
    from visual_odometry_ros_amd import synthetic as S
    st = S.StereoStream(width=640, height=240, K=K, n_u=20, n_v=8, seed=2, speed=0.5)
    imgs = [st.render_pair(p)[:2] for p in st.poses(N_FRAMES)]
    bf = float(F(K[0] * st.baseline))
    return st, imgs, dict(bf=bf, d_min=0, d_max=67)


MAP = ("invd", "sigma", "n_obs", "tstatus")
STATIC = ("disparity", "score", "sigma_invd", "status")


def _run(vo, stream, mode, align, look=None):
    """one run of N_FRAMES frames with the static and the temporal option on: per frame (runSequence: the last frame only) the frame
    info's bytes, the map's planes and the static result's as bytes; the final track set; look(k, svo) after a frame's record"""
    st, imgs, prm = stream
    c, svo = _driver(vo, st, dict(prm, every="keyframe", temporal=dict(TPRM), **({"align": dict(APRM)} if align else {})))
    rec = {}

    def record(k):
        m, s = svo.getSemiDenseMap(), svo.getSemiDense()
        rec[k] = dict(map=None if m is None else {p: getattr(m, p).copy() for p in MAP}, map_id=None if m is None else (m.frame_id, m.n_fused),
                      static=None if s is None else (s.frame_id, b"".join(getattr(s, p).tobytes() for p in STATIC)))
        if look:
            look(k, svo)
    try:
        if mode == "sequence":
            got, _ = svo.runSequence([(L, R) for L, R in imgs])
            infos = [bytes(i) for i in got]
            record(N_FRAMES - 1)
        else:
            infos = []
            for k in range(N_FRAMES):
                if mode == "lookahead":
                    svo.enqueue(*imgs[k])
                    if k + 1 < N_FRAMES:
                        svo.prefetch(*imgs[k + 1])
                    gi = svo.result()
                else:
                    gi = svo.trackStereoImages(*imgs[k])
                infos.append(bytes(gi))
                record(k)
        tracks = {k: v.tobytes() for k, v in svo.getTracks().items()}
        return infos, tracks, rec
    finally:
        svo.close()
        c.close()


@pytest.fixture(scope="module")
def base_runs(vo, stream):
    """the runs with the alignment off, per calling mode (computed once)"""
    return {mode: _run(vo, stream, mode, False) for mode in ("lookahead", "sync", "sequence")}


def _same_record(a, b, k):
    assert a["map_id"] == b["map_id"] and a["static"] == b["static"], k
    if a["map"] is not None:
        for p in MAP:
            assert np.array_equal(a["map"][p].view(np.uint8), b["map"][p].view(np.uint8)), (k, p)


@pytest.mark.parametrize("mode", ["lookahead", "sync", "sequence"])
def test_driver(vo, stream, base_runs, mode):
    _, imgs, _ = stream
    infos_off, tracks_off, rec_off = base_runs[mode]
    per_frame = base_runs["sync"][2]  # (runSequence is looked at after its last frame only: the maps in between are the synchronous run's)
    assert base_runs["sync"][0] == infos_off
    info = [vo._capi.SvoFrameInfo.from_buffer_copy(b) for b in infos_off]
    T_wc = [np.array(i.T_wc, F).reshape(4, 4) for i in info]
    seen = dict(aligned=0, none=0, closer=0)

    def look(k, svo):
        r = svo.getSemiDenseAlign()
        kfs = [j for j in range(k + 1) if info[j].is_keyframe and j > 0]  # (the first frame seeds no map)
        if info[k].is_keyframe or not kfs:  # a keyframe frame, or no keyframe map yet: no result, said with a status of its own
            assert (r.status, r.key_frame_id, r.iters, r.count) == (4, -1, 0, 0) and r.frame_id == info[k].frame_id, k
            assert np.array_equal(r.T_ck, np.eye(4, dtype=F)) and np.array_equal(r.T_wc, np.eye(4, dtype=F)) and not r.H.any()
            seen["none"] += 1
            return
        kf = kfs[-1]
        before = per_frame[k - 1]["map"]  # the map as it stood before this frame's temporal launch
        T0 = TR.pose_ck(T_wc[k], T_wc[kf])
        want = AR.align(imgs[kf][0], imgs[k][0], K, T0, before, **APRM)
        d = r._asdict()
        d["H"] = np.array([r.H[i, j] for i, j in AR.PAIRS])
        ok, where = same_result(d, want)
        assert ok, (k, kf, where)
        assert (r.frame_id, r.key_frame_id) == (info[k].frame_id, info[kf].frame_id), k
        T_kc = TR.pose_ck(want["T_ck"], np.eye(4, dtype=F))  # inverseSE3(T_ck) in the driver's order
        assert np.array_equal(r.T_wc.view(np.uint32), AR.mul44(T_wc[kf], T_kc).view(np.uint32)), k
        assert want["status"] in (0, 1) and want["count"] > 5000 and 0 < want["rms"] < 20, (k, want["status"], want["count"], want["rms"])
        seen["aligned"] += 1
        # the aligned pose stays next to the odometry's (a health check, not a bound on either): centimetres, a fraction of a degree
        E = np.linalg.inv(T0.astype(np.float64)) @ want["T_ck"].astype(np.float64)
        seen["closer"] += int(np.linalg.norm(E[:3, 3]) < 0.05 and np.linalg.norm(E[:3, :3] - np.eye(3)) < 0.01)

    infos_on, tracks_on, rec_on = _run(vo, stream, mode, True, look)
    assert infos_on == infos_off and tracks_on == tracks_off  # the odometry: the same bits
    assert sorted(rec_on) == sorted(rec_off)
    for k in rec_on:
        _same_record(rec_on[k], rec_off[k], k)  # the static result and the map: the same bits
    if mode == "sequence":
        assert seen["aligned"] + seen["none"] == 1
    else:
        assert seen["aligned"] >= 3 and seen["none"] >= 2 and seen["closer"] == seen["aligned"], seen


def test_driver_option_lifecycle(vo, stream):
    st, imgs, prm = stream
    c, svo = _driver(vo, st)

    def count(ctx_):
        n = C.c_longlong()
        ctx_.check(ctx_.lib.vo_debug_allocation_count(ctx_.handle, C.byref(n)))
        return n.value
    try:
        assert not hasattr(vo.MonoVO, "setSemiDenseAlign")  # a stereo driver's option (the C call refuses a mono driver's core)
        svo.setSemiDense(dict(prm))
        with pytest.raises(vo.VoError) as e:  # needs the temporal option
            svo.setSemiDenseAlign({})
        assert e.value.code == -1
        svo.setSemiDenseTemporal(dict(TPRM))
        with pytest.raises(vo.VoError):  # the option is off
            svo.getSemiDenseAlign()
        with pytest.raises(vo.VoError):
            svo.setSemiDenseAlign(dict(max_iters=0))
        with pytest.raises(ValueError):
            svo.setSemiDenseAlign(dict(bf=1.0))
        n0 = count(c)
        svo.setSemiDenseAlign(dict(APRM))
        assert count(c) == n0 + 1  # the option's only allocation
        assert svo.getSemiDenseAlign().status == 4  # no frame yet
        svo.enqueue(*imgs[0])
        for call in (lambda: svo.setSemiDenseAlign(None), lambda: svo.setSemiDenseAlign({}), svo.getSemiDenseAlign):  # in flight
            with pytest.raises(vo.VoError) as e:
                call()
            assert e.value.code == -1
        svo.result()
        infos = [None, svo.trackStereoImages(*imgs[1])]  # (the first keyframe)
        assert infos[1].is_keyframe and svo.getSemiDenseAlign().status == 4
        infos.append(svo.trackStereoImages(*imgs[2]))
        assert not infos[2].is_keyframe
        m1 = svo.getSemiDenseMap()
        a2 = svo.getSemiDenseAlign()
        assert a2.status in (0, 1) and a2.frame_id == infos[2].frame_id and a2.key_frame_id == infos[1].frame_id
        # off: the getter refuses, the frames go on; on again: no allocation, no result until the next frame, which then has one
        svo.setSemiDenseAlign(None)
        with pytest.raises(vo.VoError):
            svo.getSemiDenseAlign()
        n1 = count(c)
        svo.setSemiDenseAlign(dict(APRM))
        assert count(c) == n1 and svo.getSemiDenseAlign().status == 4
        infos.append(svo.trackStereoImages(*imgs[3]))
        a3 = svo.getSemiDenseAlign()
        if infos[3].is_keyframe:
            assert a3.status == 4
        else:
            T = lambda i: np.array(i.T_wc, F).reshape(4, 4)
            want = AR.align(imgs[1][0], imgs[3][0], K, TR.pose_ck(T(infos[3]), T(infos[1])), {p: getattr(m1, p) for p in ("invd", "sigma", "n_obs")},
                            **APRM)
            d = a3._asdict()
            d["H"] = np.array([a3.H[i, j] for i, j in AR.PAIRS])
            ok, where = same_result(d, want)
            assert ok, where
        # the temporal option off: the alignment has nothing to read and its getter says so
        svo.setSemiDenseTemporal(None)
        with pytest.raises(vo.VoError):
            svo.getSemiDenseAlign()
    finally:
        svo.close()
        c.close()
