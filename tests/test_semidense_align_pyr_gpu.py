"""The coarse-to-fine alignment on a map pyramid on the device (include/vo_hip.h, "Semi-dense alignment on a map pyramid"; DESIGN.md
§21) against the numpy restatement (tests/semidense_align_pyr_restatement.py), every field and every plane bit for bit: the map
pyramid and the operator on the emulation test's crops — host planes and device planes, each twice in a row —, levels = 1 against
vo_semidense_align, the refusals; and StereoVO's option through the look-ahead calls, the synchronous call and runSequence, with
start="odometry" and start="previous": the odometry, the static result and the map the same bits as without it, every frame's
getSemiDenseAlign() the restatement applied to the keyframe's levels, the frame's levels, the map as it stood before the frame's
temporal launch and the start the rule gives (for "previous" the restatement's own results are chained); with "previous" every
aligned T_wc within PREVIOUS_BOUND of the odometry's; the option off and on again, its one round of allocations. None of the entry
points exists without the feature."""
import ctypes as C

import numpy as np
import pytest

import semidense_align_pyr_restatement as PR
import semidense_align_restatement as AR
import semidense_temporal_restatement as TR
from test_semidense_align import distance
from test_semidense_align_emu import same_result, synthetic_setup
from test_semidense_align_gpu import MAP, _same_record
from test_semidense_align_pyr_emu import CASES, case_inputs, same_levels, same_maps
from test_semidense_temporal_gpu import K, N_FRAMES, TPRM, _driver
from util import DeviceBuffer

pytestmark = pytest.mark.gpu

F = np.float32
I4 = np.eye(4, dtype=F)
APRM = dict(huber=8.0, max_iters=6, levels=4, max_iters_level=(4, 0, 0, 8))  # (not the defaults: the driver must carry the caller's)
STATIC = ("disparity", "score", "sigma_invd", "status")
# start="previous": the largest distance of an aligned T_wc to the odometry's T_wc over the stream's non-keyframe frames, measured
# with the restatement chain on the CPU (6.18 mm, 0.0189 degrees over the six frames 2, 3, 4, 5, 8, 9; the starts lie
# 500 mm from the odometry's pose), with the project's margin of a quarter
PREVIOUS_BOUND = (1.25 * 6.18, 1.25 * 0.0189)


@pytest.fixture(scope="module")
def frames():
    return synthetic_setup()


@pytest.fixture(scope="module")
def pyr_down(oracle):
    return oracle.pyr_down


@pytest.fixture(scope="module")
def pyr_ctx(vo):
    c = vo.Context(device=0, max_width=203, max_height=61, max_points=256, n_slots=2, max_level=2)
    yield c
    c.close()


def _fields(r):
    d = r._asdict()
    d["H"] = np.array([r.H[i, j] for i, j in AR.PAIRS])
    d["levels"] = [lv._asdict() for lv in r.levels]
    return d


def _download(buf, n, dtype):
    out = np.zeros(n, dtype)
    assert buf.hip.hipMemcpy(out.ctypes.data_as(C.c_void_p), buf.ptr, C.c_size_t(out.nbytes), 2) == 0  # D2H
    return out


# ---- 1. the operators ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(CASES))
def test_operators_equal_restatement(vo, pyr_ctx, frames, pyr_down, name):
    ctx = pyr_ctx
    key, cur, Kc, T, m, prm, _ = case_inputs(frames, pyr_down, name)
    L = prm["levels"]
    h, w = key[0].shape
    ctx.set_image(0, key[0])
    ctx.set_image(1, cur[0])
    want_maps = PR.map_pyramid(m, L)
    want = PR.align_pyr(key, cur, Kc, T, m, **prm)
    n = sum(x["invd"].size for x in want_maps[1:])
    bufs = {k: DeviceBuffer(np.ascontiguousarray(m[k])) for k in ("invd", "sigma", "n_obs")}
    outs = {k: DeviceBuffer(np.full(n, 0xEE, np.uint8).repeat(1 if k == "n_obs" else 4)) for k in ("invd", "sigma", "n_obs")}
    try:
        for rep in range(2):
            ok, where = same_maps(ctx.semiDenseMapPyramid(m, L), want_maps)
            assert ok, (name, rep, where)
            ctx.semiDenseMapPyramid({k: b.data_ptr() for k, b in bufs.items()}, L, on_device=(w, h), out={k: b.data_ptr() for k, b in outs.items()})
            flat = {k: _download(outs[k], n, np.uint8 if k == "n_obs" else F) for k in outs}
            off, dev = 0, [None]
            for x in want_maps[1:]:
                dev.append({k: flat[k][off:off + x["invd"].size].reshape(x["invd"].shape) for k in flat})
                off += x["invd"].size
            ok, where = same_maps(dev, want_maps)
            assert ok, (name, rep, "device planes", where)
            got = ctx.semiDenseAlignPyramid(0, 1, Kc, T, m, **prm)
            on_dev = ctx.semiDenseAlignPyramid(0, 1, Kc, T, {k: b.data_ptr() for k, b in bufs.items()}, map_on_device=True, **prm)
            for g in (got, on_dev):
                d = _fields(g)
                ok, where = same_result(d, want)
                assert ok, (name, rep, where)
                ok, where = same_levels(d["levels"], want["levels"])
                assert ok, (name, rep, where)
                assert g.T_wc is None and g.frame_id is None and g.start is None and len(g.levels) == L
    finally:
        for b in list(bufs.values()) + list(outs.values()):
            b.free()


def test_one_level_equals_the_level_0_operator(vo, pyr_ctx, frames, pyr_down):
    ctx = pyr_ctx
    key, cur, Kc, T, m, prm, _ = case_inputs(frames, pyr_down, "203x61_3_levels")
    ctx.set_image(0, key[0])
    ctx.set_image(1, cur[0])
    p0 = {k: v for k, v in prm.items() if k != "levels"}
    a = ctx.semiDenseAlign(key[0], 1, Kc, T, m, **p0)
    b = ctx.semiDenseAlignPyramid(0, 1, Kc, T, m, levels=1, **p0)
    for f in ("T_ck", "H", "b"):
        assert np.array_equal(getattr(a, f).view(np.uint8), getattr(b, f).view(np.uint8)), f
    assert (a.status, a.iters, a.count) == (b.status, b.iters, b.count) and np.float64(a.rms).tobytes() == np.float64(b.rms).tobytes()
    assert b.levels == ((b.status, b.iters, b.count, b.rms),)


def test_operator_refusals(vo, pyr_ctx, frames, pyr_down):
    ctx = pyr_ctx
    key, cur, Kc, T, m, prm, _ = case_inputs(frames, pyr_down, "203x61_3_levels")
    ctx.set_image(0, key[0])
    ctx.set_image(1, cur[0])
    for bad in (dict(levels=0), dict(levels=7), dict(max_iters_level=(0, 33)), dict(max_iters_level=(-1,)), dict(min_obs=0), dict(huber=0.0),
                dict(max_iters=0), dict(max_iters=33), dict(eps=float("nan")), dict(min_pixels=5)):
        with pytest.raises(vo.VoError) as e:
            ctx.semiDenseAlignPyramid(0, 1, Kc, T, m, **dict(prm, **bad))
        assert e.value.code == -1, bad
    with pytest.raises(vo.VoError) as e:  # the slots hold levels 0..2
        ctx.semiDenseAlignPyramid(0, 1, Kc, T, m, **dict(prm, levels=4))
    assert e.value.code == -1
    with pytest.raises(vo.VoError):
        ctx.semiDenseAlignPyramid(0, 5, Kc, T, m, **prm)
    bad_T = T.copy()
    bad_T[1, 3] = np.inf
    with pytest.raises(vo.VoError):
        ctx.semiDenseAlignPyramid(0, 1, Kc, bad_T, m, **prm)
    with pytest.raises(ValueError):
        ctx.semiDenseAlignPyramid(0, 1, Kc, T, {k: v[:, :50] for k, v in m.items()}, **prm)
    with pytest.raises(vo.VoError):
        ctx.semiDenseMapPyramid(m, 1)
    with pytest.raises(vo.VoError):
        ctx.semiDenseMapPyramid(m, 7)
    with pytest.raises(vo.VoError):  # beyond vo_config.max_width
        ctx.semiDenseMapPyramid(TR.empty_map((61, 204)), 2)
    # a level below 3 pixels a side: VO_ERR_SIZE
    small = np.ascontiguousarray(key[0][:5, :40])  # (levels 40 x 5, 20 x 3, 10 x 2)
    ctx.set_image(0, small)
    ctx.set_image(1, small)
    with pytest.raises(vo.VoError) as e:
        ctx.semiDenseAlignPyramid(0, 1, Kc, T, TR.empty_map(small.shape), levels=3)
    assert e.value.code == -4  # VO_ERR_SIZE
    # an empty map: status 2 at every level, the pose is the start
    ctx.set_image(0, key[0])
    ctx.set_image(1, cur[0])
    r = ctx.semiDenseAlignPyramid(0, 1, Kc, T, TR.empty_map(key[0].shape), levels=3)
    assert r.levels == ((2, 1, 0, 0.0),) * 3 and r.status == 2 and np.array_equal(r.T_ck[:3], T[:3]) and not r.H.any()


# ---- 2. the driver --------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def stream():
    from visual_odometry_ros_amd import synthetic as S
    st = S.StereoStream(width=640, height=240, K=K, n_u=20, n_v=8, seed=2, speed=0.5)
    imgs = [st.render_pair(p)[:2] for p in st.poses(N_FRAMES)]
    bf = float(F(K[0] * st.baseline))
    return st, imgs, dict(bf=bf, d_min=0, d_max=67)


def _run(vo, stream, mode, align, look=None):
    """one run of N_FRAMES frames with the static and the temporal option on: per frame (runSequence: the last frame only) the frame
    info's bytes, the map's planes and the static result's as bytes; the final track set; look(k, svo) after a frame's record"""
    st, imgs, prm = stream
    c, svo = _driver(vo, st, dict(prm, every="keyframe", temporal=dict(TPRM), **({"align": dict(align)} if align else {})))
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
    return {mode: _run(vo, stream, mode, None) for mode in ("lookahead", "sync", "sequence")}


@pytest.fixture(scope="module")
def expected(vo, stream, base_runs, pyr_down):
    """per start, per frame: None (a keyframe frame, or no keyframe map yet) or the restatement's result with kf, start and T_wc — from
    the synchronous run's poses and maps, the restatement's own results chained for "previous" (computed once)"""
    _, imgs, _ = stream
    infos, _, per_frame = base_runs["sync"]
    info = [vo._capi.SvoFrameInfo.from_buffer_copy(b) for b in infos]
    T_wc = [np.array(i.T_wc, F).reshape(4, 4) for i in info]
    levels = [PR.image_pyramid(L, APRM["levels"], pyr_down) for L, _ in imgs]
    out = {}
    for start in ("odometry", "previous"):
        chain = []
        for k in range(N_FRAMES):
            kfs = [j for j in range(k + 1) if info[j].is_keyframe and j > 0]  # (the first frame seeds no map)
            if info[k].is_keyframe or not kfs:
                chain.append(None)
                continue
            kf = kfs[-1]
            T0, used = TR.pose_ck(T_wc[k], T_wc[kf]), "odometry"
            if start == "previous":
                if k == kf + 1:
                    T0 = I4
                elif chain[k - 1] is not None and chain[k - 1]["kf"] == kf and chain[k - 1]["status"] in (0, 1):
                    T0, used = chain[k - 1]["T_ck"], "previous"
            before = per_frame[k - 1]["map"]  # the map as it stood before this frame's temporal launch
            want = PR.align_pyr(levels[kf], levels[k], K, T0, before, **APRM)
            T_kc = TR.pose_ck(want["T_ck"], I4)  # inverseSE3(T_ck) in the driver's order
            want.update(kf=kf, start=used, T_wc=AR.mul44(T_wc[kf], T_kc), from_odometry=distance(AR.mul44(T_wc[kf], T_kc), T_wc[k]),
                        start_off=distance(T0, TR.pose_ck(T_wc[k], T_wc[kf])))
            chain.append(want)
        out[start] = chain
        far = [w["from_odometry"] for w in chain if w is not None]
        print(f"start={start}: the aligned T_wc lies at most {max(t for t, _ in far):.3f} mm, {max(r for _, r in far):.4f} degrees from the odometry's "
              f"over {len(far)} frames: {[(round(t, 3), round(r, 4)) for t, r in far]}")
    return info, out


@pytest.mark.parametrize("start", ["odometry", "previous"])
@pytest.mark.parametrize("mode", ["lookahead", "sync", "sequence"])
def test_driver(vo, stream, base_runs, expected, mode, start):
    infos_off, tracks_off, rec_off = base_runs[mode]
    assert base_runs["sync"][0] == infos_off
    info, chains = expected
    chain = chains[start]
    seen = dict(aligned=0, none=0, previous=0, identity=0)

    def look(k, svo):
        r = svo.getSemiDenseAlign()
        want = chain[k]
        if want is None:  # a keyframe frame, or no keyframe map yet: no result, said with a status of its own
            assert (r.status, r.key_frame_id, r.iters, r.count) == (4, -1, 0, 0) and r.frame_id == info[k].frame_id, k
            assert np.array_equal(r.T_ck, I4) and np.array_equal(r.T_wc, I4) and not r.H.any()
            assert r.levels == ((4, 0, 0, 0.0),) * APRM["levels"]
            seen["none"] += 1
            return
        d = _fields(r)
        ok, where = same_result(d, want)
        assert ok, (k, want["kf"], where)
        ok, where = same_levels(d["levels"], want["levels"])
        assert ok, (k, where)
        assert (r.frame_id, r.key_frame_id, r.start) == (info[k].frame_id, info[want["kf"]].frame_id, want["start"]), k
        assert np.array_equal(r.T_wc.view(np.uint32), want["T_wc"].view(np.uint32)), k
        t, rot = want["from_odometry"]
        print(f"{mode} {start} frame {k} (keyframe {want['kf']}): start {want['start']}, {want['start_off'][0]:.1f} mm / {want['start_off'][1]:.4f} degrees "
              f"from the odometry's; levels (0 first) {[(x['status'], x['iters'], x['count']) for x in want['levels']]}; the aligned T_wc lies "
              f"{t:.3f} mm, {rot:.4f} degrees from the odometry's")
        assert want["status"] in (0, 1) and want["count"] > 5000 and 0 < want["rms"] < 20, (k, want["status"], want["count"], want["rms"])
        if start == "previous":
            assert t <= PREVIOUS_BOUND[0] and rot <= PREVIOUS_BOUND[1], (k, t, rot)
        seen["aligned"] += 1
        seen["previous"] += want["start"] == "previous"
        seen["identity"] += start == "previous" and k == want["kf"] + 1

    infos_on, tracks_on, rec_on = _run(vo, stream, mode, dict(APRM, start=start), look)
    assert infos_on == infos_off and tracks_on == tracks_off  # the odometry: the same bits
    assert sorted(rec_on) == sorted(rec_off)
    for k in rec_on:
        _same_record(rec_on[k], rec_off[k], k)  # the static result and the map: the same bits
    if mode == "sequence":
        assert seen["aligned"] + seen["none"] == 1
    else:
        assert seen["aligned"] >= 3 and seen["none"] >= 2, seen
        if start == "previous":  # the chain ran: a start at the identity, one or more hundred millimetres off, and a start on the previous pose
            assert seen["identity"] >= 1 and seen["previous"] >= 1, seen
            assert max(w["start_off"][0] for w in chain if w is not None) > 100.0
        else:
            assert seen["previous"] == 0


def test_driver_option_lifecycle(vo, stream, pyr_down):
    st, imgs, prm = stream
    c, svo = _driver(vo, st)

    def count(ctx_):
        n = C.c_longlong()
        ctx_.check(ctx_.lib.vo_debug_allocation_count(ctx_.handle, C.byref(n)))
        return n.value
    try:
        assert not hasattr(vo.MonoVO, "setSemiDenseAlignPyramid")  # a stereo driver's option (the C call refuses a mono driver's core)
        svo.setSemiDense(dict(prm))
        with pytest.raises(vo.VoError) as e:  # needs the temporal option
            svo.setSemiDenseAlignPyramid({})
        assert e.value.code == -1
        svo.setSemiDenseTemporal(dict(TPRM))
        with pytest.raises(vo.VoError):  # the option is off
            svo.getSemiDenseAlign()
        for bad in (dict(levels=0), dict(levels=7), dict(max_iters_level=(40,)), dict(max_iters=0)):
            with pytest.raises(vo.VoError):
                svo.setSemiDenseAlignPyramid(bad)
        for bad in (dict(bf=1.0), dict(start="keyframe")):
            with pytest.raises(ValueError):
                svo.setSemiDenseAlignPyramid(bad)
        n0 = count(c)
        svo.setSemiDenseAlign(dict(APRM, start="previous"))  # (a dict that names levels or start: the coarse-to-fine option)
        assert count(c) == n0 + 2  # the state block; the key levels with the map pyramid's planes
        assert svo.getSemiDenseAlign().status == 4  # no frame yet
        svo.enqueue(*imgs[0])
        for call in (lambda: svo.setSemiDenseAlignPyramid(None), lambda: svo.setSemiDenseAlignPyramid({}), svo.getSemiDenseAlign):  # in flight
            with pytest.raises(vo.VoError) as e:
                call()
            assert e.value.code == -1
        svo.result()
        infos = [None, svo.trackStereoImages(*imgs[1])]  # (the first keyframe)
        assert infos[1].is_keyframe and svo.getSemiDenseAlign().status == 4
        infos.append(svo.trackStereoImages(*imgs[2]))
        assert not infos[2].is_keyframe
        a2 = svo.getSemiDenseAlign()
        assert a2.status in (0, 1) and a2.frame_id == infos[2].frame_id and a2.key_frame_id == infos[1].frame_id and a2.start == "odometry"
        assert len(a2.levels) == 4 and a2.levels[0][:3] == (a2.status, a2.iters, a2.count)
        # off: the getter refuses, the frames go on; on again: no allocation; the keyframe's levels were not kept in between, so there
        # is no result until the next keyframe
        svo.setSemiDenseAlignPyramid(None)
        with pytest.raises(vo.VoError):
            svo.getSemiDenseAlign()
        n1 = count(c)  # (the frames have made the driver's own allocations since)
        svo.setSemiDenseAlignPyramid(dict(APRM))
        assert count(c) == n1 and svo.getSemiDenseAlign().status == 4
        infos.append(svo.trackStereoImages(*imgs[3]))
        a3 = svo.getSemiDenseAlign()
        assert a3.status == 4 and a3.frame_id == infos[3].frame_id and count(c) == n1
        # the level-0 option in its place: no allocation (the state block is shared), and a result at the next frame
        svo.setSemiDenseAlign(dict(huber=8.0, max_iters=6))
        assert count(c) == n1
        infos.append(svo.trackStereoImages(*imgs[4]))
        a4 = svo.getSemiDenseAlign()
        if not infos[3].is_keyframe and not infos[4].is_keyframe:
            assert a4.status in (0, 1) and len(a4.levels) == 1 and a4.levels[0][:3] == (a4.status, a4.iters, a4.count)
        # the temporal option off: the alignment has nothing to read and its getter says so
        svo.setSemiDenseTemporal(None)
        with pytest.raises(vo.VoError):
            svo.getSemiDenseAlign()
    finally:
        svo.close()
        c.close()
