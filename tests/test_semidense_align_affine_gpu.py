"""The alignment with affine brightness on the device (include/vo_hip.h, "Semi-dense alignment with affine brightness")
against the numpy restatement (tests/semidense_align_affine_restatement.py), every field bit for bit: vo_semidense_align_pyr_affine on
the emulation test's cases (host planes and device planes, each twice in a row) and vo_semidense_align_affine on their level 0 (a host
key plane and a device key plane with a padded stride); one whole 640 x 240 image mapped by (0.7, +25), also held to the pose, gain
and offset bounds of tests/test_semidense_align_affine.py; the refusals. StereoVO's modifier on the 10-frame 640 x 240 stream of
tests/test_semidense_align_pyr_gpu.py with every second pair mapped by (0.85, +10), both images alike, through the look-ahead calls
and the synchronous call, for the level-0 option and for levels = 4, start = "previous" (gain0 = 0.95, offset0 = 2, so that a start
from the parameters shows): (a) frame infos, track sets, static result and map the same bits as with the modifier off; (b) every
frame's result the restatement on the keyframe's and the frame's images, the map as it stood before the frame's temporal launch and
the start the rule gives, G and O taken over from the previous frame exactly when the pose is; (c) status 4 at a keyframe frame, the
frame behind it starting from G0, O0; (d) off, on, off between frames: the frames with it off return what a run that never had it on
returns. Quality: over the modified frames the aligned pose lies closer to the odometry's with the modifier than without (the
figures are printed; DESIGN.md §22 records them). None of the entry points exists without the feature."""
import ctypes as C

import numpy as np
import pytest

import semidense_align_affine_restatement as FR
import semidense_align_pyr_restatement as PR
import semidense_align_restatement as AR
import semidense_temporal_restatement as TR
from test_semidense_align import distance
from test_semidense_align_affine import GAIN_BOUND, OFFSET_BOUND, POSE_BOUND_MM
from test_semidense_align_affine_emu import CASES, case_inputs, same_levels, same_result
from test_semidense_align_emu import XI_START, perturbed, synthetic_setup
from test_semidense_align_gpu import MAP, STATIC, _same_record
from test_semidense_temporal_gpu import K, N_FRAMES, TPRM, _driver
from util import DeviceBuffer

pytestmark = pytest.mark.gpu

F = np.float32
I4 = np.eye(4, dtype=F)
AFFINE = dict(gain0=0.95, offset0=2.0)
CONFIGS = {  # name -> the alignment option's parameters (not the defaults: the driver must carry the caller's)
    "level_0": dict(huber=8.0, max_iters=6),
    "pyr_previous": dict(huber=8.0, max_iters=6, levels=4, max_iters_level=(4, 0, 0, 8), start="previous"),
}
CHANGE = (0.85, 10)  # every second pair's exposure


@pytest.fixture(scope="module")
def frames():
    return synthetic_setup()


@pytest.fixture(scope="module")
def pyr_down(oracle):
    return oracle.pyr_down


@pytest.fixture(scope="module")
def crop_ctx(vo):
    c = vo.Context(device=0, max_width=203, max_height=61, max_points=256, n_slots=2, max_level=2)
    yield c
    c.close()


def _fields(r):
    d = r._asdict()
    d["H"] = np.array([r.H[i, j] for i, j in FR.PAIRS])
    d["levels"] = [lv._asdict() for lv in r.levels] if r.levels is not None else None
    return d


def _split(prm):
    """a case's parameters -> (the alignment's, the affine ones)"""
    p = dict(prm)
    return p, {k: p.pop(k) for k in ("gain0", "offset0") if k in p}


# ---- 1. the operators ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(CASES))
def test_operators_equal_restatement(vo, crop_ctx, frames, pyr_down, name):
    ctx = crop_ctx
    key, cur, Kc, T, m, prm, _ = case_inputs(frames, pyr_down, name)
    p, ap = _split(prm)
    L = p["levels"]
    h, w = key[0].shape
    ctx.set_image(0, key[0])
    ctx.set_image(1, cur[0])
    want = FR.align_pyr(key, cur, Kc, T, m, **prm)
    p0 = {k: v for k, v in p.items() if k != "levels"}
    want0 = FR.align(key[0], cur[0], Kc, T, m, **p0, **ap)
    padded = np.full((h, w + 5), 0xEE, np.uint8)  # the key plane on the device, with a padded stride
    padded[:, :w] = key[0]
    bufs = {k: DeviceBuffer(np.ascontiguousarray(m[k])) for k in ("invd", "sigma", "n_obs")}
    dkey = DeviceBuffer(padded)
    dev_map = {k: b.data_ptr() for k, b in bufs.items()}
    try:
        for rep in range(2):
            got = ctx.semiDenseAlignPyramid(0, 1, Kc, T, m, affine=ap or True, **p)
            on_dev = ctx.semiDenseAlignPyramid(0, 1, Kc, T, dev_map, map_on_device=True, affine=ap or True, **p)
            for g in (got, on_dev):
                d = _fields(g)
                ok, where = same_result(d, want)
                assert ok, (name, rep, where)
                ok, where = same_levels(d["levels"], want["levels"], pose=False)
                assert ok, (name, rep, where)
                assert (g.gain, g.offset) == (want["G"] / 65536.0, want["O"] / 16.0) and g.H.shape == (8, 8) and g.b.shape == (8,)
                assert g.T_wc is None and g.frame_id is None and g.start is None and len(g.levels) == L and np.array_equal(g.H, g.H.T)
            got = ctx.semiDenseAlign(key[0], 1, Kc, T, m, affine=ap or True, **p0)
            on_dev = ctx.semiDenseAlign(dkey.data_ptr(), 1, Kc, T, dev_map, key_on_device=w + 5, map_on_device=True, affine=ap or True, **p0)
            for g in (got, on_dev):
                ok, where = same_result(_fields(g), want0)
                assert ok, (name, rep, "level 0", where)
                assert g.levels is None and (g.gain, g.offset) == (want0["gain"], want0["offset"])
    finally:
        dkey.free()
        for b in bufs.values():
            b.free()


def test_whole_image_under_an_exposure_change(vo, frames):
    fr = frames
    cur = FR.map_image(fr["L"][3], 0.7, 25)
    T0 = perturbed(fr["T"][3], XI_START)
    c = vo.Context(device=0, max_width=640, max_height=240, max_points=256, n_slots=1, max_level=0)
    try:
        c.set_image(0, cur)
        got = c.semiDenseAlign(fr["L"][2], 0, K, T0, fr["map2"], affine=True, max_iters=20)
        plain = c.semiDenseAlign(fr["L"][2], 0, K, T0, fr["map2"], max_iters=20)
    finally:
        c.close()
    ok, where = same_result(_fields(got), FR.align(fr["L"][2], cur, K, T0, fr["map2"], max_iters=20))
    assert ok, where
    t, tp = distance(got.T_ck, fr["T"][3])[0], distance(plain.T_ck, fr["T"][3])[0]
    print(f"640 x 240, (0.7, +25): affine status {got.status} after {got.iters} iterations, rms {got.rms:.2f}, t = {t:.3f} mm, gain {got.gain:.4f}, "
          f"offset {got.offset:.2f}; plain status {plain.status}, rms {plain.rms:.2f}, t = {tp:.3f} mm")
    assert got.status in (0, 1) and t < POSE_BOUND_MM < tp
    assert abs(got.gain - 0.7) <= GAIN_BOUND and abs(got.offset - 25) <= OFFSET_BOUND


def test_operator_refusals(vo, crop_ctx, frames, pyr_down):
    ctx = crop_ctx
    key, cur, Kc, T, m, prm, _ = case_inputs(frames, pyr_down, "203x61_3_levels")
    ctx.set_image(0, key[0])
    ctx.set_image(1, cur[0])
    for bad in (dict(gain0=0.12), dict(gain0=8.5), dict(gain0=float("nan")), dict(offset0=255.5), dict(offset0=-256.0), dict(offset0=float("inf"))):
        for call in (lambda: ctx.semiDenseAlignPyramid(0, 1, Kc, T, m, affine=bad, **prm), lambda: ctx.semiDenseAlign(key[0], 1, Kc, T, m, affine=bad)):
            with pytest.raises(vo.VoError) as e:
                call()
            assert e.value.code == -1, bad
    for ok in (dict(gain0=0.125, offset0=-255.0), dict(gain0=8.0, offset0=255.0)):
        ctx.semiDenseAlign(key[0], 1, Kc, T, m, affine=ok, max_iters=1)
    with pytest.raises(vo.VoError):  # the alignment's own refusals stand
        ctx.semiDenseAlign(key[0], 1, Kc, T, m, affine=True, max_iters=0)
    with pytest.raises(vo.VoError):
        ctx.semiDenseAlignPyramid(0, 1, Kc, T, m, affine=True, levels=4)  # the slots hold levels 0..2
    with pytest.raises(ValueError):
        ctx.semiDenseAlign(key[0], 1, Kc, T, m, affine=dict(gain=1.0))
    r = ctx.semiDenseAlignPyramid(0, 1, Kc, T, TR.empty_map(key[0].shape), levels=3, affine=dict(AFFINE))
    G0, O0 = FR.start_GO(**AFFINE)
    assert r.levels == ((2, 1, 0, 0.0, G0, O0),) * 3 and r.status == 2 and np.array_equal(r.T_ck[:3], T[:3]) and not r.H.any() and (r.G, r.O) == (G0, O0)


# ---- 2. the driver --------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def stream():
    from visual_odometry_ros_amd import synthetic as S
    st = S.StereoStream(width=640, height=240, K=K, n_u=20, n_v=8, seed=2, speed=0.5)
    imgs = [st.render_pair(p)[:2] for p in st.poses(N_FRAMES)]
    imgs = [(FR.map_image(L, *CHANGE), FR.map_image(R, *CHANGE)) if k % 2 else (L, R) for k, (L, R) in enumerate(imgs)]
    bf = float(F(K[0] * st.baseline))
    return st, imgs, dict(bf=bf, d_min=0, d_max=67)


def _run(vo, stream, mode, align, look=None, before=None):
    """one run of N_FRAMES frames with the static and the temporal option and the alignment `align` on: per frame the frame info's
    bytes, the map's planes and the static result's as bytes, getSemiDenseAlign(); the final track set; before(k, svo) in front of
    frame k, look(k, svo) after its record"""
    st, imgs, prm = stream
    c, svo = _driver(vo, st, dict(prm, every="keyframe", temporal=dict(TPRM), align=dict(align)))
    rec = {}
    try:
        infos = []
        for k in range(N_FRAMES):
            if before:
                before(k, svo)
            if mode == "lookahead":
                svo.enqueue(*imgs[k])
                if k + 1 < N_FRAMES:
                    svo.prefetch(*imgs[k + 1])
                gi = svo.result()
            else:
                gi = svo.trackStereoImages(*imgs[k])
            infos.append(bytes(gi))
            m, s = svo.getSemiDenseMap(), svo.getSemiDense()
            rec[k] = dict(map=None if m is None else {p: getattr(m, p).copy() for p in MAP}, map_id=None if m is None else (m.frame_id, m.n_fused),
                          static=None if s is None else (s.frame_id, b"".join(getattr(s, p).tobytes() for p in STATIC)), align=svo.getSemiDenseAlign())
            if look:
                look(k, svo)
        tracks = {k: v.tobytes() for k, v in svo.getTracks().items()}
        return infos, tracks, rec
    finally:
        svo.close()
        c.close()


@pytest.fixture(scope="module")
def base_runs(vo, stream):
    """the runs with the alignment on and the modifier off, per configuration and calling mode (computed once)"""
    return {(cfg, mode): _run(vo, stream, mode, CONFIGS[cfg]) for cfg in CONFIGS for mode in ("lookahead", "sync")}


@pytest.fixture(scope="module")
def expected(vo, stream, base_runs, pyr_down):
    """per configuration, per frame: None (a keyframe frame, or no keyframe map yet) or the restatement's result with kf, start and
    T_wc — from the synchronous run's poses and maps, the restatement's own results chained for start = "previous" (computed once)"""
    _, imgs, _ = stream
    infos, _, per_frame = base_runs[("level_0", "sync")]
    info = [vo._capi.SvoFrameInfo.from_buffer_copy(b) for b in infos]
    T_wc = [np.array(i.T_wc, F).reshape(4, 4) for i in info]
    levels = [PR.image_pyramid(L, 4, pyr_down) for L, _ in imgs]
    G0, O0 = FR.start_GO(**AFFINE)
    out = {}
    for cfg, prm in CONFIGS.items():
        prm = dict(prm)
        start = prm.pop("start", "odometry")
        chain = []
        for k in range(N_FRAMES):
            kfs = [j for j in range(k + 1) if info[j].is_keyframe and j > 0]  # (the first frame seeds no map)
            if info[k].is_keyframe or not kfs:
                chain.append(None)
                continue
            kf = kfs[-1]
            T0, G, O, used = TR.pose_ck(T_wc[k], T_wc[kf]), G0, O0, "odometry"
            if start == "previous":
                if k == kf + 1:
                    T0 = I4
                elif chain[k - 1] is not None and chain[k - 1]["kf"] == kf and chain[k - 1]["status"] in (0, 1):
                    T0, G, O, used = chain[k - 1]["T_ck"], chain[k - 1]["G"], chain[k - 1]["O"], "previous"
            m = per_frame[k - 1]["map"]  # the map as it stood before this frame's temporal launch
            if "levels" in prm:
                want = FR.align_pyr(levels[kf], levels[k], K, T0, m, G=G, O=O, **prm, **AFFINE)
            else:
                want = FR.align_state(imgs[kf][0], imgs[k][0], K, T0, G, O, m, **prm)
                want["levels"] = [{f: want[f] for f in ("status", "iters", "count", "rms", "G", "O")}]
            T_kc = TR.pose_ck(want["T_ck"], I4)  # inverseSE3(T_ck) in the driver's order
            want.update(kf=kf, start=used, start_GO=(G, O), T_wc=AR.mul44(T_wc[kf], T_kc), from_odometry=distance(AR.mul44(T_wc[kf], T_kc), T_wc[k]))
            chain.append(want)
        out[cfg] = chain
    return info, out


@pytest.mark.parametrize("cfg", sorted(CONFIGS))
@pytest.mark.parametrize("mode", ["lookahead", "sync"])
def test_driver(vo, stream, base_runs, expected, mode, cfg):
    infos_off, tracks_off, rec_off = base_runs[(cfg, mode)]
    assert base_runs[("level_0", "sync")][0] == infos_off
    info, chains = expected
    chain = chains[cfg]
    n_levels = CONFIGS[cfg].get("levels", 1)
    G0, O0 = FR.start_GO(**AFFINE)
    seen = dict(aligned=0, none=0, previous=0, after_keyframe=0)
    far = dict(affine=[], plain=[])

    def look(k, svo):
        r = svo.getSemiDenseAlign()
        want = chain[k]
        if want is None:  # (c) a keyframe frame, or no keyframe map yet: no result, said with a status of its own
            assert (r.status, r.key_frame_id, r.iters, r.count) == (4, -1, 0, 0) and r.frame_id == info[k].frame_id, k
            assert np.array_equal(r.T_ck, I4) and np.array_equal(r.T_wc, I4) and not r.H.any() and (r.G, r.O) == (G0, O0)
            assert [lv.status for lv in r.levels] == [4] * n_levels
            seen["none"] += 1
            return
        d = _fields(r)
        ok, where = same_result(d, want)
        assert ok, (k, want["kf"], where)
        ok, where = same_levels(d["levels"], want["levels"], pose=False)
        assert ok, (k, where)
        assert (r.frame_id, r.key_frame_id, r.start) == (info[k].frame_id, info[want["kf"]].frame_id, want["start"]), k
        assert np.array_equal(r.T_wc.view(np.uint32), want["T_wc"].view(np.uint32)), k
        assert want["status"] in (0, 1) and want["count"] > 5000 and 0 < want["rms"] < 20, (k, want["status"], want["count"], want["rms"])
        if k == want["kf"] + 1:  # (c) the first frame after a keyframe starts from the parameters
            assert want["start_GO"] == (G0, O0) and want["start"] == "odometry"
            seen["after_keyframe"] += 1
        if want["start"] == "previous":  # (b) ... and takes G, O over with the pose, which shows in the result unless they were G0, O0
            assert want["start_GO"] == (chain[k - 1]["G"], chain[k - 1]["O"]) != (G0, O0)
            seen["previous"] += 1
        # the existing getter: the affine run's fields, H and b cut to the pose's rows and columns
        res = vo._capi.SemiDenseAlignResult()
        svo.ctx.check(svo.lib.vo_svo_get_semidense_align(svo._h, C.byref(res), None, None, None))
        assert (res.status, res.iters, res.count, res.rms) == (r.status, r.iters, r.count, r.rms) and bytes(res.T_ck) == r.T_ck.tobytes()
        assert list(res.H) == [r.H[i, j] for i, j in AR.PAIRS] and list(res.b) == list(r.b[:6])
        seen["aligned"] += 1
        if k % 2:  # a modified frame
            p = rec_off[k]["align"]
            far["affine"].append(want["from_odometry"][0])
            far["plain"].append(distance(p.T_wc, np.array(info[k].T_wc, F).reshape(4, 4))[0])
            print(f"{mode} {cfg} frame {k} (keyframe {want['kf']}, start {want['start']}): gain {r.gain:.4f}, offset {r.offset:.2f}, rms {r.rms:.2f}, "
                  f"{far['affine'][-1]:.3f} mm from the odometry's; without the modifier rms {p.rms:.2f}, {far['plain'][-1]:.3f} mm")

    infos_on, tracks_on, rec_on = _run(vo, stream, mode, dict(CONFIGS[cfg], affine=dict(AFFINE)), look)
    assert infos_on == infos_off and tracks_on == tracks_off  # (a) the odometry: the same bits
    for k in rec_on:
        _same_record(rec_on[k], rec_off[k], k)  # (a) the static result and the map: the same bits
    assert seen["aligned"] >= 3 and seen["none"] >= 2 and seen["after_keyframe"] >= 1, seen
    assert (seen["previous"] >= 1) == (cfg == "pyr_previous"), seen
    print(f"{mode} {cfg}: over the modified frames the aligned pose lies at most {max(far['affine']):.3f} mm from the odometry's with the modifier, "
          f"{max(far['plain']):.3f} mm without")
    assert max(far["affine"]) < max(far["plain"])


def test_driver_off_on_off(vo, stream, base_runs, expected):
    """(d) the modifier switched on in front of frames 3 and 6 and off in front of frames 4 and 7 (the level-0 option, whose results
    do not depend on the previous frame's): the frames with it off return the never-on run's bits, the others the affine chain's."""
    _, tracks_off, rec_off = base_runs[("level_0", "sync")]
    chain = expected[1]["level_0"]
    on_at = {3, 6}
    assert all(chain[k] is not None for k in on_at)

    def before(k, svo):
        if k in on_at:
            svo.setSemiDenseAlignAffine(dict(AFFINE))
        elif k - 1 in on_at:
            svo.setSemiDenseAlignAffine(None)

    _, tracks, rec = _run(vo, stream, "sync", CONFIGS["level_0"], before=before)
    assert tracks == tracks_off
    seen = dict(on=0, off=0)
    for k in range(N_FRAMES):
        _same_record(rec[k], rec_off[k], k)
        r = rec[k]["align"]
        if k in on_at and chain[k] is not None:
            ok, where = same_result(_fields(r), chain[k])
            assert ok, (k, where)
            seen["on"] += 1
        else:
            p = rec_off[k]["align"]
            assert r.gain is None and r.H.shape == (6, 6) and (r.status, r.iters, r.count, r.rms, r.frame_id, r.key_frame_id) == (
                p.status, p.iters, p.count, p.rms, p.frame_id, p.key_frame_id), k
            assert all(np.array_equal(getattr(r, f).view(np.uint8), getattr(p, f).view(np.uint8)) for f in ("T_ck", "T_wc", "H", "b")), k
            seen["off"] += r.status in (0, 1)
    assert seen["on"] >= 1 and seen["off"] >= 2, seen


def test_driver_modifier_lifecycle(vo, stream):
    st, imgs, prm = stream
    c, svo = _driver(vo, st)

    def count(ctx_):
        n = C.c_longlong()
        ctx_.check(ctx_.lib.vo_debug_allocation_count(ctx_.handle, C.byref(n)))
        return n.value
    try:
        assert not hasattr(vo.MonoVO, "setSemiDenseAlignAffine")  # a stereo driver's modifier (the C call refuses a mono driver's core)
        svo.setSemiDense(dict(prm))
        svo.setSemiDenseTemporal(dict(TPRM))
        with pytest.raises(vo.VoError) as e:  # needs an alignment option
            svo.setSemiDenseAlignAffine(True)
        assert e.value.code == -1
        svo.setSemiDenseAlignAffine(None)  # (off is always accepted)
        svo.setSemiDenseAlign(dict(CONFIGS["level_0"]))
        for bad in (dict(gain0=0.1), dict(gain0=9.0), dict(offset0=300.0), dict(gain0=float("nan"))):
            with pytest.raises(vo.VoError):
                svo.setSemiDenseAlignAffine(bad)
        with pytest.raises(ValueError):
            svo.setSemiDenseAlignAffine(dict(huber=2.0))
        assert svo.getSemiDenseAlign().gain is None
        n0 = count(c)
        svo.setSemiDenseAlignAffine(True)
        assert count(c) == n0 + 1  # the modifier's state block with its rows of partial sums
        r = svo.getSemiDenseAlign()
        assert r.status == 4 and (r.gain, r.offset) == (1.0, 0.0)  # no frame yet
        svo.enqueue(*imgs[0])
        for call in (lambda: svo.setSemiDenseAlignAffine(None), lambda: svo.setSemiDenseAlignAffine(True), svo.getSemiDenseAlign):  # in flight
            with pytest.raises(vo.VoError) as e:
                call()
            assert e.value.code == -1
        svo.result()
        infos = [None, svo.trackStereoImages(*imgs[1]), svo.trackStereoImages(*imgs[2])]
        assert infos[1].is_keyframe and not infos[2].is_keyframe
        a2 = svo.getSemiDenseAlign()
        assert a2.status in (0, 1) and a2.key_frame_id == infos[1].frame_id and a2.gain is not None and len(a2.levels) == 1
        # off and on again: no allocation; the alignment off turns the modifier off with it
        svo.setSemiDenseAlignAffine(None)
        assert svo.getSemiDenseAlign().gain is None and svo.getSemiDenseAlign().status == 4  # (the switch forgets the last result)
        n1 = count(c)  # (the frames have made the driver's own allocations since)
        svo.setSemiDenseAlignAffine(dict(AFFINE))
        assert count(c) == n1
        svo.setSemiDenseAlign(None)
        res = vo._capi.SemiDenseAlignAffineResult()
        assert svo.lib.vo_svo_get_semidense_align_affine(svo._h, C.byref(res), None, None, None) == -1
        svo.setSemiDenseAlign(dict(CONFIGS["pyr_previous"], affine=True))  # (through the alignment's own dict, as the constructor passes it)
        assert count(c) == n1 + 1  # (the coarse-to-fine option's key levels and map pyramid; its state block exists)
        svo.trackStereoImages(*imgs[3])
        assert svo.getSemiDenseAlign().gain == 1.0
    finally:
        svo.close()
        c.close()
