"""StereoVO's world map fed from the dense result (include/vo_hip.h, "Semi-dense map merge"): the sources "dense" and
"merged" of setSemiDenseWorld on the 640 x 240, 10-frame stream. The odometry's bits (poses, ids, track sets), the semi-dense map and the
dense results are those of the sources off; after every keyframe change getSemiDenseWorldSource() equals the restated merge
(tests/semidense_map_merge_restatement.py) of the map the driver itself returned for the outgoing keyframe and the dense result it
returned at that keyframe's own frame, to the bit; the world table after the flush equals a fresh table fed those restated planes in
order through the operator (which tests/test_semidense_world_gpu.py holds to its restatement) — through the look-ahead calls, the
synchronous call and runSequence, with the dense option per keyframe and per frame (the same bits), with and without the speckle
filter; with re-anchoring at min_move 0 (on 20 frames of the stream, where the local BA does move keyframes whose maps are in the table)
the table equals the operator fed at the anchors' poses, which are the keyframes' current ones;
with the carve on the free counts equal the operator's carve of the same planes; the flush; the errors; the one allocation; a keyframe
without a dense result integrates nothing. None of the sources or entry points exists without the feature."""
import ctypes as C

import numpy as np
import pytest

from semidense_map_merge_restatement import merge
from test_dense_stereo_gpu import K, N_FRAMES, SH, SW, _driver, _run
from test_dense_stereo_gpu import stream  # noqa: F401  (a fixture: the 640 x 240, 10-frame stream and the dense parameters)
from test_semidense_map_merge_emu import same_result
from test_semidense_temporal_gpu import TPRM
from test_semidense_world_gpu import WPRM as WPRM_RAW, _same_world

pytestmark = pytest.mark.gpu

N_LONG = 20
CARVE = dict(margin=1.5, chi=2.0, z_near=0.5)  # (not the defaults: the driver must carry the caller's)
WPRM = dict(WPRM_RAW, capacity_log2=21)  # (a dense-fed keyframe brings several times the voxels of a map of edges: room for the stream)


def _options(stream, source, every="keyframe", speckle=False, **world):
    _, _, dprm = stream
    sd = dict(bf=dprm["bf"], d_min=0, d_max=67, every="keyframe", temporal=dict(TPRM))
    if source is not None:
        sd["world"] = dict(WPRM, source=source, **world)
    dense = dict(dprm, every=every)
    if speckle:
        dense["speckle"] = True
    return dict(semidense=sd, dense=dense)


def _run_source(vo, stream, mode, source, every="keyframe", speckle=False, mprm=None, n=N_FRAMES, **world):
    """the stream through a driver with the static, temporal and dense options on and the world map fed from `source` (None: no world
    map). Returns the infos, tracks, per-frame snapshots of the map and the dense result, the restated planes of every keyframe that
    left (checked against getSemiDenseWorldSource() on the way) and the table after the flush."""
    _, imgs, dprm = stream
    if mprm:
        world["merge"] = mprm
    s = dict(prev=None, dense_at={}, left=[], snaps=[], index={})
    from_dense = source in ("dense", "merged")

    def leave(svo):
        m = s["prev"]
        ds = s["dense_at"][m.frame_id]
        want = merge(dict(invd=m.invd, sigma=m.sigma, n_obs=m.n_obs) if source == "merged" else None, ds.disparity, ds.sigma_invd, ds.status,
                     dprm["bf"], **(mprm or {}))
        got = svo.getSemiDenseWorldSource()
        assert got is not None and got.frame_id == m.frame_id, (got and got.frame_id, m.frame_id)
        assert same_result(got._asdict(), want) is None, (m.frame_id, same_result(got._asdict(), want))
        s["left"].append((want, m.T_wc, m.frame_id))

    def check(k, gi, svo):
        s["index"][gi.frame_id] = k
        if mode == "sequence":
            return
        m, ds = svo.getSemiDenseMap(), svo.getDenseStereo()
        if gi.is_keyframe:
            if from_dense and s["prev"] is not None:
                leave(svo)
            if ds is not None and ds.frame_id == gi.frame_id:
                s["dense_at"][gi.frame_id] = ds
        if every == "keyframe":  # (per frame the dense result is another one every frame: compared where it is a keyframe's)
            s["snaps"].append(None if ds is None else b"".join(np.ascontiguousarray(v).tobytes() for v in ds[:4]))
        s["snaps"].append(None if m is None else b"".join(getattr(m, p).tobytes() for p in ("invd", "sigma", "n_obs", "tstatus")) + m.T_wc.tobytes())
        s["prev"] = m

    def at_end(svo):
        if source is None:
            return None
        svo.flushSemiDenseWorld()
        if mode != "sequence" and from_dense:
            leave(svo)
        svo.flushSemiDenseWorld()  # (a second flush integrates nothing)
        return dict(rec=svo.getSemiDenseWorld(max_free=(0, 0)) if world.get("carve") else svo.getSemiDenseWorld(), stats=svo.getSemiDenseWorldStats(),
                    anchors=svo.getSemiDenseWorldAnchors() if world.get("reanchor") else None, kfs=[T for T, _ in svo.getKeyframes()],
                    src=svo.getSemiDenseWorldSource())

    infos, tracks, end = _run(vo, stream, mode, _options(stream, source, every, speckle, **world), check, n=n, at_end=at_end)
    return dict(infos=infos, tracks=tracks, snaps=s["snaps"], left=s["left"], index=s["index"], end=end)


def _operator_fed(vo, stream, run, poses=None, carve=None):
    """a fresh table of the driver's parameters fed the restated planes in order, each with its keyframe's pose (or `poses`) and left image"""
    _, imgs, _ = stream
    c = vo.Context(device=0, max_width=SW, max_height=SH, max_points=256, n_slots=2, max_level=0)
    try:
        with c.semiDenseWorld(**WPRM) as wm:
            for j, (want, T, fid) in enumerate(run["left"]):
                T = T if poses is None else poses[j]
                wm.integrate(want, K, T, key=imgs[run["index"][fid]][0])
                if carve:
                    wm.carve(want, K, T, **carve)
            return (wm.points(max_free=(0, 0)) if carve else wm.points()), wm.stats()
    finally:
        c.close()


@pytest.fixture(scope="module")
def off_run(vo, stream):
    return _run_source(vo, stream, "lookahead", None)


@pytest.fixture(scope="module")
def merged_run(vo, stream):
    return _run_source(vo, stream, "lookahead", "merged", speckle=True)


def _check_table(vo, stream, run):
    want, wstats = _operator_fed(vo, stream, run)
    _same_world(run["end"]["rec"], want)
    assert run["end"]["stats"] == wstats and wstats["integrations"] == len(run["left"]) >= 3 and wstats["refused"] == 0
    assert run["end"]["src"].frame_id == run["left"][-1][2]


def test_merged_source_lookahead_keeps_every_bit(vo, stream, off_run, merged_run):
    on = merged_run
    plain = _run(vo, stream, "lookahead", {})
    assert on["infos"] == plain[0] and on["tracks"] == plain[1]  # the odometry of every option off
    off = _run_source(vo, stream, "lookahead", None, speckle=True)
    assert on["infos"] == off["infos"] and on["tracks"] == off["tracks"] and on["snaps"] == off["snaps"] and off_run["infos"] == off["infos"]
    _check_table(vo, stream, on)
    counts = on["end"]["src"].counts
    assert int(counts.sum()) == SW * SH and counts[3] > 0 and counts[2] > counts[1] > 0  # fused pixels, and far more dense-only than map-only ones
    raw = _run_source(vo, stream, "lookahead", "raw")
    assert raw["end"]["src"] is None and len(on["end"]["rec"].xyz) > len(raw["end"]["rec"].xyz) > 0  # more voxels than the map of edges


@pytest.mark.parametrize("source,mode,every,speckle", [("merged", "sync", "frame", True), ("dense", "lookahead", "keyframe", False),
                                                       ("dense", "sync", "frame", True), ("merged", "lookahead", "frame", False)])
def test_sources_modes_and_every(vo, stream, off_run, merged_run, source, mode, every, speckle):
    run = _run_source(vo, stream, mode, source, every=every, speckle=speckle)
    assert run["infos"] == off_run["infos"] and run["tracks"] == off_run["tracks"]
    _check_table(vo, stream, run)
    if source == "merged" and speckle:  # per frame or per keyframe, look-ahead or synchronous: the same planes and the same table
        for (a, _, fa), (b, _, fb) in zip(run["left"], merged_run["left"]):
            assert fa == fb and same_result(a, b) is None
        _same_world(run["end"]["rec"], merged_run["end"]["rec"])
    if source == "dense":
        assert run["end"]["src"].counts[[1, 3, 4, 5]].sum() == 0


def test_run_sequence(vo, stream, off_run, merged_run):
    run = _run_source(vo, stream, "sequence", "merged", speckle=True)
    assert run["infos"] == off_run["infos"] and run["tracks"] == off_run["tracks"]
    _same_world(run["end"]["rec"], merged_run["end"]["rec"])
    assert run["end"]["stats"] == merged_run["end"]["stats"]
    assert same_result(run["end"]["src"]._asdict(), merged_run["end"]["src"]._asdict()) is None


def test_merge_parameters_reach_the_launch(vo, stream, merged_run):
    run = _run_source(vo, stream, "sync", "merged", speckle=True, mprm=dict(chi=0.5, keep_obs=1))
    _check_table(vo, stream, run)
    assert run["end"]["src"].counts[5] == 0 and run["end"]["src"].counts[4] > merged_run["end"]["src"].counts[4]


@pytest.fixture(scope="module")
def long_stream(stream):
    """the same stream, 20 frames of it as tests/test_semidense_world_reanchor_gpu.py takes: within the first 10 the local BA moves no
    keyframe whose map is in the table already, and the re-anchoring would be checked on nothing"""
    st, _, dprm = stream
    return st, [st.render_pair(p)[:2] for p in st.poses(N_LONG)], dprm


def test_reanchor_and_carve(vo, stream, long_stream):
    off = _run(vo, long_stream, "lookahead", {}, n=N_LONG)
    run = _run_source(vo, long_stream, "lookahead", "merged", speckle=True, n=N_LONG, reanchor=dict(min_move=0.0), carve=dict(CARVE))
    assert run["infos"] == off[0] and run["tracks"] == off[1]
    an = run["end"]["anchors"]
    assert list(an["frame_id"]) == [fid for _, _, fid in run["left"]]
    for j, T in zip(an["index"], an["T_wk"]):  # min_move 0: the map agrees with the published trajectory to the byte
        assert T.tobytes() == run["end"]["kfs"][j].tobytes(), j
    assert sum(T.tobytes() != a.tobytes() for (_, T, _), a in zip(run["left"], an["T_wk"])) >= 1  # the BA moved a keyframe in the table
    # the carve ran at each keyframe's own pose, when it left; the records but for `free` are those of the final poses
    want, _ = _operator_fed(vo, long_stream, run, poses=list(an["T_wk"]))
    _same_world(run["end"]["rec"], want)
    plain = _run_source(vo, stream, "lookahead", "merged", speckle=True, carve=dict(CARVE))
    wantf, wstats = _operator_fed(vo, stream, plain, carve=CARVE)
    _same_world(plain["end"]["rec"], wantf)
    assert plain["end"]["rec"].free.tobytes() == wantf.free.tobytes() and int(wantf.free.sum()) > 0 and plain["end"]["stats"] == wstats


def test_errors_allocation_and_a_keyframe_without_a_dense_result(vo, stream):
    st, imgs, dprm = stream
    c, svo = _driver(vo, st)
    try:
        n = C.c_longlong()
        count = lambda: (c.check(c.lib.vo_debug_allocation_count(c.handle, C.byref(n))), n.value)[1]
        svo.setSemiDense(dict(bf=dprm["bf"], d_min=0, d_max=67))
        svo.setSemiDenseTemporal(dict(TPRM))
        for src in ("dense", "merged"):
            with pytest.raises(vo.VoError) as e:  # needs the dense option
                svo.setSemiDenseWorld(dict(WPRM, source=src))
            assert e.value.code == -1 and "vo_svo_set_dense_stereo" in str(e.value)
        svo.setSemiDenseWorld(dict(WPRM))  # raw: the table's allocation, none for the merge
        assert svo.getSemiDenseWorldSource() is None
        svo.setDenseStereo(dict(dprm))
        for bad in (dict(chi=0.0), dict(chi=float("nan")), dict(keep_obs=-1), dict(keep_obs=257)):
            with pytest.raises(vo.VoError) as e:
                svo.setSemiDenseWorldMerge(bad)
            assert e.value.code == -1, bad
        with pytest.raises(ValueError):
            svo.setSemiDenseWorldMerge(dict(keep=3))
        for k in (0, 1, 2):  # a keyframe whose dense result exists, but which the source was not on for
            svo.trackStereoImages(*imgs[k])
        n0 = count()
        svo.setSemiDenseWorld(dict(WPRM, source="merged"))
        assert count() == n0 + 1  # the sources' only allocation, once
        svo.setSemiDenseWorld(dict(WPRM, source="dense"))
        svo.setSemiDenseWorld(dict(WPRM, source="merged", merge=dict(chi=2.0)))
        svo.setSemiDenseWorldMerge(None)
        assert count() == n0 + 1
        base = svo.getSemiDenseWorldStats()["integrations"]  # (what the raw source integrated so far)
        svo.flushSemiDenseWorld()  # the current keyframe has no kept dense result: nothing is integrated, now or later
        assert svo.getSemiDenseWorldStats()["integrations"] == base and svo.getSemiDenseWorldSource() is None
        k, seen = 3, 0
        while k < N_FRAMES and seen < 2:  # the next keyframe change integrates nothing either; the one after it does
            if k == 3:
                svo.enqueue(*imgs[k])
                for call in (lambda: svo.setSemiDenseWorldMerge(None), svo.getSemiDenseWorldSource):  # a frame is in flight
                    with pytest.raises(vo.VoError) as e:
                        call()
                    assert e.value.code == -1
                gi = svo.result()
            else:
                gi = svo.trackStereoImages(*imgs[k])
            k += 1
            if gi.is_keyframe:
                seen += 1
                assert svo.getSemiDenseWorldStats()["integrations"] == base + seen - 1, k
        assert seen == 2 and svo.getSemiDenseWorldSource() is not None
        svo.setDenseStereo(None)  # dense off: the next enable of such a source fails, and a keyframe replaced meanwhile integrates nothing
        with pytest.raises(vo.VoError):
            svo.setSemiDenseWorld(dict(WPRM, source="merged"))
        before = svo.getSemiDenseWorldStats()["integrations"]
        svo.flushSemiDenseWorld()
        assert svo.getSemiDenseWorldStats()["integrations"] == before
        assert count() == n0 + 1
        svo.setSemiDenseWorld(None)
        with pytest.raises(vo.VoError):  # the world option is off
            svo.getSemiDenseWorldSource()
        assert not hasattr(vo.MonoVO, "setSemiDenseWorldMerge") and not hasattr(vo.MonoVO, "getSemiDenseWorldSource")
    finally:
        svo.close()
        c.close()
    with pytest.raises(ValueError):  # the constructor's form says so too
        _driver(vo, st, semidense=dict(bf=dprm["bf"], d_min=0, d_max=67, temporal=dict(TPRM), world=dict(WPRM, source="merged")))
