"""Removal and re-anchoring on the world-frame voxel map on the device (include/vo_hip.h, "Semi-dense world map: removal and
re-anchoring"), everything bit for bit after the canonical sort by key. The operator — remove, reanchor, reanchorStats
— on the operations of tests/test_semidense_world_reanchor.py against the numpy restatement, with host planes and with device planes
(key stride padded); equal poses; the empty table; the refusals. And StereoVO's option on the 640 x 240 stream with the static,
temporal, propagation, regularisation and world options on: THE INVARIANT — after the flush the world map's records equal those of a
fresh table fed, in order, the maps that left, each with the applied pose getSemiDenseWorldAnchors() reports, and differ from the
table fed the maps' own T_wc (what the driver gives without the option); with min_move 0 every applied pose is the keyframe's pose
of getKeyframes() to the byte; nothing missing, nothing refused — through the look-ahead calls, the synchronous call and
runSequence, raw and regularised source; a large min_move re-anchors nothing; the option changes no bit of the odometry, the
semi-dense results or the keyframe poses; one allocation; the error returns (the C call's refusal of a mono driver is not exercised: no public call yields the vo_svo core of a
MonoVO, so only the absence of the method on MonoVO is asserted). None of the entry points exists without the feature."""
import ctypes as C

import numpy as np
import pytest

import semidense_world_reanchor_restatement as RR
from test_semidense_propagate_gpu import PPRM
from test_semidense_temporal_gpu import K, SH, SW, TPRM, _driver
from test_semidense_world import CASES, case_steps, same_records
from test_semidense_world_gpu import RPRM, WPRM, _same_world, _snapshot
from test_semidense_world_reanchor import OP_CASES, apply_ops, filled_past_the_bound, moved_pose, reanchor_ops, restated_ops
from util import DeviceBuffer

pytestmark = pytest.mark.gpu

F = np.float32
# The stream of the world map's tests, lengthened from 10 frames to 20: in 10 it has three keyframes, and the local BA, which holds the
# first two keyframes of its window fixed, has then moved no keyframe whose map is in the table (the condition is asserted below).
N_FRAMES = 20
FIELDS = ("index", "sums", "count", "keyframes", "weight", "grey", "xyz")


@pytest.fixture(scope="module")
def sdw_ctx(vo):
    c = vo.Context(device=0, max_width=203, max_height=61, max_points=256, n_slots=2, max_level=0)
    yield c
    c.close()


# ---- 1. the operator ----------------------------------------------------------------------------------------------------------------
def _apply(wm, ops, device):
    moved = []
    for op, s, T, T2 in ops:
        h, w = s["map"]["invd"].shape
        poses = (T,) if op != "reanchor" else (T, T2)
        call = dict(integrate=wm.integrate, remove=wm.remove, reanchor=wm.reanchor)[op]
        if not device:
            moved.append(call(s["map"], s["K"], *poses, key=s["Lk"]))
            continue
        bufs = [DeviceBuffer(np.ascontiguousarray(s["map"][k])) for k in ("invd", "sigma", "n_obs")]
        dkey = None
        if s["Lk"] is not None:
            padded = np.full((h, w + 5), 0xEE, np.uint8)
            padded[:, :w] = s["Lk"]
            dkey = DeviceBuffer(padded)
        try:
            moved.append(call(dict(zip(("invd", "sigma", "n_obs"), (b.data_ptr() for b in bufs))), s["K"], *poses,
                              key=None if dkey is None else dkey.data_ptr(), on_device=(w, h), key_on_device=None if dkey is None else w + 5))
        finally:
            for b in bufs + ([] if dkey is None else [dkey]):
                b.free()
    return moved


def _check(wm, w, name):
    ok, where = same_records(wm.points()._asdict(), w.records(), fields=FIELDS)
    assert ok, (name, where)
    assert wm.stats() == w.stats, (name, wm.stats(), w.stats)
    assert wm.reanchorStats() == w.rstats, (name, wm.reanchorStats(), w.rstats)


@pytest.mark.parametrize("name", OP_CASES)
def test_operator_equals_restatement(vo, sdw_ctx, name):
    ops, want = reanchor_ops(name), restated_ops(name)
    for device in (False, True):
        with sdw_ctx.semiDenseWorld(**CASES[name]) as wm:
            moved = _apply(wm, ops, device)
            assert [m for (op, *_), m in zip(ops, moved) if op == "reanchor"] == [False] + [True] * (want.rstats["reanchors"])
            _check(wm, want, name)
            assert want.rstats["missing"] == 0 and want.rstats["vacant"] >= 1


def test_reanchor_with_equal_poses_is_nothing(vo, sdw_ctx):
    name = "a_203x61"
    A, B = case_steps(name)
    w = RR.World(**CASES[name])
    with sdw_ctx.semiDenseWorld(**CASES[name]) as wm:
        for s in (A, B):
            wm.integrate(s["map"], s["K"], s["T"], key=s["Lk"])
            w.integrate(s["map"], s["K"], s["T"], s["Lk"])
        before = (wm.points(), wm.stats(), wm.reanchorStats())
        T2 = A["T"].copy()
        T2[3] = (5.0, 6.0, 7.0, 8.0)  # (the last row is not part of the pose)
        assert wm.reanchor(A["map"], A["K"], A["T"], T2, key=A["Lk"]) is False
        after = (wm.points(), wm.stats(), wm.reanchorStats())
        assert all(x.tobytes() == y.tobytes() for x, y in zip(before[0], after[0])) and before[1:] == after[1:]
        assert after[2] == dict.fromkeys(RR.RCOUNTERS, 0)
        # no sequence number was taken: what follows equals the restatement, which took none
        T3 = moved_pose(A["T"])
        assert wm.reanchor(A["map"], A["K"], A["T"], T3, key=A["Lk"]) is True and w.reanchor(A["map"], A["K"], A["T"], T3, A["Lk"])
        _check(wm, w, name)
        with pytest.raises(vo.VoError):  # a pose that is not finite: refused before either launch
            wm.reanchor(A["map"], A["K"], T3, np.full((4, 4), np.nan, F), key=A["Lk"])
        _check(wm, w, name)


def test_removal_from_an_empty_table_and_the_refusals(vo, sdw_ctx):
    name = "a_203x61"
    A = case_steps(name)[0]
    with sdw_ctx.semiDenseWorld(**CASES[name]) as wm:
        wm.remove(A["map"], A["K"], A["T"], key=A["Lk"])
        w = apply_ops(RR.World(**CASES[name]), [("remove", A, A["T"], None)])
        _check(wm, w, name)
        assert wm.reanchorStats()["missing"] >= 1000 and wm.stats()["occupied"] == 0 and len(wm.points().xyz) == 0
    name = "b_cap12_strips"
    ops, s = filled_past_the_bound()
    base = apply_ops(RR.World(**CASES[name]), ops)
    for extra in (("remove", s, s["T"], None), ("reanchor", s, s["T"], moved_pose(s["T"]))):
        with sdw_ctx.semiDenseWorld(**CASES[name]) as wm:
            _apply(wm, ops, False)
            _check(wm, base, name)
            full = wm.points(), wm.stats()
            _apply(wm, [extra], True)
            assert all(x.tobytes() == y.tobytes() for x, y in zip(full[0], wm.points()))
            assert wm.stats() == dict(full[1], refused=full[1]["refused"] + (extra[0] == "reanchor"))
            r = wm.reanchorStats()
            assert r["refused_removals"] == 1 and r["removals"] == 0 and r["removed"] == 0 and r["reanchors"] == (extra[0] == "reanchor")
            _check(wm, apply_ops(RR.World(**CASES[name]), ops + [extra]), name)


# ---- 2. the driver --------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def stream():
    from visual_odometry_ros_amd import synthetic as S
    st = S.StereoStream(width=SW, height=SH, K=K, n_u=20, n_v=8, seed=2, speed=0.5)
    imgs = [st.render_pair(p)[:2] for p in st.poses(N_FRAMES)]
    bf = float(F(K[0] * st.baseline))
    return st, imgs, dict(bf=bf, d_min=0, d_max=67)


def _run(vo, stream, mode, world, window=None):
    """the stream through a driver with the static, temporal, propagation, regularisation and world options on; returns the infos
    (bytes), the final tracks, per-frame snapshots, the maps that left (raw, regularised) in order, and after the flush the world
    map's records and statistics, the anchors and the keyframes' poses"""
    st, imgs, prm = stream
    sd = dict(prm, every="keyframe", temporal=dict(TPRM), propagate=dict(PPRM), regularize=dict(RPRM), world=dict(world))
    if window is None:
        c, svo = _driver(vo, st, sd)
    else:  # (_driver's settings with a shorter window of keyframes)
        c = vo.Context(device=0, max_width=SW, max_height=SH, max_points=4096, n_slots=5, max_level=4)
        svo = vo.StereoVO(c, SW, SH, K, K, st.T_lr, 20, 8, thres_fastscore=15, window_size=21, max_level=4, strict_border=4, local_ba=True,
                          thres_trans=1.2, thres_alive_ratio=0.6, n_max_keyframes_in_window=window, semidense=sd)
    try:
        infos, snaps, left, prev = [], [], [], None
        if mode == "sequence":
            got, _ = svo.runSequence([(L, R) for L, R in imgs])
            infos = [bytes(i) for i in got]
        else:
            for k in range(N_FRAMES):
                if mode == "lookahead":
                    svo.enqueue(*imgs[k])
                    if k + 1 < N_FRAMES:
                        svo.prefetch(*imgs[k + 1])
                    gi = svo.result()
                else:
                    gi = svo.trackStereoImages(*imgs[k])
                infos.append(bytes(gi))
                snap, reg, raw = _snapshot(svo)
                snaps.append(snap)
                if gi.is_keyframe and prev is not None and prev[0] is not None:
                    left.append(prev)  # the map as it stood after the last frame before the keyframe change
                prev = (raw, reg)
            if prev is not None and prev[0] is not None:
                left.append(prev)
        svo.flushSemiDenseWorld()
        reanchor = "reanchor" in world
        return dict(infos=infos, tracks={k: v.tobytes() for k, v in svo.getTracks().items()}, snaps=snaps, left=left, rec=svo.getSemiDenseWorld(),
                    stats=svo.getSemiDenseWorldStats(), anchors=svo.getSemiDenseWorldAnchors() if reanchor else None,
                    rstats=svo.getSemiDenseWorldReanchorStats(), kfs=[T for T, _ in svo.getKeyframes()],
                    index={vo._capi.SvoFrameInfo.from_buffer_copy(b).frame_id: k for k, b in enumerate(infos)})
    finally:
        svo.close()
        c.close()


def _operator_fed(vo, stream, run, which, world, poses):
    """a fresh table of the same parameters fed the maps that left in order, map i with poses[i] and its keyframe's left image"""
    _, imgs, _ = stream
    c = vo.Context(device=0, max_width=SW, max_height=SH, max_points=256, n_slots=2, max_level=0)
    try:
        prm = {k: v for k, v in world.items() if k not in ("source", "reanchor")}
        with c.semiDenseWorld(**prm) as wm:
            for (raw, reg), T in zip(run["left"], poses):
                wm.integrate(raw if which == "raw" else reg, K, T, key=imgs[run["index"][raw.frame_id]][0])
            return wm.points()
    finally:
        c.close()


def _differs(a, b):
    return any(getattr(a, k).shape != getattr(b, k).shape or getattr(a, k).tobytes() != getattr(b, k).tobytes() for k in ("index", "xyz", "weight", "count"))


def _check_invariant(vo, stream, run, which, world, all_in_window=True):
    an, left = run["anchors"], run["left"]
    assert len(left) >= 3 and list(an["frame_id"]) == [raw.frame_id for raw, _ in left]  # one anchor per integrated keyframe, in order
    assert list(an["index"]) == sorted(set(an["index"]))
    assert an["in_window"].all() == all_in_window  # (the stream has fewer keyframes than the default window holds)
    own = [raw.T_wc for raw, _ in left]
    n_moved = sum(T.tobytes() != a.tobytes() for T, a in zip(own, an["T_wk"]))
    print(which, "keyframes integrated", len(left), "moved by the local BA since", n_moved, run["rstats"], run["stats"])
    assert n_moved >= 1  # non-vacuity: the BA has moved a keyframe whose map was in the table
    for j, T in zip(an["index"], an["T_wk"]):  # min_move 0: the map agrees with the published trajectory to the byte
        assert T.tobytes() == run["kfs"][j].tobytes(), j
    _same_world(run["rec"], _operator_fed(vo, stream, run, which, world, an["T_wk"]))
    stale = _operator_fed(vo, stream, run, which, world, own)  # what the driver gives without the option
    assert _differs(run["rec"], stale)
    r = run["rstats"]
    assert r["missing"] == 0 and r["refused_removals"] == 0 and r["reanchors"] == r["removals"] >= n_moved and run["stats"]["refused"] == 0
    assert run["stats"]["integrations"] == len(left) + r["reanchors"]
    return stale


@pytest.fixture(scope="module")
def off_run(vo, stream):
    return _run(vo, stream, "lookahead", WPRM)


@pytest.fixture(scope="module")
def on_run(vo, stream):
    return _run(vo, stream, "lookahead", dict(WPRM, reanchor=True))


def test_the_world_map_follows_the_local_ba(vo, stream, off_run, on_run):
    stale = _check_invariant(vo, stream, on_run, "raw", WPRM)
    _same_world(off_run["rec"], stale)  # (and without the option the driver gives exactly that)
    # option on against off: the odometry, every semi-dense result and the keyframes' poses are the same bytes
    assert on_run["infos"] == off_run["infos"] and on_run["tracks"] == off_run["tracks"] and on_run["snaps"] == off_run["snaps"]
    assert [T.tobytes() for T in on_run["kfs"]] == [T.tobytes() for T in off_run["kfs"]]
    assert off_run["rstats"] == dict.fromkeys(RR.RCOUNTERS, 0)


@pytest.mark.parametrize("mode", ["sync", "sequence"])
def test_the_other_calling_modes(vo, stream, on_run, mode):
    run = _run(vo, stream, mode, dict(WPRM, reanchor=dict(min_move=0.0)))
    assert run["infos"] == on_run["infos"] and run["tracks"] == on_run["tracks"]
    if mode == "sync":
        _check_invariant(vo, stream, run, "raw", WPRM)
    _same_world(run["rec"], on_run["rec"])
    assert run["stats"] == on_run["stats"] and {k: v for k, v in run["rstats"].items()} == on_run["rstats"]
    assert all(run["anchors"][k].tobytes() == on_run["anchors"][k].tobytes() for k in ("frame_id", "index", "T_wk", "in_window"))


def test_regularised_source(vo, stream, on_run):
    world = dict(WPRM, source="regularized")
    run = _run(vo, stream, "sync", dict(world, reanchor=True))
    assert run["infos"] == on_run["infos"] and run["snaps"] == on_run["snaps"]
    _check_invariant(vo, stream, run, "regularized", world)


def test_a_short_window_freezes_the_anchors_that_leave_it(vo, stream):
    """A window of 4 keyframes under the stream's 7: keyframes leave the window, their anchors are frozen and their ring places (4)
    taken again. The local BA moves a keyframe only while it is in the window, and the pass of the last keyframe frame it was in has
    re-anchored it, so a frozen anchor's pose is still the published one, and the invariant holds as before."""
    run = _run(vo, stream, "lookahead", dict(WPRM, reanchor=True), window=4)
    inw = run["anchors"]["in_window"]
    print("in window", inw)
    assert len(inw) >= 6 and inw.sum() == 4 and not inw[:len(inw) - 4].any() and inw[len(inw) - 4:].all()
    _check_invariant(vo, stream, run, "raw", WPRM, all_in_window=False)
    off = _run(vo, stream, "lookahead", WPRM, window=4)
    assert run["infos"] == off["infos"] and run["snaps"] == off["snaps"] and [T.tobytes() for T in run["kfs"]] == [T.tobytes() for T in off["kfs"]]


def test_a_large_min_move_reanchors_nothing(vo, stream, off_run):
    run = _run(vo, stream, "lookahead", dict(WPRM, reanchor=dict(min_move=1e6)))
    assert run["rstats"] == dict.fromkeys(RR.RCOUNTERS, 0) and run["stats"] == off_run["stats"]
    _same_world(run["rec"], off_run["rec"])
    assert [T.tobytes() for T in run["anchors"]["T_wk"]] == [raw.T_wc.tobytes() for raw, _ in run["left"]]  # the applied poses stay


def test_refused_pairs_leave_the_applied_pose(vo, stream):
    """2^18 slots: 640 x 240 pixels exceed half the table, so the device refuses every integration and every pair. The host enqueues
    the pairs without knowing; the getters read refused_removals and give every anchor its pose back."""
    run = _run(vo, stream, "lookahead", dict(WPRM, capacity_log2=18, reanchor=True))
    r, st = run["rstats"], run["stats"]
    print(r, st)
    assert r["reanchors"] >= 1 and r["refused_removals"] == r["reanchors"] and r["removals"] == 0 and r["removed"] == 0 and r["vacant"] == 0
    assert st["integrations"] == 0 and st["refused"] == len(run["left"]) + r["reanchors"] and st["occupied"] == 0 and len(run["rec"].xyz) == 0
    assert [T.tobytes() for T in run["anchors"]["T_wk"]] == [raw.T_wc.tobytes() for raw, _ in run["left"]]


def test_one_allocation_and_the_error_returns(vo, stream):
    st, imgs, prm = stream
    assert not hasattr(vo.MonoVO, "setSemiDenseWorldReanchor")  # a stereo driver's option (the C call refuses a mono driver's core)
    sd = dict(prm, every="keyframe", temporal=dict(TPRM))
    c = vo.Context(device=0, max_width=SW, max_height=SH, max_points=4096, n_slots=5, max_level=4)
    svo = vo.StereoVO(c, SW, SH, K, K, st.T_lr, 20, 8, thres_fastscore=15, window_size=21, max_level=4, strict_border=4, local_ba=False,
                      thres_trans=1.2, thres_alive_ratio=0.6, semidense=dict(sd, world=dict(WPRM)))
    try:
        with pytest.raises(vo.VoError) as e:  # nothing moves a keyframe without the local BA
            svo.setSemiDenseWorldReanchor(True)
        assert e.value.code == -1
        svo.setSemiDenseWorldReanchor(None)  # (off is always accepted)
    finally:
        svo.close()
        c.close()
    c, svo = _driver(vo, st, sd)
    try:
        with pytest.raises(vo.VoError) as e:  # needs the world map
            svo.setSemiDenseWorldReanchor(True)
        assert e.value.code == -1
        with pytest.raises(vo.VoError):
            svo.getSemiDenseWorldAnchors()
        n = C.c_longlong()
        count = lambda: (c.check(c.lib.vo_debug_allocation_count(c.handle, C.byref(n))), n.value)[1]
        svo.trackStereoImages(*imgs[0])
        svo.setSemiDenseWorld(dict(WPRM))
        n0 = count()
        for bad in (-1.0, float("nan"), float("inf")):
            with pytest.raises(vo.VoError) as e:
                svo.setSemiDenseWorldReanchor(dict(min_move=bad))
            assert e.value.code == -1
        with pytest.raises(ValueError):
            svo.setSemiDenseWorldReanchor(dict(radius=1))
        assert count() == n0
        svo.setSemiDenseWorldReanchor(True)
        assert count() == n0 + 1  # the option's only allocation: the ring of retained maps
        svo.setSemiDenseWorldReanchor(None)
        svo.setSemiDenseWorldReanchor(dict(min_move=0.5))
        assert count() == n0 + 1 and len(svo.getSemiDenseWorldAnchors()["frame_id"]) == 0
        svo.enqueue(*imgs[1])
        for call in (lambda: svo.setSemiDenseWorldReanchor(True), lambda: svo.setSemiDenseWorldReanchor(None), svo.getSemiDenseWorldAnchors,
                     svo.getSemiDenseWorldReanchorStats):  # in flight
            with pytest.raises(vo.VoError) as e:
                call()
            assert e.value.code == -1
        svo.result()
        svo.flushSemiDenseWorld()
        an = svo.getSemiDenseWorldAnchors()
        assert len(an["frame_id"]) == 1 and an["T_wk"][0].tobytes() == svo.getSemiDenseMap().T_wc.tobytes()
        svo.clearSemiDenseWorld()  # the table is empty: no map is in it
        assert len(svo.getSemiDenseWorldAnchors()["frame_id"]) == 0 and svo.getSemiDenseWorldReanchorStats() == dict.fromkeys(RR.RCOUNTERS, 0)
    finally:
        svo.close()
        c.close()
