"""Free-space carving on the world-frame voxel map on the device (include/vo_hip.h, "Semi-dense world map: free-space carving";
DESIGN.md §26) against the numpy restatement (tests/semidense_world_carve_restatement.py), everything bit for bit after the canonical
sort by key: the operator on the cases of tests/test_semidense_world_carve.py — host planes and device planes, the pre-aggregated
kernel form and the simple one —, the free filter, the extraction's capacity, the argument errors, two fresh tables fed alike, clear
and the same input again, the guards on the full 640 x 240 maps; and StereoVO's option through the look-ahead calls, the synchronous
call and runSequence: the odometry, every semi-dense result and every field of the world map but `free` the same bits as without it,
`free` and the carve's counters equal to an operator fed the maps the driver itself returned, no keyframe carved twice, the option
switched off and on, the refusals, re-anchoring next to it; and the sequence example's PLY against the same loop in process. None of
the entry points exists without the feature."""
import ctypes as C

import numpy as np
import pytest

import semidense_world_carve_restatement as CR
import semidense_world_restatement as WR
from test_semidense_propagate_gpu import PPRM
from test_semidense_temporal_gpu import K, N_FRAMES, SH, SW, TPRM, _driver
from test_semidense_world import full_maps, same_records
from test_semidense_world_carve import (CARVE_CASES, GUARD, assert_guards, carve_ops, guard_figures, guard_shares, phantom_maps, restated)
from test_semidense_world_gpu import RPRM, WPRM, _same_world, _snapshot, sdw_ctx, stream  # noqa: F401 (fixtures)
from util import DeviceBuffer

pytestmark = pytest.mark.gpu

F = np.float32
VO_DBG_SDW_FORM = 10
ALL = (0, 0)  # max_free: no filter, `free` returned
FIELDS = ("index", "sums", "count", "keyframes", "weight", "grey", "xyz")


def _apply(wm, ops, device):
    for op, s, prm in ops:
        if op == "clear":
            wm.clear()
            continue
        h, w = s["map"]["invd"].shape
        bufs = [DeviceBuffer(np.ascontiguousarray(s["map"][k])) for k in ("invd", "sigma", "n_obs")] if device else []
        m = dict(zip(("invd", "sigma", "n_obs"), (b.data_ptr() for b in bufs))) if device else s["map"]
        on_device = (w, h) if device else None
        try:
            if op == "carve":
                wm.carve(m, s["K"], s["T"], on_device=on_device, **prm)
            else:
                (wm.integrate if op == "integrate" else wm.remove)(m, s["K"], s["T"], key=s["Lk"], on_device=on_device)
        finally:
            for b in bufs:
                b.free()


def _check(wm, w):
    want = w.records()
    got = wm.points(max_free=ALL)
    ok, where = same_records(got._asdict(), want, fields=FIELDS + ("free",))
    assert ok, where
    assert wm.carveStats() == w.cstats and wm.stats() == w.stats and wm.reanchorStats() == w.rstats, (wm.carveStats(), w.cstats)
    plain = wm.points()  # without max_free: what it returned before there was a carve
    assert type(plain).__name__ == "SemiDenseWorldPoints" and plain._fields == ("index", "xyz", "weight", "count", "keyframes", "grey", "sums")
    ok, where = same_records(plain._asdict(), want, fields=FIELDS)
    assert ok, where
    return got


# ---- 1. the operator ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(CARVE_CASES))
def test_operator_equals_restatement(vo, sdw_ctx, name):  # noqa: F811
    ctx = sdw_ctx
    try:
        for form in (0, 1):
            ctx.debug_set(VO_DBG_SDW_FORM, form)
            for device in (False, True):
                with ctx.semiDenseWorld(**CARVE_CASES[name]) as wm:
                    _apply(wm, carve_ops(name), device)
                    _check(wm, restated(name))
    finally:
        ctx.debug_set(VO_DBG_SDW_FORM, 0)


def test_filter_capacity_and_errors(vo, sdw_ctx):  # noqa: F811
    ctx = sdw_ctx
    name = "j_phantom"
    w = restated(name)
    ops = carve_ops(name)
    with ctx.semiDenseWorld(**CARVE_CASES[name]) as wm:
        _apply(wm, ops, False)
        _check(wm, w)
        for mf in ((0, 1), (1, 2), (1, 1), (3, 1), (1000000, 3)):
            want = w.records(max_free=mf)
            got = wm.points(max_free=mf)
            ok, where = same_records(got._asdict(), want, fields=FIELDS + ("free",))
            assert ok and 0 < len(want["key"]), (mf, where)
        assert len(w.records(max_free=(0, 1))["key"]) < len(w.records(max_free=(3, 1))["key"]) <= len(w.records()["key"])
        want = w.records(min_keyframes=1, min_count=2, max_free=(1, 2))
        got = wm.points(min_count=2, max_free=(1, 2))
        assert same_records(got._asdict(), want, fields=FIELDS + ("free",))[0]
        # a capacity below the count: the true count, the first records in key order, nothing behind them
        want = w.records(max_free=(1, 1))
        n_all = len(want["key"])
        with pytest.raises(vo.VoError) as e:
            wm.points(max_free=(1, 1), capacity=10)
        assert e.value.code == -8 and e.value.n == n_all > 11
        n = C.c_int()
        free, cnt = np.full(11, 77, np.uint32), np.full(11, 78, np.uint32)
        pf = ctx.lib.vo_semidense_world_points_free
        rc = pf(wm._h, 1, 1, 1, 1, 10, None, None, None, cnt.ctypes.data, None, None, None, free.ctypes.data, C.byref(n))
        assert rc == -8 and n.value == n_all
        assert np.array_equal(free[:10], want["free"][:10]) and free[10] == 77 and np.array_equal(cnt[:10], want["count"][:10]) and cnt[10] == 78
        assert pf(wm._h, 1, 1, 1, 1, 0, None, None, None, None, None, None, None, None, C.byref(n)) == -8 and n.value == n_all
        for bad in ((0, 1, 1, 1), (1, 0, 1, 1), (1, 1, -1, 1), (1, 1, 1, -1)):
            assert pf(wm._h, *bad, 0, None, None, None, None, None, None, None, None, C.byref(n)) == -1
        # argument errors: none of them touches the table or a counter
        before = (wm.points(max_free=ALL), wm.carveStats(), wm.stats())
        s = ops[0][1]
        for bad in (dict(margin=0.5), dict(margin=float("nan")), dict(margin=float("inf")), dict(chi=-0.1), dict(chi=float("nan")), dict(z_near=0.0),
                    dict(z_near=-1.0), dict(z_near=float("inf"))):
            with pytest.raises(vo.VoError) as e:
                wm.carve(s["map"], s["K"], s["T"], **bad)
            assert e.value.code == -1, bad
        with pytest.raises(ValueError):
            wm.carve(s["map"], s["K"], s["T"], radius=2)
        for Kb in ((0.0, 1.0, 0.0, 0.0), (1.0, -1.0, 0.0, 0.0), (1.0, 1.0, float("nan"), 0.0)):
            with pytest.raises(vo.VoError) as e:
                wm.carve(s["map"], Kb, s["T"])
            assert e.value.code == -1
        Tb = s["T"].copy()
        Tb[1, 3] = np.inf
        with pytest.raises(vo.VoError):
            wm.carve(s["map"], s["K"], Tb)
        big = {k: np.zeros((62, 203), v.dtype) for k, v in s["map"].items()}
        with pytest.raises(vo.VoError) as e:  # beyond vo_config.max_width x max_height
            wm.carve(big, s["K"], s["T"])
        assert e.value.code == -4
        after = (wm.points(max_free=ALL), wm.carveStats(), wm.stats())
        assert all(x.tobytes() == y.tobytes() for x, y in zip(before[0], after[0])) and before[1:] == after[1:]


def test_two_tables_and_clear(vo, sdw_ctx):  # noqa: F811
    ctx = sdw_ctx
    name = "m_vacated"
    ops = carve_ops(name)
    with ctx.semiDenseWorld(**CARVE_CASES[name]) as a, ctx.semiDenseWorld(**CARVE_CASES[name]) as b:
        _apply(a, ops, False)
        _apply(b, ops, False)
        ra, rb = _check(a, restated(name)), _check(b, restated(name))
        assert all(x.tobytes() == y.tobytes() for x, y in zip(ra, rb)) and (ra.free >= 1).any()
        a.clear()
        assert a.carveStats() == dict.fromkeys(CR.CCOUNTERS, 0) and len(a.points(max_free=ALL).free) == 0
        _apply(a, ops[2:3], True)  # the far plane alone after the clear: no free count survived in the slots' words
        assert not a.points(max_free=ALL).free.any()
        a.clear()
        _apply(a, ops, True)
        _check(a, restated(name))
    _check_n_clear = restated("n_clear")
    with ctx.semiDenseWorld(**CARVE_CASES["n_clear"]) as a:
        _apply(a, carve_ops("n_clear"), False)
        _check(a, _check_n_clear)


@pytest.mark.parametrize("voxel", [0.1, 0.2])
def test_guards_on_the_device_result(vo, voxel):
    """the guards of tests/test_semidense_world_carve.py on the device's own result, static scene and phantom, and the figures equal to
    the restatement's"""
    ctx = vo.Context(device=0, max_width=SW, max_height=SH, max_points=256, n_slots=2, max_level=0)
    try:
        (mp, T2), (alone, _), (m6, T6) = phantom_maps()
        prm = dict(GUARD, voxel=voxel)
        keys = np.unique(WR.points(alone, K, T2, None, **prm)[0]["key"])
        for phantom in (False, True):
            with ctx.semiDenseWorld(**prm) as wm:
                for m, T in ((mp if phantom else full_maps()[0][0], T2), (m6, T6)):
                    wm.integrate(m, K, T)
                    wm.carve(m, K, T)
                g = guard_shares(voxel, wm.points(max_free=ALL)._asdict(), keys if phantom else None)
                cs = wm.carveStats()
            print(g, cs)
            assert_guards(g)
            assert (g, cs) == guard_figures(voxel, phantom)
    finally:
        ctx.close()


# ---- 2. the driver --------------------------------------------------------------------------------------------------------------
def _run(vo, stream, mode, world, flush_every_frame=False, n_frames=N_FRAMES):  # noqa: F811
    """the stream through a driver with the static, temporal, propagation and regularisation options on and `world`, as
    tests/test_semidense_world_gpu.py runs it; the world map's records with `free` and every counter after the flush"""
    st, imgs, prm = stream
    if n_frames > len(imgs):
        imgs = [st.render_pair(p)[:2] for p in st.poses(n_frames)]
    sd = dict(prm, every="keyframe", temporal=dict(TPRM), propagate=dict(PPRM), regularize=dict(RPRM), world=dict(world))
    c, svo = _driver(vo, st, sd)
    try:
        infos, snaps, left, prev = [], [], [], None
        if mode == "sequence":
            got, _ = svo.runSequence([(L, R) for L, R in imgs])
            infos = [bytes(i) for i in got]
        else:
            for k in range(n_frames):
                if mode == "lookahead":
                    svo.enqueue(*imgs[k])
                    if k + 1 < n_frames:
                        svo.prefetch(*imgs[k + 1])
                    gi = svo.result()
                else:
                    gi = svo.trackStereoImages(*imgs[k])
                infos.append(bytes(gi))
                snap, reg, raw = _snapshot(svo)
                snaps.append(snap)
                if gi.is_keyframe and prev is not None and prev[0] is not None and not flush_every_frame:
                    left.append(prev)  # the map as it stood after the last frame before the keyframe change
                if flush_every_frame and gi.is_keyframe:
                    left.append((raw, reg))
                prev = (raw, reg)
                if flush_every_frame:
                    svo.flushSemiDenseWorld()
            if prev is not None and prev[0] is not None and not flush_every_frame:
                left.append(prev)
        svo.flushSemiDenseWorld()
        return dict(infos=infos, tracks={k: v.tobytes() for k, v in svo.getTracks().items()}, snaps=snaps, left=left, plain=svo.getSemiDenseWorld(),
                    rec=svo.getSemiDenseWorld(max_free=ALL), stats=svo.getSemiDenseWorldStats(), cstats=svo.getSemiDenseWorldCarveStats(),
                    rstats=svo.getSemiDenseWorldReanchorStats(), kfs=[T.tobytes() for T, _ in svo.getKeyframes()],
                    n_kf=sum(vo._capi.SvoFrameInfo.from_buffer_copy(b).is_keyframe for b in infos))
    finally:
        svo.close()
        c.close()


def _operator_fed(vo, run, world):
    """a fresh table of the same parameters fed the maps the driver returned, integrate and carve per keyframe in order"""
    c = vo.Context(device=0, max_width=SW, max_height=SH, max_points=256, n_slots=2, max_level=0)
    try:
        prm = {k: v for k, v in world.items() if k != "carve"}
        carve = {} if world["carve"] is True else world["carve"]
        with c.semiDenseWorld(**prm) as wm:
            for raw, _ in run["left"]:
                wm.integrate(raw, K, raw.T_wc)  # (no key plane: grey is not compared)
                wm.carve(raw, K, raw.T_wc, **carve)
            return wm.points(max_free=ALL), wm.carveStats()
    finally:
        c.close()


def _same_free(got, want):
    for k in ("index", "count", "keyframes", "free"):
        a, b = getattr(got, k), getattr(want, k)
        assert a.shape == b.shape and a.tobytes() == b.tobytes(), (k, a.shape, b.shape)


CARVE = dict(margin=2.0, chi=2.5, z_near=0.75)  # (not the defaults: the driver must carry the caller's)


@pytest.fixture(scope="module")
def off_run(vo, stream):  # noqa: F811
    return _run(vo, stream, "lookahead", WPRM)


@pytest.fixture(scope="module")
def on_run(vo, stream):  # noqa: F811
    return _run(vo, stream, "lookahead", dict(WPRM, carve=CARVE))


def test_driver_keeps_every_bit_and_equals_the_operator(vo, stream, off_run, on_run):  # noqa: F811
    on, off = on_run, off_run
    assert on["infos"] == off["infos"] and on["tracks"] == off["tracks"] and on["snaps"] == off["snaps"] and on["kfs"] == off["kfs"]
    _same_world(on["plain"], off["plain"])
    _same_world(on["rec"], off["plain"])  # every field but free
    assert on["stats"] == off["stats"] and on["rstats"] == off["rstats"]
    assert off["cstats"] == dict.fromkeys(CR.CCOUNTERS, 0) and not off["rec"].free.any()
    want, wc = _operator_fed(vo, on, dict(WPRM, carve=CARVE))
    _same_free(on["rec"], want)
    print(on["cstats"], "voxels", len(on["rec"].free), "with free", int((on["rec"].free >= 1).sum()))
    assert on["cstats"] == wc and wc["carves"] == on["n_kf"] == on["stats"]["integrations"] >= 3 and wc["visits"] > 100000


@pytest.mark.parametrize("mode", ["sync", "sequence"])
def test_driver_other_calling_modes(vo, stream, on_run, mode):  # noqa: F811
    run = _run(vo, stream, mode, dict(WPRM, carve=CARVE))
    assert run["infos"] == on_run["infos"] and run["tracks"] == on_run["tracks"]
    _same_world(run["rec"], on_run["rec"])
    _same_free(run["rec"], on_run["rec"])
    assert run["cstats"] == on_run["cstats"] and run["stats"] == on_run["stats"]


def test_driver_flush_then_keyframe_change_carves_once(vo, stream, off_run):  # noqa: F811
    world = dict(WPRM, carve=True)
    run = _run(vo, stream, "sync", world, flush_every_frame=True)
    assert run["infos"] == off_run["infos"]
    assert run["cstats"]["carves"] == run["stats"]["integrations"] == run["n_kf"] == len(run["left"])
    want, wc = _operator_fed(vo, run, world)  # (each keyframe's map as it stood right after its own frame)
    _same_free(run["rec"], want)
    assert run["cstats"] == wc


def test_driver_with_reanchoring(vo, stream):  # noqa: F811
    """min_move 0: the maps follow the local BA; a re-anchor does not re-carve, and the carve changes no field but free. 20 frames, as
    tests/test_semidense_world_reanchor_gpu.py runs the stream: within the first 10 the local BA moves no keyframe whose map is in."""
    ra = _run(vo, stream, "lookahead", dict(WPRM, reanchor=dict(min_move=0.0)), n_frames=20)
    both = _run(vo, stream, "lookahead", dict(WPRM, reanchor=dict(min_move=0.0), carve=True), n_frames=20)
    assert both["infos"] == ra["infos"] and both["snaps"] == ra["snaps"] and both["kfs"] == ra["kfs"]
    _same_world(both["rec"], ra["plain"])
    assert both["stats"] == ra["stats"] and both["rstats"] == ra["rstats"] and ra["rstats"]["reanchors"] >= 1
    assert both["cstats"]["carves"] == both["stats"]["integrations"] - both["rstats"]["reanchors"] == both["n_kf"]


def test_driver_off_and_on_and_errors(vo, stream):  # noqa: F811
    st, imgs, prm = stream
    assert not hasattr(vo.MonoVO, "setSemiDenseWorldCarve")  # a stereo driver's option (the C call refuses a mono driver's core)
    c, svo = _driver(vo, st, dict(prm, every="keyframe", temporal=dict(TPRM)))
    try:
        with pytest.raises(vo.VoError) as e:  # needs the world map
            svo.setSemiDenseWorldCarve(True)
        assert e.value.code == -1
        svo.setSemiDenseWorldCarve(None)  # (off is always accepted)
        with pytest.raises(vo.VoError):
            svo.getSemiDenseWorldCarveStats()
        n = C.c_longlong()
        count = lambda: (c.check(c.lib.vo_debug_allocation_count(c.handle, C.byref(n))), n.value)[1]
        svo.trackStereoImages(*imgs[0])
        svo.setSemiDenseWorld(dict(WPRM))
        n0 = count()
        for bad in (dict(margin=0.0), dict(chi=float("nan")), dict(z_near=0.0)):
            with pytest.raises(vo.VoError) as e:
                svo.setSemiDenseWorldCarve(bad)
            assert e.value.code == -1
        with pytest.raises(ValueError):
            svo.setSemiDenseWorldCarve(dict(radius=1))
        svo.setSemiDenseWorldCarve(True)
        svo.setSemiDenseWorldCarve(dict(CARVE))
        assert count() == n0  # enabling allocates nothing
        svo.enqueue(*imgs[1])
        for call in (lambda: svo.setSemiDenseWorldCarve(True), lambda: svo.setSemiDenseWorldCarve(None), svo.getSemiDenseWorldCarveStats,
                     lambda: svo.getSemiDenseWorld(max_free=ALL)):  # in flight
            with pytest.raises(vo.VoError) as e:
                call()
            assert e.value.code == -1
        svo.result()
        svo.flushSemiDenseWorld()
        svo.flushSemiDenseWorld()  # (the map is marked: nothing more)
        c1 = svo.getSemiDenseWorldCarveStats()
        assert c1["carves"] == 1 == svo.getSemiDenseWorldStats()["integrations"] and c1["rays"] > 1000
        svo.setSemiDenseWorldCarve(None)  # off: later integrations are not carved
        for k in range(2, 6):
            svo.trackStereoImages(*imgs[k])
        svo.flushSemiDenseWorld()
        assert svo.getSemiDenseWorldCarveStats() == c1 and svo.getSemiDenseWorldStats()["integrations"] >= 2
        svo.setSemiDenseWorldCarve(True)  # on again
        for k in range(6, N_FRAMES):
            svo.trackStereoImages(*imgs[k])
        svo.flushSemiDenseWorld()
        c2 = svo.getSemiDenseWorldCarveStats()
        assert c2["carves"] > c1["carves"] and len(svo.getSemiDenseWorld(max_free=ALL).free) == svo.getSemiDenseWorldStats()["occupied"]
        svo.clearSemiDenseWorld()
        assert svo.getSemiDenseWorldCarveStats() == dict.fromkeys(CR.CCOUNTERS, 0)
        svo.setSemiDenseWorld(None)  # the world map off takes the carve with it
        svo.setSemiDenseWorld(dict(WPRM))
        svo.flushSemiDenseWorld()
        assert svo.getSemiDenseWorldCarveStats()["carves"] == 0 and svo.getSemiDenseWorldStats()["integrations"] == 1
    finally:
        svo.close()
        c.close()


# ---- 3. the example ---------------------------------------------------------------------------------------------------------------
def test_sequence_runner_writes_free_into_the_world_ply(vo, tmp_path):
    """examples/run_stereo_sequence.py ... --semidense-world FILE.ply --semidense-world-carve: the PLY's rows, `free` behind
    `keyframes`, are the voxels the same loop gives in process; without the flag the file has today's header and rows"""
    import os
    import subprocess
    import sys
    from test_stereo_vo_gpu import _stream
    PIL = pytest.importorskip("PIL.Image")
    W, H, Kc = 640, 240, (400.0, 400.0, 320.0, 120.0)
    st, imgs = _stream(W, H, Kc, 20, 8, 9, 0.5, 7)
    dl, dr = tmp_path / "image_0", tmp_path / "image_1"
    dl.mkdir()
    dr.mkdir()
    for k, (L, R) in enumerate(imgs):
        PIL.fromarray(L).save(dl / f"{k:06d}.png")
        PIL.fromarray(R).save(dr / f"{k:06d}.png")
    T_lr = np.asarray(st.T_lr, np.float32)
    cam = lambda side: "".join(f"Camera.{side}.{k}: {v}\n" for k, v in (  # noqa: E731
        ("fx", Kc[0]), ("fy", Kc[1]), ("cx", Kc[2]), ("cy", Kc[3]), ("k1", 0.0), ("k2", 0.0), ("p1", 0.0), ("p2", 0.0), ("k3", 0.0),
        ("width", W), ("height", H)))
    cfg = tmp_path / "rig.yaml"
    cfg.write_text("%YAML:1.0\nflagDoUndistortion: 0\n" + cam("left") + cam("right") +
                   "T_lr: !!opencv-matrix\n  rows: 4\n  cols: 4\n  dt: f\n  data: [" + ",".join(repr(float(v)) for v in T_lr.reshape(-1)) + "]\n"
                   "feature_tracker.thres_error: 80.0\nfeature_tracker.thres_bidirection: 0.5\nfeature_tracker.thres_sampson: 60.0\n"
                   "feature_tracker.window_size: 21\nfeature_tracker.max_level: 4\nmap_update.thres_parallax: 1.0\n"
                   "feature_extractor.n_features: 2000\nfeature_extractor.n_bins_u: 20\nfeature_extractor.n_bins_v: 8\n"
                   "feature_extractor.thres_fastscore: 15.0\nfeature_extractor.radius: 5.0\nmotion_estimator.thres_1p_error: 120.0\n"
                   "motion_estimator.thres_5p_error: 1.0\nmotion_estimator.thres_poseba_error: 3.0\nkeyframe_update.thres_alive_ratio: 0.6\n"
                   "keyframe_update.thres_mean_parallax: 1.0\nkeyframe_update.thres_trans: 1.2\nkeyframe_update.thres_rotation: 15.0\n"
                   "keyframe_update.n_max_keyframes_in_window: 9\n")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    base = [sys.executable, os.path.join(root, "examples", "run_stereo_sequence.py"), "--config", str(cfg), "--left", str(dl), "--right", str(dr),
            "--trajectory", str(tmp_path / "traj.txt"), "--semidense", str(tmp_path / "sd"), "--semidense-temporal", "--semidense-voxel", "0.2"]
    plain, carved = tmp_path / "map.ply", tmp_path / "map_free.ply"
    r = subprocess.run(base + ["--semidense-world", str(plain)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "world map carving" not in r.stdout, r.stdout[-1500:] + r.stderr[-1500:]
    r = subprocess.run(base + ["--semidense-world", str(carved), "--semidense-world-carve", "--semidense-world-max-free", "1", "1"],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "world map carving:" in r.stdout, r.stdout[-1500:] + r.stderr[-1500:]
    r = subprocess.run(base + ["--semidense-world", str(carved), "--semidense-world-max-free", "0", "1"], capture_output=True, text=True, timeout=600)
    assert r.returncode != 0 and "--semidense-world-carve" in r.stderr  # (refused while the arguments are read: nothing runs)
    svo = vo.StereoVO.from_yaml(str(cfg), semidense=dict(z_min=3.0, every="keyframe", temporal=True, world=dict(voxel=0.2, carve=True)))
    try:
        for L, R in imgs:
            svo.trackStereoImages(L, R)
        svo.flushSemiDenseWorld()
        w, kept = svo.getSemiDenseWorld(max_free=ALL), svo.getSemiDenseWorld(max_free=(1, 1))
    finally:
        svo.close()
    row = lambda v: [f"{x:.6g} {y:.6g} {z:.6g} {int(g)} {int(c)} {int(k)}" for (x, y, z), g, c, k in zip(v.xyz, v.grey, v.count, v.keyframes)]  # noqa: E731
    head = lambda v: ["ply", "format ascii 1.0", f"element vertex {len(v.xyz)}", "property float x", "property float y", "property float z", "property uchar grey",
                      "property uint count", "property uint keyframes"]  # noqa: E731
    assert len(w.xyz) > 1000 and plain.read_text().splitlines() == head(w) + ["end_header"] + row(w)  # today's format, line for line
    assert carved.read_text().splitlines() == head(kept) + ["property uint free", "end_header"] + [f"{r} {int(f)}" for r, f in zip(row(kept), kept.free)]
    assert 0 < len(kept.xyz) <= len(w.xyz) and (kept.free <= kept.count).all()
