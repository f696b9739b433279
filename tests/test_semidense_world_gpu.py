"""The world-frame voxel map on the device (include/vo_hip.h, "Semi-dense world map") against the numpy restatement
(tests/semidense_world_restatement.py), everything bit for bit after the canonical sort by key: the operator on the restatement
test's cases — host planes and device planes with a padded key stride, the pre-aggregated kernel form and the simple one —, two fresh
tables fed alike, clear and the same input again, the extraction's capacity, its argument errors, the guards on the full 640 x 240
maps; and StereoVO's option through the look-ahead calls, the synchronous call and runSequence: the odometry, the static result, the
map, its origin and the regularised planes the same bits as without it, the world map after the flush equal to the operator fed the
maps the driver itself returned before each keyframe change (raw and regularised), no keyframe integrated twice, the option switched
off and on, the refusals; and the sequence example's PLY against the same loop in process. None of the entry points exists without
the feature."""
import ctypes as C

import numpy as np
import pytest

import semidense_world_restatement as WR
from test_semidense_propagate_gpu import PPRM
from test_semidense_temporal_gpu import K, N_FRAMES, SH, SW, TPRM, _driver
from test_semidense_world import BASE, CASES, case_steps, full_maps, restated, same_records, surface_distance
from util import DeviceBuffer

pytestmark = pytest.mark.gpu

F = np.float32
VO_DBG_SDW_FORM = 10
WPRM = dict(voxel=0.1, capacity_log2=20, min_obs=1, z_max=30.0)  # (not the defaults: the driver must carry the caller's)
RPRM = dict(chi=2.5, fill_min=6)


@pytest.fixture(scope="module")
def sdw_ctx(vo):
    c = vo.Context(device=0, max_width=203, max_height=61, max_points=256, n_slots=2, max_level=0)
    yield c
    c.close()


def _feed(ctx, wm, steps, device):
    for s in steps:
        h, w = s["map"]["invd"].shape
        if not device:
            wm.integrate(s["map"], s["K"], s["T"], key=s["Lk"])
            continue
        bufs = [DeviceBuffer(np.ascontiguousarray(s["map"][k])) for k in ("invd", "sigma", "n_obs")]
        dkey = None
        if s["Lk"] is not None:
            padded = np.full((h, w + 5), 0xEE, np.uint8)
            padded[:, :w] = s["Lk"]
            dkey = DeviceBuffer(padded)
        try:
            wm.integrate(dict(zip(("invd", "sigma", "n_obs"), (b.data_ptr() for b in bufs))), s["K"], s["T"], key=None if dkey is None else dkey.data_ptr(),
                         on_device=(w, h), key_on_device=None if dkey is None else w + 5)
        finally:
            for b in bufs + ([] if dkey is None else [dkey]):
                b.free()


def _check(wm, name):
    w, want, _ = restated(name)
    got = wm.points()
    ok, where = same_records(got._asdict(), want, fields=("index", "sums", "count", "keyframes", "weight", "grey", "xyz"))
    assert ok, (name, where)
    assert wm.stats() == w.stats, (name, wm.stats(), w.stats)
    return got


# ---- 1. the operator ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(CASES))
def test_operator_equals_restatement(vo, sdw_ctx, name):
    ctx = sdw_ctx
    steps = case_steps(name)
    try:
        for form in (0, 1):
            ctx.debug_set(VO_DBG_SDW_FORM, form)
            for device in (False, True):
                with ctx.semiDenseWorld(**CASES[name]) as wm:
                    _feed(ctx, wm, steps, device)
                    _check(wm, name)
    finally:
        ctx.debug_set(VO_DBG_SDW_FORM, 0)


def test_two_tables_clear_and_capacity(vo, sdw_ctx):
    ctx = sdw_ctx
    name = "a_203x61"
    steps = case_steps(name)
    w, want, _ = restated(name)
    with ctx.semiDenseWorld(**CASES[name]) as a, ctx.semiDenseWorld(**CASES[name]) as b:
        _feed(ctx, a, steps, False)
        _feed(ctx, b, steps, False)
        ra, rb = _check(a, name), _check(b, name)
        for x, y in zip(ra, rb):
            assert x.tobytes() == y.tobytes()
        a.clear()
        assert a.stats() == dict.fromkeys(WR.COUNTERS, 0) | {"capacity": 1 << CASES[name]["capacity_log2"]} and len(a.points().xyz) == 0
        _feed(ctx, a, steps, True)
        _check(a, name)
        # min_count / min_keyframes, and a capacity below the count: the true count, the first records in key order
        for mc, mk in ((1, 2), (3, 1), (2, 2)):
            sel = (want["count"] >= mc) & (want["keyframes"] >= mk)
            got = a.points(min_count=mc, min_keyframes=mk)
            assert sel.sum() >= 10 and np.array_equal(got.sums, want["sums"][sel]) and np.array_equal(got.xyz.view(np.uint32), want["xyz"][sel].view(np.uint32))
        n_all = len(want["key"])
        with pytest.raises(vo.VoError) as e:
            a.points(capacity=10)
        assert e.value.code == -8 and e.value.n == n_all
        n = C.c_int()
        xyz, cnt = np.full((11, 3), -7, F), np.full(11, 77, np.uint32)
        rc = ctx.lib.vo_semidense_world_points(a._h, 1, 1, 10, None, xyz.ctypes.data, None, cnt.ctypes.data, None, None, None, C.byref(n))
        assert rc == -8 and n.value == n_all
        assert np.array_equal(xyz[:10].view(np.uint32), want["xyz"][:10].view(np.uint32)) and (xyz[10] == -7).all()
        assert np.array_equal(cnt[:10], want["count"][:10]) and cnt[10] == 77
        assert ctx.lib.vo_semidense_world_points(a._h, 1, 1, 0, None, None, None, None, None, None, None, C.byref(n)) == -8 and n.value == n_all
        for bad in ((0, 1), (1, 0)):
            assert ctx.lib.vo_semidense_world_points(a._h, *bad, 0, None, None, None, None, None, None, None, C.byref(n)) == -1


def test_operator_argument_errors(vo, sdw_ctx):
    ctx = sdw_ctx
    for bad in (dict(voxel=0.0), dict(voxel=-1.0), dict(voxel=float("nan")), dict(voxel=float("inf")), dict(capacity_log2=9), dict(capacity_log2=29),
                dict(min_obs=0), dict(min_obs=256), dict(z_max=0.0), dict(z_max=float("inf")), dict(z_max=float("nan"))):
        with pytest.raises(vo.VoError) as e:
            ctx.semiDenseWorld(**dict(BASE, **bad))
        assert e.value.code == -1, bad
    with pytest.raises(ValueError):
        ctx.semiDenseWorld(radius=2)
    s = case_steps("c_97x45_plane")[0]
    with ctx.semiDenseWorld(**dict(BASE, capacity_log2=10)) as wm:
        before = wm.stats()
        for Kb in ((0.0, 1.0, 0.0, 0.0), (1.0, -1.0, 0.0, 0.0), (1.0, 1.0, float("nan"), 0.0)):
            with pytest.raises(vo.VoError) as e:
                wm.integrate(s["map"], Kb, s["T"], key=s["Lk"])
            assert e.value.code == -1
        Tb = s["T"].copy()
        Tb[1, 3] = np.inf
        with pytest.raises(vo.VoError):
            wm.integrate(s["map"], s["K"], Tb)
        big = {k: np.zeros((62, 203), v.dtype) for k, v in s["map"].items()}
        with pytest.raises(vo.VoError) as e:  # beyond vo_config.max_width x max_height
            wm.integrate(big, s["K"], s["T"])
        assert e.value.code == -4
        with pytest.raises(ValueError):
            wm.integrate(s["map"], s["K"], s["T"], key=s["Lk"][:, :50])
        assert wm.stats() == before  # none of them took a sequence number or touched the table
        wm.integrate(s["map"], s["K"], s["T"], key=s["Lk"])  # 97 x 45 = 4 365 > 512: refused on the device
        assert wm.stats() == dict(before, refused=1) and len(wm.points().xyz) == 0


def test_guards_on_the_device_result(vo):
    """what a user has today — the concatenated per-keyframe clouds of the same min_obs and z_max — against the voxel map, at the
    three voxel sizes DESIGN.md §24 quotes: fewer voxels than points, and a larger share of the two-keyframe voxels within one voxel
    edge of the corridor's surface than of the clouds' points"""
    ctx = vo.Context(device=0, max_width=SW, max_height=SH, max_points=256, n_slots=2, max_level=0)
    try:
        cloud = []
        for m, L, T in full_maps():
            cam, _, _ = ctx.semiDenseMapPoints(m["invd"], m["sigma"], m["n_obs"], K=K, min_obs=1)
            wld, _, _ = ctx.semiDenseMapPoints(m["invd"], m["sigma"], m["n_obs"], K=K, T=T, min_obs=1)
            cloud.append(wld[cam[:, 2] <= F(30.0)])
        cloud = np.concatenate(cloud)
        for voxel in (0.05, 0.1, 0.2):
            with ctx.semiDenseWorld(**dict(BASE, voxel=voxel, capacity_log2=20)) as wm:
                for m, L, T in full_maps():
                    wm.integrate(m, K, T, key=L)
                r1, r2 = wm.points(), wm.points(min_keyframes=2)
            share = lambda xyz: float((surface_distance(xyz) <= voxel).mean())
            print(voxel, dict(points=len(cloud), voxels=len(r1.xyz), voxels_kf2=len(r2.xyz), share_cloud=share(cloud), share_kf2=share(r2.xyz)))
            assert len(r1.xyz) < len(cloud)
            assert share(r2.xyz) > share(cloud)
    finally:
        ctx.close()


# ---- 2. the driver --------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def stream():
    from visual_odometry_ros_amd import synthetic as S
    st = S.StereoStream(width=SW, height=SH, K=K, n_u=20, n_v=8, seed=2, speed=0.5)
    imgs = [st.render_pair(p)[:2] for p in st.poses(N_FRAMES)]
    bf = float(F(K[0] * st.baseline))
    return st, imgs, dict(bf=bf, d_min=0, d_max=67)


def _snapshot(svo):
    """every semi-dense result of the driver as bytes"""
    out = []
    sd = svo.getSemiDense()
    out.append(None if sd is None else b"".join(np.ascontiguousarray(v).tobytes() for v in sd[:4]) + bytes([sd.frame_id & 255]))
    m = svo.getSemiDenseMap()
    out.append(None if m is None else b"".join(getattr(m, p).tobytes() for p in ("invd", "sigma", "n_obs", "tstatus")) + m.T_wc.tobytes())
    o = svo.getSemiDenseOrigin()
    out.append(None if o is None else o[0].tobytes())
    r = svo.getSemiDenseMap(regularized=True)
    out.append(None if r is None else b"".join(getattr(r, p).tobytes() for p in ("invd", "sigma", "n_obs", "rstatus")))
    return out, (r if r is not None else None), m


def _run_world(vo, stream, mode, world, flush_every_frame=False, snapshots=True):
    """the stream through a driver with the static, temporal, propagation and regularisation options on and `world` (None: off);
    returns infos (bytes), the final tracks, per-frame snapshots, the maps that left (raw, regularised, key image) in order, and the
    world map's records and stats after the flush"""
    st, imgs, prm = stream
    sd = dict(prm, every="keyframe", temporal=dict(TPRM), propagate=dict(PPRM), regularize=dict(RPRM))
    if world is not None:
        sd["world"] = dict(world)
    c, svo = _driver(vo, st, sd)
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
                if snapshots or flush_every_frame:
                    snap, reg, raw = _snapshot(svo)
                    snaps.append(snap)
                    if gi.is_keyframe and prev is not None and prev[0] is not None and not flush_every_frame:
                        left.append(prev)  # the map as it stood after the last frame before the keyframe change
                    if flush_every_frame and gi.is_keyframe:
                        left.append((raw, reg))
                    prev = (raw, reg)
                if flush_every_frame and world is not None:
                    svo.flushSemiDenseWorld()
            if prev is not None and prev[0] is not None and not flush_every_frame:
                left.append(prev)
        rec = stats = None
        if world is not None:
            svo.flushSemiDenseWorld()
            rec, stats = svo.getSemiDenseWorld(), svo.getSemiDenseWorldStats()
        g = svo.getTracks()
        return dict(infos=infos, tracks={k: v.tobytes() for k, v in g.items()}, snaps=snaps, left=left, rec=rec, stats=stats,
                    n_kf=sum(vo._capi.SvoFrameInfo.from_buffer_copy(b).is_keyframe for b in infos),
                    index={vo._capi.SvoFrameInfo.from_buffer_copy(b).frame_id: k for k, b in enumerate(infos)})
    finally:
        svo.close()
        c.close()


def _operator_fed(vo, stream, run, which, world):
    """a fresh table of the same parameters fed the maps in order, with each map's own T_wc and its keyframe's left image"""
    _, imgs, _ = stream
    c = vo.Context(device=0, max_width=SW, max_height=SH, max_points=256, n_slots=2, max_level=0)
    try:
        prm = {k: v for k, v in world.items() if k != "source"}
        with c.semiDenseWorld(**prm) as wm:
            for raw, reg in run["left"]:
                m = raw if which == "raw" else reg
                wm.integrate(m, K, raw.T_wc, key=imgs[run["index"][raw.frame_id]][0])
            return wm.points(), wm.stats()
    finally:
        c.close()


def _same_world(got, want):
    for k in ("index", "xyz", "weight", "count", "keyframes", "grey"):
        a, b = getattr(got, k), getattr(want, k)
        assert a.shape == b.shape and a.tobytes() == b.tobytes(), (k, a.shape, b.shape)


@pytest.fixture(scope="module")
def off_run(vo, stream):
    return _run_world(vo, stream, "lookahead", None)


@pytest.fixture(scope="module")
def lookahead_run(vo, stream):
    return _run_world(vo, stream, "lookahead", WPRM)


def test_driver_keeps_every_bit_and_equals_the_operator(vo, stream, off_run, lookahead_run):
    on, off = lookahead_run, off_run
    assert on["infos"] == off["infos"] and on["tracks"] == off["tracks"]
    assert on["snaps"] == off["snaps"] and any(s[1] is not None and s[2] is not None and s[3] is not None for s in on["snaps"])
    assert on["n_kf"] >= 3 and len(on["left"]) == on["n_kf"]
    assert [raw.frame_id for raw, _ in on["left"]] == sorted({raw.frame_id for raw, _ in on["left"]})
    want, wstats = _operator_fed(vo, stream, on, "raw", WPRM)
    _same_world(on["rec"], want)
    assert on["stats"] == wstats and on["stats"]["integrations"] == on["n_kf"] and on["stats"]["refused"] == 0
    assert (on["rec"].keyframes >= 2).sum() >= 100 and len(on["rec"].xyz) > 10000


def test_driver_synchronous_regularised_source(vo, stream, off_run):
    world = dict(WPRM, source="regularized")
    on = _run_world(vo, stream, "sync", world)
    assert on["infos"] == off_run["infos"] and on["tracks"] == off_run["tracks"] and on["snaps"] == off_run["snaps"]
    want, wstats = _operator_fed(vo, stream, on, "regularized", world)
    _same_world(on["rec"], want)
    assert on["stats"] == wstats and on["stats"]["integrations"] == on["n_kf"]


def test_driver_run_sequence(vo, stream, off_run, lookahead_run):
    on = _run_world(vo, stream, "sequence", WPRM)
    assert on["infos"] == off_run["infos"] and on["tracks"] == off_run["tracks"]
    _same_world(on["rec"], lookahead_run["rec"])
    assert on["stats"] == lookahead_run["stats"]


def test_driver_flush_then_keyframe_change_integrates_once(vo, stream, off_run):
    on = _run_world(vo, stream, "sync", WPRM, flush_every_frame=True)
    assert on["infos"] == off_run["infos"]
    assert on["stats"]["integrations"] == on["n_kf"] == len(on["left"]) and on["stats"]["refused"] == 0
    want, wstats = _operator_fed(vo, stream, on, "raw", WPRM)  # (each keyframe's map as it stood right after its own frame)
    _same_world(on["rec"], want)
    assert on["stats"] == wstats


def test_driver_off_and_on_and_errors(vo, stream):
    st, imgs, prm = stream
    c, svo = _driver(vo, st)
    try:
        assert not hasattr(vo.MonoVO, "setSemiDenseWorld")  # a stereo driver's option (the C call refuses a mono driver's core)
        svo.setSemiDense(dict(prm))
        with pytest.raises(vo.VoError) as e:  # needs the temporal option
            svo.setSemiDenseWorld(dict(WPRM))
        assert e.value.code == -1
        svo.setSemiDenseTemporal(dict(TPRM))
        for call in (svo.getSemiDenseWorld, svo.getSemiDenseWorldStats, svo.flushSemiDenseWorld, svo.clearSemiDenseWorld):  # the option is off
            with pytest.raises(vo.VoError):
                call()
        with pytest.raises(vo.VoError):  # the regularised source needs the regularise option
            svo.setSemiDenseWorld(dict(WPRM, source="regularized"))
        with pytest.raises(ValueError):
            svo.setSemiDenseWorld(dict(WPRM, source="smoothed"))
        with pytest.raises(ValueError):
            svo.setSemiDenseWorld(dict(WPRM, radius=1))
        with pytest.raises(vo.VoError):
            svo.setSemiDenseWorld(dict(WPRM, capacity_log2=9))
        n = C.c_longlong()
        count = lambda: (c.check(c.lib.vo_debug_allocation_count(c.handle, C.byref(n))), n.value)[1]
        svo.trackStereoImages(*imgs[0])
        n0 = count()
        svo.setSemiDenseWorld(dict(WPRM))
        assert count() == n0 + 1  # the option's only allocation
        svo.setSemiDenseWorld(dict(WPRM))
        with pytest.raises(vo.VoError):  # capacity_log2 is fixed by the first enable
            svo.setSemiDenseWorld(dict(WPRM, capacity_log2=21))
        assert count() == n0 + 1 and svo.getSemiDenseWorldStats()["integrations"] == 0 and len(svo.getSemiDenseWorld().xyz) == 0
        svo.enqueue(*imgs[1])
        for call in (lambda: svo.setSemiDenseWorld(None), lambda: svo.setSemiDenseWorld(dict(WPRM)), svo.getSemiDenseWorld, svo.getSemiDenseWorldStats,
                     svo.flushSemiDenseWorld, svo.clearSemiDenseWorld):  # in flight
            with pytest.raises(vo.VoError) as e:
                call()
            assert e.value.code == -1
        svo.result()
        n1 = count()
        svo.flushSemiDenseWorld()
        svo.flushSemiDenseWorld()  # (the map is marked: nothing more)
        st1 = svo.getSemiDenseWorldStats()
        assert st1["integrations"] == 1 and st1["inserted"] > 1000 and st1["occupied"] == len(svo.getSemiDenseWorld().xyz)
        svo.setSemiDenseWorld(None)  # off: the table stays, nothing is integrated
        for k in range(2, 6):
            svo.trackStereoImages(*imgs[k])
        with pytest.raises(vo.VoError):
            svo.getSemiDenseWorldStats()
        svo.setSemiDenseWorld(dict(WPRM))  # on again: the same table; the current keyframe's map has not been integrated yet
        assert svo.getSemiDenseWorldStats() == st1
        svo.flushSemiDenseWorld()
        st2 = svo.getSemiDenseWorldStats()
        assert st2["integrations"] == 2 and st2["occupied"] > st1["occupied"]
        svo.setSemiDenseWorld(dict(WPRM, voxel=0.2))  # another voxel: the old sums mean nothing, the table is cleared
        assert svo.getSemiDenseWorldStats()["occupied"] == 0
        svo.flushSemiDenseWorld()
        assert svo.getSemiDenseWorldStats()["integrations"] == 1
        svo.clearSemiDenseWorld()
        assert svo.getSemiDenseWorldStats()["integrations"] == 0 and len(svo.getSemiDenseWorld().xyz) == 0
        assert count() >= n1  # (the getters' scratch may have grown; the table was allocated once)
    finally:
        svo.close()
        c.close()


# ---- 3. the example ---------------------------------------------------------------------------------------------------------------
def test_sequence_runner_writes_the_world_ply(vo, tmp_path):
    """examples/run_stereo_sequence.py --semidense DIR --semidense-temporal --semidense-world FILE.ply: PNG pairs on disk and a
    configuration file -> one PLY whose rows are the voxels the same loop gives in process after its flush"""
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
    ply = tmp_path / "map.ply"
    r = subprocess.run([sys.executable, os.path.join(root, "examples", "run_stereo_sequence.py"), "--config", str(cfg), "--left", str(dl),
                        "--right", str(dr), "--trajectory", str(tmp_path / "traj.txt"), "--semidense", str(tmp_path / "sd"), "--semidense-temporal",
                        "--semidense-world", str(ply), "--semidense-voxel", "0.2"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "world map:" in r.stdout, r.stdout[-1500:] + r.stderr[-1500:]
    svo = vo.StereoVO.from_yaml(str(cfg), semidense=dict(z_min=3.0, every="keyframe", temporal=True, world=dict(voxel=0.2)))
    try:
        n_kf = sum(int(svo.trackStereoImages(L, R).is_keyframe) for L, R in imgs)
        svo.flushSemiDenseWorld()
        w, stats = svo.getSemiDenseWorld(), svo.getSemiDenseWorldStats()
    finally:
        svo.close()
    lines = ply.read_text().splitlines()
    assert stats["integrations"] >= 2 and stats["integrations"] <= n_kf and len(w.xyz) > 1000
    assert lines[2] == f"element vertex {len(w.xyz)}" and lines[9] == "end_header" and len(lines) == 10 + len(w.xyz)
    want = [f"{x:.6g} {y:.6g} {z:.6g} {int(g)} {int(c)} {int(k)}" for (x, y, z), g, c, k in zip(w.xyz, w.grey, w.count, w.keyframes)]
    assert lines[10:] == want
