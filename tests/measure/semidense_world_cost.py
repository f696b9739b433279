"""What the world-frame voxel map (vo_semidense_world_*, vo_svo_set_semidense_world) costs on one MI355X, at
1241 x 376 with bf = 386.1, voxel 0.1 m, min_obs 1, z_max 40 m:
  launch       the map of the stream's third pair — its static result, fused with the next three left images by the device's own
               operators — integrated, every plane on the device: the launch between two events on the stream (the context's
               profiler), one launch at a time, for the pre-aggregated kernel form and the simple one (vo_debug_set(VO_DBG_SDW_FORM)),
               into an EMPTY table (every voxel claims its slot; the table is cleared in front of each launch) and AGAIN into the
               table that holds the map's voxels already (every probe finds its key). With the counts the restatement gives: points,
               distinct voxels, distinct voxels per workgroup of 1024 raster indices summed over the workgroups, and the global
               atomics per launch that follow from them (per global update one compare-and-swap per probed slot — counted as one —,
               four or five 64-bit adds, a 32-bit add, a 32-bit max and at most one more 32-bit add).
  load         the same launch (again into a table that holds the voxels) with 2^24 slots filled to a load of 0.1 and of 0.45 by
               the same map integrated under poses shifted by multiples of 150 m.
  extraction   vo_semidense_world_points of that table once it holds a million voxels or more: the whole call, compaction, copy
               and host sort included.
  loops        the stereo loop at BASELINE configs[1] (the stream and settings of pose_covariance_cost.py, device images), per
               frame: static per keyframe + temporal, against the same with the world map on, through
                 sync        one trackStereoImages call per frame
                 look_ahead  result k, enqueue k + 1, prefetch k + 2, call by call from Python
The settings ALTERNATE within one run, every repeat on a fresh context; reported: median and min..max over the repeats.
Measurement tool, not a test.
usage: python tests/measure/semidense_world_cost.py [--frames 80] [--repeats 5] [--no-load]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from pose_covariance_cost import WARM, Stereo  # noqa: E402
from semidense_regularize_cost import BF, K_AUX, Z_MIN, fused_map, stats  # noqa: E402

VO_DBG_SDW_FORM = 10
WPRM = dict(voxel=0.1, min_obs=1, z_max=40.0)
FORMS = (("aggregated", 0), ("simple", 1))


def counts(m, cfg, T_wk):
    """points, distinct voxels, and distinct voxels per workgroup summed, by the restatement"""
    import semidense_world_restatement as WR
    P, n_skip, n_oor = WR.points(m, cfg.K, T_wk, None, **WPRM, capacity_log2=22)
    h, w = m["invd"].shape
    block = (P["y"].astype(np.int64) * w + P["x"]) // 1024
    per_wg = len(np.unique(np.stack([block.astype(np.uint64), P["key"]], -1), axis=0))
    n, d = len(P["key"]), len(np.unique(P["key"]))
    per_update = 1 + 5 + 2  # compare-and-swap, five 64-bit adds (sg too: a key plane is given), 32-bit add and max
    return dict(entries=int(WR.entries(m).sum()), points=n, skipped=n_skip, out_of_range=n_oor, distinct_voxels=d, points_per_voxel=round(n / d, 3),
                distinct_per_workgroup_sum=per_wg, points_per_distinct_voxel_per_workgroup=round(n / per_wg, 3),
                global_atomics_simple=n * per_update + d, global_atomics_aggregated=per_wg * per_update + d)


def timed(c, call, n):
    c.profile_set_classes(1 << K_AUX)
    t = []
    for _ in range(n):
        c.profile_reset()
        call()
        k, ms = c.profile_get(K_AUX)
        assert k == 1
        t.append(1e3 * ms)
    c.profile_set_classes(1 << 0)  # (the profiler cannot be switched off: a class these launches are not in)
    return t


def launch(vo, DeviceBuffer, cfg, repeats, load, batch=20):
    F = np.float32
    La = cfg.imgs[2][0]
    h, w = La.shape
    out = {"pixels": int(h * w)}
    T_wk = np.asarray(cfg.st.poses(7)[2], F)
    with vo.Context(device=0, max_width=w, max_height=h, max_points=256, n_slots=2, max_level=0) as c:
        m, _ = fused_map(vo, c, cfg, 5)
        out["counts"] = counts(m, cfg, T_wk)
        bufs = {k: DeviceBuffer(np.ascontiguousarray(v)) for k, v in m.items()}
        dkey = DeviceBuffer(La)
        planes = {k: b.data_ptr() for k, b in bufs.items()}
        try:
            c.profile_enable(4)
            with c.semiDenseWorld(**WPRM, capacity_log2=22) as wm:
                call = lambda T=T_wk: wm.integrate(planes, cfg.K, T, key=dkey.data_ptr(), on_device=(w, h), key_on_device=w)

                def fresh():
                    wm.clear()
                    call()
                ref = None
                for name, form in FORMS:
                    c.debug_set(VO_DBG_SDW_FORM, form)
                    fresh()
                    rec = wm.points()
                    assert len(rec.xyz) == out["counts"]["distinct_voxels"] and int(rec.count.sum()) == out["counts"]["points"]
                    ref = rec if ref is None else ref
                    assert all(a.tobytes() == b.tobytes() for a, b in zip(rec, ref))  # (both forms: the same table)
                    out[name] = {"empty_table_us": stats(timed(c, fresh, repeats * batch), 2), "again_us": stats(timed(c, call, repeats * batch), 2)}
                    t_call = []
                    for _ in range(repeats):
                        t0 = time.perf_counter()
                        for _k in range(batch):
                            call()
                        t_call.append(1e6 * (time.perf_counter() - t0) / batch)
                    out[name]["whole_call_us"] = stats(t_call, 1)
            if load:
                with c.semiDenseWorld(**WPRM, capacity_log2=24) as wm:
                    cap = 1 << 24
                    call = lambda T: wm.integrate(planes, cfg.K, T, key=dkey.data_ptr(), on_device=(w, h), key_on_device=w)
                    c.debug_set(VO_DBG_SDW_FORM, 0)
                    k, res, ext = 0, {}, None
                    for target in (0.1, 0.45):
                        while wm.stats()["occupied"] < target * cap:
                            T = T_wk.copy()
                            T[0, 3] += 150.0 * (k % 600 - 300)
                            T[2, 3] += 150.0 * (k // 600)
                            k += 1
                            call(T)
                            assert wm.stats()["refused"] == 0
                        st = wm.stats()
                        res[f"load_{target}"] = {"occupied": st["occupied"], "load": round(st["occupied"] / cap, 4), "integrations": st["integrations"]}
                        for name, form in FORMS:
                            c.debug_set(VO_DBG_SDW_FORM, form)
                            res[f"load_{target}"][name + "_again_us"] = stats(timed(c, lambda: call(T), repeats * batch), 2)
                        if ext is None and st["occupied"] >= 1000000:  # the extraction, once: the whole call with room for every record
                            n = st["occupied"]
                            xyz, cnt = np.zeros((n, 3), F), np.zeros(n, np.uint32)
                            kf, grey, nn = np.zeros(n, np.uint32), np.zeros(n, np.uint8), C.c_int()
                            t = []
                            for _ in range(max(repeats, 3)):
                                t0 = time.perf_counter()
                                rc = c.lib.vo_semidense_world_points(wm._h, 1, 1, n, None, xyz.ctypes.data, None, cnt.ctypes.data, kf.ctypes.data,
                                                                     grey.ctypes.data, None, C.byref(nn))
                                t.append(1e3 * (time.perf_counter() - t0))
                                assert rc == 0 and nn.value == n
                            ext = {"voxels": n, "whole_call_ms": stats(t, 2)}
                    out["load_2^24"] = res
                    out["extraction"] = ext
        finally:
            c.debug_set(VO_DBG_SDW_FORM, 0)
            dkey.free()
            for b in bufs.values():
                b.free()
    return out


def one_run(vo, cfg, mode, setting):
    src, n = cfg.src, len(cfg.src)
    n_kf = 0
    with cfg.context(vo) as c:
        o, _ = cfg.make(vo, c, False)
        o.setSemiDense(dict(bf=BF, z_min=Z_MIN), every="keyframe")
        o.setSemiDenseTemporal({})
        if setting == "world":
            o.setSemiDenseWorld(dict(WPRM))  # (the default 2^22 slots)
        t0 = None
        if mode == "sync":
            for k in range(n):
                if k == WARM:
                    t0 = time.perf_counter()
                n_kf += int(cfg.track(o, src[k]).is_keyframe)
        else:
            cfg.enqueue(o, src[0])
            cfg.prefetch(o, src[1])
            for k in range(n):
                if k == WARM:
                    t0 = time.perf_counter()
                n_kf += int(o.result().is_keyframe)
                if k + 1 < n:
                    cfg.enqueue(o, src[k + 1])
                    if k + 2 < n:
                        cfg.prefetch(o, src[k + 2])
        o.getSemiDenseMap()  # (the last launch belongs to the run)
        dt = time.perf_counter() - t0
        st = o.getSemiDenseWorldStats() if setting == "world" else None
        o.close()
    return 1e3 * dt / (n - WARM), n_kf, st


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=80)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--no-load", action="store_true")
    a = ap.parse_args()
    import visual_odometry_ros_amd as vo
    from visual_odometry_ros_amd import synthetic as S
    from util import DeviceBuffer
    cfg = Stereo(S, a.frames)
    out = {"launch_1241x376": launch(vo, DeviceBuffer, cfg, a.repeats, not a.no_load)}
    print(json.dumps(out), flush=True)
    cfg.upload(DeviceBuffer)
    res = {}
    try:
        for mode in ("sync", "look_ahead"):
            one_run(vo, cfg, mode, "world")  # (untimed: code objects loaded, clocks up)
            t = {"temporal": [], "world": []}
            for _ in range(a.repeats):
                for s in t:
                    ms, n_kf, st = one_run(vo, cfg, mode, s)
                    t[s].append(ms)
                    if st:
                        res.setdefault("world_stats", st)
            res[mode] = {s: stats(v) for s, v in t.items()}
            res[mode]["keyframes"] = n_kf
    finally:
        cfg.free()
    out["stereo_configs1"] = res
    out["unit"] = "loops: ms per frame; launch: us"
    out["frames_timed"], out["repeats"] = a.frames - WARM, a.repeats
    print(json.dumps(out))


if __name__ == "__main__":
    main()
