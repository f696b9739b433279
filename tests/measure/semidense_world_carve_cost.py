"""What free-space carving on the world-frame voxel map (vo_semidense_world_carve, vo_svo_set_semidense_world_carve)
costs on one MI355X, at 1241 x 376 with bf = 386.1, voxel 0.1 m, min_obs 1, z_max 40 m, the default carve parameters, in the form of
semidense_world_reanchor_cost.py:
  launch       the map of semidense_world_cost.py (the stream's third pair fused with the next three left images), every plane on the
               device: the carve alone between two events on the stream (the context's profiler), both kernel forms (VO_DBG_SDW_FORM),
               in a table of 2^22 slots that holds that map alone and in one of 2^20 slots loaded to about 0.45 (the map in strips of
               32 rows at poses a few metres apart, until the table refuses); next to it the integration launch of the same map, the
               yardstick. Visits, hits and rays of one carve from the counters.
  loops        the stereo loop at BASELINE configs[1] (the stream and settings of semidense_world_cost.py, device images), per frame:
               static per keyframe + temporal + world map, against THE SAME RUN with the carving on, through
                 sync        one trackStereoImages call per frame
                 look_ahead  result k, enqueue k + 1, prefetch k + 2, call by call from Python
               The settings ALTERNATE within one run, every repeat on a fresh context; median and min..max over the repeats.
Measurement tool, not a test.
usage: python tests/measure/semidense_world_carve_cost.py [--frames 80] [--repeats 4] [--no-loops]"""
import argparse
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
from semidense_world_cost import WPRM  # noqa: E402
from semidense_world_reanchor_cost import timed  # noqa: E402

SETTINGS = (("world", None), ("carve", True))
FORMS = (("simple", 0), ("aggregated", 1))  # (VO_DBG_SDW_FORM = 1: the carve's other form)
VO_DBG_SDW_FORM = 10
F = np.float32


def launch(vo, DeviceBuffer, cfg, repeats, batch=10):
    La = cfg.imgs[2][0]
    h, w = La.shape
    out = {"pixels": int(h * w)}
    T0 = np.asarray(cfg.st.poses(7)[2], F)
    with vo.Context(device=0, max_width=w, max_height=h, max_points=256, n_slots=2, max_level=0) as c:
        m, _ = fused_map(vo, c, cfg, 5)
        bufs = {k: DeviceBuffer(np.ascontiguousarray(v)) for k, v in m.items()}
        planes = {k: b.data_ptr() for k, b in bufs.items()}
        try:
            c.profile_enable(4)
            for load, cap in (("one_map", 22), ("loaded", 20)):
                with c.semiDenseWorld(**WPRM, capacity_log2=cap) as wm:
                    res = {}
                    if load == "loaded":  # strips of 32 rows, the pose moved along x by 3 m a time, until the table refuses
                        rows, j = 32, 0
                        while wm.stats()["refused"] == 0 and j < 64:
                            T = T0.copy()
                            T[0, 3] += F(3.0 * j)
                            for y0 in range(0, h - rows + 1, rows):
                                strip = {"invd": planes["invd"] + 4 * y0 * w, "sigma": planes["sigma"] + 4 * y0 * w, "n_obs": planes["n_obs"] + y0 * w}
                                wm.integrate(strip, (cfg.K[0], cfg.K[1], cfg.K[2], cfg.K[3] - y0), T, on_device=(w, rows))
                            j += 1
                    else:
                        wm.integrate(planes, cfg.K, T0, on_device=(w, h))
                        res["integrate_us"] = stats(timed(c, lambda: None, lambda: wm.integrate(planes, cfg.K, T0, on_device=(w, h)), repeats * batch, 1), 2)
                    st = wm.stats()
                    res["load"] = round(st["occupied"] / st["capacity"], 4)
                    for name, form in FORMS:
                        c.debug_set(VO_DBG_SDW_FORM, form)
                        c0 = wm.carveStats()
                        res["carve_us_" + name] = stats(timed(c, lambda: None, lambda: wm.carve(planes, cfg.K, T0, on_device=(w, h)), repeats * batch, 1), 2)
                        c1 = wm.carveStats()
                        n = c1["carves"] - c0["carves"]
                        res["per_carve"] = {k: (c1[k] - c0[k]) // n for k in ("rays", "short_rays", "visits", "hits")}
                    c.debug_set(VO_DBG_SDW_FORM, 0)
                    out[load] = res
        finally:
            for b in bufs.values():
                b.free()
    return out


def one_run(vo, cfg, mode, carve):
    src, n = cfg.src, len(cfg.src)
    n_kf = 0
    with cfg.context(vo) as c:
        o, _ = cfg.make(vo, c, False)
        o.setSemiDense(dict(bf=BF, z_min=Z_MIN), every="keyframe")
        o.setSemiDenseTemporal({})
        o.setSemiDenseWorld(dict(WPRM))  # (the default 2^22 slots)
        if carve is not None:
            o.setSemiDenseWorldCarve(carve)
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
        o.getSemiDenseWorldStats()  # (the side stream's last launch belongs to the run)
        dt = time.perf_counter() - t0
        st = dict(o.getSemiDenseWorldStats(), **o.getSemiDenseWorldCarveStats())
        o.close()
    return 1e3 * dt / (n - WARM), n_kf, st


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=80)
    ap.add_argument("--repeats", type=int, default=4)
    ap.add_argument("--no-loops", action="store_true")
    a = ap.parse_args()
    import visual_odometry_ros_amd as vo
    from visual_odometry_ros_amd import synthetic as S
    from util import DeviceBuffer
    cfg = Stereo(S, a.frames)
    out = {"launch_1241x376": launch(vo, DeviceBuffer, cfg, a.repeats)}
    print(json.dumps(out), flush=True)
    if not a.no_loops:
        cfg.upload(DeviceBuffer)
        res = {}
        try:
            for mode in ("sync", "look_ahead"):
                one_run(vo, cfg, mode, True)  # (untimed: code objects loaded, clocks up)
                t = {s: [] for s, _ in SETTINGS}
                for _ in range(a.repeats):
                    for s, cv in SETTINGS:
                        ms, n_kf, st = one_run(vo, cfg, mode, cv)
                        t[s].append(ms)
                        res.setdefault("stats_" + s, st)
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
