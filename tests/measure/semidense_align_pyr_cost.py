"""What the coarse-to-fine alignment on a map pyramid (vo_semidense_map_pyramid, vo_semidense_align_pyr, vo_svo_set_semidense_align_pyr;
DESIGN.md §21) costs on one MI355X, at 1241 x 376 with bf = 386.1 and the default parameters (4 levels, 10 iterations each):
  launches     the map of the stream's third pair — its static result, fused with the next two left images by the device's own
               operators — and the fourth left image, one frame's motion (0.8 m) on, every map plane on the device, each between two
               events on the stream (the context's profiler): the map pyramid's three launches; one iteration per level (levels = 4
               with one iteration each, the map pyramid's launches included and then subtracted); the default call from the IDENTITY,
               0.8 m off (the launches behind a level's "done" return at once); and the operator's whole call (the launches, the host's
               wait for them and the state block's copy). With the outcome: per-level status, iterations and pixels, and the distance
               of the end point to the stream's pose next to the level-0 operator's after 32 iterations.
  loops        the stereo loop at BASELINE configs[1] (the stream and settings of pose_covariance_cost.py, device images), per
               frame: static per keyframe + temporal + the level-0 alignment, against the same with 4 levels (start="odometry") and
               with 4 levels and start="previous", through
                 sync        one trackStereoImages call per frame
                 look_ahead  result k, enqueue k + 1, prefetch k + 2, call by call from Python
The settings ALTERNATE within one run, every repeat on a fresh context; reported: median and min..max over the repeats.
Measurement tool, not a test.
usage: python tests/measure/semidense_align_pyr_cost.py [--frames 80] [--repeats 5]"""
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
from semidense_align_cost import BF, K_AUX, Z_MIN, stats  # noqa: E402

SETTINGS = {"level_0": {}, "levels_4": dict(levels=4), "levels_4_previous": dict(levels=4, start="previous")}


def launches(vo, DeviceBuffer, cfg, repeats, batch=30):
    F = np.float32
    poses = cfg.st.poses(6)
    La, Ra = cfg.imgs[2]
    Lc = cfg.imgs[3][0]
    h, w = La.shape
    d_min, d_max = vo.semidense_disparity_range(BF, Z_MIN)
    T = lambda b, a: (np.linalg.inv(poses[b]) @ poses[a]).astype(F)
    I4 = np.eye(4, dtype=F)
    with vo.Context(device=0, max_width=w, max_height=h, max_points=256, n_slots=2, max_level=3) as c:
        c.set_image(0, La)
        c.set_image(1, Ra)
        s = c.semiDenseStereo(0, 1, d_min=d_min, d_max=d_max, bf=BF)
        m = c.semiDenseMapSeed(s.disparity, s.sigma_invd, s.status, BF)
        for i in (3, 4):
            c.set_image(1, cfg.imgs[i][0])
            m = c.semiDenseTemporal(La, 1, cfg.K, T(i, 2), m)
        c.set_image(1, Lc)
        mm = dict(invd=m.invd, sigma=m.sigma, n_obs=m.n_obs)
        bufs = {k: DeviceBuffer(np.ascontiguousarray(v)) for k, v in mm.items()}
        n = sum(((w + (1 << l) - 1) >> l) * ((h + (1 << l) - 1) >> l) for l in (1, 2, 3))  # ((w + 1) / 2 repeated = ceil(w / 2^l))
        outs = {k: DeviceBuffer(np.zeros(n, np.uint8 if k == "n_obs" else F)) for k in mm}
        dev = {k: b.data_ptr() for k, b in bufs.items()}
        call = lambda **p: c.semiDenseAlignPyramid(0, 1, cfg.K, I4, dev, map_on_device=True, **p)
        pyramid = lambda: c.semiDenseMapPyramid(dev, 4, on_device=(w, h), out={k: b.data_ptr() for k, b in outs.items()})
        try:
            got = call()
            lone = c.semiDenseAlign(La, 1, cfg.K, I4, mm, max_iters=32)
            c.profile_enable(64)
            c.profile_set_classes(1 << K_AUX)
            t = {"map_pyramid": [], "one_iteration_per_level": [], "default_call": []}
            for _ in range(repeats * batch):
                for name, f in (("map_pyramid", pyramid), ("one_iteration_per_level", lambda: call(max_iters=1)), ("default_call", call)):
                    c.profile_reset()
                    f()
                    t[name].append(1e3 * c.profile_get(K_AUX)[1])  # (the operator's two launch groups — pyramid, levels — summed)
            c.profile_set_classes(1 << 0)  # (the profiler cannot be switched off: a class these launches are not in)
            t_call = []
            for _ in range(repeats):
                t0 = time.perf_counter()
                for _k in range(batch):
                    call()
                t_call.append(1e6 * (time.perf_counter() - t0) / batch)
        finally:
            for b in list(bufs.values()) + list(outs.values()):
                b.free()

    def off(Tm):
        E = np.linalg.inv(T(3, 2).astype(np.float64)) @ Tm.astype(np.float64)
        return round(1e3 * float(np.linalg.norm(E[:3, 3])), 2)
    return {"map_pyramid_3_launches_us": stats(t["map_pyramid"], 2), "pyramid_and_one_iteration_per_level_us": stats(t["one_iteration_per_level"], 2),
            "default_call_launches_us": stats(t["default_call"], 2), "whole_call_us": stats(t_call, 1),
            "levels_status_iters_count": [tuple(lv[:3]) for lv in got.levels], "status": got.status,
            "translation_error_mm": dict(start=off(I4), level_0_alone_32_iterations=off(lone.T_ck), levels_4=off(got.T_ck)),
            "level_0_alone": dict(status=lone.status, iters=lone.iters), "pixels": int(h * w), "map_pixels": int((m.n_obs >= 1).sum())}


def one_run(vo, cfg, mode, setting):
    src, n = cfg.src, len(cfg.src)
    n_kf = 0
    with cfg.context(vo) as c:
        o, _ = cfg.make(vo, c, False)
        o.setSemiDense(dict(bf=BF, z_min=Z_MIN), every="keyframe")
        o.setSemiDenseTemporal({})
        o.setSemiDenseAlign(dict(SETTINGS[setting]))
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
        a = o.getSemiDenseAlign()
        o.close()
    return 1e3 * dt / (n - WARM), n_kf, [tuple(lv[:2]) for lv in a.levels]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=80)
    ap.add_argument("--repeats", type=int, default=5)
    a = ap.parse_args()
    import visual_odometry_ros_amd as vo
    from visual_odometry_ros_amd import synthetic as S
    from util import DeviceBuffer
    cfg = Stereo(S, a.frames)
    out = {"launches_1241x376": launches(vo, DeviceBuffer, cfg, a.repeats)}
    print(json.dumps(out), flush=True)
    cfg.upload(DeviceBuffer)
    res = {}
    try:
        for mode in ("sync", "look_ahead"):
            one_run(vo, cfg, mode, "levels_4")  # (untimed: code objects loaded, clocks up)
            t = {s: [] for s in SETTINGS}
            last = {}
            for _ in range(a.repeats):
                for s in t:
                    ms, n_kf, last[s] = one_run(vo, cfg, mode, s)
                    t[s].append(ms)
            res[mode] = {s: stats(v) for s, v in t.items()}
            res[mode]["keyframes"], res[mode]["last_frame_levels_status_iters"] = n_kf, last
    finally:
        cfg.free()
    out["stereo_configs1"] = res
    out["unit"] = "loops: ms per frame; launches: us"
    out["frames_timed"], out["repeats"] = a.frames - WARM, a.repeats
    print(json.dumps(out))


if __name__ == "__main__":
    main()
