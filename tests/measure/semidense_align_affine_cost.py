"""What the alignment with affine brightness (vo_semidense_align_affine, vo_semidense_align_pyr_affine,
vo_svo_set_semidense_align_affine) costs on one MI355X next to the same call without it, at 1241 x 376 with bf = 386.1
and the default parameters:
  launches     the setup of semidense_align_pyr_cost.py (the map of the stream's third pair fused with the next two left images, the
               fourth left image as the current one, every map plane on the device), each between two events on the stream (the
               context's profiler): one level-0 iteration (max_iters = 1) and the default level-0 call from the stream's pose; one
               iteration per level (levels = 4, the map pyramid's launches included) and the default 4-level call from the identity;
               each with and without affine=True, alternating; the operators' whole calls; the iterations each call ran.
  loops        the stereo loop at BASELINE configs[1] (the stream and settings of pose_covariance_cost.py, device images), per
               frame: static per keyframe + temporal + the alignment (level 0, and 4 levels), with and without the modifier, through
                 sync        one trackStereoImages call per frame
                 look_ahead  result k, enqueue k + 1, prefetch k + 2, call by call from Python
The settings ALTERNATE within one run, every repeat on a fresh context; reported: median and min..max over the repeats.
Measurement tool, not a test.
usage: python tests/measure/semidense_align_affine_cost.py [--frames 80] [--repeats 5]"""
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

SETTINGS = {"level_0": {}, "level_0_affine": dict(affine=True), "levels_4": dict(levels=4), "levels_4_affine": dict(levels=4, affine=True)}


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
        dkey = DeviceBuffer(np.ascontiguousarray(La))
        dev = {k: b.data_ptr() for k, b in bufs.items()}
        lvl0 = lambda affine, **p: c.semiDenseAlign(dkey.data_ptr(), 1, cfg.K, T(3, 2), dev, key_on_device=w, map_on_device=True, affine=affine, **p)
        pyr = lambda affine, **p: c.semiDenseAlignPyramid(0, 1, cfg.K, I4, dev, map_on_device=True, affine=affine, **p)
        calls = {}
        for tag, affine in (("", None), ("_affine", True)):
            calls["level_0_one_iteration" + tag] = lambda a=affine: lvl0(a, max_iters=1)
            calls["level_0_default_call" + tag] = lambda a=affine: lvl0(a)
            calls["levels_4_one_iteration_per_level" + tag] = lambda a=affine: pyr(a, max_iters=1)
            calls["levels_4_default_call" + tag] = lambda a=affine: pyr(a)
        try:
            outcome = {k: f() for k, f in calls.items()}
            c.profile_enable(64)
            c.profile_set_classes(1 << K_AUX)
            t = {k: [] for k in calls}
            for _ in range(repeats * batch):
                for name, f in calls.items():
                    c.profile_reset()
                    f()
                    t[name].append(1e3 * c.profile_get(K_AUX)[1])
            c.profile_set_classes(1 << 0)  # (the profiler cannot be switched off: a class these launches are not in)
            t_call = {k: [] for k in calls if "default" in k}
            for _ in range(repeats):
                for name in t_call:
                    t0 = time.perf_counter()
                    for _k in range(batch):
                        calls[name]()
                    t_call[name].append(1e6 * (time.perf_counter() - t0) / batch)
        finally:
            dkey.free()
            for b in bufs.values():
                b.free()
    out = {"launches_us": {k: stats(v, 2) for k, v in t.items()}, "whole_call_us": {k: stats(v, 1) for k, v in t_call.items()},
           "pixels": int(h * w), "map_pixels": int((m.n_obs >= 1).sum())}
    out["outcome"] = {k: dict(status=r.status, iters=r.iters if r.levels is None else [lv.iters for lv in r.levels], count=r.count,
                              **({} if r.gain is None else dict(gain=round(r.gain, 4), offset=round(r.offset, 2)))) for k, r in outcome.items()}
    return out


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
            one_run(vo, cfg, mode, "levels_4_affine")  # (untimed: code objects loaded, clocks up)
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
