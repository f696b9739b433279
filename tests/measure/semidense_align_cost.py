"""What the direct image alignment on the semi-dense map (vo_semidense_align, vo_svo_set_semidense_align) costs on
one MI355X, at 1241 x 376 with bf = 386.1 and the default parameters:
  launches     the map of the stream's third pair — its static result, fused with the next two left images by the device's own
               operators — aligned with the sixth left image from the stream's relative pose perturbed by 62 mm and 0.21 degrees,
               every plane on the device: one iteration (max_iters = 1) and the default call (max_iters = 10: the launches behind
               "done" return at once), each between two events on the stream (the context's profiler), and the operator's whole
               call (the launches, the host's wait for them and the state block's copy). With the restatement's iteration count
               and pixel count for the same call.
  loops        the stereo loop at BASELINE configs[1] (the stream and settings of pose_covariance_cost.py, device images), per
               frame: static per keyframe + temporal, against the same with the alignment added, through
                 sync        one trackStereoImages call per frame
                 look_ahead  result k, enqueue k + 1, prefetch k + 2, call by call from Python
The settings ALTERNATE within one run, every repeat on a fresh context; reported: median and min..max over the repeats.
Measurement tool, not a test.
usage: python tests/measure/semidense_align_cost.py [--frames 80] [--repeats 5]"""
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

BF, Z_MIN = 386.1, 3.0
K_AUX = 5  # VO_K_AUX
XI = (0.03, -0.02, 0.05, 0.002, -0.003, 0.001)


def stats(v, nd=4):
    return dict(median=round(float(np.median(v)), nd), min=round(min(v), nd), max=round(max(v), nd))


def launches(vo, S, DeviceBuffer, cfg, repeats, batch=30):
    import semidense_align_restatement as AR
    F = np.float32
    poses = cfg.st.poses(6)
    La, Ra = cfg.imgs[2]
    Lc = cfg.imgs[5][0]
    h, w = La.shape
    d_min, d_max = vo.semidense_disparity_range(BF, Z_MIN)
    T = lambda b, a: (np.linalg.inv(poses[b]) @ poses[a]).astype(F)
    T0 = (S.se3_exp(np.array(XI)) @ T(5, 2).astype(np.float64)).astype(F)
    with vo.Context(device=0, max_width=w, max_height=h, max_points=256, n_slots=2, max_level=0) as c:
        c.set_image(0, La)
        c.set_image(1, Ra)
        s = c.semiDenseStereo(0, 1, d_min=d_min, d_max=d_max, bf=BF)
        m = c.semiDenseMapSeed(s.disparity, s.sigma_invd, s.status, BF)
        for i in (3, 4):
            c.set_image(1, cfg.imgs[i][0])
            m = c.semiDenseTemporal(La, 1, cfg.K, T(i, 2), m)
        c.set_image(0, Lc)
        mm = dict(invd=m.invd, sigma=m.sigma, n_obs=m.n_obs)
        want = AR.align(La, Lc, cfg.K, T0, mm)
        bufs = {k: DeviceBuffer(np.ascontiguousarray(v)) for k, v in mm.items()}
        dkey = DeviceBuffer(La)
        call = lambda **p: c.semiDenseAlign(dkey.data_ptr(), 0, cfg.K, T0, {k: b.data_ptr() for k, b in bufs.items()}, key_on_device=w,
                                            map_on_device=True, **p)
        try:
            got = call()
            assert got.status == want["status"] and got.iters == want["iters"] and np.array_equal(got.T_ck, want["T_ck"])  # (what is timed is the restatement's call)
            c.profile_enable(64)
            c.profile_set_classes(1 << K_AUX)
            t = {"one_iteration": [], "default_call": [], "empty_set": []}
            for _ in range(repeats * batch):
                # (empty_set: min_obs = 255 leaves no pixel — the map reads, the ticket and the last workgroup's sum over the 456 rows,
                # without the per-pixel work and the solve)
                for name, p in (("one_iteration", dict(max_iters=1)), ("default_call", {}), ("empty_set", dict(max_iters=1, min_obs=255))):
                    c.profile_reset()
                    call(**p)
                    n, ms = c.profile_get(K_AUX)
                    assert n == 1
                    t[name].append(1e3 * ms)
            c.profile_set_classes(1 << 0)  # (the profiler cannot be switched off: a class these launches are not in)
            t_call = []
            for _ in range(repeats):
                t0 = time.perf_counter()
                for _k in range(batch):
                    call()
                t_call.append(1e6 * (time.perf_counter() - t0) / batch)
        finally:
            dkey.free()
            for b in bufs.values():
                b.free()
    # one block: a 32 x 32 crop — a launch, one workgroup, the solve and the update, next to nothing else
    crop = lambda a: np.ascontiguousarray(a[170:202, 600:632])
    t_small = []
    with vo.Context(device=0, max_width=32, max_height=32, max_points=256, n_slots=2, max_level=0) as c:
        c.set_image(0, crop(Lc))
        Kc = (cfg.K[0], cfg.K[1], cfg.K[2] - 600, cfg.K[3] - 170)
        ms_ = {k: crop(v) for k, v in mm.items()}
        small = c.semiDenseAlign(crop(La), 0, Kc, T(5, 2), ms_, max_iters=1, min_pixels=6)
        c.profile_enable(64)
        c.profile_set_classes(1 << K_AUX)
        for _ in range(repeats * batch):
            c.profile_reset()
            c.semiDenseAlign(crop(La), 0, Kc, T(5, 2), ms_, max_iters=1, min_pixels=6)
            t_small.append(1e3 * c.profile_get(K_AUX)[1])
    E = np.linalg.inv(T(5, 2).astype(np.float64)) @ want["T_ck"].astype(np.float64)
    E0 = np.linalg.inv(T(5, 2).astype(np.float64)) @ T0.astype(np.float64)
    return {"one_iteration_us": stats(t["one_iteration"], 2), "default_call_launches_us": stats(t["default_call"], 2), "whole_call_us": stats(t_call, 1),
            "one_iteration_empty_set_us": stats(t["empty_set"], 2), "one_iteration_one_block_us": stats(t_small, 2),
            "one_block": dict(status=small.status, count=small.count), "iterations": want["iters"], "status": want["status"], "pixels_in_set": want["count"], "map_pixels": int((m.n_obs >= 1).sum()),
            "pixels": int(h * w), "blocks": (h * w + 1023) // 1024, "rms": round(want["rms"], 3),
            "translation_error_mm": [round(1e3 * float(np.linalg.norm(E0[:3, 3])), 2), round(1e3 * float(np.linalg.norm(E[:3, 3])), 2)]}


def one_run(vo, cfg, mode, setting):
    src, n = cfg.src, len(cfg.src)
    n_kf = n_al = 0
    with cfg.context(vo) as c:
        o, _ = cfg.make(vo, c, False)
        o.setSemiDense(dict(bf=BF, z_min=Z_MIN), every="keyframe")
        o.setSemiDenseTemporal({})
        if setting == "align":
            o.setSemiDenseAlign({})
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
        if setting == "align":
            n_al = o.getSemiDenseAlign().iters
        o.close()
    return 1e3 * dt / (n - WARM), n_kf, n_al


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=80)
    ap.add_argument("--repeats", type=int, default=5)
    a = ap.parse_args()
    import visual_odometry_ros_amd as vo
    from visual_odometry_ros_amd import synthetic as S
    from util import DeviceBuffer
    cfg = Stereo(S, a.frames)
    out = {"launches_1241x376": launches(vo, S, DeviceBuffer, cfg, a.repeats)}
    print(json.dumps(out), flush=True)
    cfg.upload(DeviceBuffer)
    res = {}
    try:
        for mode in ("sync", "look_ahead"):
            one_run(vo, cfg, mode, "align")  # (untimed: code objects loaded, clocks up)
            t = {"temporal": [], "align": []}
            for _ in range(a.repeats):
                for s in t:
                    ms, n_kf, n_al = one_run(vo, cfg, mode, s)
                    t[s].append(ms)
            res[mode] = {s: stats(v) for s, v in t.items()}
            res[mode]["keyframes"], res[mode]["last_frame_iterations"] = n_kf, n_al
    finally:
        cfg.free()
    out["stereo_configs1"] = res
    out["unit"] = "loops: ms per frame; launches: us"
    out["frames_timed"], out["repeats"] = a.frames - WARM, a.repeats
    print(json.dumps(out))


if __name__ == "__main__":
    main()
