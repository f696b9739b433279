"""What the ignore mask (vo_svo_set_mask / vo_mvo_set_mask) costs per frame on one MI355X: the stereo loop at
BASELINE configs[1] and the mono loop at configs[2] (the streams and settings of pose_covariance_cost.py), device images, with
  off        no mask (the code path of a driver that never heard of the option)
  all_255    a mask that ignores nothing, set before the first frame: the same features as `off`, plus the byte loads of the
             vote and the gate — the mask's own overhead
  static     one mask set before the first frame (bottom band and a box: a vehicle's bonnet and a time stamp); it removes
             features, so the loop has less to do than `off`
  per_frame  a new mask before every pair is handed over (host memory: one upload, one device copy and one event per frame)
through
  sync        one trackStereoImages / trackImage call per frame (setMask in front of it)
  look_ahead  result k, enqueue k + 1, setMask, prefetch k + 2, driven call by call from Python for every setting alike
and the setMask call alone (host mask; device mask), between frames with nothing in flight. The settings ALTERNATE within one
run, every repeat on a fresh context; reported: ms per frame (us for the call), median and min..max over the repeats.
Measurement tool, not a test. usage: python tests/measure/mask_cost.py [--frames 80] [--repeats 5]"""
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

from pose_covariance_cost import WARM, Mono, Stereo  # noqa: E402


def masks(cfg, n):
    """the static mask and n per-frame ones (the box moves 4 px per frame)"""
    out = []
    for k in range(n + 1):
        m = np.full((cfg.H, cfg.W), 255, np.uint8)
        m[int(cfg.H * 0.85):] = 0
        x0 = (cfg.W // 2 + 4 * k) % (cfg.W - 120)
        m[cfg.H // 4:cfg.H // 2, x0:x0 + 100] = 0
        out.append(m)
    return out[0], out[1:]


def one_run(vo, cfg, mode, setting, static, per_frame):
    src, n = cfg.src, len(cfg.src)
    with cfg.context(vo) as c:
        o, hook = cfg.make(vo, c, False)

        def at(k):
            if hook is not None:
                hook.k = k

        def mask_for(k):
            if setting == "per_frame":
                o.setMask(per_frame[k])

        if setting == "static":
            o.setMask(static)
        if setting == "all_255":
            o.setMask(np.full_like(static, 255))
        if mode == "sync":
            t0 = None
            for k in range(n):
                if k == WARM:
                    t0 = time.perf_counter()
                at(k)
                mask_for(k)
                cfg.track(o, src[k])
        else:
            mask_for(0)
            cfg.enqueue(o, src[0])
            mask_for(1)
            cfg.prefetch(o, src[1])
            t0 = None
            for k in range(n):
                if k == WARM:
                    t0 = time.perf_counter()
                at(k)
                o.result()
                if k + 1 < n:
                    cfg.enqueue(o, src[k + 1])
                    if k + 2 < n:
                        mask_for(k + 2)
                        cfg.prefetch(o, src[k + 2])
        dt = time.perf_counter() - t0
        o.close()
    return 1e3 * dt / (n - WARM)


def set_mask_us(vo, cfg, static, DeviceBuffer, reps=200):
    """the call alone, nothing in flight: us per call for a host mask and for a device mask"""
    out = {}
    with cfg.context(vo) as c:
        o, hook = cfg.make(vo, c, False)
        for k in range(WARM):
            if hook is not None:
                hook.k = k
            cfg.track(o, cfg.src[k])
        d = DeviceBuffer(static)
        for name, arg in (("host", static), ("device", (d.data_ptr(), cfg.W))):
            o.setMask(arg)
            t0 = time.perf_counter()
            for _ in range(reps):
                o.setMask(arg)
            out[name] = round(1e6 * (time.perf_counter() - t0) / reps, 2)
        d.free()
        o.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=80)
    ap.add_argument("--repeats", type=int, default=5)
    a = ap.parse_args()
    import visual_odometry_ros_amd as vo
    from visual_odometry_ros_amd import synthetic as S
    from util import DeviceBuffer
    out = {}
    settings = ("off", "all_255", "static", "per_frame")
    for name, cls in (("stereo_configs1", Stereo), ("mono_configs2", Mono)):
        cfg = cls(S, a.frames)
        cfg.upload(DeviceBuffer)
        static, per_frame = masks(cfg, a.frames)
        res = {}
        try:
            for mode in ("sync", "look_ahead"):
                one_run(vo, cfg, mode, "static", static, per_frame)  # (untimed: code objects loaded, clocks up)
                t = {s: [] for s in settings}
                for _ in range(a.repeats):
                    for s in settings:
                        t[s].append(one_run(vo, cfg, mode, s, static, per_frame))
                res[mode] = {s: dict(median=round(float(np.median(v)), 4), min=round(min(v), 4), max=round(max(v), 4)) for s, v in t.items()}
            res["set_mask_call_us"] = set_mask_us(vo, cfg, static, DeviceBuffer)
        finally:
            cfg.free()
        out[name] = res
        print(json.dumps({name: res}), flush=True)
    out["unit"] = "ms per frame"
    out["frames_timed"], out["repeats"] = a.frames - WARM, a.repeats
    print(json.dumps(out))


if __name__ == "__main__":
    main()
