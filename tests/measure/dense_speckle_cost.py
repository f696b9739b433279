"""What the speckle filter (vo_disparity_speckle_filter, vo_svo_set_dense_speckle) costs on one MI355X, behind the dense
stereo disparity at 1241 x 376 with bf = 386.1, z_min = 3 m, 128 disparities and 8 paths (the settings of dense_stereo_cost.py), always
against the same run without it:
  kernel       into device planes, one call at a time (the launches and the host's wait for them), per call: vo_dense_stereo alone;
               vo_dense_stereo and the filter behind it (denseStereo(speckle=True): two synchronous calls); the filter alone, in
               place on the dense result with max_size = 0 (every launch runs on the same planes each time; nothing is removed) and
               with the defaults on planes it has filtered before. n_removed and n_components of the defaults on that pair.
               --calls-only N: N filter calls and nothing else, for a kernel-trace run that gives the time per launch.
  loops        the stereo loop at BASELINE configs[1] (the stream and settings of pose_covariance_cost.py, device images), per
               frame, dense per keyframe, with the filter off and on, through
                 sync        one trackStereoImages call per frame
                 look_ahead  result k, enqueue k + 1, prefetch k + 2, call by call from Python
The settings ALTERNATE within one run, every repeat on a fresh context; reported: median and min..max over the repeats.
Measurement tool, not a test.
usage: python tests/measure/dense_speckle_cost.py [--frames 80] [--repeats 4] [--calls-only N]"""
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

from dense_stereo_cost import BF, N_DISP, Z_MIN, stats  # noqa: E402
from pose_covariance_cost import WARM, Stereo  # noqa: E402

DENSE = dict(bf=BF, z_min=Z_MIN, n_disp=N_DISP, paths=8)


def kernel(vo, DeviceBuffer, cfg, repeats, batch=20, calls_only=0):
    L, R = cfg.imgs[2]
    h, w = L.shape
    bufs = {k: DeviceBuffer(np.zeros((h, w), dt)) for k, dt in (("disparity", np.float32), ("cost", np.uint16), ("sigma_invd", np.float32),
                                                                 ("status", np.uint8))}
    t = {"dense_and_filter": [], "dense": [], "filter_max_size_0": [], "filter_defaults_filtered_before": []}  # (timed in this order)
    try:
        with vo.Context(device=0, max_width=w, max_height=h, max_points=256, n_slots=2, max_level=0) as c:
            c.set_image(0, L)
            c.set_image(1, R)
            out = {k: b.data_ptr() for k, b in bufs.items()}
            planes = (out["disparity"], out["sigma_invd"], out["status"])
            calls = {"dense": lambda: c.denseStereo(0, 1, out=out, **DENSE),
                     "dense_and_filter": lambda: c.denseStereo(0, 1, out=out, speckle=True, **DENSE),
                     "filter_max_size_0": lambda: c.disparitySpeckleFilter(*planes, max_size=0, on_device=(w, h)),
                     "filter_defaults_filtered_before": lambda: c.disparitySpeckleFilter(*planes, on_device=(w, h))}
            calls["dense"]()
            first = calls["filter_max_size_0"]()
            if calls_only:
                for _ in range(calls_only):
                    calls["filter_max_size_0"]()
                return {"calls": calls_only + 1, "n_components": first.n_components}
            calls["dense_and_filter"]()
            for _ in range(repeats):
                for name in t:  # (the dense calls leave unfiltered planes for filter_max_size_0; the last one runs on its own output)
                    t0 = time.perf_counter()
                    for _k in range(batch):
                        calls[name]()
                    t[name].append(1e6 * (time.perf_counter() - t0) / batch)
            calls["dense"]()
            res = calls["filter_defaults_filtered_before"]()
            again = calls["filter_defaults_filtered_before"]()
            r = c.denseStereo(0, 1, **DENSE)
            ws = c.disparitySpeckleWorkspace(w, h)
    finally:
        for b in bufs.values():
            b.free()
    return {"call_us": {k: stats(v, 1) for k, v in t.items()}, "accepted": r.n_accepted, "n_removed": res.n_removed,
            "n_components": res.n_components, "n_components_after": again.n_components, "n_removed_after": again.n_removed, "workspace_bytes": ws}


def one_run(vo, cfg, mode, speckle):
    src, n = cfg.src, len(cfg.src)
    n_kf = 0
    with cfg.context(vo) as c:
        o, _ = cfg.make(vo, c, False)
        o.setDenseStereo(dict(DENSE), every="keyframe")
        if speckle:
            o.setDenseSpeckle(True)
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
        o.getDenseStereo()  # (the last launches belong to the run)
        dt = time.perf_counter() - t0
        last = o.getDenseSpeckleStats() if speckle else None
        o.close()
    return 1e3 * dt / (n - WARM), n_kf, last


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=80)
    ap.add_argument("--repeats", type=int, default=4)
    ap.add_argument("--calls-only", type=int, default=0, metavar="N", help="N filter calls and nothing else (for a kernel trace)")
    a = ap.parse_args()
    import visual_odometry_ros_amd as vo
    from visual_odometry_ros_amd import synthetic as S
    from util import DeviceBuffer
    cfg = Stereo(S, a.frames if not a.calls_only else 4)
    out = {"kernel_1241x376": kernel(vo, DeviceBuffer, cfg, a.repeats, calls_only=a.calls_only)}
    print(json.dumps(out), flush=True)
    if a.calls_only:
        return
    cfg.upload(DeviceBuffer)
    res = {}
    try:
        for mode in ("sync", "look_ahead"):
            one_run(vo, cfg, mode, True)  # (untimed: code objects loaded, clocks up)
            t = {"filter_off": [], "filter_on": []}
            for _ in range(a.repeats):
                for s in t:
                    ms, n_kf, last = one_run(vo, cfg, mode, s == "filter_on")
                    t[s].append(ms)
            res[mode] = {s: stats(v) for s, v in t.items()}
            res[mode]["keyframes"], res[mode]["last_result_removed_components"] = n_kf, last
    finally:
        cfg.free()
    out["stereo_configs1_dense_per_keyframe"] = res
    out["unit"] = "loops: ms per frame; kernel: us per call"
    out["frames_timed"], out["repeats"] = a.frames - WARM, a.repeats
    print(json.dumps(out))


if __name__ == "__main__":
    main()
