"""What the dense stereo disparity (vo_dense_stereo, vo_svo_set_dense_stereo) costs on one MI355X, at 1241 x 376 with
bf = 386.1, z_min = 3 m and 128 disparities, 4 and 8 paths, always against the same run with the option off:
  kernel       vo_dense_stereo into device planes, one call at a time (the launches and the host's wait for them), per call; the bytes
               the aggregation launches must move (per direction: the volume's lines written, and read by every direction but the
               first; the two census planes read once) — over the aggregation kernels' time of a kernel-trace run (--calls-only: the
               calls alone, for such a run) that gives the achieved bytes per second; the workspace in bytes
  fractions    accepted / pixels on the stream's third pair
  loops        the stereo loop at BASELINE configs[1] (the stream and settings of pose_covariance_cost.py, device images), per
               frame, with every = keyframes and every = frames, through
                 sync        one trackStereoImages call per frame
                 look_ahead  result k, enqueue k + 1, prefetch k + 2, call by call from Python
The settings ALTERNATE within one run, every repeat on a fresh context; reported: median and min..max over the repeats.
Measurement tool, not a test.
usage: python tests/measure/dense_stereo_cost.py [--frames 80] [--repeats 5] [--calls-only N]"""
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

BF, Z_MIN, N_DISP = 386.1, 3.0, 128


def stats(v, nd=4):
    return dict(median=round(float(np.median(v)), nd), min=round(min(v), nd), max=round(max(v), nd))


def aggregation_bytes(w, h, n_disp, paths):
    """what the aggregation launches must move: per direction the volume written, and read but by the first; the census planes read"""
    vol = w * h * n_disp * 2
    return paths * vol + (paths - 1) * vol + paths * 2 * w * h * 8


def kernel(vo, DeviceBuffer, cfg, repeats, paths, batch=20, calls_only=0):
    L, R = cfg.imgs[2]
    h, w = L.shape
    prm = dict(bf=BF, z_min=Z_MIN, n_disp=N_DISP, paths=paths)
    bufs = {k: DeviceBuffer(np.zeros((h, w), dt)) for k, dt in (("disparity", np.float32), ("cost", np.uint16), ("sigma_invd", np.float32),
                                                                 ("status", np.uint8))}
    t = []
    try:
        with vo.Context(device=0, max_width=w, max_height=h, max_points=256, n_slots=2, max_level=0) as c:
            c.set_image(0, L)
            c.set_image(1, R)
            out = {k: b.data_ptr() for k, b in bufs.items()}
            call = lambda: c.denseStereo(0, 1, out=out, **prm)  # noqa: E731
            call()
            if calls_only:
                for _ in range(calls_only):
                    call()
                return {"paths": paths, "calls": calls_only + 1, "aggregation_bytes_per_call": aggregation_bytes(w, h, N_DISP, paths)}
            for _ in range(repeats):
                t0 = time.perf_counter()
                for _k in range(batch):
                    call()
                t.append(1e6 * (time.perf_counter() - t0) / batch)
            r = c.denseStereo(0, 1, **prm)
            ws = c.denseStereoWorkspace(w, h, **prm)
    finally:
        for b in bufs.values():
            b.free()
    p = vo.api._dense_stereo_params(vo.load(), prm)
    return {"paths": paths, "call_us": stats(t, 1), "disparities": [p.d_min, p.d_min + p.n_disp - 1], "accepted": r.n_accepted,
            "accepted_fraction": round(r.n_accepted / (w * h), 4), "workspace_bytes": ws,
            "aggregation_bytes_per_call": aggregation_bytes(w, h, N_DISP, paths)}


def one_run(vo, cfg, mode, every, paths=8):
    src, n = cfg.src, len(cfg.src)
    n_kf = 0
    with cfg.context(vo) as c:
        o, _ = cfg.make(vo, c, False)
        if every:
            o.setDenseStereo(dict(bf=BF, z_min=Z_MIN, n_disp=N_DISP, paths=paths), every=every)
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
        if every:
            o.getDenseStereo()  # (the last launches belong to the run)
        dt = time.perf_counter() - t0
        o.close()
    return 1e3 * dt / (n - WARM), n_kf


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=80)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--calls-only", type=int, default=0, metavar="N", help="N operator calls per path count and nothing else (for a kernel trace)")
    a = ap.parse_args()
    import visual_odometry_ros_amd as vo
    from visual_odometry_ros_amd import synthetic as S
    from util import DeviceBuffer
    cfg = Stereo(S, a.frames if not a.calls_only else 4)
    out = {"kernel_1241x376": [kernel(vo, DeviceBuffer, cfg, a.repeats, paths, calls_only=a.calls_only) for paths in (4, 8)]}
    print(json.dumps(out), flush=True)
    if a.calls_only:
        return
    cfg.upload(DeviceBuffer)
    res = {}
    try:
        for mode in ("sync", "look_ahead"):
            one_run(vo, cfg, mode, "frame")  # (untimed: code objects loaded, clocks up)
            t = {"off": [], "keyframe": [], "frame": []}
            for _ in range(a.repeats):
                for s in t:
                    ms, n_kf = one_run(vo, cfg, mode, None if s == "off" else s)
                    t[s].append(ms)
            res[mode] = {s: stats(v) for s, v in t.items()}
            res[mode]["keyframes"] = n_kf
    finally:
        cfg.free()
    out["stereo_configs1"] = res
    out["unit"] = "loops: ms per frame (8 paths); kernel: us per call"
    out["frames_timed"], out["repeats"] = a.frames - WARM, a.repeats
    print(json.dumps(out))


if __name__ == "__main__":
    main()
