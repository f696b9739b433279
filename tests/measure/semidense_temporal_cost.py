"""What the temporal semi-dense search and fusion (vo_semidense_temporal, vo_svo_set_semidense_temporal) costs on one
MI355X, at 1241 x 376 with bf = 386.1 and the default parameters, always against the same run with the option off:
  kernel       vo_semidense_temporal into device planes (key plane on the device), one call at a time (the launch and the host's
               wait for it), per call, with a map seeded from the static result of the stream's third pair and with an empty
               one, the fourth left image as the current one under the stream's own relative pose; the map is written back to
               its first state before every call (a device copy, inside the timed region for both settings alike); from the
               restatement of the same call: gradient candidates, searched pixels, positions scored, updated pixels — per second
  loops        the stereo loop at BASELINE configs[1] (the stream and settings of pose_covariance_cost.py, device images), per
               frame: option off, static per keyframe, static per keyframe + temporal, through
                 sync        one trackStereoImages call per frame
                 look_ahead  result k, enqueue k + 1, prefetch k + 2, call by call from Python
The settings ALTERNATE within one run, every repeat on a fresh context; reported: median and min..max over the repeats.
Measurement tool, not a test.
usage: python tests/measure/semidense_temporal_cost.py [--frames 80] [--repeats 5]"""
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

BF, Z_MIN = 386.1, 3.0


def stats(v, nd=4):
    return dict(median=round(float(np.median(v)), nd), min=round(min(v), nd), max=round(max(v), nd))


def kernel(vo, DeviceBuffer, cfg, repeats, batch=30):
    import semidense_restatement as SR
    import semidense_temporal_restatement as TR
    (Lk, Rk), (Lc, _) = cfg.imgs[2], cfg.imgs[3]
    h, w = Lk.shape
    poses = cfg.st.poses(4)
    T_ck = (np.linalg.inv(poses[3]) @ poses[2]).astype(np.float32)
    d_min, d_max = vo.semidense_disparity_range(BF, Z_MIN)
    s = SR.semidense(Lk, Rk, d_min=d_min, d_max=d_max, bf=BF)
    maps = {"seeded": TR.seed(s["disparity"], s["sigma_invd"], s["status"], np.float32(BF)), "empty": TR.empty_map((h, w))}
    out = {}
    with vo.Context(device=0, max_width=w, max_height=h, max_points=256, n_slots=2, max_level=0) as c:
        c.set_image(0, Lc)
        dkey = DeviceBuffer(Lk)
        try:
            for name, m in maps.items():
                want = TR.temporal(Lk, Lc, cfg.K, T_ck, m)
                first = {k: DeviceBuffer(np.ascontiguousarray(m[k])) for k in ("invd", "sigma", "n_obs", "tstatus")}
                work = {k: DeviceBuffer(np.ascontiguousarray(m[k])) for k in ("invd", "sigma", "n_obs", "tstatus")}
                hip = dkey.hip

                def call():
                    for k in work:  # the map back to its first state (device to device)
                        assert hip.hipMemcpy(work[k].ptr, first[k].ptr, C.c_size_t(m[k].nbytes), 3) == 0
                    c.semiDenseTemporal(dkey.data_ptr(), 0, cfg.K, T_ck, {k: b.data_ptr() for k, b in work.items()}, key_on_device=w,
                                        map_on_device=True)

                def copies():
                    for k in work:
                        assert hip.hipMemcpy(work[k].ptr, first[k].ptr, C.c_size_t(m[k].nbytes), 3) == 0
                try:
                    call()
                    t, t_copy = [], []
                    for _ in range(repeats):
                        t0 = time.perf_counter()
                        for _k in range(batch):
                            call()
                        t.append(1e6 * (time.perf_counter() - t0) / batch)
                        t0 = time.perf_counter()
                        for _k in range(batch):
                            copies()
                        t_copy.append(1e6 * (time.perf_counter() - t0) / batch)
                    call()  # (the copies above left the first state behind)
                    got = np.zeros((h, w), np.uint8)
                    assert hip.hipMemcpy(got.ctypes.data_as(C.c_void_p), work["tstatus"].ptr, C.c_size_t(got.nbytes), 2) == 0
                    assert np.array_equal(got, want["tstatus"])  # (what was timed is the restatement's launch)
                finally:
                    for b in list(first.values()) + list(work.values()):
                        b.free()
                us = float(np.median(t)) - float(np.median(t_copy))
                cnt = want["counts"]
                upd = int((want["tstatus"] == 1).sum())
                out[name] = {"call_with_reset_us": stats(t, 1), "reset_copies_us": stats(t_copy, 1), "call_us": round(us, 1), **cnt, "updated": upd,
                             "status_histogram": np.bincount(want["tstatus"].ravel(), minlength=9).tolist(),
                             "candidates_per_s": round(cnt["candidates"] / (us * 1e-6), -6), "updated_per_s": round(upd / (us * 1e-6), -6),
                             "positions_per_s": round(cnt["positions"] / (us * 1e-6), -6)}
        finally:
            dkey.free()
    return out


def one_run(vo, cfg, mode, setting):
    src, n = cfg.src, len(cfg.src)
    n_kf = 0
    with cfg.context(vo) as c:
        o, _ = cfg.make(vo, c, False)
        if setting != "off":
            o.setSemiDense(dict(bf=BF, z_min=Z_MIN), every="keyframe")
        if setting == "temporal":
            o.setSemiDenseTemporal({})
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
        if setting == "temporal":
            o.getSemiDenseMap()  # (the last launch belongs to the run)
        elif setting == "keyframe":
            o.getSemiDense()
        dt = time.perf_counter() - t0
        o.close()
    return 1e3 * dt / (n - WARM), n_kf


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=80)
    ap.add_argument("--repeats", type=int, default=5)
    a = ap.parse_args()
    import visual_odometry_ros_amd as vo
    from visual_odometry_ros_amd import synthetic as S
    from util import DeviceBuffer
    cfg = Stereo(S, a.frames)
    out = {"kernel_1241x376": kernel(vo, DeviceBuffer, cfg, a.repeats)}
    print(json.dumps(out), flush=True)
    cfg.upload(DeviceBuffer)
    res = {}
    try:
        for mode in ("sync", "look_ahead"):
            one_run(vo, cfg, mode, "temporal")  # (untimed: code objects loaded, clocks up)
            t = {"off": [], "keyframe": [], "temporal": []}
            for _ in range(a.repeats):
                for s in t:
                    ms, n_kf = one_run(vo, cfg, mode, s)
                    t[s].append(ms)
            res[mode] = {s: stats(v) for s, v in t.items()}
            res[mode]["keyframes"] = n_kf
    finally:
        cfg.free()
    out["stereo_configs1"] = res
    out["unit"] = "loops: ms per frame; kernel: us per call"
    out["frames_timed"], out["repeats"] = a.frames - WARM, a.repeats
    print(json.dumps(out))


if __name__ == "__main__":
    main()
