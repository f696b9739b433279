"""What carrying the semi-dense map over to the next keyframe (vo_semidense_map_propagate, vo_svo_set_semidense_propagate;
DESIGN.md §19) costs on one MI355X, at 1241 x 376 with bf = 386.1 and the default parameters:
  launches     the map of the stream's third pair — its static result, fused with the next three left images by the device's own
               operators — carried to the seventh pair under the stream's relative pose, every plane on the device: the scatter
               alone and the resolve alone (vo_debug_set(VO_DBG_SDP_STAGE)), each between two events on the stream (the context's
               profiler), one launch at a time, scatter then resolve, so that every resolve finds the scatter's keys; and the
               operator's call with both (the two launches and the host's wait for them). With the counts the restatement of the
               same call gives: sources, atomics (sources kept), collisions — the atomics per second of the scatter.
  loops        the stereo loop at BASELINE configs[1] (the stream and settings of pose_covariance_cost.py, device images), per
               frame: static per keyframe + temporal, against the same with the propagation added, through
                 sync        one trackStereoImages call per frame
                 look_ahead  result k, enqueue k + 1, prefetch k + 2, call by call from Python
The settings ALTERNATE within one run, every repeat on a fresh context; reported: median and min..max over the repeats.
Measurement tool, not a test.
usage: python tests/measure/semidense_propagate_cost.py [--frames 80] [--repeats 5]"""
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
K_AUX = 5  # VO_K_AUX


def stats(v, nd=4):
    return dict(median=round(float(np.median(v)), nd), min=round(min(v), nd), max=round(max(v), nd))


def launches(vo, DeviceBuffer, cfg, repeats, batch=30):
    import semidense_propagate_restatement as PR
    F = np.float32
    poses = cfg.st.poses(7)
    (La, Ra), (Lb, Rb) = cfg.imgs[2], cfg.imgs[6]
    h, w = La.shape
    d_min, d_max = vo.semidense_disparity_range(BF, Z_MIN)
    T = lambda b, a: (np.linalg.inv(poses[b]) @ poses[a]).astype(F)
    with vo.Context(device=0, max_width=w, max_height=h, max_points=256, n_slots=2, max_level=0) as c:
        c.set_image(0, La)
        c.set_image(1, Ra)
        s = c.semiDenseStereo(0, 1, d_min=d_min, d_max=d_max, bf=BF)
        m = c.semiDenseMapSeed(s.disparity, s.sigma_invd, s.status, BF)
        for i in (3, 4, 5):
            c.set_image(1, cfg.imgs[i][0])
            m = c.semiDenseTemporal(La, 1, cfg.K, T(i, 2), m)
        c.set_image(0, Lb)
        c.set_image(1, Rb)
        sb = c.semiDenseStereo(0, 1, d_min=d_min, d_max=d_max, bf=BF)
        old = dict(invd=m.invd, sigma=m.sigma, n_obs=m.n_obs)
        stat = dict(disparity=sb.disparity, sigma_invd=sb.sigma_invd, status=sb.status)
        want = PR.propagate(old, La, Lb, stat, F(BF), cfg.K, T(6, 2))
        bufs = {k: DeviceBuffer(np.ascontiguousarray(v)) for k, v in {**old, **stat}.items()}
        outs = {k: DeviceBuffer(np.zeros((h, w), dt)) for k, dt in (("invd", F), ("sigma", F), ("n_obs", np.uint8), ("tstatus", np.uint8),
                                                                     ("origin", np.uint8))}
        dkey = DeviceBuffer(La)
        call = lambda: c.semiDenseMapPropagate({k: bufs[k].data_ptr() for k in old}, dkey.data_ptr(), 0, {k: bufs[k].data_ptr() for k in stat}, BF,
                                               cfg.K, T(6, 2), out={k: b.data_ptr() for k, b in outs.items()}, key_on_device=w)
        try:
            call()
            got = np.zeros((h, w), np.uint8)
            assert dkey.hip.hipMemcpy(got.ctypes.data_as(C.c_void_p), outs["origin"].ptr, C.c_size_t(got.nbytes), 2) == 0
            assert np.array_equal(got, want["origin"])  # (what is timed is the restatement's call)
            c.profile_enable(4)
            c.profile_set_classes(1 << K_AUX)
            t = {"scatter": [], "resolve": []}
            for _ in range(repeats * batch):
                for stage, name in ((1, "scatter"), (2, "resolve")):
                    c.debug_set(c.DBG_SDP_STAGE, stage)
                    c.profile_reset()
                    call()
                    n, ms = c.profile_get(K_AUX)
                    assert n == 1
                    t[name].append(1e3 * ms)
            c.debug_set(c.DBG_SDP_STAGE, 0)
            c.profile_set_classes(1 << 0)  # (the profiler cannot be switched off: a class these launches are not in)
            t_call = []
            for _ in range(repeats):
                t0 = time.perf_counter()
                for _k in range(batch):
                    call()
                t_call.append(1e6 * (time.perf_counter() - t0) / batch)
            assert dkey.hip.hipMemcpy(got.ctypes.data_as(C.c_void_p), outs["origin"].ptr, C.c_size_t(got.nbytes), 2) == 0
            assert np.array_equal(got, want["origin"])
        finally:
            dkey.free()
            for b in list(bufs.values()) + list(outs.values()):
                b.free()
    cnt = want["counts"]
    us = float(np.median(t["scatter"]))
    return {"scatter_us": stats(t["scatter"], 2), "resolve_us": stats(t["resolve"], 2), "call_both_us": stats(t_call, 1), **cnt,
            "origin_histogram": np.bincount(want["origin"].ravel(), minlength=5).tolist(), "pixels": int(h * w),
            "atomics_per_s": round(cnt["kept"] / (us * 1e-6), -6)}


def one_run(vo, cfg, mode, setting):
    src, n = cfg.src, len(cfg.src)
    n_kf = 0
    with cfg.context(vo) as c:
        o, _ = cfg.make(vo, c, False)
        o.setSemiDense(dict(bf=BF, z_min=Z_MIN), every="keyframe")
        o.setSemiDenseTemporal({})
        if setting == "propagate":
            o.setSemiDensePropagate({})
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
    out = {"launches_1241x376": launches(vo, DeviceBuffer, cfg, a.repeats)}
    print(json.dumps(out), flush=True)
    cfg.upload(DeviceBuffer)
    res = {}
    try:
        for mode in ("sync", "look_ahead"):
            one_run(vo, cfg, mode, "propagate")  # (untimed: code objects loaded, clocks up)
            t = {"temporal": [], "propagate": []}
            for _ in range(a.repeats):
                for s in t:
                    ms, n_kf = one_run(vo, cfg, mode, s)
                    t[s].append(ms)
            res[mode] = {s: stats(v) for s, v in t.items()}
            res[mode]["keyframes"] = n_kf
    finally:
        cfg.free()
    out["stereo_configs1"] = res
    out["unit"] = "loops: ms per frame; launches: us"
    out["frames_timed"], out["repeats"] = a.frames - WARM, a.repeats
    print(json.dumps(out))


if __name__ == "__main__":
    main()
