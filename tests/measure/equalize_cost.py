"""What the CLAHE equalisation (vo_set_equalize) costs on one MI355X, always against the same run with the option off:
  launches     the two launches alone, for a pair: 200 pair ingestions (vo_set_stereo_pair_device) queued back to back and one
               wait at the end, on minus off, per pair — what the device spends on them with nothing to hide behind
  chain        one pair's ingestion chain (equalisation, pyramids of both images) from the call to the end of the device work,
               one pair at a time, at 1241 x 376 and at 752 x 480
  operator     vo_equalize_image on a device image into a device image (the two launches, a device copy and the host's wait)
  loops        the stereo loop at BASELINE configs[1] and the mono loop at configs[2] (the streams and settings of
               pose_covariance_cost.py, device images) through
                 sync        one trackStereoImages / trackImage call per frame. With the option on this route gives up the
                             early start of the keypoint detection from the caller's image (it reads the equalised image, which
                             exists behind the blend launch only) and takes the deferred detection from the slot: the figure
                             holds both costs.
                 look_ahead  result k, enqueue k + 1, prefetch k + 2, call by call from Python: the route is the same on and off
The equalised stream is not the same workload as the raw one (the detector finds other keypoints), so the loops' difference is the
option's cost on this stream, not the launches' alone. The settings ALTERNATE within one run, every repeat on a fresh context;
reported: median and min..max over the repeats. Measurement tool, not a test.
usage: python tests/measure/equalize_cost.py [--frames 80] [--repeats 5]"""
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

EQ = dict(clip_limit=40.0, tiles=(8, 8))


def stats(v, nd=4):
    return dict(median=round(float(np.median(v)), nd), min=round(min(v), nd), max=round(max(v), nd))


def ingestion(vo, DeviceBuffer, w, h, repeats, batch=200):
    rng = np.random.default_rng(1)
    imgs = [rng.integers(0, 256, (h, w), dtype=np.uint8) for _ in range(2)]
    dev = [DeviceBuffer(im) for im in imgs]
    t = {k: {"off": [], "on": []} for k in ("queued", "single", "operator")}
    try:
        with vo.Context(device=0, max_width=w, max_height=h, max_points=256, n_slots=2, max_level=5) as c:
            pair = lambda: c.set_stereo_pair_device(0, dev[0].data_ptr(), 1, dev[1].data_ptr(), w, h, w)  # noqa: E731
            c.set_equalize("clahe", **EQ)
            out = DeviceBuffer(np.zeros((h, w), np.uint8))
            for _ in range(repeats + 1):  # (the first round is untimed)
                for setting in ("off", "on"):
                    c.set_equalize("clahe" if setting == "on" else None, **EQ)
                    pair()
                    c.synchronize()
                    t0 = time.perf_counter()
                    for _k in range(batch):
                        pair()
                    c.synchronize()
                    t["queued"][setting].append(1e6 * (time.perf_counter() - t0) / batch)
                    t0 = time.perf_counter()
                    for _k in range(batch):
                        pair()
                        c.synchronize()
                    t["single"][setting].append(1e6 * (time.perf_counter() - t0) / batch)
                t0 = time.perf_counter()
                for _k in range(batch):
                    c.check(c.lib.vo_equalize_image(c.handle, dev[0].data_ptr(), w, w, h, out.data_ptr(), w, None, 1))
                t["operator"]["on"].append(1e6 * (time.perf_counter() - t0) / batch)
            out.free()
    finally:
        for d in dev:
            d.free()
    q = {s: t["queued"][s][1:] for s in ("off", "on")}
    s1 = {s: t["single"][s][1:] for s in ("off", "on")}
    return {"launches_pair_us": stats([a - b for a, b in zip(q["on"], q["off"])], 2),
            "queued_pair_us": {s: stats(v, 2) for s, v in q.items()},
            "chain_pair_us": {s: stats(v, 2) for s, v in s1.items()},
            "operator_call_us": stats(t["operator"]["on"][1:], 2)}


def one_run(vo, cfg, mode, on):
    src, n = cfg.src, len(cfg.src)
    with cfg.context(vo) as c:
        if on:
            c.set_equalize("clahe", **EQ)
        o, hook = cfg.make(vo, c, False)

        def at(k):
            if hook is not None:
                hook.k = k

        t0 = None
        if mode == "sync":
            for k in range(n):
                if k == WARM:
                    t0 = time.perf_counter()
                at(k)
                cfg.track(o, src[k])
        else:
            cfg.enqueue(o, src[0])
            cfg.prefetch(o, src[1])
            for k in range(n):
                if k == WARM:
                    t0 = time.perf_counter()
                at(k)
                o.result()
                if k + 1 < n:
                    cfg.enqueue(o, src[k + 1])
                    if k + 2 < n:
                        cfg.prefetch(o, src[k + 2])
        dt = time.perf_counter() - t0
        o.close()
    return 1e3 * dt / (n - WARM)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=80)
    ap.add_argument("--repeats", type=int, default=5)
    a = ap.parse_args()
    import visual_odometry_ros_amd as vo
    from visual_odometry_ros_amd import synthetic as S
    from util import DeviceBuffer
    out = {}
    for w, h in ((1241, 376), (752, 480)):
        out[f"ingestion_{w}x{h}"] = ingestion(vo, DeviceBuffer, w, h, a.repeats)
        print(json.dumps({f"ingestion_{w}x{h}": out[f"ingestion_{w}x{h}"]}), flush=True)
    for name, cls in (("stereo_configs1", Stereo), ("mono_configs2", Mono)):
        cfg = cls(S, a.frames)
        cfg.upload(DeviceBuffer)
        res = {}
        try:
            for mode in ("sync", "look_ahead"):
                one_run(vo, cfg, mode, True)  # (untimed: code objects loaded, clocks up)
                t = {"off": [], "on": []}
                for _ in range(a.repeats):
                    for s in ("off", "on"):
                        t[s].append(one_run(vo, cfg, mode, s == "on"))
                res[mode] = {s: stats(v) for s, v in t.items()}
        finally:
            cfg.free()
        out[name] = res
        print(json.dumps({name: res}), flush=True)
    out["unit"] = "loops: ms per frame; ingestion: us per pair / per call"
    out["frames_timed"], out["repeats"] = a.frames - WARM, a.repeats
    print(json.dumps(out))


if __name__ == "__main__":
    main()
