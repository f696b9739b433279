"""What the ZNCC gate (vo_svo_set_zncc_gate / vo_mvo_set_zncc_gate) costs per frame on one MI355X: the stereo loop
at BASELINE configs[1] and the mono loop at configs[2] (the streams and settings of pose_covariance_cost.py), device images,
centred 15 x 15 patches, with
  off              no gate (the code path of a driver that never heard of the option)
  off_ordered      no gate, and the strict-border replay stream-ordered behind the frame kernel (mode 1 instead of 4): the
                   arrangement every gated frame runs in — `off` against this row is what the replay's own stream was worth,
                   this row against `all_pass_*` is the launch's own cost
  all_pass_t       thres = -2, temporal: every finite value passes, so the features are those of `off` — the launch's own cost
  all_pass_ts      the same with the stereo pair as well (StereoVO only): two pairs in the one launch
  temporal         thres = 0.8, temporal: the gate removes features, so the loop has less to do than `off`
  temporal_stereo  thres = 0.9, temporal + stereo (StereoVO only)
through
  sync        one trackStereoImages / trackImage call per frame
  look_ahead  result k, enqueue k + 1, prefetch k + 2, driven call by call from Python for every setting alike
The settings ALTERNATE within one run, every repeat on a fresh context; reported: ms per frame, median and min..max over the
repeats — always to be read against `off` of the same run.
Measurement tool, not a test. usage: python tests/measure/zncc_cost.py [--frames 80] [--repeats 5]"""
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

SETTINGS = {"off": None,
            "off_ordered": None,
            "all_pass_t": dict(thres=-2.0, win=15, pattern="centered", pairs=("temporal",)),
            "all_pass_ts": dict(thres=-2.0, win=15, pattern="centered", pairs=("temporal", "stereo")),
            "temporal": dict(thres=0.8, win=15, pattern="centered", pairs=("temporal",)),
            "temporal_stereo": dict(thres=0.9, win=15, pattern="centered", pairs=("temporal", "stereo"))}


def one_run(vo, cfg, mode, gate, ordered=False):
    src, n = cfg.src, len(cfg.src)
    with cfg.context(vo) as c:
        o, hook = cfg.make(vo, c, False)
        o.setZnccGate(gate)
        if ordered:
            c.check(c.lib.vo_stereo_frame_set_strict_border(c.handle, 1))

        def at(k):
            if hook is not None:
                hook.k = k

        if mode == "sync":
            t0 = None
            for k in range(n):
                if k == WARM:
                    t0 = time.perf_counter()
                at(k)
                cfg.track(o, src[k])
        else:
            cfg.enqueue(o, src[0])
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
    for name, cls in (("stereo_configs1", Stereo), ("mono_configs2", Mono)):
        cfg = cls(S, a.frames)
        cfg.upload(DeviceBuffer)
        settings = [s for s, g in SETTINGS.items() if cls is Stereo or g is None or "stereo" not in g["pairs"]]
        res = {}
        try:
            for mode in ("sync", "look_ahead"):
                one_run(vo, cfg, mode, SETTINGS["temporal"])  # (untimed: code objects loaded, clocks up)
                t = {s: [] for s in settings}
                for _ in range(a.repeats):
                    for s in settings:
                        t[s].append(one_run(vo, cfg, mode, SETTINGS[s], ordered=s == "off_ordered"))
                res[mode] = {s: dict(median=round(float(np.median(v)), 4), min=round(min(v), 4), max=round(max(v), 4)) for s, v in t.items()}
        finally:
            cfg.free()
        out[name] = res
        print(json.dumps({name: res}), flush=True)
    out["unit"] = "ms per frame"
    out["frames_timed"], out["repeats"] = a.frames - WARM, a.repeats
    print(json.dumps(out))


if __name__ == "__main__":
    main()
