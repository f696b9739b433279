"""What MonoVO's debug image (vo_mvo_set_debug_image) costs per frame on one MI355X: the mono loop at BASELINE configs[2]
(752 x 480, 40 x 25 buckets, window 15, 5 levels, local BA, strict border 4, device images) with the option off, on, and on with
the picture read after every frame (as the reference's node publishes it), through
  sync        one trackImage call per image
  look_ahead  the library's sequence loop (result k, enqueue k + 1, prefetch k + 2); `on_read` there is the same loop driven call
              by call from Python with getDebugImage() after every result, and `off_calls` its counterpart without the option
The settings ALTERNATE within one run (off, on, on_read, off, ...), every repeat on a fresh context, so that drift of the machine
hits all of them alike; reported: ms per frame, median and min..max over the repeats.
Measurement tool, not a test. usage: python tests/measure/mono_debug_image_cost.py [--frames 80] [--repeats 5]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

W, H, K, NU, NV = 752, 480, (458.654, 457.296, 367.215, 248.375), 40, 25
WARM = 12  # first image, initialisation, the first keyframes


class TruePoseHook:
    def __init__(self, poses):
        self.poses, self.k = poses, 1

    def __call__(self, pts0, pts1):
        T10 = np.linalg.inv(self.poses[self.k]) @ self.poses[self.k - 1]
        return True, T10[:3, :3].astype(np.float32), T10[:3, 3].astype(np.float32), np.ones(len(pts0), bool)


def one_run(vo, poses, src, mode, setting):
    """ms per frame of frames WARM .. n - 1"""
    n = len(src)
    hook = TruePoseHook(poses)
    on, read = setting in ("on", "on_read"), setting == "on_read"
    with vo.Context(device=0, max_width=W, max_height=H, max_points=2 * NU * NV + 512, n_slots=3, max_level=5) as c:
        mvo = vo.MonoVO(c, W, H, K, NU, NV, hook, thres_fastscore=15, window_size=15, max_level=5, thres_error=20.0, thres_bidirection=1.0,
                        thres_poseba_error=5, thres_sampson=1.0, thres_parallax=1.0, thres_translation=3.0, strict_border=4, local_ba=True,
                        debug_image=on)
        if mode == "sync":
            for k in range(WARM):
                hook.k = k
                mvo.trackImage(src[k])
            t0 = time.perf_counter()
            for k in range(WARM, n):
                hook.k = k
                mvo.trackImage(src[k])
                if read:
                    mvo.getDebugImage()
            dt = time.perf_counter() - t0
        elif setting in ("on_read", "off_calls"):
            mvo.enqueue(src[0])
            mvo.prefetch(src[1])
            t0 = None
            for k in range(n):
                if k == WARM:
                    t0 = time.perf_counter()
                hook.k = k
                mvo.result()
                if k + 1 < n:
                    mvo.enqueue(src[k + 1])
                    if k + 2 < n:
                        mvo.prefetch(src[k + 2])
                if read:
                    mvo.getDebugImage()
            dt = time.perf_counter() - t0
        else:
            mvo.runSequence(src, 0, WARM)
            t0 = time.perf_counter()
            infos, _ = mvo.runSequence(src, WARM, n)
            dt = time.perf_counter() - t0
            assert not any(i.used_five_point for i in infos)
        if on:
            assert mvo.getDebugImage().shape == (H, W, 3) and mvo.getDebugPoints()[0] == 2
        mvo.close()
    return 1e3 * dt / (n - WARM)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=80)
    ap.add_argument("--repeats", type=int, default=5)
    a = ap.parse_args()
    import visual_odometry_ros_amd as vo
    from visual_odometry_ros_amd import synthetic as S
    from util import DeviceBuffer
    st = S.StereoStream(width=W, height=H, K=K, n_u=NU, n_v=NV, seed=2, speed=0.25)
    poses = st.poses(a.frames)
    imgs = [np.ascontiguousarray(st.render_pair(p)[0]) for p in poses]
    dev = [DeviceBuffer(I) for I in imgs]
    src = [(d.data_ptr(), W) for d in dev]
    out = {}
    try:
        for mode, settings in (("sync", ("off", "on", "on_read")), ("look_ahead", ("off", "on", "off_calls", "on_read"))):
            one_run(vo, poses, src, mode, "on")  # (untimed: code objects loaded, clocks up)
            t = {s: [] for s in settings}
            for _ in range(a.repeats):
                for s in settings:
                    t[s].append(one_run(vo, poses, src, mode, s))
            out[mode] = {s: dict(median=round(float(np.median(v)), 4), min=round(min(v), 4), max=round(max(v), 4)) for s, v in t.items()}
    finally:
        for d in dev:
            d.free()
    out["unit"] = "ms per frame"
    out["frames_timed"], out["repeats"] = a.frames - WARM, a.repeats
    print(json.dumps(out))


if __name__ == "__main__":
    main()
