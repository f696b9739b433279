"""What the pose covariance (vo_svo_set_pose_covariance / vo_mvo_set_pose_covariance) costs per frame on one MI355X: the stereo
loop at BASELINE configs[1] (1241 x 376, 60 x 25 buckets, window 21, 6 levels, local BA, strict border 4) and the mono loop at
configs[2] (752 x 480, 40 x 25 buckets, window 15, 5 levels, local BA, strict border 4), device images, with the option off, on,
and on with the covariance read after every frame (as a node fills pose.covariance), through
  sync        one trackStereoImages / trackImage call per frame
  look_ahead  the library's sequence loop (result k, enqueue k + 1, prefetch k + 2); `on_read` there is the same loop driven call
              by call from Python with getPoseCovariance() after every result, and `off_calls` its counterpart without the option
The settings ALTERNATE within one run (off, on, on_read, off, ...), every repeat on a fresh context, so that drift of the machine
hits all of them alike; reported: ms per frame, median and min..max over the repeats. The kernel's own time is the class of the
covariance launch in vo_profile_* (VO_K_AUX) with the option on minus the same class with it off, per frame, in a run of its own.
Measurement tool, not a test. usage: python tests/measure/pose_covariance_cost.py [--frames 80] [--repeats 5]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

MONO = dict(W=752, H=480, K=(458.654, 457.296, 367.215, 248.375), NU=40, NV=25)
WARM = 12  # first frames, initialisation, the first keyframes
VO_K_AUX = 5


class TruePoseHook:
    def __init__(self, poses):
        self.poses, self.k = poses, 1

    def __call__(self, pts0, pts1):
        T10 = np.linalg.inv(self.poses[self.k]) @ self.poses[self.k - 1]
        return True, T10[:3, :3].astype(np.float32), T10[:3, 3].astype(np.float32), np.ones(len(pts0), bool)


class Stereo:
    def __init__(self, S, frames):
        self.W, self.H = S.KITTI_SIZE
        self.st = S.StereoStream(width=self.W, height=self.H, K=S.KITTI_K, n_u=60, n_v=25, seed=2, speed=0.8)
        self.K = S.KITTI_K
        self.imgs = [tuple(np.ascontiguousarray(a) for a in self.st.render_pair(p)[:2]) for p in self.st.poses(frames)]

    def upload(self, DeviceBuffer):
        self.dev = [(DeviceBuffer(L), DeviceBuffer(R)) for L, R in self.imgs]
        self.src = [((a.data_ptr(), self.W), (b.data_ptr(), self.W)) for a, b in self.dev]

    def free(self):
        for a, b in self.dev:
            a.free()
            b.free()

    def context(self, vo):
        return vo.Context(device=0, max_width=self.W, max_height=self.H, max_points=4024, n_slots=5, max_level=6)

    def make(self, vo, c, on):
        return vo.StereoVO(c, self.W, self.H, self.K, self.K, self.st.T_lr, 60, 25, thres_fastscore=15, window_size=21, max_level=6,
                           strict_border=4, local_ba=True, pose_covariance=on), None

    track = staticmethod(lambda o, s: o.trackStereoImages(*s))
    enqueue = staticmethod(lambda o, s: o.enqueue(*s))
    prefetch = staticmethod(lambda o, s: o.prefetch(*s))


class Mono:
    def __init__(self, S, frames):
        m = MONO
        self.W, self.H = m["W"], m["H"]
        st = S.StereoStream(width=m["W"], height=m["H"], K=m["K"], n_u=m["NU"], n_v=m["NV"], seed=2, speed=0.25)
        self.poses = st.poses(frames)
        self.imgs = [np.ascontiguousarray(st.render_pair(p)[0]) for p in self.poses]

    def upload(self, DeviceBuffer):
        self.dev = [DeviceBuffer(I) for I in self.imgs]
        self.src = [(d.data_ptr(), self.W) for d in self.dev]

    def free(self):
        for d in self.dev:
            d.free()

    def context(self, vo):
        return vo.Context(device=0, max_width=self.W, max_height=self.H, max_points=2 * MONO["NU"] * MONO["NV"] + 512, n_slots=3, max_level=5)

    def make(self, vo, c, on):
        hook = TruePoseHook(self.poses)
        return vo.MonoVO(c, self.W, self.H, MONO["K"], MONO["NU"], MONO["NV"], hook, thres_fastscore=15, window_size=15, max_level=5,
                         thres_error=20.0, thres_bidirection=1.0, thres_poseba_error=5, thres_sampson=1.0, thres_parallax=1.0,
                         thres_translation=3.0, strict_border=4, local_ba=True, pose_covariance=on), hook

    track = staticmethod(lambda o, s: o.trackImage(s))
    enqueue = staticmethod(lambda o, s: o.enqueue(s))
    prefetch = staticmethod(lambda o, s: o.prefetch(s))


def one_run(vo, cfg, mode, setting):
    """ms per frame of frames WARM .. n - 1"""
    src, n = cfg.src, len(cfg.src)
    on, read = setting in ("on", "on_read"), setting == "on_read"
    with cfg.context(vo) as c:
        o, hook = cfg.make(vo, c, on)

        def at(k):
            if hook is not None:
                hook.k = k

        if mode == "sync":
            for k in range(WARM):
                at(k)
                cfg.track(o, src[k])
            t0 = time.perf_counter()
            for k in range(WARM, n):
                at(k)
                cfg.track(o, src[k])
                if read:
                    o.getPoseCovariance()
            dt = time.perf_counter() - t0
        elif setting in ("on_read", "off_calls"):
            cfg.enqueue(o, src[0])
            cfg.prefetch(o, src[1])
            t0 = None
            for k in range(n):
                if k == WARM:
                    t0 = time.perf_counter()
                at(k)
                o.result()
                if read:  # (before the next frame is in flight: the getter is refused while one is)
                    o.getPoseCovariance()
                if k + 1 < n:
                    cfg.enqueue(o, src[k + 1])
                    if k + 2 < n:
                        cfg.prefetch(o, src[k + 2])
            dt = time.perf_counter() - t0
        else:
            o.runSequence(src, 0, WARM)
            t0 = time.perf_counter()
            o.runSequence(src, WARM, n)
            dt = time.perf_counter() - t0
        if on:
            cov = o.getPoseCovariance()
            assert cov.valid and (np.diag(cov.P) > 0).all()
        o.close()
    return 1e3 * dt / (n - WARM)


def kernel_us(vo, cfg):
    """us per frame of the VO_K_AUX class with the option on minus off (the covariance launch is the only difference)"""
    per = {}
    for on in (False, True):
        with cfg.context(vo) as c:
            o, hook = cfg.make(vo, c, on)
            for k in range(WARM):
                if hook is not None:
                    hook.k = k
                cfg.track(o, cfg.src[k])
            c.profile_enable(4096)
            c.profile_set_classes(1 << VO_K_AUX)
            m = min(len(cfg.src), WARM + 30)
            for k in range(WARM, m):
                if hook is not None:
                    hook.k = k
                cfg.track(o, cfg.src[k])
            c.synchronize()
            launches, ms = c.profile_get(VO_K_AUX)
            per[on] = (1e3 * ms / (m - WARM), launches / (m - WARM))
            o.close()
    return dict(us_per_frame=round(per[True][0] - per[False][0], 2), launches_per_frame=round(per[True][1] - per[False][1], 3))


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
        res = {}
        try:
            for mode, settings in (("sync", ("off", "on", "on_read")), ("look_ahead", ("off", "on", "off_calls", "on_read"))):
                one_run(vo, cfg, mode, "on")  # (untimed: code objects loaded, clocks up)
                t = {s: [] for s in settings}
                for _ in range(a.repeats):
                    for s in settings:
                        t[s].append(one_run(vo, cfg, mode, s))
                res[mode] = {s: dict(median=round(float(np.median(v)), 4), min=round(min(v), 4), max=round(max(v), 4)) for s, v in t.items()}
            res["kernel"] = kernel_us(vo, cfg)
        finally:
            cfg.free()
        out[name] = res
        print(json.dumps({name: res}), flush=True)
    out["unit"] = "ms per frame"
    out["frames_timed"], out["repeats"] = a.frames - WARM, a.repeats
    print(json.dumps(out))


if __name__ == "__main__":
    main()
