"""What the semi-dense stereo depth (vo_semidense_stereo, vo_svo_set_semidense) costs on one MI355X, at 1241 x 376
with bf = 386.1, z_min = 3 m, z_max = inf (disparities 0..129), always against the same run with the option off:
  kernel       vo_semidense_stereo into device planes, one call at a time (the launch and the host's wait for it), per call; the
               same as candidate x disparity scores per second (the scores the definition asks for, and the lane-scores the
               launch executes: ranges padded to chunks of 64) and as a share of the v_dot4 issue rate (15 v_dot4_u32_u8 per
               score with the default 17 x 3 window; nominal rate: 256 CUs x 4 SIMDs x 32 lanes per cycle x 2.4 GHz)
  fractions    candidates / pixels and accepted / candidates on the stream's third pair
  loops        the stereo loop at BASELINE configs[1] (the stream and settings of pose_covariance_cost.py, device images), per
               frame, with every = keyframes and every = frames, through
                 sync        one trackStereoImages call per frame
                 look_ahead  result k, enqueue k + 1, prefetch k + 2, call by call from Python
The settings ALTERNATE within one run, every repeat on a fresh context; reported: median and min..max over the repeats.
Measurement tool, not a test.
usage: python tests/measure/semidense_cost.py [--frames 80] [--repeats 5]"""
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
DOT4_PER_SCORE = 15          # (2 hh + 1) x ceil((2 hw + 1) / 4) with hw = 8, hh = 1
DOT4_LANE_RATE = 256 * 4 * 32 * 2.4e9


def stats(v, nd=4):
    return dict(median=round(float(np.median(v)), nd), min=round(min(v), nd), max=round(max(v), nd))


def kernel(vo, DeviceBuffer, cfg, repeats, batch=50):
    from semidense_restatement import candidates
    L, R = cfg.imgs[2]
    h, w = L.shape
    d_min, d_max = vo.semidense_disparity_range(BF, Z_MIN)
    cand, _, _ = candidates(L)
    xs = np.arange(w)[None, :].repeat(h, 0)[cand]
    nd = np.minimum(d_max, xs - 8) - d_min + 1
    nd = nd[nd >= 2 * 2 + 3]
    scores, lane_scores = int(nd.sum()), int(((nd + 63) // 64 * 64).sum())
    bufs = {k: DeviceBuffer(np.zeros((h, w), np.uint8 if k == "status" else np.float32)) for k in ("disparity", "score", "sigma_invd", "status")}
    t = []
    try:
        with vo.Context(device=0, max_width=w, max_height=h, max_points=256, n_slots=2, max_level=0) as c:
            c.set_image(0, L)
            c.set_image(1, R)
            out = {k: b.data_ptr() for k, b in bufs.items()}
            call = lambda: c.semiDenseStereo(0, 1, out=out, bf=BF, z_min=Z_MIN)  # noqa: E731
            call()
            for _ in range(repeats):
                t0 = time.perf_counter()
                for _k in range(batch):
                    call()
                t.append(1e6 * (time.perf_counter() - t0) / batch)
            r = c.semiDenseStereo(0, 1, bf=BF, z_min=Z_MIN)
    finally:
        for b in bufs.values():
            b.free()
    us = float(np.median(t))
    return {"call_us": stats(t, 1), "disparities": [d_min, d_max], "candidates": int(cand.sum()), "candidate_fraction": round(float(cand.mean()), 4),
            "accepted": r.n_accepted, "accepted_fraction": round(r.n_accepted / max(int(cand.sum()), 1), 4),
            "scores": scores, "lane_scores": lane_scores, "scores_per_s": round(scores / (us * 1e-6), -6),
            "lane_scores_per_s": round(lane_scores / (us * 1e-6), -6),
            "dot4_share_of_nominal_issue_rate": round(lane_scores * DOT4_PER_SCORE / (us * 1e-6) / DOT4_LANE_RATE, 4)}


def one_run(vo, cfg, mode, every):
    src, n = cfg.src, len(cfg.src)
    n_kf = 0
    with cfg.context(vo) as c:
        o, _ = cfg.make(vo, c, False)
        if every:
            o.setSemiDense(dict(bf=BF, z_min=Z_MIN), every=every)
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
            o.getSemiDense()  # (the last launch belongs to the run)
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
    out["unit"] = "loops: ms per frame; kernel: us per call"
    out["frames_timed"], out["repeats"] = a.frames - WARM, a.repeats
    print(json.dumps(out))


if __name__ == "__main__":
    main()
