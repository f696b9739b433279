"""What ORB orientation + descriptors cost on the device: host-clock time per synchronous call of vo_orb_detect_and_compute
against vo_orb_detect on the same image (the difference is the feature's cost: the detection's kernels are the same),
of vo_orb_compute for the same keypoints, and of vo_orb_match_sets on the left / right sets, at 1241 x 376 and 3840 x 2160,
after warm-up. Kernel times: run under `rocprofv3 --kernel-trace --stats` (orb_describe_kernel, orb_match_kernel).
Measurement tool, not a test. usage: python tests/measure/orb_describe_cost.py [--calls 50]"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))


def timed(fn, calls):
    for _ in range(5):
        fn()
    t = []
    for _ in range(calls):
        t0 = time.perf_counter()
        fn()
        t.append(time.perf_counter() - t0)
    return dict(us_median=round(1e6 * float(np.median(t)), 1), us_min=round(1e6 * min(t), 1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=50)
    a = ap.parse_args()
    import visual_odometry_ros_amd as vo
    from visual_odometry_ros_amd import synthetic as S
    out = {}
    for (W, H) in ((1241, 376), (3840, 2160)):
        K = (0.58 * W, 0.58 * W, W / 2, H / 2)
        st = S.StereoStream(width=W, height=H, K=K, n_u=8, n_v=4, n_new=8, seed=4)
        L, R, _ = st.render_pair(st.poses(1)[0])
        with vo.Context(device=0, max_width=W, max_height=H, max_points=4096, n_slots=2, max_level=4) as c:
            fe = vo.FeatureExtractor(c)
            fe.initParams(W, H, 20, 12, THRES_FAST=15)
            c.set_image(0, L)
            c.set_image(1, R)
            xy, resp, octv, ang, size, desc = fe.extractAndComputeORB(0, set=0)
            fe.extractAndComputeORB(1, set=1)
            r = dict(keypoints=int(xy.shape[0]))
            r["detect"] = timed(lambda: fe.detect(0), a.calls)
            r["detect_and_compute"] = timed(lambda: fe.extractAndComputeORB(0, set=0), a.calls)
            r["detect_and_compute_unsteered"] = timed(lambda: fe.extractAndComputeORB(0, set=0, steer=False), a.calls)
            r["compute_caller_keypoints"] = timed(lambda: fe.compute(0, xy, octv), a.calls)
            fe.extractAndComputeORB(0, set=0)
            r["match_sets"] = timed(lambda: fe.matchSets(0, 1), a.calls)
            r["accepted"] = int((fe.matchSets(0, 1)[0] >= 0).sum())
        out[f"{W}x{H}"] = r
    print(json.dumps(out))


if __name__ == "__main__":
    main()
