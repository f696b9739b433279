"""What the reference summation order costs (vo_set_sum_order): the closed StereoVO loop at BASELINE configs[1]'s shape
(1241x376, 60x25 buckets, win 21, 6 levels, local BA) and the closed MonoVO loop at configs[2]'s (752x480, 40x25 buckets,
win 15, 5 levels, local BA), each in both orders, steady-state frames/s over --steps frames after --warmup. The rendered
frames are played back and forth (the mono loop's 5-point hook gets the true pose of the frame actually played).
Measurement tool, not a test. usage: python tests/measure/sum_order_cost.py [--steps 400] [--warmup 20] [--frames 12]"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
MONO_K = (458.654, 457.296, 367.215, 248.375)


def _playback(n_rendered, n):
    period = 2 * (n_rendered - 1)
    return [k % period if k % period < n_rendered else period - k % period for k in range(n)]


def _loop(enqueue, prefetch, result, seq, warmup):
    t0 = None
    for k, i in enumerate(seq):
        if k == warmup:
            t0 = time.perf_counter()
        enqueue(i)
        if k + 1 < len(seq):
            prefetch(seq[k + 1])
        result()
    return (len(seq) - warmup) / (time.perf_counter() - t0)


def stereo(V, S, order, args):
    W, H = S.KITTI_SIZE
    st = S.StereoStream(width=W, height=H, K=S.KITTI_K, n_u=60, n_v=25, seed=2, speed=0.8)
    imgs = [st.render_pair(p)[:2] for p in st.poses(args.frames)]
    seq = _playback(args.frames, args.warmup + args.steps)
    with V.Context(device=0, max_width=W, max_height=H, max_points=8192, n_slots=5, max_level=6, sum_order=order) as c:
        svo = V.StereoVO(c, W, H, S.KITTI_K, S.KITTI_K, st.T_lr, 60, 25, thres_fastscore=15, window_size=21, max_level=6,
                         strict_border=4, local_ba=True, thres_trans=1.0)
        fps = _loop(lambda i: svo.enqueue(*imgs[i]), lambda i: svo.prefetch(*imgs[i]), svo.result, seq, args.warmup)
        svo.close()
    return fps


def mono(V, S, order, args):
    W, H = 752, 480
    st = S.StereoStream(width=W, height=H, K=MONO_K, n_u=40, n_v=25, seed=5, speed=0.25)
    poses = st.poses(args.frames)
    imgs = [st.render_pair(p)[0] for p in poses]
    seq = _playback(args.frames, args.warmup + args.steps)
    state = {"k": 0}

    def hook(pts0, pts1):  # the true relative pose of the played frame against the one before it
        k = state["k"]
        T10 = np.linalg.inv(poses[seq[k]]) @ poses[seq[k - 1]]
        return True, T10[:3, :3].astype(np.float32), T10[:3, 3].astype(np.float32), np.ones(len(pts0), bool)

    def enqueue(i):
        mvo.enqueue(imgs[i])

    def result():
        mvo.result()
        state["k"] += 1

    with V.Context(device=0, max_width=W, max_height=H, max_points=8192, n_slots=3, max_level=5, sum_order=order) as c:
        mvo = V.MonoVO(c, W, H, MONO_K, 40, 25, hook, thres_fastscore=15, window_size=15, max_level=5, thres_error=20.0,
                       thres_bidirection=1.0, thres_poseba_error=5, thres_sampson=1.0, thres_parallax=1.0, thres_translation=2.5,
                       strict_border=4, local_ba=True)
        fps = _loop(enqueue, lambda i: mvo.prefetch(imgs[i]), result, seq, args.warmup)
        mvo.close()
    return fps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=400)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--frames", type=int, default=12)
    args = ap.parse_args()
    import visual_odometry_ros_amd as V
    from visual_odometry_ros_amd import synthetic as S
    V.load()
    out = {}
    for name, fn in (("stereo_configs1", stereo), ("mono_configs2", mono)):
        for order in ("tree", "reference"):
            out[f"{name}_{order}_fps"] = round(fn(V, S, order, args), 1)
            print(json.dumps({f"{name}_{order}_fps": out[f"{name}_{order}_fps"]}), flush=True)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
