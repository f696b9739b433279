"""What the nodes' image encodings and the debug image cost on the device, on one MI355X; three repeats, median and
min..max of the three:
  (a) vo_set_stereo_pair_rectified_device per call (enqueue + synchronize) for mono8, rgb8 and f32 at 1241 x 376 and 3840 x 2160
  (b) the rectified StereoVO loop (runSequence, device images) at 1241 x 376 with rgb8 against mono8 input, frames / s
  (c) the same loop with debug_image on against off, frames / s
Kernel times of the remap and render kernels: run under `rocprofv3 --kernel-trace --stats` (remap_level0_kernel<...>,
draw_cover_kernel, draw_resolve_kernel and the picture's device-to-host copy).
Measurement tool, not a test. usage: python tests/measure/node_io_cost.py [--calls 50] [--frames 40] [--only a|b|c]"""
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


def three(fn):
    v = sorted(fn() for _ in range(3))
    return dict(median=round(v[1], 2), min=round(v[0], 2), max=round(v[2], 2))


def colour(g):
    g = g.astype(np.int32)
    return np.stack([g, 3 * g // 4 + 20, (255 - g) // 3], -1).astype(np.uint8)


def ingest_cost(vo, DeviceBuffer, W, H, calls):
    rng = np.random.default_rng(0)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float32)
    mu, mv = xx + np.float32(0.37) + 3 * np.sin(yy / 50).astype(np.float32), yy + np.float32(0.61)
    out = {}
    with vo.Context(device=0, max_width=W, max_height=H, max_points=256, n_slots=2, max_level=4) as c:
        fp = C.POINTER(C.c_float)
        for cam in (0, 1):
            c.check(c.lib.vo_rectify_set_maps(c.handle, cam, mu.ctypes.data_as(fp), mv.ctypes.data_as(fp), W, H))
        g = rng.integers(0, 256, (H, W), dtype=np.uint8)
        for fmt, img in (("mono8", g), ("rgb8", colour(g)), ("f32", g.astype(np.float32))):
            c.set_input_format(fmt)
            d = DeviceBuffer(img)

            def call():
                c.set_stereo_pair_rectified_device(0, d.data_ptr(), 1, d.data_ptr(), W, H, img.strides[0])
                c.synchronize()

            def median_us():
                for _ in range(5):
                    call()
                t = []
                for _ in range(calls):
                    t0 = time.perf_counter()
                    call()
                    t.append(time.perf_counter() - t0)
                return 1e6 * float(np.median(t))
            out[fmt] = three(median_us)
            d.free()
        c.set_input_format("mono8")
    return out


def loop_fps(vo, DeviceBuffer, S, fmt, debug_image, frames):
    W, H = S.KITTI_SIZE
    st = S.StereoStream(width=W, height=H, K=S.KITTI_K, n_u=60, n_v=25, seed=2, speed=0.8)
    pairs = [st.render_pair(p)[:2] for p in st.poses(frames)]
    if fmt == "rgb8":
        pairs = [(colour(L), colour(R)) for L, R in pairs]
    Kl = np.array(S.KITTI_K, np.float32)
    D = np.array([-0.05, 0.01, 0.0003, -0.0002, 0.0], np.float32)
    out = []
    for _ in range(3):
        with vo.Context(device=0, max_width=W, max_height=H, max_points=4024, n_slots=5, max_level=6) as c:
            c.set_input_format(fmt)
            cam = vo.StereoCamera(c)
            cam.initParams(W, H, Kl, D, Kl, D)
            cam.setStereoPoseLeft2Right(st.T_lr)
            cam.initStereoCameraToRectify()
            svo = vo.StereoVO(c, W, H, cam.K_rect, cam.K_rect, cam.T_lr_rect, 60, 25, thres_fastscore=15, window_size=21, max_level=6,
                              strict_border=4, local_ba=True, thres_trans=1.0, rectify=True, debug_image=debug_image)
            dev = [(DeviceBuffer(L), DeviceBuffer(R)) for L, R in pairs]
            src = [((a.data_ptr(), L.strides[0]), (b.data_ptr(), L.strides[0])) for (a, b), (L, _) in zip(dev, pairs)]
            svo.runSequence(src, 0, 4)  # warm-up: first pair, first keyframes
            t0 = time.perf_counter()
            svo.runSequence(src, 4, frames)
            out.append((frames - 4) / (time.perf_counter() - t0))
            if debug_image:
                assert svo.getDebugImage().shape == (H, W, 3)
            svo.close()
            for a, b in dev:
                a.free()
                b.free()
    v = sorted(out)
    return dict(median=round(v[1], 1), min=round(v[0], 1), max=round(v[2], 1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--frames", type=int, default=40)
    ap.add_argument("--only", default="abc")
    a = ap.parse_args()
    import visual_odometry_ros_amd as vo
    from visual_odometry_ros_amd import synthetic as S
    from util import DeviceBuffer
    out = {}
    if "a" in a.only:
        out["a_pair_rectified_device_us"] = {f"{W}x{H}": ingest_cost(vo, DeviceBuffer, W, H, a.calls) for W, H in ((1241, 376), (3840, 2160))}
    if "b" in a.only:
        out["b_rectified_loop_fps"] = {fmt: loop_fps(vo, DeviceBuffer, S, fmt, False, a.frames) for fmt in ("mono8", "rgb8")}
    if "c" in a.only:
        out["c_debug_image_loop_fps"] = {str(on): loop_fps(vo, DeviceBuffer, S, "mono8", on, a.frames) for on in (False, True)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
