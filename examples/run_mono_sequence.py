"""Monocular visual odometry over an image sequence on disk, configured by one of the reference's YAML files — what
`ros2 run visual_odometry mono_vo_node` does with a rosbag, without ROS and without OpenCV: the essential-matrix pose of the
initialisation and of the 5-point fallback is the library's own (FivePointRansac, motion_estimator.thres_5p_error).

    python examples/run_mono_sequence.py --config config/mono/kitti_00.yaml \
        --images /data/kitti/sequences/00/image_0 --trajectory frame_poses.txt [--keyframes keyframes.txt] [--max-frames N]
        [--debug-images DIR] [--covariance cov.txt]

Images: 8-bit grey PNG / PGM / JPEG ... (whatever PIL opens; colour is converted), in sorted file-name order. The next image
is handed over while the current one is tracked (vo_mvo_prefetch). Output: the reference's trajectory format (`id` + the 12
numbers of [R|t], `%.4f`), one line per frame; optionally every keyframe's current pose after the last frame. Monocular
poses carry the scale of the first motion (unit length). --debug-images DIR: the reference's img_debug_ (showTracking /
showTrackingBA, drawn on the device) of every frame as DIR/debug_<frame>.ppm, a binary PPM in the channel order the node
publishes (bgr8), written without an image library; a frame that draws nothing repeats the previous picture. --covariance FILE:
the pose's covariance as a node would put it into nav_msgs::Odometry::pose.covariance, in map units (up to the stream's scale),
one line per frame: the id, the 36 values (row-major; x, y, z, rot x, rot y, rot z), `valid` and `n_unknown_steps` (frames whose
pose did not come from the pose-only BA: the first image, the initialisation, 5-point fallbacks)."""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def load_grey(path):
    from PIL import Image
    im = Image.open(path)
    if im.mode != "L":
        im = im.convert("L")
    return np.ascontiguousarray(np.asarray(im, dtype=np.uint8))


def write_ppm(path, img):
    """(H, W, 3) uint8 as a binary PPM (P6): header, then the bytes as they are"""
    with open(path, "wb") as f:
        f.write(b"P6\n%d %d\n255\n" % (img.shape[1], img.shape[0]))
        f.write(np.ascontiguousarray(img, np.uint8).tobytes())


def mask_options(args):
    """--mask / --mask-rectified as keyword arguments of from_yaml: the ignore mask every frame carries (0 = ignore)"""
    if args.mask and args.mask_rectified is not None:
        raise SystemExit("--mask and --mask-rectified exclude each other")
    if args.mask:
        from visual_odometry_ros_amd.config import read_pgm
        return {"mask": read_pgm(args.mask)}
    if args.mask_rectified is not None:
        if not 0 <= args.mask_rectified <= 31:
            raise SystemExit("--mask-rectified: ERODE is 0..31")
        return {"mask": "rectified", "mask_erode": args.mask_rectified}
    return {}


def clahe_options(args):
    """--clahe [CLIP] / --clahe-tiles X Y as the `equalize` argument of from_yaml: CLAHE on every image before the tracker"""
    if args.clahe is None:
        if args.clahe_tiles is not None:
            raise SystemExit("--clahe-tiles needs --clahe")
        return {}
    tiles = tuple(args.clahe_tiles) if args.clahe_tiles is not None else (8, 8)
    if not (args.clahe >= 0 and args.clahe < float("inf")) or not all(1 <= t <= 32 for t in tiles):
        raise SystemExit("--clahe: CLIP is finite and >= 0; --clahe-tiles: X and Y are 1..32")
    return {"equalize": {"clip_limit": args.clahe, "tiles": tiles}}


def zncc_options(args):
    """--zncc THRES [--zncc-win N] as the `zncc_gate` argument of from_yaml: a track survives only where the ZNCC of its
    N x N patches (centred) exceeds THRES"""
    if args.zncc is None:
        if args.zncc_win is not None:
            raise SystemExit("--zncc-win needs --zncc")
        return {}
    win = 15 if args.zncc_win is None else args.zncc_win
    if not (win % 2 == 1 and 3 <= win <= 31) or args.zncc != args.zncc:
        raise SystemExit("--zncc: THRES is a number; --zncc-win: N is odd, 3..31")
    return {"zncc_gate": {"thres": args.zncc, "win": win, "pattern": "centered", "pairs": ("temporal",)}}


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--config", required=True, help="a config/mono/*.yaml file of the reference")
    ap.add_argument("--images", required=True, help="directory of the images")
    ap.add_argument("--trajectory", default="frame_poses.txt")
    ap.add_argument("--keyframes", default=None, help="also write the keyframes' current poses there")
    ap.add_argument("--max-frames", type=int, default=0)
    ap.add_argument("--covariance", default=None, metavar="FILE", help="also write every frame's pose covariance (ROS form) there")
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--strict-border", type=int, default=4, help="see vo_stereo_frame_set_strict_border (0: masked border taps)")
    ap.add_argument("--no-local-ba", action="store_true")
    ap.add_argument("--debug-images", default=None, metavar="DIR", help="write the debug image of every frame there (binary PPM)")
    ap.add_argument("--mask", default=None, metavar="FILE.pgm",
                    help="ignore mask (binary PGM of the image's size, 0 = ignore): no keypoints and no surviving tracks there")
    ap.add_argument("--mask-rectified", nargs="?", type=int, const=0, default=None, metavar="ERODE",
                    help="with flagDoUndistortion: ignore what the rectification fills in, and ERODE (0..31, default 0) pixels around it")
    ap.add_argument("--clahe", nargs="?", type=float, const=40.0, default=None, metavar="CLIP",
                    help="equalise every image with CLAHE before the tracker (clip limit CLIP, default 40; 0: no clipping)")
    ap.add_argument("--clahe-tiles", nargs=2, type=int, default=None, metavar=("X", "Y"), help="CLAHE tile grid (default 8 8; each 1..32)")
    ap.add_argument("--zncc", type=float, default=None, metavar="THRES",
                    help="appearance gate: a track survives only where the ZNCC of its patches in the previous and the current image exceeds THRES")
    ap.add_argument("--zncc-win", type=int, default=None, metavar="N", help="patch size of --zncc (odd, 3..31; default 15)")
    return ap.parse_args(argv)


def main():
    args = parse_args()
    import visual_odometry_ros_amd as V
    names = sorted(os.listdir(args.images))
    n = len(names) if not args.max_frames else min(len(names), args.max_frames)
    if n == 0:
        raise SystemExit("no images found")
    mvo = V.MonoVO.from_yaml(args.config, device=args.device, strict_border=args.strict_border, local_ba=not args.no_local_ba,
                             debug_image=bool(args.debug_images), pose_covariance=bool(args.covariance), **mask_options(args), **clahe_options(args),
                             **zncc_options(args))
    cov_file = open(args.covariance, "w") if args.covariance else None
    if args.debug_images:
        os.makedirs(args.debug_images, exist_ok=True)
    image = lambda k: load_grey(os.path.join(args.images, names[k]))  # noqa: E731
    ids, poses, n_kf, n_5p = [], [], 0, 0
    cur = image(0)
    t0 = time.perf_counter()
    for k in range(n):
        mvo.enqueue(cur)
        nxt = image(k + 1) if k + 1 < n else None  # (decoded while the GPU tracks frame k)
        if nxt is not None:
            mvo.prefetch(nxt)
        info = mvo.result()
        ids.append(info.frame_id)
        poses.append(np.array(info.T_wc, np.float32).reshape(4, 4))
        n_kf += int(info.is_keyframe)
        if cov_file:
            cov = mvo.getPoseCovariance()
            ros = V.pose_covariance_ros(cov.P, poses[-1])
            cov_file.write(f"{info.frame_id} " + " ".join(f"{v:.9e}" for v in ros) + f" {int(cov.valid)} {cov.n_unknown_steps}\n")
        n_5p += int(info.used_five_point)
        if args.debug_images:
            write_ppm(os.path.join(args.debug_images, f"debug_{k:06d}.ppm"), mvo.getDebugImage())
        if k % 100 == 0 or k == n - 1:
            t = poses[-1][:3, 3]
            print(f"frame {k:6d}: {info.n_tracks_out:5d} tracks, {n_kf:4d} keyframes, {n_5p:4d} 5-point poses, "
                  f"position ({t[0]:9.3f} {t[1]:9.3f} {t[2]:9.3f})", flush=True)
        cur = nxt
    dt = time.perf_counter() - t0
    V.write_trajectory(args.trajectory, ids, np.stack(poses))
    if args.keyframes:
        kfs = mvo.getKeyframes()
        V.write_trajectory(args.keyframes, list(range(len(kfs))), np.stack([T for T, _ in kfs]) if kfs else np.zeros((0, 4, 4), np.float32))
    if cov_file:
        cov_file.close()
    mvo.close()
    print(f"{n} frames in {dt:.2f} s ({n / dt:.1f} frames/s incl. image decoding); trajectory -> {args.trajectory}")


if __name__ == "__main__":
    main()
