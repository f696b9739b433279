"""Stereo visual odometry over an image sequence on disk, configured by one of the reference's YAML files — what
`ros2 run visual_odometry stereo_vo_node` does with a rosbag, without ROS:

    python examples/run_stereo_sequence.py --config config/stereo/kitti_00_stereo.yaml \
        --left  /data/kitti/sequences/00/image_0 --right /data/kitti/sequences/00/image_1 \
        --trajectory frame_poses.txt [--keyframes keyframes.txt] [--max-frames N] [--covariance cov.txt]

Images: 8-bit grey PNG / PGM / JPEG ... (whatever PIL opens; colour is converted), paired by sorted file name. The next pair
is handed over while the current one is tracked (vo_svo_prefetch: upload, pyramids and keypoint detection run under the
frame in flight). Output: the reference's trajectory format (`id` + the 12 numbers of [R|t], `%.4f`,
stereo_vo.cpp:62-80), one line per frame; optionally every keyframe's current pose after the last frame. --covariance FILE: the
pose's covariance as a node would put it into nav_msgs::Odometry::pose.covariance (chained on the device behind every frame's
pose-only BA), one line per frame: the id, the 36 values (row-major; x, y, z, rot x, rot y, rot z), `valid` and
`n_unknown_steps` (frames whose pose did not come from the BA). --semidense DIR [--semidense-every frame] [--semidense-depth Z_MIN
[Z_MAX]]: semi-dense stereo depth of every keyframe's (every frame's) own pair, computed on the device behind the frame; one ASCII
PLY per result in DIR (`semidense_<frame id>.ply`: x y z in the world frame and the standard deviation of the inverse depth).
--semidense-temporal [--semidense-min-obs N]: with --semidense, every keyframe's result seeds a map that the following frames
update (the temporal search and fusion); `semidense_fused_<keyframe's frame id>.ply` holds the map's pixels with at least N (default
2) observations (N = 1 keeps what the static result alone gave), written when the next keyframe replaces the map and at the end
of the run. --semidense-propagate: with --semidense-temporal, a keyframe's map is carried over to the next keyframe (warped under
the odometry's pose, fused with the new static result) instead of being seeded afresh, so a keyframe's file also holds what earlier
keyframes observed. --semidense-world FILE.ply: with --semidense-temporal, every keyframe's map is fused into one world-frame voxel
map when the next keyframe replaces it (the last one at the end); FILE.ply has x y z grey count keyframes per voxel
(--semidense-voxel V: the voxel's edge, default 0.1 m; --semidense-world-min-keyframes N: only voxels N keyframes reached;
--semidense-world-reanchor [MIN_MOVE]: the map follows the local bundle adjustment, so that it agrees with the keyframe poses;
--semidense-world-carve [MARGIN]: every integration is followed by a free-space carve, FILE.ply gets a `free` property behind
`keyframes` — the number of later rays that passed through the voxel — and --semidense-world-max-free NUM DEN writes only the voxels
with free * DEN <= count * NUM; --semidense-world-source raw|regularized|dense|merged: what is integrated — with --dense DIR, `dense` is
every keyframe's dense result and `merged` the keyframe's map merged per pixel with it, so that the world map holds walls as well as
edges; --semidense-world-merge-chi C and --semidense-world-keep-obs N set that merge's gate and its rule for a disagreement).
--semidense-regularize: with --semidense-temporal, a regularised copy of the map is kept next to it (entries their
neighbours contradict removed, high-gradient holes whose neighbours agree filled, values smoothed) and written as
`semidense_regularized_<keyframe's frame id>.ply` wherever the fused file is written; its filled pixels have one observation, so N
applies to the measured ones only. --semidense-align FILE: with --semidense-temporal, every frame that is not a keyframe aligns its left image
photometrically against the keyframe's map, from the odometry's pose (a second pose estimate; nothing uses it); one line per frame:
frame id, keyframe's frame id (-1 at a keyframe frame), status (0 converged, 1 max_iters, 2 too few pixels, 3 singular, 4 none),
iterations, pixel count, rms in grey levels, the 12 numbers of the aligned [R|t] of T_wc, and its translation [m] and rotation
[degrees] distance to the odometry's pose. --semidense-align-levels N (1..6) runs that alignment coarse to fine on N levels of a map
pyramid, which converges from a frame's motion and more; --semidense-align-start previous then makes it an odometry of its own: the
identity at the first frame after a keyframe, afterwards the previous frame's aligned pose where that frame converged, else the
odometry's. With either, the line ends with the start that was used and "status:iterations:pixels" per level, level 0 first.
--semidense-align-affine: the alignment also estimates a gain and an offset of the keyframe's grey levels (for streams whose exposure
changes between a keyframe and its frames; status 5: they left their range); the line then carries the two behind the rotation
distance, in front of the start.
--dense DIR [--dense-every frame] [--dense-disparities N] [--dense-paths 4|8]: a dense disparity (census + semi-global matching) of
every keyframe's (or every frame's) pair, independent of --semidense; `dense_<frame id>.ply` per result in DIR, as the semi-dense
files. N (default 128) disparities are searched, ending at a depth of 3 m.
--dense-speckle [MAX_SIZE] [--dense-speckle-diff D]: with --dense, the speckle filter behind every dense result: connected components
(4-neighbours, disparities at most D = 1 px apart) of at most MAX_SIZE (default 100) pixels are left out of the files."""
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
    """--zncc THRES [--zncc-win N] [--zncc-stereo] as the `zncc_gate` argument of from_yaml: a track survives only where the ZNCC of its
    N x N patches (centred) exceeds THRES"""
    if args.zncc is None:
        if args.zncc_win is not None or args.zncc_stereo:
            raise SystemExit("--zncc-win / --zncc-stereo need --zncc")
        return {}
    win = 15 if args.zncc_win is None else args.zncc_win
    if not (win % 2 == 1 and 3 <= win <= 31) or args.zncc != args.zncc:
        raise SystemExit("--zncc: THRES is a number; --zncc-win: N is odd, 3..31")
    return {"zncc_gate": {"thres": args.zncc, "win": win, "pattern": "centered", "pairs": ("temporal", "stereo") if args.zncc_stereo else ("temporal",)}}


def dense_options(args):
    """--dense DIR [--dense-every frame] [--dense-disparities N] [--dense-paths 4|8] as the `dense` argument of from_yaml: a dense
    disparity (census + semi-global matching) of every keyframe's (or every frame's) pair; bf comes from the file's camera, the range
    from a smallest depth of 3 m. --dense-speckle [MAX_SIZE] [--dense-speckle-diff D]: its "speckle" entry"""
    if args.dense is None:
        if args.dense_every is not None or args.dense_disparities is not None or args.dense_paths is not None:
            raise SystemExit("--dense-every / --dense-disparities / --dense-paths need --dense DIR")
        if args.dense_speckle is not None or args.dense_speckle_diff is not None:
            raise SystemExit("--dense-speckle / --dense-speckle-diff need --dense DIR")
        return {}
    if args.dense_speckle is None and args.dense_speckle_diff is not None:
        raise SystemExit("--dense-speckle-diff needs --dense-speckle")
    if args.dense_speckle is not None and args.dense_speckle < 0:
        raise SystemExit("--dense-speckle MAX_SIZE: >= 0")
    if args.dense_speckle_diff is not None and not 0 <= args.dense_speckle_diff < float("inf"):
        raise SystemExit("--dense-speckle-diff D: finite and >= 0")
    if args.dense_disparities is not None and not 1 <= args.dense_disparities <= 256:
        raise SystemExit("--dense-disparities N: 1..256 (rounded up to 64, 128, 192 or 256)")
    ds = {"z_min": 3.0, "n_disp": args.dense_disparities or 128, "every": args.dense_every or "keyframe"}
    if args.dense_paths is not None:
        ds["paths"] = args.dense_paths
    if args.dense_speckle is not None:
        ds["speckle"] = {"max_size": args.dense_speckle}
        if args.dense_speckle_diff is not None:
            ds["speckle"]["max_diff"] = args.dense_speckle_diff
    return {"dense": ds}


def semidense_options(args):
    """--semidense DIR [--semidense-every frame] [--semidense-depth Z_MIN [Z_MAX]] as the `semidense` argument of from_yaml: semi-dense
    stereo depth of every keyframe's (or every frame's) pair; bf comes from the configured camera"""
    if args.semidense is None:
        if args.semidense_every is not None or args.semidense_depth is not None:
            raise SystemExit("--semidense-every / --semidense-depth need --semidense DIR")
        if args.semidense_temporal or args.semidense_min_obs is not None or args.semidense_propagate or args.semidense_align:
            raise SystemExit("--semidense-temporal / --semidense-min-obs / --semidense-propagate / --semidense-align need --semidense DIR")
        if args.semidense_regularize:
            raise SystemExit("--semidense-regularize needs --semidense DIR")
        if args.semidense_world or args.semidense_voxel is not None or args.semidense_world_min_keyframes is not None:
            raise SystemExit("--semidense-world / --semidense-voxel / --semidense-world-min-keyframes need --semidense DIR")
        if args.semidense_world_reanchor is not None:
            raise SystemExit("--semidense-world-reanchor needs --semidense DIR")
        if args.semidense_world_carve is not None or args.semidense_world_max_free is not None:
            raise SystemExit("--semidense-world-carve / --semidense-world-max-free need --semidense DIR")
        if args.semidense_world_source is not None or args.semidense_world_merge_chi is not None or args.semidense_world_keep_obs is not None:
            raise SystemExit("--semidense-world-source / --semidense-world-merge-chi / --semidense-world-keep-obs need --semidense DIR")
        return {}
    src = args.semidense_world_source
    if src is not None and not args.semidense_world:
        raise SystemExit("--semidense-world-source needs --semidense-world FILE.ply")
    if src in ("dense", "merged") and args.dense is None:
        raise SystemExit(f"--semidense-world-source {src} needs --dense DIR: the world map then reads every keyframe's dense result")
    if src == "regularized" and not args.semidense_regularize:
        raise SystemExit("--semidense-world-source regularized needs --semidense-regularize")
    if (args.semidense_world_merge_chi is not None or args.semidense_world_keep_obs is not None) and src not in ("dense", "merged"):
        raise SystemExit("--semidense-world-merge-chi / --semidense-world-keep-obs need --semidense-world-source dense | merged")
    if args.semidense_world_merge_chi is not None and not (0 < args.semidense_world_merge_chi < float("inf")):
        raise SystemExit("--semidense-world-merge-chi C: finite, > 0")
    if args.semidense_world_keep_obs is not None and not 0 <= args.semidense_world_keep_obs <= 256:
        raise SystemExit("--semidense-world-keep-obs N: 0..256")
    if args.semidense_world and not args.semidense_temporal:
        raise SystemExit("--semidense-world needs --semidense-temporal")
    if (args.semidense_voxel is not None or args.semidense_world_min_keyframes is not None) and not args.semidense_world:
        raise SystemExit("--semidense-voxel / --semidense-world-min-keyframes need --semidense-world FILE.ply")
    if args.semidense_world_reanchor is not None and (not args.semidense_world or not args.semidense_world_reanchor >= 0):
        raise SystemExit("--semidense-world-reanchor [MIN_MOVE]: voxels, >= 0, with --semidense-world FILE.ply")
    if args.semidense_world_carve is not None and (not args.semidense_world or not args.semidense_world_carve >= 1):
        raise SystemExit("--semidense-world-carve [MARGIN]: voxels, >= 1, with --semidense-world FILE.ply")
    if args.semidense_world_max_free is not None and (args.semidense_world_carve is None or min(args.semidense_world_max_free) < 0):
        raise SystemExit("--semidense-world-max-free NUM DEN: both >= 0, with --semidense-world-carve")
    if args.semidense_voxel is not None and not args.semidense_voxel > 0:
        raise SystemExit("--semidense-voxel V: metres, > 0")
    if args.semidense_world_min_keyframes is not None and args.semidense_world_min_keyframes < 1:
        raise SystemExit("--semidense-world-min-keyframes N: >= 1")
    if args.semidense_regularize and not args.semidense_temporal:
        raise SystemExit("--semidense-regularize needs --semidense-temporal")
    if args.semidense_propagate and not args.semidense_temporal:
        raise SystemExit("--semidense-propagate needs --semidense-temporal")
    if args.semidense_align and not args.semidense_temporal:
        raise SystemExit("--semidense-align needs --semidense-temporal")
    if (args.semidense_align_levels is not None or args.semidense_align_start is not None) and not args.semidense_align:
        raise SystemExit("--semidense-align-levels / --semidense-align-start need --semidense-align FILE")
    if args.semidense_align_affine and not args.semidense_align:
        raise SystemExit("--semidense-align-affine needs --semidense-align FILE")
    if args.semidense_align_levels is not None and not 1 <= args.semidense_align_levels <= 6:
        raise SystemExit("--semidense-align-levels N: 1..6")
    if args.semidense_min_obs is not None and (not args.semidense_temporal or not 1 <= args.semidense_min_obs <= 255):
        raise SystemExit("--semidense-min-obs N: 1..255, with --semidense-temporal")
    z = args.semidense_depth or [3.0]
    if len(z) > 2 or not (z[0] > 0 and (len(z) == 1 or z[1] >= z[0])):
        raise SystemExit("--semidense-depth: Z_MIN [Z_MAX] in metres, 0 < Z_MIN <= Z_MAX")
    sd = {"z_min": z[0], "every": args.semidense_every or "keyframe"}
    if len(z) == 2:
        sd["z_max"] = z[1]
    if args.semidense_temporal:
        sd["temporal"] = True
    if args.semidense_propagate:
        sd["propagate"] = True
    if args.semidense_regularize:
        sd["regularize"] = True
    if args.semidense_world:
        sd["world"] = True if args.semidense_voxel is None else {"voxel": args.semidense_voxel}
        if args.semidense_world_reanchor is not None:
            sd["world"] = dict({} if sd["world"] is True else sd["world"],
                               reanchor=True if args.semidense_world_reanchor == 0 else {"min_move": args.semidense_world_reanchor})
        if args.semidense_world_carve is not None:
            sd["world"] = dict({} if sd["world"] is True else sd["world"], carve={"margin": args.semidense_world_carve})
        if src is not None:
            sd["world"] = dict({} if sd["world"] is True else sd["world"], source=src)
            mg = {k: v for k, v in (("chi", args.semidense_world_merge_chi), ("keep_obs", args.semidense_world_keep_obs)) if v is not None}
            if mg:
                sd["world"]["merge"] = mg
    if args.semidense_align:
        sd["align"] = True
        if args.semidense_align_levels is not None or args.semidense_align_start is not None:
            sd["align"] = {"levels": args.semidense_align_levels or 4, "start": args.semidense_align_start or "odometry"}
        if args.semidense_align_affine:
            sd["align"] = dict({} if sd["align"] is True else sd["align"], affine=True)
    return {"semidense": sd}


def align_line(a, T_wc):
    """one line of --semidense-align: a = getSemiDenseAlign() of the frame whose odometry pose is T_wc"""
    E = np.linalg.inv(np.asarray(T_wc, np.float64)) @ a.T_wc.astype(np.float64)
    R = E[:3, :3]
    s = 0.5 * np.linalg.norm([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    dt, dr = (float(np.linalg.norm(E[:3, 3])), float(np.degrees(np.arcsin(min(s, 1.0))))) if a.status != 4 else (0.0, 0.0)
    tail = "" if a.gain is None else f" {a.gain:.6f} {a.offset:.4f}"  # (--semidense-align-affine)
    if a.levels is not None and len(a.levels) > 1:  # (coarse to fine: the start that was used, then every level's outcome)
        tail += f" {a.start} " + " ".join(f"{lv.status}:{lv.iters}:{lv.count}" for lv in a.levels)
    return (f"{a.frame_id} {a.key_frame_id} {a.status} {a.iters} {a.count} {a.rms:.4f} " + " ".join(f"{v:.6f}" for v in a.T_wc[:3].reshape(-1)) +
            f" {dt:.6f} {dr:.6f}{tail}\n")


def write_ply(path, xyz, sigma_invd):
    """one ASCII PLY: x y z and the standard deviation of the inverse depth per point"""
    with open(path, "w") as f:
        f.write("ply\nformat ascii 1.0\n" + f"element vertex {len(xyz)}\n" +
                "property float x\nproperty float y\nproperty float z\nproperty float sigma_invd\nend_header\n")
        for (x, y, z), s in zip(xyz, sigma_invd):
            f.write(f"{x:.6g} {y:.6g} {z:.6g} {s:.6g}\n")


def write_world_ply(path, w):
    """one ASCII PLY of a world map (a SemiDenseWorldPoints): x y z, grey, the points and the keyframes per voxel; of a
    SemiDenseWorldFreePoints (--semidense-world-carve) also the free count"""
    free = getattr(w, "free", None)
    with open(path, "w") as f:
        f.write("ply\nformat ascii 1.0\n" + f"element vertex {len(w.xyz)}\n" + "property float x\nproperty float y\nproperty float z\n"
                "property uchar grey\nproperty uint count\nproperty uint keyframes\n" + ("" if free is None else "property uint free\n") + "end_header\n")
        for i, ((x, y, z), g, c, k) in enumerate(zip(w.xyz, w.grey, w.count, w.keyframes)):
            f.write(f"{x:.6g} {y:.6g} {z:.6g} {int(g)} {int(c)} {int(k)}" + ("" if free is None else f" {int(free[i])}") + "\n")


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--config", required=True, help="a config/stereo/*.yaml file of the reference")
    ap.add_argument("--left", required=True, help="directory of the left images")
    ap.add_argument("--right", required=True, help="directory of the right images")
    ap.add_argument("--trajectory", default="frame_poses.txt")
    ap.add_argument("--keyframes", default=None, help="also write the keyframes' current poses there")
    ap.add_argument("--max-frames", type=int, default=0)
    ap.add_argument("--covariance", default=None, metavar="FILE", help="also write every frame's pose covariance (ROS form) there")
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--strict-border", type=int, default=4, help="see vo_stereo_frame_set_strict_border (0: masked border taps)")
    ap.add_argument("--no-local-ba", action="store_true")
    ap.add_argument("--sum-order", choices=("tree", "reference"), default="tree",
                    help="see vo_set_sum_order (reference: the reference's summation order, bit-exact against it; slower)")
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
    ap.add_argument("--zncc-stereo", action="store_true", help="--zncc also between the current left and right image")
    ap.add_argument("--semidense", default=None, metavar="DIR",
                    help="semi-dense stereo depth of every keyframe's pair: one ASCII PLY per result (world frame) into DIR")
    ap.add_argument("--semidense-every", choices=("keyframe", "frame"), default=None, help="a result per keyframe (default) or per frame")
    ap.add_argument("--semidense-depth", nargs="+", type=float, default=None, metavar="Z",
                    help="depth range Z_MIN [Z_MAX] in metres searched by --semidense (default 3, no upper end)")
    ap.add_argument("--semidense-temporal", action="store_true",
                    help="--semidense: fuse every keyframe's depth with the following frames; semidense_fused_<id>.ply per keyframe")
    ap.add_argument("--semidense-propagate", action="store_true",
                    help="--semidense-temporal: carry a keyframe's fused map over to the next keyframe instead of seeding it afresh")
    ap.add_argument("--semidense-regularize", action="store_true",
                    help="--semidense-temporal: also keep a regularised copy of the map; semidense_regularized_<id>.ply per keyframe")
    ap.add_argument("--semidense-world", default=None, metavar="FILE.ply",
                    help="--semidense-temporal: fuse every keyframe's map into one world-frame voxel map; one ASCII PLY at the end")
    ap.add_argument("--semidense-voxel", type=float, default=None, metavar="V", help="voxel edge of --semidense-world in metres (default 0.1)")
    ap.add_argument("--semidense-world-min-keyframes", type=int, default=None, metavar="N",
                    help="--semidense-world: write the voxels at least N keyframes have reached (default 1)")
    ap.add_argument("--semidense-world-reanchor", type=float, nargs="?", const=0.0, default=None, metavar="MIN_MOVE",
                    help="--semidense-world: the map follows the local BA: a keyframe's map is re-anchored where the BA moves the keyframe "
                         "(by MIN_MOVE voxels or more; default: any change)")
    ap.add_argument("--semidense-world-carve", type=float, nargs="?", const=2.0, default=None, metavar="MARGIN",
                    help="--semidense-world: free-space carving: every integration is followed by a march of the map's rays through the "
                         "table, to MARGIN voxels (default 2) in front of their surface; FILE.ply gets a `free` property")
    ap.add_argument("--semidense-world-source", choices=("raw", "regularized", "dense", "merged"), default=None,
                    help="--semidense-world: what is integrated: the keyframe's map (raw, the default), its regularised copy, the keyframe's "
                         "dense result (dense) or the map merged per pixel with that result (merged); dense and merged need --dense DIR")
    ap.add_argument("--semidense-world-merge-chi", type=float, default=None, metavar="C",
                    help="--semidense-world-source dense | merged: the map and the dense value agree within C sigma (default 3)")
    ap.add_argument("--semidense-world-keep-obs", type=int, default=None, metavar="N",
                    help="--semidense-world-source merged: where they disagree, a map entry with N observations or more is kept (default 2)")
    ap.add_argument("--semidense-world-max-free", type=int, nargs=2, default=None, metavar=("NUM", "DEN"),
                    help="--semidense-world-carve: write only the voxels with free * DEN <= count * NUM")
    ap.add_argument("--semidense-align", default=None, metavar="FILE",
                    help="--semidense-temporal: align every later frame's left image against the keyframe's map; one line per frame into FILE")
    ap.add_argument("--semidense-align-levels", type=int, default=None, metavar="N",
                    help="--semidense-align: coarse to fine on N levels (1..6; 4 with --semidense-align-start alone) of a map pyramid")
    ap.add_argument("--semidense-align-start", choices=("odometry", "previous"), default=None,
                    help="--semidense-align: start from the odometry's pose (default) or from the previous frame's aligned pose")
    ap.add_argument("--semidense-align-affine", action="store_true",
                    help="--semidense-align: estimate a gain and an offset of the keyframe's grey levels next to the pose; two more columns")
    ap.add_argument("--semidense-min-obs", type=int, default=None, metavar="N", help="observations a fused pixel needs (default 2)")
    ap.add_argument("--dense", default=None, metavar="DIR",
                    help="dense stereo disparity (census + semi-global matching) of every keyframe's pair; one ASCII PLY per result in DIR")
    ap.add_argument("--dense-every", choices=("keyframe", "frame"), default=None, help="a dense result per keyframe (default) or per frame")
    ap.add_argument("--dense-disparities", type=int, default=None, metavar="N",
                    help="disparities searched by --dense (default 128; rounded up to 64, 128, 192 or 256), ending at a depth of 3 m")
    ap.add_argument("--dense-paths", type=int, choices=(4, 8), default=None, help="aggregation paths of --dense (default 8)")
    ap.add_argument("--dense-speckle", type=int, nargs="?", const=100, default=None, metavar="MAX_SIZE",
                    help="--dense: remove connected components of at most MAX_SIZE (default 100) pixels from every dense result")
    ap.add_argument("--dense-speckle-diff", type=float, default=None, metavar="D",
                    help="--dense-speckle: neighbours belong to one component where their disparities differ by at most D (default 1.0) px")
    return ap.parse_args(argv)


def main():
    args = parse_args()
    import visual_odometry_ros_amd as V
    names_l, names_r = sorted(os.listdir(args.left)), sorted(os.listdir(args.right))
    n = min(len(names_l), len(names_r))
    if args.max_frames:
        n = min(n, args.max_frames)
    if n == 0:
        raise SystemExit("no image pairs found")
    svo = V.StereoVO.from_yaml(args.config, device=args.device, strict_border=args.strict_border, local_ba=not args.no_local_ba,
                               pose_covariance=bool(args.covariance), **mask_options(args), **clahe_options(args),
                               **zncc_options(args), **semidense_options(args), **dense_options(args))
    if args.semidense:
        os.makedirs(args.semidense, exist_ok=True)
    if args.dense:
        os.makedirs(args.dense, exist_ok=True)
    ds_last = -1
    sd_last, fused, regd = -1, None, None  # (fused, regd: the current keyframe's map and its regularised copy as points, as of the last frame)
    min_obs = args.semidense_min_obs or 2

    def write_fused():
        if fused is not None:
            write_ply(os.path.join(args.semidense, f"semidense_fused_{fused['frame_id']:06d}.ply"), fused["xyz"], fused["sigma_invd"])
        if regd is not None:
            write_ply(os.path.join(args.semidense, f"semidense_regularized_{regd['frame_id']:06d}.ply"), regd["xyz"], regd["sigma_invd"])
    cov_file = open(args.covariance, "w") if args.covariance else None
    align_file = open(args.semidense_align, "w") if args.semidense_align else None
    svo.ctx.sum_order = args.sum_order
    pair = lambda k: (load_grey(os.path.join(args.left, names_l[k])), load_grey(os.path.join(args.right, names_r[k])))  # noqa: E731
    ids, poses, n_kf = [], [], 0
    cur = pair(0)
    t0 = time.perf_counter()
    for k in range(n):
        svo.enqueue(*cur)
        nxt = pair(k + 1) if k + 1 < n else None  # (decoded while the GPU tracks frame k)
        if nxt is not None:
            svo.prefetch(*nxt)
        info = svo.result()
        ids.append(info.frame_id)
        poses.append(np.array(info.T_wc, np.float32).reshape(4, 4))
        n_kf += int(info.is_keyframe)
        if cov_file:
            cov = svo.getPoseCovariance()
            ros = V.pose_covariance_ros(cov.P, poses[-1])
            cov_file.write(f"{info.frame_id} " + " ".join(f"{v:.9e}" for v in ros) + f" {int(cov.valid)} {cov.n_unknown_steps}\n")
        if align_file:  # (this waits for the side stream: a caller that wants it hidden fetches a frame later)
            align_file.write(align_line(svo.getSemiDenseAlign(), poses[-1]))
        if args.semidense and (info.is_keyframe or args.semidense_every == "frame"):
            # (fetched here for simplicity: this waits for the result's launch; a caller that wants it hidden fetches a frame later)
            pts = svo.getSemiDensePoints(world=True)
            if pts is not None and pts["frame_id"] != sd_last:
                sd_last = pts["frame_id"]
                write_ply(os.path.join(args.semidense, f"semidense_{sd_last:06d}.ply"), pts["xyz"], pts["sigma_invd"])
        if args.dense and (info.is_keyframe or args.dense_every == "frame"):  # (fetched here for simplicity, as the semi-dense result)
            pts = svo.getDensePoints(world=True)
            if pts is not None and pts["frame_id"] != ds_last:
                ds_last = pts["frame_id"]
                write_ply(os.path.join(args.dense, f"dense_{ds_last:06d}.ply"), pts["xyz"], pts["sigma_invd"])
        if args.semidense and args.semidense_temporal:
            # (a keyframe has replaced the map by the time its result is here, so the map is taken after every frame — after a
            # keyframe it is the freshly seeded one, which is what gets written if the next frame is a keyframe again — and
            # written when the next keyframe comes: simple, at the price of a wait for the side stream per frame)
            if info.is_keyframe:
                write_fused()
            fused = svo.getSemiDensePoints(world=True, fused=True, min_obs=min_obs)
            if args.semidense_regularize:  # (a filled pixel has one observation: min_obs would drop what the option adds)
                regd = svo.getSemiDensePoints(world=True, fused=True, regularized=True, min_obs=1)
        if k % 100 == 0 or k == n - 1:
            t = poses[-1][:3, 3]
            print(f"frame {k:6d}: {info.n_tracks_out:5d} tracks, {n_kf:4d} keyframes, position ({t[0]:9.3f} {t[1]:9.3f} {t[2]:9.3f})", flush=True)
        cur = nxt
    dt = time.perf_counter() - t0
    if args.semidense and args.semidense_temporal:
        write_fused()
    if args.semidense_world:
        svo.flushSemiDenseWorld()  # (the last keyframe's map: no later keyframe replaces it)
        max_free = None if args.semidense_world_carve is None else tuple(args.semidense_world_max_free or (0, 0))
        wm = svo.getSemiDenseWorld(min_keyframes=args.semidense_world_min_keyframes or 1, max_free=max_free)
        write_world_ply(args.semidense_world, wm)
        st = svo.getSemiDenseWorldStats()
        print(f"world map: {len(wm.xyz)} voxels written of {st['occupied']} ({st['integrations']} keyframes integrated, {st['refused']} refused, "
              f"{st['inserted']} points) -> {args.semidense_world}")
        if args.semidense_world_carve is not None:
            cs = svo.getSemiDenseWorldCarveStats()
            print(f"world map carving: {cs['carves']} carves, {cs['rays']} rays ({cs['short_rays']} short), {cs['visits']} voxel visits, {cs['hits']} hits")
    V.write_trajectory(args.trajectory, ids, np.stack(poses))
    if args.keyframes:
        kfs = svo.getKeyframes()
        V.write_trajectory(args.keyframes, list(range(len(kfs))), np.stack([T for T, _ in kfs]) if kfs else np.zeros((0, 4, 4), np.float32))
    if cov_file:
        cov_file.close()
    if align_file:
        align_file.close()
    svo.close()
    print(f"{n} frames in {dt:.2f} s ({n / dt:.1f} frames/s incl. image decoding); trajectory -> {args.trajectory}")


if __name__ == "__main__":
    main()
