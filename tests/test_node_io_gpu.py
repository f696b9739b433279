"""The nodes' image encodings on the rectifying ingestion (vo_set_input_format) and the debug image drawn on the device
(vo_draw_tracking, vo_draw_tracking_ba; StereoVO(debug_image=True)), bit for bit against the numpy restatement of
include/vo_hip.h (tests/node_io_restatement.py) and, for the drivers, against the same driver fed pre-converted gray planes."""
import ctypes as C

import numpy as np
import pytest

import node_io_restatement as R
from util import DeviceBuffer

pytestmark = pytest.mark.gpu
W, H = 97, 61
EXTRA = 5  # bytes a source row is longer than its pixels (97*3+5 for the colour formats; odd for every format)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def nctx(vo):
    c = vo.Context(device=0, max_width=W, max_height=H, max_points=1024, n_slots=4, max_level=3)
    mu, mv = R.edge_case_maps(W, H)
    fp = C.POINTER(C.c_float)
    c.maps = ((mu, mv), (mu[::-1].copy(), mv[::-1].copy()))  # camera 0 / camera 1 (the same cases, upside down)
    for cam, (a, b) in enumerate(c.maps):
        c.check(c.lib.vo_rectify_set_maps(c.handle, cam, a.ctypes.data_as(fp), b.ctypes.data_as(fp), W, H))
    yield c
    c.close()


def _plain_pyramid(c, slot_ref, level0):
    c.set_input_format("mono8")
    c.set_image(slot_ref, level0)
    return [c.get_level(slot_ref, l) for l in range(1, 4)]


# ---- ingestion -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", ["rgb8", "bgr8", "mono16u", "mono16s", "f32"])
def test_formats_through_every_rectifying_entry_point(nctx, oracle, fmt):
    """97 x 61, source rows 5 bytes longer than their pixels, the edge-case maps: level 0 from host images, device images and the
    stereo-pair entry point equals the restatement (for the colour formats: the oracle's u8 remap of the restated gray image),
    the levels above equal the plain pyramid of that level 0."""
    c = nctx
    imgs = [R.make_image(fmt, W, H, seed=11 + k) for k in range(2)]
    refs = [R.ingest(imgs[k], fmt, *c.maps[k]) for k in range(2)]
    if fmt in ("rgb8", "bgr8"):
        for k in range(2):
            assert np.array_equal(refs[k], oracle.remap_linear_u8(R.gray(imgs[k], fmt == "bgr8"), *c.maps[k]))
    views = [R.strided(im, EXTRA) for im in imgs]  # (byte buffer, stride): rows 5 bytes longer than their pixels
    above = [_plain_pyramid(c, 3, refs[k]) for k in range(2)]
    c.set_input_format(fmt)
    assert c.input_format == fmt
    # host images (Context.set_image_rectified takes the array of the format; the strided buffer goes through the C call)
    for k in range(2):
        c.set_image_rectified(k, imgs[k], cam=k)
        assert np.array_equal(c.get_level(k, 0), refs[k]), (fmt, "host", k)
        buf, stride = views[k]
        c.check(c.lib.vo_set_image_rectified(c.handle, 2, C.c_void_p(buf.ctypes.data), W, H, stride, k))
        assert np.array_equal(c.get_level(2, 0), refs[k]), (fmt, "host, strided", k)
        for l in range(1, 4):
            assert np.array_equal(c.get_level(2, l), above[k][l - 1]), (fmt, k, l)
    # device images, one and a pair
    dev = [DeviceBuffer(v[0]) for v in views]
    try:
        for k in range(2):
            c.set_image_rectified_device(2, dev[k].data_ptr(), W, H, views[k][1], cam=k)
            c.synchronize()
            assert np.array_equal(c.get_level(2, 0), refs[k]), (fmt, "device", k)
        c.set_stereo_pair_rectified_device(0, dev[0].data_ptr(), 1, dev[1].data_ptr(), W, H, views[0][1])
        c.synchronize()
        for k in range(2):
            assert np.array_equal(c.get_level(k, 0), refs[k]), (fmt, "pair", k)
            for l in range(1, 4):
                assert np.array_equal(c.get_level(k, l), above[k][l - 1]), (fmt, "pair", k, l)
    finally:
        for d in dev:
            d.free()
        c.set_input_format("mono8")


@pytest.mark.parametrize("fmt", ["mono16u", "mono16s", "f32"])
def test_small_integers_equal_the_mono8_path(nctx, fmt):
    c = nctx
    img = R.make_image("mono8", W, H, seed=21)
    c.set_input_format("mono8")
    c.set_image_rectified(0, img, cam=0)
    want = c.get_level(0, 0)
    try:
        c.set_input_format(fmt)
        c.set_image_rectified(1, img.astype(R.DTYPES[fmt]), cam=0)
        assert np.array_equal(c.get_level(1, 0), want)
    finally:
        c.set_input_format("mono8")


def test_refusals(nctx, vo):
    c = nctx
    img = R.make_image("mono8", W, H, seed=1)
    rgb = R.make_image("rgb8", W, H, seed=1)
    d = DeviceBuffer(img)
    try:
        c.set_input_format("rgb8")
        for call in (lambda: c.set_image(0, img), lambda: c.set_image_device(0, d.data_ptr(), W, H, W),
                     lambda: c.set_stereo_pair_device(0, d.data_ptr(), 1, d.data_ptr(), W, H, W),
                     lambda: c.set_stereo_pair_host_async(0, img.ctypes.data, 1, img.ctypes.data, W, H, W)):
            with pytest.raises(vo.VoError) as e:
                call()
            assert e.value.code == -1 and "VO_PIX_MONO8" in str(e.value)  # VO_ERR_INVALID, and the message says why
        # arrays that do not match the context's format
        for bad in (img, rgb.astype(np.uint16), rgb[:, :, :2], img.astype(np.float32)):
            with pytest.raises(vo.VoError):
                c.set_image_rectified(0, bad, cam=0)
        c.set_image_rectified(0, rgb, cam=0)
        with pytest.raises(vo.VoError):
            c.check(c.lib.vo_set_input_format(c.handle, 6))
        with pytest.raises(ValueError):
            c.set_input_format("rgba8")
        assert c.input_format == "rgb8"
    finally:
        d.free()
        c.set_input_format("mono8")
    with pytest.raises(vo.VoError):
        c.set_image_rectified(0, rgb, cam=0)  # (mono8 takes planes)


def test_format_change_is_refused_while_a_frame_is_in_flight(vo):
    from visual_odometry_ros_amd import synthetic as S
    from visual_odometry_ros_amd.api import StereoFramePipeline, make_stereo_params
    st = S.StereoStream(width=320, height=200, K=(300.0, 300.0, 160.0, 100.0), n_u=10, n_v=6, n_new=10, seed=7, margin=5.0)
    poses = st.poses(2)
    L0, _, _ = st.render_pair(poses[0])
    L1, R1, _ = st.render_pair(poses[1])
    ts = st.track_set(0, poses[0], poses[1])
    with vo.Context(device=0, max_width=320, max_height=200, max_points=256, n_slots=3, max_level=3) as c:
        pipe = StereoFramePipeline(c, make_stereo_params(320, 200, 21, 3, 80.0, 0.5, 3.0, st.K, st.K, st.T_lr), strict_border=True)
        for k, im in enumerate((L0, L1, R1)):
            c.set_image(k, im)
        n0 = c.allocation_count()
        c.set_input_format("f32")
        n1 = c.allocation_count()
        c.set_input_format("rgb8")
        c.set_input_format("mono8")
        assert n1 == n0 + 2 and c.allocation_count() == n1  # the staging pair grows once per size, never shrinks
        pipe.enqueue(ts["pts_l0"], ts["pts_r0"], ts["Xp"], ts["dT_prior"], ts["pts_new"])
        with pytest.raises(vo.VoError) as e:
            c.set_input_format("rgb8")
        assert e.value.code == -1 and c.input_format == "mono8"
        pipe.result()
        c.set_input_format("rgb8")
        assert c.input_format == "rgb8"


# ---- drivers -----------------------------------------------------------------------------------------------------------
SW, SH, SK = 640, 240, (400.0, 400.0, 320.0, 120.0)


def _colour(g):
    g = g.astype(np.int32)
    return np.stack([g, 3 * g // 4 + 20, (255 - g) // 3], -1).astype(np.uint8)


@pytest.fixture(scope="module")
def rig():
    """the 640 x 240 distorted stereo rig of tests/test_stereo_vo_gpu.py::test_closed_loop_with_rectification, 6 frames, rendered in
    colour (R = g, G = 3g // 4 + 20, B = (255 - g) // 3) and as the gray planes the library makes of that"""
    from visual_odometry_ros_amd import synthetic as S
    st = S.StereoStream(width=SW, height=SH, K=SK, n_u=20, n_v=8, seed=9, speed=0.5)
    pairs = [st.render_pair(p)[:2] for p in st.poses(6)]
    colour = [(_colour(L), _colour(Rt)) for L, Rt in pairs]
    gray = [(R.gray(L), R.gray(Rt)) for L, Rt in colour]
    assert not np.array_equal(gray[0][0], pairs[0][0])  # (the conversion is not the identity on this palette)
    cams = dict(Kl=np.array(SK, np.float32), Kr=np.array([402.0, 401.0, 318.0, 121.0], np.float32),
                Dl=np.array([-0.08, 0.02, 0.0005, -0.0004, 0.0], np.float32), Dr=np.array([-0.07, 0.015, -0.0003, 0.0006, 0.0], np.float32),
                T_lr=(st.T_lr.astype(np.float64) @ S.se3_exp([0, 0, 0, 0.004, -0.006, 0.003])).astype(np.float32))
    return dict(colour=colour, gray=gray, **cams)


def _frame_record(info, tracks):
    keep = ("frame_id", "is_keyframe", "lba_ran", "n_tracks_in", "n_final", "n_new", "n_tracks_out")
    rec = {k: getattr(info, k) for k in keep if hasattr(info, k)}
    rec["T_wc"] = _bits(np.array(info.T_wc)).tolist()
    if tracks is not None:
        rec.update(ids=tracks["ids"].tolist(), flags=tracks["flags"].tolist(),
                   pts=_bits(tracks["pts_l"] if "pts_l" in tracks else tracks["pts"]).tolist())
    return rec


def _run_stereo(vo, rig, fmt, on_device, sequence, debug_image=False, collect=None):
    imgs = rig["colour"] if fmt == "rgb8" else rig["gray"]
    c = vo.Context(device=0, max_width=SW, max_height=SH, max_points=4096, n_slots=5, max_level=4)
    keep, out = [], []
    try:
        if fmt != "mono8":
            c.set_input_format(fmt)
        cam = vo.StereoCamera(c)
        cam.initParams(SW, SH, rig["Kl"], rig["Dl"], rig["Kr"], rig["Dr"])
        cam.setStereoPoseLeft2Right(rig["T_lr"])
        cam.initStereoCameraToRectify()
        kw = dict(debug_image=True) if debug_image else {}
        svo = vo.StereoVO(c, SW, SH, cam.K_rect, cam.K_rect, cam.T_lr_rect, 20, 8, thres_fastscore=15, window_size=21, max_level=4,
                          strict_border=4, local_ba=True, thres_trans=1.2, rectify=True, **kw)
        if on_device:
            for L, Rt in imgs:
                keep.append((DeviceBuffer(L), DeviceBuffer(Rt)))
            src = [((a.data_ptr(), L.strides[0]), (b.data_ptr(), L.strides[0])) for (a, b), (L, _) in zip(keep, imgs)]
        else:
            src = imgs
        if sequence:
            infos, _ = svo.runSequence(src)
            out = [_frame_record(i, None) for i in infos]
            out[-1].update(_frame_record(infos[-1], svo.getTracks()))
        else:
            for k, (L, Rt) in enumerate(src):
                info = svo.trackStereoImages(L, Rt)
                out.append(_frame_record(info, svo.getTracks()))
                if collect is not None:
                    collect(k, c, svo, info, cam)
        svo.close()
    finally:
        for a, b in keep:
            a.free()
            b.free()
        c.close()
    return out


@pytest.mark.parametrize("on_device", [False, True])
@pytest.mark.parametrize("sequence", [False, True])
def test_stereo_driver_rgb8_equals_pre_converted_gray(vo, rig, on_device, sequence):
    """6 frames of the rectified closed loop: poses, ids, pixels, flags and keyframe decisions with rgb8 input are the bits of the
    same driver fed the gray planes, for host and device images, through the synchronous call and through runSequence"""
    got = _run_stereo(vo, rig, "rgb8", on_device, sequence)
    want = _run_stereo(vo, rig, "mono8", on_device, sequence)
    assert got == want
    assert len(got) == 6 and len(got[-1]["ids"]) > 100 and any(r["is_keyframe"] for r in got[1:])


def _run_mono(vo, rig, fmt, on_device, sequence):
    imgs = [p[0] for p in (rig["colour"] if fmt == "rgb8" else rig["gray"])]
    c = vo.Context(device=0, max_width=SW, max_height=SH, max_points=2 * 20 * 8 + 512, n_slots=3, max_level=4)
    keep = []
    try:
        if fmt != "mono8":
            c.set_input_format(fmt)
        vo.Camera(c, 0).initParams(SW, SH, rig["Kl"], rig["Dl"])
        mvo = vo.MonoVO(c, SW, SH, SK, 20, 8, thres_fastscore=15, window_size=15, max_level=4, thres_translation=1.2, strict_border=4,
                        local_ba=True, rectify=True)  # (five_point=None: the library's 5-point solver)
        if on_device:
            keep = [DeviceBuffer(I) for I in imgs]
            src = [(d.data_ptr(), I.strides[0]) for d, I in zip(keep, imgs)]
        else:
            src = imgs
        if sequence:
            infos, _ = mvo.runSequence(src)
            out = [_frame_record(i, None) for i in infos]
            out[-1].update(_frame_record(infos[-1], mvo.getTracks()))
        else:
            out = [_frame_record(mvo.trackImage(I), mvo.getTracks()) for I in src]
        mvo.close()
    finally:
        for d in keep:
            d.free()
        c.close()
    return out


@pytest.mark.parametrize("on_device", [False, True])
@pytest.mark.parametrize("sequence", [False, True])
def test_mono_driver_rgb8_equals_pre_converted_gray(vo, rig, on_device, sequence):
    """the same on the left camera with the library's 5-point solver"""
    got = _run_mono(vo, rig, "rgb8", on_device, sequence)
    want = _run_mono(vo, rig, "mono8", on_device, sequence)
    assert got == want
    assert len(got) == 6 and len(got[-1]["ids"]) > 50


def test_from_yaml_takes_the_input_format(vo):
    import os
    root = os.path.dirname(os.path.abspath(__file__))
    path = os.path.join(root, "golden", "reference_config", "stereo", "exp_stereo2.yaml")
    svo = vo.StereoVO.from_yaml(path, input_format="rgb8")
    try:
        assert svo.ctx.input_format == "rgb8"
        if svo.prm.rectify:
            with pytest.raises(vo.VoError):
                svo.trackStereoImages(np.zeros((svo.height, svo.width), np.uint8), np.zeros((svo.height, svo.width), np.uint8))
    finally:
        svo.close()


# ---- debug image: operators ----------------------------------------------------------------------------------------------
def _points():
    """about 300 points: on and beyond every border, exact .5 coordinates, NaN, coincident points of different kinds"""
    rng = np.random.default_rng(4)
    inside = rng.uniform((0, 0), (W - 1, H - 1), (60, 2))
    border = [(0, 0), (W - 1, 0), (0, H - 1), (W - 1, H - 1), (-1, 10), (W, 10), (10, -1), (10, H), (-0.5, 20.5), (W - 0.5, 30.5),
              (40.5, -0.5), (41.5, H - 0.5), (-7, -7), (W + 6, H + 6), (-8, 30), (W + 7, 30), (2.5, 3.5), (3.5, 2.5), (1e6, 5), (5, -1e6)]
    bad = [(np.nan, 5.0), (5.0, np.nan), (2e9, 5.0), (-3e9, 1.0), (np.inf, 3.0)]
    p0 = np.array(list(inside) + border + bad, np.float32)
    p1 = (p0 + rng.uniform(-9, 9, p0.shape)).astype(np.float32)
    p1[:6] = p0[:6]                      # coincident points of two kinds: overlap order
    p1[6] = p0[6] + np.float32(0.25)     # nearly coincident: the same centre
    p1[60] = (W - 1, H - 1)              # one line across the whole image, corner to corner ...
    p0[61], p1[61] = (-40.0, 70.0), (150.0, -20.0)  # ... and one that starts and ends outside
    new = np.array(list(rng.uniform((-5, -5), (W + 5, H + 5), (110, 2))) + [tuple(p0[0]), tuple(p1[1]), (np.nan, np.nan)], np.float32)
    return p0, p1, new


def test_draw_operators_equal_the_restatement(nctx):
    c = nctx
    gray = R.make_image("mono8", W, H, seed=31)
    c.set_image(0, gray)
    p0, p1, new = _points()
    assert len(p0) + len(p1) + len(new) >= 280
    assert np.array_equal(c.draw_tracking(0, p0, p1, new), R.draw_tracking(gray, p0, p1, new))
    assert np.array_equal(c.draw_tracking(0, p0, p1[:40], new[:0]), R.draw_tracking(gray, p0, p1[:40], new[:0]))
    assert np.array_equal(c.draw_tracking_ba(0, p0, new), R.draw_tracking_ba(gray, p0, new))
    assert np.array_equal(c.draw_tracking_ba(0, new[:0], p1), R.draw_tracking_ba(gray, new[:0], p1))
    # n = 0: pure GRAY2RGB
    plain = np.repeat(gray[:, :, None], 3, 2)
    assert np.array_equal(c.draw_tracking(0, p0[:0], p0[:0], p0[:0]), plain)
    assert np.array_equal(c.draw_tracking_ba(0, p0[:0], p0[:0]), plain)
    # a padded output image; more lines than start points is refused
    out = np.full((H, 3 * W + 7), 0xAB, np.uint8)
    c.check(c.lib.vo_draw_tracking_ba(c.handle, 0, p0.ctypes.data, len(p0), new.ctypes.data, len(new), out.ctypes.data, out.strides[0]))
    assert np.array_equal(out[:, :3 * W].reshape(H, W, 3), R.draw_tracking_ba(gray, p0, new)) and (out[:, 3 * W:] == 0xAB).all()
    assert c.lib.vo_draw_tracking(c.handle, 0, p0.ctypes.data, 3, p1.ctypes.data, 4, None, 0, out.ctypes.data, out.strides[0]) == -1


def test_draw_properties_without_the_restatement(nctx):
    """every pixel further than 8 from all points and lines keeps its gray value in all three channels; the centre of every
    pts_proj square keeps it too (the square is hollow) unless another primitive covers it. The distance to a point is the
    larger of |dx| and |dy|: rect(6, 2) reaches 7 pixels along both axes, so its corners lie 9.9 from the centre in the Euclidean
    sense and no Euclidean bound of 8 could hold for the header's own rule; to a line it is the Euclidean one."""
    c = nctx
    gray = R.make_image("mono8", W, H, seed=32)
    c.set_image(0, gray)
    p0, p1, new = _points()
    pick = [0, 1, 2, 60, 61, 80, 81]  # few enough to leave ground untouched: three pairs inside, the two long lines, NaN, 2e9
    p0, p1, new = p0[pick], p1[pick], new[[0, 1, 2, 3, 4, 5, -1]]
    ok = np.isfinite(p0).all(1) & np.isfinite(p1).all(1) & (np.abs(p0) < 1e5).all(1) & (np.abs(p1) < 1e5).all(1)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)

    def dist_points(pts):
        pts = pts[np.isfinite(pts).all(1)].astype(np.float64)
        return np.maximum(np.abs(xx[..., None] - pts[:, 0]), np.abs(yy[..., None] - pts[:, 1])).min(-1)

    def dist_segments(a, b):
        a, b = a.astype(np.float64), b.astype(np.float64)
        d = b - a
        t = np.clip(((xx[..., None] - a[:, 0]) * d[:, 0] + (yy[..., None] - a[:, 1]) * d[:, 1]) / np.maximum((d ** 2).sum(1), 1e-12), 0, 1)
        return np.sqrt((xx[..., None] - (a[:, 0] + t * d[:, 0])) ** 2 + (yy[..., None] - (a[:, 1] + t * d[:, 1])) ** 2).min(-1)

    img = c.draw_tracking(0, p0, p1, new)
    far = (np.minimum(np.minimum(dist_points(p0), dist_points(p1)), dist_points(new)) > 8) & (dist_segments(p0[ok], p1[ok]) > 8)
    assert far.sum() > 50 and (img[far] == gray[far][:, None]).all()
    assert (img != np.repeat(gray[:, :, None], 3, 2)).any(2).sum() > 200  # (something was drawn)
    ba = c.draw_tracking_ba(0, p0, new)
    far = np.minimum(dist_points(p0), dist_points(new)) > 8
    assert (ba[far] == gray[far][:, None]).all()
    n_centres = 0
    for p in new[np.isfinite(new).all(1)]:
        cx, cy = int(np.rint(p[0])), int(np.rint(p[1]))
        others = np.concatenate([new[np.isfinite(new).all(1)], p0[np.isfinite(p0).all(1)]]).astype(np.float64)
        d = np.abs(np.rint(others) - (cx, cy)).max(1)
        if 0 <= cx < W and 0 <= cy < H and (np.sort(d)[1:] > 8).all():  # no other primitive near the centre
            assert (ba[cy, cx] == gray[cy, cx]).all()
            n_centres += 1
    assert n_centres >= 3


# ---- debug image: the stereo driver ----------------------------------------------------------------------------------------
def test_stereo_driver_debug_image(vo, rig):
    """the 6-frame stream with debug_image=True: every result equals the run without it; the first pair draws nothing (the image
    is empty); frame k's picture equals vo_draw_tracking_ba on the rectified current left image with pts empty and pts_proj = the
    frame's surviving landmarks (the first n_final of getTracks()); the option's three allocations are made by set(on) alone."""
    off_allocs, on_allocs, pics = [], [], []
    ctx2 = vo.Context(device=0, max_width=SW, max_height=SH, max_points=4096, n_slots=1, max_level=1)

    def collect_on(k, c, svo, info, cam):
        on_allocs.append(c.allocation_count())
        img = svo.getDebugImage()
        if k == 0:
            assert img.shape == (0, 0, 3)
            return
        ctx2.set_image(0, R.remap_u8(rig["gray"][k][0], *cam.maps()[0]))
        want = ctx2.draw_tracking_ba(0, np.zeros((0, 2), np.float32), svo.getTracks()["pts_l"][:info.n_final])
        assert img.shape == (SH, SW, 3) and np.array_equal(img, want), f"frame {k}"
        assert np.array_equal(svo.getDebugImage(), img)  # (asking again gives the same picture)
        pics.append((img != np.repeat(ctx2.get_level(0, 0)[:, :, None], 3, 2)).any(2).sum())

    try:
        on = _run_stereo(vo, rig, "mono8", False, False, debug_image=True, collect=collect_on)
        off = _run_stereo(vo, rig, "mono8", False, False, collect=lambda k, c, svo, info, cam: off_allocs.append(c.allocation_count()))
    finally:
        ctx2.close()
    assert on == off
    assert [a - b for a, b in zip(on_allocs, off_allocs)] == [3] * 6  # index plane, device picture, pinned picture: nothing per frame
    assert len(pics) == 5 and min(pics) > 2000  # (a hollow 15 x 15 square with a 3-pixel rim is 144 pixels: more than a dozen of them in every frame)
    # through the sequence loop and with device images: the same results, and the last frame's picture is there
    seq_on = _run_stereo(vo, rig, "rgb8", True, True, debug_image=True)
    seq_off = _run_stereo(vo, rig, "rgb8", True, True)
    assert seq_on == seq_off


def test_adapter_stereo_vo_takes_colour_pairs_and_publishes_the_debug_image(vo, rig, tmp_path):
    """tests/cpp/node_io_adapter_demo.cpp: the adapter's StereoVO with flagDoUndistortion is fed CV_8UC3 Mats and asked for
    getDebugImage() after every frame, as the ROS nodes do — the poses are the Python driver's bits (rgb8 input), the image is
    empty after the first pair, then a CV_8UC3 Mat, and the last one is the Python driver's picture."""
    import os
    import struct
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    libdir = os.path.join(root, "visual_odometry_ros_amd", "lib")
    stubs = os.path.join(root, "tests", "typecheck_stubs")
    exe = str(tmp_path / "node_io_adapter_demo")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-I", root, "-I", os.path.join(stubs, "thirdparty"), "-I", os.path.join(stubs, "reference"),
                           os.path.join(root, "tests", "cpp", "node_io_adapter_demo.cpp"), "-o", exe, "-L", libdir, "-lvo_hip",
                           f"-Wl,-rpath,{libdir}", "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib", "-lamdhip64"])
    n = 4
    blob = struct.pack("3i", n, SW, SH) + b"".join(np.asarray(rig[k], np.float32).tobytes() for k in ("Kl", "Kr", "Dl", "Dr", "T_lr"))
    blob += b"".join(L.tobytes() + Rt.tobytes() for L, Rt in rig["colour"][:n])
    inp, outp = tmp_path / "in.bin", tmp_path / "out.bin"
    inp.write_bytes(blob)
    subprocess.check_call([exe, str(inp), str(outp)])
    raw = outp.read_bytes()
    last = {}
    want = _run_stereo(vo, dict(rig, colour=rig["colour"][:n]), "rgb8", False, False, debug_image=True,
                       collect=lambda k, c, svo, info, cam: last.update(img=svo.getDebugImage()))
    assert len(raw) == n * (64 + 12) + SW * SH * 3
    for k in range(n):
        T = np.frombuffer(raw, np.float32, 16, k * 76)
        rows, cols, typ = np.frombuffer(raw, np.int32, 3, k * 76 + 64)
        assert _bits(T).tolist() == want[k]["T_wc"], f"frame {k}"
        assert (rows, cols, typ) == ((0, 0, -1) if k == 0 else (SH, SW, 16)), f"frame {k}"  # 16 = CV_8UC3
    pic = np.frombuffer(raw, np.uint8, SW * SH * 3, n * 76).reshape(SH, SW, 3)
    assert np.array_equal(pic, last["img"]) and (pic[:, :, 1] != pic[:, :, 0]).sum() > 2000
