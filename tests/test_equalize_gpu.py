"""CLAHE equalisation in front of the ingestion (vo_set_equalize) on the GPU, bit for bit: the operator against the
numpy restatement (tests/clahe_restatement.py); every ingestion entry point and both drivers with equalisation on and raw images
against the same code with equalisation off and restatement-equalised images; off is off; the refusals."""
import ctypes as C

import numpy as np
import pytest

import node_io_restatement as R
from clahe_restatement import clahe
from test_equalize_emu import SHAPES, make_image
from util import DeviceBuffer

pytestmark = pytest.mark.gpu
BIG = (1241, 376, (8, 8))  # rows extended by a full 8 (376 divides, 1241 does not): th = 48
SPLIT = (1241, 376, (2, 3))  # tiles of 621 x 126 pixels: ten histogram workgroups share a tile's counters and ticket


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _download(dev, nbytes):
    out = np.empty(nbytes, np.uint8)
    assert dev.hip.hipMemcpy(C.c_void_p(out.ctypes.data), dev.ptr, C.c_size_t(nbytes), 2) == 0  # D2H
    return out


@pytest.fixture(scope="module")
def octx(vo):
    c = vo.Context(device=0, max_width=1241, max_height=376, max_points=256, n_slots=2, max_level=2)
    yield c
    c.close()


# ---- the operator ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h,tiles,clip0", SHAPES + [BIG + (40.0,), SPLIT + (40.0,)])
def test_operator_equals_restatement(octx, w, h, tiles, clip0):
    """vo_equalize_image: look-up tables and bytes equal the restatement for clip 40, 2 and 0 (and the shape's own); a host image,
    a host image with padded rows, and a device image with padded rows into a padded device destination"""
    c = octx
    img = make_image("half" if (w, h) == (72, 45) else "noise", w, h, seed=3)
    low = make_image("low", w, h, seed=4)
    for clip in sorted({clip0, 40.0, 2.0, 0.0}):
        c.set_equalize("clahe", clip, tiles)
        assert c.equalize == {"mode": "clahe", "clip_limit": clip, "tiles": tiles}
        want, want_luts = clahe(img, clip, tiles)
        out, luts = c.equalizeImage(img)
        assert np.array_equal(luts, want_luts), (clip, "tables")
        assert np.array_equal(out, want), (clip, "host")
        buf, stride = R.strided(low, 7)
        padded = np.lib.stride_tricks.as_strided(buf, (h, w), (stride, 1))
        want2, want_luts2 = clahe(low, clip, tiles)
        out2, luts2 = c.equalizeImage(padded)
        assert np.array_equal(luts2, want_luts2) and np.array_equal(out2, want2), (clip, "host, padded rows")
        # device source with padded rows, device destination with other padded rows, device tables
        dst_stride = w + 11
        src = DeviceBuffer(buf)
        dst = DeviceBuffer(np.full(h * dst_stride + tiles[0] * tiles[1] * 256, 0xCD, np.uint8))
        try:
            c.check(c.lib.vo_equalize_image(c.handle, src.ptr, stride, w, h, dst.ptr, dst_stride, C.c_void_p(dst.data_ptr() + h * dst_stride), 1))
            raw = _download(dst, h * dst_stride + tiles[0] * tiles[1] * 256)
            got = raw[:h * dst_stride].reshape(h, dst_stride)
            assert np.array_equal(got[:, :w], want2) and (got[:, w:] == 0xCD).all(), (clip, "device")
            assert np.array_equal(raw[h * dst_stride:].reshape(want_luts2.shape), want_luts2)
            assert np.array_equal(_download(src, buf.nbytes), buf)  # the caller's image is only read
            o3, l3 = c.equalizeImage((src.data_ptr(), stride, w, h))
            assert np.array_equal(o3, want2) and np.array_equal(l3, want_luts2)
        finally:
            src.free()
            dst.free()
    c.set_equalize(None)
    assert c.equalize is None


# ---- every ingestion entry point ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("side", [False, True])
@pytest.mark.parametrize("w,h", [(160, 120), (163, 117)])
def test_every_ingestion_entry_point(vo, w, h, side):
    """equalisation on + the raw image(s) gives, level by level, what the same context gives with equalisation off and the
    restatement-equalised image(s): the plain and the rectifying entry points, host and device images, single images and pairs
    whose two images differ (a shared table would show), ingestion on the main and on the side stream"""
    nl = 3
    c = vo.Context(device=0, max_width=w, max_height=h, max_points=256, n_slots=4, max_level=nl - 1)
    dev = []
    try:
        maps = R.edge_case_maps(w, h)
        fp = C.POINTER(C.c_float)
        for cam, (a, b) in enumerate((maps, (maps[0][::-1].copy(), maps[1][::-1].copy()))):
            c.check(c.lib.vo_rectify_set_maps(c.handle, cam, a.ctypes.data_as(fp), b.ctypes.data_as(fp), w, h))
        c.set_ingest_side_stream(side)
        raw = [make_image("low", w, h, seed=21), make_image("half", w, h, seed=22)]
        tiles, clip = (8, 8), 40.0
        pre = [clahe(im, clip, tiles)[0] for im in raw]
        assert not np.array_equal(clahe(raw[1], clip, tiles)[1], clahe(raw[0], clip, tiles)[1])
        stride = w + 9
        views = {"raw": [R.strided(im, 9)[0] for im in raw], "pre": [R.strided(im, 9)[0] for im in pre]}
        dbuf = {k: [DeviceBuffer(b) for b in v] for k, v in views.items()}
        dev = dbuf["raw"] + dbuf["pre"]
        host = {"raw": raw, "pre": pre}

        def levels(slots):
            c.synchronize()
            return [[c.get_level(s, l) for l in range(nl)] for s in slots]

        def ingest(kind, which):
            d, hs = dbuf[which], host[which]
            if kind == "set_image":
                c.set_image(0, hs[1])
                return levels([0])
            if kind == "set_image_device":
                c.set_image_device(1, d[0].data_ptr(), w, h, stride)
                return levels([1])
            if kind == "pair_device":
                c.set_stereo_pair_device(2, d[0].data_ptr(), 3, d[1].data_ptr(), w, h, stride)
                return levels([2, 3])
            if kind == "pair_host_async":
                c.set_stereo_pair_host_async(0, views[which][0].ctypes.data, 1, views[which][1].ctypes.data, w, h, stride)
                return levels([0, 1])
            if kind == "rectified":
                c.set_image_rectified(2, hs[0], cam=1)
                return levels([2])
            if kind == "rectified_device":
                c.set_image_rectified_device(3, d[1].data_ptr(), w, h, stride, cam=0)
                return levels([3])
            c.set_stereo_pair_rectified_device(1, d[1].data_ptr(), 2, d[0].data_ptr(), w, h, stride)
            return levels([1, 2])

        for kind in ("set_image", "set_image_device", "pair_device", "pair_host_async", "rectified", "rectified_device", "pair_rectified_device"):
            c.set_equalize(None)
            want = ingest(kind, "pre")
            plain = ingest(kind, "raw")
            c.set_equalize("clahe", clip, tiles)
            got = ingest(kind, "raw")
            for s, (g, wnt, p) in enumerate(zip(got, want, plain)):
                for l in range(nl):
                    assert np.array_equal(g[l], wnt[l]), (kind, s, l)
                assert not np.array_equal(g[0], p[0]), kind  # (equalisation does something to this image)
            if "rectified" not in kind:
                assert np.array_equal(got[0][0], pre[1] if kind == "set_image" else pre[0]), kind  # level 0 IS the equalised image
        for k, d in enumerate(dbuf["raw"]):
            assert np.array_equal(_download(d, views["raw"][k].nbytes), views["raw"][k])  # the caller's device images: untouched
    finally:
        for d in dev:
            d.free()
        c.close()


# ---- both drivers --------------------------------------------------------------------------------------------------------------
SW, SH, SK = 640, 240, (400.0, 400.0, 320.0, 120.0)
NF = 8
EQ = dict(clip_limit=40.0, tiles=(8, 8))


@pytest.fixture(scope="module")
def stream():
    """the 640 x 240 synthetic stereo stream of the closed-loop tests, 8 frames, compressed to a quarter of its contrast around
    mid-grey; `pre`: every image equalised by the restatement, each on its own"""
    from visual_odometry_ros_amd import synthetic as S
    st = S.StereoStream(width=SW, height=SH, K=SK, n_u=20, n_v=8, seed=5, speed=0.5)
    low = lambda im: (128 + (im.astype(np.int32) - 128) // 4).astype(np.uint8)  # noqa: E731
    raw = [tuple(low(im) for im in st.render_pair(p)[:2]) for p in st.poses(NF)]
    pre = [tuple(clahe(im, EQ["clip_limit"], EQ["tiles"])[0] for im in pair) for pair in raw]
    mask = np.full((SH, SW), 255, np.uint8)
    mask[SH - 50:] = 0
    mask[40:120, 200:330] = 0
    return dict(raw=raw, pre=pre, T_lr=st.T_lr, mask=mask)


def _record(info, tracks, extra=None):
    keep = ("frame_id", "is_keyframe", "lba_ran", "n_tracks_in", "n_final", "n_new", "n_tracks_out")
    rec = {k: getattr(info, k) for k in keep}
    rec["T_wc"] = _bits(np.array(info.T_wc)).tolist()
    if tracks is not None:
        rec.update(ids=tracks["ids"].tolist(), flags=tracks["flags"].tolist(),
                   pts=_bits(tracks["pts_l"] if "pts_l" in tracks else tracks["pts"]).tolist(), Xw=_bits(tracks["Xw"]).tolist())
    if extra:
        rec.update(extra)
    return rec


def _drive(vo, stream, which, equalize, stereo, mode, on_device, debug=False, mask=False, toggle_first=False, allocs=None):
    """one run of a driver over the stream; mode: "sync" (the synchronous call), "ahead" (enqueue / prefetch / result), "run"""
    pairs = stream[which]
    c = vo.Context(device=0, max_width=SW, max_height=SH, max_points=4096, n_slots=5 if stereo else 3, max_level=4)
    keep, out = [], []
    try:
        if toggle_first:  # had the option on once (everything allocated), off again before the driver exists
            c.set_equalize("clahe", **EQ)
            c.equalizeImage(pairs[0][0])
            c.set_equalize(None)
        if equalize:
            c.set_equalize("clahe", **EQ)
        kw = dict(debug_image=True) if debug else {}
        if mask:
            kw["mask"] = stream["mask"]
        if stereo:
            drv = vo.StereoVO(c, SW, SH, SK, SK, stream["T_lr"], 20, 8, thres_fastscore=15, window_size=21, max_level=4, strict_border=4,
                              local_ba=True, thres_trans=0.9, **kw)
        else:
            drv = vo.MonoVO(c, SW, SH, SK, 20, 8, thres_fastscore=15, window_size=15, max_level=4, thres_translation=0.9, strict_border=4,
                            local_ba=True, **kw)
        if on_device:
            keep = [tuple(DeviceBuffer(im) for im in pair) for pair in pairs]
            src = [tuple((d.data_ptr(), SW) for d in pair) for pair in keep]
        else:
            src = pairs
        if not stereo:
            src = [p[0] for p in src]
        one = (lambda f, a: f(*a)) if stereo else (lambda f, a: f(a))

        def rec(info):
            extra = {}
            if stereo and not info.is_first:  # (the first pair has no step [10])
                npts = drv.getNewPoints()
                extra["new"] = _bits(npts["pts_l"]).tolist() + npts["accept"].tolist()
            if debug:
                extra["picture"] = drv.getDebugImage().tobytes()
            if allocs is not None:
                allocs.append(c.allocation_count())
            return _record(info, drv.getTracks(), extra)

        if mode == "run":
            infos, _ = drv.runSequence(src)
            out = [_record(i, None) for i in infos]
            out[-1] = rec(infos[-1])
        elif mode == "sync":
            track = drv.trackStereoImages if stereo else drv.trackImage
            out = [rec(one(track, a)) for a in src]
        else:
            one(drv.enqueue, src[0])
            for k in range(len(src)):
                if k + 1 < len(src):
                    one(drv.prefetch, src[k + 1])
                out.append(rec(drv.result()))
                if k + 1 < len(src):
                    one(drv.enqueue, src[k + 1])
        drv.close()
    finally:
        for pair in keep:
            for d in pair:
                d.free()
        c.close()
    return out


@pytest.mark.parametrize("mode,on_device,debug,mask", [("sync", False, True, False), ("sync", True, False, True), ("ahead", False, False, False),
                                                       ("ahead", True, True, False), ("run", True, False, False), ("run", False, False, False)])
@pytest.mark.parametrize("stereo", [True, False])
def test_driver_equals_pre_equalised_run(vo, stream, stereo, mode, on_device, debug, mask):
    """8 low-contrast frames: equalisation on + raw images gives the bits of equalisation off + pre-equalised images — poses, ids,
    pixels, landmarks, flags, counts, keyframe and local-BA decisions, the new points, the debug picture — through the
    synchronous call, the look-ahead calls and the sequence loop, with host and device images, with and without a mask"""
    got = _drive(vo, stream, "raw", True, stereo, mode, on_device, debug, mask)
    want = _drive(vo, stream, "pre", False, stereo, mode, on_device, debug, mask)
    assert got == want
    assert len(got) == NF and len(got[-1]["ids"]) > (100 if stereo else 50)
    assert any(r["is_keyframe"] for r in got[1:]) and any(r["lba_ran"] for r in got)
    if debug:
        assert len(got[-1]["picture"]) == SW * SH * 3


def test_the_option_matters_on_this_stream(vo, stream):
    """the same driver on the raw low-contrast stream without equalisation tracks differently (the comparison above is not vacuous)"""
    on = _drive(vo, stream, "raw", True, True, "sync", False)
    off = _drive(vo, stream, "raw", False, True, "sync", False)
    assert [r["ids"] for r in on] != [r["ids"] for r in off]


# ---- off is off -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("stereo", [True, False])
def test_off_is_off_and_nothing_is_allocated_per_frame(vo, stream, stereo):
    a_never, a_toggled, a_on = [], [], []
    never = _drive(vo, stream, "raw", False, stereo, "sync", False, allocs=a_never)
    toggled = _drive(vo, stream, "raw", False, stereo, "sync", False, toggle_first=True, allocs=a_toggled)
    assert toggled == never
    # the first set allocates one block per slot and one for the operator; nothing else ever does
    n_eq = (5 if stereo else 3) + 1
    assert [b - a for a, b in zip(a_never, a_toggled)] == [n_eq] * NF
    # with the option on: frame by frame the count of the same loop without it plus the first set's, and constant from the second
    # frame on (MonoVO: from the frame at which the loop without the option has made its own last allocation — its first
    # steady-state frame, the third)
    a_off = []
    _drive(vo, stream, "raw", True, stereo, "ahead", True, allocs=a_on)
    _drive(vo, stream, "raw", False, stereo, "ahead", True, allocs=a_off)
    assert [b - a for a, b in zip(a_off, a_on)] == [n_eq] * NF
    k0 = max(1, min(k for k in range(NF) if len(set(a_off[k:])) == 1))
    assert k0 <= 2 and len(set(a_on[k0:])) == 1


# ---- refusals ---------------------------------------------------------------------------------------------------------------------
def test_refusals(vo):
    from visual_odometry_ros_amd import synthetic as S
    from visual_odometry_ros_amd.api import StereoFramePipeline, make_stereo_params
    st = S.StereoStream(width=320, height=200, K=(300.0, 300.0, 160.0, 100.0), n_u=10, n_v=6, n_new=10, seed=7, margin=5.0)
    poses = st.poses(2)
    L0, _, _ = st.render_pair(poses[0])
    L1, R1, _ = st.render_pair(poses[1])
    ts = st.track_set(0, poses[0], poses[1])
    with vo.Context(device=0, max_width=320, max_height=200, max_points=256, n_slots=3, max_level=3) as c:
        small = np.full((9, 40), 7, np.uint8)
        out = np.zeros_like(small)

        def op(img=small):
            return c.lib.vo_equalize_image(c.handle, img.ctypes.data, img.strides[0], img.shape[1], img.shape[0], out.ctypes.data,
                                           img.shape[1], None, 0)

        assert c.equalize is None
        assert op() == -1  # the operator with the mode off
        with pytest.raises(vo.VoError):
            c.equalizeImage(small)
        n0 = c.allocation_count()
        c.set_equalize("clahe", 3.0, (4, 2))
        state = dict(mode="clahe", clip_limit=3.0, tiles=(4, 2))
        n1 = c.allocation_count()
        assert c.equalize == state and n1 == n0 + 4
        set_eq = lambda mode, clip, tx, ty: c.lib.vo_set_equalize(c.handle, mode, C.c_double(clip), tx, ty)  # noqa: E731
        for bad in ((1, 40.0, 0, 8), (1, 40.0, 8, 0), (1, 40.0, 33, 8), (1, 40.0, 8, 33), (1, -1.0, 8, 8), (1, float("nan"), 8, 8),
                    (1, float("inf"), 8, 8), (2, 40.0, 8, 8), (-1, 40.0, 8, 8), (0, 40.0, 0, 8), (0, float("nan"), 8, 8)):
            assert set_eq(*bad) == -1, bad
            assert c.equalize == state
        with pytest.raises(ValueError):
            c.set_equalize("histogram")
        # the input format, in both directions
        with pytest.raises(vo.VoError) as e:
            c.set_input_format("rgb8")
        assert e.value.code == -1 and c.input_format == "mono8" and c.equalize == state
        c.set_input_format("mono8")  # (no change: accepted)
        c.set_equalize(None)
        c.set_input_format("mono16u")
        with pytest.raises(vo.VoError) as e:
            c.set_equalize("clahe")
        assert e.value.code == -1 and c.equalize is None
        c.set_equalize(None)  # (off stays legal under any format)
        c.set_input_format("mono8")
        # an image not larger than the tile counts: VO_ERR_SIZE, at the operator and at every kind of ingestion; the slot keeps its image
        c.set_equalize("clahe", 40.0, (8, 9))
        c.set_image(0, L0)
        for img in (np.zeros((9, 40), np.uint8), np.zeros((20, 8), np.uint8)):
            assert op(img) == -4
            with pytest.raises(vo.VoError) as e:
                c.set_image(0, img)
            assert e.value.code == -4 and c.slot_image_size(0) == (320, 200)
            assert c.lib.vo_set_image_rectified(c.handle, 0, C.c_void_p(img.ctypes.data), img.shape[1], img.shape[0], img.strides[0], 0) == -4
        assert op(np.zeros((10, 9), np.uint8)) == 0  # one more than the tile counts each way: accepted
        # an unknown residency (0: host, 1: device, 2: device source and host result) is refused before anything is read
        ok = np.zeros((10, 9), np.uint8)
        for bad in (3, -1):
            assert c.lib.vo_equalize_image(c.handle, ok.ctypes.data, 9, 9, 10, out.ctypes.data, 9, None, bad) == -1
        # a frame in flight
        c.set_equalize("clahe", 40.0, (8, 8))
        state = dict(mode="clahe", clip_limit=40.0, tiles=(8, 8))
        pipe = StereoFramePipeline(c, make_stereo_params(320, 200, 21, 3, 80.0, 0.5, 3.0, st.K, st.K, st.T_lr), strict_border=True)
        for k, im in enumerate((L0, L1, R1)):
            c.set_image(k, im)
        pipe.enqueue(ts["pts_l0"], ts["pts_r0"], ts["Xp"], ts["dT_prior"], ts["pts_new"])
        for args in ((0, 40.0, 8, 8), (1, 2.0, 4, 4)):
            assert set_eq(*args) == -1
        assert c.equalize == state
        pipe.result()
        n2 = c.allocation_count()
        c.set_equalize("clahe", 2.0, (4, 4))
        assert c.equalize == dict(mode="clahe", clip_limit=2.0, tiles=(4, 4)) and c.allocation_count() == n2  # (only the first set allocates)
