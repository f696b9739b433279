"""The ignore mask (include/vo_hip.h, "Ignore mask") on the device against the CPU loops with the lookup
composed into their two hooks (tests/mask_ref.py): the candidate table's vote, the stage-4 gate of both drivers, the binding of a
mask to the pair it was ingested with, the rectification validity mask and the contract of the setters. Everything bit for bit."""
import ctypes as C

import numpy as np
import pytest

from mask_ref import MaskedMonoVORef, MaskedStereoVORef, lookup, masked_table
from test_mono_vo_gpu import TruePoseHook
from test_rectify_gpu import DL, DR, KL, KR, _T_lr
from util import DeviceBuffer

pytestmark = pytest.mark.gpu


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ---- 1. the candidate table ---------------------------------------------------------------------------------------------------
def _frame(seed, w, h):
    from visual_odometry_ros_amd import synthetic as S
    stream = S.StereoStream(width=w, height=h, n_u=8, n_v=4, n_new=8, seed=seed)
    return stream.render_pair(stream.poses(1)[0])[0]


def _tables(ctx, fe):
    """the table of slot 0 by the tile kernels and by the per-stage kernels"""
    out = []
    for staged in (0, 1):
        ctx.debug_set(ctx.DBG_STAGED_DETECT, staged)
        try:
            fe.enqueueCandidates(0, staged)
            out.append(fe.getCandidates(staged))
        finally:
            ctx.debug_set(ctx.DBG_STAGED_DETECT, 0)
    return out


@pytest.mark.parametrize("w,h,nu,nv", [(333, 251, 10, 8), (620, 188, 30, 12)])
def test_candidate_table_with_mask(vo, oracle, w, h, nu, nv):
    img = _frame(3, w, h)
    c = vo.Context(device=0, max_width=w, max_height=h, max_points=2048, n_slots=2, max_level=4)
    try:
        fe = vo.FeatureExtractor(c)
        fe.initParams(w, h, nu, nv, THRES_FAST=15)
        c.set_image(0, img)
        plain = _tables(c, fe)
        xy0, has0, nd0 = plain[0]
        assert has0.sum() > 20
        # blocks, a masked bottom band, and single-pixel holes on every second winner of the unmasked table
        mask = np.full((h, w), 255, np.uint8)
        mask[h - 40:] = 0
        mask[50:90, 60:130] = 0
        mask[100:140, w - 120:w - 70] = 0
        win = xy0[has0]
        holes = win[lookup(mask, win)][::2]
        for x, y in holes:
            mask[int(np.float32(y) + np.float32(0.5)), int(np.float32(x) + np.float32(0.5))] = 0
        assert len(holes) >= 5
        tab, has, nd, displaced, pts = masked_table(img, mask, fe.inv_u_step_, fe.inv_v_step_, nu, nv)
        assert nd == nd0 and displaced >= len(holes) + 3           # the mask bites: blocks, band and holes
        assert 0 < has.sum() and not np.array_equal(tab, np.where(has0[:, None], xy0, 0))
        c.set_slot_mask(0, mask)
        for xy, hs, n in _tables(c, fe):                           # tile path, per-stage path
            assert n == nd0                                        # the keypoint count is the unmasked detection's
            assert np.array_equal(hs, has.astype(bool)) and np.array_equal(_bits(xy), _bits(tab))
        # extractORBwithBinning_fast with weights (synchronous and on the side stream): the same composition
        fe.suppressCenterBins()
        fe.weight[::3] = 0
        *_, pts_w = masked_table(img, mask, fe.inv_u_step_, fe.inv_v_step_, nu, nv, weight=fe.weight)
        got = fe.extractORBwithBinning_fast(0)
        assert fe.n_detected == nd0 and np.array_equal(_bits(got), _bits(pts_w)) and len(pts_w) > 0
        fe.enqueueExtract(0)
        assert np.array_equal(_bits(fe.resultExtract()), _bits(pts_w))
        assert fe.detect(0)[0].shape[0] == nd0                     # vo_orb_detect never reads a mask
        # a mask in device memory with padded rows
        wide = np.zeros((h, w + 24), np.uint8)
        wide[:, :w] = mask
        d = DeviceBuffer(wide)
        c.set_slot_mask(0, (d.data_ptr(), w + 24))
        d.free()                                                   # (the library copied)
        for xy, hs, n in _tables(c, fe):
            assert np.array_equal(hs, has.astype(bool)) and np.array_equal(_bits(xy), _bits(tab))
        # all 255 = no mask; all 0 = an empty table and no error; None = no mask again
        c.set_slot_mask(0, np.full((h, w), 255, np.uint8))
        for (xy, hs, n), (xp, hp, npl) in zip(_tables(c, fe), plain):
            assert n == npl and np.array_equal(hs, hp) and np.array_equal(_bits(xy), _bits(xp))
        c.set_slot_mask(0, np.zeros((h, w), np.uint8))
        for xy, hs, n in _tables(c, fe):
            assert n == nd0 and not hs.any() and not xy.any()
        assert fe.extractORBwithBinning_fast(0).shape[0] == 0
        c.set_slot_mask(0, None)
        for (xy, hs, n), (xp, hp, npl) in zip(_tables(c, fe), plain):
            assert n == npl and np.array_equal(hs, hp) and np.array_equal(_bits(xy), _bits(xp))
        with pytest.raises(vo.VoError) as e:                       # a mask has the image's size
            c.set_slot_mask(0, mask[:-1])
        assert e.value.code == -1
    finally:
        c.close()


# ---- 2., 3. the stereo closed loop --------------------------------------------------------------------------------------------
SW, SH, SK = 640, 240, (400.0, 400.0, 320.0, 120.0)


@pytest.fixture(scope="module")
def stereo_frames():
    from visual_odometry_ros_amd import synthetic as S
    st = S.StereoStream(width=SW, height=SH, K=SK, n_u=20, n_v=8, seed=5, speed=0.5)
    return st, [st.render_pair(p)[:2] for p in st.poses(12)]


def _stereo_mask(shift=0):
    m = np.full((SH, SW), 255, np.uint8)
    m[200:] = 0
    m[60:130, 400 - shift:470 - shift] = 0
    return m


def _run_stereo(vo, oracle, frames, masks, strict, prefetch, ctx=None, ctor_mask=False):
    """test_stereo_vo_gpu.py::_run_both with mask k for frame k on both sides (masks[k] None: no mask), set before the pair is
    handed over — under look-ahead before its prefetch, a frame ahead of its own frame. ctx: run on that context (which stays
    open, its id counters reset) instead of a fresh one; ctor_mask: masks[0] goes in through the constructor's mask=."""
    st, imgs = frames
    n = len(masks)
    ref = MaskedStereoVORef(SW, SH, SK, SK, st.T_lr, 20, 8, thres_fast=15, win=21, max_level=4, kf_trans=10.0, kf_overlap=0.6, lba=True,
                            sum_mode=oracle.SUM_TREE, tree_width=512, ic_border=oracle.IC_REFERENCE if strict else oracle.IC_MASKED,
                            n_threads=8)
    c = ctx if ctx is not None else vo.Context(device=0, max_width=SW, max_height=SH, max_points=4096, n_slots=5, max_level=4)
    try:
        if ctx is not None:
            vo.TrackIds(c).reset(0, 0)
        svo = vo.StereoVO(c, SW, SH, SK, SK, st.T_lr, 20, 8, thres_fastscore=15, window_size=21, max_level=4, strict_border=strict,
                          local_ba=True, thres_trans=10.0, thres_alive_ratio=0.6, mask=masks[0] if ctor_mask else None)
        kfs, allocs = [], []
        if prefetch and not ctor_mask:
            svo.setMask(masks[0])
        for k in range(n):
            L, R = imgs[k]
            if prefetch:
                svo.enqueue(L, R)
                if k + 1 < n:
                    svo.setMask(masks[k + 1])  # for the pair handed over next; the frame in flight keeps mask k
                    svo.prefetch(*imgs[k + 1])
                gi = svo.result()
            else:
                if not (ctor_mask and k == 0):
                    svo.setMask(masks[k])
                gi = svo.trackStereoImages(L, R)
            ref.mask = masks[k]
            ri = ref.track(L, R)
            g = svo.getTracks()
            where = f"frame {k}"
            assert gi.frame_id == ri["frame_id"], where
            assert bool(gi.is_keyframe) == ri["keyframe"], where
            assert np.array_equal(g["ids"], ref.ids), where
            assert np.array_equal(_bits(g["pts_l"]), _bits(ref.pts_l)) and np.array_equal(_bits(g["pts_r"]), _bits(ref.pts_r)), where
            assert np.array_equal(g["flags"], ref.flags), where
            tri = (ref.flags & 1) != 0
            assert np.array_equal(_bits(g["Xw"][tri]), _bits(ref.Xw[tri])), where
            assert np.array_equal(_bits(np.array(gi.T_wc).reshape(4, 4)), _bits(ref.T_wp)), where
            if k > 0:
                assert (gi.n_final, gi.n_new, gi.n_kf_tracked) == (ri["n_surv"], ri["n_new"], ri["n_kf_tracked"]), where
                npg = svo.getNewPoints()
                assert np.array_equal(_bits(npg["pts_l"]), _bits(ri["cand"])) and np.array_equal(npg["accept"], ri["accept"]), where
                assert np.array_equal(npg["mask_new"], ri["mask_new"]), where
            if gi.is_keyframe:
                kfs.append(k)
            allocs.append(c.allocation_count())
        svo.close()
        return ref, kfs, allocs
    finally:
        if ctx is None:
            c.close()


@pytest.mark.parametrize("strict,prefetch", [(4, False), (1, True)])
def test_stereo_closed_loop_with_mask(vo, oracle, stereo_frames, strict, prefetch):
    """test_closed_loop_small's stream with the local BA, rows >= 200 and a box masked. On the CPU loop the gate demotes 50
    features and 56 winners of unmasked buckets lie on masked pixels; the second keyframe falls on frame 8 (9 without the mask),
    so a device that ignored the mask could not pass."""
    ref, kfs, _ = _run_stereo(vo, oracle, stereo_frames, [_stereo_mask()] * 12, strict, prefetch)
    assert ref.n_demoted >= 10 and ref.n_displaced >= 10
    if strict == 4:  # (the measured run: the strict-border replay as the reference has it)
        assert kfs[:2] == [1, 8], kfs


def test_stereo_per_frame_masks_under_lookahead(vo, oracle, stereo_frames):
    """The box moves 8 px per frame; setMask before each pair's prefetch. A prefetched pair keeps the mask it was ingested with:
    the device equals the CPU loop that uses mask k for frame k."""
    ref, _, allocs = _run_stereo(vo, oracle, stereo_frames, [_stereo_mask(8 * k) for k in range(12)], 4, True)
    assert ref.n_demoted >= 10 and ref.n_displaced >= 10


# ---- 4. the mono closed loop --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("strict,prefetch", [(1, False), (4, True)])
def test_mono_closed_loop_with_mask(vo, oracle, strict, prefetch):
    """On the CPU loop the gate demotes 193 features, and frame 3 takes the 5-point fallback, where the mask acts on the
    detection only."""
    from visual_odometry_ros_amd import synthetic as S
    W, H, K, nu, nv, n = 376, 240, (229.3, 228.6, 183.6, 124.2), 20, 12, 12
    st = S.StereoStream(width=W, height=H, K=K, n_u=nu, n_v=nv, seed=5, speed=0.25)
    poses = st.poses(n)
    imgs = [st.render_pair(p)[0] for p in poses]
    mask = np.full((H, W), 255, np.uint8)
    mask[204:] = 0
    mask[60:120, 233:274] = 0
    hook_g, hook_r = TruePoseHook(poses), TruePoseHook(poses)
    ref = MaskedMonoVORef(W, H, K, nu, nv, hook_r, thres_fast=15, win=15, max_level=5, thres_err=20.0, thres_bidir=1.0, thres_poseba=5,
                          thres_sampson=1.0, thres_parallax_deg=1.0, kf_trans=1.0, lba=True, sum_mode=oracle.SUM_TREE, tree_width=512,
                          ic_border=oracle.IC_REFERENCE, n_threads=8)
    ref.mask = mask
    c = vo.Context(device=0, max_width=W, max_height=H, max_points=2 * nu * nv + 512, n_slots=3, max_level=5)
    try:
        mvo = vo.MonoVO(c, W, H, K, nu, nv, hook_g, thres_fastscore=15, window_size=15, max_level=5, thres_error=20.0,
                        thres_bidirection=1.0, thres_poseba_error=5, thres_sampson=1.0, thres_parallax=1.0, thres_translation=1.0,
                        strict_border=strict, local_ba=True, mask=mask)
        fallbacks = 0
        for k in range(n):
            hook_g.k = hook_r.k = k
            if prefetch:
                mvo.enqueue(imgs[k])
                if k + 1 < n:
                    mvo.prefetch(imgs[k + 1])
                gi = mvo.result()
            else:
                gi = mvo.trackImage(imgs[k])
            ri = ref.track(imgs[k])
            g = mvo.getTracks()
            where = f"frame {k}"
            assert bool(gi.is_keyframe) == ri["keyframe"], where
            assert np.array_equal(g["ids"], ref.ids), where
            assert np.array_equal(_bits(g["pts"]), _bits(ref.pts)), where
            assert np.array_equal(g["flags"], ref.flags()), where
            tri = (g["flags"] & 1) != 0
            assert np.array_equal(_bits(g["Xw"][tri]), _bits(ref.Xw()[tri])), where
            assert np.array_equal(_bits(np.array(gi.T_wc).reshape(4, 4)), _bits(ref.frames[k]["T_wc"])), where
            if k > 0:
                assert (gi.n_final, gi.n_new) == (ri["n_final"], ri["n_new"]), where
            assert bool(gi.used_five_point) == ri["five_point"], where
            fallbacks += int(k > 1 and ri["five_point"])
        assert hook_g.calls == hook_r.calls
        assert ref.n_demoted >= 10 and fallbacks >= 1
        mvo.close()
    finally:
        c.close()


# ---- 5. the validity mask -----------------------------------------------------------------------------------------------------
def _validity_numpy(mu, mv, erode):
    from scipy import ndimage
    h, w = mu.shape
    with np.errstate(invalid="ignore"):
        valid = ((mu >= 0) & (mu <= np.float32(w - 1)) & (mv >= 0) & (mv <= np.float32(h - 1))).astype(np.uint8)
    return ndimage.minimum_filter(valid, size=2 * erode + 1, mode="constant", cval=1) * np.uint8(255)


def test_rectify_validity_mask(vo, oracle):
    """tests/test_rectify_gpu.py's rig, and the same rig with the radial terms' signs turned (pincushion). With the former's
    barrel distortion every rectified pixel samples inside the source — measured on the CPU maps: the mask is all 255 for both
    cameras — so the "neither all 0 nor all 255" property and the four frames are checked on the pincushion rig, whose rectified
    corners lie outside the source (80 % valid at erode 0, 62 % at 31)."""
    from visual_odometry_ros_amd import synthetic as S
    W, H = 752, 480
    pin = lambda D: (-D[0], -D[1], D[2], D[3], D[4])
    c = vo.Context(device=0, max_width=W, max_height=H, max_points=2048, n_slots=5, max_level=4)
    try:
        cam = vo.StereoCamera(c)
        with pytest.raises(vo.VoError):
            cam.validityMask(0)
        for dl, dr, mixed in ((DL, DR, False), (pin(DL), pin(DR), True)):
            cam.initParams(W, H, KL, dl, KR, dr)
            cam.setStereoPoseLeft2Right(_T_lr())
            cam.initStereoCameraToRectify()
            maps = cam.maps()
            for cam_id in (0, 1):
                mu, mv = maps[cam_id]
                for erode in (0, 3, 31):
                    got = cam.validityMask(erode, cam=cam_id)
                    assert np.array_equal(got, _validity_numpy(mu, mv, erode)), (mixed, cam_id, erode)
                    if mixed:
                        assert got.min() == 0 and got.max() == 255
        mu, mv = maps[0]
        nan = mu.copy()
        nan[100:103, 200:205] = np.nan  # NaN is invalid
        c.check(c.lib.vo_rectify_set_maps(c.handle, 0, C.c_void_p(nan.ctypes.data), C.c_void_p(mv.ctypes.data), W, H))
        got = cam.validityMask(1)
        assert np.array_equal(got, _validity_numpy(nan, mv, 1)) and not got[99:104, 199:206].any()
        c.check(c.lib.vo_rectify_set_maps(c.handle, 0, C.c_void_p(mu.ctypes.data), C.c_void_p(mv.ctypes.data), W, H))
        out = np.zeros((H, W), np.uint8)
        for bad in (-1, 32):
            assert c.lib.vo_rectify_validity_mask(c.handle, 0, bad, out.ctypes.data, W, 0) == -1
        # four frames through the maps with the left camera's mask: nothing is tracked where cv::remap filled in
        mask = cam.validityMask(3)
        st = S.StereoStream(width=W, height=H, K=KL, baseline=0.11, n_u=20, n_v=12, seed=5, speed=0.25)
        st.T_lr = _T_lr()
        imgs = [st.render_pair(p)[:2] for p in st.poses(4)]
        m = oracle.stereo_rectify_maps(W, H, KL, pin(DL), KR, pin(DR), _T_lr())
        ref = MaskedStereoVORef(W, H, m["K_rect"], m["K_rect"], m["T_lr_rect"], 20, 12, thres_fast=15, win=21, max_level=4, kf_trans=1.2,
                                lba=True, sum_mode=oracle.SUM_TREE, tree_width=512, ic_border=oracle.IC_REFERENCE, n_threads=8,
                                rectify_maps=(m["left"], m["right"]))
        ref.mask = mask
        svo = vo.StereoVO(c, W, H, cam.K_rect, cam.K_rect, cam.T_lr_rect, 20, 12, thres_fastscore=15, window_size=21, max_level=4,
                          strict_border=4, local_ba=True, thres_trans=1.2, rectify=True, mask=mask)
        for k, (L, R) in enumerate(imgs):
            svo.trackStereoImages(L, R)
            ref.track(L, R)
            g = svo.getTracks()
            assert len(g["ids"]) > 100 and lookup(mask, g["pts_l"]).all(), k
            assert np.array_equal(g["ids"], ref.ids) and np.array_equal(_bits(g["pts_l"]), _bits(ref.pts_l)), k
        assert ref.n_displaced >= 10  # (without the mask 12 to 17 of each frame's tracks sit on the fill's edge)
        svo.close()
    finally:
        c.close()


# ---- 6. the contract ----------------------------------------------------------------------------------------------------------
def test_set_mask_none_after_masked_frames(vo, oracle, stereo_frames):
    """Six frames under the mask, then setMask(None) with the planes allocated and switched on: the later frames equal the CPU
    loop that drops the mask at the same frame (under look-ahead: the pair prefetched during frame 5 is the first without)."""
    ref, _, _ = _run_stereo(vo, oracle, stereo_frames, [_stereo_mask()] * 6 + [None] * 4, 4, True)
    assert ref.n_demoted >= 10
    ref, _, _ = _run_stereo(vo, oracle, stereo_frames, [_stereo_mask()] * 3 + [None] * 3, 1, False)
    assert ref.n_demoted >= 1


def test_two_drivers_on_one_context_with_different_masks(vo, oracle, stereo_frames):
    """Drivers follow each other on one context and use the same image slots: the second one's mask is its own — not the copy
    the first one left in the slots — whether it comes through setMask or the constructor, and a third driver without a mask
    sees none. Each equals its CPU loop bit for bit."""
    m1, m2 = _stereo_mask(), _stereo_mask(120)
    m2[:, :90] = 0
    c = vo.Context(device=0, max_width=SW, max_height=SH, max_points=4096, n_slots=5, max_level=4)
    try:
        a, _, _ = _run_stereo(vo, oracle, stereo_frames, [m1] * 5, 4, True, ctx=c)
        b, _, _ = _run_stereo(vo, oracle, stereo_frames, [m2] * 5, 4, True, ctx=c)
        assert not np.array_equal(a.ids, b.ids) or not np.array_equal(a.pts_l, b.pts_l)  # (the two masks give different loops)
        _run_stereo(vo, oracle, stereo_frames, [m1] * 4, 4, False, ctx=c, ctor_mask=True)
        _run_stereo(vo, oracle, stereo_frames, [m2] * 4, 4, False, ctx=c, ctor_mask=True)
        plain, _, _ = _run_stereo(vo, oracle, stereo_frames, [None] * 4, 4, False, ctx=c)
        assert plain.n_demoted == 0
        # an operator call on a slot a destroyed driver used sees no mask
        fe = vo.FeatureExtractor(c)
        fe.initParams(SW, SH, 20, 8, THRES_FAST=15)
        L = stereo_frames[1][0][0]
        c.set_image(0, L)
        fe.enqueueCandidates(0, 0)
        xy, has, _ = fe.getCandidates(0)
        tab, hs, *_ = masked_table(L, None, fe.inv_u_step_, fe.inv_v_step_, 20, 8)
        assert np.array_equal(has, hs.astype(bool)) and np.array_equal(_bits(xy), _bits(tab))
        # a slot's mask is dropped when an image of another size goes into the slot
        c.set_slot_mask(0, np.zeros((SH, SW), np.uint8))
        small = np.ascontiguousarray(L[:200, :600])
        c.set_image(0, small)
        fe2 = vo.FeatureExtractor(c)
        fe2.initParams(600, 200, 20, 8, THRES_FAST=15)
        fe2.enqueueCandidates(0, 1)
        assert fe2.getCandidates(1)[1].sum() > 20
        with pytest.raises(vo.VoError) as e:
            c.set_slot_mask(0, np.zeros((SH, SW), np.uint8))  # (the image is 600 x 200 now)
        assert e.value.code == -1
        assert c.slot_image_size(0) == (600, 200)
        d = DeviceBuffer(np.zeros((200, 600), np.uint8))
        with pytest.raises(vo.VoError) as e:
            c.set_slot_mask(0, (d.data_ptr(), 599))  # the device form: a stride below the image's width
        assert e.value.code == -1
        c.set_slot_mask(0, (d.data_ptr(), 600))
        d.free()
        fe2.enqueueCandidates(0, 1)
        assert not fe2.getCandidates(1)[1].any()
    finally:
        c.close()


def _alloc_counts(vo, stereo_frames, masked, n=6):
    """allocation counts of a look-ahead loop on a fresh context, relative to the count right behind the driver's
    construction: (what the first setMask allocated, [after frame 0, after frame 1, ...])"""
    st, imgs = stereo_frames
    c = vo.Context(device=0, max_width=SW, max_height=SH, max_points=4096, n_slots=5, max_level=4)
    try:
        svo = vo.StereoVO(c, SW, SH, SK, SK, st.T_lr, 20, 8, thres_fastscore=15, window_size=21, max_level=4, strict_border=4,
                          local_ba=True, thres_trans=10.0, thres_alive_ratio=0.6)
        start = c.allocation_count()
        first = 0
        if masked:
            svo.setMask(_stereo_mask())
            first = c.allocation_count() - start
        counts = []
        for k in range(n):
            svo.enqueue(*imgs[k])
            if k + 1 < n:
                if masked:
                    svo.setMask(_stereo_mask(8 * (k + 1)))  # a new mask for every pair
                svo.prefetch(*imgs[k + 1])
            svo.result()
            counts.append(c.allocation_count() - start)
        if masked:
            for k in range(4):
                svo.setMask(_stereo_mask(3 * k))
                svo.setMask(None)
            counts.append(c.allocation_count() - start)
        svo.close()
        return first, counts
    finally:
        c.close()


def test_mask_contract(vo, oracle, stereo_frames):
    st, imgs = stereo_frames
    # every allocation of the option happens at the FIRST setMask — the master and the three left slots' planes — and the count
    # does not move because of the mask afterwards: frame by frame, the first two included, a loop with a new mask every frame
    # allocates exactly what the unmasked loop allocates (the driver's and the context's own first-use allocations)
    _, plain = _alloc_counts(vo, stereo_frames, False)
    first, masked = _alloc_counts(vo, stereo_frames, True)
    assert first == 4, first
    assert masked[:6] == [v + first for v in plain], (plain, masked)
    assert masked[6] == masked[5]  # set / clear again and again with nothing in flight
    c = vo.Context(device=0, max_width=SW, max_height=SH, max_points=4096, n_slots=5, max_level=4)
    try:
        assert c.slot_image_size(2) == (0, 0)
        with pytest.raises(vo.VoError) as e:
            c.set_slot_mask(2, np.zeros((SH, SW), np.uint8))  # the slot holds no image yet
        assert e.value.code == -1

        def make():
            return vo.StereoVO(c, SW, SH, SK, SK, st.T_lr, 20, 8, thres_fastscore=15, window_size=21, max_level=4, strict_border=4,
                               local_ba=True, thres_trans=10.0, thres_alive_ratio=0.6)
        # the unmasked bits of six frames
        svo = make()
        plain = []
        for L, R in imgs[:6]:
            svo.trackStereoImages(L, R)
            plain.append(svo.getTracks())
        svo.close()
        vo.TrackIds(c).reset(0, 0)
        svo = make()
        for bad in (np.zeros((SH, SW - 1), np.uint8), np.zeros((SH + 1, SW), np.uint8), np.zeros((SH, SW), np.float32)):
            with pytest.raises(vo.VoError) as e:
                svo.setMask(bad)
            assert e.value.code == -1
        m = _stereo_mask()
        assert c.lib.vo_svo_set_mask(svo._h, m.ctypes.data, SW - 1, 0) == -1  # VO_ERR_INVALID: a stride below the width
        # a mask and setMask(None) before anything is ingested: the unmasked bits
        svo.setMask(m)
        svo.setMask(None)
        for k, (L, R) in enumerate(imgs[:6]):
            svo.trackStereoImages(L, R)
            g = svo.getTracks()
            assert np.array_equal(g["ids"], plain[k]["ids"]) and np.array_equal(_bits(g["pts_l"]), _bits(plain[k]["pts_l"])), k
        svo.close()
    finally:
        c.close()
