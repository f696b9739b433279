"""calcZNCC on the device and the ZNCC gate of both drivers (include/vo_hip.h, "ZNCC") against the numpy
restatement and the CPU loops with the gate composed into their frame() hook (tests/zncc_restatement.py). Everything bit for bit,
NaN as NaN."""
import numpy as np
import pytest

from test_mask_gpu import SH, SK, SW, _stereo_mask
from test_mono_vo_gpu import TruePoseHook
from zncc_restatement import GatedMonoVORef, GatedStereoVORef, with_mask, zncc

pytestmark = pytest.mark.gpu


def _bits(a):
    a = np.ascontiguousarray(a, np.float32)
    return np.where(np.isnan(a), np.uint32(0x7FC00000), a.view(np.uint32))  # (NaN as NaN)


# ---- 1. the operator ------------------------------------------------------------------------------------------------------------
MAX_POINTS = 300


def _image(w, h, seed):
    from visual_odometry_ros_amd import synthetic as S
    st = S.StereoStream(width=max(w, 160), height=max(h, 120), n_u=8, n_v=4, n_new=8, seed=seed)
    L, R = st.render_pair(st.poses(1)[0])[:2]
    return np.ascontiguousarray(L[:h, :w]), np.ascontiguousarray(R[:h, :w])


def _points(w, h, win, n, seed):
    """n pairs: the named cases first (as many as n allows), uniformly drawn ones over the image and a margin behind them"""
    f = np.float32
    named = np.array([[w * 0.4 + 0.25, h * 0.5 + 0.75], [w // 2, h // 2],                       # interior: fractional, integer
                      [win - 0.5, h * 0.5], [w - win + 0.5, h * 0.4], [w * 0.5, win - 1.25], [w * 0.45, h - win + 0.5],  # four borders
                      [-0.5, h * 0.5], [w * 0.5, -0.75],                                        # u, v in (-1, 0)
                      [w - 1.0, h * 0.5], [w + 40.0, h * 0.5], [w * 0.5, h - 1.0],              # u >= W - 1, v >= H - 1
                      [np.nan, h * 0.5], [w * 0.5, np.nan], [1e12, 3.0], [-1.0, 5.0]], f)       # NaN, beyond int, exactly -1
    rng = np.random.default_rng(seed)
    rnd = np.stack([rng.uniform(-win, w + win, n), rng.uniform(-win, h + win, n)], 1).astype(f)
    p0 = np.concatenate([named, rnd])[:n]
    p1 = (p0 + rng.uniform(-1.5, 1.5, p0.shape).astype(f)).astype(f)
    if n > 1:
        p1[1] = p0[1]
    return p0, p1


@pytest.fixture(scope="module")
def operator_setup(vo):
    out = {}
    for w, h in ((97, 61), (640, 240)):
        c = vo.Context(device=0, max_width=w, max_height=h, max_points=MAX_POINTS, n_slots=3, max_level=2)
        L, R = _image(w, h, 3)
        c.set_image(0, L)
        c.set_image(1, R)
        c.set_image(2, np.full((h, w), 77, np.uint8))
        out[(w, h)] = (c, L, R)
    yield out
    for c, _, _ in out.values():
        c.close()


@pytest.mark.parametrize("order", ["tree", "reference"])
@pytest.mark.parametrize("pattern", ["reference", "centered"])
@pytest.mark.parametrize("win", [3, 15, 21, 31])
@pytest.mark.parametrize("size", [(97, 61), (640, 240)])
def test_operator_equals_restatement(vo, operator_setup, size, win, pattern, order):
    """n in {0, 1, 65, max_points}; the points of _points; a constant image (NaN out); the same slot twice. Fails on a library
    without vo_zncc: the symbol does not exist."""
    c, L, R = operator_setup[size]
    w, h = size
    c.sum_order = order
    try:
        for n in (0, 1, 65, MAX_POINTS):
            p0, p1 = _points(w, h, win, n, 7 + n)
            got = c.calcZNCC(0, 1, p0, p1, win=win, pattern=pattern)
            want = zncc(L, R, p0, p1, win, pattern, order)
            assert got.shape == (n,) and np.array_equal(_bits(got), _bits(want)), (n, got[:16], want[:16])
            if n >= 65:
                assert np.isfinite(want).sum() >= 30 and np.isnan(want[11:13]).all()
        p0, p1 = _points(w, h, win, 65, 1)
        flat = np.full((h, w), 77, np.uint8)
        got = c.calcZNCC(2, 1, p0, p1, win=win, pattern=pattern)          # a constant image
        assert np.array_equal(_bits(got), _bits(zncc(flat, R, p0, p1, win, pattern, order)))
        if pattern == "centered":
            assert np.isnan(got[:2]).all()                                 # (the interior patches are flat: 0 / 0)
        got = c.calcZNCC(0, 0, p0, p1, win=win, pattern=pattern)          # the same slot twice
        assert np.array_equal(_bits(got), _bits(zncc(L, L, p0, p1, win, pattern, order)))
        got = c.calcZNCC(0, 0, p0, p0, win=win, pattern=pattern)
        assert np.array_equal(_bits(got), _bits(zncc(L, L, p0, p0, win, pattern, order)))
    finally:
        c.sum_order = "tree"


def test_operator_argument_errors(vo, operator_setup):
    c, L, R = operator_setup[(97, 61)]
    p = np.array([[40.0, 30.0]], np.float32)
    for win in (2, 1, 16, 33, -3):
        with pytest.raises(vo.VoError) as e:
            c.calcZNCC(0, 1, p, p, win=win)
        assert e.value.code == -1
    assert c.lib.vo_zncc(c.handle, 0, 1, p.ctypes.data, p.ctypes.data, 1, 15, 2, p.ctypes.data) == -1   # pattern
    assert c.lib.vo_zncc(c.handle, 0, 9, p.ctypes.data, p.ctypes.data, 1, 15, 0, p.ctypes.data) == -1   # slot
    assert c.lib.vo_zncc(c.handle, 0, 1, None, p.ctypes.data, 1, 15, 0, p.ctypes.data) == -1
    big = np.zeros((MAX_POINTS + 1, 2), np.float32)
    with pytest.raises(vo.VoError):
        c.calcZNCC(0, 1, big, big)


# ---- 2. the stereo closed loop ---------------------------------------------------------------------------------------------------
GATE_T = dict(thres=0.8, win=15, pattern="centered", pairs=("temporal",))
GATE_TS = dict(thres=0.9, win=15, pattern="centered", pairs=("temporal", "stereo"))


@pytest.fixture(scope="module")
def stereo_frames():
    from visual_odometry_ros_amd import synthetic as S
    st = S.StereoStream(width=SW, height=SH, K=SK, n_u=20, n_v=8, seed=5, speed=0.5)
    return st, [st.render_pair(p)[:2] for p in st.poses(12)]


def _stereo_ref(oracle, st, strict, masked=False):
    cls = with_mask(GatedStereoVORef) if masked else GatedStereoVORef
    return cls(SW, SH, SK, SK, st.T_lr, 20, 8, thres_fast=15, win=21, max_level=4, kf_trans=10.0, kf_overlap=0.6, lba=True,
               sum_mode=oracle.SUM_TREE, tree_width=512, ic_border=oracle.IC_REFERENCE if strict else oracle.IC_MASKED, n_threads=8)


@pytest.fixture(scope="module")
def ungated_counts(oracle, stereo_frames):
    """track counts of the CPU loop without a gate, frame by frame (computed once)"""
    st, imgs = stereo_frames
    ref = _stereo_ref(oracle, st, 4)
    out = []
    for L, R in imgs:
        ref.track(L, R)
        out.append(len(ref.ids))
    return out


def _run_stereo(vo, oracle, frames, gates, strict, prefetch, masks=None, check_zncc=True):
    """test_mask_gpu.py::_run_stereo's protocol with gate k for frame k on both sides (None: off), set before the frame is
    enqueued (the setter is refused while a frame is in flight). masks: also mask k for frame k, as there."""
    st, imgs = frames
    n = len(gates)
    ref = _stereo_ref(oracle, st, strict, masked=masks is not None)
    c = vo.Context(device=0, max_width=SW, max_height=SH, max_points=4096, n_slots=5, max_level=4)
    try:
        svo = vo.StereoVO(c, SW, SH, SK, SK, st.T_lr, 20, 8, thres_fastscore=15, window_size=21, max_level=4, strict_border=strict,
                          local_ba=True, thres_trans=10.0, thres_alive_ratio=0.6, zncc_gate=gates[0])
        kfs, counts, allocs = [], [], []
        if masks is not None and prefetch:
            svo.setMask(masks[0])
        for k in range(n):
            L, R = imgs[k]
            if k > 0:
                svo.setZnccGate(gates[k])
            if prefetch:
                svo.enqueue(L, R)
                if k + 1 < n:
                    if masks is not None:
                        svo.setMask(masks[k + 1])
                    svo.prefetch(*imgs[k + 1])
                gi = svo.result()
            else:
                if masks is not None:
                    svo.setMask(masks[k])
                gi = svo.trackStereoImages(L, R)
            ref.gate = gates[k]
            if masks is not None:
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
                if gates[k] is not None and check_zncc:
                    # vo_svo_get_zncc: the restatement's bits for every feature the CPU loop has at stage >= 3
                    z = svo.getZncc()
                    live = ri["frame"]["stage"] >= 3
                    assert live.sum() > 50, where
                    for name in ("temporal", "stereo"):
                        if name in gates[k]["pairs"]:
                            assert z[name].shape == live.shape, where
                            assert np.array_equal(_bits(z[name][live]), _bits(ref.last[name][live])), (where, name)
                        else:
                            assert z[name] is None
            if gi.is_keyframe:
                kfs.append(k)
            counts.append(len(ref.ids))
            allocs.append(c.allocation_count())
        svo.close()
        return ref, kfs, counts, allocs
    finally:
        c.close()


@pytest.mark.parametrize("gate", [GATE_T, GATE_TS], ids=["temporal-0.8", "temporal+stereo-0.9"])
@pytest.mark.parametrize("strict,prefetch", [(4, False), (1, True)])
def test_stereo_closed_loop_with_gate(vo, oracle, stereo_frames, ungated_counts, strict, prefetch, gate):
    """test_mask_gpu.py's 640 x 240 stream with the local BA, centred 15 x 15 patches. Counted on the CPU loop with the exact
    float32 restatement (tree sums), 11 steady frames:
      thres 0.8, temporal            72 features demoted, keyframes on [1, 8] (ungated: [1, 9]), track counts 0.957 .. 1.026 of
                                     the ungated loop's
      thres 0.9, temporal + stereo   289 demoted, keyframes on [1, 5, 9], track counts 0.873 .. 0.913 of the ungated loop's
    (ungated track counts: 112, 133, 150, 161, 161, 169, 178, 189, 186, 192, 195, 197). No value of a feature at stage >= 3 is
    NaN on this stream."""
    ref, kfs, counts, _ = _run_stereo(vo, oracle, stereo_frames, [gate] * 12, strict, prefetch)
    assert ref.n_demoted >= 50                                                 # the gate bites ...
    assert all(a >= 0.8 * b for a, b in zip(counts, ungated_counts)), counts   # ... and does not kill everything
    assert kfs == ([1, 5, 9] if gate is GATE_TS else [1, 8]), kfs


# ---- 3. the mono closed loop -----------------------------------------------------------------------------------------------------
MW, MH, MK, MNU, MNV, MN = 376, 240, (229.3, 228.6, 183.6, 124.2), 20, 12, 12
MONO_THRES = 0.8


def _mono_mask():
    mask = np.full((MH, MW), 255, np.uint8)
    mask[204:] = 0
    mask[60:120, 233:274] = 0
    return mask


@pytest.fixture(scope="module")
def mono_stream():
    from visual_odometry_ros_amd import synthetic as S
    st = S.StereoStream(width=MW, height=MH, K=MK, n_u=MNU, n_v=MNV, seed=5, speed=0.25)
    poses = st.poses(MN)
    return poses, [st.render_pair(p)[0] for p in poses]


def _mono_ref(oracle, hook):
    return with_mask(GatedMonoVORef)(MW, MH, MK, MNU, MNV, hook, thres_fast=15, win=15, max_level=5, thres_err=20.0, thres_bidir=1.0,
                                     thres_poseba=5, thres_sampson=1.0, thres_parallax_deg=1.0, kf_trans=1.0, lba=True,
                                     sum_mode=oracle.SUM_TREE, tree_width=512, ic_border=oracle.IC_REFERENCE, n_threads=8)


@pytest.fixture(scope="module")
def mono_ungated_counts(oracle, mono_stream):
    poses, imgs = mono_stream
    hook = TruePoseHook(poses)
    ref = _mono_ref(oracle, hook)
    ref.mask = _mono_mask()
    out = []
    for k in range(MN):
        hook.k = k
        ref.track(imgs[k])
        out.append(len(ref.ids))
    return out


@pytest.mark.parametrize("strict,prefetch", [(1, False), (4, True)])
def test_mono_closed_loop_with_gate(vo, oracle, mono_stream, mono_ungated_counts, strict, prefetch):
    """test_mask_gpu.py's 376 x 240 stream and protocol — its mask included, under which frame 3 takes the 5-point fallback —
    with the gate on top: centred 15 x 15, temporal. Counted on the CPU loop with the exact restatement, out of {0.8, 0.9, 0.95}:
      0.8    52 demoted by the gate, track counts 0.951 .. 1.004 of the loop without the gate, fallback on frame 3   <- used
      0.9    188 demoted, 0.923 .. 0.988, fallback on frame 3
      0.95   546 demoted, 0.881 .. 0.943, and the fallback no longer happens
    The fallback frame is host-driven: not gated."""
    poses, imgs = mono_stream
    mask = _mono_mask()
    gate = dict(thres=MONO_THRES, win=15, pattern="centered")
    hook_g, hook_r = TruePoseHook(poses), TruePoseHook(poses)
    ref = _mono_ref(oracle, hook_r)
    ref.mask, ref.gate = mask, gate
    c = vo.Context(device=0, max_width=MW, max_height=MH, max_points=2 * MNU * MNV + 512, n_slots=3, max_level=5)
    try:
        mvo = vo.MonoVO(c, MW, MH, MK, MNU, MNV, hook_g, thres_fastscore=15, window_size=15, max_level=5, thres_error=20.0,
                        thres_bidirection=1.0, thres_poseba_error=5, thres_sampson=1.0, thres_parallax=1.0, thres_translation=1.0,
                        strict_border=strict, local_ba=True, mask=mask, zncc_gate=gate)
        with pytest.raises(vo.VoError):
            mvo.setZnccGate(dict(thres=0.5, pairs=("temporal",), win=14))
        with pytest.raises(ValueError):
            mvo.setZnccGate(dict(thres=0.5, pairs=("stereo",)))
        assert c.lib.vo_mvo_set_zncc_gate(mvo._h, 2, 15, 1, 0.5) == -1  # VO_ZNCC_STEREO on a MonoVO
        fallbacks, counts = 0, []
        for k in range(MN):
            hook_g.k = hook_r.k = k
            if prefetch:
                mvo.enqueue(imgs[k])
                if k + 1 < MN:
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
            if k > 1 and not ri["five_point"]:
                live = ri["frame"]["stage"] >= 3
                z = mvo.getZncc()
                assert z.shape == live.shape and live.sum() > 50, where
                assert np.array_equal(_bits(z[live]), _bits(ref.last["temporal"][live])), where
            counts.append(len(ref.ids))
        assert hook_g.calls == hook_r.calls
        assert ref.n_zncc_demoted >= 10 and fallbacks >= 1
        assert all(a >= 0.8 * b for a, b in zip(counts, mono_ungated_counts)), counts
        mvo.close()
    finally:
        c.close()


# ---- 4. the contract ----------------------------------------------------------------------------------------------------------
def test_gate_off_after_gated_frames(vo, oracle, stereo_frames):
    """Six gated frames, then setZnccGate(None): from that frame on the device equals the CPU loop that drops the gate at the
    same frame — the ungated loop's arithmetic on the track set the gate left behind."""
    ref, _, _, _ = _run_stereo(vo, oracle, stereo_frames, [GATE_TS] * 6 + [None] * 4, 4, True)
    assert ref.n_demoted >= 50
    ref, _, _, _ = _run_stereo(vo, oracle, stereo_frames, [GATE_TS] * 3 + [None] * 3, 1, False)
    assert ref.n_demoted >= 10


def test_threshold_below_every_value_is_no_gate(vo, oracle, stereo_frames):
    """thres = -2: every finite value passes, and on this stream no feature at stage >= 3 has a NaN (the CPU loop demotes 0), so
    the bits are those of no gate — while the kernel runs and vo_svo_get_zncc delivers."""
    all_pass = dict(thres=-2.0, win=15, pattern="centered", pairs=("temporal", "stereo"))
    gated, kfs_g, counts_g, _ = _run_stereo(vo, oracle, stereo_frames, [all_pass] * 8, 4, True)
    plain, kfs_p, counts_p, _ = _run_stereo(vo, oracle, stereo_frames, [None] * 8, 4, True)
    assert gated.n_demoted == 0 and kfs_g == kfs_p and counts_g == counts_p
    assert np.array_equal(gated.ids, plain.ids) and np.array_equal(_bits(gated.pts_l), _bits(plain.pts_l))


@pytest.mark.parametrize("strict,prefetch", [(4, True), (1, False)])
def test_mask_and_gate_together(vo, oracle, stereo_frames, strict, prefetch):
    """the two gates combine by AND: the device equals the CPU loop with both"""
    ref, _, _, _ = _run_stereo(vo, oracle, stereo_frames, [GATE_T] * 8, strict, prefetch, masks=[_stereo_mask()] * 8)
    assert ref.n_zncc_demoted >= 10 and ref.n_demoted - ref.n_zncc_demoted >= 10 and ref.n_displaced >= 10


def test_gate_contract(vo, oracle, stereo_frames):
    st, imgs = stereo_frames

    def run(gated):
        """a look-ahead loop on a fresh context: (what the first setZnccGate allocated, allocation counts after frame 0, 1, ...
        relative to the count right behind the driver's construction)"""
        c = vo.Context(device=0, max_width=SW, max_height=SH, max_points=4096, n_slots=5, max_level=4)
        try:
            svo = vo.StereoVO(c, SW, SH, SK, SK, st.T_lr, 20, 8, thres_fastscore=15, window_size=21, max_level=4, strict_border=4,
                              local_ba=True, thres_trans=10.0, thres_alive_ratio=0.6)
            start = c.allocation_count()
            first = 0
            if gated:
                svo.setZnccGate(GATE_TS)
                first = c.allocation_count() - start
            counts = []
            for k in range(6):
                if gated:  # a new window for every frame, off in between; thres = -2 lets everything pass, so that the track
                    svo.setZnccGate(None)  # sets — and with them the keyframes' own allocations — are the ungated loop's
                    svo.setZnccGate(dict(GATE_TS, thres=-2.0, win=(15, 21, 31)[k % 3]))
                svo.enqueue(*imgs[k])
                if k + 1 < 6:
                    svo.prefetch(*imgs[k + 1])
                svo.result()
                counts.append(c.allocation_count() - start)
            if gated:
                # refused while a frame is in flight, and for bad arguments; a refused call changes nothing
                svo.enqueue(*imgs[6])
                assert c.lib.vo_svo_set_zncc_gate(svo._h, 1, 15, 1, 0.5) == -1
                assert c.lib.vo_svo_set_zncc_gate(svo._h, 0, 15, 1, 0.5) == -1
                n = np.zeros(1, np.int32)
                assert c.lib.vo_svo_get_zncc(svo._h, None, None, 0, n.ctypes.data) == -1
                svo.result()
                for pairs, win, pattern, thres in ((4, 15, 1, 0.5), (1, 16, 1, 0.5), (1, 1, 1, 0.5), (1, 33, 1, 0.5), (1, 15, 2, 0.5),
                                                   (3, 15, -1, 0.5), (1, 15, 1, float("nan"))):
                    assert c.lib.vo_svo_set_zncc_gate(svo._h, pairs, win, pattern, thres) == -1, (pairs, win, pattern, thres)
                z = svo.getZncc()
                assert z["temporal"] is not None and z["stereo"] is not None and len(z["temporal"]) > 100
                svo.setZnccGate(None)
                with pytest.raises(vo.VoError):
                    svo.getZncc()  # the gate is off
            svo.close()
            return first, counts
        finally:
            c.close()
    # the allocation count: everything of the option at the first enable — one buffer — and flat afterwards: frame by frame the
    # gated loop allocates what the ungated loop allocates (the driver's and the context's own first-use allocations)
    _, plain = run(False)
    first, gated = run(True)
    assert first == 1, first
    assert gated == [v + first for v in plain], (plain, gated)
