"""The look-ahead loop tracks a prefetched pair's new-point candidates AHEAD of that pair's frame: the candidate role of the
frame kernel as a launch of its own on the side stream, right behind the pair's keypoint detection, its results kept with
the candidate table (frame_pipeline.hip: vo_frame_candidates_enqueue). It is the same kernel on the same inputs in a
different launch, so nothing may move: every case runs its stream twice — as built, and with VO_DBG_CANDS_IN_FRAME, which
keeps the candidates inside the frame kernel — and compares after EVERY frame the track set (ids, both pixel arrays, flags,
world points), the pose, the keyframe decision and step [10]'s candidates and masks, bit for bit.

A frame whose result call raises (a left image without texture loses every feature) is part of the comparison: both runs must
raise the same error at the same frame and go on alike."""
import numpy as np
import pytest

from test_stereo_vo_gpu import _bits, _stream

pytestmark = pytest.mark.gpu

W, H, K = 640, 240, (400.0, 400.0, 320.0, 120.0)
NU, NV, N = 20, 8, 12  # the bucket grid and length of test_closed_loop_small


@pytest.fixture(scope="module")
def frames():
    st, imgs = _stream(W, H, K, NU, NV, 5, 0.5, N)
    for L, R in imgs:
        L.setflags(write=False)
        R.setflags(write=False)
    return st, imgs


def _snap(svo, gi):
    g = svo.getTracks()
    tri = (g["flags"] & 1) != 0
    rec = dict(frame_id=int(gi.frame_id), kf=bool(gi.is_keyframe), lba=bool(gi.lba_ran), T=_bits(np.array(gi.T_wc)).copy(),
               ids=g["ids"].copy(), pl=_bits(g["pts_l"]).copy(), pr=_bits(g["pts_r"]).copy(), flags=g["flags"].copy(),
               Xw=_bits(g["Xw"][tri]).copy(), counts=(int(gi.n_final), int(gi.n_new), int(gi.n_kf_tracked), int(gi.n_new_candidates)))
    if not gi.is_first:
        p = svo.getNewPoints()
        rec.update(np_l=_bits(p["pts_l"]).copy(), np_r=_bits(p["pts_r"]).copy(), np_m=p["mask_new"].copy(), np_a=p["accept"].copy())
    return rec


def _same(a, b, where):
    assert a.keys() == b.keys(), where
    for key in a:
        x, y = a[key], b[key]
        if isinstance(x, np.ndarray):
            assert x.shape == y.shape and np.array_equal(x, y), (where, key)
        else:
            assert x == y, (where, key, x, y)


def _run(vo, st, imgs, *, in_frame, strict=4, lba=True, sum_order="tree", prefetch=None, sync=(), fail_join_at=None, probe=None):
    """One stream through the look-ahead loop: enqueue(k), prefetch(what follows), result(k).
    prefetch: {k: pair or None} — what is handed over behind enqueue(k) instead of imgs[k + 1]; sync: frames that go through the
    one-call form (nothing handed over for them counts: a prefetch in front of them is left behind);
    fail_join_at: the frame whose device-side joins cannot be met (VO_DBG_FAIL_JOIN); probe(k, ctx) runs after every frame.
    Returns the per-frame records and the context's count of re-issued frames."""
    prefetch = prefetch or {}
    c = vo.Context(device=0, max_width=W, max_height=H, max_points=4096, n_slots=5, max_level=4, sum_order=sum_order)
    try:
        c.debug_set(c.DBG_CANDS_IN_FRAME, 1 if in_frame else 0)
        svo = vo.StereoVO(c, W, H, K, K, st.T_lr, NU, NV, thres_fastscore=15, window_size=21, max_level=4, strict_border=strict,
                          local_ba=lba, thres_trans=0.9)
        recs = []
        for k, (L, R) in enumerate(imgs):
            try:
                if k in sync:
                    gi = svo.trackStereoImages(L, R)
                else:
                    if fail_join_at == k:
                        c.debug_set(c.DBG_FAIL_JOIN, 1)
                    svo.enqueue(L, R)
                    c.debug_set(c.DBG_FAIL_JOIN, 0)
                    nxt = prefetch.get(k, imgs[k + 1] if k + 1 < len(imgs) and (k + 1) not in sync else None)
                    if nxt is not None:
                        svo.prefetch(*nxt)
                    gi = svo.result()
                recs.append(_snap(svo, gi))
            except vo.VoError as e:
                recs.append(dict(error=str(e)))
            if probe:
                probe(k, c)
        rec = c.frame_recoveries()
        svo.close()
        return recs, rec
    finally:
        c.close()


def _both(vo, st, imgs, **kw):
    a, ra = _run(vo, st, imgs, in_frame=False, **kw)
    b, rb = _run(vo, st, imgs, in_frame=True, **kw)
    assert len(a) == len(b) == len(imgs)
    for k, (x, y) in enumerate(zip(a, b)):
        _same(x, y, f"frame {k}")
    return a, ra, rb


@pytest.mark.parametrize("strict", [1, 4])
@pytest.mark.parametrize("lba", [False, True])
def test_look_ahead_loop(vo, frames, strict, lba):
    st, imgs = frames
    recs, ra, rb = _both(vo, st, imgs, strict=strict, lba=lba)
    assert ra == rb == 0 and not any("error" in r for r in recs)
    assert sum(r["kf"] for r in recs) >= 2 and len(recs[-1]["ids"]) > 100
    assert any(r["np_m"].any() for r in recs[1:])  # (step [10] emitted and accepted something: the masks are not vacuous)
    if lba:
        assert sum(r["lba"] for r in recs) >= 2


def test_reference_summation_order(vo, frames):
    st, imgs = frames
    recs, ra, rb = _both(vo, st, imgs, strict=4, lba=True, sum_order="reference")
    assert ra == rb == 0 and not any("error" in r for r in recs) and sum(r["lba"] for r in recs) >= 2


def test_tracked_ahead_launches_are_bracketed_as_the_frame_kernel(vo, frames):
    """The path under test is the one taken: with the event brackets on, every prefetched pair adds one launch under the frame
    kernel's key (VO_K_KLT) — and none with the switch."""
    st, imgs = frames
    n = {}
    for in_frame in (False, True):
        c = vo.Context(device=0, max_width=W, max_height=H, max_points=4096, n_slots=5, max_level=4)
        try:
            c.debug_set(c.DBG_CANDS_IN_FRAME, int(in_frame))
            c.profile_enable(256)
            c.profile_set_classes(1 << 1)
            svo = vo.StereoVO(c, W, H, K, K, st.T_lr, NU, NV, thres_fastscore=15, window_size=21, max_level=4, strict_border=4,
                              local_ba=False, thres_trans=0.9)
            for k in range(6):
                svo.enqueue(*imgs[k])
                if k + 1 < 6:
                    svo.prefetch(*imgs[k + 1])
                svo.result()
            c.synchronize()
            n[in_frame] = c.profile_get(1)[0]
            svo.close()
        finally:
            c.close()
    assert n[False] - n[True] == 5, n


def test_flat_left_image_mid_stream(vo, frames):
    """A table without a keypoint in any bin: every workgroup of the candidates' launch takes the early return — and must still
    count itself, or the BA launch's join would time out and the frame be issued again."""
    st, imgs = frames
    imgs = list(imgs)
    imgs[6] = (np.full_like(imgs[6][0], 90), imgs[6][1])
    recs, ra, rb = _both(vo, st, imgs, strict=4, lba=True)
    assert ra == rb == 0
    assert "error" in recs[6] or recs[6]["counts"][3] == 0, recs[6]  # (nothing to emit from that table)


def test_keypoints_in_the_first_bucket_row_only(vo, frames):
    """Texture strong enough for FAST in the first bucket row only (below it the contrast is a tenth): the table's other
    rows are empty, the launch mixes early returns with tracked candidates."""
    st, imgs = frames
    imgs = list(imgs)
    L = imgs[6][0].astype(np.float32)
    v_step = H // NV
    L[v_step:] = 100.0 + 0.1 * (L[v_step:] - 100.0)
    imgs[6] = (np.clip(np.rint(L), 0, 255).astype(np.uint8), imgs[6][1])
    recs, ra, rb = _both(vo, st, imgs, strict=4, lba=True)
    assert ra == rb == 0
    if "error" not in recs[6]:
        assert (recs[6]["np_l"].view(np.float32).reshape(-1, 2)[:, 1] < v_step).all()


def test_prefetched_pair_is_not_the_one_enqueued(vo, frames):
    """Pair 9 is handed over behind frame 5, then pair 6 is enqueued: the table tracked for pair 9 is left behind (its launch
    still counts), frame 6 takes the synchronous call's path — and equals that call's result without any prefetch before it."""
    st, imgs = frames
    recs, ra, rb = _both(vo, st, imgs, prefetch={5: imgs[9]})
    assert ra == rb == 0 and not any("error" in r for r in recs)
    plain, rp = _run(vo, st, imgs, in_frame=False, prefetch={5: None})
    assert rp == 0
    for k, (x, y) in enumerate(zip(recs, plain)):
        _same(x, y, f"frame {k}")


def test_prefetch_at_the_end_without_its_enqueue(vo, frames):
    """The last pair is handed over and never enqueued; one more pair (the same pixels in other arrays) then comes through the
    one-call form. It equals the loop that enqueues the prefetched pair."""
    st, imgs = frames
    last = (imgs[N - 1][0].copy(), imgs[N - 1][1].copy())
    seq = list(imgs[:N - 1]) + [last]
    recs, ra, rb = _both(vo, st, seq, prefetch={N - 2: imgs[N - 1]}, sync=(N - 1,))
    assert ra == rb == 0 and not any("error" in r for r in recs)
    loop, rl = _run(vo, st, imgs, in_frame=False)
    assert rl == 0
    for k, (x, y) in enumerate(zip(recs, loop)):
        _same(x, y, f"frame {k}")


def test_join_timeout_with_a_tracked_table(vo, frames):
    """VO_DBG_FAIL_JOIN for frame 4, whose table was tracked ahead: the BA launch's joins run into their bound, the frame is
    issued again once — in stream order, from the table's results — and the stream equals the undisturbed one; from then on
    (the concurrent arrangements are off) nothing is tracked ahead, and the table tracked for pair 5 before the time-out is
    used in stream order. The time-out is faked through the switch: nothing faults."""
    st, imgs = frames
    calm, r0 = _run(vo, st, imgs, in_frame=False, strict=3)
    hit, r1 = _run(vo, st, imgs, in_frame=False, strict=3, fail_join_at=4)
    inside, r2 = _run(vo, st, imgs, in_frame=True, strict=3)
    assert (r0, r1, r2) == (0, 1, 0)
    for k in range(N):
        _same(calm[k], hit[k], f"frame {k}")
        _same(calm[k], inside[k], f"frame {k}")


def test_second_frame_of_a_stream(vo, frames):
    """Pair 1 is prefetched behind the stream's first frame, when neither its table nor the frame state exists yet."""
    st, imgs = frames
    recs, ra, rb = _both(vo, st, imgs[:3], lba=False)
    assert ra == rb == 0 and not any("error" in r for r in recs) and recs[1]["counts"][3] > 0


def test_steady_frames_allocate_nothing(vo):
    """The probe of test_steady_state_frames_allocate_nothing on the look-ahead path: the tables' result arrays and events
    exist from the second pair's prefetch on."""
    st, imgs = _stream(W, H, K, NU, NV, 21, 0.5, 31)
    seen = {}

    def probe(k, c):
        if k == 2 or k == 30:
            seen[k] = c.allocation_count()

    recs, rec = _run(vo, st, imgs, in_frame=False, probe=probe)
    assert rec == 0 and not any("error" in r for r in recs)
    assert sum(r["kf"] for r in recs) >= 10 and sum(r["lba"] for r in recs) >= 8
    assert seen[2] == seen[30], seen
