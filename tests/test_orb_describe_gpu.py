"""ORB orientation and descriptors on the device (vo_orb_compute, vo_orb_detect_and_compute, vo_orb_match_sets) against the
numpy restatement of include/vo_hip.h (tests/orb_describe_restatement.py): every comparison is an equality — the
definition is integer arithmetic plus individually rounded float operations."""
import os
import subprocess

import numpy as np
import pytest

import orb_describe_restatement as R
from visual_odometry_ros_amd import synthetic as S

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _frame(seed, w=1241, h=376, right=False):
    st = S.StereoStream(width=w, height=h, n_u=8, n_v=4, n_new=8, seed=seed)
    return st.render_pair(st.poses(1)[0])[1 if right else 0]


def _fe(ctx, vo, img, thr=15, **orb):
    fe = vo.FeatureExtractor(ctx)
    fe.initParams(img.shape[1], img.shape[0], 20, 12, THRES_FAST=thr)
    for k, v in orb.items():
        setattr(fe.orb, k, v)
    ctx.set_image(0, img)
    return fe


def _restate(oracle, fe, img, xy, octv, steer=True, pattern=None):
    o = oracle.orb_detect(img, fe.orb.fast_threshold, nfeatures=fe.orb.nfeatures, scale_factor=fe.orb.scale_factor,
                          n_levels=fe.orb.n_levels, edge_threshold=fe.orb.edge_threshold, with_levels=True, max_kp=400000)
    _, _, ls, _ = oracle.orb_level_sizes(img.shape[1], img.shape[0], fe.orb.scale_factor, fe.orb.n_levels, fe.orb.nfeatures)
    return R.describe(o["levels"], ls, xy, octv, R.seeded_pattern() if pattern is None else pattern, fe.orb.edge_threshold, steer)


def _check_full(ctx, vo, oracle, img, thr=15, **orb):
    fe = _fe(ctx, vo, img, thr, **orb)
    xy0, resp0, oct0 = fe.detect(0)
    xy, resp, octv, ang, size, desc = fe.extractAndComputeORB(0)
    assert np.array_equal(xy.view(np.uint32), xy0.view(np.uint32)) and np.array_equal(resp.view(np.uint32), resp0.view(np.uint32))
    assert np.array_equal(octv, oct0)
    a_ref, d_ref, v_ref = _restate(oracle, fe, img, xy, octv)
    bad = np.nonzero((ang.view(np.uint32) != a_ref.view(np.uint32)) | (desc != d_ref).any(axis=1))[0]
    print(f"{img.shape[1]}x{img.shape[0]} {orb}: {xy.shape[0]} keypoints, {bad.size} differ from the restatement")
    assert v_ref.all() and bad.size == 0, (bad[:10], ang[bad[:10]], a_ref[bad[:10]])
    assert np.array_equal(size, (np.float32(31.0) * oracle.orb_level_sizes(img.shape[1], img.shape[0], fe.orb.scale_factor,
                                                                             fe.orb.n_levels, fe.orb.nfeatures)[2][octv]))
    return fe, xy, octv, ang, desc


@pytest.mark.parametrize("seed", [4, 9])
def test_extract_and_compute_kitti_shape(ctx, vo, oracle, seed):
    fe, xy, octv, ang, desc = _check_full(ctx, vo, oracle, _frame(seed))
    assert xy.shape[0] > 5000 and len(np.unique(desc, axis=0)) > 0.9 * xy.shape[0]


def test_extract_and_compute_other_shapes(vo, oracle):
    c = vo.Context(device=0, max_width=752, max_height=480, max_points=2048, n_slots=2, max_level=4)
    try:
        _check_full(c, vo, oracle, _frame(5, 752, 480), 20)
        fe = _fe(c, vo, np.full((480, 752), 90, np.uint8), 20)  # no keypoint at all
        out = fe.extractAndComputeORB(0, set=1)
        assert out[0].shape == (0, 2) and out[5].shape == (0, 32)
    finally:
        c.close()


def test_extract_and_compute_4k(ctx5, vo, oracle):
    st = S.StereoStream(width=3840, height=2160, K=(718.856 * 3.0, 718.856 * 3.0, 1920.0, 1080.0), n_u=100, n_v=80, seed=2)
    _check_full(ctx5, vo, oracle, st.render_pair(st.poses(1)[0])[0])


def test_compute_on_caller_keypoints(ctx, vo, oracle):
    img = _frame(4)
    fe, xy, octv, ang, desc = _check_full(ctx, vo, oracle, img)
    rng = np.random.default_rng(3)
    sel = rng.permutation(xy.shape[0])[:3000]
    a, d, v = fe.compute(0, xy[sel], octv[sel])
    assert v.all() and np.array_equal(a.view(np.uint32), ang[sel].view(np.uint32)) and np.array_equal(d, desc[sel])
    # steer = 0: plain BRIEF
    a0, d0, v0 = fe.compute(0, xy[sel], octv[sel], steer=False)
    a_ref, d_ref, v_ref = _restate(oracle, fe, img, xy[sel], octv[sel], steer=False)
    assert v0.all() and not a0.any() and np.array_equal(d0, d_ref) and not np.array_equal(d0, d)
    # out of the border, octaves that do not exist, a NaN: invalid, zero descriptor, angle 0
    kp = np.array([[5.0, 100.0], [600.0, 30.9], [600.0, 31.0], [1241.0 - 31.4, 200.0], [600.0, 200.0], [600.0, 200.0], [np.nan, 200.0],
                   [600.0, 376.0 - 31.6]], np.float32)
    oc = np.array([0, 0, 0, 0, -1, 8, 0, 0], np.int32)
    a, d, v = fe.compute(0, kp, oc)
    a_ref, d_ref, v_ref = _restate(oracle, fe, img, kp, oc)
    assert v.tolist() == v_ref.tolist() == [False, True, True, False, False, False, False, True]
    assert np.array_equal(a.view(np.uint32), a_ref.view(np.uint32)) and np.array_equal(d, d_ref) and not d[~v].any() and not a[~v].any()
    # n = 0
    a, d, v = fe.compute(0, np.zeros((0, 2), np.float32), np.zeros(0, np.int32))
    assert a.shape == (0,) and d.shape == (0, 32) and v.shape == (0,)


def test_other_detector_parameters(ctx, vo, oracle):
    img = _frame(9)
    _check_full(ctx, vo, oracle, img, 7, nfeatures=600)
    fe, xy, octv, ang, desc = _check_full(ctx, vo, oracle, img, 12, n_levels=3, scale_factor=1.5, edge_threshold=16)
    # windows that cross the level's border (edge threshold 16 < 25)
    kp = np.array([[16.0, 16.0], [1241.0 - 17, 376.0 - 17], [16.0 * 1.5, 200.0], [24.0, 24.0]], np.float32)
    oc = np.array([0, 0, 1, 2], np.int32)
    a, d, v = fe.compute(0, kp, oc)
    a_ref, d_ref, v_ref = _restate(oracle, fe, img, kp, oc)
    assert v.tolist() == v_ref.tolist() and v[:3].all()
    assert np.array_equal(a.view(np.uint32), a_ref.view(np.uint32)) and np.array_equal(d, d_ref)


def test_set_pattern(vo, oracle):
    c = vo.Context(device=0, max_width=1241, max_height=376, max_points=2048, n_slots=2, max_level=4)
    try:
        img = _frame(4)
        fe = _fe(c, vo, img)
        assert np.array_equal(fe.getPattern(), R.seeded_pattern())
        xy, resp, octv, ang, size, desc = fe.extractAndComputeORB(0)
        other = R.seeded_pattern(12345)
        fe.setPattern(other)
        assert np.array_equal(fe.getPattern(), other)
        xy2, _, octv2, ang2, _, desc2 = fe.extractAndComputeORB(0)
        a_ref, d_ref, _ = _restate(oracle, fe, img, xy2, octv2, pattern=other)
        assert np.array_equal(ang2.view(np.uint32), ang.view(np.uint32)) and np.array_equal(desc2, d_ref) and not np.array_equal(desc2, desc)
        bad = other.copy()
        bad[100, 1] = 16
        with pytest.raises(vo.VoError) as e:
            fe.setPattern(bad)
        assert e.value.code == -1 and np.array_equal(fe.getPattern(), other)
    finally:
        c.close()


def test_match_sets_and_repeated_calls(ctx, vo, oracle):
    L, Rt = _frame(4), _frame(4, right=True)
    fe = _fe(ctx, vo, L)
    outL = fe.extractAndComputeORB(0, set=0)
    ctx.set_image(1, Rt)
    outR = fe.extractAndComputeORB(1, set=1)
    bi, bd, sd = fe.matchSets(0, 1)
    ri, rd, rs = oracle.hamming_match(outL[5], outR[5], 50, 0.6)
    assert np.array_equal(bi, ri) and np.array_equal(bd, rd) and np.array_equal(sd, rs)
    assert (bi >= 0).sum() > 0.2 * bi.shape[0]
    m = 4000  # a prefix the upload path takes (<= max_points)
    pi, pd, ps = fe.match(outL[5][:m], outR[5])
    assert np.array_equal(pi, bi[:m]) and np.array_equal(pd, bd[:m]) and np.array_equal(ps, sd[:m])
    # repeated calls: the same bytes and no allocation
    n0 = ctx.allocation_count()
    for _ in range(3):
        again = fe.extractAndComputeORB(0, set=0)
        assert all(np.array_equal(x, y) for x, y in zip(again, outL))
        bi2, bd2, sd2 = fe.matchSets(0, 1)
        assert np.array_equal(bi2, bi) and np.array_equal(bd2, bd)
        a, d, v = fe.compute(0, outL[0][:3000], outL[2][:3000])
        assert np.array_equal(d, outL[5][:3000])
        if _ == 0:
            n0 = ctx.allocation_count()  # (the first compute of this size may allocate)
    assert ctx.allocation_count() == n0


def test_cpp_demo_writes_the_python_bytes(ctx, vo, tmp_path):
    """tests/cpp/orb_describe_demo.cpp: vo::FeatureExtractor::extractAndComputeORB / compute / matchSets on plain arrays."""
    libdir = os.path.join(ROOT, "visual_odometry_ros_amd", "lib")
    exe = str(tmp_path / "orb_describe_demo")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I", ROOT, os.path.join(ROOT, "tests", "cpp", "orb_describe_demo.cpp"), "-o", exe,
                           "-L", libdir, "-lvo_hip", f"-Wl,-rpath,{libdir}", "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib", "-lamdhip64"])
    L, Rt = _frame(4), _frame(4, right=True)
    raw, out = tmp_path / "pair.u8", tmp_path / "out.bin"
    raw.write_bytes(L.tobytes() + Rt.tobytes())
    r = subprocess.run([exe, str(raw), "1241", "376", "15", str(out)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-1500:]
    fe = _fe(ctx, vo, L)
    xy, resp, octv, ang, size, desc = fe.extractAndComputeORB(0, set=0)
    ctx.set_image(1, Rt)
    fe.extractAndComputeORB(1, set=1)
    bi, bd, sd = fe.matchSets(0, 1)
    blob = out.read_bytes()
    n = int(np.frombuffer(blob, np.int32, 1)[0])
    want = xy.tobytes() + octv.tobytes() + ang.tobytes() + size.tobytes() + desc.tobytes() + bi.tobytes() + bd.tobytes()
    assert n == xy.shape[0] and blob[4:] == want
