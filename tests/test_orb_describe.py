"""CPU suite of the ORB orientation / descriptor (vo_orb_compute, vo_orb_detect_and_compute): the numpy restatement of
include/vo_hip.h (tests/orb_describe_restatement.py) is shown to be a descriptor worth having — rotation invariance, stereo
matching precision — the default table is pinned, the kernel's text runs on CPU threads against the restatement, and the
compiler's resource report of the kernel is checked. The GPU inherits these properties through the bit equalities of
tests/test_orb_describe_gpu.py."""
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import orb_describe_restatement as R
from visual_odometry_ros_amd import synthetic as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _stream(seed):
    return S.StereoStream(width=1241, height=376, n_u=8, n_v=4, n_new=8, seed=seed)


def _detect_describe(oracle, img, steer=True, nfeatures=2000, thr=15):
    o = oracle.orb_detect(img, thr, nfeatures=nfeatures, with_levels=True)
    _, _, ls, _ = oracle.orb_level_sizes(img.shape[1], img.shape[0], 1.2, 8, nfeatures)
    ang, desc, valid = R.describe(o["levels"], ls, o["xy"], o["octave"], R.seeded_pattern(), 31, steer)
    assert valid.all()  # the detector returns nothing nearer than the edge threshold to a level's border
    return o["xy"], o["octave"], desc


def test_default_pattern_is_the_documented_stream(vo):
    lib = vo.load()
    pat = np.zeros((512, 2), np.int8)
    assert lib.vo_orb_default_pattern(pat.ctypes.data) == 0
    assert np.array_equal(pat, R.seeded_pattern()) and pat.min() == -15 and pat.max() == 15


@pytest.mark.parametrize("seed", [4, 5, 9])
def test_rotation_invariance_of_the_restated_descriptor(oracle, seed):
    """An image and its exact np.rot90: octave-0 keypoints map one to one, (x, y) -> (y, W - 1 - x). Steered, at least 95 % of
    them are accepted by the rule (50, 0.6) with their true counterpart (0.5 px); unsteered fewer than 5 %. Observed:
    every one of them at distance 0 / none."""
    st = _stream(seed)
    img = st.render_pair(st.poses(1)[0])[0]
    rot = np.ascontiguousarray(np.rot90(img))
    W = img.shape[1]
    for steer in (True, False):
        xa, oa, da = _detect_describe(oracle, img, steer)
        xb, ob, db = _detect_describe(oracle, rot, steer)
        sa, sb = oa == 0, ob == 0
        bi, bd, sd = oracle.hamming_match(da[sa], db[sb], 50, 0.6)
        truth = np.stack([xa[sa][:, 1], (W - 1) - xa[sa][:, 0]], 1)
        err = np.linalg.norm(xb[sb][np.maximum(bi, 0)] - truth, axis=1)
        good = int(((bi >= 0) & (err <= 0.5)).sum())
        total = int(sa.sum())
        print(f"seed {seed} steer {steer}: {good} of {total} octave-0 keypoints accepted with their counterpart "
              f"({int((bi >= 0).sum())} accepted, {int(sb.sum())} in the rotated image)")
        assert total > 100
        if steer:
            assert good >= 0.95 * total
        else:
            assert good < 0.05 * total


STEREO_FLOOR = 787 / 808 - 0.02  # the lowest of the three measured precisions below (seed 9), minus 0.02


@pytest.mark.parametrize("seed", [4, 5, 9])
def test_stereo_precision_of_the_restated_descriptor(oracle, seed):
    """Left -> right under the rule (50, 0.6) on StereoStream(1241, 376, n_u=8, n_v=4, n_new=8, seed) frame 0, FAST 15,
    nfeatures 2000: correct = within 3 px of (x - fx b / z, y). Measured on this restatement with the default table
    (accepted / correct / keypoints): seed 4: 784 / 775 / 2000 (0.989); seed 5: 764 / 753 / 2000 (0.986); seed 9: 808 /
    787 / 2000 (0.974). The floor is the lowest of the three minus 0.02 — room for another table, not for a broken
    descriptor (random bytes give no accepted match at all); at least a quarter of the keypoints must be accepted."""
    st = _stream(seed)
    L, Rt, depth = st.render_pair(st.poses(1)[0])
    xa, oa, da = _detect_describe(oracle, L)
    xb, ob, db = _detect_describe(oracle, Rt)
    bi, bd, sd = oracle.hamming_match(da, db, 50, 0.6)
    h, w = L.shape
    z = depth[np.clip(np.rint(xa[:, 1]).astype(int), 0, h - 1), np.clip(np.rint(xa[:, 0]).astype(int), 0, w - 1)]
    truth = np.stack([xa[:, 0] - st.K[0] * st.baseline / z, xa[:, 1]], 1)
    err = np.linalg.norm(xb[np.maximum(bi, 0)] - truth, axis=1)
    acc = int((bi >= 0).sum())
    good = int(((bi >= 0) & (err <= 3.0)).sum())
    print(f"seed {seed}: accepted {acc}, correct {good} ({good / max(acc, 1):.3f}) of {xa.shape[0]} keypoints")
    assert acc >= 0.25 * xa.shape[0]
    assert good / acc >= STEREO_FLOOR


def _emu_cases(oracle):
    """333 x 251 noise, edge threshold 16: keypoints on every level incl. ones whose window crosses the level's border, ones
    too near the border, bad octaves and a NaN."""
    rng = np.random.default_rng(0)
    img = rng.integers(0, 256, (251, 333), dtype=np.uint8)
    o = oracle.orb_detect(img, 60, nfeatures=50, edge_threshold=16, with_levels=True, max_kp=400000)
    lw, lh, ls, _ = oracle.orb_level_sizes(333, 251, 1.2, 8, 50)
    xy, octv = [], []
    for l in range(8):
        w, h, s = int(lw[l]), int(lh[l]), np.float32(ls[l])
        for (x, y) in ((16, 16), (w - 17, h - 17), (16, h // 2), (w // 2, 16), (w // 2, h // 2), (w - 17, 20), (15, 40), (40, h - 16),
                       (w - 16, 40), (rng.integers(16, w - 16), rng.integers(16, h - 16))):
            xy.append((np.float32(x) * s if l else x, np.float32(y) * s if l else y))
            octv.append(l)
    xy += [(100.0, 100.0), (100.0, 100.0), (float("nan"), 50.0), (-1e30, 50.0), (100.4, 99.6)]
    octv += [-1, 8, 0, 0, 0]
    return o["levels"], ls, np.array(xy, np.float32), np.array(octv, np.int32)


@pytest.fixture(scope="module")
def emu_describe(tmp_path_factory):
    out = tmp_path_factory.mktemp("emu") / "emu_describe"
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-pthread", "-ffp-contract=off", os.path.join(ROOT, "tests", "emu", "emu_describe.cpp"),
                           "-o", str(out)])
    return str(out)


@pytest.mark.parametrize("steer", [1, 0])
def test_describe_kernel_text_on_cpu_threads(oracle, emu_describe, tmp_path, steer):
    """csrc/orb_describe.hpp compiled by g++ and run on OS threads (tests/emu/hip_emu.h): descriptors, angles and `valid`
    equal to the restatement, with the default table and with another seeded one."""
    levels, ls, xy, octv = _emu_cases(oracle)
    n = xy.shape[0]
    for pat in (R.seeded_pattern(), R.seeded_pattern(77)):
        blob = struct.pack("4i", len(levels), 16, steer, n)
        for l, im in enumerate(levels):
            blob += struct.pack("2if", im.shape[1], im.shape[0], float(ls[l]))
        blob += b"".join(np.ascontiguousarray(im).tobytes() for im in levels) + xy.tobytes() + octv.tobytes() + pat.tobytes()
        fin, fout = tmp_path / "in.bin", tmp_path / "out.bin"
        fin.write_bytes(blob)
        subprocess.check_call([emu_describe, str(fin), str(fout)])
        raw = fout.read_bytes()
        ang = np.frombuffer(raw, np.float32, n, 0)
        desc = np.frombuffer(raw, np.uint8, 32 * n, 4 * n).reshape(n, 32)
        valid = np.frombuffer(raw, np.uint8, n, 36 * n)
        a_ref, d_ref, v_ref = R.describe(levels, ls, xy, octv, pat, 16, bool(steer))
        assert np.array_equal(valid, v_ref.astype(np.uint8)) and 50 < int(v_ref.sum()) < n
        assert np.array_equal(ang.view(np.uint32), a_ref.view(np.uint32))
        assert np.array_equal(desc, d_ref)
        assert not desc[~v_ref].any() and len(np.unique(desc[v_ref], axis=0)) > 40


def test_describe_kernel_uses_no_scratch_memory():
    """the pattern and the window live in LDS, nothing is indexed at run time in registers: 0 scratch bytes, 0 spilled VGPRs
    (same method as tests/test_kernel_resources.py)"""
    from visual_odometry_ros_amd import build as B
    if not os.path.exists(B.HIPCC):
        pytest.skip("no hipcc")
    flags = [f for f in B.FLAGS if f not in ("-Wall", "-Wno-unused-function")]
    cmd = [B.HIPCC] + flags + ["-I" + os.path.join(ROOT, "include"), "-I" + B.CSRC, "--offload-device-only",
                               "-Rpass-analysis=kernel-resource-usage", "-c", os.path.join(B.CSRC, "orb_describe.hip"), "-o", os.devnull]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    txt = r.stderr[r.stderr.index("orb_describe_kernel"):]
    got = {k: int(re.search(re.escape(k) + r": (\d+)", txt).group(1)) for k in ("ScratchSize [bytes/lane]", "VGPRs Spill", "VGPRs", "LDS Size [bytes/block]")}
    print(got)
    assert got["ScratchSize [bytes/lane]"] == 0 and got["VGPRs Spill"] == 0 and got["LDS Size [bytes/block]"] <= 16384
