"""The ZNCC kernel (csrc/zncc_device.hpp) on CPU threads (tests/emu/emu_zncc.cpp, with the product's launch geometry: one
wavefront per feature, four features per workgroup, two image pairs in one launch) against the numpy restatement
(tests/zncc_restatement.py): every float equal to the bit, NaN as NaN. Windows of every register count per lane (1, 2, 4, 8,
16), both patterns, both summation orders; points inside, on integers, within a window of each border, with u in (-1, 0), beyond
W - 1 and NaN; a constant image; a source whose stride exceeds its width; a feature count that is no multiple of the workgroup's
four. No GPU."""
import os
import subprocess

import numpy as np
import pytest

from zncc_restatement import zncc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H = 97, 61


@pytest.fixture(scope="module")
def emu_zncc(tmp_path_factory):
    out = tmp_path_factory.mktemp("emu") / "emu_zncc"
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-pthread", "-ffp-contract=off", os.path.join(ROOT, "tests", "emu", "emu_zncc.cpp"),
                           "-o", str(out)])
    return str(out)


def images(kind):
    rng = np.random.default_rng(11)
    base = rng.integers(0, 256, (H + 4, W + 4), dtype=np.uint8)
    smooth = ((base[:-4, :-4].astype(np.int32) + base[2:-2, 2:-2] + base[4:, 4:] + base[:-4, 4:]) // 4).astype(np.uint8)
    if kind == "const":
        return np.full((H, W), 77, np.uint8), smooth
    other = np.clip(smooth.astype(np.int32) // 2 + 40 + rng.integers(-6, 7, (H, W)), 0, 255).astype(np.uint8)  # gain, offset, noise
    return smooth, other


def points(win):
    """pts0 [n, 2], pts1 [n, 2]: 13 points (four workgroups, the last one with a single feature)"""
    f = np.float32
    p0 = np.array([[40.25, 30.75], [50.0, 31.0], [win - 0.5, 33.3], [W - 2.5, 20.1], [44.4, win - 1.25], [47.7, H - 1.5],
                   [-0.5, 30.0], [30.0, -0.75], [W - 1.0, 30.0], [W + 40.0, 30.0], [np.nan, 30.0], [40.0, np.nan], [60.5, 40.5]], f)
    p1 = p0 + np.array([0.4, -0.3], f)
    p1[1] = p0[1]  # (integer coordinates on both sides)
    return p0, p1


def run_emu(exe, tmp_path, img0, img1, stride, p0, p1, win, pattern, order):
    h, w = img0.shape
    files = []
    for k, img in enumerate((img0, img1)):
        buf = np.full((h, stride), 0xEE, np.uint8)
        buf[:, :w] = img
        files.append(tmp_path / f"img{k}.raw")
        files[-1].write_bytes(buf.tobytes())
    fp, fo = tmp_path / "pts.raw", tmp_path / "out.raw"
    fp.write_bytes(np.concatenate([p0, p1]).astype(np.float32).tobytes())
    subprocess.check_call([exe, str(w), str(h), str(stride), str(win), str(int(pattern == "centered")), str(int(order == "reference")),
                           str(len(p0)), str(files[0]), str(files[1]), str(fp), str(fo)])
    out = np.frombuffer(fo.read_bytes(), np.float32).reshape(2, len(p0))
    return out[0], out[1]


def bits(a):
    """the floats' bit patterns, every NaN as one pattern (NaN as NaN)"""
    a = np.ascontiguousarray(a, np.float32)
    return np.where(np.isnan(a), np.uint32(0x7FC00000), a.view(np.uint32))


def same_bits(a, b):
    return np.array_equal(bits(a), bits(b))


@pytest.mark.parametrize("order", ["tree", "reference"])
@pytest.mark.parametrize("pattern", ["reference", "centered"])
@pytest.mark.parametrize("win", [3, 9, 15, 21, 31])
def test_kernel_text_equals_restatement(emu_zncc, tmp_path, win, pattern, order):
    img0, img1 = images("noise")
    p0, p1 = points(win)
    want01 = zncc(img0, img1, p0, p1, win, pattern, order)
    want10 = zncc(img1, img0, p1, p0, win, pattern, order)
    assert np.isfinite(want01).sum() >= 6 and np.isnan(want01[-3:-1]).all()  # (a NaN coordinate: every tap -2, a flat patch)
    got01, got10 = run_emu(emu_zncc, tmp_path, img0, img1, W + 13, p0, p1, win, pattern, order)
    assert same_bits(got01, want01), (got01, want01)
    assert same_bits(got10, want10), (got10, want10)


def test_constant_image_is_nan(emu_zncc, tmp_path):
    img0, img1 = images("const")
    p0, p1 = points(15)
    want = zncc(img0, img1, p0, p1, 15, "centered", "tree")
    assert np.isnan(want[[0, 1, 12]]).all()  # a flat patch: 0 / 0 (a patch over the border is not flat: its outside taps read -2)
    got, _ = run_emu(emu_zncc, tmp_path, img0, img1, W, p0, p1, 15, "centered", "tree")
    assert same_bits(got, want), (got, want)
