"""The CLAHE kernels (csrc/clahe_device.hpp) on CPU threads (tests/emu/emu_clahe.cpp, with the product's launch geometry) against
the numpy restatement (tests/clahe_restatement.py): look-up tables and output bytes equal. Shapes: no extension; both dimensions
extended; the full-tile extension of a dividing dimension; a clip limit that floors to 0 and is raised to 1; one-pixel steps next to
the reflected edge. Contents: noise, low contrast, constant, a half of one value (the residual path in some tiles only), and a
source whose stride exceeds its width. No GPU."""
import os
import subprocess

import numpy as np
import pytest

from clahe_restatement import clahe, extension

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SHAPES = [(64, 48, (8, 8), 40.0), (67, 45, (4, 3), 40.0), (72, 45, (8, 8), 40.0), (40, 24, (8, 8), 0.5), (33, 17, (32, 16), 40.0)]
CONTENTS = ["noise", "low", "const", "half", "strided"]


@pytest.fixture(scope="module")
def emu_clahe(tmp_path_factory):
    out = tmp_path_factory.mktemp("emu") / "emu_clahe"
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-pthread", "-ffp-contract=off", os.path.join(ROOT, "tests", "emu", "emu_clahe.cpp"),
                           "-o", str(out)])
    return str(out)


def make_image(kind, w, h, seed=0):
    rng = np.random.default_rng(seed + w * 1000 + h)
    noise = rng.integers(0, 256, (h, w), dtype=np.uint8)
    if kind == "low":
        return (100 + noise // 8).astype(np.uint8)
    if kind == "const":
        return np.full((h, w), 77, np.uint8)
    if kind == "half":
        img = noise.copy()
        img[:, :w // 2] = 200
        return img
    return noise


def run_emu(exe, tmp_path, img, stride, tiles, clip, slab_px=None):
    h, w = img.shape
    buf = np.full((h, stride), 0xEE, np.uint8)
    buf[:, :w] = img
    fin, fout, flut = tmp_path / "in.raw", tmp_path / "out.raw", tmp_path / "luts.raw"
    fin.write_bytes(buf.tobytes())
    cmd = [exe, str(w), str(h), str(stride), str(tiles[0]), str(tiles[1]), repr(float(clip)), str(fin), str(fout), str(flut)]
    subprocess.check_call(cmd + ([str(slab_px)] if slab_px else []))
    out = np.frombuffer(fout.read_bytes(), np.uint8).reshape(h, w)
    luts = np.frombuffer(flut.read_bytes(), np.uint8).reshape(tiles[1], tiles[0], 256)
    return out, luts


@pytest.mark.parametrize("kind", CONTENTS)
@pytest.mark.parametrize("w,h,tiles,clip", SHAPES)
def test_kernel_text_equals_restatement(emu_clahe, tmp_path, w, h, tiles, clip, kind):
    img = make_image(kind, w, h)
    want, want_luts = clahe(img, clip, tiles)
    out, luts = run_emu(emu_clahe, tmp_path, img, w + 13 if kind == "strided" else w, tiles, clip)
    assert np.array_equal(luts, want_luts)
    assert np.array_equal(out, want)


@pytest.mark.parametrize("w,h,tiles,clip", [(67, 45, (4, 3), 40.0), (72, 45, (8, 8), 2.0), (300, 21, (2, 4), 0.0)])
def test_several_workgroups_per_tile(emu_clahe, tmp_path, w, h, tiles, clip):
    """a small slab makes several workgroups share a tile's counters and ticket (the full-size images' path); 300 wide: two
    workgroups per row of the blend"""
    _, _, tw, th = extension(w, h, *tiles)
    assert th >= 3
    img = make_image("half", w, h, seed=5)
    want, want_luts = clahe(img, clip, tiles)
    out, luts = run_emu(emu_clahe, tmp_path, img, w, tiles, clip, slab_px=2 * tw)
    assert np.array_equal(luts, want_luts) and np.array_equal(out, want)
