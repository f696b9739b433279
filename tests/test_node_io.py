"""CPU suite of the nodes' image encodings (vo_set_input_format) and of the debug image's rasterisation (vo_draw_tracking,
vo_draw_tracking_ba): the kernels' own sample functions and coverage predicates (csrc/ingest_formats.hpp, csrc/draw_device.hpp)
run on the CPU against the numpy restatement of include/vo_hip.h (tests/node_io_restatement.py); the gray restatement against
the float formula; the adapter's new image types against the stand-in headers; the compiler's resource report of the render
kernels. The GPU inherits the restatement through the bit equalities of tests/test_node_io_gpu.py."""
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import node_io_restatement as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STUBS = os.path.join(ROOT, "tests", "typecheck_stubs")
LIBDIR = os.path.join(ROOT, "visual_odometry_ros_amd", "lib")


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    out = tmp_path_factory.mktemp("emu") / "emu_node_io"
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-pthread", "-ffp-contract=off", os.path.join(ROOT, "tests", "emu", "emu_node_io.cpp"),
                           "-o", str(out)])
    return str(out)


def _run(emu, tmp_path, blob, n_out):
    fin, fout = tmp_path / "in.bin", tmp_path / "out.bin"
    fin.write_bytes(blob)
    subprocess.check_call([emu, str(fin), str(fout)])
    raw = fout.read_bytes()
    assert len(raw) == n_out
    return np.frombuffer(raw, np.uint8)


# ---- ingestion ---------------------------------------------------------------------------------------------------
W, H = 37, 29


@pytest.mark.parametrize("fmt", list(R.FORMATS))
def test_ingest_sample_text_on_the_cpu(emu, tmp_path, fmt):
    """csrc/ingest_formats.hpp compiled by g++: 37 x 29, rows 3 bytes longer than the pixels need (odd: 16-bit and float rows
    are not aligned), the edge-case maps, the special samples of the format — bytes equal to the restatement."""
    img = R.make_image(fmt, W, H, seed=3)
    mu, mv = R.edge_case_maps(W, H)
    buf, stride = R.strided(img, 3)
    blob = struct.pack("5i", 0, R.FORMATS[fmt], W, H, stride) + buf[:H * stride].tobytes() + mu.tobytes() + mv.tobytes()
    got = _run(emu, tmp_path, blob, W * H).reshape(H, W)
    ref = R.ingest(img, fmt, mu, mv)
    assert np.array_equal(got, ref)
    assert ref[1, 6] == 0 and ref[3, 0] == 0 and (ref > 0).mean() > 0.25  # far outside, NaN coordinate; the rest is image (half of the signed samples are negative)
    if fmt not in ("rgb8", "bgr8"):
        assert ref[4, 0] == 10 and ref[4, 1] == 12  # 10.5 -> 10, 11.5 -> 12


def test_float_conversion_rules():
    """the three rules of the final convertTo(CV_8UC1), on the restatement and through unmixed samples of the header's text (the
    f32 case above reads them through integer map coordinates)"""
    s = np.array(R.F32_SPECIALS, np.float32)
    want = [0, 0, 0, 0, 0, 254, 255, 255, 0, 2, 0, 0, 255]
    # NaN, +inf, -inf, 3e9 (>= 2^31), -7, 254.5 (even), 255.5 -> 256 -> 255, 300.5, 0.5 -> 0, 1.5 -> 2, +-2^31, just below 2^31
    assert R.float_to_u8(s).tolist() == want
    img = R.make_image("f32", W, H, seed=3)
    mu, mv = R.edge_case_maps(W, H)
    assert R.ingest(img, "f32", mu, mv)[5, :len(want)].tolist() == want
    for fmt, sp in (("mono16u", R.U16_SPECIALS), ("mono16s", R.S16_SPECIALS)):
        img = R.make_image(fmt, W, H, seed=3)
        assert R.ingest(img, fmt, mu, mv)[5, :len(sp)].tolist() == [min(max(v, 0), 255) for v in sp]


def test_restated_u8_remap_is_the_oracles(oracle):
    img = R.make_image("mono8", W, H, seed=3)
    mu, mv = R.edge_case_maps(W, H)
    assert np.array_equal(R.remap_u8(img, mu, mv), oracle.remap_linear_u8(img, mu, mv))
    # integers in [0, 255] as 16-bit or float samples: the float path gives the u8 path's bytes
    for fmt in ("mono16u", "mono16s", "f32"):
        assert np.array_equal(R.ingest(img.astype(R.DTYPES[fmt]), fmt, mu, mv), R.remap_u8(img, mu, mv))


def test_gray_restatement_against_the_float_formula():
    """All 2^24 colours: |((R*9798 + G*19235 + B*3735 + 16384) >> 15) - (0.299 R + 0.587 G + 0.114 B)| <= 1 gray level.
    Measured maximum: 0.503 (the rounding half plus the error of 0.299, 0.587, 0.114 in 15 bits)."""
    worst = 0.0
    g, b = np.meshgrid(np.arange(256), np.arange(256), indexing="ij")
    for r in range(256):
        rgb = np.stack([np.full_like(g, r), g, b], -1).astype(np.uint8)
        ref = 0.299 * r + 0.587 * g + 0.114 * b
        worst = max(worst, float(np.abs(R.gray(rgb).astype(np.float64) - ref).max()))
        if r == 200:  # channel 0 is R for rgb8, channel 2 for bgr8
            assert np.array_equal(R.gray(rgb[..., ::-1], bgr=True), R.gray(rgb))
    print(f"largest deviation of the 15-bit gray from the float formula: {worst:.6f}")
    assert worst <= 1.0
    assert R.gray(np.array([[[255, 255, 255]]], np.uint8))[0, 0] == 255 and R.gray(np.zeros((1, 1, 3), np.uint8))[0, 0] == 0


# ---- debug image -------------------------------------------------------------------------------------------------
DW, DH = 41, 33


def _draw_emu(emu, tmp_path, mode, sets, gray):
    sets = [np.asarray(s, np.float32).reshape(-1, 2) for s in sets] + [np.zeros((0, 2), np.float32)] * (3 - len(sets))
    blob = struct.pack("7i", 1, mode, len(sets[0]), len(sets[1]), len(sets[2]), gray.shape[1], gray.shape[0])
    blob += b"".join(s.tobytes() for s in sets) + gray.tobytes()
    return _run(emu, tmp_path, blob, gray.size * 3).reshape(gray.shape[0], gray.shape[1], 3)


def test_every_stamp_kind(emu, tmp_path):
    """each stamp alone in the middle of a flat image: the header's inequalities, pixel by pixel, and the shapes they give"""
    gray = np.full((DH, DW), 90, np.uint8)
    c = (20.0, 16.0)
    none = np.zeros((0, 2), np.float32)
    for mode, sets, (r, t, covers, colour) in ((1, ([c], none), (1, 4, R.circle_covers, (0, 0, 255))),
                                                 (1, (none, [c]), (6, 2, R.rect_covers, (0, 255, 0))),
                                                 (0, ([c], none, none), (2, 1, R.circle_covers, (255, 0, 255))),
                                                 (0, (none, none, [c]), (2, 1, R.circle_covers, (255, 0, 0)))):
        got = _draw_emu(emu, tmp_path, mode, sets, gray)
        want = np.repeat(gray[:, :, None], 3, 2)
        for y in range(DH):
            for x in range(DW):
                if mode == 0 and R.circle_covers(x - 20, y - 16, 3, 2):
                    want[y, x] = (0, 0, 0)
                if covers(x - 20, y - 16, r, t):
                    want[y, x] = colour
        assert np.array_equal(got, want)
    disc = _draw_emu(emu, tmp_path, 1, ([c], none), gray)
    assert (disc[16, 17:24] == (0, 0, 255)).all() and (disc[16, 16] == 90).all()  # circle(1, 4): a filled disc of radius 3
    sq = _draw_emu(emu, tmp_path, 1, (none, [c]), gray)
    assert (sq[16, 20] == 90).all() and (sq[16, 13:16] == (0, 255, 0)).all() and (sq[16, 16] == 90).all()  # hollow, 3 px wide
    assert (sq[9, 13:28] == (0, 255, 0)).all() and (sq[8, 13:28] == 90).all()


def test_lines_of_all_octants_and_overlap_order(emu, tmp_path):
    """lines from one centre into the eight octants and along the axes, n = 0, exact halves, points outside, NaN: the header's text
    equals the restatement; the line formula visits one pixel per step of the major axis and ends on both end points"""
    rng = np.random.default_rng(2)
    gray = rng.integers(0, 256, (DH, DW), dtype=np.uint8)
    ends = [(35, 20), (35, 9), (27, 2), (14, 2), (5, 9), (5, 22), (13, 30), (28, 30), (35, 16), (20, 2), (5, 16), (20, 30), (20, 16)]
    p0 = [(20.0, 16.0)] * len(ends) + [(2.5, 3.5), (-30.0, -20.0), (np.nan, 5.0), (10.0, 2e9)]
    p1 = [tuple(map(float, e)) for e in ends] + [(3.5, 4.5), (70.0, 60.0), (9.0, 9.0), (10.0, 10.0)]
    new = [(0.0, 0.0), (DW - 1.0, DH - 1.0), (DW + 2.0, 5.0), (20.0, 16.0)]
    got = _draw_emu(emu, tmp_path, 0, (p0, p1, new), gray)
    assert np.array_equal(got, R.draw_tracking(gray, np.array(p0, np.float32), np.array(p1, np.float32), np.array(new, np.float32)))
    for e in ends:
        px = R.line_pixels((20, 16), e, DW, DH)
        n = max(abs(e[0] - 20), abs(e[1] - 16))
        assert len(px) == n + 1 and px[0] == (20, 16) and px[-1] == e
        assert all(max(abs(a[0] - b[0]), abs(a[1] - b[1])) == 1 for a, b in zip(px, px[1:]))
    # a -> b and b -> a need not be the same pixels (floor division), but both are clipped, not wrapped
    assert R.line_pixels((-30, -20), (70, 60), DW, DH) and all(0 <= x < DW and 0 <= y < DH for x, y in R.line_pixels((-30, -20), (70, 60), DW, DH))
    # the same with lines of extreme length: python integers against the 64-bit arithmetic of the header
    far0 = [(-1.0e9, -1.0e9), (1.0e9, 7.0), (5.0, -1.0e9)]
    far1 = [(1.0e9, 1.0e9 + 64.0), (-1.0e9, 9.0), (6.0, 1.0e9)]
    got = _draw_emu(emu, tmp_path, 0, (far0, far1, []), gray)
    want = R.draw_tracking(gray, np.array(far0, np.float32), np.array(far1, np.float32), np.zeros((0, 2), np.float32))
    assert np.array_equal(got, want) and (want != np.repeat(gray[:, :, None], 3, 2)).any()


# ---- adapter -----------------------------------------------------------------------------------------------------
ADAPTER_SRC = r'''
#include "visual_odometry_ros_amd/core/visual_odometry/reference_adapter.h"
#include <cstdio>
#include <type_traits>
#include <utility>
static_assert(std::is_same<decltype(std::declval<StereoVO &>().getDebugImage()), const cv::Mat &>::value, "getDebugImage");
static_assert(std::is_same<decltype(std::declval<MonoVO &>().getDebugImage()), const cv::Mat &>::value, "getDebugImage");
// with flagDoUndistortion: what the ROS 2 node wraps (bgr8 / rgb8 -> CV_8UC3, mono16 -> CV_16UC1, 32FC1) is accepted
vo::Image undistorting(const cv::Mat &m, vo::Context &ctx, bool &set) { return vo_adapter::view(m, ctx, true, set); }
int main() {
  unsigned char buf[6 * 64] = {0};
  const int types[5] = {CV_8UC1, CV_8UC3, CV_16UC1, CV_16SC1, CV_32FC1};
  const int want[5] = {VO_PIX_MONO8, VO_PIX_RGB8, VO_PIX_MONO16U, VO_PIX_MONO16S, VO_PIX_F32};
  for (int k = 0; k < 5; ++k)
    if (vo_adapter::pixel_format(cv::Mat(6, 5, types[k], buf, 64)) != want[k]) return 1;
  if (vo_adapter::pixel_format(cv::Mat(6, 5, 24 /* CV_8UC4 */, buf, 64)) != -1) return 2;
  bool threw = false;
  try {
    (void)vo_adapter::view(cv::Mat(6, 5, CV_8UC3, buf, 64));  // without flagDoUndistortion the check stays as it is
  } catch (const std::runtime_error &) {
    threw = true;
  }
  if (!threw) return 3;
  const vo::Image im(buf, 5, 6, 64, 0, VO_PIX_RGB8);
  if (im.format != VO_PIX_RGB8 || vo::Image(buf, 5, 6, 64).format != VO_PIX_MONO8) return 4;
  std::printf("adapter image types ok\n");
  return 0;
}
'''


def test_adapter_accepts_the_nodes_image_types(tmp_path, vo):
    src, exe = tmp_path / "adapter_node_io.cpp", str(tmp_path / "adapter_node_io")
    src.write_text(ADAPTER_SRC)
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", ROOT, "-I", os.path.join(STUBS, "thirdparty"), "-I",
                           os.path.join(STUBS, "reference"), "-O1", str(src), "-o", exe, "-L", LIBDIR, "-lvo_hip", f"-Wl,-rpath,{LIBDIR}"])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "adapter image types ok" in r.stdout, (r.returncode, r.stdout + r.stderr)


# ---- kernel resources ----------------------------------------------------------------------------------------------
def test_render_kernels_fit_next_to_a_frame_in_flight():
    """the side-chain budget of tests/test_kernel_resources.py (same compile, same rule) for the two render kernels and for every
    instantiation of the remap: no scratch, no spills, registers (in units of 8) x lanes / 256 <= 236"""
    from visual_odometry_ros_amd import build as B
    import test_kernel_resources as K
    if not os.path.exists(B.HIPCC):
        pytest.skip("no hipcc")
    for src, kernels, n_hits in (("draw.hip", (("draw_cover_kernel", 256), ("draw_resolve_kernel", 256)), 1),
                                 ("pyramid.hip", (("remap_level0_kernel", 256),), 6)):
        res = K._usage(src)
        for k, lanes in kernels:
            hit = [v for n, v in res.items() if k in n]
            assert len(hit) == n_hits, (src, k, sorted(res))
            for v in hit:
                per_simd = (lanes // 256) * ((v["VGPRs"] + 7) // 8 * 8)
                print(src, k, v)
                assert per_simd <= 236 and v["ScratchSize [bytes/lane]"] == 0 and v["VGPRs Spill"] == 0, (src, k, lanes, v)
