"""The ignore mask's host side (no GPU): the lookup's rounding and out-of-range rule, the new C symbols, the C++ mirrors'
setMask against the type-check stand-ins, the examples' --mask options and the PGM reader behind them."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STUBS = os.path.join(ROOT, "tests", "typecheck_stubs")
NEW_SYMBOLS = ("vo_set_slot_mask", "vo_slot_image_size", "vo_svo_set_mask", "vo_mvo_set_mask", "vo_rectify_validity_mask")


def test_lookup_rounding_and_range():
    """mask[(int)(y + 0.5f)][(int)(x + 0.5f)]: halves round up, the cast truncates toward zero (so (-1.5, -0.5) reads index 0, as
    the reference's expression does), everything else outside the plane and NaN read as 0."""
    from visual_odometry_ros_amd.api import mask_lookup
    from mask_ref import lookup
    m = np.zeros((4, 6), np.uint8)
    m[1, 2] = 7          # any non-zero value is "usable"
    m[0, 0] = m[3, 5] = 255
    cases = [((2.0, 1.0), True), ((1.5, 0.5), True), ((2.49, 1.49), True), ((2.5, 1.0), False), ((2.0, 1.5), False),
             ((1.49, 1.0), False), ((0.0, 0.0), True), ((-0.5, -0.5), True), ((-1.4, 0.0), True), ((-1.5, 0.0), False),
             ((0.0, -1.5), False), ((5.49, 3.49), True), ((5.5, 3.0), False), ((5.0, 3.5), False), ((6.0, 3.0), False),
             ((np.nan, 1.0), False), ((2.0, np.nan), False), ((np.inf, 1.0), False), ((-np.inf, 1.0), False), ((1e12, 1e12), False)]
    pts = np.array([c[0] for c in cases], np.float32)
    want = np.array([c[1] for c in cases])
    assert np.array_equal(lookup(m, pts), want)
    assert np.array_equal(mask_lookup(m, pts[:, 0], pts[:, 1]), want)
    assert bool(mask_lookup(m, 2.0, 1.0)) and not bool(mask_lookup(m, 3.0, 1.0))
    # float32 rounding of the sum: 2.4999999 + 0.5f is 3.0f in float32 (ties to even), so the pixel is column 3
    x = np.float32(2.4999999)
    assert x + np.float32(0.5) == np.float32(3.0) and not bool(mask_lookup(m, x, 1.0))
    rng = np.random.default_rng(0)
    big = (rng.random((50, 70)) < 0.5).astype(np.uint8)
    p = np.stack([rng.uniform(-3, 73, 4000), rng.uniform(-3, 53, 4000)], 1).astype(np.float32)
    assert np.array_equal(mask_lookup(big, p[:, 0], p[:, 1]), lookup(big, p))


def test_new_symbols_declared_listed_and_exported(vo):
    from visual_odometry_ros_amd import _capi
    header = open(os.path.join(ROOT, "include", "vo_hip.h")).read()
    lib = vo.load()
    for name in NEW_SYMBOLS:
        assert name in _capi.SYMBOLS and f"int {name}(" in header and hasattr(lib, name), name
    assert lib.vo_abi_version() == 3  # additions only
    for cls in (vo.StereoVO, vo.MonoVO):
        assert callable(cls.setMask)
    assert callable(vo.Context.set_slot_mask) and callable(vo.StereoCamera.validityMask) and callable(vo.Camera.validityMask)


def test_mask_argument_forms():
    from visual_odometry_ros_amd.api import _mask_arg
    m = np.zeros((5, 8), np.uint8)
    keep, ptr, stride, dev = _mask_arg(m, 8, 5)
    assert ptr == m.ctypes.data and stride == 8 and dev == 0
    wide = np.zeros((5, 12), np.uint8)[:, :8]                      # padded rows are passed as they are
    assert _mask_arg(wide, 8, 5)[1:] == (wide.ctypes.data, 12, 0)
    keep, ptr, stride, dev = _mask_arg(np.ones((5, 8), bool), 8, 5)  # bool: True = usable
    assert keep.dtype == np.uint8 and keep.min() == 255
    assert _mask_arg((0x7F0000001000, 64), 8, 5)[1:] == (0x7F0000001000, 64, 1)  # (device address, stride)
    assert _mask_arg(None, 8, 5) == (None, None, 0, 0)
    from visual_odometry_ros_amd import VoError
    for bad in (np.zeros((5, 7), np.uint8), np.zeros((6, 8), np.uint8), np.zeros((5, 8), np.float32), np.zeros((5, 8, 1), np.uint8)):
        with pytest.raises(VoError) as e:
            _mask_arg(bad, 8, 5)
        assert e.value.code == -1  # VO_ERR_INVALID


def test_adapters_set_mask_type_checks():
    src = os.path.join(ROOT, "tests", "cpp", "mask_typecheck.cpp")
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", ROOT, "-I", os.path.join(STUBS, "thirdparty"),
                        "-I", os.path.join(STUBS, "reference"), "-fsyntax-only", src], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]


@pytest.mark.parametrize("example,base", [("run_stereo_sequence", ["--config", "c.yaml", "--left", "l", "--right", "r"]),
                                          ("run_mono_sequence", ["--config", "c.yaml", "--images", "i"])])
def test_examples_mask_options(tmp_path, example, base):
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    try:
        ex = __import__(example)
    finally:
        sys.path.pop(0)
    assert ex.mask_options(ex.parse_args(base)) == {}
    assert ex.mask_options(ex.parse_args(base + ["--mask-rectified"])) == {"mask": "rectified", "mask_erode": 0}
    assert ex.mask_options(ex.parse_args(base + ["--mask-rectified", "7"])) == {"mask": "rectified", "mask_erode": 7}
    m = (np.arange(6 * 9).reshape(6, 9) % 3 == 0).astype(np.uint8) * 255
    path = tmp_path / "mask.pgm"
    path.write_bytes(b"P5\n# a comment\n9 6\n255\n" + m.tobytes())
    got = ex.mask_options(ex.parse_args(base + ["--mask", str(path)]))
    assert list(got) == ["mask"] and got["mask"].dtype == np.uint8 and np.array_equal(got["mask"], m)
    for bad in (["--mask", str(path), "--mask-rectified"], ["--mask-rectified", "32"]):
        with pytest.raises(SystemExit):
            ex.mask_options(ex.parse_args(base + bad))
    (tmp_path / "short.pgm").write_bytes(b"P5 9 6 255\n" + m.tobytes()[:-1])
    (tmp_path / "ascii.pgm").write_bytes(b"P2 1 1 255\n0\n")
    for name in ("short.pgm", "ascii.pgm"):
        with pytest.raises(ValueError):
            ex.mask_options(ex.parse_args(base + ["--mask", str(tmp_path / name)]))


def test_from_yaml_rectified_mask_needs_undistortion():
    """mask="rectified" is an error for a file without flagDoUndistortion — found before any device is touched"""
    import visual_odometry_ros_amd as V
    cfg = os.path.join(ROOT, "tests", "golden", "reference_config")
    with pytest.raises(ValueError):
        V.StereoVO.from_yaml(os.path.join(cfg, "stereo", "kitti_00_stereo.yaml"), mask="rectified")
    with pytest.raises(ValueError):
        V.MonoVO.from_yaml(os.path.join(cfg, "mono", "kitti_00.yaml"), mask="rectified", mask_erode=2)
    with pytest.raises(ValueError):
        V.StereoVO.from_yaml(os.path.join(cfg, "stereo", "exp_stereo.yaml"), mask="bonnet")
