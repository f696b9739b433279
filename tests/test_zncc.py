"""calcZNCC and the ZNCC gate, host side (no GPU): the new C symbols, argument errors that need no device, the restatement's own
properties, the Python argument forms, the C++ mirrors' setZnccGate against the type-check stand-ins and the examples' --zncc
options."""
import os
import subprocess
import sys

import numpy as np
import pytest

from zncc_restatement import interp, offsets, zncc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STUBS = os.path.join(ROOT, "tests", "typecheck_stubs")
NEW_SYMBOLS = ("vo_zncc", "vo_svo_set_zncc_gate", "vo_svo_get_zncc", "vo_mvo_set_zncc_gate", "vo_mvo_get_zncc")


def test_new_symbols_declared_listed_and_exported(vo):
    from visual_odometry_ros_amd import _capi
    header = open(os.path.join(ROOT, "include", "vo_hip.h")).read()
    lib = vo.load()
    for name in NEW_SYMBOLS:
        assert name in _capi.SYMBOLS and f"int {name}(" in header and hasattr(lib, name), name
    assert lib.vo_abi_version() == 3  # additions only
    for text in ("VO_ZNCC_PATTERN_REFERENCE = 0", "VO_ZNCC_PATTERN_CENTERED = 1", "VO_ZNCC_TEMPORAL = 1", "VO_ZNCC_STEREO = 2"):
        assert text in header
    for cls in (vo.StereoVO, vo.MonoVO):
        assert callable(cls.setZnccGate) and callable(cls.getZncc)
    assert callable(vo.Context.calcZNCC)
    assert vo.Context.ZNCC_PATTERNS == {"reference": 0, "centered": 1} and vo.Context.ZNCC_PAIRS == {"temporal": 1, "stereo": 2}


def test_null_handles_are_invalid(vo):
    lib = vo.load()
    out = np.zeros(4, np.float32)
    n = np.zeros(1, np.int32)
    assert lib.vo_zncc(None, 0, 1, out.ctypes.data, out.ctypes.data, 1, 15, 0, out.ctypes.data) == -1
    assert lib.vo_svo_set_zncc_gate(None, 1, 15, 1, 0.5) == -1 and lib.vo_mvo_set_zncc_gate(None, 1, 15, 1, 0.5) == -1
    assert lib.vo_svo_get_zncc(None, None, None, 0, n.ctypes.data) == -1 and lib.vo_mvo_get_zncc(None, None, 0, n.ctypes.data) == -1


def test_gate_argument_forms():
    from visual_odometry_ros_amd.api import _zncc_gate_arg
    assert _zncc_gate_arg(None, True)[0] == 0                                    # off
    assert _zncc_gate_arg(dict(thres=0.5), True) == (1, 15, 1, 0.5)              # centred 15 x 15, temporal
    assert _zncc_gate_arg(dict(thres=0.9, win=21, pattern="reference", pairs=("temporal", "stereo")), True) == (3, 21, 0, 0.9)
    assert _zncc_gate_arg(dict(thres=0.9, pairs="stereo"), True)[0] == 2
    for bad in (dict(win=15), dict(thres=0.5, pattern="centre"), dict(thres=0.5, pairs=("flow",)), dict(thres=0.5, pairs=()),
                dict(thres=0.5, window=15), 0.5):
        with pytest.raises(ValueError):
            _zncc_gate_arg(bad, True)
    with pytest.raises(ValueError):
        _zncc_gate_arg(dict(thres=0.5, pairs=("temporal", "stereo")), False)     # MonoVO has no stereo pair


def test_restatement_properties():
    """the definition's corner cases on the restatement itself, and ZNCC's reason to be here: no change under gain and offset"""
    rng = np.random.default_rng(2)
    img = rng.integers(0, 200, (40, 50), dtype=np.uint8)
    ox, oy = offsets(3, "reference")
    assert list(zip(ox, oy))[:4] == [(-3.0, -3.0), (-3.0, -2.0), (-3.0, -1.0), (-2.0, -3.0)]  # tap k = i * win + j: i runs along x
    ox, oy = offsets(5, "centered")
    assert ox.min() == -2 and ox.max() == 2 and ox[12] == 0 and oy[12] == 0
    f = np.float32
    u = np.array([-0.5, -1.0, 0.0, 48.0, 48.999, 49.0, np.nan, 1e12, 10.0], f)
    v = np.array([5.0, 5.0, -0.25, 38.5, 5.0, 5.0, 5.0, 5.0, 39.0], f)
    got = interp(img, u, v)
    assert list(got == f(-2.0)) == [False, True, False, False, False, True, True, True, True]
    # u in (-1, 0): u0 = 0 and ax = -0.5 — an extrapolation, as the text does
    I1, I2 = f(img[5, 0]), f(img[5, 1])
    assert got[0] == f(f(f(-0.5) * f(-I1 + I2)) + I1)
    p = np.array([[25.3, 20.6], [30.0, 23.0]], f)  # (both patterns' patches lie inside the image)
    for pattern in ("reference", "centered"):
        for order in ("tree", "reference"):
            same = zncc(img, img, p, p, 15, pattern, order)
            assert np.allclose(same, 1.0, atol=1e-5)
            gain = (img.astype(np.int32) // 2 + 30).astype(np.uint8)  # (a rounded gain: close to 1, not equal)
            assert (zncc(img, gain, p, p, 15, pattern, order) > 0.99).all()
            assert (np.abs(zncc(img, img, p, p + f(7.0), 15, pattern, order)) < 0.5).all()  # another patch of noise
            assert (zncc(img, (255 - img), p, p, 15, pattern, order) < -0.99).all()
    flat = np.full((40, 50), 9, np.uint8)
    assert np.isnan(zncc(flat, img, p, p, 15, "centered")).all()
    # the two orders are different roundings of the same sums
    a, b = zncc(img, gain, p, p + f(0.3), 31, "centered", "tree"), zncc(img, gain, p, p + f(0.3), 31, "centered", "reference")
    assert np.allclose(a, b, atol=1e-4)


def test_adapters_set_zncc_gate_type_checks():
    src = os.path.join(ROOT, "tests", "cpp", "zncc_typecheck.cpp")
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", ROOT, "-I", os.path.join(STUBS, "thirdparty"),
                        "-I", os.path.join(STUBS, "reference"), "-fsyntax-only", src], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]


@pytest.mark.parametrize("example,base", [("run_stereo_sequence", ["--config", "c.yaml", "--left", "l", "--right", "r"]),
                                          ("run_mono_sequence", ["--config", "c.yaml", "--images", "i"])])
def test_examples_zncc_options(example, base):
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    try:
        ex = __import__(example)
    finally:
        sys.path.pop(0)
    from visual_odometry_ros_amd.api import _zncc_gate_arg
    stereo = example == "run_stereo_sequence"
    assert ex.zncc_options(ex.parse_args(base)) == {}
    got = ex.zncc_options(ex.parse_args(base + ["--zncc", "0.8"]))
    assert got == {"zncc_gate": {"thres": 0.8, "win": 15, "pattern": "centered", "pairs": ("temporal",)}}
    assert _zncc_gate_arg(got["zncc_gate"], stereo) == (1, 15, 1, 0.8)
    got = ex.zncc_options(ex.parse_args(base + ["--zncc", "0.5", "--zncc-win", "21"]))
    assert got["zncc_gate"]["win"] == 21
    if stereo:
        got = ex.zncc_options(ex.parse_args(base + ["--zncc", "0.9", "--zncc-stereo"]))
        assert got["zncc_gate"]["pairs"] == ("temporal", "stereo") and _zncc_gate_arg(got["zncc_gate"], True)[0] == 3
        with pytest.raises(SystemExit):
            ex.zncc_options(ex.parse_args(base + ["--zncc-stereo"]))
    else:
        with pytest.raises(SystemExit):
            ex.parse_args(base + ["--zncc", "0.9", "--zncc-stereo"])  # (no such option on the mono example)
    for bad in (["--zncc-win", "15"], ["--zncc", "0.5", "--zncc-win", "16"], ["--zncc", "0.5", "--zncc-win", "33"], ["--zncc", "nan"]):
        with pytest.raises(SystemExit):
            ex.zncc_options(ex.parse_args(base + bad))
