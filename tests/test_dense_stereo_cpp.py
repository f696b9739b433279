"""The C++ side of the dense stereo option (setDenseStereo / getDensePoints on vo::StereoVO and the reference-typed adapter)
type-checks against the stand-in headers; the sequence example's options, next to the semi-dense ones, which are unchanged. No GPU."""
import os
import subprocess
import sys

import pytest

from test_zncc import ROOT, STUBS


def test_adapter_dense_stereo_type_checks():
    src = os.path.join(ROOT, "tests", "cpp", "dense_stereo_typecheck.cpp")
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", ROOT, "-I", os.path.join(STUBS, "thirdparty"),
                        "-I", os.path.join(STUBS, "reference"), "-fsyntax-only", src], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]


def test_example_dense_options():
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    try:
        import run_stereo_sequence as ex
    finally:
        sys.path.pop(0)
    base = ["--config", "c.yaml", "--left", "l", "--right", "r"]
    assert ex.dense_options(ex.parse_args(base)) == {}
    assert ex.dense_options(ex.parse_args(base + ["--dense", "out"])) == {"dense": {"z_min": 3.0, "n_disp": 128, "every": "keyframe"}}
    got = ex.dense_options(ex.parse_args(base + ["--dense", "out", "--dense-every", "frame", "--dense-disparities", "150", "--dense-paths", "4"]))
    assert got == {"dense": {"z_min": 3.0, "n_disp": 150, "every": "frame", "paths": 4}}
    from visual_odometry_ros_amd import api, load
    p = api._dense_stereo_params(load(), {k: v for k, v in dict(got["dense"], bf=386.1).items() if k != "every"})
    assert (p.d_min, p.n_disp, p.paths) == (0, 192, 4)  # (d_max = 129: the range 0..191 holds it)
    p = api._dense_stereo_params(load(), dict(bf=386.1, z_min=3.0, n_disp=64))
    assert (p.d_min, p.n_disp) == (66, 64)
    for bad in (["--dense-every", "frame"], ["--dense-disparities", "64"], ["--dense-paths", "4"], ["--dense", "o", "--dense-disparities", "0"],
                ["--dense", "o", "--dense-disparities", "257"]):
        with pytest.raises(SystemExit):
            ex.dense_options(ex.parse_args(base + bad))
    with pytest.raises(SystemExit):
        ex.parse_args(base + ["--dense", "o", "--dense-paths", "6"])
    # the semi-dense options are what they were, with and without --dense
    for extra in ([], ["--dense", "out", "--dense-every", "frame"]):
        assert ex.semidense_options(ex.parse_args(base + extra)) == {}
        assert ex.semidense_options(ex.parse_args(base + extra + ["--semidense", "out"])) == {"semidense": {"z_min": 3.0, "every": "keyframe"}}
        got = ex.semidense_options(ex.parse_args(base + extra + ["--semidense", "out", "--semidense-every", "frame", "--semidense-depth", "2", "40"]))
        assert got == {"semidense": {"z_min": 2.0, "z_max": 40.0, "every": "frame"}}
