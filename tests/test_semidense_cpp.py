"""The C++ side of the semi-dense stereo option (setSemiDense / getSemiDensePoints on vo::StereoVO and the reference-typed
adapter) type-checks against the stand-in headers; the sequence example's options. No GPU."""
import os
import subprocess
import sys

import numpy as np
import pytest

from test_zncc import ROOT, STUBS


def test_adapter_semidense_type_checks():
    src = os.path.join(ROOT, "tests", "cpp", "semidense_typecheck.cpp")
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", ROOT, "-I", os.path.join(STUBS, "thirdparty"),
                        "-I", os.path.join(STUBS, "reference"), "-fsyntax-only", src], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]


def test_example_semidense_options(tmp_path):
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    try:
        import run_stereo_sequence as ex
    finally:
        sys.path.pop(0)
    base = ["--config", "c.yaml", "--left", "l", "--right", "r"]
    assert ex.semidense_options(ex.parse_args(base)) == {}
    assert ex.semidense_options(ex.parse_args(base + ["--semidense", "out"])) == {"semidense": {"z_min": 3.0, "every": "keyframe"}}
    got = ex.semidense_options(ex.parse_args(base + ["--semidense", "out", "--semidense-every", "frame", "--semidense-depth", "2", "40"]))
    assert got == {"semidense": {"z_min": 2.0, "z_max": 40.0, "every": "frame"}}
    from visual_odometry_ros_amd import api, load
    p = api._semidense_params(load(), {k: v for k, v in dict(got["semidense"], bf=386.1).items() if k != "every"})
    assert (p.d_min, p.d_max) == (9, 194)
    for bad in (["--semidense-every", "frame"], ["--semidense-depth", "3"], ["--semidense", "o", "--semidense-depth", "0"],
                ["--semidense", "o", "--semidense-depth", "5", "3"], ["--semidense", "o", "--semidense-depth", "1", "2", "3"]):
        with pytest.raises(SystemExit):
            ex.semidense_options(ex.parse_args(base + bad))
    xyz = np.array([[1.0, 2.0, 3.5], [-0.25, 0.0, 10.0]], np.float32)
    ex.write_ply(str(tmp_path / "a.ply"), xyz, np.array([0.01, 0.002], np.float32))
    lines = (tmp_path / "a.ply").read_text().split("\n")
    assert lines[:3] == ["ply", "format ascii 1.0", "element vertex 2"] and lines[7] == "end_header"
    assert [float(v) for v in lines[8].split()] == pytest.approx([1.0, 2.0, 3.5, 0.01]) and len(lines[9].split()) == 4
