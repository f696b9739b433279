"""The C++ side of the semi-dense alignment (setSemiDenseAlign / getSemiDenseAlign on vo::StereoVO and the reference-typed adapter)
type-checks against the stand-in headers; the sequence example's option and its line format. No GPU."""
import os
import subprocess
import sys

import numpy as np
import pytest

from test_zncc import ROOT, STUBS


def test_adapter_semidense_align_type_checks():
    src = os.path.join(ROOT, "tests", "cpp", "semidense_align_typecheck.cpp")
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", ROOT, "-I", os.path.join(STUBS, "thirdparty"),
                        "-I", os.path.join(STUBS, "reference"), "-fsyntax-only", src], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]


def test_example_semidense_align_option():
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    try:
        import run_stereo_sequence as ex
    finally:
        sys.path.pop(0)
    base = ["--config", "c.yaml", "--left", "l", "--right", "r"]
    got = ex.semidense_options(ex.parse_args(base + ["--semidense", "out", "--semidense-temporal", "--semidense-align", "a.txt"]))
    assert got == {"semidense": {"z_min": 3.0, "every": "keyframe", "temporal": True, "align": True}}
    got = ex.semidense_options(ex.parse_args(base + ["--semidense", "out", "--semidense-temporal", "--semidense-propagate", "--semidense-align", "a"]))
    assert got == {"semidense": {"z_min": 3.0, "every": "keyframe", "temporal": True, "propagate": True, "align": True}}
    for bad in (["--semidense-align", "a.txt"], ["--semidense", "o", "--semidense-align", "a.txt"], ["--semidense-temporal", "--semidense-align", "a"]):
        with pytest.raises(SystemExit):
            ex.semidense_options(ex.parse_args(base + bad))
    # the line: ids, status fields, the 12 pose entries, the two distances to the odometry's pose
    from visual_odometry_ros_amd.api import SemiDenseAligned
    T = np.eye(4, dtype=np.float32)
    T[0, 3] = 0.5
    a = SemiDenseAligned(np.eye(4, dtype=np.float32), 0, 5, 1234, 4.25, np.zeros((6, 6)), np.zeros(6), T, 7, 3)
    f = ex.align_line(a, np.eye(4, dtype=np.float32)).split()
    assert len(f) == 6 + 12 + 2 and f[:6] == ["7", "3", "0", "5", "1234", "4.2500"] and float(f[9]) == 0.5
    assert float(f[18]) == 0.5 and float(f[19]) == 0.0
    none = SemiDenseAligned(np.eye(4, dtype=np.float32), 4, 0, 0, 0.0, np.zeros((6, 6)), np.zeros(6), np.eye(4, dtype=np.float32), 8, -1)
    assert ex.align_line(none, T).split()[:3] == ["8", "-1", "4"] and ex.align_line(none, T).split()[18:] == ["0.000000", "0.000000"]
