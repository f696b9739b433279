"""The C++ side of the semi-dense regularisation (setSemiDenseRegularize / getSemiDenseRegularizedPoints on vo::StereoVO and the
reference-typed adapter) type-checks against the stand-in headers; the sequence example's option. No GPU."""
import os
import subprocess
import sys

import pytest

from test_zncc import ROOT, STUBS


def test_adapter_semidense_regularize_type_checks():
    src = os.path.join(ROOT, "tests", "cpp", "semidense_regularize_typecheck.cpp")
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", ROOT, "-I", os.path.join(STUBS, "thirdparty"),
                        "-I", os.path.join(STUBS, "reference"), "-fsyntax-only", src], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]


def test_example_semidense_regularize_option():
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    try:
        import run_stereo_sequence as ex
    finally:
        sys.path.pop(0)
    base = ["--config", "c.yaml", "--left", "l", "--right", "r"]
    got = ex.semidense_options(ex.parse_args(base + ["--semidense", "out", "--semidense-temporal", "--semidense-regularize"]))
    assert got == {"semidense": {"z_min": 3.0, "every": "keyframe", "temporal": True, "regularize": True}}
    got = ex.semidense_options(ex.parse_args(base + ["--semidense", "out", "--semidense-temporal", "--semidense-propagate",
                                                     "--semidense-regularize"]))
    assert got == {"semidense": {"z_min": 3.0, "every": "keyframe", "temporal": True, "propagate": True, "regularize": True}}
    got = ex.semidense_options(ex.parse_args(base + ["--semidense", "out", "--semidense-temporal"]))
    assert got == {"semidense": {"z_min": 3.0, "every": "keyframe", "temporal": True}}
    for bad in (["--semidense-regularize"], ["--semidense", "o", "--semidense-regularize"],
                ["--semidense-temporal", "--semidense-regularize"]):
        with pytest.raises(SystemExit):
            ex.semidense_options(ex.parse_args(base + bad))
