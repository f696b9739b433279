"""The C++ side of the speckle option (setDenseSpeckle / getDenseSpeckleStats on vo::StereoVO, setDenseSpeckle on the reference-typed
adapter) and the operator's C interface type-check against the stand-in headers; the sequence example's options. No GPU."""
import os
import subprocess
import sys

import pytest

from test_zncc import ROOT, STUBS


def test_adapter_dense_speckle_type_checks():
    src = os.path.join(ROOT, "tests", "cpp", "dense_speckle_typecheck.cpp")
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", ROOT, "-I", os.path.join(STUBS, "thirdparty"),
                        "-I", os.path.join(STUBS, "reference"), "-fsyntax-only", src], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]


def test_example_dense_speckle_options():
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    try:
        import run_stereo_sequence as ex
    finally:
        sys.path.pop(0)
    base = ["--config", "c.yaml", "--left", "l", "--right", "r"]
    plain = {"z_min": 3.0, "n_disp": 128, "every": "keyframe"}
    assert ex.dense_options(ex.parse_args(base + ["--dense", "out"])) == {"dense": plain}  # (as before)
    assert ex.dense_options(ex.parse_args(base + ["--dense", "out", "--dense-speckle"])) == {"dense": dict(plain, speckle={"max_size": 100})}
    assert ex.dense_options(ex.parse_args(base + ["--dense", "out", "--dense-speckle", "40"])) == {"dense": dict(plain, speckle={"max_size": 40})}
    got = ex.dense_options(ex.parse_args(base + ["--dense", "out", "--dense-speckle", "0", "--dense-speckle-diff", "2.5"]))
    assert got == {"dense": dict(plain, speckle={"max_size": 0, "max_diff": 2.5})}
    for bad in (["--dense-speckle"], ["--dense-speckle-diff", "2"], ["--dense", "o", "--dense-speckle-diff", "2"],
                ["--dense", "o", "--dense-speckle", "-1"], ["--dense", "o", "--dense-speckle", "--dense-speckle-diff", "-0.5"],
                ["--dense", "o", "--dense-speckle", "--dense-speckle-diff", "inf"], ["--dense", "o", "--dense-speckle", "--dense-speckle-diff", "nan"]):
        with pytest.raises(SystemExit):
            ex.dense_options(ex.parse_args(base + bad))
