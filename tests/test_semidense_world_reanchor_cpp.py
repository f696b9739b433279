"""The C++ side of the world map's re-anchoring (setSemiDenseWorldReanchor / getSemiDenseWorldAnchors / getSemiDenseWorldReanchorStats
on vo::StereoVO and the reference-typed adapter, the operator's C calls) type-checks against the stand-in headers; the sequence
example's option. No GPU."""
import os
import subprocess
import sys

import pytest

from test_zncc import ROOT, STUBS


def test_adapter_semidense_world_reanchor_type_checks():
    src = os.path.join(ROOT, "tests", "cpp", "semidense_world_reanchor_typecheck.cpp")
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", ROOT, "-I", os.path.join(STUBS, "thirdparty"),
                        "-I", os.path.join(STUBS, "reference"), "-fsyntax-only", src], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]


def test_example_semidense_world_reanchor_option():
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    try:
        import run_stereo_sequence as ex
    finally:
        sys.path.pop(0)
    base = ["--config", "c.yaml", "--left", "l", "--right", "r", "--semidense", "out", "--semidense-temporal", "--semidense-world", "map.ply"]
    opt = lambda *a: ex.semidense_options(ex.parse_args(base + list(a)))["semidense"]["world"]  # noqa: E731
    assert opt() is True
    assert opt("--semidense-world-reanchor") == {"reanchor": True}
    assert opt("--semidense-world-reanchor", "0.5") == {"reanchor": {"min_move": 0.5}}
    assert opt("--semidense-voxel", "0.2", "--semidense-world-reanchor", "0.25") == {"voxel": 0.2, "reanchor": {"min_move": 0.25}}
    for bad in (base[:6] + ["--semidense-world-reanchor"], base[:8] + ["--semidense-world-reanchor"], base + ["--semidense-world-reanchor", "-1"]):
        with pytest.raises(SystemExit):
            ex.semidense_options(ex.parse_args(bad))
