"""The C++ mirror of the world map's dense-fed sources (setSemiDenseWorldMerge, getSemiDenseWorldSource in stereo_vo.h and
reference_adapter.h) and the merge operator's C interface type-check against the stand-in headers, and the sequence example's
--semidense-world-source options turn into the `semidense` argument as documented. No GPU."""
import os
import subprocess
import sys

import pytest

from test_zncc import ROOT, STUBS


def test_adapter_semidense_map_merge_type_checks():
    src = os.path.join(ROOT, "tests", "cpp", "semidense_map_merge_typecheck.cpp")
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", ROOT, "-I", os.path.join(STUBS, "thirdparty"),
                        "-I", os.path.join(STUBS, "reference"), "-fsyntax-only", src], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]


def test_example_world_source_options():
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    try:
        import run_stereo_sequence as ex
    finally:
        sys.path.pop(0)
    base = ["--config", "c.yaml", "--left", "l", "--right", "r", "--semidense", "out", "--semidense-temporal", "--semidense-world", "w.ply"]
    world = lambda extra: ex.semidense_options(ex.parse_args(base + extra))["semidense"]["world"]
    assert world([]) is True  # (as before)
    assert world(["--semidense-world-source", "raw"]) == {"source": "raw"}
    assert world(["--dense", "d", "--semidense-world-source", "dense"]) == {"source": "dense"}
    assert world(["--dense", "d", "--semidense-world-source", "merged", "--semidense-voxel", "0.2"]) == {"voxel": 0.2, "source": "merged"}
    got = world(["--dense", "d", "--semidense-world-source", "merged", "--semidense-world-merge-chi", "2.5", "--semidense-world-keep-obs", "3"])
    assert got == {"source": "merged", "merge": {"chi": 2.5, "keep_obs": 3}}
    assert world(["--semidense-regularize", "--semidense-world-source", "regularized"]) == {"source": "regularized"}
    for bad in (["--semidense-world-source", "dense"], ["--semidense-world-source", "merged"],  # need --dense, and the script says so
                ["--semidense-world-source", "regularized"], ["--semidense-world-merge-chi", "2"],
                ["--semidense-world-source", "raw", "--semidense-world-keep-obs", "2"],
                ["--dense", "d", "--semidense-world-source", "merged", "--semidense-world-merge-chi", "0"],
                ["--dense", "d", "--semidense-world-source", "merged", "--semidense-world-merge-chi", "nan"],
                ["--dense", "d", "--semidense-world-source", "merged", "--semidense-world-keep-obs", "257"]):
        with pytest.raises(SystemExit) as e:
            ex.semidense_options(ex.parse_args(base + bad))
        if bad[-1] in ("dense", "merged"):
            assert "--dense" in str(e.value)
    with pytest.raises(SystemExit):  # without the world map
        ex.semidense_options(ex.parse_args(base[:9] + ["--semidense-world-source", "raw"]))
