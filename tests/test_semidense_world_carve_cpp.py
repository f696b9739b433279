"""The C++ side of the world map's free-space carving (setSemiDenseWorldCarve / getSemiDenseWorldFree / getSemiDenseWorldCarveStats on
vo::StereoVO and the reference-typed adapter, the operator's C calls) type-checks against the stand-in headers; the C header still
reads as C; the sequence example's options. No GPU."""
import os
import subprocess
import sys

import pytest

from test_zncc import ROOT, STUBS


def test_adapter_semidense_world_carve_type_checks():
    src = os.path.join(ROOT, "tests", "cpp", "semidense_world_carve_typecheck.cpp")
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", ROOT, "-I", os.path.join(STUBS, "thirdparty"),
                        "-I", os.path.join(STUBS, "reference"), "-fsyntax-only", src], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]


def test_the_header_reads_as_c(tmp_path):
    src = tmp_path / "carve_abi.c"
    src.write_text('#include <stdlib.h>\n#include "include/vo_hip.h"\n'
                   "int f(vo_semidense_world *wm, vo_semidense_world_carve_info *i) { return vo_semidense_world_carve_stats(wm, i); }\n"
                   "_Static_assert(sizeof(vo_semidense_world_carve_params) == 12, \"three floats\");\n"
                   "_Static_assert(sizeof(vo_semidense_world_carve_info) == 40, \"five 64-bit counts\");\n")
    r = subprocess.run(["gcc", "-std=c11", "-Wall", "-Wextra", "-Werror", "-Wshadow", "-I", ROOT, "-fsyntax-only", str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]


def test_example_semidense_world_carve_options():
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    try:
        import run_stereo_sequence as ex
    finally:
        sys.path.pop(0)
    base = ["--config", "c.yaml", "--left", "l", "--right", "r", "--semidense", "out", "--semidense-temporal", "--semidense-world", "map.ply"]
    args = lambda *a: ex.parse_args(base + list(a))  # noqa: E731
    opt = lambda *a: ex.semidense_options(args(*a))["semidense"]["world"]  # noqa: E731
    assert opt() is True  # without the flag: what it was
    assert opt("--semidense-world-carve") == {"carve": {"margin": 2.0}}
    assert opt("--semidense-world-carve", "3.5") == {"carve": {"margin": 3.5}}
    assert opt("--semidense-voxel", "0.2", "--semidense-world-reanchor", "--semidense-world-carve") == {"voxel": 0.2, "reanchor": True, "carve": {"margin": 2.0}}
    assert args("--semidense-world-carve", "--semidense-world-max-free", "1", "2").semidense_world_max_free == [1, 2]
    for bad in (base[:6] + ["--semidense-world-carve"], base[:8] + ["--semidense-world-carve"], base + ["--semidense-world-carve", "0.5"],
                base + ["--semidense-world-max-free", "1", "2"], base + ["--semidense-world-carve", "--semidense-world-max-free", "-1", "2"]):
        with pytest.raises(SystemExit):
            ex.semidense_options(ex.parse_args(bad))
