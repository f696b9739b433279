"""The C++ side of the world map (setSemiDenseWorld / flushSemiDenseWorld / getSemiDenseWorldPoints on vo::StereoVO and the
reference-typed adapter) type-checks against the stand-in headers; a small C program links against the library and runs through the
C ABI what needs no device; the sequence example's options. No GPU."""
import os
import subprocess
import sys

import pytest

from test_zncc import ROOT, STUBS


def test_adapter_semidense_world_type_checks():
    src = os.path.join(ROOT, "tests", "cpp", "semidense_world_typecheck.cpp")
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", ROOT, "-I", os.path.join(STUBS, "thirdparty"),
                        "-I", os.path.join(STUBS, "reference"), "-fsyntax-only", src], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]


def test_c_program_links_and_runs_through_the_abi(tmp_path):
    libdir = os.path.join(ROOT, "visual_odometry_ros_amd", "lib")
    if not os.path.exists(os.path.join(libdir, "libvo_hip.so")):
        pytest.skip("libvo_hip.so is not built")
    exe = str(tmp_path / "semidense_world_abi")
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Wextra", "-Werror", "-I", ROOT, os.path.join(ROOT, "tests", "cpp", "semidense_world_abi.c"),
                           "-o", exe, "-L", libdir, "-lvo_hip", f"-Wl,-rpath,{libdir}", "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib", "-lamdhip64"])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "semidense world abi ok" in r.stdout, (r.returncode, r.stdout, r.stderr)


def test_example_semidense_world_options():
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    try:
        import run_stereo_sequence as ex
    finally:
        sys.path.pop(0)
    base = ["--config", "c.yaml", "--left", "l", "--right", "r"]
    got = ex.semidense_options(ex.parse_args(base + ["--semidense", "out", "--semidense-temporal", "--semidense-world", "map.ply"]))
    assert got == {"semidense": {"z_min": 3.0, "every": "keyframe", "temporal": True, "world": True}}
    args = ex.parse_args(base + ["--semidense", "out", "--semidense-temporal", "--semidense-world", "map.ply", "--semidense-voxel", "0.2",
                                 "--semidense-world-min-keyframes", "2"])
    assert ex.semidense_options(args) == {"semidense": {"z_min": 3.0, "every": "keyframe", "temporal": True, "world": {"voxel": 0.2}}}
    assert args.semidense_world_min_keyframes == 2
    got = ex.semidense_options(ex.parse_args(base + ["--semidense", "out", "--semidense-temporal"]))
    assert got == {"semidense": {"z_min": 3.0, "every": "keyframe", "temporal": True}}
    for bad in (["--semidense-world", "m.ply"], ["--semidense", "o", "--semidense-world", "m.ply"],
                ["--semidense", "o", "--semidense-temporal", "--semidense-voxel", "0.2"],
                ["--semidense", "o", "--semidense-temporal", "--semidense-world", "m.ply", "--semidense-voxel", "0"],
                ["--semidense", "o", "--semidense-temporal", "--semidense-world", "m.ply", "--semidense-world-min-keyframes", "0"]):
        with pytest.raises(SystemExit):
            ex.semidense_options(ex.parse_args(base + bad))


def test_example_writes_a_world_ply(tmp_path):
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    try:
        import run_stereo_sequence as ex
    finally:
        sys.path.pop(0)
    import numpy as np
    import visual_odometry_ros_amd as V
    w = V.SemiDenseWorldPoints(np.zeros((2, 3), np.int32), np.array([[0.05, -1.5, 3.25], [1, 2, 3]], np.float32), np.array([7, 9], np.uint32),
                               np.array([3, 1], np.uint32), np.array([2, 1], np.uint32), np.array([200, 17], np.uint8))
    path = tmp_path / "map.ply"
    ex.write_world_ply(str(path), w)
    lines = path.read_text().splitlines()
    assert lines[2] == "element vertex 2" and lines[-2:] == ["0.05 -1.5 3.25 200 3 2", "1 2 3 17 1 1"]
    assert [ln.split()[-1] for ln in lines[3:9]] == ["x", "y", "z", "grey", "count", "keyframes"]
