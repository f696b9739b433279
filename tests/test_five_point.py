"""CPU checks of the 5-point RANSAC pose's surroundings: the mono configuration files of the reference read by the Python reader
(config.load_mono_config) and by the C++ reader (mono_vo_config.h: vo::loadMonoVOParams) alike, and the new kernels' resources
(no scratch memory, no VGPR spills) from a gfx950 cross-compile."""
import glob
import os
import subprocess

import numpy as np
import pytest

from visual_odometry_ros_amd import build as B
from visual_odometry_ros_amd import config

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MONO_YAML = os.path.join(ROOT, "tests", "golden", "reference_config", "mono")

READER = r'''
#include <cstdio>
#include "visual_odometry_ros_amd/core/visual_odometry/mono_vo_config.h"
int main(int argc, char **argv) {
  try {
    const vo::MonoVOParams p = vo::loadMonoVOParams(argv[1]);
    printf("width %d\nheight %d\nflagDoUndistortion %d\n", p.width, p.height, (int)p.flagDoUndistortion);
    for (int k = 0; k < 4; ++k) printf("K%d %.9g\n", k, p.K[k]);
    for (int k = 0; k < 5; ++k) printf("D%d %.9g\n", k, p.D[k]);
    printf("thres_error %.9g\nthres_bidirection %.9g\nthres_sampson %.9g\nwindow_size %d\nmax_level %d\n", p.feature_tracker.thres_error,
           p.feature_tracker.thres_bidirection, p.feature_tracker.thres_sampson, p.feature_tracker.window_size, p.feature_tracker.max_level);
    printf("n_features %d\nn_bins_u %d\nn_bins_v %d\nthres_fastscore %.9g\nradius %.9g\n", p.feature_extractor.n_features,
           p.feature_extractor.n_bins_u, p.feature_extractor.n_bins_v, p.feature_extractor.thres_fastscore, p.feature_extractor.radius);
    printf("thres_1p_error %.9g\nthres_5p_error %.9g\nthres_poseba_error %.9g\n", p.motion_estimator.thres_1p_error,
           p.motion_estimator.thres_5p_error, p.motion_estimator.thres_poseba_error);
    printf("thres_translation %.9g\nthres_rotation %.9g\nthres_overlap_ratio %.9g\nn_max_keyframes_in_window %d\n",
           p.keyframe_update.thres_translation, p.keyframe_update.thres_rotation, p.keyframe_update.thres_overlap_ratio,
           p.keyframe_update.n_max_keyframes_in_window);
    printf("thres_parallax %.9g\n", p.map_update.thres_parallax);
  } catch (const std::exception &e) {
    printf("error %s\n", e.what());
    return 2;
  }
  return 0;
}
'''


def _files():
    return sorted(glob.glob(os.path.join(MONO_YAML, "*.yaml")))


def test_every_mono_fixture_is_read():
    fs = _files()
    assert len(fs) == 14
    for f in fs:
        c = config.load_mono_config(f)
        assert c["camera"]["width"] > 0 and c["camera"]["height"] > 0 and c["camera"]["K"][0] > 0, f
        assert c["feature_tracker"]["window_size"] in (13, 15, 21, 31), f
    k = config.load_mono_config(os.path.join(MONO_YAML, "kitti_00.yaml"))
    assert (k["camera"]["width"], k["camera"]["height"]) == (1241, 376)
    assert k["camera"]["K"][0] == np.float32(718.856)
    assert (k["feature_tracker"]["window_size"], k["feature_tracker"]["max_level"]) == (21, 6)
    assert (k["feature_extractor"]["n_bins_u"], k["feature_extractor"]["n_bins_v"]) == (30, 12)
    assert k["motion_estimator"]["thres_5p_error"] == 1.0 and k["flagDoUndistortion"] == 0 and not k["missing"]
    m = config.load_mono_config(os.path.join(MONO_YAML, "mono0.yaml"))
    assert (m["camera"]["width"], m["camera"]["height"]) == (752, 480) and m["flagDoUndistortion"] == 1
    assert "motion_estimator.thres_5p_error" in m["missing"] and m["motion_estimator"]["thres_5p_error"] == 0.0


def test_cpp_reader_agrees_with_the_python_reader(tmp_path):
    assert len(_files()) == 14
    libdir = os.path.join(ROOT, "visual_odometry_ros_amd", "lib")
    src, exe = tmp_path / "reader.cpp", str(tmp_path / "reader")
    src.write_text(READER)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I", ROOT, str(src), "-o", exe, "-L", libdir, "-lvo_hip", f"-Wl,-rpath,{libdir}",
                           "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib", "-lamdhip64"])
    for f in _files():
        r = subprocess.run([exe, f], capture_output=True, text=True)
        assert r.returncode == 0, (f, r.stdout)
        got = dict(line.split(" ", 1) for line in r.stdout.strip().splitlines())
        c = config.load_mono_config(f)
        want = {"width": c["camera"]["width"], "height": c["camera"]["height"], "flagDoUndistortion": c["flagDoUndistortion"]}
        for k in range(4):
            want[f"K{k}"] = c["camera"]["K"][k]
        for k in range(5):
            want[f"D{k}"] = c["camera"]["D"][k]
        for sec in ("feature_tracker", "feature_extractor", "motion_estimator", "keyframe_update", "map_update"):
            want.update(c[sec])
        assert set(got) == set(want), f
        for k, v in want.items():
            assert np.float32(float(got[k])) == np.float32(v), (f, k, got[k], v)


@pytest.mark.skipif(not os.path.exists(B.HIPCC), reason="no hipcc")
def test_five_point_kernels_use_no_scratch_memory():
    import re
    flags = [f for f in B.FLAGS if f not in ("-Wall", "-Wno-unused-function")]
    cmd = [B.HIPCC] + flags + ["-I" + os.path.join(ROOT, "include"), "-I" + B.CSRC, "--offload-device-only",
                               "-Rpass-analysis=kernel-resource-usage", "-c", os.path.join(B.CSRC, "five_point.hip"), "-o", os.devnull]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    out, name = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            out[name] = {}
        for key in ("ScratchSize [bytes/lane]", "VGPRs Spill"):
            m = re.search(re.escape(key) + r": (\d+)", line)
            if m and name:
                out[name].setdefault(key, int(m.group(1)))
    for k in ("ep5_solve_kernel", "ep5_score_kernel", "ep5_select_kernel"):
        hit = [v for n, v in out.items() if k in n]
        assert hit, (k, sorted(out))
        for v in hit:
            assert v["ScratchSize [bytes/lane]"] == 0 and v["VGPRs Spill"] == 0, (k, v)
