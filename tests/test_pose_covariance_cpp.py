"""The C++ mirrors of the pose covariance (core/visual_odometry/pose_covariance.h; getPoseCovariance / getPoseCovarianceRos of
motion_estimator.h, stereo_vo.h, mono_vo.h and the two adapters of reference_adapter.h): compile check on the CPU, the demo
against the Python driver on the GPU."""
import os
import struct
import subprocess

import numpy as np
import pytest

from test_cpp_mirror import ADAPTER_INC, ROOT, _compile

TYPECHECK = r"""
#include <type_traits>
#include <utility>
#include "visual_odometry_ros_amd/core/visual_odometry/motion_estimator.h"
#include "visual_odometry_ros_amd/core/visual_odometry/mono_vo.h"
#include "visual_odometry_ros_amd/core/visual_odometry/stereo_vo.h"
#include "visual_odometry_ros_amd/core/visual_odometry/reference_adapter.h"
static_assert(std::is_same<decltype(std::declval<vo::MotionEstimator &>().getPoseCovariance()), const vo::PoseInformation &>::value, "");
static_assert(std::is_same<decltype(std::declval<vo::StereoVO &>().getPoseCovariance()), vo::PoseCovariance>::value, "");
static_assert(std::is_same<decltype(std::declval<vo::MonoVO &>().getPoseCovariance()), vo::PoseCovariance>::value, "");
static_assert(std::is_same<decltype(std::declval<vo::StereoVO &>().getPoseCovarianceRos()), std::array<double, 36>>::value, "");
static_assert(std::is_same<decltype(std::declval<vo::MonoVO &>().getPoseCovarianceRos()), std::array<double, 36>>::value, "");
static_assert(std::is_same<decltype(std::declval<StereoVO &>().getPoseCovarianceRos()), std::array<double, 36>>::value, "");
static_assert(std::is_same<decltype(std::declval<MonoVO &>().getPoseCovarianceRos()), std::array<double, 36>>::value, "");
static_assert(std::is_same<decltype(std::declval<StereoVO &>().getPoseCovariance()), vo::PoseCovariance>::value, "");
static_assert(std::is_same<decltype(std::declval<MonoVO &>().getPoseCovariance()), vo::PoseCovariance>::value, "");
int main() {
  // poseCovarianceRos: C = B P B^T on a rotation about z by 90 degrees
  vo::Mat66d P{};
  for (int i = 0; i < 6; ++i) P[(std::size_t)(i * 6 + i)] = i + 1.0;
  const float T[16] = {0, -1, 0, 5, 1, 0, 0, 6, 0, 0, 1, 7, 0, 0, 0, 1};
  const std::array<double, 36> C = vo::poseCovarianceRos(P, T);
  const double want[6] = {2, 1, 3, 5, 4, 6};
  for (int i = 0; i < 6; ++i)
    for (int j = 0; j < 6; ++j)
      if (C[(std::size_t)(i * 6 + j)] != (i == j ? want[i] : 0.0)) return 1;
  return 0;
}
"""


def test_cpp_mirrors_compile_and_the_ros_form_is_right(vo, tmp_path):
    vo.load()
    src = tmp_path / "pose_covariance_typecheck.cpp"
    src.write_text(TYPECHECK)
    exe = str(tmp_path / "pose_covariance_typecheck")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", ROOT, *ADAPTER_INC, str(src), "-o", exe])
    subprocess.check_call([exe])
    assert os.path.exists(_compile(tmp_path, "pose_covariance_demo"))


@pytest.mark.gpu
def test_cpp_demo_prints_the_python_drivers_covariance(vo, tmp_path):
    """tests/cpp/pose_covariance_demo.cpp over 10 pairs of the smallest stereo stream: the 36 values of getPoseCovarianceRos(),
    valid and n_unknown_steps of every frame equal the Python driver's (the same library: the same bits)."""
    from visual_odometry_ros_amd import synthetic as S
    W, H, K, n = 640, 240, (400.0, 400.0, 320.0, 120.0), 10
    st = S.StereoStream(width=W, height=H, K=K, n_u=20, n_v=8, seed=5, speed=0.5)
    imgs = [st.render_pair(p)[:2] for p in st.poses(n)]
    kw = dict(thres_trans=0.9, thres_alive_ratio=0.6, thres_rotation=15.0)
    exe = _compile(tmp_path, "pose_covariance_demo")
    inp, outp = tmp_path / "cov_in.bin", tmp_path / "cov_out.txt"
    with open(inp, "wb") as f:
        f.write(struct.pack("9i", n, W, H, 20, 8, 21, 4, 0, 1))
        f.write(np.array(list(K) + list(np.asarray(st.T_lr, np.float32).reshape(16)) +
                         [80.0, 0.5, 3.0, kw["thres_alive_ratio"], kw["thres_trans"], kw["thres_rotation"]], np.float32).tobytes())
        for L, R in imgs:
            f.write(np.ascontiguousarray(L).tobytes())
            f.write(np.ascontiguousarray(R).tobytes())
    subprocess.check_call([exe, str(inp), str(outp)])
    lines = [ln.split() for ln in open(outp).read().splitlines()]
    assert len(lines) == n and all(len(ln) == 39 for ln in lines)
    c = vo.Context(device=0, max_width=W, max_height=H, max_points=4096, n_slots=5, max_level=4)
    try:
        svo = vo.StereoVO(c, W, H, K, K, st.T_lr, 20, 8, thres_fastscore=15, window_size=21, max_level=4, local_ba=True,
                          pose_covariance=True, **kw)
        for k, (L, R) in enumerate(imgs):
            i = svo.trackStereoImages(L, R)
            cov, ros = svo.getPoseCovariance(), svo.getPoseCovarianceRos()
            assert int(lines[k][0]) == i.frame_id and (int(lines[k][37]), int(lines[k][38])) == (int(cov.valid), cov.n_unknown_steps), k
            got = np.array([float(v) for v in lines[k][1:37]])
            # (two summation orders of B P B^T, numpy's and the header's: 6 products per entry)
            assert np.abs(got - ros).max() <= 64 * 2.0 ** -53 * max(np.abs(ros).max(), 1e-300), k
        assert cov.valid and (np.diag(ros.reshape(6, 6)) > 0).all()
        svo.close()
    finally:
        c.close()
