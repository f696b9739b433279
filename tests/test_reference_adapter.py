"""T13 / §8(b): the reference-typed class surface (reference_adapter.h: FeatureTracker, MotionEstimator,
FeatureExtractor with the reference's exact signatures on cv:: / Eigen:: types) is type-checked with g++ against
minimal stand-in headers (tests/typecheck_stubs/: declared stand-ins, used for type-checking only — the image has
neither Eigen nor OpenCV), and its layout conversions (column-major Eigen <-> row-major C ABI, pixel / point vectors,
image views) are executed on the CPU with a non-symmetric 4x4."""
import os
import subprocess


ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STUBS = os.path.join(ROOT, "tests", "typecheck_stubs")
SRC = os.path.join(ROOT, "tests", "cpp", "adapter_typecheck.cpp")
LIBDIR = os.path.join(ROOT, "visual_odometry_ros_amd", "lib")
BASE = ["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", ROOT, "-I", os.path.join(STUBS, "thirdparty")]


def test_adapter_type_checks_against_stand_in_headers():
    r = subprocess.run(BASE + ["-I", os.path.join(STUBS, "reference"), "-fsyntax-only", SRC], capture_output=True,
                       text=True)
    assert r.returncode == 0, r.stderr[-4000:]


def test_ros_include_paths_resolve_to_the_adapter(tmp_path):
    """The ROS nodes include core/visual_odometry/stereo_vo/stereo_vo.h (ros2/visual_odometry/stereo_vo_ros2.h:28,
    ros1/.../stereo_vo_ros1.h:31), core/visual_odometry/mono_vo/mono_vo.h (ros1/.../mono_vo_ros1.h:32) and call
    Landmark::setPatch: with visual_odometry_ros_amd/ros_include in front of the reference root those three names give the
    libvo_hip-backed classes — what the nodes' own lines need type-checks against them."""
    src = tmp_path / "ros_side.cpp"
    src.write_text('''
#include "core/visual_odometry/stereo_vo/stereo_vo.h"
#include "core/visual_odometry/mono_vo/mono_vo.h"
#include "core/visual_odometry/landmark.h"
#include <memory>
// ros2/visual_odometry/stereo_vo_ros2.cpp:18-20, :104; ros1/visual_odometry/mono_vo_ros1.cpp:49, :60, :123
double node(const cv::Mat &l, const cv::Mat &r, double t, const std::string &dir) {
  Landmark::setPatch(7);
  std::unique_ptr<StereoVO> stereo_vo_ = std::make_unique<StereoVO>("rosbag", dir);
  stereo_vo_->trackStereoImages(l, r, t);
  std::unique_ptr<MonoVO> mono_vo_ = std::make_unique<MonoVO>("rosbag", dir);
  mono_vo_->trackImage(l, t);
  const StereoVO::AlgorithmStatistics &stat = stereo_vo_->getStatistics();
  const MonoVO::AlgorithmStatistics &ms = mono_vo_->getStatistics();
  return stat.stats_frame.back().Twc(0, 3) + ms.stats_frame.back().Twc(1, 3) + stat.stats_landmark.back().avg_age;
}
''')
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "visual_odometry_ros_amd", "ros_include"),
                        "-I", os.path.join(STUBS, "reference"), "-I", ROOT, "-I", os.path.join(STUBS, "thirdparty"), "-fsyntax-only", str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]


def test_adapter_layout_conversions_round_trip(tmp_path, vo):
    """Column-major Eigen::Matrix4f -> row-major C ABI -> back, on a NON-symmetric matrix (a symmetric one would hide
    a missing transpose); runs on the CPU: no GPU entry point is called."""
    exe = str(tmp_path / "adapter_typecheck")
    subprocess.check_call(BASE + ["-I", os.path.join(STUBS, "reference"), "-O1", SRC, "-o", exe, "-L", LIBDIR,
                                  "-lvo_hip", f"-Wl,-rpath,{LIBDIR}"])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "adapter conversions ok" in r.stdout, r.stdout + r.stderr
