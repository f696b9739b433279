// setMask of the reference-typed drivers (reference_adapter.h) and of the classes behind them (stereo_vo.h, mono_vo.h),
// type-checked against the stand-in headers of tests/typecheck_stubs (tests/test_mask.py); nothing here is run.
#include "visual_odometry_ros_amd/core/visual_odometry/reference_adapter.h"

#include <cstdint>
#include <vector>

void stereo_side(StereoVO &s, const cv::Mat &mask, const cv::Mat &l, const cv::Mat &r) {
  s.setMask(mask);       // CV_8UC1, the left image's size
  s.trackStereoImages(l, r, 0.0);
  s.setMask(cv::Mat());  // none
  std::vector<std::uint8_t> plane((std::size_t)s.device().width() * (std::size_t)s.device().height(), 255);
  s.device().setMask(plane.data(), s.device().width());
  s.device().setMask(plane.data(), s.device().width(), /*on_device=*/false);
  s.device().setMask(nullptr, 0);
}

void mono_side(MonoVO &m, const cv::Mat &mask, const cv::Mat &img) {
  m.setMask(mask);
  m.trackImage(img, 0.0);
  m.setMask(cv::Mat());
  const std::uint8_t *none = nullptr;
  m.device().setMask(none, m.device().width());
}
