// setZnccGate of the reference-typed drivers (reference_adapter.h) and of the classes behind them (stereo_vo.h, mono_vo.h),
// type-checked against the stand-in headers of tests/typecheck_stubs (tests/test_zncc.py); nothing here is run.
#include "visual_odometry_ros_amd/core/visual_odometry/reference_adapter.h"

void stereo_side(StereoVO &s, const cv::Mat &l, const cv::Mat &r) {
  s.setZnccGate(VO_ZNCC_TEMPORAL);  // the commented-out call's numbers: 15 x 15, > 0.5
  s.setZnccGate(VO_ZNCC_TEMPORAL | VO_ZNCC_STEREO, 0.8f, 21, VO_ZNCC_PATTERN_CENTERED);
  s.trackStereoImages(l, r, 0.0);
  s.setZnccGate(0);  // off
  s.device().setZnccGate(VO_ZNCC_STEREO, 0.9f, 15, VO_ZNCC_PATTERN_REFERENCE);
}

void mono_side(MonoVO &m, const cv::Mat &img) {
  m.setZnccGate(VO_ZNCC_TEMPORAL, 0.8f);
  m.trackImage(img, 0.0);
  m.setZnccGate(0);
  m.device().setZnccGate(VO_ZNCC_TEMPORAL, 0.5f, 31);
}
