// setEqualize of the context (vo_context.h), of the classes on it (stereo_vo.h, mono_vo.h) and of the reference-typed drivers
// (reference_adapter.h), type-checked against the stand-in headers of tests/typecheck_stubs (tests/test_equalize.py); nothing
// here is run.
#include "visual_odometry_ros_amd/core/visual_odometry/reference_adapter.h"

void context_side(vo::Context &c) {
  c.setEqualize(VO_EQ_CLAHE);
  c.setEqualize(VO_EQ_CLAHE, 2.0, 4, 3);
  c.setEqualize(VO_EQ_OFF);
}

void stereo_side(StereoVO &s, const cv::Mat &l, const cv::Mat &r) {
  s.setEqualize(VO_EQ_CLAHE);
  s.trackStereoImages(l, r, 0.0);
  s.setEqualize(VO_EQ_CLAHE, 3.5, 16, 8);
  s.device().setEqualize(VO_EQ_OFF);
}

void mono_side(MonoVO &m, const cv::Mat &img) {
  m.setEqualize(VO_EQ_CLAHE, 40.0, 8, 8);
  m.trackImage(img, 0.0);
  m.device().setEqualize(VO_EQ_OFF);
}
