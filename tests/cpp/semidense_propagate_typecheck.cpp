// setSemiDensePropagate of the reference-typed stereo driver (reference_adapter.h) and setSemiDensePropagate / getSemiDenseOrigin of
// the class behind it (stereo_vo.h), type-checked against the stand-in headers of tests/typecheck_stubs
// (tests/test_semidense_propagate_cpp.py); nothing here is run.
#include "visual_odometry_ros_amd/core/visual_odometry/reference_adapter.h"

PointVec stereo_side(StereoVO &s, const cv::Mat &l, const cv::Mat &r) {
  vo_semidense_params p = vo::StereoVO::defaultSemiDenseParams(386.1f, 129);
  s.setSemiDense(&p);
  vo_semidense_temporal_params t = vo::StereoVO::defaultSemiDenseTemporalParams();
  s.setSemiDenseTemporal(&t);
  vo_semidense_propagate_params g = vo::StereoVO::defaultSemiDensePropagateParams();
  g.min_obs = 2;
  g.max_diff = 20;
  g.chi = 2.5f;
  g.sigma_add = 0.005f;
  s.setSemiDensePropagate(&g);  // from the second keyframe on, the map is carried over
  s.trackStereoImages(l, r, 0.0);
  PointVec cloud = s.getSemiDenseMapPoints();  // world frame, n_obs >= 2: not empty on a keyframe frame either
  std::vector<uint8_t> origin;
  int w = 0, h = 0, from = -1;
  const bool have = s.device().getSemiDenseOrigin(origin, &w, &h, &from);
  (void)have;
  s.setSemiDensePropagate(nullptr);  // off
  s.device().setSemiDensePropagate(&g);
  return cloud;
}
