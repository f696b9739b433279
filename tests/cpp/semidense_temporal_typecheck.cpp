// setSemiDenseTemporal / getSemiDenseMapPoints of the reference-typed stereo driver (reference_adapter.h) and of the class behind it
// (stereo_vo.h), type-checked against the stand-in headers of tests/typecheck_stubs (tests/test_semidense_temporal_cpp.py); nothing
// here is run.
#include "visual_odometry_ros_amd/core/visual_odometry/reference_adapter.h"

PointVec stereo_side(StereoVO &s, const cv::Mat &l, const cv::Mat &r) {
  vo_semidense_params p = vo::StereoVO::defaultSemiDenseParams(386.1f, 129);
  s.setSemiDense(&p);  // the static result of every keyframe seeds the map
  vo_semidense_temporal_params t = vo::StereoVO::defaultSemiDenseTemporalParams();
  t.z_max = 80.0f;
  t.max_search = 96;
  s.setSemiDenseTemporal(&t);
  s.trackStereoImages(l, r, 0.0);
  PointVec cloud = s.getSemiDenseMapPoints();  // world frame, n_obs >= 2
  PointVec in_camera = s.getSemiDenseMapPoints(false, 3);
  s.setSemiDenseTemporal(nullptr);  // off
  vo::PointVec xyz;
  std::vector<float> sigma;
  int frame_id = -1;
  const bool have = s.device().getSemiDenseMapPoints(xyz, &sigma, true, 2, &frame_id);
  (void)have;
  cloud.insert(cloud.end(), in_camera.begin(), in_camera.end());
  return cloud;
}
