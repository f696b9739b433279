// setSemiDense / getSemiDensePoints of the reference-typed stereo driver (reference_adapter.h) and of the class behind it
// (stereo_vo.h), type-checked against the stand-in headers of tests/typecheck_stubs (tests/test_semidense_cpp.py); nothing here
// is run.
#include "visual_odometry_ros_amd/core/visual_odometry/reference_adapter.h"

PointVec stereo_side(StereoVO &s, const cv::Mat &l, const cv::Mat &r) {
  vo_semidense_params p = vo::StereoVO::defaultSemiDenseParams(386.1f, 129);
  p.hw = 8;
  p.thres_best = 0.95f;
  s.setSemiDense(&p);  // per keyframe
  s.trackStereoImages(l, r, 0.0);
  PointVec cloud = s.getSemiDensePoints();  // world frame: what convertPointVecToPointCloud2 takes
  s.setSemiDense(&p, VO_SEMIDENSE_FRAMES);
  PointVec in_camera = s.getSemiDensePoints(false);
  s.setSemiDense(nullptr);  // off
  vo::PointVec xyz;
  std::vector<float> sigma;
  int frame_id = -1;
  const bool have = s.device().getSemiDensePoints(xyz, &sigma, true, &frame_id);
  (void)have;
  cloud.insert(cloud.end(), in_camera.begin(), in_camera.end());
  return cloud;
}
