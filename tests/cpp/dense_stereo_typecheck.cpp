// setDenseStereo / getDensePoints of the reference-typed stereo driver (reference_adapter.h) and of the class behind it
// (stereo_vo.h), type-checked against the stand-in headers of tests/typecheck_stubs (tests/test_dense_stereo_cpp.py); nothing here
// is run.
#include "visual_odometry_ros_amd/core/visual_odometry/reference_adapter.h"

PointVec stereo_side(StereoVO &s, const cv::Mat &l, const cv::Mat &r) {
  vo_dense_stereo_params p = vo::StereoVO::defaultDenseStereoParams(386.1f, 128, 2);
  p.paths = 4;
  p.uniqueness = 15;
  s.setDenseStereo(&p);  // per keyframe
  s.trackStereoImages(l, r, 0.0);
  PointVec cloud = s.getDensePoints();  // world frame: what convertPointVecToPointCloud2 takes
  s.setDenseStereo(&p, VO_SEMIDENSE_FRAMES);
  PointVec in_camera = s.getDensePoints(false);
  s.setDenseStereo(nullptr);  // off
  vo::PointVec xyz;
  std::vector<float> sigma;
  int frame_id = -1;
  const bool have = s.device().getDensePoints(xyz, &sigma, true, &frame_id);
  (void)have;
  size_t bytes = 0;
  (void)vo_dense_stereo_workspace(1241, 376, &p, &bytes);
  cloud.insert(cloud.end(), in_camera.begin(), in_camera.end());
  return cloud;
}
