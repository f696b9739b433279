// setSemiDenseWorld / flushSemiDenseWorld / getSemiDenseWorldPoints of the reference-typed stereo driver (reference_adapter.h) and of
// the class behind it (stereo_vo.h), type-checked against the stand-in headers of tests/typecheck_stubs
// (tests/test_semidense_world_cpp.py); nothing here is run.
#include "visual_odometry_ros_amd/core/visual_odometry/reference_adapter.h"

PointVec stereo_side(StereoVO &s, const cv::Mat &l, const cv::Mat &r) {
  vo_semidense_params p = vo::StereoVO::defaultSemiDenseParams(386.1f, 129);
  s.setSemiDense(&p);
  vo_semidense_temporal_params t = vo::StereoVO::defaultSemiDenseTemporalParams();
  s.setSemiDenseTemporal(&t);
  vo_semidense_world_params w = vo::StereoVO::defaultSemiDenseWorldParams();
  w.voxel = 0.2f;
  w.capacity_log2 = 20;
  w.min_obs = 3;
  w.z_max = 25.0f;
  s.setSemiDenseWorld(&w);  // from the next keyframe change on, the outgoing keyframe's map goes into the table
  s.trackStereoImages(l, r, 0.0);
  s.flushSemiDenseWorld();  // the end of the sequence: the current keyframe's map too
  PointVec cloud = s.getSemiDenseWorldPoints();
  PointVec confirmed = s.getSemiDenseWorldPoints(1, 2);  // seen by two keyframes
  vo::PointVec xyz;
  std::vector<uint32_t> count, keyframes;
  std::vector<uint8_t> grey;
  const int n = s.device().getSemiDenseWorldPoints(xyz, 2, 1, &count, &keyframes, &grey);
  const vo_semidense_world_info info = s.device().getSemiDenseWorldStats();
  (void)n;
  (void)info.occupied;
  s.device().clearSemiDenseWorld();
  s.setSemiDenseWorld(nullptr);  // off
  vo_semidense_regularize_params g = vo::StereoVO::defaultSemiDenseRegularizeParams();
  s.setSemiDenseRegularize(&g);
  s.device().setSemiDenseWorld(&w, VO_SEMIDENSE_WORLD_REGULARIZED);
  return cloud.empty() ? confirmed : cloud;
}
