// setSemiDenseWorldCarve / getSemiDenseWorldFree / getSemiDenseWorldCarveStats of the reference-typed stereo driver
// (reference_adapter.h) and of the class behind it (stereo_vo.h), and the operator's C calls, type-checked against the stand-in headers
// of tests/typecheck_stubs (tests/test_semidense_world_carve_cpp.py); nothing here is run.
#include "visual_odometry_ros_amd/core/visual_odometry/reference_adapter.h"

int stereo_side(StereoVO &s, const cv::Mat &l, const cv::Mat &r) {
  vo_semidense_params p = vo::StereoVO::defaultSemiDenseParams(386.1f, 129);
  s.setSemiDense(&p);
  vo_semidense_temporal_params t = vo::StereoVO::defaultSemiDenseTemporalParams();
  s.setSemiDenseTemporal(&t);
  vo_semidense_world_params w = vo::StereoVO::defaultSemiDenseWorldParams();
  s.setSemiDenseWorld(&w);
  vo_semidense_world_carve_params c = vo::StereoVO::defaultSemiDenseWorldCarveParams();
  c.margin = 3.0f;
  s.setSemiDenseWorldCarve(&c);  // from now on every integration is followed by the carve of the same map
  s.trackStereoImages(l, r, 0.0);
  s.flushSemiDenseWorld();
  std::vector<uint32_t> free_count, count, keyframes;
  std::vector<uint8_t> grey;
  PointVec all = s.getSemiDenseWorldFree(free_count);
  PointVec kept = s.getSemiDenseWorldFree(free_count, 1, 2, 1, 2);  // free <= count / 2, seen by two keyframes
  vo::PointVec xyz;
  const int n = s.device().getSemiDenseWorldFree(xyz, free_count, 0, 1, 1, 1, &count, &keyframes, &grey);
  const vo_semidense_world_carve_info info = s.device().getSemiDenseWorldCarveStats();
  s.setSemiDenseWorldCarve(nullptr);
  return n + (int)all.size() + (int)kept.size() + (int)info.carves + (int)info.rays + (int)info.short_rays + (int)info.visits + (int)info.hits;
}

int operator_side(vo_semidense_world *wm, const float *invd, const float *sigma, const uint8_t *n_obs, const float K[4], const float T_wk[16]) {
  vo_semidense_world_carve_params prm;
  int rc = vo_semidense_world_carve_default_params(&prm);
  if (!rc) rc = vo_semidense_world_carve(wm, invd, sigma, n_obs, 640, 240, 0, K, T_wk, &prm);
  vo_semidense_world_carve_info info;
  if (!rc) rc = vo_semidense_world_carve_stats(wm, &info);
  int n = 0;
  uint32_t free_count[16], count[16];
  float xyz[48];
  uint64_t sums[80];
  if (!rc) rc = vo_semidense_world_points_free(wm, 1, 1, 1, 2, 16, nullptr, xyz, nullptr, count, nullptr, nullptr, sums, free_count, &n);
  return rc ? rc : n + (int)info.carves + (int)(prm.margin + prm.chi + prm.z_near);
}
