// setSemiDenseWorldReanchor / getSemiDenseWorldAnchors / getSemiDenseWorldReanchorStats of the reference-typed stereo driver
// (reference_adapter.h) and of the class behind it (stereo_vo.h), and the operator's C calls, type-checked against the stand-in headers
// of tests/typecheck_stubs (tests/test_semidense_world_reanchor_cpp.py); nothing here is run.
#include "visual_odometry_ros_amd/core/visual_odometry/reference_adapter.h"

int stereo_side(StereoVO &s, const cv::Mat &l, const cv::Mat &r) {
  vo_semidense_params p = vo::StereoVO::defaultSemiDenseParams(386.1f, 129);
  s.setSemiDense(&p);
  vo_semidense_temporal_params t = vo::StereoVO::defaultSemiDenseTemporalParams();
  s.setSemiDenseTemporal(&t);
  vo_semidense_world_params w = vo::StereoVO::defaultSemiDenseWorldParams();
  s.setSemiDenseWorld(&w);
  s.setSemiDenseWorldReanchor(true);  // from now on the maps in the table follow the local BA
  s.trackStereoImages(l, r, 0.0);
  s.flushSemiDenseWorld();
  std::vector<int32_t> frame_id, kf_index, in_window;
  std::vector<float> T_wk;
  const int n = s.device().getSemiDenseWorldAnchors(&frame_id, &kf_index, &T_wk, &in_window);
  const int m = s.device().getSemiDenseWorldAnchors(nullptr, nullptr, &T_wk);
  const vo_semidense_world_reanchor_info info = s.device().getSemiDenseWorldReanchorStats();
  s.device().setSemiDenseWorldReanchor(true, 0.5f);  // only motions of half a voxel or more
  s.setSemiDenseWorldReanchor(false);
  return n + m + (int)info.reanchors + (int)info.vacant + (int)info.missing;
}

int operator_side(vo_semidense_world *wm, const float *invd, const float *sigma, const uint8_t *n_obs, const uint8_t *key, const float K[4],
                  const float T_old[16], const float T_new[16]) {
  int moved = 0;
  int rc = vo_semidense_world_remove(wm, invd, sigma, n_obs, key, 640, 0, 640, 240, 0, K, T_old);
  if (!rc) rc = vo_semidense_world_reanchor(wm, invd, sigma, n_obs, key, 640, 0, 640, 240, 0, K, T_old, T_new, &moved);
  vo_semidense_world_reanchor_info info;
  if (!rc) rc = vo_semidense_world_reanchor_stats(wm, &info);
  return rc ? rc : moved + (int)info.removals + (int)info.refused_removals + (int)info.removed;
}
