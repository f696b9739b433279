// setSemiDenseWorldMerge / getSemiDenseWorldSource of the reference-typed stereo driver (reference_adapter.h) and of the class behind
// it (stereo_vo.h), the world map's two sources that read the dense result, and the operator's C interface, type-checked against the
// stand-in headers of tests/typecheck_stubs (tests/test_semidense_map_merge_cpp.py); nothing here is run.
#include "visual_odometry_ros_amd/core/visual_odometry/reference_adapter.h"

int stereo_side(StereoVO &s, const cv::Mat &l, const cv::Mat &r) {
  static_assert(VO_SEMIDENSE_WORLD_DENSE == 2 && VO_SEMIDENSE_WORLD_MERGED == 3, "the sources behind raw and regularized");
  vo_dense_stereo_params p = vo::StereoVO::defaultDenseStereoParams(386.1f, 128, 2);
  s.setDenseStereo(&p);
  vo_semidense_world_params wp;
  vo_semidense_world_default_params(&wp);
  s.setSemiDenseWorld(&wp, VO_SEMIDENSE_WORLD_MERGED);
  vo_semidense_map_merge_params mp = vo::StereoVO::defaultSemiDenseWorldMergeParams();
  mp.chi = 2.5f;
  mp.keep_obs = 3;
  s.setSemiDenseWorldMerge(&mp);
  s.trackStereoImages(l, r, 0.0);
  std::vector<float> invd, sigma;
  std::vector<uint8_t> n_obs, origin;
  int w = 0, h = 0;
  uint64_t counts[6];
  int frame_id = s.getSemiDenseWorldSource(&invd, &sigma, &n_obs, &origin, &w, &h, counts);
  frame_id += s.device().getSemiDenseWorldSource(nullptr, nullptr, &n_obs, nullptr, &w, &h);
  s.setSemiDenseWorldMerge(nullptr);  // the defaults
  s.setSemiDenseWorld(&wp, VO_SEMIDENSE_WORLD_DENSE);
  s.device().setSemiDenseWorldMerge(&mp);
  return frame_id;
}

int operator_side(vo_ctx *ctx, const float *m_invd, const float *m_sigma, const uint8_t *m_n_obs, const float *disparity, const float *sigma_invd,
                  const uint8_t *status, float *invd, float *sigma, uint8_t *n_obs, uint8_t *origin) {
  vo_semidense_map_merge_params mp;
  int rc = vo_semidense_map_merge_default_params(&mp);
  uint64_t counts[6];
  rc |= vo_semidense_map_merge(ctx, m_invd, m_sigma, m_n_obs, disparity, sigma_invd, status, 1241, 376, 386.1f, &mp, invd, sigma, n_obs, origin, counts, 0);
  rc |= vo_semidense_map_merge(ctx, nullptr, nullptr, nullptr, disparity, sigma_invd, status, 1241, 376, 386.1f, &mp, invd, sigma, n_obs, nullptr, nullptr, 1);
  return rc;
}
