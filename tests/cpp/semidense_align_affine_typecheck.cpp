// setSemiDenseAlignAffine / getSemiDenseAlign (with gain and offset) of the reference-typed stereo driver (reference_adapter.h) and of the
// class behind it (stereo_vo.h), type-checked against the stand-in headers of tests/typecheck_stubs
// (tests/test_semidense_align_affine_cpp.py); nothing here is run.
#include "visual_odometry_ros_amd/core/visual_odometry/reference_adapter.h"

double stereo_side(StereoVO &s, const cv::Mat &l, const cv::Mat &r) {
  vo_semidense_params p = vo::StereoVO::defaultSemiDenseParams(386.1f, 129);
  s.setSemiDense(&p);
  vo_semidense_temporal_params t = vo::StereoVO::defaultSemiDenseTemporalParams();
  s.setSemiDenseTemporal(&t);
  vo_semidense_align_pyr_params g = vo::StereoVO::defaultSemiDenseAlignPyramidParams();
  s.setSemiDenseAlignPyramid(&g, VO_SEMIDENSE_ALIGN_START_PREVIOUS);
  vo_semidense_affine_params a = vo::StereoVO::defaultSemiDenseAffineParams();
  a.gain0 = 0.9f;
  a.offset0 = 4.0f;
  s.setSemiDenseAlignAffine(&a);  // a modifier of the alignment that is on
  s.trackStereoImages(l, r, 0.0);
  vo_semidense_align_affine_result res;
  float T_wc[16];
  int frame_id = -1, key_frame_id = -1;
  const bool have = s.getSemiDenseAlign(res, T_wc, &frame_id, &key_frame_id);
  double health = have && res.status != VO_SEMIDENSE_ALIGN_AFFINE_RANGE ? res.rms + res.gain + res.offset + res.G + res.O + res.H[35] + res.b[7] : -1.0;
  for (int lv = 0; lv < res.levels; ++lv) health += res.level_status[lv] + res.level_iters[lv] + res.level_count[lv] + res.level_rms[lv] + res.level_G[lv] + res.level_O[lv];
  health += res.start_prev + T_wc[3];
  vo_semidense_align_pyr_result per_level;  // the getters without gain and offset serve while the modifier is on
  vo_semidense_align_result plain;
  const bool again = s.getSemiDenseAlign(per_level) && s.device().getSemiDenseAlign(plain);
  (void)again;
  s.setSemiDenseAlignAffine(nullptr);  // off
  s.device().setSemiDenseAlignAffine(&a);
  return health;
}
