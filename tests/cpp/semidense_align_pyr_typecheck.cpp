// setSemiDenseAlignPyramid / getSemiDenseAlign (per level) of the reference-typed stereo driver (reference_adapter.h) and of the class
// behind it (stereo_vo.h), type-checked against the stand-in headers of tests/typecheck_stubs (tests/test_semidense_align_pyr_cpp.py);
// nothing here is run.
#include "visual_odometry_ros_amd/core/visual_odometry/reference_adapter.h"

double stereo_side(StereoVO &s, const cv::Mat &l, const cv::Mat &r) {
  vo_semidense_params p = vo::StereoVO::defaultSemiDenseParams(386.1f, 129);
  s.setSemiDense(&p);
  vo_semidense_temporal_params t = vo::StereoVO::defaultSemiDenseTemporalParams();
  s.setSemiDenseTemporal(&t);
  vo_semidense_align_pyr_params g = vo::StereoVO::defaultSemiDenseAlignPyramidParams();
  g.huber = 8.0f;
  g.levels = 4;
  g.max_iters_level[3] = 12;
  s.setSemiDenseAlignPyramid(&g, VO_SEMIDENSE_ALIGN_START_PREVIOUS);  // from the first frame behind the next keyframe on
  s.trackStereoImages(l, r, 0.0);
  vo_semidense_align_pyr_result res;
  float T_wc[16];
  int frame_id = -1, key_frame_id = -1;
  const bool have = s.getSemiDenseAlign(res, T_wc, &frame_id, &key_frame_id);
  double health = have && res.status <= VO_SEMIDENSE_ALIGN_MAX_ITERS ? res.rms : -1.0;
  for (int lv = 0; lv < res.levels; ++lv) health += res.level_status[lv] + res.level_iters[lv] + res.level_count[lv] + res.level_rms[lv];
  health += res.start_prev + T_wc[3];
  vo_semidense_align_result plain;  // the level-0 getter serves either setter
  const bool again = s.device().getSemiDenseAlign(plain);
  (void)again;
  s.setSemiDenseAlignPyramid(nullptr);  // off
  s.device().setSemiDenseAlignPyramid(&g);
  return health;
}
