// setSemiDenseAlign / getSemiDenseAlign of the reference-typed stereo driver (reference_adapter.h) and of the class behind it
// (stereo_vo.h), type-checked against the stand-in headers of tests/typecheck_stubs (tests/test_semidense_align_cpp.py); nothing
// here is run.
#include "visual_odometry_ros_amd/core/visual_odometry/reference_adapter.h"

double stereo_side(StereoVO &s, const cv::Mat &l, const cv::Mat &r) {
  vo_semidense_params p = vo::StereoVO::defaultSemiDenseParams(386.1f, 129);
  s.setSemiDense(&p);
  vo_semidense_temporal_params t = vo::StereoVO::defaultSemiDenseTemporalParams();
  s.setSemiDenseTemporal(&t);
  vo_semidense_align_params g = vo::StereoVO::defaultSemiDenseAlignParams();
  g.min_obs = 2;
  g.huber = 8.0f;
  g.max_iters = 6;
  g.eps = 1e-4f;
  g.min_pixels = 500;
  s.setSemiDenseAlign(&g);  // from the first frame behind a keyframe on, every frame has an alignment
  s.trackStereoImages(l, r, 0.0);
  vo_semidense_align_result res;
  float T_wc[16];
  int frame_id = -1, key_frame_id = -1;
  const bool have = s.getSemiDenseAlign(res, T_wc, &frame_id, &key_frame_id);
  double health = have && res.status <= VO_SEMIDENSE_ALIGN_MAX_ITERS ? res.rms : -1.0;
  health += res.H[0] + res.b[5] + res.T_ck[3] + T_wc[3] + res.iters + res.count;
  const bool again = s.device().getSemiDenseAlign(res);
  (void)again;
  s.setSemiDenseAlign(nullptr);  // off
  s.device().setSemiDenseAlign(&g);
  return health;
}
