// setDenseSpeckle / getDenseSpeckleStats of the reference-typed stereo driver (reference_adapter.h) and of the class behind it
// (stereo_vo.h), and the operator's C interface, type-checked against the stand-in headers of tests/typecheck_stubs
// (tests/test_dense_speckle_cpp.py); nothing here is run.
#include "visual_odometry_ros_amd/core/visual_odometry/reference_adapter.h"

PointVec stereo_side(StereoVO &s, const cv::Mat &l, const cv::Mat &r) {
  vo_dense_stereo_params p = vo::StereoVO::defaultDenseStereoParams(386.1f, 128, 2);
  s.setDenseStereo(&p);
  vo_speckle_params sp = vo::StereoVO::defaultSpeckleParams();
  sp.max_size = 50;
  sp.max_diff = 2.0f;
  s.setDenseSpeckle(&sp);
  s.trackStereoImages(l, r, 0.0);
  PointVec cloud = s.getDensePoints();  // without the speckles
  int n_removed = 0, n_components = 0;
  s.device().getDenseSpeckleStats(&n_removed, &n_components);
  s.setDenseSpeckle(nullptr);  // off
  s.device().setDenseSpeckle(&sp);
  return cloud;
}

int operator_side(vo_ctx *ctx, float *disparity, float *sigma_invd, uint8_t *status, int32_t *label, int32_t *size) {
  static_assert(VO_DISPARITY_SPECKLE == 6, "the status of a removed pixel");
  vo_speckle_params sp;
  int rc = vo_speckle_default_params(&sp);
  size_t bytes = 0;
  rc |= vo_speckle_workspace(1241, 376, &bytes);
  int n_removed = 0, n_components = 0;
  rc |= vo_disparity_speckle_filter(ctx, disparity, sigma_invd, status, 1241, 376, &sp, label, size, &n_removed, &n_components, 0);
  rc |= vo_disparity_speckle_filter(ctx, disparity, nullptr, status, 1241, 376, &sp, nullptr, nullptr, nullptr, nullptr, 1);
  return rc;
}
