// pose_covariance.hpp — result block and launcher of the pose covariance kernel (pose_covariance.hip).
#pragma once
#include "vo_internal.hpp"

// What one launch leaves behind (device copy; the drivers also get it in pinned host memory). Row-major 6x6, order
// xi = [rho; phi] of se3Exp_f (translation part first).
struct VoPoseCovBlock {
  double H[36];      // sum_i w_i sum_rows J J^T at the returned pose (no (1 + lambda) factor)
  double Sigma[36];  // s2 * H^-1 (sigma_px^2 * H^-1 with a caller-given sigma_px); zero when !valid
  double P[36];      // the chain: Ad(T10) P_prev Ad(T10)^T (+ Sigma when valid); zero without a previous block
  double s2;         // sum_i w_i |r_i|^2 / (rows * sum_i w_i - 6), px^2
  int valid;
  int n;
  int n_unknown_steps;  // frames of the chain whose pose did not come from the BA (or whose block is not valid)
  int pad_;
};

// One launch (one workgroup) on stream `st`, reading device-resident inputs:
//   n / d_n        the number of points, from the argument or (d_n != null) read on the device
//   T01 / d_T01    the pose the BA returned (row-major 4x4, f32), from the argument or read on the device
//   have_pose      0: the frame's pose did not come from the BA (the chain is only carried with T01)
//   d_is_nan       optional device flag of the BA launch (vo_gn_dev_info::is_nan): non-zero = no BA pose either
//   prev           the chain's previous block (null: P is not chained and stays zero)
//   out, out_host  the block on the device and (may be null) its copy in pinned host memory
int vo_pose_cov_enqueue(vo_ctx *c, hipStream_t st, bool stereo, const float *dX, const float *dP1, const float *dP2, int n,
                        const int *d_n, const float Kl[4], const float Kr[4], const float T_lr[16], const float T01[16],
                        const float *d_T01, int have_pose, const int *d_is_nan, double sigma_px, const VoPoseCovBlock *prev,
                        VoPoseCovBlock *out, VoPoseCovBlock *out_host);

// ---- the drivers' side (vo_svo_set_pose_covariance / vo_mvo_set_pose_covariance) ----
// The chain's last accepted block is d_blk[cur]; a frame's launch reads it and writes d_blk[cur ^ 1] (and the pinned copy), and
// the driver's result call accepts the step (cur ^= 1) — so a frame whose launch is issued again (a frame re-issued after a join
// time-out, MonoVO's 5-point fallback) chains from the same previous block again.
struct VoPoseCovState {
  bool on = false, launched = false;  // switched on; the frame in flight has a launch
  double sigma_px = 0.0;
  VoPoseCovBlock *d_blk = nullptr, *h_blk = nullptr;
  hipEvent_t done = nullptr;
  int cur = 0, recoveries = 0;
};
int vo_pose_cov_state_set(vo_ctx *c, VoPoseCovState *v, int on, double sigma_px);  // the option's only allocations
void vo_pose_cov_state_free(VoPoseCovState *v);
// one step on the main stream: stereo / mono by `stereo`; carry_T01 != null: the frame's pose (carry_T01) did not come from the BA
int vo_pose_cov_state_step(vo_ctx *c, VoPoseCovState *v, bool stereo, const float Kl[4], const float Kr[4], const float T_lr[16],
                           const float *carry_T01, const int *d_no_pose);
inline void vo_pose_cov_state_accept(VoPoseCovState *v) {
  if (v->launched) v->cur ^= 1;
  v->launched = false;
}
int vo_pose_cov_state_get(vo_ctx *c, VoPoseCovState *v, double P[36], double Sigma_xi[36], double *s2, int *valid, int *n_points,
                          int *n_unknown_steps);
// what the last steady-state frame's launch read (the BA set of the frame operator and the T01 the BA launch wrote)
int vo_pose_cov_inputs(vo_ctx *c, bool stereo, float *X, float *pts_l, float *pts_r, int cap, int *n, float T01[16]);
