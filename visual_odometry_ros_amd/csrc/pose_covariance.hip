// pose_covariance.hip — covariance of the pose the pose-only Gauss-Newton returned.
//
// The estimator (gn_pose.hip) builds the 6x6 normal matrix of its residuals in f32 every iteration and discards it. This
// kernel restates it once, in f64, at the pose that was returned: the Jacobian rows are the reference's
// (core/visual_odometry/motion_estimator.cpp:976-981, :993-998 stereo left; :755-760, :784-789 mono; the right camera's rows are
// the exact derivative, which the reference's :1009-1014, :1026-1031 are not),
// the weight is the estimator's own Huber weight at that pose, every point of the set enters. One workgroup:
//   thread t   : serial f64 partials over points t, t + PC_T, ...   (21 H + sum w |r|^2 + sum w)
//   workgroup  : the PC_T partials of every sum through LDS, halving tree in natural order (fixed: same bits every run)
//   36 lanes   : H -> S H S (S = diag(H)^-1/2) -> Cholesky -> inverse -> unscale -> Sigma = s2 H^-1,
//                P = Ad(T10) P_prev Ad(T10)^T + Sigma, one result block
// Kept out of gn_pose.hip so that the hot kernels' code does not move; it is launched only on request.
#include "pose_covariance.hpp"

#include "frame_state.hpp"

#define PC_T 256
#define PC_NS 23  // 21 H (upper triangle) + sum w |r|^2 + sum w

struct PcArgs {
  const float *X, *p1, *p2;
  int n, cap;
  const int *d_n;
  float Kl[4], Kr[4];
  double Rrl[9], trl[3];
  float T01[16];
  const float *d_T01;
  int have_pose;
  const int *d_is_nan;
  double sigma_px;
  const VoPoseCovBlock *prev;
  VoPoseCovBlock *out, *out_host;
};

// upper-triangular index of (i, j), i <= j, row-major
__device__ __forceinline__ constexpr int pc_ut(int i, int j) { return i * 6 - (i * (i - 1)) / 2 + (j - i); }

__device__ __forceinline__ void pc_row(double (&acc)[PC_NS], double w, const double (&J)[6]) {
#pragma unroll
  for (int i = 0; i < 6; ++i) {
    const double l = w * J[i];
#pragma unroll
    for (int j = i; j < 6; ++j) acc[pc_ut(i, j)] += l * J[j];
  }
}
__device__ __forceinline__ void pc_jac_x(double (&J)[6], double f, double iz, double xiz, double yiz) {
  const double fxxiz = f * xiz;
  J[0] = f * iz;
  J[1] = 0.0;
  J[2] = -fxxiz * iz;
  J[3] = -fxxiz * yiz;
  J[4] = f * (1.0 + xiz * xiz);
  J[5] = -f * yiz;
}
__device__ __forceinline__ void pc_jac_y(double (&J)[6], double f, double iz, double xiz, double yiz) {
  const double fyyiz = f * yiz;
  J[0] = 0.0;
  J[1] = f * iz;
  J[2] = -fyyiz * iz;
  J[3] = -f * (1.0 + yiz * yiz);
  J[4] = fyyiz * xiz;
  J[5] = f * xiz;
}

// A right-camera row: the derivative of the right projection under T10 <- exp(delta) T10. Xr = R_rl Xl + t_rl moves as
// R_rl [I | -[Xl]x] delta, so with a = (d proj / d Xr) R_rl the row is [a | a x-rotated by Xl]. For R_rl = I and t_rl = 0 these
// are the reference's rows; the reference's own right rows put Xr into the rotation columns, which is not the derivative
// (DESIGN.md §13).
__device__ __forceinline__ void pc_jac_right(double (&J)[6], double d0, double d1, double d2, const double (&M)[9], const double (&Xl)[3]) {
  const double a0 = (d0 * M[0] + d1 * M[3]) + d2 * M[6];
  const double a1 = (d0 * M[1] + d1 * M[4]) + d2 * M[7];
  const double a2 = (d0 * M[2] + d1 * M[5]) + d2 * M[8];
  J[0] = a0;
  J[1] = a1;
  J[2] = a2;
  J[3] = a2 * Xl[1] - a1 * Xl[2];
  J[4] = a0 * Xl[2] - a2 * Xl[0];
  J[5] = a1 * Xl[0] - a0 * Xl[1];
}

template <bool STEREO>
__global__ __launch_bounds__(PC_T) void pose_cov_kernel(PcArgs a) {
  __shared__ double s_red[PC_NS * PC_T];
  __shared__ double s_H[36], s_A[36], s_L[36], s_Li[36], s_Sig[36], s_Ad[36], s_P[36], s_Tm[36];
  __shared__ double s_d[6], s_T10[12], s_s2;
  __shared__ int s_bad, s_valid;

  const int tid = threadIdx.x;
  int n = a.d_n ? *a.d_n : a.n;
  n = n < 0 ? 0 : (n > a.cap ? a.cap : n);
  // T10 = the SE(3) inverse of the f32 T01, in f64
  double R10[9], t10[3];
  {
    float T01[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) T01[k] = a.d_T01 ? a.d_T01[k] : a.T01[k];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int j = 0; j < 3; ++j) R10[i * 3 + j] = (double)T01[j * 4 + i];
    const double t0 = (double)T01[3], t1 = (double)T01[7], t2 = (double)T01[11];
#pragma unroll
    for (int i = 0; i < 3; ++i) t10[i] = -((R10[i * 3 + 0] * t0 + R10[i * 3 + 1] * t1) + R10[i * 3 + 2] * t2);
  }
  if (tid == 0) {
#pragma unroll
    for (int k = 0; k < 9; ++k) s_T10[k] = R10[k];
#pragma unroll
    for (int k = 0; k < 3; ++k) s_T10[9 + k] = t10[k];
    s_bad = 0;
  }

  double acc[PC_NS];
#pragma unroll
  for (int k = 0; k < PC_NS; ++k) acc[k] = 0.0;
  int bad = 0;
  const double fx_l = (double)a.Kl[0], fy_l = (double)a.Kl[1], cx_l = (double)a.Kl[2], cy_l = (double)a.Kl[3];
  for (int i = tid; i < n; i += PC_T) {
    const double X0 = (double)a.X[3 * i], X1 = (double)a.X[3 * i + 1], X2 = (double)a.X[3 * i + 2];
    double Xl[3];
#pragma unroll
    for (int r = 0; r < 3; ++r) Xl[r] = ((R10[r * 3 + 0] * X0 + R10[r * 3 + 1] * X1) + R10[r * 3 + 2] * X2) + t10[r];
    const double iz_l = 1.0 / Xl[2];
    const double xiz_l = Xl[0] * iz_l, yiz_l = Xl[1] * iz_l;
    const double rx_l = (fx_l * xiz_l + cx_l) - (double)a.p1[2 * i], ry_l = (fy_l * yiz_l + cy_l) - (double)a.p1[2 * i + 1];
    double J[6];
    if (STEREO) {
      const double fx_r = (double)a.Kr[0], fy_r = (double)a.Kr[1], cx_r = (double)a.Kr[2], cy_r = (double)a.Kr[3];
      double Xr[3];
#pragma unroll
      for (int r = 0; r < 3; ++r) Xr[r] = ((a.Rrl[r * 3 + 0] * Xl[0] + a.Rrl[r * 3 + 1] * Xl[1]) + a.Rrl[r * 3 + 2] * Xl[2]) + a.trl[r];
      const double iz_r = 1.0 / Xr[2];
      const double xiz_r = Xr[0] * iz_r, yiz_r = Xr[1] * iz_r;
      const double rx_r = (fx_r * xiz_r + cx_r) - (double)a.p2[2 * i], ry_r = (fy_r * yiz_r + cy_r) - (double)a.p2[2 * i + 1];
      const double ab = 0.5 * (((fabs(rx_l) + fabs(ry_l)) + fabs(rx_r)) + fabs(ry_r));
      const double w = ab < 0.5 ? 1.0 : 0.5 / ab;
      if (!__builtin_isfinite(ab)) bad = 1;
      pc_jac_x(J, fx_l, iz_l, xiz_l, yiz_l);
      pc_row(acc, w, J);
      pc_jac_y(J, fy_l, iz_l, xiz_l, yiz_l);
      pc_row(acc, w, J);
      // the right camera's rows: the exact derivative (pc_jac_right)
      pc_jac_right(J, fx_r * iz_r, 0.0, -(fx_r * xiz_r) * iz_r, a.Rrl, Xl);
      pc_row(acc, w, J);
      pc_jac_right(J, 0.0, fy_r * iz_r, -(fy_r * yiz_r) * iz_r, a.Rrl, Xl);
      pc_row(acc, w, J);
      acc[21] += w * ((rx_l * rx_l + ry_l * ry_l) + (rx_r * rx_r + ry_r * ry_r));
      acc[22] += w;
    } else {
      const double ab = fabs(rx_l) + fabs(ry_l);
      const double w = ab < 0.5 ? 1.0 : 0.5 / ab;
      if (!__builtin_isfinite(ab)) bad = 1;
      pc_jac_x(J, fx_l, iz_l, xiz_l, yiz_l);
      pc_row(acc, w, J);
      pc_jac_y(J, fy_l, iz_l, xiz_l, yiz_l);
      pc_row(acc, w, J);
      acc[21] += w * (rx_l * rx_l + ry_l * ry_l);
      acc[22] += w;
    }
  }

  // ---- the PC_T partials of every sum: halving tree in natural order ----
#pragma unroll
  for (int k = 0; k < PC_NS; ++k) s_red[k * PC_T + tid] = acc[k];
  bad = __syncthreads_or(bad);
  for (int s = PC_T / 2; s >= 1; s >>= 1) {
    if (tid < s) {
#pragma unroll
      for (int k = 0; k < PC_NS; ++k) s_red[k * PC_T + tid] = s_red[k * PC_T + tid] + s_red[k * PC_T + tid + s];
    }
    __syncthreads();
  }

  // ---- 36 lanes, one per entry (i, j); (lo, hi) so that both halves of a symmetric result get the same operations ----
  const int ei = tid / 6, ej = tid % 6;
  const int lo = ei < ej ? ei : ej, hi = ei < ej ? ej : ei;
  const bool el = tid < 36;
  if (el) {
    const double h = s_red[(lo * 6 - (lo * (lo - 1)) / 2 + (hi - lo)) * PC_T];
    s_H[tid] = h;
    if (!__builtin_isfinite(h)) s_bad = 1;
    s_L[tid] = 0.0;
    s_Li[tid] = 0.0;
  }
  const double rows = STEREO ? 4.0 : 2.0;
  if (tid == 0) {
    const double swr = s_red[21 * PC_T], sw = s_red[22 * PC_T];
    const double den = rows * sw - 6.0;
    const double s2 = swr / den;
    if (!(den > 0.0) || !__builtin_isfinite(s2)) s_bad = 1;
    s_s2 = (den > 0.0 && __builtin_isfinite(s2)) ? s2 : 0.0;
  }
  __syncthreads();
  if (tid < 6) {
    const double dg = s_H[tid * 6 + tid];
    if (!(dg > 0.0)) s_bad = 1;
    s_d[tid] = 1.0 / sqrt(dg);
  }
  __syncthreads();
  if (el) s_A[tid] = (s_H[tid] * s_d[lo]) * s_d[hi];
  __syncthreads();
  // Cholesky of S H S (lower), column by column. S H S has a unit diagonal, so a pivot is 1 minus a sum of at most five
  // squares of entries that were divided by the square roots of the earlier pivots: "not positive definite" is a pivot <= 0
  // up to that rounding error, 36 * 2^-53 / (the smallest earlier pivot), or NaN
  double min_piv = 1.0;
  for (int k = 0; k < 6; ++k) {
    if (tid == 0) {
      double s = s_A[k * 6 + k];
      for (int m = 0; m < k; ++m) s -= s_L[k * 6 + m] * s_L[k * 6 + m];
      if (!(s > (36.0 * 0x1p-53) / min_piv)) s_bad = 1;
      min_piv = s < min_piv ? s : min_piv;
      s_L[k * 6 + k] = sqrt(s);
    }
    __syncthreads();
    if (tid > k && tid < 6) {
      double s = s_A[tid * 6 + k];
      for (int m = 0; m < k; ++m) s -= s_L[tid * 6 + m] * s_L[k * 6 + m];
      s_L[tid * 6 + k] = s / s_L[k * 6 + k];
    }
    __syncthreads();
  }
  // L^-1, one column per lane
  if (tid < 6) {
    const int j = tid;
    s_Li[j * 6 + j] = 1.0 / s_L[j * 6 + j];
    for (int i = j + 1; i < 6; ++i) {
      double s = 0.0;
      for (int m = j; m < i; ++m) s += s_L[i * 6 + m] * s_Li[m * 6 + j];
      s_Li[i * 6 + j] = -s / s_L[i * 6 + i];
    }
  }
  __syncthreads();
  double hinv = 0.0;
  if (el) {
    double s = 0.0;
    for (int m = hi; m < 6; ++m) s += s_Li[m * 6 + lo] * s_Li[m * 6 + hi];  // (S H S)^-1 = L^-T L^-1
    hinv = (s * s_d[lo]) * s_d[hi];
    if (!__builtin_isfinite(hinv)) s_bad = 1;
  }
  __syncthreads();
  if (tid == 0) {
    const int is_nan = a.d_is_nan ? *a.d_is_nan : 0;
    s_valid = (a.have_pose && !is_nan && n >= 3 && !bad && !s_bad) ? 1 : 0;
  }
  __syncthreads();
  const int valid = s_valid;
  if (el) {
    const double scale = a.sigma_px > 0.0 ? a.sigma_px * a.sigma_px : s_s2;
    s_Sig[tid] = valid ? scale * hinv : 0.0;
    // Ad(T10) = [[R, [t]x R], [0, R]] for the order [rho; phi]
    const int bi = ei / 3, bj = ej / 3, r = ei % 3, cc = ej % 3;
    double v = 0.0;
    if (bi == bj) {
      v = s_T10[r * 3 + cc];
    } else if (bi == 0) {
      const int r1 = (r + 1) % 3, r2 = (r + 2) % 3;
      v = s_T10[9 + r1] * s_T10[r2 * 3 + cc] - s_T10[9 + r2] * s_T10[r1 * 3 + cc];
    }
    s_Ad[tid] = v;
    s_P[tid] = a.prev ? a.prev->P[tid] : 0.0;
  }
  __syncthreads();
  if (el) {
    double s = 0.0;
    for (int m = 0; m < 6; ++m) s += s_Ad[ei * 6 + m] * s_P[m * 6 + ej];
    s_Tm[tid] = s;
  }
  __syncthreads();
  if (el) {
    double p = 0.0;
    if (a.prev) {
      for (int m = 0; m < 6; ++m) p += s_Tm[lo * 6 + m] * s_Ad[hi * 6 + m];
      p += s_Sig[lo * 6 + hi];
    }
    const double h = s_H[tid], sg = s_Sig[tid];
    a.out->H[tid] = h;
    a.out->Sigma[tid] = sg;
    a.out->P[tid] = p;
    if (a.out_host) {
      a.out_host->H[tid] = h;
      a.out_host->Sigma[tid] = sg;
      a.out_host->P[tid] = p;
    }
  }
  if (tid == 0) {
    const int unk = (a.prev ? a.prev->n_unknown_steps : 0) + (valid ? 0 : 1);
    const double s2 = valid ? s_s2 : 0.0;
    a.out->s2 = s2;
    a.out->valid = valid;
    a.out->n = n;
    a.out->n_unknown_steps = unk;
    a.out->pad_ = 0;
    if (a.out_host) {
      a.out_host->s2 = s2;
      a.out_host->valid = valid;
      a.out_host->n = n;
      a.out_host->n_unknown_steps = unk;
      a.out_host->pad_ = 0;
    }
  }
}

int vo_pose_cov_enqueue(vo_ctx *c, hipStream_t st, bool stereo, const float *dX, const float *dP1, const float *dP2, int n,
                        const int *d_n, const float Kl[4], const float Kr[4], const float T_lr[16], const float T01[16],
                        const float *d_T01, int have_pose, const int *d_is_nan, double sigma_px, const VoPoseCovBlock *prev,
                        VoPoseCovBlock *out, VoPoseCovBlock *out_host) {
  PcArgs a;
  memset(&a, 0, sizeof(a));
  a.X = dX;
  a.p1 = dP1;
  a.p2 = dP2;
  a.n = n;
  a.cap = c->cfg.max_points;
  a.d_n = d_n;
  for (int i = 0; i < 4; ++i) {
    a.Kl[i] = Kl[i];
    a.Kr[i] = Kr ? Kr[i] : Kl[i];
  }
  if (stereo) {  // T_rl = the SE(3) inverse of the f32 T_lr, in f64
    for (int i = 0; i < 3; ++i) {
      for (int j = 0; j < 3; ++j) a.Rrl[i * 3 + j] = (double)T_lr[j * 4 + i];
      a.trl[i] = -((a.Rrl[i * 3 + 0] * (double)T_lr[3] + a.Rrl[i * 3 + 1] * (double)T_lr[7]) + a.Rrl[i * 3 + 2] * (double)T_lr[11]);
    }
  }
  if (T01)
    memcpy(a.T01, T01, sizeof(a.T01));
  else
    for (int i = 0; i < 16; ++i) a.T01[i] = (i % 5 == 0) ? 1.0f : 0.0f;
  a.d_T01 = d_T01;
  a.have_pose = have_pose;
  a.d_is_nan = d_is_nan;
  a.sigma_px = sigma_px;
  a.prev = prev;
  a.out = out;
  a.out_host = out_host;
  const bool prof = st == c->stream;
  if (prof) vo_prof_begin(c, VO_K_AUX);
  if (stereo)
    hipLaunchKernelGGL(HIP_KERNEL_NAME(pose_cov_kernel<true>), dim3(1), dim3(PC_T), 0, st, a);
  else
    hipLaunchKernelGGL(HIP_KERNEL_NAME(pose_cov_kernel<false>), dim3(1), dim3(PC_T), 0, st, a);
  if (prof) vo_prof_end(c);
  VO_CHECK_HIP(c, hipGetLastError());
  return VO_OK;
}

// ---- operators: host arrays in, doubles out (like vo_gn_pose_*) -------------------------------------------------------
static int pc_operator(vo_ctx *c, bool stereo, const float *X, const float *p1, const float *p2, int n, const float Kl[4],
                       const float Kr[4], const float T_lr[16], const float T01[16], double sigma_px, double H[36],
                       double Sigma[36], double *s2, int *valid) {
  if (n < 0) VO_FAIL(c, VO_ERR_INVALID, "negative point count");
  if (n > c->cfg.max_points) VO_FAIL(c, VO_ERR_CAPACITY, "n=%d exceeds vo_config.max_points=%d", n, c->cfg.max_points);
  VO_CHECK_HIP(c, hipSetDevice(c->device));
  hipStream_t st = c->stream;
  if (n > 0) {
    VO_CHECK_HIP(c, hipMemcpyAsync(c->d_X, X, sizeof(float) * 3 * (size_t)n, hipMemcpyHostToDevice, st));
    VO_CHECK_HIP(c, hipMemcpyAsync(c->d_pts0, p1, sizeof(float) * 2 * (size_t)n, hipMemcpyHostToDevice, st));
    if (stereo) VO_CHECK_HIP(c, hipMemcpyAsync(c->d_pts1, p2, sizeof(float) * 2 * (size_t)n, hipMemcpyHostToDevice, st));
  }
  static_assert(sizeof(VoPoseCovBlock) <= 256 * sizeof(float), "the block lives in vo_ctx::d_mat");
  VoPoseCovBlock *d_blk = (VoPoseCovBlock *)c->d_mat;
  int rc = vo_pose_cov_enqueue(c, st, stereo, c->d_X, c->d_pts0, stereo ? c->d_pts1 : nullptr, n, nullptr, Kl, Kr, T_lr, T01,
                               nullptr, 1, nullptr, sigma_px, nullptr, d_blk, nullptr);
  if (rc) return rc;
  VoPoseCovBlock b;
  VO_CHECK_HIP(c, hipMemcpyAsync(&b, d_blk, sizeof(b), hipMemcpyDeviceToHost, st));
  VO_CHECK_HIP(c, hipStreamSynchronize(st));
  memcpy(H, b.H, sizeof(b.H));
  memcpy(Sigma, b.Sigma, sizeof(b.Sigma));
  *s2 = b.s2;
  *valid = b.valid;
  return VO_OK;
}

extern "C" int vo_gn_pose_information_stereo(vo_ctx *c, const float *X, const float *pts_l1, const float *pts_r1, int n,
                                             const float Kl[4], const float Kr[4], const float T_lr[16], const float T01[16],
                                             double sigma_px, double H[36], double Sigma[36], double *s2, int *valid) {
  if (!c || !X || !pts_l1 || !pts_r1 || !Kl || !Kr || !T_lr || !T01 || !H || !Sigma || !s2 || !valid) return VO_ERR_INVALID;
  return pc_operator(c, true, X, pts_l1, pts_r1, n, Kl, Kr, T_lr, T01, sigma_px, H, Sigma, s2, valid);
}

extern "C" int vo_gn_pose_information_mono(vo_ctx *c, const float *X, const float *pts1, int n, const float K[4],
                                           const float R01[9], const float t01[3], double sigma_px, double H[36],
                                           double Sigma[36], double *s2, int *valid) {
  if (!c || !X || !pts1 || !K || !R01 || !t01 || !H || !Sigma || !s2 || !valid) return VO_ERR_INVALID;
  const float T01[16] = {R01[0], R01[1], R01[2], t01[0], R01[3], R01[4], R01[5], t01[1],
                         R01[6], R01[7], R01[8], t01[2], 0, 0, 0, 1};
  return pc_operator(c, false, X, pts1, nullptr, n, K, K, nullptr, T01, sigma_px, H, Sigma, s2, valid);
}

// ---- the drivers' side ---------------------------------------------------------------------------------------------------
int vo_pose_cov_state_set(vo_ctx *c, VoPoseCovState *v, int on, double sigma_px) {
  if (!(sigma_px >= 0.0)) VO_FAIL(c, VO_ERR_INVALID, "sigma_px must be >= 0 (0: the a-posteriori variance)");
  VO_CHECK_HIP(c, hipSetDevice(c->device));
  if (on && !v->d_blk) {  // the option's only allocations
    VO_CHECK_HIP(c, vo_dev_malloc(c, (void **)&v->d_blk, 2 * sizeof(VoPoseCovBlock)));
    VO_CHECK_HIP(c, vo_host_malloc(c, (void **)&v->h_blk, sizeof(VoPoseCovBlock), hipHostMallocDefault));
    VO_CHECK_HIP(c, hipEventCreateWithFlags(&v->done, hipEventDisableTiming));
  }
  if (on) {  // the chain starts here: P = 0, no unknown steps
    VO_CHECK_HIP(c, hipMemsetAsync(v->d_blk, 0, 2 * sizeof(VoPoseCovBlock), c->stream_main));
    VO_CHECK_HIP(c, hipStreamSynchronize(c->stream_main));
    memset(v->h_blk, 0, sizeof(VoPoseCovBlock));
    v->cur = 0;
    v->sigma_px = sigma_px;
  }
  v->launched = false;
  v->on = on != 0;
  return VO_OK;
}

void vo_pose_cov_state_free(VoPoseCovState *v) {
  if (v->done) {
    (void)hipEventSynchronize(v->done);
    (void)hipEventDestroy(v->done);
  }
  if (v->d_blk) (void)hipFree(v->d_blk);
  if (v->h_blk) (void)hipHostFree(v->h_blk);
  *v = VoPoseCovState();
}

// Behind the frame's BA launch on the main stream: the next frame's BA launch comes later in the same stream, so it cannot
// overwrite the compacted set or the header under this launch. It reads the size of the BA set, the T01 and the flag the BA
// launch wrote on the device.
int vo_pose_cov_state_step(vo_ctx *c, VoPoseCovState *v, bool stereo, const float Kl[4], const float Kr[4], const float T_lr[16],
                           const float *carry_T01, const int *d_no_pose) {
  const VoPoseCovBlock *prev = v->d_blk + v->cur;
  VoPoseCovBlock *out = v->d_blk + (v->cur ^ 1);
  int rc;
  if (carry_T01) {
    rc = vo_pose_cov_enqueue(c, c->stream_main, stereo, nullptr, nullptr, nullptr, 0, nullptr, Kl, Kr, T_lr, carry_T01, nullptr, 0,
                             nullptr, v->sigma_px, prev, out, v->h_blk);
  } else {
    vo_frame_state *f = c->frame;
    if (!f || !f->hdr) VO_FAIL(c, VO_ERR_INVALID, "pose covariance: no frame operator has run");
    // (the size of the BA set in the frame's header: word 4 of the stereo frame, word 2 — n_ba — of the mono frame, whose gate
    // rewrites the counts behind the iterations)
    rc = vo_pose_cov_enqueue(c, c->stream_main, stereo, f->C_X, f->C_pl1, stereo ? f->C_pr1 : nullptr, 0, &f->hdr->cnt[stereo ? 4 : 2], Kl, Kr,
                             T_lr, nullptr, f->hdr->dT, 1, d_no_pose, v->sigma_px, prev, out, v->h_blk);
  }
  if (rc < 0) return rc;
  VO_CHECK_HIP(c, hipEventRecord(v->done, c->stream_main));
  v->launched = true;
  v->recoveries = c->frame_recoveries;
  return VO_OK;
}

int vo_pose_cov_state_get(vo_ctx *c, VoPoseCovState *v, double P[36], double Sigma_xi[36], double *s2, int *valid, int *n_points,
                          int *n_unknown_steps) {
  if (!v->on) VO_FAIL(c, VO_ERR_INVALID, "the pose covariance is off: vo_svo_set_pose_covariance / vo_mvo_set_pose_covariance");
  VO_CHECK_HIP(c, hipSetDevice(c->device));
  VO_CHECK_HIP(c, hipEventSynchronize(v->done));  // the last covariance launch only (before the first one: nothing)
  const VoPoseCovBlock &b = *v->h_blk;
  if (P) memcpy(P, b.P, sizeof(b.P));
  if (Sigma_xi) memcpy(Sigma_xi, b.Sigma, sizeof(b.Sigma));
  if (s2) *s2 = b.s2;
  if (valid) *valid = b.valid;
  if (n_points) *n_points = b.n;
  if (n_unknown_steps) *n_unknown_steps = b.n_unknown_steps;
  return VO_OK;
}

int vo_pose_cov_inputs(vo_ctx *c, bool stereo, float *X, float *pts_l, float *pts_r, int cap, int *n, float T01[16]) {
  *n = 0;
  vo_frame_state *f = c->frame;
  if (!f || !f->hdr) VO_FAIL(c, VO_ERR_INVALID, "no steady-state frame has run yet");
  VO_CHECK_HIP(c, hipSetDevice(c->device));
  VO_CHECK_HIP(c, hipStreamSynchronize(c->stream_main));
  vo_frame_hdr h;
  VO_CHECK_HIP(c, hipMemcpy(&h, f->hdr, sizeof(h), hipMemcpyDeviceToHost));
  const int m = h.cnt[stereo ? 4 : 2];
  *n = m;
  if (T01) memcpy(T01, h.dT, sizeof(float) * 16);
  if (m > cap && (X || pts_l || pts_r)) VO_FAIL(c, VO_ERR_CAPACITY, "%d points, room for %d", m, cap);
  if (m <= 0) return VO_OK;
  if (X) VO_CHECK_HIP(c, hipMemcpy(X, f->C_X, sizeof(float) * 3 * (size_t)m, hipMemcpyDeviceToHost));
  if (pts_l) VO_CHECK_HIP(c, hipMemcpy(pts_l, f->C_pl1, sizeof(float) * 2 * (size_t)m, hipMemcpyDeviceToHost));
  if (stereo && pts_r) VO_CHECK_HIP(c, hipMemcpy(pts_r, f->C_pr1, sizeof(float) * 2 * (size_t)m, hipMemcpyDeviceToHost));
  return VO_OK;
}
