// five_point.hip — MotionEstimator::calcPose5PointsAlgorithm (core/visual_odometry/motion_estimator.cpp:21-123, findCorrectRT
// :205-263) on the device: cv::findEssentialMat(pts0, pts1, K, RANSAC, confidence, thres) restated as a batched RANSAC whose
// selection follows the sequential rule of OpenCV's RANSACPointSetRegistrator, then the reference's own SVD decomposition
// and chirality test. Semantics: include/vo_hip.h (vo_five_point_*); design and measurements: DESIGN.md §10.
//
// Three launches per call, all on the context's main stream:
//   ep5_solve_kernel   one wavefront per sample: the sample's 5 indices (counter-based generator), the null space of the 5x9
//                      epipolar system, the 10x20 cubic constraints, Gauss-Jordan, Nister's hidden-variable 3x3 in z, the
//                      real roots of its degree-10 determinant, back substitution; at most 10 unit-norm models in double
//   ep5_score_kernel   (sample, block of points): Sampson errors of every model of the sample, inliers counted by ballot +
//                      popcount, one integer atomic per wavefront and model (order-free, so the counts are deterministic)
//   ep5_select_kernel  one workgroup: the sequential walk over the per-sample counts, E rounded to float, Eigen's 3x3
//                      JacobiSVD restated in f32, the four (R, t), mapping::triangulateDLT of every point under each, the
//                      chirality count, the mask and the record
#include <float.h>

#include <cmath>

#include <algorithm>
#include <vector>

#include "svo_device.hpp"
#include "vo_internal.hpp"

#define EP5_MAX_MODELS 10
#define EP5_MAX_ITERS 4096
#define EP5_DRAWS 256         // draws per sample before it is given up (repeats are rejected)
#define EP5_SCORE_THREADS 256
#define EP5_SCORE_PTS 1024    // points per score workgroup (4 per lane)
#define EP5_SELECT_THREADS 1024
#ifndef EP5_RES_TOL
#define EP5_RES_TOL 1e-8      // a root's unit-norm E is kept when every constraint residual is below this
#endif

enum { EP5_OK = 0, EP5_NO_MODEL = 1, EP5_NO_CHIRALITY = 2 };

struct Ep5Rec {  // device -> host result of one call (followed by the n mask bytes)
  int status;
  int n_inliers_5p, n_inliers, iterations, models, best_sample, best_model, n;
  float R[9], t[3], E[9];
  float pad[3];
};

struct vo_five_point {
  vo_ctx *c;
  vo_five_point_params prm;
  int max_points;
  void *d_in, *h_in;        // packed points: n x double4 (normalised x0, y0, x1, y1), then n x float4 (pixels u0, v0, u1, v1)
  double *d_models;         // [max_iters][10][9]
  int32_t *d_nmod;          // [max_iters]
  int32_t *d_sub;           // [max_iters][5]
  int32_t *d_cnt;           // [max_iters][10]
  void *d_out, *h_out;      // Ep5Rec + max_points mask bytes
  int last_samples;         // samples of the last vo_five_point_pose call
};

// ---- the sample stream (restated in numpy by tests/test_five_point_gpu.py) --------------------------------------------
__host__ __device__ static inline uint64_t ep5_mix(uint64_t z) {
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
__host__ __device__ static inline int ep5_draw(uint64_t seed, int s, int j, int n) {
  const uint64_t k = (uint64_t)s * EP5_DRAWS + (uint64_t)j;
  const uint64_t z = ep5_mix(seed + (k + 1) * 0x9E3779B97F4A7C15ull);
  return (int)(((z >> 32) * (uint64_t)n) >> 32);
}

// cubic monomials of (x, y, z, w = 1) in Nister's column order: x^3 y^3 x^2y xy^2 x^2z x^2 y^2z y^2 xyz xy | xz^2 xz x yz^2 yz
// y z^3 z^2 z 1, each as its sorted variable triple (0 = x, 1 = y, 2 = z, 3 = w)
__constant__ unsigned char EP5_CUBIC[20][3] = {{0, 0, 0}, {1, 1, 1}, {0, 0, 1}, {0, 1, 1}, {0, 0, 2}, {0, 0, 3}, {1, 1, 2},
                                               {1, 1, 3}, {0, 1, 2}, {0, 1, 3}, {0, 2, 2}, {0, 2, 3}, {0, 3, 3}, {1, 2, 2},
                                               {1, 2, 3}, {1, 3, 3}, {2, 2, 2}, {2, 2, 3}, {2, 3, 3}, {3, 3, 3}};
__constant__ unsigned char EP5_QUAD[10][2] = {{0, 0}, {0, 1}, {0, 2}, {0, 3}, {1, 1}, {1, 2}, {1, 3}, {2, 2}, {2, 3}, {3, 3}};
// the 2x2 minors of det E = E00 C0 - E01 C1 + E02 C2, as (a, b, c, d) of C = E_a E_b - E_c E_d
__constant__ unsigned char EP5_MINOR[3][4] = {{4, 8, 5, 7}, {3, 8, 5, 6}, {3, 7, 4, 6}};

__device__ static inline int ep5_pair(int a, int b) {  // index of the quadratic monomial v_a v_b (a <= b) in EP5_QUAD
  return a * 4 - (a * (a - 1)) / 2 + (b - a);
}
__device__ static inline int ep5_sym(int i, int j) {  // index of (EE^T)_ij, i <= j, in (00, 01, 02, 11, 12, 22)
  return i * 3 - (i * (i - 1)) / 2 + (j - i);
}

struct Ep5Lds {
  double N[4][9];       // orthonormal basis of the null space: E = x N0 + y N1 + z N2 + N3
  double E1[9][4];      // entry e of E as a linear polynomial in (x, y, z, w): E1[e][v] = N[v][e]
  double Q[5][9];       // epipolar system, reduced in place
  double P[6][10];      // (EE^T)_ij, i <= j, quadratic polynomials in (x, y, z, w)
  double T[10];         // tr(EE^T)
  double C[3][10];      // the three 2x2 minors of det E
  double A[10][20];     // the ten cubic constraints (det E, 2 EE^T E - tr(EE^T) E), Gauss-Jordan in place
  double A0[10][20];    // the same before the elimination: what a root is polished against
  double F[10];
  double B[3][3][5];    // Nister's hidden-variable matrix, entries polynomials in z (powers 0..4)
  double M[3][8];       // its 2x2 minors
  double D[2][11][11];  // [p(z) on [-1, 1], z^d p(1/z) on [-1, 1]][derivative order][coefficient]
  double R[2][12];      // roots of the current derivative level
  double amax[64];
  int idx[5];
  int piv[5];
  int deg, bad;
};

// coefficient of v_a v_b in L1 * L2 (linear polynomials in (x, y, z, w))
__device__ static inline double ep5_qprod(const double *L1, const double *L2, int a, int b) {
  return a == b ? L1[a] * L2[a] : L1[a] * L2[b] + L1[b] * L2[a];
}
// coefficient of v_a v_b v_c (a <= b <= c) in Qp * L (Qp quadratic, indexed by ep5_pair)
__device__ static inline double ep5_cprod(const double *Qp, const double *L, int a, int b, int c) {
  double r = Qp[ep5_pair(b, c)] * L[a];
  if (b != a) r += Qp[ep5_pair(a, c)] * L[b];
  if (c != b) r += Qp[ep5_pair(a, b)] * L[c];
  return r;
}
__device__ static inline double ep5_horner(const double *c, int deg, double x) {
  double f = c[deg];
  for (int i = deg - 1; i >= 0; --i) f = f * x + c[i];
  return f;
}

__device__ static inline double ep5_var(int a, double x, double y, double z) { return a == 0 ? x : (a == 1 ? y : (a == 2 ? z : 1.0)); }

// Gauss-Newton on the ten original cubic constraints in (x, y, z): two steps from the root found through the hidden variable
__device__ static void ep5_polish(const Ep5Lds &L, double &x, double &y, double &z) {
  for (int itn = 0; itn < 2; ++itn) {
    double r[10], J[10][3];
#pragma unroll
    for (int i = 0; i < 10; ++i) r[i] = J[i][0] = J[i][1] = J[i][2] = 0.0;
#pragma unroll 1
    for (int k = 0; k < 20; ++k) {
      const int a = EP5_CUBIC[k][0], b = EP5_CUBIC[k][1], c = EP5_CUBIC[k][2];
      const double va = ep5_var(a, x, y, z), vb = ep5_var(b, x, y, z), vc = ep5_var(c, x, y, z);
      const double m = va * vb * vc;
      double d[3];
#pragma unroll
      for (int u = 0; u < 3; ++u) d[u] = (a == u ? vb * vc : 0.0) + (b == u ? va * vc : 0.0) + (c == u ? va * vb : 0.0);
#pragma unroll
      for (int i = 0; i < 10; ++i) {
        const double q = L.A0[i][k];
        r[i] += q * m;
        J[i][0] += q * d[0];
        J[i][1] += q * d[1];
        J[i][2] += q * d[2];
      }
    }
    double N[3][3], g[3];
#pragma unroll
    for (int u = 0; u < 3; ++u) {
      g[u] = 0.0;
#pragma unroll
      for (int v = 0; v < 3; ++v) N[u][v] = 0.0;
#pragma unroll
      for (int i = 0; i < 10; ++i) {
        g[u] += J[i][u] * r[i];
#pragma unroll
        for (int v = 0; v < 3; ++v) N[u][v] += J[i][u] * J[i][v];
      }
    }
    const double c00 = N[1][1] * N[2][2] - N[1][2] * N[2][1], c01 = N[1][2] * N[2][0] - N[1][0] * N[2][2],
                 c02 = N[1][0] * N[2][1] - N[1][1] * N[2][0];
    const double det = N[0][0] * c00 + N[0][1] * c01 + N[0][2] * c02;
    if (!(fabs(det) > 0.0) || !isfinite(det)) return;
    // delta = -N^-1 g (N symmetric: the adjugate by cofactors)
    const double c11 = N[0][0] * N[2][2] - N[0][2] * N[2][0], c12 = N[0][1] * N[2][0] - N[0][0] * N[2][1];
    const double c22 = N[0][0] * N[1][1] - N[0][1] * N[1][0];
    const double dx = -(c00 * g[0] + c01 * g[1] + c02 * g[2]) / det;
    const double dy = -(c01 * g[0] + c11 * g[1] + c12 * g[2]) / det;
    const double dz = -(c02 * g[0] + c12 * g[1] + c22 * g[2]) / det;
    if (!isfinite(dx) || !isfinite(dy) || !isfinite(dz)) return;
    x += dx;
    y += dy;
    z += dz;
  }
}

// unit-Frobenius E = x N0 + y N1 + z N2 + N3 and its largest constraint residual (five epipolar, det E, 2 EE^T E - tr(EE^T) E)
__device__ static double ep5_model(const Ep5Lds &L, const double4 *norm, double x, double y, double z, double (&E)[9]) {
  double nn = 0.0;
#pragma unroll
  for (int e = 0; e < 9; ++e) {
    E[e] = ((x * L.N[0][e] + y * L.N[1][e]) + z * L.N[2][e]) + L.N[3][e];
    nn += E[e] * E[e];
  }
  nn = sqrt(nn);
#pragma unroll
  for (int e = 0; e < 9; ++e) E[e] /= nn;
  double res = 0.0;
  for (int q = 0; q < 5; ++q) {
    const double4 p = norm[L.idx[q]];
    const double e0 = (E[0] * p.x + E[1] * p.y) + E[2], e1 = (E[3] * p.x + E[4] * p.y) + E[5], e2 = (E[6] * p.x + E[7] * p.y) + E[8];
    res = fmax(res, fabs((p.z * e0 + p.w * e1) + e2));
  }
  const double det = E[0] * (E[4] * E[8] - E[5] * E[7]) - E[1] * (E[3] * E[8] - E[5] * E[6]) + E[2] * (E[3] * E[7] - E[4] * E[6]);
  res = fmax(res, fabs(det));
  double EEt[9];
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) EEt[i * 3 + j] = (E[i * 3] * E[j * 3] + E[i * 3 + 1] * E[j * 3 + 1]) + E[i * 3 + 2] * E[j * 3 + 2];
  const double tr = (EEt[0] + EEt[4]) + EEt[8];
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      const double v = (EEt[i * 3] * E[j] + EEt[i * 3 + 1] * E[3 + j]) + EEt[i * 3 + 2] * E[6 + j];
      res = fmax(res, fabs(2.0 * v - tr * E[i * 3 + j]));
    }
  return isfinite(res) ? res : 1e300;
}

struct Ep5SolveArgs {
  const double4 *norm;
  int n, mode;  // mode 0: the generator; 1: sample s = points 5s .. 5s + 4
  unsigned long long seed;
  double *models;
  int32_t *n_models, *subsets, *counts;
};

// One wavefront per sample. Everything indexed at run time lives in LDS (no scratch).
__global__ __launch_bounds__(64) void ep5_solve_kernel(Ep5SolveArgs a) {
  __shared__ Ep5Lds L;
  const int lane = threadIdx.x;
  const int s = blockIdx.x;
  if (lane < EP5_MAX_MODELS) a.counts[(size_t)s * EP5_MAX_MODELS + lane] = 0;
  if (lane == 0) {
    int k = 0;
    if (a.mode == 1) {
      for (; k < 5; ++k) L.idx[k] = 5 * s + k;
    } else {
      for (int j = 0; j < EP5_DRAWS && k < 5; ++j) {
        const int v = ep5_draw(a.seed, s, j, a.n);
        bool dup = false;
        for (int q = 0; q < k; ++q) dup |= L.idx[q] == v;
        if (!dup) L.idx[k++] = v;
      }
    }
    for (int q = 0; q < 5; ++q) a.subsets[(size_t)s * 5 + q] = q < k ? L.idx[q] : -1;
    L.bad = k < 5;
  }
  __syncthreads();
  if (L.bad) {
    if (lane == 0) a.n_models[s] = 0;
    return;
  }
  // 5 x 9 epipolar rows: x1^T E x0 = sum_ij x1_i x0_j E_ij
  if (lane < 45) {
    const int r = lane / 9, c = lane % 9;
    const double4 p = a.norm[L.idx[r]];
    const double u1[3] = {p.z, p.w, 1.0}, u0[3] = {p.x, p.y, 1.0};
    const int i = c / 3, j = c % 3;
    const double xi = i == 0 ? u1[0] : (i == 1 ? u1[1] : u1[2]);
    const double xj = j == 0 ? u0[0] : (j == 1 ? u0[1] : u0[2]);
    L.Q[r][c] = xi * xj;
  }
  __syncthreads();
  // null space: Gauss-Jordan with complete pivoting (lane 0), basis of the four free columns, Gram-Schmidt twice
  if (lane == 0) {
    double qmax = 0.0;
    for (int r = 0; r < 5; ++r)
      for (int c = 0; c < 9; ++c) qmax = fmax(qmax, fabs(L.Q[r][c]));
    unsigned used = 0;
    int bad = !(qmax > 0.0) || !isfinite(qmax);
    for (int r = 0; r < 5 && !bad; ++r) {
      int pr = r, pc = -1;
      double best = 0.0;
      for (int i = r; i < 5; ++i)
        for (int c = 0; c < 9; ++c)
          if (!(used & (1u << c)) && fabs(L.Q[i][c]) > best) {
            best = fabs(L.Q[i][c]);
            pr = i;
            pc = c;
          }
      if (pc < 0 || best <= 1e-11 * qmax) {
        bad = 1;
        break;
      }
      for (int c = 0; c < 9; ++c) {
        const double t = L.Q[r][c];
        L.Q[r][c] = L.Q[pr][c];
        L.Q[pr][c] = t;
      }
      const double pv = L.Q[r][pc];
      for (int c = 0; c < 9; ++c) L.Q[r][c] /= pv;
      for (int i = 0; i < 5; ++i)
        if (i != r) {
          const double f = L.Q[i][pc];
          for (int c = 0; c < 9; ++c) L.Q[i][c] -= f * L.Q[r][c];
        }
      used |= 1u << pc;
      L.piv[r] = pc;
    }
    if (!bad) {
      int b = 0;
      for (int f = 0; f < 9; ++f) {
        if (used & (1u << f)) continue;
        for (int c = 0; c < 9; ++c) L.N[b][c] = 0.0;
        L.N[b][f] = 1.0;
        for (int r = 0; r < 5; ++r) L.N[b][L.piv[r]] = -L.Q[r][f];
        ++b;
      }
      for (int pass = 0; pass < 2; ++pass)
        for (int b0 = 0; b0 < 4; ++b0) {
          for (int b1 = 0; b1 < b0; ++b1) {
            double d = 0.0;
            for (int c = 0; c < 9; ++c) d += L.N[b0][c] * L.N[b1][c];
            for (int c = 0; c < 9; ++c) L.N[b0][c] -= d * L.N[b1][c];
          }
          double nn = 0.0;
          for (int c = 0; c < 9; ++c) nn += L.N[b0][c] * L.N[b0][c];
          nn = sqrt(nn);
          for (int c = 0; c < 9; ++c) L.N[b0][c] /= nn;
        }
    }
    L.bad = bad;
  }
  __syncthreads();
  if (L.bad) {
    if (lane == 0) a.n_models[s] = 0;
    return;
  }
  if (lane < 36) L.E1[lane >> 2][lane & 3] = L.N[lane & 3][lane >> 2];
  __syncthreads();
#define EP5_LIN(e, out) const double *out = L.E1[e];
  if (lane < 60) {  // (EE^T)_ij = sum_k E_ik E_jk
    const int pi = lane / 10, m = lane % 10;
    const int i = pi < 3 ? 0 : (pi < 5 ? 1 : 2);
    const int j = pi < 3 ? pi : (pi < 5 ? pi - 2 : 2);
    const int qa = EP5_QUAD[m][0], qb = EP5_QUAD[m][1];
    double v = 0.0;
    for (int k = 0; k < 3; ++k) {
      EP5_LIN(3 * i + k, l1)
      EP5_LIN(3 * j + k, l2)
      v += ep5_qprod(l1, l2, qa, qb);
    }
    L.P[pi][m] = v;
  }
  if (lane < 30) {
    const int mi = lane / 10, m = lane % 10;
    const int qa = EP5_QUAD[m][0], qb = EP5_QUAD[m][1];
    EP5_LIN(EP5_MINOR[mi][0], l0)
    EP5_LIN(EP5_MINOR[mi][1], l1)
    EP5_LIN(EP5_MINOR[mi][2], l2)
    EP5_LIN(EP5_MINOR[mi][3], l3)
    L.C[mi][m] = ep5_qprod(l0, l1, qa, qb) - ep5_qprod(l2, l3, qa, qb);
  }
  __syncthreads();
  if (lane < 10) L.T[lane] = (L.P[0][lane] + L.P[3][lane]) + L.P[5][lane];
  __syncthreads();
  double amax = 0.0;
  for (int t = lane; t < 200; t += 64) {
    const int r = t / 20, col = t % 20;
    const int ca = EP5_CUBIC[col][0], cb = EP5_CUBIC[col][1], cc = EP5_CUBIC[col][2];
    double v;
    if (r == 0) {
      EP5_LIN(0, e0)
      EP5_LIN(1, e1)
      EP5_LIN(2, e2)
      v = (ep5_cprod(L.C[0], e0, ca, cb, cc) - ep5_cprod(L.C[1], e1, ca, cb, cc)) + ep5_cprod(L.C[2], e2, ca, cb, cc);
    } else {
      const int i = (r - 1) / 3, j = (r - 1) % 3;
      v = 0.0;
      for (int k = 0; k < 3; ++k) {
        EP5_LIN(3 * k + j, ekj)
        v += 2.0 * ep5_cprod(L.P[ep5_sym(i < k ? i : k, i < k ? k : i)], ekj, ca, cb, cc);
      }
      EP5_LIN(3 * i + j, eij)
      v -= ep5_cprod(L.T, eij, ca, cb, cc);
    }
    L.A[r][col] = L.A0[r][col] = v;
    amax = fmax(amax, fabs(v));
  }
#undef EP5_LIN
  L.amax[lane] = amax;
  __syncthreads();
  if (lane == 0) {
    double m = 0.0;
    for (int i = 0; i < 64; ++i) m = fmax(m, L.amax[i]);
    L.amax[0] = m;
  }
  __syncthreads();
  const double tol = 1e-13 * L.amax[0];
  // Gauss-Jordan on the first ten columns, partial pivoting over rows; lanes own columns
  for (int c = 0; c < 10; ++c) {
    int p = c;
    double best = fabs(L.A[c][c]);
    for (int r = c + 1; r < 10; ++r) {
      const double v = fabs(L.A[r][c]);
      if (v > best) {
        best = v;
        p = r;
      }
    }
    if (!(best > tol)) {  // (every lane read the same LDS: a uniform exit)
      if (lane == 0) a.n_models[s] = 0;
      return;
    }
    const double pv = L.A[p][c];
    __syncthreads();
    if (lane < 20) {
      const double t0 = L.A[c][lane], t1 = L.A[p][lane];
      L.A[p][lane] = t0;
      L.A[c][lane] = t1 / pv;
    }
    __syncthreads();
    if (lane < 10) L.F[lane] = lane == c ? 0.0 : L.A[lane][c];
    __syncthreads();
    if (lane < 20) {
      const double pc = L.A[c][lane];
      for (int r = 0; r < 10; ++r) L.A[r][lane] -= L.F[r] * pc;
    }
    __syncthreads();
  }
  // rows e..j = 4..9 pair up as (x^2 z, x^2), (y^2 z, y^2), (xyz, xy): <e> - z <f> leaves x (cubic in z) + y (cubic) + 1 (quartic)
  if (lane < 9) {
    const int b = lane / 3, part = lane % 3;
    const int r1 = 4 + 2 * b, r2 = r1 + 1;
    double e[4], f[4];  // coefficients by power of z
    if (part < 2) {
      const int base = part == 0 ? 10 : 13;
      e[0] = L.A[r1][base + 2], e[1] = L.A[r1][base + 1], e[2] = L.A[r1][base], e[3] = 0.0;
      f[0] = L.A[r2][base + 2], f[1] = L.A[r2][base + 1], f[2] = L.A[r2][base], f[3] = 0.0;
    } else {
      e[0] = L.A[r1][19], e[1] = L.A[r1][18], e[2] = L.A[r1][17], e[3] = L.A[r1][16];
      f[0] = L.A[r2][19], f[1] = L.A[r2][18], f[2] = L.A[r2][17], f[3] = L.A[r2][16];
    }
    L.B[b][part][0] = e[0];
    L.B[b][part][1] = e[1] - f[0];
    L.B[b][part][2] = e[2] - f[1];
    L.B[b][part][3] = e[3] - f[2];
    L.B[b][part][4] = -f[3];
  }
  __syncthreads();
  if (lane < 24) {  // M0 = B11 B22 - B12 B21, M1 = B10 B22 - B12 B20, M2 = B10 B21 - B11 B20
    const int mi = lane / 8, k = lane % 8;
    const int c0 = mi == 0 ? 1 : 0, c1 = mi == 2 ? 1 : 2;
    double v = 0.0;
    for (int i = k > 4 ? k - 4 : 0; i <= (k < 4 ? k : 4); ++i)
      v += L.B[1][c0][i] * L.B[2][c1][k - i] - L.B[1][c1][i] * L.B[2][c0][k - i];
    L.M[mi][k] = v;
  }
  __syncthreads();
  if (lane < 11) {  // det B = B00 M0 - B01 M1 + B02 M2, degree <= 10
    const int k = lane;
    double v = 0.0;
    for (int i = k > 7 ? k - 7 : 0; i <= (k < 4 ? k : 4); ++i)
      v += (L.B[0][0][i] * L.M[0][k - i] - L.B[0][1][i] * L.M[1][k - i]) + L.B[0][2][i] * L.M[2][k - i];
    L.D[0][0][k] = v;
  }
  __syncthreads();
  if (lane == 0) {
    double m = 0.0;
    int d = -1;
    for (int k = 0; k <= 10; ++k) {
      m = fmax(m, fabs(L.D[0][0][k]));
      if (L.D[0][0][k] != 0.0) d = k;
    }
    L.deg = (isfinite(m) && m > 0.0) ? d : -1;
    if (L.deg > 0)
      for (int k = 0; k <= 10; ++k) L.D[0][0][k] /= m;
  }
  __syncthreads();
  const int deg = L.deg;
  if (deg <= 0) {
    if (lane == 0) a.n_models[s] = 0;
    return;
  }
  // real roots: p on [-1, 1] (lanes 0..31) and its reversal q(w) = w^d p(1/w) on [-1, 1] (lanes 32..63, roots |w| < 1 give
  // z = 1/w). The roots of every derivative separate those of the level below: each interval between consecutive roots of
  // p^(k+1) holds at most one root of p^(k), found by bisection on a sign change to full double precision.
  const int h = lane >> 5, li = lane & 31;
  if (h == 1 && li <= deg) L.D[1][0][li] = L.D[0][0][deg - li];
  __syncthreads();
  for (int k = 1; k < deg; ++k)
    if (li <= deg - k) {
      double f = 1.0;
      for (int t = 0; t < k; ++t) f *= (double)(li + k - t);
      L.D[h][k][li] = L.D[h][0][li + k] * f;
    }
  __syncthreads();
  int nr = 0;
  const unsigned long long half = h ? 0xFFFFFFFF00000000ull : 0x00000000FFFFFFFFull;
  const unsigned long long below = (1ull << lane) - 1ull;
  for (int k = deg - 1; k >= 0; --k) {
    const int dk = deg - k;
    const double *cf = L.D[h][k];
    bool has = false;
    double r = 0.0;
    if (li <= nr) {
      double lo = li == 0 ? -1.0 : L.R[h][li - 1];
      double hi = li == nr ? 1.0 : L.R[h][li];
      double flo = ep5_horner(cf, dk, lo), fhi = ep5_horner(cf, dk, hi);
      // a root in (lo, hi]: a zero at lo belongs to the interval on its left
      has = flo < 0.0 ? fhi >= 0.0 : (flo > 0.0 ? fhi <= 0.0 : false);
      if (has) {
        if (fhi == 0.0) {
          r = hi;
        } else {
          for (int it = 0; it < 100; ++it) {
            const double mid = lo + 0.5 * (hi - lo);
            if (!(mid > lo && mid < hi)) break;
            const double fm = ep5_horner(cf, dk, mid);
            if (fm == 0.0) {
              lo = hi = mid;
              break;
            }
            if ((fm < 0.0) == (flo < 0.0)) {
              lo = mid;
              flo = fm;
            } else {
              hi = mid;
            }
          }
          r = lo + 0.5 * (hi - lo);
        }
      }
    }
    const unsigned long long bal = __ballot(has);
    __syncthreads();
    if (has) L.R[h][__popcll(bal & half & below)] = r;
    nr = __popcll(bal & half);
    __syncthreads();
  }
  // candidates: roots of p in [-1, 1] ascending, then roots of q with 0 < |w| < 1 ascending in w
  bool cand = false;
  double z = 0.0;
  if (li < nr) {
    const double v = L.R[h][li];
    if (h == 0) {
      cand = true;
      z = v;
    } else if (v != 0.0 && fabs(v) < 1.0) {
      cand = true;
      z = 1.0 / v;
    }
  }
  double E[9];
  bool keep = false;
  if (cand) {
    double Bz[3][3];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int j = 0; j < 3; ++j) Bz[i][j] = ep5_horner(L.B[i][j], 4, z);
    // (x, y, 1) is the null vector of B(z): the cross product of the two rows that give the largest third component
    double cr[3][3];
#pragma unroll
    for (int q = 0; q < 3; ++q) {
      const int r0 = q == 2 ? 1 : 0, r1 = q == 0 ? 1 : 2;
      cr[q][0] = Bz[r0][1] * Bz[r1][2] - Bz[r0][2] * Bz[r1][1];
      cr[q][1] = Bz[r0][2] * Bz[r1][0] - Bz[r0][0] * Bz[r1][2];
      cr[q][2] = Bz[r0][0] * Bz[r1][1] - Bz[r0][1] * Bz[r1][0];
    }
    double cx = cr[0][0], cy = cr[0][1], cw = cr[0][2];
#pragma unroll
    for (int q = 1; q < 3; ++q)
      if (fabs(cr[q][2]) > fabs(cw)) cx = cr[q][0], cy = cr[q][1], cw = cr[q][2];
    const double x = cx / cw, y = cy / cw;
    double px = x, py = y, pz = z, E2[9];
    ep5_polish(L, px, py, pz);
    double res = ep5_model(L, a.norm, x, y, z, E);
    const double res2 = ep5_model(L, a.norm, px, py, pz, E2);
    if (res2 < res) {  // (the polished root only where it is better)
      res = res2;
#pragma unroll
      for (int e = 0; e < 9; ++e) E[e] = E2[e];
    }
    keep = res <= EP5_RES_TOL;
  }
  const unsigned long long kb = __ballot(keep);
  const int slot = __popcll(kb & below);
  if (keep && slot < EP5_MAX_MODELS) {
    double *o = a.models + ((size_t)s * EP5_MAX_MODELS + slot) * 9;
#pragma unroll
    for (int e = 0; e < 9; ++e) o[e] = E[e];
  }
  if (lane == 0) a.n_models[s] = min(__popcll(kb), EP5_MAX_MODELS);
}

// Sampson error of OpenCV's EMEstimatorCallback::computeError, in double, rounded to float
__device__ static inline float ep5_sampson(const double (&E)[9], double x0, double y0, double x1, double y1) {
  const double a = (E[0] * x0 + E[1] * y0) + E[2];
  const double b = (E[3] * x0 + E[4] * y0) + E[5];
  const double c = (E[6] * x0 + E[7] * y0) + E[8];
  const double d = (E[0] * x1 + E[3] * y1) + E[6];
  const double e = (E[1] * x1 + E[4] * y1) + E[7];
  const double r = (x1 * a + y1 * b) + c;
  return (float)((r * r) / (((a * a + b * b) + d * d) + e * e));
}

__global__ __launch_bounds__(EP5_SCORE_THREADS) void ep5_score_kernel(const double4 *norm, int n, const double *models,
                                                                      const int32_t *n_models, int32_t *counts, float thr) {
  const int s = blockIdx.y;
  const int nm = n_models[s];
  if (nm <= 0) return;
  constexpr int PER = EP5_SCORE_PTS / EP5_SCORE_THREADS;
  double4 P[PER];
  bool ok[PER];
#pragma unroll
  for (int q = 0; q < PER; ++q) {
    const int i = blockIdx.x * EP5_SCORE_PTS + q * EP5_SCORE_THREADS + (int)threadIdx.x;
    ok[q] = i < n;
    P[q] = ok[q] ? norm[i] : make_double4(0.0, 0.0, 0.0, 0.0);
  }
  for (int m = 0; m < nm; ++m) {
    const double *Em = models + ((size_t)s * EP5_MAX_MODELS + m) * 9;
    double E[9];
#pragma unroll
    for (int e = 0; e < 9; ++e) E[e] = Em[e];
    int cnt = 0;
#pragma unroll
    for (int q = 0; q < PER; ++q) {
      const bool in = ok[q] && ep5_sampson(E, P[q].x, P[q].y, P[q].z, P[q].w) <= thr;
      cnt += __popcll(__ballot(in));
    }
    if ((threadIdx.x & 63) == 0 && cnt) atomicAdd(&counts[(size_t)s * EP5_MAX_MODELS + m], cnt);
  }
}

// OpenCV's RANSACUpdateNumIters(p, ep, 5, niters); (1 - ep)^5 as ((q q)(q q)) q
__device__ static int ep5_update_iters(double p, double ep, int niters) {
  p = fmin(fmax(p, 0.0), 1.0);
  ep = fmin(fmax(ep, 0.0), 1.0);
  double num = fmax(1.0 - p, DBL_MIN);
  const double q = 1.0 - ep, q2 = q * q;
  double den = 1.0 - (q2 * q2) * q;
  if (den < DBL_MIN) return 0;
  num = log(num);
  den = log(den);
  return (den >= 0.0 || -num >= (double)niters * (-den)) ? niters : (int)rint(num / den);
}

// Eigen::JacobiSVD<Matrix3f>(E, ComputeFullU | ComputeFullV) of Eigen 3.4 (no preconditioner for a square matrix): the
// sweeps of svo_svd4_nullvec with U accumulated, signs made positive, singular values sorted descending
__device__ static void ep5_svd3(const float (&M)[9], float (&U)[9], float (&V)[9]) {
  const float FMIN = 1.17549435e-38f, FEPS = 1.1920929e-07f, FMAX = 3.40282347e+38f;
  float W[9];
  float scale = 0.0f;
  bool finite = true;
#pragma unroll
  for (int i = 0; i < 9; ++i) {
    const float a = fabsf(M[i]);
    if (!(a <= FMAX)) finite = false;
    if (a > scale) scale = a;
    U[i] = V[i] = (i % 4 == 0) ? 1.0f : 0.0f;
  }
  if (!finite) return;
  if (scale == 0.0f) scale = 1.0f;
#pragma unroll
  for (int i = 0; i < 9; ++i) W[i] = M[i] / scale;
  const float precision = 2.0f * FEPS;
  float max_diag = 0.0f;
#pragma unroll
  for (int i = 0; i < 3; ++i)
    if (fabsf(W[i * 4]) > max_diag) max_diag = fabsf(W[i * 4]);
  for (int sweeps = 1;; ++sweeps) {
    bool finished = true;
#pragma unroll
    for (int p = 1; p < 3; ++p)
#pragma unroll
      for (int q = 0; q < p; ++q) {
        const float pm = precision * max_diag;
        const float threshold = FMIN > pm ? FMIN : pm;
        if (fabsf(W[p * 3 + q]) > threshold || fabsf(W[q * 3 + p]) > threshold) {
          finished = false;
          float m00 = W[p * 3 + p], m01 = W[p * 3 + q], m10 = W[q * 3 + p], m11 = W[q * 3 + q];
          float c1, s1;
          const float t = m00 + m11;
          const float d = m10 - m01;
          if (fabsf(d) < FMIN) {
            s1 = 0.0f;
            c1 = 1.0f;
          } else {
            const float u = t / d;
            const float tmp = sqrtf(1.0f + u * u);
            s1 = 1.0f / tmp;
            c1 = u / tmp;
          }
          if (!(c1 == 1.0f && s1 == 0.0f)) {
            svo_rot(m00, m10, c1, s1);
            svo_rot(m01, m11, c1, s1);
          }
          float cr, sr;
          const float deno = 2.0f * fabsf(m01);
          if (deno < FMIN) {
            cr = 1.0f;
            sr = 0.0f;
          } else {
            const float tau = (m00 - m11) / deno;
            const float w = sqrtf(tau * tau + 1.0f);
            float tt;
            if (tau > 0.0f)
              tt = 1.0f / (tau + w);
            else
              tt = 1.0f / (tau - w);
            const float sign_t = tt > 0.0f ? 1.0f : -1.0f;
            const float n = 1.0f / sqrtf(tt * tt + 1.0f);
            sr = -sign_t * (m01 / fabsf(m01)) * fabsf(tt) * n;
            cr = n;
          }
          const float ct = cr, st = -sr;
          const float cl = c1 * ct - s1 * st;
          const float sl = c1 * st + s1 * ct;
          if (!(cl == 1.0f && sl == 0.0f)) {  // W.applyOnTheLeft(p, q, j_left); U.applyOnTheRight(p, q, j_left^T)
#pragma unroll
            for (int k = 0; k < 3; ++k) svo_rot(W[p * 3 + k], W[q * 3 + k], cl, sl);
#pragma unroll
            for (int k = 0; k < 3; ++k) svo_rot(U[k * 3 + p], U[k * 3 + q], cl, sl);
          }
          if (!(ct == 1.0f && st == 0.0f)) {  // W.applyOnTheRight(p, q, j_right); V.applyOnTheRight(p, q, j_right)
#pragma unroll
            for (int k = 0; k < 3; ++k) svo_rot(W[k * 3 + p], W[k * 3 + q], ct, st);
#pragma unroll
            for (int k = 0; k < 3; ++k) svo_rot(V[k * 3 + p], V[k * 3 + q], ct, st);
          }
          const float a = fabsf(W[p * 3 + p]), b = fabsf(W[q * 3 + q]);
          const float mx = a > b ? a : b;
          if (mx > max_diag) max_diag = mx;
        }
      }
    if (finished || sweeps > 1000) break;
  }
  float sv[3];
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    const float a = W[i * 4];
    sv[i] = fabsf(a);
    if (a < 0.0f) {
#pragma unroll
      for (int k = 0; k < 3; ++k) U[k * 3 + i] = -U[k * 3 + i];
    }
  }
#pragma unroll
  for (int i = 0; i < 3; ++i) sv[i] *= scale;
  bool stop = false;
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    int pos = i;
    float best = sv[i];
#pragma unroll
    for (int k = i + 1; k < 3; ++k)
      if (sv[k] > best) {
        best = sv[k];
        pos = k;
      }
    if (best == 0.0f) stop = true;
    if (!stop) {
#pragma unroll
      for (int k = i + 1; k < 3; ++k)
        if (pos == k) {
          const float ts = sv[i];
          sv[i] = sv[k];
          sv[k] = ts;
#pragma unroll
          for (int r = 0; r < 3; ++r) {
            float tu = U[r * 3 + i];
            U[r * 3 + i] = U[r * 3 + k];
            U[r * 3 + k] = tu;
            tu = V[r * 3 + i];
            V[r * 3 + i] = V[r * 3 + k];
            V[r * 3 + k] = tu;
          }
        }
    }
  }
}

__device__ static inline float ep5_dot3(float a0, float b0, float a1, float b1, float a2, float b2) { return a0 * b0 + (a1 * b1 + a2 * b2); }
__device__ static inline float ep5_det3(const float (&m)[9]) {  // Eigen's 3x3 determinant
  return m[0] * (m[4] * m[8] - m[5] * m[7]) - m[3] * (m[1] * m[8] - m[2] * m[7]) + m[6] * (m[1] * m[5] - m[2] * m[4]);
}

struct Ep5SelectArgs {
  const double4 *norm;
  const float4 *pix;
  int n, S, single;
  const double *models;
  const int32_t *n_models, *counts;
  float thr;
  double confidence;
  int max_iters;
  float K[4];
  uint8_t *mask;
  Ep5Rec *rec;
};

__global__ __launch_bounds__(EP5_SELECT_THREADS) void ep5_select_kernel(Ep5SelectArgs a) {
  __shared__ int sbest[EP5_MAX_ITERS];
  __shared__ SvoCam cams[4];
  __shared__ float Ef[9];
  __shared__ int dec[8];  // best sample, best model, iterations, status, best candidate
  __shared__ int cnt[8];  // chirality counts [4], mask_5p count, final count, models evaluated
  const int tid = threadIdx.x;
  if (tid < 8) cnt[tid] = 0;
  for (int s = tid; s < a.S; s += EP5_SELECT_THREADS) {  // per sample: (count << 4 | model) of the first model of the largest count
    const int nm = a.n_models[s];
    int best = -1, bm = 0;
    for (int m = 0; m < nm; ++m) {
      const int c = a.counts[(size_t)s * EP5_MAX_MODELS + m];
      if (c > best) {
        best = c;
        bm = m;
      }
    }
    sbest[s] = nm > 0 ? (best << 4 | bm) : -1;
  }
  __syncthreads();
  if (tid == 0) {
    int bs = -1, bmod = 0, it = 0;
    if (a.single) {
      if (a.n_models[0] > 0) bs = 0;
      it = 1;
    } else {
      // the sequential rule: samples in order, within a sample the models in solver order; the first model of the sample's
      // largest count is the one the walk over all of its models would keep, and RANSACUpdateNumIters applied to it alone
      // gives the same niters as applied after every intermediate replacement (its estimate only falls as the count rises)
      int niters = a.max_iters, best = -1;
      while (it < a.S) {
        const int v = sbest[it];
        if (v >= 0) {
          const int c = v >> 4;
          if (c > max(best, 4)) {
            best = c;
            bs = it;
            bmod = v & 15;
            niters = ep5_update_iters(a.confidence, (double)(a.n - best) / (double)a.n, niters);
          }
        }
        ++it;
        if (it >= niters) break;
      }
    }
    dec[0] = bs;
    dec[1] = bmod;
    dec[2] = it;
    dec[3] = bs < 0 ? EP5_NO_MODEL : EP5_OK;
    if (bs >= 0) {
      float e[9], U[9], V[9];
      const double *Em = a.models + ((size_t)bs * EP5_MAX_MODELS + bmod) * 9;
#pragma unroll
      for (int i = 0; i < 9; ++i) Ef[i] = e[i] = (float)Em[i];  // cv::cv2eigen into Mat33
      ep5_svd3(e, U, V);
      if (ep5_det3(U) < 0.0f)
#pragma unroll
        for (int r = 0; r < 3; ++r) U[r * 3 + 2] = -U[r * 3 + 2];
      if (ep5_det3(V) < 0.0f)
#pragma unroll
        for (int r = 0; r < 3; ++r) V[r * 3 + 2] = -V[r * 3 + 2];
      // R0 = R1 = U W V^T, R2 = R3 = U W^T V^T, t0 = t2 = U.col(2), t1 = t3 = -t0 (motion_estimator.cpp:79-102)
      const float Wm[9] = {0.0f, -1.0f, 0.0f, 1.0f, 0.0f, 0.0f, 0.0f, 0.0f, 1.0f};
      const float Km[9] = {a.K[0], 0.0f, a.K[2], 0.0f, a.K[1], a.K[3], 0.0f, 0.0f, 1.0f};
#pragma unroll
      for (int w = 0; w < 2; ++w) {
        float UW[9], R[9];
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
          for (int j = 0; j < 3; ++j) {
            const float w0 = w == 0 ? Wm[0 * 3 + j] : Wm[j * 3 + 0];
            const float w1 = w == 0 ? Wm[1 * 3 + j] : Wm[j * 3 + 1];
            const float w2 = w == 0 ? Wm[2 * 3 + j] : Wm[j * 3 + 2];
            UW[i * 3 + j] = ep5_dot3(U[i * 3 + 0], w0, U[i * 3 + 1], w1, U[i * 3 + 2], w2);
          }
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
          for (int j = 0; j < 3; ++j) R[i * 3 + j] = ep5_dot3(UW[i * 3 + 0], V[j * 3 + 0], UW[i * 3 + 1], V[j * 3 + 1], UW[i * 3 + 2], V[j * 3 + 2]);
#pragma unroll
        for (int sg = 0; sg < 2; ++sg) {
          SvoCam &cam = cams[2 * w + sg];
#pragma unroll
          for (int i = 0; i < 9; ++i) cam.R10[i] = R[i];
#pragma unroll
          for (int i = 0; i < 3; ++i) cam.t10[i] = sg == 0 ? U[i * 3 + 2] : -U[i * 3 + 2];
#pragma unroll
          for (int i = 0; i < 3; ++i) {
#pragma unroll
            for (int j = 0; j < 3; ++j)
              cam.P10[i * 4 + j] = ep5_dot3(Km[i * 3 + 0], cam.R10[0 * 3 + j], Km[i * 3 + 1], cam.R10[1 * 3 + j], Km[i * 3 + 2], cam.R10[2 * 3 + j]);
            cam.P10[i * 4 + 3] = ep5_dot3(Km[i * 3 + 0], cam.t10[0], Km[i * 3 + 1], cam.t10[1], Km[i * 3 + 2], cam.t10[2]);
          }
#pragma unroll
          for (int k = 0; k < 4; ++k) cam.K0[k] = cam.K1[k] = a.K[k];
        }
      }
    }
  }
  __syncthreads();
  if (dec[3] == EP5_OK && !a.single)
    for (int s = tid; s < dec[2]; s += EP5_SELECT_THREADS) atomicAdd(&cnt[6], a.n_models[s]);
  if (dec[3] != EP5_OK) {
    if (tid == 0) {
      a.rec->status = dec[3];
      a.rec->iterations = dec[2];
      a.rec->models = 0;
      a.rec->best_sample = -1;
      a.rec->best_model = -1;
      a.rec->n_inliers_5p = a.rec->n_inliers = 0;
      a.rec->n = a.n;
    }
    for (int i = tid; i < a.n; i += EP5_SELECT_THREADS) a.mask[i] = 0;
    return;
  }
  double Ed[9];
#pragma unroll
  for (int i = 0; i < 9; ++i) Ed[i] = (double)Ef[i];
  int c0 = 0, c1 = 0, c2 = 0, c3 = 0, c5 = 0;
  for (int i = tid; i < a.n; i += EP5_SELECT_THREADS) {
    const double4 p = a.norm[i];
    const float4 q = a.pix[i];
    int bits = a.single ? 1 : (ep5_sampson(Ed, p.x, p.y, p.z, p.w) <= a.thr ? 1 : 0);
#pragma unroll 1
    for (int c = 0; c < 4; ++c) {
      float X0[3], X1[3];
      svo_triangulate(cams[c], q.x, q.y, q.z, q.w, X0, X1);
      if (X0[2] > 0.0f && X1[2] > 0.0f) bits |= 2 << c;
    }
    a.mask[i] = (uint8_t)bits;
    c5 += bits & 1;
    c0 += (bits >> 1) & 1;
    c1 += (bits >> 2) & 1;
    c2 += (bits >> 3) & 1;
    c3 += (bits >> 4) & 1;
  }
  atomicAdd(&cnt[0], c0);
  atomicAdd(&cnt[1], c1);
  atomicAdd(&cnt[2], c2);
  atomicAdd(&cnt[3], c3);
  atomicAdd(&cnt[4], c5);
  __syncthreads();
  if (tid == 0) {  // findCorrectRT: the first candidate with a strictly larger count
    int bc = -1, mx = 0;
    for (int c = 0; c < 4; ++c)
      if (cnt[c] > mx) {
        mx = cnt[c];
        bc = c;
      }
    dec[4] = bc;
  }
  __syncthreads();
  const int bc = dec[4];
  int cf = 0;
  for (int i = tid; i < a.n; i += EP5_SELECT_THREADS) {
    const int b = a.mask[i];
    const int v = bc >= 0 ? ((b & 1) & (b >> (1 + bc))) : 0;
    a.mask[i] = (uint8_t)v;
    cf += v;
  }
  atomicAdd(&cnt[5], cf);
  __syncthreads();
  if (tid == 0) {
    Ep5Rec *r = a.rec;
    r->status = bc >= 0 ? EP5_OK : EP5_NO_CHIRALITY;
    r->n_inliers_5p = cnt[4];
    r->n_inliers = cnt[5];
    r->iterations = dec[2];
    r->models = a.single ? a.n_models[0] : cnt[6];
    r->best_sample = dec[0];
    r->best_model = dec[1];
    r->n = a.n;
    const SvoCam &cam = cams[bc >= 0 ? bc : 0];
#pragma unroll
    for (int i = 0; i < 9; ++i) {
      r->R[i] = cam.R10[i];
      r->E[i] = Ef[i];
    }
#pragma unroll
    for (int i = 0; i < 3; ++i) r->t[i] = cam.t10[i];
  }
}

// ---- host ------------------------------------------------------------------------------------------------------------
static size_t ep5_in_bytes(int n) { return (size_t)n * (sizeof(double4) + sizeof(float4)); }

extern "C" void vo_five_point_destroy(vo_five_point *fp) {
  if (!fp) return;
  if (fp->c) {
    (void)hipSetDevice(fp->c->device);
    (void)hipStreamSynchronize(fp->c->stream_main);
  }
  void *d[] = {fp->d_in, fp->d_models, fp->d_nmod, fp->d_sub, fp->d_cnt, fp->d_out};
  for (void *p : d)
    if (p) (void)hipFree(p);
  if (fp->h_in) (void)hipHostFree(fp->h_in);
  if (fp->h_out) (void)hipHostFree(fp->h_out);
  delete fp;
}

extern "C" int vo_five_point_create(vo_ctx *c, const vo_five_point_params *prm, int max_points, vo_five_point **out) {
  if (!c || !prm || !out) return VO_ERR_INVALID;
  *out = nullptr;
  if (max_points <= 0) max_points = c->cfg.max_points;
  if (max_points < 5) VO_FAIL(c, VO_ERR_INVALID, "vo_five_point_create: max_points must be at least 5");
  if (prm->max_iters < 1 || prm->max_iters > EP5_MAX_ITERS)
    VO_FAIL(c, VO_ERR_INVALID, "vo_five_point_create: max_iters must be in [1, %d]", EP5_MAX_ITERS);
  if (!(prm->thres_px > 0.0f) || !(prm->confidence > 0.0f && prm->confidence < 1.0f))
    VO_FAIL(c, VO_ERR_INVALID, "vo_five_point_create: thres_px must be > 0 and confidence in (0, 1)");
  VO_CHECK_HIP(c, hipSetDevice(c->device));
  vo_five_point *fp = new vo_five_point();
  memset(fp, 0, sizeof(*fp));
  fp->c = c;
  fp->prm = *prm;
  fp->max_points = max_points;
  const size_t S = (size_t)prm->max_iters;
  int rc = VO_OK;
  auto dm = [&](void **p, size_t bytes) {
    if (rc == VO_OK && vo_dev_malloc(c, p, bytes) != hipSuccess) rc = VO_ERR_HIP;
  };
  auto hm = [&](void **p, size_t bytes) {
    if (rc == VO_OK && vo_host_malloc(c, p, bytes, hipHostMallocDefault) != hipSuccess) rc = VO_ERR_HIP;
  };
  const size_t out_bytes = sizeof(Ep5Rec) + (size_t)max_points;
  dm(&fp->d_in, ep5_in_bytes(max_points));
  dm((void **)&fp->d_models, sizeof(double) * 9 * EP5_MAX_MODELS * S);
  dm((void **)&fp->d_nmod, sizeof(int32_t) * S);
  dm((void **)&fp->d_sub, sizeof(int32_t) * 5 * S);
  dm((void **)&fp->d_cnt, sizeof(int32_t) * EP5_MAX_MODELS * S);
  dm(&fp->d_out, out_bytes);
  hm(&fp->h_in, ep5_in_bytes(max_points));
  hm(&fp->h_out, out_bytes);
  if (rc != VO_OK) {
    vo_five_point_destroy(fp);
    VO_FAIL(c, rc, "vo_five_point_create: device allocation failed");
  }
  *out = fp;
  return VO_OK;
}

static int ep5_launch_solve(vo_five_point *fp, int S, int n, int mode) {
  vo_ctx *c = fp->c;
  Ep5SolveArgs a;
  a.norm = (const double4 *)fp->d_in;
  a.n = n;
  a.mode = mode;
  a.seed = fp->prm.seed;
  a.models = fp->d_models;
  a.n_models = fp->d_nmod;
  a.subsets = fp->d_sub;
  a.counts = fp->d_cnt;
  hipLaunchKernelGGL(ep5_solve_kernel, dim3(S), dim3(64), 0, c->stream_main, a);
  VO_CHECK_HIP(c, hipGetLastError());
  return VO_OK;
}

extern "C" int vo_five_point_pose(vo_five_point *fp, const float *pts0, const float *pts1, int n, const float K[4], float R10[9],
                                  float t10[3], uint8_t *mask, vo_five_point_info *info) {
  if (!fp || !fp->c || !K || !R10 || !t10 || n < 0 || (n > 0 && (!pts0 || !pts1 || !mask))) return VO_ERR_INVALID;
  vo_ctx *c = fp->c;
  if (n < 5) VO_FAIL(c, VO_ERR_GN_FAILED, "calcPose5PointsAlgorithm: %d correspondences, the 5-point RANSAC needs at least 5", n);
  if (n > fp->max_points) VO_FAIL(c, VO_ERR_CAPACITY, "%d correspondences exceed the solver's max_points=%d", n, fp->max_points);
  const double fx = K[0], fy = K[1], cx = K[2], cy = K[3];
  if (!(fx != 0.0 && fy != 0.0 && std::isfinite(fx) && std::isfinite(fy) && fx + fy != 0.0))
    VO_FAIL(c, VO_ERR_INVALID, "vo_five_point_pose: bad camera matrix");
  VO_CHECK_HIP(c, hipSetDevice(c->device));
  double4 *hn = (double4 *)fp->h_in;
  float4 *hp = (float4 *)((char *)fp->h_in + sizeof(double4) * (size_t)n);
  for (int i = 0; i < n; ++i) {
    hn[i] = make_double4(((double)pts0[2 * i] - cx) / fx, ((double)pts0[2 * i + 1] - cy) / fy, ((double)pts1[2 * i] - cx) / fx,
                         ((double)pts1[2 * i + 1] - cy) / fy);
    hp[i] = make_float4(pts0[2 * i], pts0[2 * i + 1], pts1[2 * i], pts1[2 * i + 1]);
  }
  const double t = (double)fp->prm.thres_px / ((fx + fy) / 2.0);
  const float thr = (float)(t * t);
  hipStream_t st = c->stream_main;
  VO_CHECK_HIP(c, hipMemcpyAsync(fp->d_in, fp->h_in, ep5_in_bytes(n), hipMemcpyHostToDevice, st));
  const int single = n == 5;
  const int S = single ? 1 : fp->prm.max_iters;
  int rc = ep5_launch_solve(fp, S, n, single ? 1 : 0);
  if (rc != VO_OK) return rc;
  if (!single) {
    hipLaunchKernelGGL(ep5_score_kernel, dim3((n + EP5_SCORE_PTS - 1) / EP5_SCORE_PTS, S), dim3(EP5_SCORE_THREADS), 0, st,
                       (const double4 *)fp->d_in, n, (const double *)fp->d_models, (const int32_t *)fp->d_nmod, fp->d_cnt, thr);
    VO_CHECK_HIP(c, hipGetLastError());
  }
  Ep5SelectArgs a;
  a.norm = (const double4 *)fp->d_in;
  a.pix = (const float4 *)((char *)fp->d_in + sizeof(double4) * (size_t)n);
  a.n = n;
  a.S = S;
  a.single = single;
  a.models = fp->d_models;
  a.n_models = fp->d_nmod;
  a.counts = fp->d_cnt;
  a.thr = thr;
  a.confidence = (double)fp->prm.confidence;
  a.max_iters = fp->prm.max_iters;
  for (int k = 0; k < 4; ++k) a.K[k] = K[k];
  a.rec = (Ep5Rec *)fp->d_out;
  a.mask = (uint8_t *)fp->d_out + sizeof(Ep5Rec);
  hipLaunchKernelGGL(ep5_select_kernel, dim3(1), dim3(EP5_SELECT_THREADS), 0, st, a);
  VO_CHECK_HIP(c, hipGetLastError());
  VO_CHECK_HIP(c, hipMemcpyAsync(fp->h_out, fp->d_out, sizeof(Ep5Rec) + (size_t)n, hipMemcpyDeviceToHost, st));
  VO_CHECK_HIP(c, hipStreamSynchronize(st));
  fp->last_samples = single ? 0 : S;
  const Ep5Rec *r = (const Ep5Rec *)fp->h_out;
  if (info) {
    memcpy(info->E10, r->E, sizeof(info->E10));
    info->n_inliers_5p = r->n_inliers_5p;
    info->n_inliers = r->n_inliers;
    info->iterations = r->iterations;
    info->models = r->models;
    info->best_sample = r->best_sample;
  }
  if (r->status == EP5_NO_MODEL) VO_FAIL(c, VO_ERR_GN_FAILED, "calcPose5PointsAlgorithm: the RANSAC found no essential matrix with more than 4 inliers");
  if (r->status == EP5_NO_CHIRALITY) VO_FAIL(c, VO_ERR_GN_FAILED, "calcPose5PointsAlgorithm: no point lies in front of both cameras under any (R, t)");
  memcpy(R10, r->R, sizeof(float) * 9);
  memcpy(t10, r->t, sizeof(float) * 3);
  memcpy(mask, (const uint8_t *)fp->h_out + sizeof(Ep5Rec), (size_t)n);
  return VO_OK;
}

// the MonoVO hook (vo_five_point_fn): non-zero on success
static int ep5_hook(void *user, const float *pts0, const float *pts1, int n, const float K[4], float R10[9], float t10[3], uint8_t *mask) {
  return vo_five_point_pose((vo_five_point *)user, pts0, pts1, n, K, R10, t10, mask, nullptr) == VO_OK ? 1 : 0;
}

extern "C" int vo_mvo_params_set_five_point(vo_mvo_params *prm, vo_five_point *fp) {
  if (!prm || !fp) return VO_ERR_INVALID;
  prm->five_point = &ep5_hook;
  prm->five_point_user = fp;
  return VO_OK;
}

extern "C" int vo_five_point_minimal(vo_five_point *fp, const double *x0, const double *x1, int n_sets, double *E, int *n_sol) {
  if (!fp || !fp->c || !x0 || !x1 || !E || !n_sol || n_sets < 0) return VO_ERR_INVALID;
  vo_ctx *c = fp->c;
  VO_CHECK_HIP(c, hipSetDevice(c->device));
  const int chunk = std::min(fp->prm.max_iters, fp->max_points / 5);
  hipStream_t st = c->stream_main;
  for (int b = 0; b < n_sets; b += chunk) {
    const int S = std::min(chunk, n_sets - b);
    double4 *hn = (double4 *)fp->h_in;
    for (int i = 0; i < 5 * S; ++i) {
      const size_t k = (size_t)5 * b + i;
      hn[i] = make_double4(x0[2 * k], x0[2 * k + 1], x1[2 * k], x1[2 * k + 1]);
    }
    VO_CHECK_HIP(c, hipMemcpyAsync(fp->d_in, fp->h_in, sizeof(double4) * 5 * (size_t)S, hipMemcpyHostToDevice, st));
    int rc = ep5_launch_solve(fp, S, 5 * S, 1);
    if (rc != VO_OK) return rc;
    VO_CHECK_HIP(c, hipMemcpyAsync(E + (size_t)b * 90, fp->d_models, sizeof(double) * 90 * (size_t)S, hipMemcpyDeviceToHost, st));
    VO_CHECK_HIP(c, hipMemcpyAsync(n_sol + b, fp->d_nmod, sizeof(int32_t) * (size_t)S, hipMemcpyDeviceToHost, st));
    VO_CHECK_HIP(c, hipStreamSynchronize(st));
  }
  fp->last_samples = 0;
  return VO_OK;
}

extern "C" int vo_five_point_samples(const vo_five_point *fp, int32_t *subsets, int32_t *n_models, int32_t *best_count, int cap,
                                     int *n_samples) {
  if (!fp || !fp->c || !n_samples) return VO_ERR_INVALID;
  vo_ctx *c = fp->c;
  const int S = fp->last_samples;
  *n_samples = S;
  if (!subsets && !n_models && !best_count) return VO_OK;
  if (cap < S) VO_FAIL(c, VO_ERR_CAPACITY, "vo_five_point_samples: %d samples, room for %d", S, cap);
  if (S == 0) return VO_OK;
  VO_CHECK_HIP(c, hipSetDevice(c->device));
  hipStream_t st = c->stream_main;
  std::vector<int32_t> nm(S), cnt((size_t)S * EP5_MAX_MODELS);
  if (subsets) VO_CHECK_HIP(c, hipMemcpyAsync(subsets, fp->d_sub, sizeof(int32_t) * 5 * (size_t)S, hipMemcpyDeviceToHost, st));
  VO_CHECK_HIP(c, hipMemcpyAsync(nm.data(), fp->d_nmod, sizeof(int32_t) * (size_t)S, hipMemcpyDeviceToHost, st));
  VO_CHECK_HIP(c, hipMemcpyAsync(cnt.data(), fp->d_cnt, sizeof(int32_t) * EP5_MAX_MODELS * (size_t)S, hipMemcpyDeviceToHost, st));
  VO_CHECK_HIP(c, hipStreamSynchronize(st));
  for (int s = 0; s < S; ++s) {
    if (n_models) n_models[s] = nm[s];
    if (best_count) {
      int b = -1;
      for (int m = 0; m < nm[s]; ++m) b = std::max(b, cnt[(size_t)s * EP5_MAX_MODELS + m]);
      best_count[s] = b;
    }
  }
  return VO_OK;
}

extern "C" int vo_five_point_counts(const vo_five_point *fp, int32_t *counts, int cap, int *n_samples) {
  if (!fp || !fp->c || !n_samples) return VO_ERR_INVALID;
  vo_ctx *c = fp->c;
  const int S = fp->last_samples;
  *n_samples = S;
  if (!counts || S == 0) return VO_OK;
  if (cap < S) VO_FAIL(c, VO_ERR_CAPACITY, "vo_five_point_counts: %d samples, room for %d", S, cap);
  VO_CHECK_HIP(c, hipSetDevice(c->device));
  hipStream_t st = c->stream_main;
  std::vector<int32_t> nm(S);
  VO_CHECK_HIP(c, hipMemcpyAsync(nm.data(), fp->d_nmod, sizeof(int32_t) * (size_t)S, hipMemcpyDeviceToHost, st));
  VO_CHECK_HIP(c, hipMemcpyAsync(counts, fp->d_cnt, sizeof(int32_t) * EP5_MAX_MODELS * (size_t)S, hipMemcpyDeviceToHost, st));
  VO_CHECK_HIP(c, hipStreamSynchronize(st));
  for (int s = 0; s < S; ++s)
    for (int m = nm[s]; m < EP5_MAX_MODELS; ++m) counts[(size_t)s * EP5_MAX_MODELS + m] = -1;
  return VO_OK;
}
