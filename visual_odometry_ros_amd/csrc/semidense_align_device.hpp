// semidense_align_device.hpp — the kernel of the direct image alignment on the semi-dense map (include/vo_hip.h, "Semi-dense
// alignment", has the definition). Included by semidense_align.hip and, through tests/emu/hip_emu.h, by the CPU
// harness (tests/emu/emu_semidense_align.cpp) that runs this text against the numpy restatement
// (tests/semidense_align_restatement.py).
//
//   semidense_align_kernel   grid ceil(W H / SDA_BLOCK), SDA_NT threads; one launch per iteration. A workgroup owns the SDA_BLOCK
//                      consecutive raster indices of its block — the block of the definition, whatever the launch looks like.
//                      (a) four rounds of SDA_NT coalesced map reads; the pixels of the set are packed into an LDS list by lane-mask
//                      population counts (the map holds 5 - 25 % of a plane: without the list three lanes in four would idle
//                      through (b)). (b) one listed pixel per thread and turn: the per-pixel constants, the warp under the pose
//                      of the state block, the sample (sdt_sample: the cell is clamped before the address is formed), residual and
//                      weight, left in LDS as eight integers. (c) the 30 sums: thread t forms sum (t & 31) over the listed pixels
//                      e = t >> 5 (mod 8) in int64 — the sums are exact, so neither the list's order nor this split shows — and
//                      the eight parts are added; 30 plain stores into the block's row of `partial`. (d) a ticket: the last
//                      workgroup to get there (one agent-scope release per workgroup in front of the ticket, one acquire in the last) converts the rows to f64 and adds them in block order (staged through LDS, SDA_STAGE
//                      rows at a time, so that the loads are not one behind the other), and thread 0 solves the 6 x 6 system,
//                      updates the pose and writes the state block. No float atomics; the ticket is the only atomic.
//                      A launch that finds `done` set returns at once.
//                      The coarse-to-fine operator runs the same kernel level by level: `first` says where a launch
//                      takes its pose from (SDA_FIRST_*), `level` which record of the state block its result is filed under.
//
// The includer provides __global__, __shared__, __syncthreads, the built-in indices, int sda_wave_rank(bool, int *n) (the number of
// lower lanes of the wavefront whose argument is true; *n: all lanes'), SDA_DRAIN (the wavefront's stores have left) and the
// agent-scope spellings SDA_ST_AGENT, SDA_ATOMIC_ADD_AGENT, SDA_FENCE_RELEASE, SDA_FENCE_ACQUIRE (each with its own wait).
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include "semidense_sample.hpp"  // SDT_MUL / SDT_ADD / SDT_SUB, sdt_q, sdt_in, sdt_sample

#define SDA_BLOCK 1024        // raster indices per block: a constant of the definition
#define SDA_NT 256
#define SDA_NSUM 30           // 21 H, 6 b, sum w r^2, sum w, count
#define SDA_STAGE 128         // rows of `partial` staged in LDS at a time (SDA_STAGE * 32 doubles = the records' 32 KB)
#define SDA_QMAX 4194304.0f   // 2^22: |16 J_i| at or above this drops the pixel
#define SDA_FRONT 0.1f
#define SDA_PIVOT (1.0 / 1048576.0)  // 2^-20: a pivot at or below this share of its diagonal entry is refused
#define SDA_MAX_ITERS 32
#define SDA_MAX_LEVELS 6
// SdaArgs.first: 0 = a level's later launch (the pose of the state block; returns at once behind "done"); the others start a
// level, whatever "done" holds, with iters = 0:
#define SDA_FIRST_CALL 1   // a call's first launch: the pose is T0, the state block is overwritten
#define SDA_FIRST_LEVEL 2  // the first launch of a lower level: the pose the level above left in the state block
#define SDA_FIRST_PREV 3   // a call's first launch that starts from the PREVIOUS call's result where its status is 0 or 1, else T0

struct SdaLevel {  // one level's last evaluated system, as far as the result reports it
  int status, iters, count, pad;
  double swrr, sw;
};

struct SdaState {  // the small device block: pose, status and the "done" word; the last evaluated system
  float T[16];
  int status, iters, done, count;
  unsigned ticket;
  int pad;
  double swrr, sw;  // sum w r^2, sum w (unscaled)
  double H[21], b[6];
  SdaLevel lv[SDA_MAX_LEVELS];  // per level of the coarse-to-fine operator ([0] alone for the level-0 operator)
  int start_prev, pad2;         // the call started from the previous call's result (SDA_FIRST_PREV and its status was 0 or 1)
};

struct SdaArgs {
  const uint8_t *Lk, *Lc;  // level-0 pixel (0, 0) of the key / current left image, W x H each
  int strideK, strideC;    // bytes per row
  int W, H;
  const float *invd, *sigma;  // the map, W x H planes, tightly packed
  const uint8_t *n_obs;
  int min_obs, kq, max_iters, min_pixels;  // kq = (int)floorf(16 huber + 0.5f)
  double eps2;  // (double)eps * (double)eps: exact
  float fx, fy, cx, cy;
  int n_blocks;
  int first;     // SDA_FIRST_*; 1: the call's first launch: the pose is T0, whatever the state block holds is overwritten (its ticket is 0)
  int level;     // the pyramid level these planes are: the record of the state block that this launch's result is filed under
  float T0[12];  // the start, rows 0..2
  long long *partial;  // [n_blocks][SDA_NSUM]
  SdaState *st;
};

// host: the parameters as the kernel takes them (host code: -ffp-contract=off)
static inline void sda_params(SdaArgs *a, int min_obs, float huber, int max_iters, float eps, int min_pixels) {
  a->min_obs = min_obs;
  a->kq = (int)floorf(16.0f * huber + 0.5f);
  a->max_iters = max_iters;
  a->min_pixels = min_pixels;
  a->eps2 = (double)eps * (double)eps;
}

// geometry::se3Exp_f as gn_pose.hip evaluates it: float32, the three coefficients through float64 (below 0.25 rad by the Taylor
// series, whose operations are the definition's); rows 0..2
__device__ static inline void sda_se3_exp(const float xi[6], float T[12]) {
  const float v[3] = {xi[0], xi[1], xi[2]}, w[3] = {xi[3], xi[4], xi[5]};
  const float theta = sqrtf(SDT_ADD(SDT_ADD(SDT_MUL(w[0], w[0]), SDT_MUL(w[1], w[1])), SDT_MUL(w[2], w[2])));
  const float wx[9] = {0.0f, -w[2], w[1], w[2], 0.0f, -w[0], -w[1], w[0], 0.0f};
  float wx2[9];
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      float s = 0.0f;
#pragma unroll
      for (int k = 0; k < 3; ++k) s = SDT_ADD(s, SDT_MUL(wx[i * 3 + k], wx[k * 3 + j]));
      wx2[i * 3 + j] = s;
    }
  float a, b, c;
  if ((double)theta < 1e-7) {
    a = 1.0f;
    b = 0.5f;
    c = 0.33333333333333333333333333f;
  } else {
    const double th = (double)theta;
    double sn, cs1;  // sin(th), 1 - cos(th)
    if (th < 0.25) {
      const double t2 = th * th;
      sn = th * (1.0 + t2 * (-1.0 / 6 + t2 * (1.0 / 120 + t2 * (-1.0 / 5040 + t2 * (1.0 / 362880 + t2 * (-1.0 / 39916800 + t2 * (1.0 / 6227020800.0)))))));
      cs1 = t2 * (0.5 + t2 * (-1.0 / 24 + t2 * (1.0 / 720 + t2 * (-1.0 / 40320 + t2 * (1.0 / 3628800 + t2 * (-1.0 / 479001600.0))))));
    } else {
      sn = sin(th);
      cs1 = 1 - cos(th);
    }
    a = (float)(sn / th);
    b = (float)(cs1 / (double)SDT_MUL(theta, theta));
    c = (float)((th - sn) / (double)SDT_MUL(SDT_MUL(theta, theta), theta));
  }
  float V[9];
#pragma unroll
  for (int i = 0; i < 9; ++i) {
    const float I = (i == 0 || i == 4 || i == 8) ? 1.0f : 0.0f;
    T[(i / 3) * 4 + i % 3] = SDT_ADD(SDT_ADD(I, SDT_MUL(a, wx[i])), SDT_MUL(b, wx2[i]));
    V[i] = SDT_ADD(SDT_ADD(I, SDT_MUL(b, wx[i])), SDT_MUL(c, wx2[i]));
  }
#pragma unroll
  for (int i = 0; i < 3; ++i) T[i * 4 + 3] = SDT_ADD(SDT_ADD(SDT_MUL(V[i * 3], v[0]), SDT_MUL(V[i * 3 + 1], v[1])), SDT_MUL(V[i * 3 + 2], v[2]));
}

// the last workgroup's thread 0: S = the 30 sums in f64 (unscaled). Solves, updates the pose, writes the state block.
__device__ static inline void sda_finish(const SdaArgs &a, const double *S, const float Tin[12], bool from_T0) {
  SdaState *st = a.st;
  double A[6][6], bv[6];
  {
    int n = 0;
#pragma unroll
    for (int i = 0; i < 6; ++i)
#pragma unroll
      for (int j = i; j < 6; ++j, ++n) {
        const double h = S[n] * (1.0 / 65536.0);
        A[i][j] = A[j][i] = h;
        st->H[n] = h;
      }
#pragma unroll
    for (int i = 0; i < 6; ++i) st->b[i] = bv[i] = S[21 + i] * (1.0 / 65536.0);
  }
  const int count = (int)S[29], iters = (a.first ? 0 : st->iters) + 1;
  st->count = count;
  st->iters = iters;
  st->swrr = S[27];
  st->sw = S[28];
  int status = 1, done = iters >= a.max_iters ? 1 : 0;
  float To[12];
#pragma unroll
  for (int i = 0; i < 12; ++i) To[i] = Tin[i];
  if (count < a.min_pixels) {
    status = 2;
    done = 1;
  } else {
    double L[6][6], Dg[6], y[6], x[6];
    bool ok = true;
    // (no early exit: every loop has constant bounds and unrolls, so that the arrays stay in registers; after a refused pivot the
    // values that follow are not used)
#pragma unroll
    for (int j = 0; j < 6; ++j) {
      double d = A[j][j];
#pragma unroll
      for (int k = 0; k < j; ++k) d = d - (L[j][k] * L[j][k]) * Dg[k];
      ok = ok && d > 0.0 && d > A[j][j] * SDA_PIVOT && d <= 1.7976931348623157e308;
      Dg[j] = d;
#pragma unroll
      for (int i = j + 1; i < 6; ++i) {
        double s = A[i][j];
#pragma unroll
        for (int k = 0; k < j; ++k) s = s - (L[i][k] * L[j][k]) * Dg[k];
        L[i][j] = s / d;
      }
    }
#pragma unroll
    for (int i = 0; i < 6; ++i) {
      double s = bv[i];
#pragma unroll
      for (int k = 0; k < i; ++k) s = s - L[i][k] * y[k];
      y[i] = s;
    }
#pragma unroll
    for (int i = 5; i >= 0; --i) {
      double s = y[i] / Dg[i];
#pragma unroll
      for (int k = i + 1; k < 6; ++k) s = s - L[k][i] * x[k];
      x[i] = s;
    }
#pragma unroll
    for (int i = 0; i < 6; ++i) ok = ok && fabs(x[i]) <= 1.7976931348623157e308;
    if (!ok) {
      status = 3;
      done = 1;
    } else {
      const double nrm2 = ((((x[0] * x[0] + x[1] * x[1]) + x[2] * x[2]) + x[3] * x[3]) + x[4] * x[4]) + x[5] * x[5];
      float xi[6], E[12];
#pragma unroll
      for (int i = 0; i < 6; ++i) xi[i] = -(float)x[i];
      sda_se3_exp(xi, E);
#pragma unroll
      for (int i = 0; i < 3; ++i)  // T <- T * exp(-xi) in svo_mul44's order (row 3 of both: 0 0 0 1)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          float r = SDT_MUL(Tin[i * 4 + 0], E[j]);
          r = SDT_ADD(SDT_MUL(Tin[i * 4 + 1], E[4 + j]), r);
          r = SDT_ADD(SDT_MUL(Tin[i * 4 + 2], E[8 + j]), r);
          r = SDT_ADD(SDT_MUL(Tin[i * 4 + 3], j == 3 ? 1.0f : 0.0f), r);
          To[i * 4 + j] = r;
        }
      if (nrm2 < a.eps2) {
        status = 0;
        done = 1;
      }
    }
  }
#pragma unroll
  for (int i = 0; i < 12; ++i) st->T[i] = To[i];
  st->T[12] = st->T[13] = st->T[14] = 0.0f;
  st->T[15] = 1.0f;
  st->status = status;
  st->done = done;
  SdaLevel *lv = &st->lv[a.level];
  lv->status = status;
  lv->iters = iters;
  lv->count = count;
  lv->pad = 0;
  lv->swrr = S[27];
  lv->sw = S[28];
  if (a.first == SDA_FIRST_CALL || a.first == SDA_FIRST_PREV) st->start_prev = from_T0 ? 0 : 1;
}

__global__ __launch_bounds__(SDA_NT) void semidense_align_kernel(SdaArgs a) {
  __shared__ union {
    int rec[8 * SDA_BLOCK];        // field f of listed pixel e at [f * SDA_BLOCK + e]: q0..q5, w | valid << 24, r
    double stage[SDA_STAGE * 32];  // then the staged rows of `partial`
  } s_u;
  int *const s_rec = s_u.rec;
  __shared__ uint16_t s_list[SDA_BLOCK];
  __shared__ long long s_part[8][32];
  __shared__ int s_wn[SDA_NT / 64];
  __shared__ int s_last;
  __shared__ double s_sum[32];
  const int tid = (int)threadIdx.x, wave = tid >> 6;
  if (!a.first && a.st->done) return;  // (written by an earlier launch: every thread reads the same word)
  const int W = a.W, H = a.H;
  const long long np = (long long)W * (long long)H, base = (long long)blockIdx.x * SDA_BLOCK;
  // (the state block's words read here were written by an earlier launch: every thread of every workgroup reads the same)
  const bool from_T0 = a.first == SDA_FIRST_CALL || (a.first == SDA_FIRST_PREV && (unsigned)a.st->status > 1u);
  float T[12];
#pragma unroll
  for (int i = 0; i < 12; ++i) T[i] = from_T0 ? a.T0[i] : a.st->T[i];
  // ---- (a) the block's pixels of the set, packed ----------------------------------------------------------------------------------
  int n = 0;
  for (int k = 0; k < SDA_BLOCK / SDA_NT; ++k) {
    const int li = k * SDA_NT + tid;
    const long long i = base + li;
    bool in = false;
    if (i < np) {
      const int y = (int)(i / W), x = (int)(i - (long long)y * W);
      if (x >= 1 && x <= W - 2 && y >= 1 && y <= H - 2 && (int)a.n_obs[i] >= a.min_obs) in = a.sigma[i] > 0.0f && a.invd[i] > 0.0f;
    }
    int cnt;
    const int r = sda_wave_rank(in, &cnt);
    if ((tid & 63) == 0) s_wn[wave] = cnt;
    __syncthreads();
    int off = n;
    for (int v = 0; v < SDA_NT / 64; ++v) {
      off += v < wave ? s_wn[v] : 0;
      n += s_wn[v];
    }
    if (in) s_list[off + r] = (uint16_t)li;
    __syncthreads();
  }
  // ---- (b) one listed pixel per thread and turn ----------------------------------------------------------------------------------
  for (int e = tid; e < n; e += SDA_NT) {
    const long long i = base + (int)s_list[e];
    const int y = (int)(i / W), x = (int)(i - (long long)y * W);
    const uint8_t *c = a.Lk + (size_t)y * (size_t)a.strideK + (size_t)x;
    const float gx = (float)((int)c[1] - (int)c[-1]), gy = (float)((int)c[a.strideK] - (int)c[-a.strideK]);
    const float invd = a.invd[i];
    const float Z = 1.0f / invd;
    const float u = SDT_SUB((float)x, a.cx) / a.fx, v = SDT_SUB((float)y, a.cy) / a.fy;
    const float X = SDT_MUL(u, Z), Y = SDT_MUL(v, Z);
    const float fu = SDT_MUL(a.fx, u), fv = SDT_MUL(a.fy, v);
    const float Ju[6] = {SDT_MUL(a.fx, invd), 0.0f, -SDT_MUL(fu, invd), -SDT_MUL(fu, v), SDT_ADD(a.fx, SDT_MUL(fu, u)), -SDT_MUL(a.fx, v)};
    const float Jv[6] = {0.0f, SDT_MUL(a.fy, invd), -SDT_MUL(fv, invd), -SDT_ADD(a.fy, SDT_MUL(fv, v)), SDT_MUL(fv, u), SDT_MUL(a.fy, u)};
    bool keep = fabsf(X) <= 3.40282347e+38f && fabsf(Y) <= 3.40282347e+38f && fabsf(Z) <= 3.40282347e+38f;
    int q[6];
#pragma unroll
    for (int j = 0; j < 6; ++j) {
      const float J16 = SDT_MUL(16.0f, SDT_MUL(0.5f, SDT_ADD(SDT_MUL(gx, Ju[j]), SDT_MUL(gy, Jv[j]))));
      const bool okj = fabsf(J16) < SDA_QMAX;  // (false for NaN)
      keep = keep && okj;
      q[j] = okj ? (int)floorf(SDT_ADD(J16, 0.5f)) : 0;
    }
    int wv = 0, r = 0;
    if (keep) {
      const float Xc = SDT_ADD(SDT_ADD(SDT_ADD(SDT_MUL(T[0], X), SDT_MUL(T[1], Y)), SDT_MUL(T[2], Z)), T[3]);
      const float Yc = SDT_ADD(SDT_ADD(SDT_ADD(SDT_MUL(T[4], X), SDT_MUL(T[5], Y)), SDT_MUL(T[6], Z)), T[7]);
      const float Zc = SDT_ADD(SDT_ADD(SDT_ADD(SDT_MUL(T[8], X), SDT_MUL(T[9], Y)), SDT_MUL(T[10], Z)), T[11]);
      if (Zc > SDA_FRONT) {
        const int QX = sdt_q(SDT_ADD(SDT_MUL(a.fx, Xc / Zc), a.cx)), QY = sdt_q(SDT_ADD(SDT_MUL(a.fy, Yc / Zc), a.cy));
        if (sdt_in(QX, QY, W, H)) {
          r = sdt_sample(a.Lc, a.strideC, W, H, QX, QY) - 16 * (int)c[0];
          const int ar = r < 0 ? -r : r;
          wv = (ar <= a.kq ? 256 : (256 * a.kq) / ar) | (1 << 24);
        }
      }
    }
#pragma unroll
    for (int j = 0; j < 6; ++j) s_rec[j * SDA_BLOCK + e] = keep ? q[j] : 0;
    s_rec[6 * SDA_BLOCK + e] = wv;
    s_rec[7 * SDA_BLOCK + e] = r;
  }
  __syncthreads();
  // ---- (c) the block's 30 sums ---------------------------------------------------------------------------------------------------
  {
    const int s = tid & 31, part = tid >> 5;
    // sum s: weight * A * B with (A, B) = (q_i, q_j) for the 21 pairs i <= j row by row, (q_i, r), (r, r), (1, 1), and the count
    const int i = (s >= 6) + (s >= 11) + (s >= 15) + (s >= 18) + (s >= 20), j = i + (s - (i * 6 - (i * (i - 1)) / 2));
    const int fa = s < 21 ? i : (s < 27 ? s - 21 : (s == 27 ? 7 : -1)), fb = s < 21 ? j : (s < 28 ? 7 : -1);
    long long acc = 0;
    if (s < SDA_NSUM)
      for (int e = part; e < n; e += 8) {
        const int wv = s_rec[6 * SDA_BLOCK + e];
        const long long wt = s == 29 ? (long long)(wv >> 24) : (long long)(wv & 0xFFFFFF);
        const long long A = fa >= 0 ? (long long)s_rec[fa * SDA_BLOCK + e] : 1, B = fb >= 0 ? (long long)s_rec[fb * SDA_BLOCK + e] : 1;
        acc += wt * A * B;
      }
    s_part[part][s] = acc;
  }
  __syncthreads();
  if (tid < SDA_NSUM) {
    long long t = 0;
    for (int p = 0; p < 8; ++p) t += s_part[p][tid];
    a.partial[(size_t)blockIdx.x * SDA_NSUM + tid] = t;
  }
  // ---- (d) the ticket: the last workgroup reduces, solves and updates ---------------------------------------------------------------
  SDA_DRAIN();      // every wavefront: its row entries have left ...
  __syncthreads();  // ... before thread 0 publishes them (one agent-scope release) and takes the workgroup's ticket
  if (tid == 0) {
    SDA_FENCE_RELEASE();
    s_last = (SDA_ATOMIC_ADD_AGENT(&a.st->ticket, 1u) == (unsigned)a.n_blocks - 1u) ? 1 : 0;
    if (s_last) SDA_FENCE_ACQUIRE();  // one agent-scope acquire covers the workgroup: the barrier below stands behind its wait
  }
  __syncthreads();
  if (!s_last) return;
  double *const stage = s_u.stage;  // [SDA_STAGE][32]
  double sum = 0.0;
  for (int b0 = 0; b0 < a.n_blocks; b0 += SDA_STAGE) {
    const int nb = a.n_blocks - b0 < SDA_STAGE ? a.n_blocks - b0 : SDA_STAGE;
#pragma unroll 8
    for (int k = tid; k < nb * SDA_NSUM; k += SDA_NT) {  // (plain vector loads behind the acquire: independent, so they overlap)
      const int b = k / SDA_NSUM, s = k - b * SDA_NSUM;
      stage[b * 32 + s] = (double)a.partial[(size_t)(b0 + b) * SDA_NSUM + s];
    }
    __syncthreads();
    if (tid < SDA_NSUM) {
#pragma unroll 16
      for (int b = 0; b < nb; ++b) sum = sum + stage[b * 32 + tid];  // block order, block 0 first (unrolled: the reads run ahead of the adds)
    }
    __syncthreads();
  }
  if (tid < SDA_NSUM) s_sum[tid] = sum;
  __syncthreads();
  if (tid == 0) {
    sda_finish(a, s_sum, T, from_T0);
    SDA_ST_AGENT(&a.st->ticket, 0u);  // back to zero for the next launch (every workgroup has taken its ticket: this one holds the last)
  }
}
