// semidense_regularize_device.hpp — the kernel that regularises a semi-dense map: outlier removal, fill, smoothing (include/vo_hip.h,
// "Semi-dense regularisation", has the definition). Included by semidense_regularize.hip and, through
// tests/emu/hip_emu.h, by the CPU harness (tests/emu/emu_semidense_regularize.cpp) that runs this text against the numpy restatement
// (tests/semidense_regularize_restatement.py).
//
//   semidense_regularize_kernel   one launch, both stages. A workgroup of SDR_NT threads owns a tile of SDR_TW x SDR_TH pixels. It
//                      stages invd, var = sigma sigma, 1 / var (each formed once per pixel, not once per neighbourhood) and the
//                      entry flag over the tile with a halo of 2 radius; a cell outside the image is "no entry", nothing is
//                      reflected, and the cell's global address is formed from coordinates clamped to the image BEFORE it is formed.
//                      A map is sparse (a sixth of the pixels on the test stream), so neither stage walks its region lane by pixel:
//                      the lanes first LIST the cells that have work — stage A the fill candidates of the tile with a halo of
//                      radius, stage B the pixels of map A in the tile — with one LDS atomicAdd on a counter each, and then share
//                      the list out, so that a wavefront's lanes are busy together. The list's order is whatever the arrival order
//                      was and does not matter: a cell's result depends on the staged planes alone. A fill candidate sums its
//                      neighbours' entries from LDS and writes mean and vmean into its own (until then unread) cell and 2 into its
//                      flag of map A, a plane of its own that no lane reads before the barrier. Stage B runs from LDS and writes
//                      the four output planes with plain stores; the pixels without work get their zeros in the listing pass. No
//                      cross-lane sum; the only atomics are the two LDS counters.
//
// The arrays are sized for radius SDR_MAX_R; a smaller radius uses their upper-left part at the same pitch. The includer provides
// nothing but __global__, __shared__, __syncthreads, atomicAdd and the built-in indices.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#if defined(__HIP_DEVICE_COMPILE__)
#define SDR_MUL(a, b) __fmul_rn((a), (b))
#define SDR_ADD(a, b) __fadd_rn((a), (b))
#define SDR_SUB(a, b) __fsub_rn((a), (b))
#else  // host text (the emulation harness): compiled with -ffp-contract=off
#define SDR_MUL(a, b) ((a) * (b))
#define SDR_ADD(a, b) ((a) + (b))
#define SDR_SUB(a, b) ((a) - (b))
#endif

#define SDR_NT 256
#define SDR_TW 64  // the tile: a row is one wavefront wide
#define SDR_TH 8
#define SDR_MAX_R 3
#define SDR_SW (SDR_TW + 4 * SDR_MAX_R)  // the staged region's pitch and rows
#define SDR_SH (SDR_TH + 4 * SDR_MAX_R)
#define SDR_LIST ((SDR_TW + 2 * SDR_MAX_R) * (SDR_TH + 2 * SDR_MAX_R))  // the cells stage A looks at: the longer of the two lists
#define SDR_LDS_BYTES (SDR_SW * SDR_SH * (3 * 4 + 2) + SDR_LIST * 2 + 2 * 4)
#define SDR_FLT_MAX 3.4028235e38f

struct SdrArgs {
  const float *invd, *sigma;  // the map, W x H planes, tightly packed
  const uint8_t *n_obs;
  const uint8_t *Lk;          // level-0 pixel (0, 0) of the keyframe's left image
  int strideK;                // bytes per row
  int W, H;
  const uint8_t *mask;        // the keyframe's ignore mask (0 = ignore), null: none
  int mask_stride;
  int radius, min_support, fill_min, g_min2;  // g_min g_min
  float chi2, dist2;          // chi chi, dist_sigma dist_sigma
  float *invd_r, *sigma_r;    // the regularised map
  uint8_t *n_obs_r, *rstatus;
};

__global__ __launch_bounds__(SDR_NT) void semidense_regularize_kernel(SdrArgs a) {
  __shared__ float s_invd[SDR_SH * SDR_SW], s_var[SDR_SH * SDR_SW], s_winv[SDR_SH * SDR_SW];
  __shared__ uint8_t s_ent[SDR_SH * SDR_SW], s_map[SDR_SH * SDR_SW];  // an original entry; map A: 0 nothing, 1 entry, 2 filled
  __shared__ uint16_t s_list[SDR_LIST];                               // staged cells with work: stage A's, then stage B's
  __shared__ int s_n[2];                                              // their counts
  const int tid = (int)threadIdx.x, r = a.radius, W = a.W, H = a.H;
  const int x0 = (int)blockIdx.x * SDR_TW, y0 = (int)blockIdx.y * SDR_TH;
  if (tid < 2) s_n[tid] = 0;

  // ---- the staged region: the tile with a halo of 2 r -------------------------------------------------------------------------------
  const int sw = SDR_TW + 4 * r, sh = SDR_TH + 4 * r;
  for (int idx = tid; idx < sw * sh; idx += SDR_NT) {
    const int ly = idx / sw, lx = idx - ly * sw;
    const int x = x0 - 2 * r + lx, y = y0 - 2 * r + ly;
    const bool in = x >= 0 && x < W && y >= 0 && y < H;
    const int xc = x < 0 ? 0 : (x > W - 1 ? W - 1 : x), yc = y < 0 ? 0 : (y > H - 1 ? H - 1 : y);  // clamped before any address
    const size_t g = (size_t)yc * (size_t)W + (size_t)xc;
    const int no = (int)a.n_obs[g];
    const float iv = a.invd[g], sg = a.sigma[g];
    const bool ent = in && no >= 1 && sg > 0.0f && sg <= SDR_FLT_MAX && iv > 0.0f && iv <= SDR_FLT_MAX;
    const float var = ent ? SDR_MUL(sg, sg) : 0.0f;
    const int cell = ly * SDR_SW + lx;
    s_invd[cell] = ent ? iv : 0.0f;
    s_var[cell] = var;
    s_winv[cell] = ent ? 1.0f / var : 0.0f;
    s_ent[cell] = ent ? 1 : 0;
  }
  __syncthreads();

  // ---- stage A, fill: the tile with a halo of r ---------------------------------------------------------------------------------------
  const int aw = SDR_TW + 2 * r, ah = SDR_TH + 2 * r;
  for (int idx = tid; idx < aw * ah; idx += SDR_NT) {  // the candidates are listed
    const int ay = idx / aw, ax = idx - ay * aw;
    const int x = x0 - r + ax, y = y0 - r + ay;
    const int cell = (ay + r) * SDR_SW + (ax + r);
    const int m = (int)s_ent[cell];
    s_map[cell] = (uint8_t)m;
    if (!m && a.fill_min > 0 && x >= 1 && x <= W - 2 && y >= 1 && y <= H - 2) {  // (inside the image, and so are its four taps)
      bool cand = !a.mask || a.mask[(size_t)y * (size_t)a.mask_stride + (size_t)x] != 0;
      if (cand) {
        const uint8_t *row = a.Lk + (size_t)y * (size_t)a.strideK + (size_t)x;
        const int gx = (int)row[1] - (int)row[-1];
        const int gy = (int)a.Lk[(size_t)(y + 1) * (size_t)a.strideK + (size_t)x] - (int)a.Lk[(size_t)(y - 1) * (size_t)a.strideK + (size_t)x];
        cand = gx * gx + gy * gy >= a.g_min2;
      }
      if (cand) s_list[atomicAdd(&s_n[0], 1)] = (uint16_t)cell;  // (at most aw ah <= SDR_LIST of them)
    }
  }
  __syncthreads();
  const int n_cand = s_n[0];
  for (int i = tid; i < n_cand; i += SDR_NT) {  // and shared out
    const int cell = (int)s_list[i];
    float S = 0.0f, Wt = 0.0f, V = 0.0f;
    int cnt = 0;
    for (int dy = -r; dy <= r; ++dy)
      for (int dx = -r; dx <= r; ++dx) {
        const int n = cell + dy * SDR_SW + dx;
        if (s_ent[n]) {
          const float w = s_winv[n];
          S = SDR_ADD(S, SDR_MUL(s_invd[n], w));
          Wt = SDR_ADD(Wt, w);
          V = SDR_ADD(V, s_var[n]);
          ++cnt;
        }
      }
    if (cnt < a.fill_min) continue;  // (fill_min >= 1 here: cnt >= 1 below)
    const float mean = S / Wt, vmean = V / (float)cnt;
    bool ok = true;
    for (int dy = -r; dy <= r; ++dy)
      for (int dx = -r; dx <= r; ++dx) {
        const int n = cell + dy * SDR_SW + dx;
        if (s_ent[n]) {
          const float dd = SDR_SUB(s_invd[n], mean);
          if (!(SDR_MUL(dd, dd) <= SDR_MUL(a.chi2, SDR_ADD(s_var[n], vmean)))) ok = false;
        }
      }
    if (ok) {  // this cell had no entry: no lane reads its values, or its flag of map A, before the barrier
      s_map[cell] = 2;
      s_invd[cell] = mean;
      s_var[cell] = vmean;
    }
  }
  __syncthreads();  // (the list is free again)

  // ---- stage B, support, conflict and smoothing: the tile ---------------------------------------------------------------------------
  for (int idx = tid; idx < SDR_TW * SDR_TH; idx += SDR_NT) {  // the pixels of map A are listed; the others get their zeros
    const int ty = idx / SDR_TW, tx = idx - ty * SDR_TW;
    const int x = x0 + tx, y = y0 + ty;
    if (x >= W || y >= H) continue;
    const int cell = (ty + 2 * r) * SDR_SW + (tx + 2 * r);
    if (s_map[cell]) {
      s_list[atomicAdd(&s_n[1], 1)] = (uint16_t)cell;  // (at most SDR_TW SDR_TH <= SDR_LIST of them)
    } else {
      const size_t g = (size_t)y * (size_t)W + (size_t)x;
      a.invd_r[g] = 0.0f;
      a.sigma_r[g] = 0.0f;
      a.n_obs_r[g] = 0;
      a.rstatus[g] = 0;
    }
  }
  __syncthreads();
  const int n_map = s_n[1];
  for (int i = tid; i < n_map; i += SDR_NT) {
    const int cell = (int)s_list[i];
    const int ly = cell / SDR_SW, lx = cell - ly * SDR_SW;
    const int x = x0 - 2 * r + lx, y = y0 - 2 * r + ly;  // a pixel of the tile inside the image: listed above
    const int m = (int)s_map[cell];
    const float ic = s_invd[cell], vc = s_var[cell];
    float S = 0.0f, Wt = 0.0f;
    int support = 0, conflict = 0;
    for (int dy = -r; dy <= r; ++dy)
      for (int dx = -r; dx <= r; ++dx) {
        const int n = cell + dy * SDR_SW + dx;
        const int mn = (int)s_map[n];
        if (!mn) continue;
        const float in_ = s_invd[n], vn = s_var[n];
        const float dd = SDR_SUB(in_, ic);
        const bool cons = SDR_MUL(dd, dd) <= SDR_MUL(a.chi2, SDR_ADD(vc, vn));
        if (cons) {
          const float w = 1.0f / SDR_ADD(vn, SDR_MUL(a.dist2, (float)(dx * dx + dy * dy)));
          S = SDR_ADD(S, SDR_MUL(in_, w));
          Wt = SDR_ADD(Wt, w);
        }
        if (mn == 1 && (dx | dy) != 0) {
          if (cons) ++support;
          else ++conflict;
        }
      }
    const size_t g = (size_t)y * (size_t)W + (size_t)x;
    const bool keep = support >= a.min_support && conflict <= support;
    a.invd_r[g] = keep ? S / Wt : 0.0f;
    a.sigma_r[g] = keep ? sqrtf(vc) : 0.0f;
    a.n_obs_r[g] = keep ? (m == 1 ? a.n_obs[g] : (uint8_t)1) : (uint8_t)0;
    a.rstatus[g] = (uint8_t)(keep ? (m == 1 ? 1 : 3) : (m == 1 ? 2 : 0));
  }
}
