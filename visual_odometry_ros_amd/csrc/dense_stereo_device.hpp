// dense_stereo_device.hpp — the kernels of the dense stereo disparity (include/vo_hip.h, "Dense stereo", has the definition;
// DESIGN.md §27): the census transform of both planes, the semi-global aggregation of one direction — one wavefront walks one path,
// lanes as disparities — and the decision. Read by csrc/dense_stereo.hip for gfx950 and by tests/emu/emu_dense_stereo.cpp on CPU
// threads. The includer supplies, for a wavefront all of whose 64 lanes are active:
//   DS_WAVE_MIN_U32(v)                    the smallest v of the wavefront
//   DS_WAVE_STEP(m, lo, hi, mn, up, dn)   mn = the smallest m; up = the previous lane's lo (lane 0: its own); dn = the next lane's
//                                         hi (lane 63: its own)
//   DS_POPC64(v)                          the number of set bits of a 64-bit word
// Everything is an integer up to the parabola; every pixel of the volume is written by exactly one wavefront per launch and the
// launches of the directions follow each other on one stream, so plain stores do and no arrival order enters.
#pragma once
#include <stdint.h>

#define DS_CENSUS_BITS 62
#define DS_CENSUS_HW 4   // 9 columns
#define DS_CENSUS_HH 3   // 7 rows
#define DS_NT 256        // census and decision: threads per workgroup
#define DS_AGG_NT 256    // aggregation: four wavefronts, a path each, per workgroup (one per SIMD of a compute unit)
#define DS_PIX 8         // decision: pixels per wavefront
#define DS_BIG (1 << 20)  // above every L_r: a neighbour disparity outside the range

struct DsCensusArgs {
  const uint8_t *img0, *img1;  // left, right level-0 planes
  int stride0, stride1;
  int W, H;
  unsigned long long *cen0, *cen1;  // W x H words each
};

// grid (ceil(W H / DS_NT), 2): blockIdx.y 0 left, 1 right; a thread per pixel
__global__ __launch_bounds__(DS_NT) void dense_census_kernel(DsCensusArgs a) {
  const size_t i = (size_t)blockIdx.x * DS_NT + threadIdx.x;
  if (i >= (size_t)a.W * (size_t)a.H) return;
  const bool right = blockIdx.y != 0;
  const uint8_t *img = right ? a.img1 : a.img0;
  const int stride = right ? a.stride1 : a.stride0;
  const int y = (int)(i / (size_t)a.W), x = (int)(i - (size_t)y * (size_t)a.W);
  const int c = img[(size_t)y * stride + x];
  unsigned long long w = 0;
  int bit = 0;
#pragma unroll
  for (int v = -DS_CENSUS_HH; v <= DS_CENSUS_HH; ++v) {
    int yy = y + v;
    yy = yy < 0 ? 0 : yy > a.H - 1 ? a.H - 1 : yy;
    const uint8_t *row = img + (size_t)yy * stride;
#pragma unroll
    for (int k = -DS_CENSUS_HW; k <= DS_CENSUS_HW; ++k) {
      if (v == 0 && k == 0) continue;
      int xx = x + k;
      xx = xx < 0 ? 0 : xx > a.W - 1 ? a.W - 1 : xx;
      w |= (unsigned long long)((int)row[xx] < c ? 1 : 0) << bit;
      ++bit;
    }
  }
  (right ? a.cen1 : a.cen0)[i] = w;
}

struct DsAggArgs {
  const unsigned long long *cenL, *cenR;
  uint16_t *S;  // [y][x][d], n_disp = 64 ND per pixel
  int W, H;
  int d_min, p1, p2;
  int dx, dy;   // the direction: each of -1, 0, 1, not both 0
  int n_paths;  // ds_path_count
  int first;    // the first direction stores L_r, the others add to what is there
};

// the number of paths of a direction = of pixels whose predecessor lies outside the image
__host__ __device__ inline int ds_path_count(int W, int H, int dx, int dy) { return dx != 0 ? H + (dy != 0 ? W - 1 : 0) : W; }

// path -> its first pixel: with dx != 0 the H pixels of the column the paths enter through, then (diagonals) the other W - 1 pixels
// of the row they enter through; with dx == 0 the W pixels of that row
__host__ __device__ inline void ds_path_start(int W, int H, int dx, int dy, int path, int *x, int *y) {
  const int x0 = dx > 0 ? 0 : W - 1, y0 = dy > 0 ? 0 : H - 1;
  if (dx == 0) {
    *x = path;
    *y = y0;
  } else if (path < H) {
    *x = x0;
    *y = path;
  } else {
    const int k = path - H;
    *x = dx > 0 ? k + 1 : W - 2 - k;
    *y = y0;
  }
}

// lane l holds the disparities l ND .. l ND + ND - 1: d +- 1 stay in the lane but at its ends, and a lane's share of a pixel's line
// of the volume is ND contiguous values
template <int ND>
__device__ __forceinline__ void ds_fetch(const DsAggArgs &a, int x, int y, int lane, unsigned long long &cl, unsigned long long (&cr)[ND],
                                         int (&so)[ND]) {
  const size_t pix = (size_t)y * (size_t)a.W + (size_t)x;
  cl = a.cenL[pix];
#pragma unroll
  for (int j = 0; j < ND; ++j) {
    const int d = lane * ND + j;
    const int xr = x - a.d_min - d;
    cr[j] = a.cenR[(size_t)y * (size_t)a.W + (size_t)(xr > 0 ? xr : 0)];
    so[j] = a.first ? 0 : (int)a.S[pix * (size_t)(64 * ND) + (size_t)d];
  }
}

// grid ceil(n_paths / (DS_AGG_NT / 64)); the costs are recomputed from the census planes at every step, and the words and the
// volume's line of the next step are fetched before this step's dependent chain (the wave reduction) is worked through
template <int ND>
__global__ __launch_bounds__(DS_AGG_NT) void dense_aggregate_kernel(DsAggArgs a) {
  const int lane = (int)threadIdx.x & 63;
  const int path = (int)blockIdx.x * (DS_AGG_NT / 64) + ((int)threadIdx.x >> 6);
  if (path >= a.n_paths) return;  // (the whole wavefront)
  int x, y;
  ds_path_start(a.W, a.H, a.dx, a.dy, path, &x, &y);
  int len = a.dx > 0 ? a.W - x : a.dx < 0 ? x + 1 : a.H;
  if (a.dy != 0) {
    const int ly = a.dy > 0 ? a.H - y : y + 1;
    len = a.dx != 0 && len < ly ? len : ly;
  }
  unsigned long long cl, cr[ND];
  int so[ND], prev[ND];
  ds_fetch<ND>(a, x, y, lane, cl, cr, so);
  for (int t = 0; t < len; ++t) {
    unsigned long long cl_n = 0, cr_n[ND];
    int so_n[ND];
#pragma unroll
    for (int j = 0; j < ND; ++j) cr_n[j] = 0, so_n[j] = 0;
    if (t + 1 < len) ds_fetch<ND>(a, x + a.dx, y + a.dy, lane, cl_n, cr_n, so_n);
    int cur[ND];
#pragma unroll
    for (int j = 0; j < ND; ++j) cur[j] = x - a.d_min - (lane * ND + j) >= 0 ? (int)DS_POPC64(cl ^ cr[j]) : DS_CENSUS_BITS;
    if (t > 0) {
      int m = prev[0];
#pragma unroll
      for (int j = 1; j < ND; ++j) m = prev[j] < m ? prev[j] : m;
      int mn, up, dn;
      DS_WAVE_STEP(m, prev[ND - 1], prev[0], mn, up, dn);
      if (lane == 0) up = DS_BIG;
      if (lane == 63) dn = DS_BIG;
#pragma unroll
      for (int j = 0; j < ND; ++j) {
        const int lo = j > 0 ? prev[j - 1] : up, hi = j < ND - 1 ? prev[j + 1] : dn;
        int best = (lo < hi ? lo : hi) + a.p1;
        best = prev[j] < best ? prev[j] : best;
        best = mn + a.p2 < best ? mn + a.p2 : best;
        cur[j] += best - mn;
      }
    }
    uint16_t *line = a.S + ((size_t)y * (size_t)a.W + (size_t)x) * (size_t)(64 * ND) + (size_t)(lane * ND);
#pragma unroll
    for (int j = 0; j < ND; ++j) {
      line[j] = (uint16_t)(so[j] + cur[j]);
      prev[j] = cur[j];
      cr[j] = cr_n[j];
      so[j] = so_n[j];
    }
    cl = cl_n;
    x += a.dx;
    y += a.dy;
  }
}

struct DsDecideArgs {
  const uint16_t *S;
  int W, H;
  int d_min, uniqueness, lr_max;
  float sigma;  // eps_d / bf, worked out by the host in float32
  const uint8_t *mask;  // the left slot's ignore mask (0 = ignore), null: none
  int mask_stride;
  float *disp;  // the outputs: any may be null
  uint16_t *cost;
  float *sigma_out;
  uint8_t *status;
};

// grid ceil(W H / (DS_PIX DS_NT / 64)): a wavefront per DS_PIX consecutive pixels, lanes as disparities; key = S << 8 | d, so that
// the smallest key is the smallest S at the smallest d
template <int ND>
__global__ __launch_bounds__(DS_NT) void dense_decide_kernel(DsDecideArgs a) {
  const int lane = (int)threadIdx.x & 63;
  const size_t np = (size_t)a.W * (size_t)a.H;
  const size_t first = ((size_t)blockIdx.x * (DS_NT / 64) + (threadIdx.x >> 6)) * DS_PIX;
  const int n = 64 * ND;
  for (int q = 0; q < DS_PIX; ++q) {
    const size_t pix = first + q;
    if (pix >= np) return;  // (the whole wavefront)
    const int y = (int)(pix / (size_t)a.W), x = (int)(pix - (size_t)y * (size_t)a.W);
    unsigned s[ND];
    unsigned key = 0xFFFFFFFFu;
#pragma unroll
    for (int j = 0; j < ND; ++j) {
      s[j] = a.S[pix * (size_t)n + (size_t)(lane * ND + j)];
      const unsigned k = (s[j] << 8) | (unsigned)(lane * ND + j);
      key = k < key ? k : key;
    }
    key = DS_WAVE_MIN_U32(key);
    const int d_best = (int)(key & 255u), s0 = (int)(key >> 8);
    unsigned m2 = 0xFFFFFFFFu;
#pragma unroll
    for (int j = 0; j < ND; ++j) {
      const int dd = lane * ND + j - d_best;
      if ((dd > 1 || dd < -1) && s[j] < m2) m2 = s[j];
    }
    const long long s2 = (long long)DS_WAVE_MIN_U32(m2);
    const int xr = x - a.d_min - d_best;
    int d_right = -1;
    if (a.lr_max >= 0 && xr >= 0) {  // the right view's disparity at xr from the same volume: the diagonal S(xr + d_min + d, y, d)
      unsigned kr = 0xFFFFFFFFu;
#pragma unroll
      for (int j = 0; j < ND; ++j) {
        const int d = lane * ND + j, xl = xr + a.d_min + d;
        const unsigned v = a.S[((size_t)y * (size_t)a.W + (size_t)(xl < a.W ? xl : a.W - 1)) * (size_t)n + (size_t)d];
        const unsigned k = xl < a.W ? (v << 8) | (unsigned)d : 0xFFFFFFFFu;
        kr = k < kr ? k : kr;
      }
      d_right = (int)(DS_WAVE_MIN_U32(kr) & 255u);
    }
    if (lane != 0) continue;
    int st = 1;
    if (a.lr_max >= 0) {
      const int diff = d_right - d_best;
      if (xr < 0 || diff > a.lr_max || -diff > a.lr_max) st = 3;
    }
    if (s2 * (long long)(100 - a.uniqueness) < (long long)s0 * 100) st = 2;
    if (d_best == 0 || d_best == n - 1) st = 4;
    if (a.mask && a.mask[(size_t)y * a.mask_stride + x] == 0) st = 0;
    float disp = 0.0f;
    if (st == 1) {  // (0 < d_best < n - 1 here)
      const float sm = (float)a.S[pix * (size_t)n + (size_t)(d_best - 1)], sp = (float)a.S[pix * (size_t)n + (size_t)(d_best + 1)];
      const float sc = (float)s0;
      const float den = (sm + sp) - (sc + sc);
      const float off = den != 0.0f ? (0.5f * (sm - sp)) / den : 0.0f;
      disp = (float)(a.d_min + d_best) + off;
    }
    if (a.disp) a.disp[pix] = disp;
    if (a.cost) a.cost[pix] = (uint16_t)(st != 0 ? s0 : 0);
    if (a.sigma_out) a.sigma_out[pix] = st == 1 ? a.sigma : 0.0f;
    if (a.status) a.status[pix] = (uint8_t)st;
  }
}
