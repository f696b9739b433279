// orb_describe.hpp — device code of the ORB orientation and descriptor (cv::ORB::compute restated: ICAngles, the 7x7
// sigma-2 Gaussian in fixed point, steered BRIEF with WTA_K 2). include/vo_hip.h ("ORB orientation and descriptors") fixes
// every operation; this text follows it step by step, and tests/test_orb_describe*.py check it against a numpy restatement
// written from that header.
//
// Shape: one 64-lane wavefront per keypoint, ORBD_KP keypoints per workgroup. A wavefront stages the 51 x 51 window of its
// level around the keypoint's centre in LDS with BORDER_REFLECT_101 resolved once (rotated pattern points reach 21 pixels,
// the blur adds 3; 25 is the margin the window keeps), sums the two moments over the disc with one integer wave reduction
// each, then every lane owns 4 of the 256 tests: 8 blurred samples of 49 LDS taps. Lane l's four predicates are bits
// 4 (l & 1) .. 4 (l & 1) + 3 of byte l >> 1; lanes 0, 8, .. 56 gather the dwords.
//
// Plain C++ apart from __global__ / __shared__ / __syncthreads; the includer provides
//   int orb_wave_sum(int v)             sum of v over the caller's wavefront, the same value in every lane
//   int orb_wave_get(int v, int lane)   v of lane `lane` of the caller's wavefront
// (every lane of the wavefront calls them) so that tests/emu/ can run the same text on CPU threads.
#pragma once
#include <math.h>
#include <stdint.h>

#define ORBD_KP 4        // keypoints (wavefronts) per workgroup
#define ORBD_HALF 25     // the staged window is (2 * 25 + 1)^2
#define ORBD_WIN 51
#define ORBD_STRIDE 52   // bytes per staged row
#define ORBD_REACH 22    // |rotated pattern coordinate| <= 15 (|cos| + |sin|) < 21.3; 22 + 3 taps stay inside the window

struct OrbDescLevel {
  const uint8_t *img;
  int w, h, stride;
  float inv_scale;  // 1.f / scale of the level
};
struct OrbDescArgs {
  const OrbDescLevel *levels;  // device memory (the octave of a keypoint is not uniform over a workgroup)
  int n_levels, edge, steer;
  int n;                   // keypoints, when n_dev is null
  const int *n_dev;        // else: their number is read on the device (a detection's count), at most n_cap
  int n_cap;
  const float *kp_xy;      // level-0 pixels
  const int32_t *kp_oct;
  const int8_t *pattern;   // 512 x (x, y)
  float *angle;            // degrees
  uint32_t *desc;          // 8 dwords per keypoint
  uint8_t *valid;
};

// BORDER_REFLECT_101, iterated (a level may be narrower than the window)
__device__ __forceinline__ int orbd_reflect(int p, int n) {
  while (p < 0 || p >= n) p = p < 0 ? -p : 2 * n - 2 - p;
  return p;
}

// cv::fastAtan2 (scalar form): degrees in [0, 360), every operation an individually rounded float operation
__device__ __forceinline__ float orbd_fast_atan2(float y, float x) {
  const float k = (float)(180.0 / 3.14159265358979323846);
  const float p1 = 0.9997878412794807f * k, p3 = -0.3258083974640975f * k, p5 = 0.1555786518463281f * k,
              p7 = -0.04432655554792128f * k;
  const float eps = (float)2.2204460492503131e-16;  // (float)DBL_EPSILON
  const float ax = fabsf(x), ay = fabsf(y);
  float a, c, c2;
  if (ax >= ay) {
    c = ay / (ax + eps);
    c2 = c * c;
    a = (((p7 * c2 + p5) * c2 + p3) * c2 + p1) * c;
  } else {
    c = ax / (ay + eps);
    c2 = c * c;
    a = 90.f - (((p7 * c2 + p5) * c2 + p3) * c2 + p1) * c;
  }
  if (x < 0.f) a = 180.f - a;
  if (y < 0.f) a = 360.f - a;
  return a;
}

// the blurred pixel at window position (x, y): sum of k_i k_j p(x + i, y + j), + 2^15, >> 16 (exact in 32 bits; the order of
// an integer sum is free, so the two passes of the definition collapse into one)
__device__ __forceinline__ int orbd_blur(const uint8_t *__restrict__ win, int x, int y) {
  const uint8_t *p = win + (y - 3) * ORBD_STRIDE + (x - 3);
  int acc = 0;
#pragma unroll
  for (int j = 0; j < 7; ++j) {
    const int kj = j == 3 ? 54 : (j == 2 || j == 4) ? 49 : (j == 1 || j == 5) ? 34 : 18;
    const uint8_t *q = p + j * ORBD_STRIDE;
    const int row = 18 * (q[0] + q[6]) + 34 * (q[1] + q[5]) + 49 * (q[2] + q[4]) + 54 * q[3];
    acc += kj * row;
  }
  return (acc + 32768) >> 16;
}

__global__ __launch_bounds__(64 * ORBD_KP) void orb_describe_kernel(OrbDescArgs a) {
  __shared__ __attribute__((aligned(16))) uint8_t s_win[ORBD_KP][ORBD_WIN * ORBD_STRIDE];
  __shared__ __attribute__((aligned(16))) int8_t s_pat[1024];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int k = (int)blockIdx.x * ORBD_KP + wave;
  int n = a.n;
  if (a.n_dev) {
    n = *a.n_dev;
    if (n > a.n_cap) n = a.n_cap;
  }
  ((uint32_t *)s_pat)[tid] = ((const uint32_t *)a.pattern)[tid];  // 256 lanes x 4 bytes
  uint8_t *win = s_win[wave];
  bool ok = false;
  if (k < n) {
    const int oct = a.kp_oct[k];
    if (oct >= 0 && oct < a.n_levels) {
      const OrbDescLevel L = a.levels[oct];
      const float xf = rintf(a.kp_xy[2 * k] * L.inv_scale), yf = rintf(a.kp_xy[2 * k + 1] * L.inv_scale);
      // (float compares: a NaN coordinate is invalid, and nothing out of int range is converted)
      ok = xf >= (float)a.edge && xf < (float)(L.w - a.edge) && yf >= (float)a.edge && yf < (float)(L.h - a.edge);
      if (ok) {
        const int cx = (int)xf, cy = (int)yf;
        if (lane < ORBD_WIN) {
          const int sx = orbd_reflect(cx - ORBD_HALF + lane, L.w);
          for (int r = 0; r < ORBD_WIN; ++r) {
            const int sy = orbd_reflect(cy - ORBD_HALF + r, L.h);
            win[r * ORBD_STRIDE + lane] = L.img[(size_t)sy * L.stride + sx];
          }
        }
      }
    }
  }
  __syncthreads();
  if (k >= n) return;  // (whole wavefronts)
  if (!ok) {
    if (lane < 8) a.desc[(size_t)k * 8 + lane] = 0u;
    if (lane == 0) {
      a.angle[k] = 0.f;
      a.valid[k] = 0;
    }
    return;
  }
  // ICAngles on the unblurred window: the 31 x 31 square in raster order, 64 positions at a time, masked to the disc
  int m10 = 0, m01 = 0;
  if (a.steer) {
    for (int i = lane; i < 31 * 31; i += 64) {
      const int r = i / 31, u = i - r * 31 - 15, v = r - 15, av = v < 0 ? -v : v;
      const int umax = (int)((0x3689ABCDDEEEFFFFull >> (4 * av)) & 15);  // 15 15 15 15 14 14 14 13 13 12 11 10 9 8 6 3
      if (u >= -umax && u <= umax) {
        const int I = win[(ORBD_HALF + v) * ORBD_STRIDE + ORBD_HALF + u];
        m10 += u * I;
        m01 += v * I;
      }
    }
    m10 = orb_wave_sum(m10);
    m01 = orb_wave_sum(m01);
  }
  const float ang = a.steer ? orbd_fast_atan2((float)m01, (float)m10) : 0.f;
  const double rad = (double)(ang * (float)(3.14159265358979323846 / 180.0));
  const float ca = (float)cos(rad), sa = (float)sin(rad);
  unsigned bits = 0;
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    int val[2];
#pragma unroll
    for (int e = 0; e < 2; ++e) {
      const int pi = 2 * (4 * lane + t) + e;
      const float px = (float)s_pat[2 * pi], py = (float)s_pat[2 * pi + 1];
      int ix = (int)rintf(px * ca - py * sa), iy = (int)rintf(px * sa + py * ca);
      // never taken for a table in [-15, 15]: keeps every tap inside the window whatever the table holds
      ix = ix < -ORBD_REACH ? -ORBD_REACH : ix > ORBD_REACH ? ORBD_REACH : ix;
      iy = iy < -ORBD_REACH ? -ORBD_REACH : iy > ORBD_REACH ? ORBD_REACH : iy;
      val[e] = orbd_blur(win, ORBD_HALF + ix, ORBD_HALF + iy);
    }
    bits |= (unsigned)(val[0] < val[1]) << t;
  }
  // test 4 l + t is bit (4 l + t) & 7 of byte (4 l + t) >> 3: lane l holds a nibble, eight lanes a dword
  unsigned word = 0;
#pragma unroll
  for (int q = 0; q < 8; ++q) word |= (unsigned)orb_wave_get((int)bits, (lane & ~7) + q) << (4 * q);
  if ((lane & 7) == 0) a.desc[(size_t)k * 8 + (lane >> 3)] = word;
  if (lane == 0) {
    a.angle[k] = ang;
    a.valid[k] = 1;
  }
}
