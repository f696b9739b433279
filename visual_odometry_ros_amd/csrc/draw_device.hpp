// draw_device.hpp — the debug image's rasterisation rules (include/vo_hip.h: vo_draw_tracking / vo_draw_tracking_ba): which
// primitive a number stands for, which pixels it covers, which colour it has. Included by draw.hip (the coverage and resolve
// kernels) and, through tests/emu/hip_emu.h, by the CPU harness that runs this text against the numpy restatement.
//
// Primitives are numbered in the reference's drawing order (showTracking / showTrackingBA of both drivers):
//   tracking:     [0, n1)  line pts0[i] -> pts1[i]; then for every point of pts0, of pts1 and of pts_new two numbers each:
//                 circle(3, 2) in black, circle(2, 1) in the set's colour
//   tracking_ba:  [0, n0)  circle(1, 4) around pts[i];  [n0, n0 + n1)  rect(6, 2) around pts_proj[i]
// A pixel takes the colour of the highest-numbered primitive that covers it: the coverage pass keeps that maximum per pixel.
#pragma once
#include <stdint.h>

struct DrawJob {
  int mode;                    // 0: tracking, 1: tracking_ba
  int n0, n1, n2;              // tracking: pts0, pts1 (lines for i < n1 <= n0), pts_new; tracking_ba: pts, pts_proj
  const float *p0, *p1, *p2;   // x y pairs
  int w, h;
};
enum { DRAW_LINE = 0, DRAW_CIRCLE = 1, DRAW_RECT = 2 };
enum { DRAW_REACH = 7, DRAW_BOX = 2 * DRAW_REACH + 1 };  // no stamp reaches further than 7 pixels from its centre
struct DrawPrim {
  int kind, r, t;              // circle(r, t) / rect(r, t)
  int ax, ay, bx, by;          // centre, or the line's end points
  bool ok;                     // false: a coordinate is NaN or |coordinate| >= 2^30 — nothing is drawn
};

__host__ __device__ __forceinline__ int draw_prim_count(const DrawJob &j) {
  return j.mode == 0 ? j.n1 + 2 * (j.n0 + j.n1 + j.n2) : j.n0 + j.n1;
}
// c = (rint(x), rint(y)), half to even
__device__ __forceinline__ bool draw_centre(const float *p, int &cx, int &cy) {
  const float x = p[0], y = p[1];
  if (!(__builtin_fabsf(x) < 1073741824.0f) || !(__builtin_fabsf(y) < 1073741824.0f)) return false;  // (NaN fails both)
  cx = (int)__builtin_rintf(x);
  cy = (int)__builtin_rintf(y);
  return true;
}
// circle(r, t): max(0, 2r - t)^2 <= 4 (dx^2 + dy^2) <= (2r + t)^2
__device__ __forceinline__ bool draw_circle_covers(int dx, int dy, int r, int t) {
  const int d = 4 * (dx * dx + dy * dy), lo = 2 * r - t > 0 ? 2 * r - t : 0, hi = 2 * r + t;
  return lo * lo <= d && d <= hi * hi;
}
// rect(h, t): 2h - t <= 2 max(|dx|, |dy|) <= 2h + t
__device__ __forceinline__ bool draw_rect_covers(int dx, int dy, int h, int t) {
  const int ax = dx < 0 ? -dx : dx, ay = dy < 0 ? -dy : dy, m = 2 * (ax > ay ? ax : ay);
  return 2 * h - t <= m && m <= 2 * h + t;
}
// floor((2 k d + n) / (2 n)) for 0 <= k <= n, |d| <= n < 2^31 + 1: the products reach 2^63, so unsigned, sign apart
__device__ __forceinline__ long long draw_line_step(long long k, long long d, long long n) {
  const unsigned long long m = 2ull * (unsigned long long)k * (unsigned long long)(d < 0 ? -d : d), n2 = 2ull * (unsigned long long)n;
  return d >= 0 ? (long long)((m + (unsigned long long)n) / n2) : -(long long)((m + (unsigned long long)n - 1ull) / n2);
}
// the k of a line whose pixel can lie inside the image: along the major axis the coordinate is a + sign * k exactly
__device__ __forceinline__ void draw_line_range(const DrawPrim &P, int w, int h, long long &n, long long &k0, long long &k1) {
  const long long dx = (long long)P.bx - P.ax, dy = (long long)P.by - P.ay;
  const long long adx = dx < 0 ? -dx : dx, ady = dy < 0 ? -dy : dy;
  n = adx > ady ? adx : ady;
  const bool xmajor = adx == n;
  const long long a0 = xmajor ? P.ax : P.ay, lim = xmajor ? w : h, d = xmajor ? dx : dy;
  k0 = d > 0 ? -a0 : a0 - (lim - 1);
  k1 = d > 0 ? lim - 1 - a0 : a0;
  if (n == 0) k0 = k1 = 0;  // the one pixel (the caller clips it)
  if (k0 < 0) k0 = 0;
  if (k1 > n) k1 = n;
}

__device__ __forceinline__ DrawPrim draw_decode(const DrawJob &j, int prim) {
  DrawPrim P;
  P.r = P.t = 0;
  P.bx = P.by = 0;
  if (j.mode == 0) {
    if (prim < j.n1) {
      P.kind = DRAW_LINE;
      const bool a = draw_centre(j.p0 + 2 * prim, P.ax, P.ay), b = draw_centre(j.p1 + 2 * prim, P.bx, P.by);
      P.ok = a && b;
      return P;
    }
    int q = prim - j.n1;
    const float *p = j.p0;
    if (q >= 2 * j.n0) {
      q -= 2 * j.n0;
      p = j.p1;
      if (q >= 2 * j.n1) {
        q -= 2 * j.n1;
        p = j.p2;
      }
    }
    P.kind = DRAW_CIRCLE;
    P.r = (q & 1) ? 2 : 3;
    P.t = (q & 1) ? 1 : 2;
    P.ok = draw_centre(p + 2 * (q >> 1), P.ax, P.ay);
    return P;
  }
  if (prim < j.n0) {
    P.kind = DRAW_CIRCLE;
    P.r = 1;
    P.t = 4;
    P.ok = draw_centre(j.p0 + 2 * prim, P.ax, P.ay);
  } else {
    P.kind = DRAW_RECT;
    P.r = 6;
    P.t = 2;
    P.ok = draw_centre(j.p1 + 2 * (prim - j.n0), P.ax, P.ay);
  }
  return P;
}

// channel k of the image receives component k of the reference's cv::Scalar: byte 0 | byte 1 << 8 | byte 2 << 16
__device__ __forceinline__ uint32_t draw_colour(const DrawJob &j, int prim) {
  if (j.mode == 0) {
    if (prim < j.n1) return 0x00FFFF00u;  // (0, 255, 255)
    const int q = prim - j.n1;
    if (!(q & 1)) return 0u;              // black
    if (q < 2 * j.n0) return 0x00FF00FFu;              // (255, 0, 255)
    if (q < 2 * (j.n0 + j.n1)) return 0x0000FF00u;     // (0, 255, 0)
    return 0x000000FFu;                                // (255, 0, 0)
  }
  return prim < j.n0 ? 0x00FF0000u : 0x0000FF00u;      // (0, 0, 255) / (0, 255, 0)
}

// Lane `tid` of `nt` reports its share of the pixels primitive `prim` covers inside the image: emit(x, y).
template <class Emit>
__device__ __forceinline__ void draw_cover(const DrawJob &j, int prim, int tid, int nt, Emit emit) {
  const DrawPrim P = draw_decode(j, prim);
  if (!P.ok) return;
  if (P.kind == DRAW_LINE) {
    long long n, k0, k1;
    draw_line_range(P, j.w, j.h, n, k0, k1);
    const long long dx = (long long)P.bx - P.ax, dy = (long long)P.by - P.ay;
    for (long long k = k0 + tid; k <= k1; k += nt) {
      const long long x = P.ax + (n ? draw_line_step(k, dx, n) : 0), y = P.ay + (n ? draw_line_step(k, dy, n) : 0);
      if (x >= 0 && x < j.w && y >= 0 && y < j.h) emit((int)x, (int)y);
    }
    return;
  }
  for (int o = tid; o < DRAW_BOX * DRAW_BOX; o += nt) {
    const int dy = o / DRAW_BOX - DRAW_REACH, dx = o % DRAW_BOX - DRAW_REACH;
    const bool in = P.kind == DRAW_CIRCLE ? draw_circle_covers(dx, dy, P.r, P.t) : draw_rect_covers(dx, dy, P.r, P.t);
    const long long x = (long long)P.ax + dx, y = (long long)P.ay + dy;
    if (in && x >= 0 && x < j.w && y >= 0 && y < j.h) emit((int)x, (int)y);
  }
}
