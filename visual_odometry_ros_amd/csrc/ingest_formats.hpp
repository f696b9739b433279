// ingest_formats.hpp — one output byte of the rectifying ingestion, per input pixel format (include/vo_hip.h:
// vo_set_input_format has the arithmetic and the reference lines). Included by pyramid.hip (remap_level0_kernel) and, through
// tests/emu/hip_emu.h, by the CPU harness that runs this text against the numpy restatement.
//   MONO8                      remap_sample: the integer form of cv::remap on u8 samples
//   RGB8 / BGR8                the same remap on gray = (c0*9798 + c1*19235 + c2*3735 + 16384) >> 15 of every tap
//   MONO16U / MONO16S / F32    OpenCV's scalar remapBilinear<float>, every product and sum rounded on its own, then convertTo(CV_8UC1)
#pragma once
#include <stdint.h>
#include <stddef.h>

#include "../../include/vo_hip.h"

#if defined(__HIP_DEVICE_COMPILE__)
#define INGEST_FMUL(a, b) __fmul_rn((a), (b))
#define INGEST_FADD(a, b) __fadd_rn((a), (b))
#else  // host text (the emulation harness): compiled with -ffp-contract=off
#define INGEST_FMUL(a, b) ((a) * (b))
#define INGEST_FADD(a, b) ((a) + (b))
#endif

__device__ __forceinline__ int remap_sample(const uint8_t *__restrict__ src, int w, int h, int sstride, float mu,
                                            float mv) {
  if (!(mu == mu) || !(mv == mv)) return 0;  // cvRound(NaN) = INT_MIN on the CPU: far outside
  const int fxq = (int)__builtin_rintf(mu * 32.0f), fyq = (int)__builtin_rintf(mv * 32.0f);  // saturating cvt
  const int sx = fxq >> 5, sy = fyq >> 5, ax = fxq & 31, ay = fyq & 31;
  if (sx >= w || sx + 1 < 0 || sy >= h || sy + 1 < 0) return 0;
  const bool x0 = sx >= 0, x1 = sx + 1 < w, y0 = sy >= 0, y1 = sy + 1 < h;
  const uint8_t *p = src + (ptrdiff_t)sy * sstride + sx;
  const int s00 = (x0 && y0) ? p[0] : 0, s01 = (x1 && y0) ? p[1] : 0;
  const int s10 = (x0 && y1) ? p[sstride] : 0, s11 = (x1 && y1) ? p[sstride + 1] : 0;
  const int sum = s00 * ((32 - ay) * (32 - ax)) + s01 * ((32 - ay) * ax) + s10 * (ay * (32 - ax)) + s11 * (ay * ax);
  return (sum + 511 + ((sum >> 10) & 1)) >> 10;  // round half to even of sum / 1024 (<= 255)
}

// cvtColor(COLOR_RGB2GRAY) on 8-bit data: 15-bit coefficients, channel 0 weighted as R
__device__ __forceinline__ int ingest_gray(int c0, int c1, int c2) {
  return (c0 * 9798 + c1 * 19235 + c2 * 3735 + 16384) >> 15;
}
// One 3-byte group. It starts at any byte address, and a dword load over it would read one byte past the last pixel of the
// caller's buffer: three byte loads (the four taps of neighbouring lanes share their cache lines).
template <int FMT>
__device__ __forceinline__ int ingest_tap_gray(const uint8_t *__restrict__ p) {
  const int a = p[0], b = p[1], c = p[2];
  return FMT == VO_PIX_BGR8 ? ingest_gray(c, b, a) : ingest_gray(a, b, c);
}
// One 2- or 4-byte sample as a float (16-bit values convert exactly). `stride` is in bytes and need not be a multiple of the
// sample size: the copy makes no alignment promise, global loads of gfx950 take any byte address.
template <int FMT>
__device__ __forceinline__ float ingest_tap_float(const uint8_t *__restrict__ p) {
  if (FMT == VO_PIX_MONO16U) {
    uint16_t v;
    __builtin_memcpy(&v, p, 2);
    return (float)v;
  } else if (FMT == VO_PIX_MONO16S) {
    int16_t v;
    __builtin_memcpy(&v, p, 2);
    return (float)v;
  } else {
    float v;
    __builtin_memcpy(&v, p, 4);
    return v;
  }
}
// convertTo(CV_8UC1) of a float: saturate_cast<uchar>(cvRound(s)); x86 cvRound gives INT_MIN for NaN and for |s| >= 2^31
__device__ __forceinline__ int ingest_float_to_u8(float s) {
  if (!(s == s)) return 0;
  if (!(__builtin_fabsf(s) < 2147483648.0f)) return 0;
  const float r = __builtin_rintf(s);  // half to even
  return r <= 0.0f ? 0 : (r >= 255.0f ? 255 : (int)r);
}

template <int FMT>
__device__ __forceinline__ int ingest_sample(const uint8_t *__restrict__ src, int w, int h, int sstride, float mu,
                                             float mv) {
  if (FMT == VO_PIX_MONO8) return remap_sample(src, w, h, sstride, mu, mv);
  if (!(mu == mu) || !(mv == mv)) return 0;
  const int fxq = (int)__builtin_rintf(mu * 32.0f), fyq = (int)__builtin_rintf(mv * 32.0f);
  const int sx = fxq >> 5, sy = fyq >> 5, ax = fxq & 31, ay = fyq & 31;
  if (sx >= w || sx + 1 < 0 || sy >= h || sy + 1 < 0) return 0;
  const bool x0 = sx >= 0, x1 = sx + 1 < w, y0 = sy >= 0, y1 = sy + 1 < h;
  constexpr int B = (FMT == VO_PIX_RGB8 || FMT == VO_PIX_BGR8) ? 3 : (FMT == VO_PIX_F32 ? 4 : 2);
  const uint8_t *p = src + (ptrdiff_t)sy * sstride + (ptrdiff_t)sx * B;
  if (FMT == VO_PIX_RGB8 || FMT == VO_PIX_BGR8) {
    const int s00 = (x0 && y0) ? ingest_tap_gray<FMT>(p) : 0, s01 = (x1 && y0) ? ingest_tap_gray<FMT>(p + B) : 0;
    const int s10 = (x0 && y1) ? ingest_tap_gray<FMT>(p + sstride) : 0, s11 = (x1 && y1) ? ingest_tap_gray<FMT>(p + sstride + B) : 0;
    const int sum = s00 * ((32 - ay) * (32 - ax)) + s01 * ((32 - ay) * ax) + s10 * (ay * (32 - ax)) + s11 * (ay * ax);
    return (sum + 511 + ((sum >> 10) & 1)) >> 10;
  } else {
    const float v00 = (x0 && y0) ? ingest_tap_float<FMT>(p) : 0.0f, v01 = (x1 && y0) ? ingest_tap_float<FMT>(p + B) : 0.0f;
    const float v10 = (x0 && y1) ? ingest_tap_float<FMT>(p + sstride) : 0.0f, v11 = (x1 && y1) ? ingest_tap_float<FMT>(p + sstride + B) : 0.0f;
    const float k = 1.0f / 1024.0f;  // (the integer products are below 2^11 and the scale is a power of two: exact)
    const float w00 = (float)((32 - ay) * (32 - ax)) * k, w01 = (float)((32 - ay) * ax) * k;
    const float w10 = (float)(ay * (32 - ax)) * k, w11 = (float)(ay * ax) * k;
    float s = INGEST_FADD(INGEST_FMUL(v00, w00), INGEST_FMUL(v01, w01));
    s = INGEST_FADD(s, INGEST_FMUL(v10, w10));
    s = INGEST_FADD(s, INGEST_FMUL(v11, w11));
    return ingest_float_to_u8(s);
  }
}
