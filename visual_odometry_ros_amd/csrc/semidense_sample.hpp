// semidense_sample.hpp — what the semi-dense kernels that sample an image at a float position share (semidense_temporal_device.hpp,
// semidense_align_device.hpp): float32 operations that are rounded one by one, the position in 1/32 pixel, the integer inside test
// and the 12-bit bilinear value (include/vo_hip.h, "Semi-dense temporal": taps). Plain C++ apart from __device__.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#if defined(__HIP_DEVICE_COMPILE__)
#define SDT_MUL(a, b) __fmul_rn((a), (b))
#define SDT_ADD(a, b) __fadd_rn((a), (b))
#define SDT_SUB(a, b) __fsub_rn((a), (b))
#else  // host text (the launcher's few products, the emulation harness): compiled with -ffp-contract=off
#define SDT_MUL(a, b) ((a) * (b))
#define SDT_ADD(a, b) ((a) + (b))
#define SDT_SUB(a, b) ((a) - (b))
#endif

// a coordinate in 1/32 pixel; what cannot be a tap of an image of up to 65535 pixels a side (NaN included) becomes a value whose cell
// is negative
__device__ static inline int sdt_q(float p) {
  const float t = floorf(SDT_ADD(SDT_MUL(32.0f, p), 0.5f));
  return (t >= -1048576.0f && t <= 4194304.0f) ? (int)t : -1048576;
}
// the 2 x 2 cells of the tap lie in [0, W-1] x [0, H-1]
__device__ static inline bool sdt_in(int X, int Y, int W, int H) {
  const int cx = X >> 5, cy = Y >> 5;
  return cx >= 0 && cx <= W - 2 && cy >= 0 && cy <= H - 2;
}
// the bilinear value in 12 bits (0 .. 4080), integer weights that sum to 1024. The cell is clamped BEFORE the address is formed:
// whatever X, Y hold, the four bytes read lie inside the W x H image (W, H >= 2).
__device__ static inline int sdt_sample(const uint8_t *img, int stride, int W, int H, int X, int Y) {
  int cx = X >> 5, cy = Y >> 5;
  cx = cx < 0 ? 0 : (cx > W - 2 ? W - 2 : cx);
  cy = cy < 0 ? 0 : (cy > H - 2 ? H - 2 : cy);
  const int wx = X & 31, wy = Y & 31;
  const uint8_t *p = img + (size_t)cy * (size_t)stride + (size_t)cx;
  const int top = (32 - wx) * (int)p[0] + wx * (int)p[1], bot = (32 - wx) * (int)p[stride] + wx * (int)p[stride + 1];
  return ((32 - wy) * top + wy * bot + 32) >> 6;
}
