// zncc_device.hpp — the kernel of image_processing::calcZNCC on the device (include/vo_hip.h: vo_zncc has the arithmetic;
// DESIGN.md §16). Included by zncc.hip and, through tests/emu/hip_emu.h, by the CPU harness (tests/emu/emu_zncc.cpp) that runs
// this text against the numpy restatement (tests/zncc_restatement.py).
//
//   zncc_kernel<REF, J>  grid (ceil(n / ZNCC_WAVES), pairs). One wavefront per feature, ZNCC_WAVES features per workgroup;
//                        blockIdx.y names the image pair. Lane l holds taps l, l + 64, ... of both patches in J registers each
//                        (J = 1, 2, 4, 8, 16 by the window: 31 x 31 = 961 taps need 16), sampled straight from the u8 level-0
//                        planes. Every product, sum and difference is rounded to float on its own (no FMA).
//                        REF == false: the tree sum — taps zero-padded to P = 64 * J, strides P/2 .. 64 are adds between a lane's
//                        own registers, strides 32 .. 1 take the value of lane l + stride; lane 0 has the sum. No LDS.
//                        REF == true: the patches go to LDS and lane 0 adds them in index order, as the reference's loops do.
//
// What the includer provides: ZNCC_SHFL_DOWN(v, d) (the float of lane + d of the caller's wavefront; any value where lane + d
// >= 64) and ZNCC_BCAST0(v) (lane 0's float in every lane). Every thread of a wavefront reaches both, whatever its data.
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIP_DEVICE_COMPILE__)
#define ZNCC_FMUL(a, b) __fmul_rn((a), (b))
#define ZNCC_FADD(a, b) __fadd_rn((a), (b))
#define ZNCC_FSUB(a, b) __fsub_rn((a), (b))
#else  // host text (the emulation harness): compiled with -ffp-contract=off
#define ZNCC_FMUL(a, b) ((a) * (b))
#define ZNCC_FADD(a, b) ((a) + (b))
#define ZNCC_FSUB(a, b) ((a) - (b))
#endif

#define ZNCC_WAVES 4       // features per workgroup
#define ZNCC_NT (64 * ZNCC_WAVES)
#define ZNCC_MIN_WIN 3
#define ZNCC_MAX_WIN 31    // 961 taps: 16 per lane
#define ZNCC_INVALID -2.0f // what interpImage's resize(n, -2.0f) leaves at a tap outside the image
#define ZNCC_NAN __builtin_nanf("")

struct ZnccPair {
  const uint8_t *I0, *I1;  // level-0 pixel (0, 0) of the two images, W x H each
  int stride0, stride1;    // bytes per row
  const float *pts0, *pts1;  // [n][2]: the patch anchors in I0 / I1
  float *out;              // [n]
};
struct ZnccArgs {
  ZnccPair pair[2];
  int W, H, n;             // W, H >= 2
  int win, off;            // taps (i - off, j - off), i, j < win; off = win (the reference's text) or win / 2 (centred)
  int n_elem, J;           // win * win; registers per lane: P / 64, P = the next power of two >= max(n_elem, 64)
  int q64, r64;            // 64 / win, 64 % win
};

// window -> the launch's numbers (host code, shared by the launcher and the harness); pattern: 0 reference, 1 centred
static inline void zncc_plan(ZnccArgs *a, int win, int pattern) {
  a->win = win;
  a->off = pattern ? win / 2 : win;
  a->n_elem = win * win;
  int P = 64;
  while (P < a->n_elem) P *= 2;
  a->J = P / 64;
  a->q64 = 64 / win;
  a->r64 = 64 % win;
}

// interpImage (image_processing.cpp:28-77) at one point of a u8 image: (int) truncates toward zero, so u in (-1, 0) has u0 = 0
// and a negative ax; valid iff 0 <= u0 < W - 1 and 0 <= v0 < H - 1, which for a float is -1 < u < W - 1 (false for NaN).
// Without a branch: an invalid tap loads the four pixels at (0, 0) (inside the image) and drops the value, so that the loads
// of a lane's taps are in flight together.
__device__ __forceinline__ float zncc_sample(const uint8_t *I, int stride, int W, int H, float u, float v) {
  const bool valid = u > -1.0f && u < (float)(W - 1) && v > -1.0f && v < (float)(H - 1);
  const float uc = valid ? u : 0.0f, vc = valid ? v : 0.0f;
  const int u0 = (int)uc, v0 = (int)vc;
  const float ax = ZNCC_FSUB(uc, (float)u0), ay = ZNCC_FSUB(vc, (float)v0);
  const float axay = ZNCC_FMUL(ax, ay);
  const uint8_t *p = I + (size_t)v0 * (size_t)stride + (size_t)u0;
  const float I1 = (float)p[0], I2 = (float)p[1], I3 = (float)p[stride], I4 = (float)p[stride + 1];
  float r = ZNCC_FMUL(axay, ZNCC_FADD(ZNCC_FSUB(ZNCC_FSUB(I1, I2), I3), I4));
  r = ZNCC_FADD(r, ZNCC_FMUL(ax, ZNCC_FADD(-I1, I2)));
  r = ZNCC_FADD(r, ZNCC_FMUL(ay, ZNCC_FADD(-I1, I3)));
  r = ZNCC_FADD(r, I1);
  return valid ? r : ZNCC_INVALID;
}

// the tree over P = 64 * J terms, t[j] = term lane + 64 * j: s[i] += s[i + stride] for stride = P/2 .. 1; every lane returns lane 0's
template <int J>
__device__ __forceinline__ float zncc_tree_sum(float (&t)[J]) {
#pragma unroll
  for (int m = J / 2; m >= 1; m >>= 1) {
#pragma unroll
    for (int j = 0; j < m; ++j) t[j] = ZNCC_FADD(t[j], t[j + m]);
  }
  float s = t[0];
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    const float o = ZNCC_SHFL_DOWN(s, d);
    s = ZNCC_FADD(s, o);
  }
  return ZNCC_BCAST0(s);
}

template <bool REF, int J>
__global__ __launch_bounds__(ZNCC_NT) void zncc_kernel(ZnccArgs a) {
  const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6;
  const int f = (int)blockIdx.x * ZNCC_WAVES + wave;
  const bool active = f < a.n;  // (a whole wavefront: the grid is sized by n)
  const ZnccPair &p = a.pair[blockIdx.y];
  float v0[J], v1[J];
  float x0 = 0.0f, y0 = 0.0f, x1 = 0.0f, y1 = 0.0f;
  if (active) {
    x0 = p.pts0[2 * f];
    y0 = p.pts0[2 * f + 1];
    x1 = p.pts1[2 * f];
    y1 = p.pts1[2 * f + 1];
  }
  // tap k = lane + 64 * j is (ti, tj) = (k / win, k % win); from one round to the next k grows by 64 = q64 * win + r64
  int ti = lane / a.win, tj = lane - ti * a.win;
#pragma unroll
  for (int j = 0; j < J; ++j) {
    const bool tap = active && lane + 64 * j < a.n_elem;
    const float ox = (float)(ti - a.off), oy = (float)(tj - a.off);  // patt[ind] = (i - o, j - o): i runs along x
    // (a lane without a tap samples a NaN coordinate: invalid, nothing but the pixels at (0, 0) is read)
    const float s0 = zncc_sample(p.I0, p.stride0, a.W, a.H, tap ? ZNCC_FADD(x0, ox) : ZNCC_NAN, ZNCC_FADD(y0, oy));
    const float s1 = zncc_sample(p.I1, p.stride1, a.W, a.H, tap ? ZNCC_FADD(x1, ox) : ZNCC_NAN, ZNCC_FADD(y1, oy));
    v0[j] = tap ? s0 : 0.0f;  // (0: the padding)
    v1[j] = tap ? s1 : 0.0f;
    ti += a.q64;
    tj += a.r64;
    if (tj >= a.win) {
      tj -= a.win;
      ++ti;
    }
  }
  const float fn = (float)a.n_elem;
  if constexpr (REF) {
    // index order: the two patches through LDS, one lane adds
    __shared__ float s_patch[ZNCC_WAVES][2][64 * J];
#pragma unroll
    for (int j = 0; j < J; ++j) {
      s_patch[wave][0][lane + 64 * j] = v0[j];
      s_patch[wave][1][lane + 64 * j] = v1[j];
    }
    __syncthreads();
    if (active && lane == 0) {
      const float *q0 = s_patch[wave][0], *q1 = s_patch[wave][1];
      float mean_l = 0.0f, mean_r = 0.0f;
      for (int k = 0; k < a.n_elem; ++k) {
        mean_l = ZNCC_FADD(mean_l, q0[k]);
        mean_r = ZNCC_FADD(mean_r, q1[k]);
      }
      mean_l = mean_l / fn;
      mean_r = mean_r / fn;
      float numer = 0.0f, denom_l = 0.0f, denom_r = 0.0f;
      for (int k = 0; k < a.n_elem; ++k) {
        const float dl = ZNCC_FSUB(q0[k], mean_l), dr = ZNCC_FSUB(q1[k], mean_r);
        numer = ZNCC_FADD(numer, ZNCC_FMUL(dl, dr));
        denom_l = ZNCC_FADD(denom_l, ZNCC_FMUL(dl, dl));
        denom_r = ZNCC_FADD(denom_r, ZNCC_FMUL(dr, dr));
      }
      p.out[f] = numer / sqrtf(ZNCC_FMUL(denom_l, denom_r));
    }
  } else {
    float t[J];
#pragma unroll
    for (int j = 0; j < J; ++j) t[j] = v0[j];
    const float mean_l = zncc_tree_sum<J>(t) / fn;
#pragma unroll
    for (int j = 0; j < J; ++j) t[j] = v1[j];
    const float mean_r = zncc_tree_sum<J>(t) / fn;
    float tn[J], tl[J], tr[J];
#pragma unroll
    for (int j = 0; j < J; ++j) {
      tn[j] = tl[j] = tr[j] = 0.0f;
      if (lane + 64 * j < a.n_elem) {
        const float dl = ZNCC_FSUB(v0[j], mean_l), dr = ZNCC_FSUB(v1[j], mean_r);
        tn[j] = ZNCC_FMUL(dl, dr);
        tl[j] = ZNCC_FMUL(dl, dl);
        tr[j] = ZNCC_FMUL(dr, dr);
      }
    }
    const float numer = zncc_tree_sum<J>(tn);
    const float denom_l = zncc_tree_sum<J>(tl);
    const float denom_r = zncc_tree_sum<J>(tr);
    if (active && lane == 0) p.out[f] = numer / sqrtf(ZNCC_FMUL(denom_l, denom_r));
  }
}

// the instance for a summation order and J = 1, 2, 4, 8 or 16 registers per lane (zncc_plan); null for any other J
typedef void (*zncc_kernel_fn)(ZnccArgs);
template <bool REF>
static inline zncc_kernel_fn zncc_kernel_for_j(int J) {
  switch (J) {
    case 1: return zncc_kernel<REF, 1>;
    case 2: return zncc_kernel<REF, 2>;
    case 4: return zncc_kernel<REF, 4>;
    case 8: return zncc_kernel<REF, 8>;
    case 16: return zncc_kernel<REF, 16>;
  }
  return nullptr;
}
static inline zncc_kernel_fn zncc_kernel_for(bool ref, int J) { return ref ? zncc_kernel_for_j<true>(J) : zncc_kernel_for_j<false>(J); }
