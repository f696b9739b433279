// semidense_propagate_device.hpp — the kernels that carry a keyframe's semi-dense map over to the next keyframe (include/vo_hip.h,
// "Semi-dense propagation", has the definition). Included by semidense_propagate.hip and, through tests/emu/hip_emu.h,
// by the CPU harness (tests/emu/emu_semidense_propagate.cpp) that runs this text against the numpy restatement
// (tests/semidense_propagate_restatement.py).
//
//   semidense_propagate_scatter_kernel   one lane per pixel of the old map, SDP_NT threads. A source that passes the tests of the
//                      definition, in its order, does one 64-bit unsigned atomicMax on the W x H plane of keys at its target:
//                      (bits(invd_b) << 32) | (0xFFFFFFFF - source index). invd_b > 0, so its bits order like the float and no key is
//                      0: the plane's maximum is the definition's winner (the nearest; on equal bits the smallest source index)
//                      whatever the arrival order. The target's address — in the new left plane, its mask and the keys — is formed
//                      from coordinates clamped to the image BEFORE it is formed, as sdt_sample does; a source whose target fails
//                      the integer inside test never reaches the atomic.
//   semidense_propagate_resolve_kernel   one lane per pixel of the new map. It decodes its key, recomputes the winner's invd_b,
//                      sigma_b and n_obs from the old map at the decoded index by the same function the scatter used (the bits are
//                      the restatement's), fuses with the static planes and writes the new map, origin and src with plain stores —
//                      a different set of planes than the old map, which other lanes still read — and stores 0 back into its key:
//                      the plane, zeroed once at allocation, is clean for the next call without a memset launch.
//
// The includer provides nothing but __global__, the built-in indices, atomicMax and __float_as_uint.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "semidense_map_fuse.hpp"  // sdm_fuse: the consistency test and the fusion, shared with the map merge

#if defined(__HIP_DEVICE_COMPILE__)
#define SDP_MUL(a, b) __fmul_rn((a), (b))
#define SDP_ADD(a, b) __fadd_rn((a), (b))
#define SDP_SUB(a, b) __fsub_rn((a), (b))
#else  // host text (the emulation harness): compiled with -ffp-contract=off
#define SDP_MUL(a, b) ((a) * (b))
#define SDP_ADD(a, b) ((a) + (b))
#define SDP_SUB(a, b) ((a) - (b))
#endif

#define SDP_NT 256
#define SDP_FRONT 0.1f            // a2 + invd t2 (the depth in the new camera over the depth in the old one) must exceed this
#define SDP_FLT_MAX 3.4028235e38f

struct SdpArgs {
  const float *invd_a, *sigma_a;  // the old map, W x H planes, tightly packed
  const uint8_t *n_obs_a;
  const uint8_t *La, *Lb;         // level-0 pixel (0, 0) of the old / new keyframe's left image
  int strideA, strideB;           // bytes per row
  int W, H;
  const uint8_t *mask;            // the new keyframe's ignore mask (0 = ignore), null: none
  int mask_stride;
  int min_obs, max_diff;
  float chi2, sigma_add2;         // chi chi, sigma_add sigma_add
  float fx, fy, cx, cy;
  float R[9], t[3];               // X_b = R X_a + t
  unsigned long long *keys;       // W x H, all 0 between calls
  const float *disp, *sigma_invd; // the new pair's static planes
  const uint8_t *status;
  float bf;
  float *invd, *sigma;            // the new map
  uint8_t *n_obs, *tstatus;
  uint8_t *origin;                // may be null
  int32_t *src;                   // may be null
};

static inline void sdp_pose(SdpArgs *a, const float T[16]) {
  for (int r = 0; r < 3; ++r) {
    for (int c = 0; c < 3; ++c) a->R[3 * r + c] = T[4 * r + c];
    a->t[r] = T[4 * r + 3];
  }
}

// the source at raster index i of the old map in the new camera; false: no source, or dropped before the target is formed
__device__ static inline bool sdp_warp(const SdpArgs &a, int i, float *invd_b, float *sigma_b, float *px, float *py, int *no) {
  *no = (int)a.n_obs_a[i];
  const float r = a.invd_a[i], sg = a.sigma_a[i];
  if (!(*no >= a.min_obs && sg > 0.0f && r > 0.0f)) return false;
  const int y = i / a.W, x = i - y * a.W;
  const float xc = SDP_SUB((float)x, a.cx), yc = SDP_SUB((float)y, a.cy);
  const float u = xc / a.fx, v = yc / a.fy;
  const float a0 = SDP_ADD(SDP_ADD(SDP_MUL(a.R[0], u), SDP_MUL(a.R[1], v)), a.R[2]);
  const float a1 = SDP_ADD(SDP_ADD(SDP_MUL(a.R[3], u), SDP_MUL(a.R[4], v)), a.R[5]);
  const float a2 = SDP_ADD(SDP_ADD(SDP_MUL(a.R[6], u), SDP_MUL(a.R[7], v)), a.R[8]);
  const float D = SDP_ADD(a2, SDP_MUL(r, a.t[2]));
  if (!(D > SDP_FRONT)) return false;
  *invd_b = r / D;
  *px = SDP_ADD(SDP_MUL(a.fx, SDP_ADD(a0, SDP_MUL(r, a.t[0])) / D), a.cx);
  *py = SDP_ADD(SDP_MUL(a.fy, SDP_ADD(a1, SDP_MUL(r, a.t[1])) / D), a.cy);
  const float sw = SDP_MUL(sg, fabsf(a2)) / SDP_MUL(D, D);
  *sigma_b = sqrtf(SDP_ADD(SDP_MUL(sw, sw), a.sigma_add2));
  return *invd_b > 0.0f && *invd_b <= SDP_FLT_MAX && *sigma_b > 0.0f && *sigma_b <= SDP_FLT_MAX;
}

// the nearest pixel; what cannot be a pixel of an image of up to 65535 a side (NaN included) becomes a negative value
__device__ static inline int sdp_pix(float p) {
  const float t = floorf(SDP_ADD(p, 0.5f));
  return (t >= -1048576.0f && t <= 4194304.0f) ? (int)t : -1048576;
}

__global__ __launch_bounds__(SDP_NT) void semidense_propagate_scatter_kernel(SdpArgs a) {
  const int i = (int)blockIdx.x * SDP_NT + (int)threadIdx.x;
  const int W = a.W, H = a.H;
  if (i >= W * H) return;
  float invd_b, sigma_b, px, py;
  int no;
  if (!sdp_warp(a, i, &invd_b, &sigma_b, &px, &py, &no)) return;
  const int X = sdp_pix(px), Y = sdp_pix(py);
  const bool in = X >= 1 && X <= W - 2 && Y >= 1 && Y <= H - 2;
  const int Xc = X < 0 ? 0 : (X > W - 1 ? W - 1 : X), Yc = Y < 0 ? 0 : (Y > H - 1 ? H - 1 : Y);  // clamped before any address
  if (!in) return;
  if (a.mask && a.mask[(size_t)Yc * (size_t)a.mask_stride + (size_t)Xc] == 0) return;
  const int y = i / W, x = i - y * W;
  const int va = (int)a.La[(size_t)y * (size_t)a.strideA + (size_t)x], vb = (int)a.Lb[(size_t)Yc * (size_t)a.strideB + (size_t)Xc];
  const int df = va > vb ? va - vb : vb - va;
  if (df > a.max_diff) return;
  const unsigned long long key = ((unsigned long long)__float_as_uint(invd_b) << 32) | (unsigned long long)(0xFFFFFFFFu - (unsigned)i);
  atomicMax(a.keys + ((size_t)Yc * (size_t)W + (size_t)Xc), key);
}

__global__ __launch_bounds__(SDP_NT) void semidense_propagate_resolve_kernel(SdpArgs a) {
  const int j = (int)blockIdx.x * SDP_NT + (int)threadIdx.x;
  const int n = a.W * a.H;
  if (j >= n) return;
  const unsigned long long key = a.keys[j];
  bool has = key != 0ull;
  int s = -1, no = 0;
  float invd_b = 0.0f, sigma_b = 0.0f, px, py;
  if (has) {
    const unsigned d = 0xFFFFFFFFu - (unsigned)(key & 0xFFFFFFFFull);
    s = d < (unsigned)n ? (int)d : 0;  // (a key the scatter wrote decodes inside the plane; the clamp keeps any other word there too)
    has = sdp_warp(a, s, &invd_b, &sigma_b, &px, &py, &no);
    a.keys[j] = 0ull;
  }
  if (!has) s = -1;
  const bool st = a.status[j] == 1;
  const float rho_s = st ? a.disp[j] / a.bf : 0.0f, sig_s = st ? a.sigma_invd[j] : 0.0f;
  float o_invd = 0.0f, o_sig = 0.0f;
  int o_no = 0, org = 0;
  if (st && has) {
    if (sdm_fuse(invd_b, sigma_b, rho_s, sig_s, a.chi2, &o_invd, &o_sig)) {
      org = 3;
      o_no = no < 255 ? no + 1 : 255;
    } else {
      org = 4, o_invd = rho_s, o_sig = sig_s, o_no = 1;
    }
  } else if (st) {
    org = 1, o_invd = rho_s, o_sig = sig_s, o_no = 1;
  } else if (has) {
    org = 2, o_invd = invd_b, o_sig = sigma_b, o_no = no;
  }
  a.invd[j] = o_invd;
  a.sigma[j] = o_sig;
  a.n_obs[j] = (uint8_t)o_no;
  a.tstatus[j] = 0;
  if (a.origin) a.origin[j] = (uint8_t)org;
  if (a.src) a.src[j] = s;
}
