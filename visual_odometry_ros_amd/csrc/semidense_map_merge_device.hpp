// semidense_map_merge_device.hpp — the kernel that merges a keyframe's semi-dense map with a disparity result of the same keyframe
// (include/vo_hip.h, "Semi-dense map merge", has the definition). Read by csrc/semidense_map_merge.hip for gfx950 and by
// tests/emu/emu_semidense_map_merge.cpp on CPU threads, against tests/semidense_map_merge_restatement.py.
//
//   semidense_map_merge_kernel   one launch, SDM_NT lanes a workgroup, SDM_PIX consecutive pixels a lane. A lane reads its pixels of
//                      the six input planes, decides, and writes its pixels of the four output planes: no lane reads what another
//                      writes, so an output plane may be the input plane of the same kind. With `vec` (every plane's address a
//                      multiple of 16 bytes for f32, of 4 for u8 — the launcher looks at the pointers) a lane whose four pixels all
//                      exist moves them as one 16-byte word per f32 plane and one 4-byte word per u8 plane; every other lane, and
//                      every lane without `vec`, moves them one by one. Both ways run the same sdm_pixel on the same values. No
//                      address is formed at or beyond n. The counts per origin: a lane packs its (at most four) pixels into two
//                      words of three 10-bit fields, SDM_WAVE_SUM adds the words over the wavefront (at most 256 a field), the
//                      wavefronts' words meet in LDS, and lanes 0..5 of the workgroup add one non-zero field each to the 64-bit
//                      words the launch's predecessor has zeroed. Integer sums only.
//
// The includer provides __global__, __shared__, __syncthreads, the built-in indices, atomicAdd on unsigned long long and
//   SDM_WAVE_SUM(v)   the sum of the unsigned v over the 64 lanes of the caller's wavefront (every lane calls it)
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "semidense_map_fuse.hpp"  // sdm_seed_entry, sdm_fuse

#define SDM_NT 256
#define SDM_PIX 4
#define SDM_ORIGINS 6  // 0 nothing, 1 the map's, 2 the result's, 3 fused, 4 inconsistent: the map kept, 5 inconsistent: dropped

struct SdmArgs {
  const float *invd_m, *sigma_m;  // the map, n pixels; all three null: no map
  const uint8_t *n_obs_m;
  const float *disp, *sigma_invd;  // the disparity result
  const uint8_t *status;
  float bf, chi2;  // chi2 = chi chi
  int keep_obs;    // 0..256
  float *invd, *sigma;  // the merged map
  uint8_t *n_obs;
  uint8_t *origin;             // may be null
  unsigned long long *counts;  // SDM_ORIGINS words, zeroed in front of the launch; may be null
  int n;                       // W H
  int vec;
};

// the launcher's rule for `vec`: every f32 plane on a 16-byte boundary, every u8 plane on a 4-byte one (a null pointer counts as aligned)
static inline int sdm_planes_aligned(const SdmArgs &a) {
  const uintptr_t f32s = (uintptr_t)a.invd_m | (uintptr_t)a.sigma_m | (uintptr_t)a.disp | (uintptr_t)a.sigma_invd | (uintptr_t)a.invd | (uintptr_t)a.sigma;
  const uintptr_t u8s = (uintptr_t)a.n_obs_m | (uintptr_t)a.status | (uintptr_t)a.n_obs | (uintptr_t)a.origin;
  return (f32s & 15) == 0 && (u8s & 3) == 0;
}
static inline unsigned sdm_grid(int n) { return (unsigned)(((long long)n + SDM_NT * SDM_PIX - 1) / (SDM_NT * SDM_PIX)); }

struct alignas(16) SdmF4 {
  float v[SDM_PIX];
};

// one pixel; returns the origin
__device__ static inline int sdm_pixel(bool has_map, float m_invd, float m_sigma, int m_no, float disp, float sigma_invd, int status, float bf,
                                       float chi2, int keep_obs, float *o_invd, float *o_sigma, int *o_no) {
  float rho, sig;
  int no_d;
  sdm_seed_entry(status, disp, sigma_invd, bf, &rho, &sig, &no_d);
  const bool m = has_map && m_no >= 1, s = no_d >= 1;
  *o_invd = 0.0f, *o_sigma = 0.0f, *o_no = 0;
  if (m && s) {
    if (sdm_fuse(m_invd, m_sigma, rho, sig, chi2, o_invd, o_sigma)) {
      *o_no = m_no < 255 ? m_no + 1 : 255;
      return 3;
    }
    if (m_no >= keep_obs) {
      *o_invd = m_invd, *o_sigma = m_sigma, *o_no = m_no;
      return 4;
    }
    return 5;
  }
  if (m) {
    *o_invd = m_invd, *o_sigma = m_sigma, *o_no = m_no;
    return 1;
  }
  if (s) {
    *o_invd = rho, *o_sigma = sig, *o_no = no_d;
    return 2;
  }
  return 0;
}

__global__ __launch_bounds__(SDM_NT) void semidense_map_merge_kernel(SdmArgs a) {
  __shared__ unsigned wcnt[SDM_NT / 64][2];
  const int t = (int)threadIdx.x;
  const long long i0 = ((long long)blockIdx.x * SDM_NT + t) * SDM_PIX;  // (n <= 2^31 - 1: the last workgroup's lanes pass it)
  const int left = i0 >= (long long)a.n ? 0 : ((long long)a.n - i0 < SDM_PIX ? (int)((long long)a.n - i0) : SDM_PIX);
  const bool has_map = a.invd_m != nullptr, wide = a.vec && left == SDM_PIX;
  float m_invd[SDM_PIX], m_sigma[SDM_PIX], disp[SDM_PIX], sg[SDM_PIX];
  int m_no[SDM_PIX], st[SDM_PIX];
#pragma unroll
  for (int k = 0; k < SDM_PIX; ++k) m_invd[k] = m_sigma[k] = disp[k] = sg[k] = 0.0f, m_no[k] = st[k] = 0;
  // ---- every load of the lane's pixels, before any store
  if (wide) {
    const SdmF4 d4 = *(const SdmF4 *)(a.disp + i0), s4 = *(const SdmF4 *)(a.sigma_invd + i0);
    const uint32_t st4 = *(const uint32_t *)(a.status + i0);
#pragma unroll
    for (int k = 0; k < SDM_PIX; ++k) disp[k] = d4.v[k], sg[k] = s4.v[k], st[k] = (int)((st4 >> (8 * k)) & 0xFFu);
    if (has_map) {
      const SdmF4 i4 = *(const SdmF4 *)(a.invd_m + i0), g4 = *(const SdmF4 *)(a.sigma_m + i0);
      const uint32_t n4 = *(const uint32_t *)(a.n_obs_m + i0);
#pragma unroll
      for (int k = 0; k < SDM_PIX; ++k) m_invd[k] = i4.v[k], m_sigma[k] = g4.v[k], m_no[k] = (int)((n4 >> (8 * k)) & 0xFFu);
    }
  } else {
#pragma unroll
    for (int k = 0; k < SDM_PIX; ++k) {
      if (k >= left) continue;
      disp[k] = a.disp[i0 + k], sg[k] = a.sigma_invd[i0 + k], st[k] = (int)a.status[i0 + k];
      if (has_map) m_invd[k] = a.invd_m[i0 + k], m_sigma[k] = a.sigma_m[i0 + k], m_no[k] = (int)a.n_obs_m[i0 + k];
    }
  }
  // ---- the decision
  SdmF4 o_invd, o_sigma;
  int o_no[SDM_PIX], org[SDM_PIX];
  unsigned c0 = 0, c1 = 0;  // fields of 10 bits: origins 0, 1, 2 | 3, 4, 5
#pragma unroll
  for (int k = 0; k < SDM_PIX; ++k) {
    org[k] = sdm_pixel(has_map, m_invd[k], m_sigma[k], m_no[k], disp[k], sg[k], st[k], a.bf, a.chi2, a.keep_obs, &o_invd.v[k], &o_sigma.v[k], &o_no[k]);
    if (k < left) {
      if (org[k] < 3) c0 += 1u << (10 * org[k]);
      else c1 += 1u << (10 * (org[k] - 3));
    }
  }
  // ---- the stores
  if (wide) {
    *(SdmF4 *)(a.invd + i0) = o_invd;
    *(SdmF4 *)(a.sigma + i0) = o_sigma;
    *(uint32_t *)(a.n_obs + i0) = (uint32_t)o_no[0] | ((uint32_t)o_no[1] << 8) | ((uint32_t)o_no[2] << 16) | ((uint32_t)o_no[3] << 24);
    if (a.origin) *(uint32_t *)(a.origin + i0) = (uint32_t)org[0] | ((uint32_t)org[1] << 8) | ((uint32_t)org[2] << 16) | ((uint32_t)org[3] << 24);
  } else {
#pragma unroll
    for (int k = 0; k < SDM_PIX; ++k) {
      if (k >= left) continue;
      a.invd[i0 + k] = o_invd.v[k];
      a.sigma[i0 + k] = o_sigma.v[k];
      a.n_obs[i0 + k] = (uint8_t)o_no[k];
      if (a.origin) a.origin[i0 + k] = (uint8_t)org[k];
    }
  }
  // ---- the counts (a.counts is the same for every lane: all of them take the barrier or none does)
  if (!a.counts) return;
  c0 = SDM_WAVE_SUM(c0);
  c1 = SDM_WAVE_SUM(c1);
  if ((t & 63) == 0) wcnt[t >> 6][0] = c0, wcnt[t >> 6][1] = c1;
  __syncthreads();
  if (t < SDM_ORIGINS) {
    unsigned sum = 0;
#pragma unroll
    for (int w = 0; w < SDM_NT / 64; ++w) sum += (wcnt[w][t / 3] >> (10 * (t % 3))) & 0x3FFu;
    if (sum) atomicAdd(a.counts + t, (unsigned long long)sum);
  }
}
