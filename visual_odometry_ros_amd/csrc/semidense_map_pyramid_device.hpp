// semidense_map_pyramid_device.hpp — the kernel that forms one coarser level of a semi-dense map (include/vo_hip.h, "Semi-dense
// alignment on a map pyramid", has the definition). Included by semidense_align.hip and, through tests/emu/hip_emu.h,
// by the CPU harness (tests/emu/emu_semidense_align_pyr.cpp) that runs this text against the numpy restatement
// (tests/semidense_align_pyr_restatement.py).
//
//   semidense_map_pyramid_kernel   grid ceil(wc hc / SDM_NT), SDM_NT threads; one launch per level, level l + 1 from level l's
//                      planes. One coarse pixel per thread: its up to nine children are read with plain loads (each cell is tested
//                      against the finer plane BEFORE its address is formed), the two float sums run in the definition's order in
//                      registers, three plain stores. No LDS, no atomics: a coarse pixel has one writer.
//
// The includer provides __global__ and the built-in indices.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "semidense_sample.hpp"  // SDT_MUL / SDT_ADD

#define SDM_NT 256
#define SDM_MAX_LEVELS 6

struct SdmArgs {
  const float *invd, *sigma;  // the finer level, w x h planes, tightly packed
  const uint8_t *n_obs;
  int w, h;
  float *o_invd, *o_sigma;  // the coarser level, wc x hc = (w + 1) / 2 x (h + 1) / 2
  uint8_t *o_n_obs;
  int wc, hc;
};

__global__ __launch_bounds__(SDM_NT) void semidense_map_pyramid_kernel(SdmArgs a) {
  const long long i = (long long)blockIdx.x * SDM_NT + (long long)threadIdx.x, nc = (long long)a.wc * (long long)a.hc;
  if (i >= nc) return;
  const int Y = (int)(i / a.wc), X = (int)(i - (long long)Y * a.wc);
  float S = 0.0f, N = 0.0f;
  int n = 0, top = 0;
#pragma unroll
  for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
    for (int dx = -1; dx <= 1; ++dx) {
      const int y = 2 * Y + dy, x = 2 * X + dx;
      if (y < 0 || y >= a.h || x < 0 || x >= a.w) continue;  // (before the address is formed)
      const size_t j = (size_t)y * (size_t)a.w + (size_t)x;
      const int no = (int)a.n_obs[j];
      const float sg = a.sigma[j], iv = a.invd[j];
      if (no >= 1 && sg > 0.0f && iv > 0.0f && sg <= 3.40282347e+38f && iv <= 3.40282347e+38f) {  // (false for NaN)
        const float wt = 1.0f / SDT_MUL(sg, sg);
        S = SDT_ADD(S, wt);
        N = SDT_ADD(N, SDT_MUL(wt, iv));
        ++n;
        top = no > top ? no : top;
      }
    }
  const bool ok = n > 0 && S > 0.0f && S <= 3.40282347e+38f;
  a.o_invd[i] = ok ? N / S : 0.0f;
  a.o_sigma[i] = ok ? sqrtf((float)n / S) : 0.0f;
  a.o_n_obs[i] = (uint8_t)(ok ? top : 0);
}
