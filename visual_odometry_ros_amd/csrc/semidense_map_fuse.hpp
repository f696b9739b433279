// semidense_map_fuse.hpp — the two pieces of per-pixel arithmetic that more than one semi-dense kernel performs, each written once:
// the map entry a static (or dense) result gives (vo_semidense_map_seed; include/vo_hip.h, "Semi-dense temporal") and the consistency
// test with the Gaussian fusion of two inverse depths (include/vo_hip.h, "Semi-dense propagation": the resolve's `fused` case).
// Included by semidense_temporal_device.hpp (the seed), semidense_propagate_device.hpp (the resolve) and
// semidense_map_merge_device.hpp (the merge), and through them by the CPU harnesses under tests/emu. float32, every operation rounded
// on its own; the includer provides nothing.
#pragma once

#if defined(__HIP_DEVICE_COMPILE__)
#define SDM_MUL(a, b) __fmul_rn((a), (b))
#define SDM_ADD(a, b) __fadd_rn((a), (b))
#define SDM_SUB(a, b) __fsub_rn((a), (b))
#else  // host text (the emulation harnesses): compiled with -ffp-contract=off
#define SDM_MUL(a, b) ((a) * (b))
#define SDM_ADD(a, b) ((a) + (b))
#define SDM_SUB(a, b) ((a) - (b))
#endif

// what vo_semidense_map_seed writes for a pixel: (disparity / bf, sigma_invd, 1) where status == 1, else (0, 0, 0)
__device__ static inline void sdm_seed_entry(int status, float disparity, float sigma_invd, float bf, float *invd, float *sigma, int *n_obs) {
  const bool ok = status == 1;
  *invd = ok ? disparity / bf : 0.0f;
  *sigma = ok ? sigma_invd : 0.0f;
  *n_obs = ok ? 1 : 0;
}

// (invd, sigma) carried by a map against a new measurement (rho, sig): true where the two agree within chi — then *o_invd, *o_sigma are
// their fusion —, false otherwise (a NaN anywhere fails) with the outputs untouched. chi2 = chi chi.
__device__ static inline bool sdm_fuse(float invd, float sigma, float rho, float sig, float chi2, float *o_invd, float *o_sigma) {
  const float dd = SDM_SUB(invd, rho);
  const float s2 = SDM_MUL(sigma, sigma), m2 = SDM_MUL(sig, sig), sum = SDM_ADD(s2, m2);
  if (!(sum > 0.0f && SDM_MUL(dd, dd) <= SDM_MUL(chi2, sum))) return false;
  *o_invd = SDM_ADD(SDM_MUL(invd, m2), SDM_MUL(rho, s2)) / sum;
  *o_sigma = sqrtf(SDM_MUL(s2, m2) / sum);
  return true;
}
