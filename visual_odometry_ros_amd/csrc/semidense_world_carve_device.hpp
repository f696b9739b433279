// semidense_world_carve_device.hpp — free-space carving on the world-frame voxel map (include/vo_hip.h, "Semi-dense world map:
// free-space carving", has the definition). Included by semidense_world.hip and, through tests/emu/hip_emu.h, by the CPU
// harness (tests/emu/emu_semidense_world_carve.cpp) that runs this text against the numpy restatement
// (tests/semidense_world_carve_restatement.py). It includes semidense_world_device.hpp, whose slot, arguments and entry test it uses.
//
//   semidense_world_carve_kernel<AGG>   one launch per carve, the integration's geometry: a workgroup of SDW_NT threads owns SDW_BLOCK
//                      raster indices and LISTS the pixels that are entries exactly as the integration does. A listed pixel that is
//                      not skipped is a ray; the rays that have a sample go to a second list with their pixel's (x - cx) / fx and
//                      (y - cy) / fy and their z_end, the others are counted as short; the block's largest k worth forming (a bound at
//                      most one past a ray's last sample) is an LDS maximum. The first sample k0 is the same for every ray of a launch
//                      (z_near and dz are the launch's): the host passes it. No lane owns a ray: the block's (k, ray) pairs, k from k0 to the block's largest bound, the
//                      ray running fastest, are shared out over the 256 lanes. A lane forms z_k, tests z_k < z_end itself, forms
//                      key_k and — unless k is k0 — key_{k-1}, and so decides "visit" with arithmetic alone.
//                      AGG = false, the simple form, the launcher's default: every visit looks its voxel up in the global table (the removal's lookup: the key
//                      words are only read; a probe that meets key 0 ends) and adds 1 to `free` on a match.
//                      AGG = true, the pre-aggregated form: the pairs are walked in rounds of SDWC_ROUND values of k; a round's visits
//                      are combined in an LDS hash of SDW_LH slots (key -> count; a visit that finds no slot within SDW_LPROBE probes
//                      looks itself up), then every occupied LDS slot does ONE global lookup and adds its count on a match.
//                      `free` is an integer and the counters are properties of the definition, so both forms leave the same bytes.
//                      The counters go out as one atomic each per workgroup; workgroup 0 counts the carve. No ticket: nothing of a
//                      carve depends on another workgroup's.
//   semidense_world_extract_free_kernel   the extraction kernel with the free filter: (u64)free * den <= (u64)cnt * num where den >= 1.
//
// The includer provides what semidense_world_device.hpp asks for.
#pragma once
#include "semidense_world_device.hpp"

#define SDWC_MAX_K 4096  // samples per ray: a constant of the definition
#define SDWC_ROUND 4     // values of k per round of the pre-aggregated form
#define SDWC_LDS_BYTES_SIMPLE (SDW_BLOCK * (2 + 4 + 4 + 4) + 7 * 4)
#define SDWC_LDS_BYTES_AGG (SDWC_LDS_BYTES_SIMPLE + 4 + SDW_LH * (8 + 4))  // (+ 4: the 64-bit keys are aligned)

// the carve's words on the device, behind SdwReanchorState
struct SdwCarveState {
  sdw_u64 carves, rays, short_rays, visits, hits;
};

struct SdwCarveArgs {
  SdwArgs a;  // the integration's (Lk null, seq unused)
  float margin, chi, z_near;
  float dz;   // voxel * 0.5f
  int k0;     // the smallest k in 1 .. SDWC_MAX_K with z_near <= (float)k * dz; SDWC_MAX_K + 1: none
  SdwCarveState *cs;
};

// the key of the sample at depth zk on the ray of a pixel with rx = ((float)x - cx) / fx, ry = ((float)y - cy) / fy: sdw_point's text
// with zk in the place of z; 0 where an axis is out of range
__device__ static inline sdw_u64 sdwc_key(const SdwArgs &a, float rx, float ry, float zk) {
  const float X0 = SDW_MUL(rx, zk), X1 = SDW_MUL(ry, zk);
  sdw_u64 key = SDW_KEY_BIT;
  for (int r = 0; r < 3; ++r) {
    const float Xw =
        SDW_ADD(SDW_ADD(SDW_MUL(a.T[4 * r], X0), SDW_ADD(SDW_MUL(a.T[4 * r + 1], X1), SDW_MUL(a.T[4 * r + 2], zk))), a.T[4 * r + 3]);
    const float fl = floorf(Xw / a.voxel);
    if (!(fl >= -SDW_RANGE && fl < SDW_RANGE)) return 0ull;  // (NaN and inf too)
    key |= (sdw_u64)((int)fl + 1048576) << (42 - 21 * r);
  }
  return key;
}

// `n` visits of one voxel: n where the voxel is in the table, 0 where the probe met an empty slot
__device__ static inline unsigned sdwc_lookup(const SdwArgs &a, sdw_u64 key, unsigned n) {
  const size_t mask = ((size_t)1 << a.capacity_log2) - 1;
  size_t h = (size_t)((key * SDW_HASH_MUL) >> (64 - a.capacity_log2));
  for (size_t t = 0; t <= mask; ++t, h = (h + 1) & mask) {
    SdwSlot *s = a.slots + h;
    const sdw_u64 k = *(const volatile sdw_u64 *)&s->key;  // (no launch that writes a key runs next to this one)
    if (k == 0ull) return 0u;
    if (k != key) continue;
    atomicAdd(&s->free, n);
    return n;
  }
  return 0u;
}

template <bool AGG>
__global__ __launch_bounds__(SDW_NT) void semidense_world_carve_kernel(SdwCarveArgs ca) {
  __shared__ uint16_t s_list[SDW_BLOCK];  // the block's raster offsets that are entries
  __shared__ float s_rx[SDW_BLOCK], s_ry[SDW_BLOCK], s_zend[SDW_BLOCK];  // the rays that have a sample, in arrival order
  __shared__ int s_n, s_nray, s_kmax;
  __shared__ unsigned s_cnt[4];  // rays, short rays, visits, hits
  __shared__ sdw_u64 s_key[AGG ? SDW_LH : 1];
  __shared__ unsigned s_c[AGG ? SDW_LH : 1];
  const SdwArgs &a = ca.a;
  const int tid = (int)threadIdx.x;
  const size_t np = (size_t)a.W * (size_t)a.H;
  if (tid == 0) s_n = 0, s_nray = 0, s_kmax = 0;
  if (tid < 4) s_cnt[tid] = 0;
  __syncthreads();
  const size_t base = (size_t)blockIdx.x * SDW_BLOCK;
  for (int k = tid; k < SDW_BLOCK; k += SDW_NT) {
    const size_t i = base + (size_t)k;
    if (i >= np) break;
    const int no = (int)a.n_obs[i];
    const float iv = a.invd[i], sg = a.sigma[i];
    if (no >= 1 && sg > 0.0f && sg <= SDW_FLT_MAX && iv > 0.0f && iv <= SDW_FLT_MAX) s_list[atomicAdd(&s_n, 1)] = (uint16_t)k;
  }
  __syncthreads();
  const int n_list = s_n;
  unsigned n_rays = 0, n_short = 0, n_visit = 0, n_hit = 0;
  for (int k = tid; k < n_list; k += SDW_NT) {
    const size_t i = base + (size_t)s_list[k];
    const float z = 1.0f / a.invd[i], sg = a.sigma[i];
    if ((int)a.n_obs[i] < a.min_obs || !(z <= a.z_max)) continue;  // SKIPPED: no ray
    ++n_rays;
    const float sz = SDW_MUL(SDW_MUL(sg, z), z);
    const float m = fmaxf(SDW_MUL(ca.margin, a.voxel), SDW_MUL(ca.chi, sz));
    const float z_end = SDW_SUB(z, m);
    if (!(ca.k0 <= SDWC_MAX_K && SDW_MUL((float)ca.k0, ca.dz) < z_end)) {  // (z_k does not fall with k: no later k is a sample either)
      ++n_short;
      continue;
    }
    // z_end / dz is within a few ulp of the last sample's k: one more covers it; every lane tests z_k < z_end itself
    const float e = fminf(z_end / ca.dz, (float)SDWC_MAX_K);
    int kend = (int)e + 1;
    if (kend > SDWC_MAX_K) kend = SDWC_MAX_K;
    const int y = (int)(i / (size_t)a.W), x = (int)(i - (size_t)y * (size_t)a.W);
    const int r = atomicAdd(&s_nray, 1);
    s_zend[r] = z_end;
    s_rx[r] = SDW_SUB((float)x, a.cx) / a.fx;
    s_ry[r] = SDW_SUB((float)y, a.cy) / a.fy;
    atomicMax(&s_kmax, kend);
  }
  __syncthreads();
  const int n_ray = s_nray, k0 = ca.k0, kmax = s_kmax;
  if (n_ray > 0) {
    const int nk_all = kmax - k0 + 1;  // (>= 1: a listed ray has k0 as a sample)
    const int per = AGG ? SDWC_ROUND : nk_all;
    for (int kb = 0; kb < nk_all; kb += per) {
      const int nk = nk_all - kb < per ? nk_all - kb : per;
      if (AGG) {
        for (int j = tid; j < SDW_LH; j += SDW_NT) s_key[j] = 0ull, s_c[j] = 0u;
        __syncthreads();
      }
      const int n_pair = nk * n_ray;  // (at most 4096 * 1024)
      for (int f = tid; f < n_pair; f += SDW_NT) {
        const int kk = f / n_ray, r = f - kk * n_ray, k = k0 + kb + kk;
        const float zk = SDW_MUL((float)k, ca.dz);
        if (!(zk < s_zend[r])) continue;  // behind the ray's last sample
        const float rx = s_rx[r], ry = s_ry[r];
        const sdw_u64 key = sdwc_key(a, rx, ry, zk);
        if (key == 0ull) continue;
        if (k != k0 && sdwc_key(a, rx, ry, SDW_MUL((float)(k - 1), ca.dz)) == key) continue;
        ++n_visit;
        bool done = false;
        if (AGG) {
          unsigned h = (unsigned)((key * SDW_HASH_MUL) >> 40) & (SDW_LH - 1);
          for (int t = 0; t < SDW_LPROBE && !done; ++t, h = (h + 1) & (SDW_LH - 1)) {
            const sdw_u64 old = sdw_cas64(&s_key[h], 0ull, key);
            if (old != 0ull && old != key) continue;
            atomicAdd(&s_c[h], 1u);
            done = true;
          }
        }
        if (!done) n_hit += sdwc_lookup(a, key, 1u);
      }
      if (AGG) {
        __syncthreads();
        for (int j = tid; j < SDW_LH; j += SDW_NT)
          if (s_key[j] != 0ull) n_hit += sdwc_lookup(a, s_key[j], s_c[j]);
        __syncthreads();
      }
    }
  }
  if (n_rays) atomicAdd(&s_cnt[0], n_rays);
  if (n_short) atomicAdd(&s_cnt[1], n_short);
  if (n_visit) atomicAdd(&s_cnt[2], n_visit);
  if (n_hit) atomicAdd(&s_cnt[3], n_hit);
  __syncthreads();
  if (tid == 0) {
    if (blockIdx.x == 0) atomicAdd(&ca.cs->carves, (sdw_u64)1);
    if (s_cnt[0]) atomicAdd(&ca.cs->rays, (sdw_u64)s_cnt[0]);
    if (s_cnt[1]) atomicAdd(&ca.cs->short_rays, (sdw_u64)s_cnt[1]);
    if (s_cnt[2]) atomicAdd(&ca.cs->visits, (sdw_u64)s_cnt[2]);
    if (s_cnt[3]) atomicAdd(&ca.cs->hits, (sdw_u64)s_cnt[3]);
  }
}

struct SdwExtractFreeArgs {
  SdwExtractArgs e;
  unsigned free_num, free_den;  // den 0: no filter
};

__global__ __launch_bounds__(SDW_NT) void semidense_world_extract_free_kernel(SdwExtractFreeArgs fa) {
  __shared__ unsigned s_n, s_base;
  const SdwExtractArgs &a = fa.e;
  const int tid = (int)threadIdx.x;
  if (tid == 0) s_n = 0;
  __syncthreads();
  const size_t i = (size_t)blockIdx.x * SDW_NT + (size_t)tid;
  bool take = i < a.n_slots && a.slots[i].key != 0ull && a.slots[i].cnt >= a.min_count && a.slots[i].kf_cnt >= a.min_keyframes;
  if (take && fa.free_den != 0u) take = (sdw_u64)a.slots[i].free * fa.free_den <= (sdw_u64)a.slots[i].cnt * fa.free_num;
  unsigned r = 0;
  if (take) r = atomicAdd(&s_n, 1u);
  __syncthreads();
  if (tid == 0 && s_n) s_base = atomicAdd(&a.st->n_extract, s_n);
  __syncthreads();
  if (take && (size_t)s_base + r < (size_t)a.cap) a.out[s_base + r] = a.slots[i];
}
