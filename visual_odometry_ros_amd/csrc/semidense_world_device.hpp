// semidense_world_device.hpp — the kernels of the world-frame voxel map that fuses the keyframes' semi-dense maps (include/vo_hip.h,
// "Semi-dense world map", has the definition). Included by semidense_world.hip and, through tests/emu/hip_emu.h, by
// the CPU harness (tests/emu/emu_semidense_world.cpp) that runs this text against the numpy restatement
// (tests/semidense_world_restatement.py).
//
//   semidense_world_integrate_kernel<AGG>   one launch per integration. A workgroup of SDW_NT threads owns SDW_BLOCK raster indices.
//                      Every workgroup first reads the committed `occupied` count, which no workgroup of this launch writes before all
//                      of them have taken their ticket, and leaves at once where the integration is refused: the decision is the same
//                      in every workgroup. The lanes LIST the pixels that are entries (one LDS atomicAdd on a counter each, as the
//                      regularisation kernel does: a map is sparse), then share the list out, so that a wavefront's atomics leave
//                      together. A listed pixel becomes a point (key, wq, three sub-voxel offsets, grey) or is counted as skipped /
//                      out of range.
//                      AGG = false, the simple form: every point probes the global table itself (one 64-bit compare-and-swap per
//                      probed slot) and adds its five 64-bit sums, its count and its keyframe mark with global atomics.
//                      AGG = true, the pre-aggregated form: the points are first combined in an LDS hash of SDW_LH slots (a 64-bit LDS
//                      compare-and-swap claims a slot, 64-bit LDS adds sum); a point that finds no slot within SDW_LPROBE probes goes
//                      to the global table directly. Behind a barrier every occupied LDS slot does ONE global update. All sums are
//                      integers, so both forms leave the same table contents whatever the arrival order; only which SLOT a voxel sits
//                      in depends on it.
//                      The counters go out as one atomic per workgroup. Then the ticket (the alignment kernel's shape): every
//                      wavefront drains, a barrier, thread 0 releases at agent scope and takes the ticket; the last workgroup acquires,
//                      adds the launch's claimed slots to `occupied`, counts the integration and zeroes the launch's words.
//   semidense_world_extract_kernel   one thread per slot; the slots that pass min_count / min_keyframes are appended to `out` (one LDS
//                      rank per thread, one global atomicAdd per workgroup) in whatever order they come: the host sorts by key. The
//                      count runs on past `cap`; nothing is written there.
//   semidense_world_remove_kernel   one launch per removal (include/vo_hip.h, "Semi-dense world map: removal and re-anchoring"; DESIGN.md
//                      §25), the integration's geometry and its pre-aggregated shape: the same refusal test on the same word, the same
//                      list, the same points (sdw_point), combined in the same LDS hash; then every occupied LDS slot, and every point
//                      that found none, LOOKS its voxel UP — the key words are only read, never compare-and-swapped — and adds the two's
//                      complement of its sums. A probe that meets an empty slot ends: the points are counted as missing. `occupied` and
//                      `claimed` are not written. The ticket's last workgroup counts the removal and zeroes the ticket; the words are a
//                      block of their own (SdwReanchorState), so that SdwState keeps its layout.
//   semidense_world_vacant_kernel   one thread per slot; counts the slots with a key and cnt == 0 (one global atomicAdd per workgroup).
//
// The includer provides __global__, __shared__, __syncthreads, the built-in indices, atomicAdd / atomicMax on 32- and 64-bit words in
// global memory and LDS, sdw_cas64(p, compare, value) (returns the old word; global and LDS) and the agent-scope spellings SDW_DRAIN,
// SDW_ST_AGENT, SDW_ATOMIC_ADD_AGENT, SDW_FENCE_RELEASE, SDW_FENCE_ACQUIRE (each with its own wait).
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#if defined(__HIP_DEVICE_COMPILE__)
#define SDW_MUL(a, b) __fmul_rn((a), (b))
#define SDW_ADD(a, b) __fadd_rn((a), (b))
#define SDW_SUB(a, b) __fsub_rn((a), (b))
#else  // host text (the emulation harness): compiled with -ffp-contract=off
#define SDW_MUL(a, b) ((a) * (b))
#define SDW_ADD(a, b) ((a) + (b))
#define SDW_SUB(a, b) ((a) - (b))
#endif

#define SDW_NT 256
#define SDW_BLOCK 1024  // raster indices per workgroup
#define SDW_LH 512      // slots of the workgroup's LDS hash (a power of two)
#define SDW_LPROBE 8    // LDS probes before a point goes to the global table itself
#define SDW_LDS_BYTES_SIMPLE (SDW_BLOCK * 2 + 6 * 4)
#define SDW_LDS_BYTES_AGG (SDW_BLOCK * 2 + 6 * 4 + SDW_LH * (6 * 8 + 4))
#define SDW_LDS_BYTES_REMOVE (SDW_BLOCK * 2 + 4 * 4 + SDW_LH * (6 * 8 + 4))
#define SDW_FLT_MAX 3.4028235e38f
#define SDW_RANGE 1048576.0f                 // 2^20 voxels either way per axis
#define SDW_HASH_MUL 0x9E3779B97F4A7C15ull   // home slot = (key * this) >> (64 - capacity_log2)
#define SDW_KEY_BIT 0x8000000000000000ull

typedef unsigned long long sdw_u64;

// one slot of the table: 64 bytes. key == 0: empty.
struct SdwSlot {
  sdw_u64 key;
  sdw_u64 sw, sx, sy, sz, sg;
  unsigned cnt, kf_cnt, last_seq, free;  // free: the carve's count (semidense_world_carve_device.hpp); no other kernel writes it
};

// the table's words on the device
struct SdwState {
  unsigned occupied;      // committed by the last accepted integration's last workgroup
  unsigned claimed;       // slots claimed by the launch in flight (0 between launches)
  unsigned ticket;        // (0 between launches)
  unsigned integrations, refused;
  unsigned n_extract;     // the extraction's count
  sdw_u64 inserted, skipped, out_of_range;
};

struct SdwArgs {
  const float *invd, *sigma;  // the map, W x H planes, tightly packed
  const uint8_t *n_obs;
  const uint8_t *Lk;          // level-0 pixel (0, 0) of the keyframe's left image, null: none
  int strideK;                // bytes per row
  int W, H;
  int min_obs;
  float z_max, voxel;
  float fx, fy, cx, cy;
  float T[12];                // X' = T X, the rows of T_wk
  unsigned seq;
  int capacity_log2;
  SdwSlot *slots;
  SdwState *st;
};

struct SdwPoint {
  sdw_u64 key;
  unsigned wq, q[3], grey;
};

// the pixel at raster index i: 0 no entry, 1 a point, 2 skipped, 3 out of range
__device__ static inline int sdw_point(const SdwArgs &a, int i, SdwPoint *p) {
  const int no = (int)a.n_obs[i];
  const float iv = a.invd[i], sg = a.sigma[i];
  if (!(no >= 1 && sg > 0.0f && sg <= SDW_FLT_MAX && iv > 0.0f && iv <= SDW_FLT_MAX)) return 0;
  const float z = 1.0f / iv;
  if (no < a.min_obs || !(z <= a.z_max)) return 2;
  const int y = i / a.W, x = i - y * a.W;
  const float X0 = SDW_MUL(SDW_SUB((float)x, a.cx) / a.fx, z), X1 = SDW_MUL(SDW_SUB((float)y, a.cy) / a.fy, z);
  sdw_u64 key = SDW_KEY_BIT;
  for (int r = 0; r < 3; ++r) {
    const float Xw =
        SDW_ADD(SDW_ADD(SDW_MUL(a.T[4 * r], X0), SDW_ADD(SDW_MUL(a.T[4 * r + 1], X1), SDW_MUL(a.T[4 * r + 2], z))), a.T[4 * r + 3]);
    const float u = Xw / a.voxel, fl = floorf(u);
    if (!(fl >= -SDW_RANGE && fl < SDW_RANGE)) return 3;  // (NaN and inf too)
    const int q = (int)SDW_MUL(SDW_SUB(u, fl), 1024.0f);  // u - fl rounds to 1.0f for a u just below an integer: the clamp
    p->q[r] = (unsigned)(q > 1023 ? 1023 : q);
    key |= (sdw_u64)((int)fl + 1048576) << (42 - 21 * r);
  }
  const float s = SDW_MUL(SDW_MUL(sg, z), z), rr = a.voxel / s, w = SDW_MUL(rr, rr);
  p->wq = w >= 65535.0f ? 65536u : (unsigned)w + 1u;
  p->key = key;
  p->grey = a.Lk ? (unsigned)a.Lk[(size_t)y * (size_t)a.strideK + (size_t)x] : 0u;
  return 1;
}

// sums of one voxel into the global table; returns 1 where it claimed an empty slot. An accepted integration finds a slot: at most
// half of the table is taken when its last point arrives.
__device__ static inline unsigned sdw_commit(const SdwArgs &a, sdw_u64 key, sdw_u64 sw, sdw_u64 sx, sdw_u64 sy, sdw_u64 sz, sdw_u64 sg,
                                             unsigned cnt) {
  const size_t mask = ((size_t)1 << a.capacity_log2) - 1;
  size_t h = (size_t)((key * SDW_HASH_MUL) >> (64 - a.capacity_log2));
  for (size_t n = 0; n <= mask; ++n, h = (h + 1) & mask) {
    SdwSlot *s = a.slots + h;
    const sdw_u64 old = sdw_cas64(&s->key, 0ull, key);
    if (old != 0ull && old != key) continue;
    atomicAdd(&s->sw, sw);
    atomicAdd(&s->sx, sx);
    atomicAdd(&s->sy, sy);
    atomicAdd(&s->sz, sz);
    if (sg) atomicAdd(&s->sg, sg);
    atomicAdd(&s->cnt, cnt);
    if (atomicMax(&s->last_seq, a.seq) < a.seq) atomicAdd(&s->kf_cnt, 1u);
    return old == 0ull ? 1u : 0u;
  }
  return 0u;  // (not reached)
}

template <bool AGG>
__global__ __launch_bounds__(SDW_NT) void semidense_world_integrate_kernel(SdwArgs a) {
  __shared__ uint16_t s_list[SDW_BLOCK];  // the block's raster offsets that are entries
  __shared__ int s_n;
  __shared__ unsigned s_cnt[4];  // inserted, skipped, out of range, claimed
  __shared__ int s_last;
  __shared__ sdw_u64 s_key[AGG ? SDW_LH : 1], s_sum[AGG ? SDW_LH * 5 : 1];
  __shared__ unsigned s_c[AGG ? SDW_LH : 1];
  const int tid = (int)threadIdx.x;
  const size_t np = (size_t)a.W * (size_t)a.H;
  // all or nothing: the same word in every workgroup of the launch
  if ((sdw_u64)a.st->occupied + (sdw_u64)np > (((sdw_u64)1 << a.capacity_log2) >> 1)) {
    if (blockIdx.x == 0 && tid == 0) atomicAdd(&a.st->refused, 1u);
    return;
  }
  if (tid == 0) s_n = 0;
  if (tid < 4) s_cnt[tid] = 0;
  if (AGG)
    for (int k = tid; k < SDW_LH; k += SDW_NT) {
      s_key[k] = 0ull;
      s_c[k] = 0;
      for (int j = 0; j < 5; ++j) s_sum[5 * k + j] = 0ull;
    }
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
  unsigned n_ins = 0, n_skip = 0, n_oor = 0, n_claim = 0;
  for (int k = tid; k < n_list; k += SDW_NT) {
    SdwPoint p;
    const int kind = sdw_point(a, (int)(base + (size_t)s_list[k]), &p);
    if (kind == 2) ++n_skip;
    if (kind == 3) ++n_oor;
    if (kind != 1) continue;
    ++n_ins;
    const sdw_u64 wq = p.wq;
    bool done = false;
    if (AGG) {
      unsigned h = (unsigned)((p.key * SDW_HASH_MUL) >> 40) & (SDW_LH - 1);
      for (int t = 0; t < SDW_LPROBE && !done; ++t, h = (h + 1) & (SDW_LH - 1)) {
        const sdw_u64 old = sdw_cas64(&s_key[h], 0ull, p.key);
        if (old != 0ull && old != p.key) continue;
        atomicAdd(&s_sum[5 * h], wq);
        atomicAdd(&s_sum[5 * h + 1], wq * p.q[0]);
        atomicAdd(&s_sum[5 * h + 2], wq * p.q[1]);
        atomicAdd(&s_sum[5 * h + 3], wq * p.q[2]);
        atomicAdd(&s_sum[5 * h + 4], wq * p.grey);
        atomicAdd(&s_c[h], 1u);
        done = true;
      }
    }
    if (!done) n_claim += sdw_commit(a, p.key, wq, wq * p.q[0], wq * p.q[1], wq * p.q[2], wq * p.grey, 1u);
  }
  if (AGG) {
    __syncthreads();
    for (int k = tid; k < SDW_LH; k += SDW_NT)
      if (s_key[k] != 0ull)
        n_claim += sdw_commit(a, s_key[k], s_sum[5 * k], s_sum[5 * k + 1], s_sum[5 * k + 2], s_sum[5 * k + 3], s_sum[5 * k + 4], s_c[k]);
  }
  if (n_ins) atomicAdd(&s_cnt[0], n_ins);
  if (n_skip) atomicAdd(&s_cnt[1], n_skip);
  if (n_oor) atomicAdd(&s_cnt[2], n_oor);
  if (n_claim) atomicAdd(&s_cnt[3], n_claim);
  // ---- the ticket: the last workgroup publishes the new `occupied` -----------------------------------------------------------------
  SDW_DRAIN();      // every wavefront: its atomics have left ...
  __syncthreads();  // ... before thread 0 adds the workgroup's counts and takes its ticket
  if (tid == 0) {
    if (s_cnt[0]) atomicAdd(&a.st->inserted, (sdw_u64)s_cnt[0]);
    if (s_cnt[1]) atomicAdd(&a.st->skipped, (sdw_u64)s_cnt[1]);
    if (s_cnt[2]) atomicAdd(&a.st->out_of_range, (sdw_u64)s_cnt[2]);
    if (s_cnt[3]) SDW_ATOMIC_ADD_AGENT(&a.st->claimed, s_cnt[3]);
    SDW_FENCE_RELEASE();
    s_last = (SDW_ATOMIC_ADD_AGENT(&a.st->ticket, 1u) == gridDim.x - 1u) ? 1 : 0;
    if (s_last) {
      SDW_FENCE_ACQUIRE();
      const unsigned claimed = SDW_ATOMIC_ADD_AGENT(&a.st->claimed, 0u);  // (at the point of coherence: every workgroup's add is in it)
      a.st->occupied = a.st->occupied + claimed;
      a.st->integrations = a.st->integrations + 1u;
      SDW_ST_AGENT(&a.st->claimed, 0u);
      SDW_ST_AGENT(&a.st->ticket, 0u);
    }
  }
}

struct SdwExtractArgs {
  const SdwSlot *slots;
  size_t n_slots;
  unsigned min_count, min_keyframes;
  SdwSlot *out;  // `cap` records; may be null with cap 0
  unsigned cap;
  SdwState *st;  // n_extract: zeroed in front of the launch
};

__global__ __launch_bounds__(SDW_NT) void semidense_world_extract_kernel(SdwExtractArgs a) {
  __shared__ unsigned s_n, s_base;
  const int tid = (int)threadIdx.x;
  if (tid == 0) s_n = 0;
  __syncthreads();
  const size_t i = (size_t)blockIdx.x * SDW_NT + (size_t)tid;
  const bool take = i < a.n_slots && a.slots[i].key != 0ull && a.slots[i].cnt >= a.min_count && a.slots[i].kf_cnt >= a.min_keyframes;
  unsigned r = 0;
  if (take) r = atomicAdd(&s_n, 1u);
  __syncthreads();
  if (tid == 0 && s_n) s_base = atomicAdd(&a.st->n_extract, s_n);
  __syncthreads();
  if (take && (size_t)s_base + r < (size_t)a.cap) a.out[s_base + r] = a.slots[i];
}

// ---- removal ------------------------------------------------------------------------------------------------------------
// the removal's words on the device, behind SdwState
struct SdwReanchorState {
  unsigned ticket;  // (0 between launches)
  unsigned removals, refused_removals;
  unsigned vacant;  // the count launch's result: zeroed in front of it
  sdw_u64 removed, missing;
};

struct SdwRemoveArgs {
  SdwArgs a;  // the integration's, with the removal's own seq
  SdwReanchorState *rs;
};

// sums of one voxel out of the global table; returns cnt where the voxel was found, 0 where the probe met an empty slot
__device__ static inline unsigned sdw_uncommit(const SdwArgs &a, sdw_u64 key, sdw_u64 sw, sdw_u64 sx, sdw_u64 sy, sdw_u64 sz, sdw_u64 sg,
                                               unsigned cnt) {
  const size_t mask = ((size_t)1 << a.capacity_log2) - 1;
  size_t h = (size_t)((key * SDW_HASH_MUL) >> (64 - a.capacity_log2));
  for (size_t n = 0; n <= mask; ++n, h = (h + 1) & mask) {
    SdwSlot *s = a.slots + h;
    const sdw_u64 k = *(const volatile sdw_u64 *)&s->key;  // (no launch that writes a key runs next to this one)
    if (k == 0ull) return 0u;
    if (k != key) continue;
    atomicAdd(&s->sw, 0ull - sw);
    atomicAdd(&s->sx, 0ull - sx);
    atomicAdd(&s->sy, 0ull - sy);
    atomicAdd(&s->sz, 0ull - sz);
    if (sg) atomicAdd(&s->sg, 0ull - sg);
    atomicAdd(&s->cnt, 0u - cnt);
    if (atomicMax(&s->last_seq, a.seq) < a.seq) atomicAdd(&s->kf_cnt, 0u - 1u);
    return cnt;
  }
  return 0u;
}

__global__ __launch_bounds__(SDW_NT) void semidense_world_remove_kernel(SdwRemoveArgs ra) {
  __shared__ uint16_t s_list[SDW_BLOCK];  // the block's raster offsets that are entries
  __shared__ int s_n;
  __shared__ unsigned s_cnt[2];  // removed, missing
  __shared__ int s_last;
  __shared__ sdw_u64 s_key[SDW_LH], s_sum[SDW_LH * 5];
  __shared__ unsigned s_c[SDW_LH];
  const SdwArgs &a = ra.a;
  const int tid = (int)threadIdx.x;
  const size_t np = (size_t)a.W * (size_t)a.H;
  // all or nothing: the integration's own test on the same word, which no removal writes
  if ((sdw_u64)a.st->occupied + (sdw_u64)np > (((sdw_u64)1 << a.capacity_log2) >> 1)) {
    if (blockIdx.x == 0 && tid == 0) atomicAdd(&ra.rs->refused_removals, 1u);
    return;
  }
  if (tid == 0) s_n = 0;
  if (tid < 2) s_cnt[tid] = 0;
  for (int k = tid; k < SDW_LH; k += SDW_NT) {
    s_key[k] = 0ull;
    s_c[k] = 0;
    for (int j = 0; j < 5; ++j) s_sum[5 * k + j] = 0ull;
  }
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
  unsigned n_rem = 0, n_miss = 0;
  for (int k = tid; k < n_list; k += SDW_NT) {
    SdwPoint p;
    if (sdw_point(a, (int)(base + (size_t)s_list[k]), &p) != 1) continue;
    const sdw_u64 wq = p.wq;
    bool done = false;
    unsigned h = (unsigned)((p.key * SDW_HASH_MUL) >> 40) & (SDW_LH - 1);
    for (int t = 0; t < SDW_LPROBE && !done; ++t, h = (h + 1) & (SDW_LH - 1)) {
      const sdw_u64 old = sdw_cas64(&s_key[h], 0ull, p.key);
      if (old != 0ull && old != p.key) continue;
      atomicAdd(&s_sum[5 * h], wq);
      atomicAdd(&s_sum[5 * h + 1], wq * p.q[0]);
      atomicAdd(&s_sum[5 * h + 2], wq * p.q[1]);
      atomicAdd(&s_sum[5 * h + 3], wq * p.q[2]);
      atomicAdd(&s_sum[5 * h + 4], wq * p.grey);
      atomicAdd(&s_c[h], 1u);
      done = true;
    }
    if (!done) {
      const unsigned r = sdw_uncommit(a, p.key, wq, wq * p.q[0], wq * p.q[1], wq * p.q[2], wq * p.grey, 1u);
      n_rem += r;
      n_miss += 1u - r;
    }
  }
  __syncthreads();
  for (int k = tid; k < SDW_LH; k += SDW_NT)
    if (s_key[k] != 0ull) {
      const unsigned r = sdw_uncommit(a, s_key[k], s_sum[5 * k], s_sum[5 * k + 1], s_sum[5 * k + 2], s_sum[5 * k + 3], s_sum[5 * k + 4], s_c[k]);
      n_rem += r;
      n_miss += s_c[k] - r;
    }
  if (n_rem) atomicAdd(&s_cnt[0], n_rem);
  if (n_miss) atomicAdd(&s_cnt[1], n_miss);
  // ---- the ticket: the last workgroup counts the removal ----------------------------------------------------------------------------
  SDW_DRAIN();      // every wavefront: its atomics have left ...
  __syncthreads();  // ... before thread 0 adds the workgroup's counts and takes its ticket
  if (tid == 0) {
    if (s_cnt[0]) atomicAdd(&ra.rs->removed, (sdw_u64)s_cnt[0]);
    if (s_cnt[1]) atomicAdd(&ra.rs->missing, (sdw_u64)s_cnt[1]);
    SDW_FENCE_RELEASE();
    s_last = (SDW_ATOMIC_ADD_AGENT(&ra.rs->ticket, 1u) == gridDim.x - 1u) ? 1 : 0;
    if (s_last) {
      SDW_FENCE_ACQUIRE();
      ra.rs->removals = ra.rs->removals + 1u;
      SDW_ST_AGENT(&ra.rs->ticket, 0u);
    }
  }
}

__global__ __launch_bounds__(SDW_NT) void semidense_world_vacant_kernel(const SdwSlot *slots, size_t n_slots, SdwReanchorState *rs) {
  __shared__ unsigned s_n;
  const int tid = (int)threadIdx.x;
  if (tid == 0) s_n = 0;
  __syncthreads();
  const size_t i = (size_t)blockIdx.x * SDW_NT + (size_t)tid;
  if (i < n_slots && slots[i].key != 0ull && slots[i].cnt == 0u) atomicAdd(&s_n, 1u);
  __syncthreads();
  if (tid == 0 && s_n) atomicAdd(&rs->vacant, s_n);
}
