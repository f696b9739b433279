// emu_semidense_world_reanchor.cpp — TEST INFRASTRUCTURE: the removal kernel of csrc/semidense_world_device.hpp, the integration it
// undoes and the vacant count on CPU threads (hip_emu.h), with the launch geometry the product's launcher uses (ceil(W H / SDW_BLOCK)
// workgroups of SDW_NT threads per launch), before any GPU sees them; in the style of emu_semidense_world.cpp.
//   emu_semidense_world_reanchor <reverse> <cpus> <voxel> <capacity_log2> <min_obs> <z_max> <ops.raw> <out.raw>
// reverse: 1 walks the workgroups of every launch from the last to the first; cpus > 0: the process is confined to that many CPUs.
// ops.raw: per operation int32 op (0 integrate, 1 remove, 2 re-anchor), w, h, stride, has_key; float K[4], T[16], T2[16] (T2: the new
// pose of a re-anchor); invd, sigma (w x h floats each), n_obs (w x h bytes); with has_key h rows of `stride` bytes (the last without
// padding). A re-anchor does what the product's call does: nothing where the first 12 floats of T and T2 have the same bits, else the
// removal with T and the pre-aggregated integration with T2, a seq each. out.raw: the SdwState words, the SdwReanchorState words
// (vacant counted by its kernel), a 64-bit count of re-anchors that launched, a 64-bit count, then EVERY claimed slot (64 bytes each;
// vacated ones too: the extraction kernel with min_count 0) sorted by key. Every buffer is allocated with exactly the bytes it holds,
// so that an address sanitizer build sees any access outside one.
#ifndef _GNU_SOURCE
#define _GNU_SOURCE
#endif
#include "hip_emu.h"

#include <sched.h>
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <memory>

static inline unsigned long long sdw_cas64(unsigned long long *p, unsigned long long cmp, unsigned long long v) {
  __atomic_compare_exchange_n(p, &cmp, v, false, __ATOMIC_SEQ_CST, __ATOMIC_SEQ_CST);
  return cmp;  // (the old word: unchanged where the exchange happened)
}
#define SDW_DRAIN()
#define SDW_ST_AGENT(p, v) __atomic_store_n((p), (v), __ATOMIC_SEQ_CST)
#define SDW_ATOMIC_ADD_AGENT(p, v) __atomic_fetch_add((p), (v), __ATOMIC_SEQ_CST)
#define SDW_FENCE_RELEASE() __atomic_thread_fence(__ATOMIC_SEQ_CST)
#define SDW_FENCE_ACQUIRE() __atomic_thread_fence(__ATOMIC_SEQ_CST)

#include "../../visual_odometry_ros_amd/csrc/semidense_world_device.hpp"

// the threads are started once and walk the grid together (as emu_semidense_world.cpp), forward or backward
template <class Kernel, class... Args>
static void emu_launch_pool(Kernel k, dim3 grid, dim3 block, bool reverse, Args... args) {
  gridDim = grid;
  blockDim = block;
  const unsigned nt = block.x;
  pthread_barrier_init(&emu_block_barrier, nullptr, nt);
  const unsigned nb = grid.x;
  std::vector<std::thread> th;
  th.reserve(nt);
  for (unsigned t = 0; t < nt; ++t)
    th.emplace_back([=]() {
      threadIdx = dim3(t, 0, 0);
      for (unsigned b = 0; b < nb; ++b) {
        if (t == 0) blockIdx = dim3(reverse ? nb - 1 - b : b, 0, 0);
        pthread_barrier_wait(&emu_block_barrier);
        k(args...);
        pthread_barrier_wait(&emu_block_barrier);
      }
    });
  for (auto &x : th) x.join();
  pthread_barrier_destroy(&emu_block_barrier);
}

static bool read_all(FILE *f, void *dst, size_t bytes) { return bytes == 0 || fread(dst, 1, bytes, f) == bytes; }

int main(int argc, char **argv) {
  if (argc < 9) return 2;
  const int reverse = atoi(argv[1]), cpus = atoi(argv[2]);
  SdwArgs a;
  memset(&a, 0, sizeof(a));
  a.voxel = strtof(argv[3], nullptr);
  a.capacity_log2 = atoi(argv[4]);
  a.min_obs = atoi(argv[5]);
  a.z_max = strtof(argv[6], nullptr);
  if (a.capacity_log2 < 10 || a.capacity_log2 > 24) return 2;
  if (cpus > 0) {
    cpu_set_t have, want;
    CPU_ZERO(&want);
    if (sched_getaffinity(0, sizeof(have), &have) != 0) return 4;
    int n = 0;
    for (int i = 0; i < CPU_SETSIZE && n < cpus; ++i)
      if (CPU_ISSET(i, &have)) CPU_SET(i, &want), ++n;
    if (sched_setaffinity(0, sizeof(want), &want) != 0) return 4;
  }
  const size_t n_slots = (size_t)1 << a.capacity_log2;
  std::unique_ptr<SdwSlot[]> slots(new SdwSlot[n_slots]);
  std::unique_ptr<SdwState> st(new SdwState);
  std::unique_ptr<SdwReanchorState> rs(new SdwReanchorState);
  memset(slots.get(), 0, n_slots * sizeof(SdwSlot));
  memset(st.get(), 0, sizeof(SdwState));
  memset(rs.get(), 0, sizeof(SdwReanchorState));
  a.slots = slots.get();
  a.st = st.get();
  unsigned long long reanchors = 0;
  FILE *f = fopen(argv[7], "rb");
  if (!f) return 3;
  int32_t hdr[5];
  while (fread(hdr, 4, 5, f) == 5) {
    const int op = hdr[0], w = hdr[1], h = hdr[2], stride = hdr[3], has_key = hdr[4];
    float KT[36];
    if (op < 0 || op > 2 || w < 1 || h < 1 || stride < w || !read_all(f, KT, sizeof(KT))) return 3;
    const size_t n = (size_t)w * h, nimg = (size_t)stride * (h - 1) + w;  // (the last row has no padding: exact)
    std::unique_ptr<float[]> invd(new float[n]), sigma(new float[n]);
    std::unique_ptr<uint8_t[]> n_obs(new uint8_t[n]), key;
    if (!read_all(f, invd.get(), 4 * n) || !read_all(f, sigma.get(), 4 * n) || !read_all(f, n_obs.get(), n)) return 3;
    if (has_key) {
      key.reset(new uint8_t[nimg]);
      if (!read_all(f, key.get(), nimg)) return 3;
    }
    a.invd = invd.get();
    a.sigma = sigma.get();
    a.n_obs = n_obs.get();
    a.Lk = key.get();
    a.strideK = stride;
    a.W = w;
    a.H = h;
    a.fx = KT[0], a.fy = KT[1], a.cx = KT[2], a.cy = KT[3];
    const dim3 grid((unsigned)((n + SDW_BLOCK - 1) / SDW_BLOCK), 1, 1);
    if (op == 2 && memcmp(KT + 4, KT + 20, 12 * sizeof(float)) == 0) continue;  // the same bits: no launch, no seq
    if (op != 0) {
      memcpy(a.T, KT + 4, sizeof(a.T));
      ++a.seq;
      SdwRemoveArgs ra;
      ra.a = a;
      ra.rs = rs.get();
      emu_launch_pool(semidense_world_remove_kernel, grid, dim3(SDW_NT), reverse != 0, ra);
      if (rs->ticket != 0) return 5;  // the launch's word is zero again
    }
    if (op != 1) {
      memcpy(a.T, KT + (op == 2 ? 20 : 4), sizeof(a.T));
      ++a.seq;
      emu_launch_pool(semidense_world_integrate_kernel<true>, grid, dim3(SDW_NT), reverse != 0, a);
      if (st->ticket != 0 || st->claimed != 0) return 5;
    }
    if (op == 2) ++reanchors;
  }
  fclose(f);
  emu_launch_pool(semidense_world_vacant_kernel, dim3((unsigned)(n_slots / SDW_NT)), dim3(SDW_NT), false, (const SdwSlot *)slots.get(), n_slots,
                  rs.get());
  // the extraction kernel with min_count 0, min_keyframes 0: every claimed slot, vacated ones too; sorted here as the host does
  SdwExtractArgs e;
  memset(&e, 0, sizeof(e));
  e.slots = slots.get();
  e.n_slots = n_slots;
  e.cap = st->occupied;
  std::unique_ptr<SdwSlot[]> out(new SdwSlot[e.cap ? e.cap : 1]);
  e.out = out.get();
  e.st = st.get();
  emu_launch_pool(semidense_world_extract_kernel, dim3((unsigned)(n_slots / SDW_NT)), dim3(SDW_NT), false, e);
  if (st->n_extract != st->occupied) return 6;  // (a removal frees no slot and claims none)
  std::sort(out.get(), out.get() + e.cap, [](const SdwSlot &x, const SdwSlot &y) { return x.key < y.key; });
  FILE *fo = fopen(argv[8], "wb");
  if (!fo) return 3;
  const unsigned long long cnt = e.cap;
  fwrite(st.get(), sizeof(SdwState), 1, fo);
  fwrite(rs.get(), sizeof(SdwReanchorState), 1, fo);
  fwrite(&reanchors, 8, 1, fo);
  fwrite(&cnt, 8, 1, fo);
  fwrite(out.get(), sizeof(SdwSlot), e.cap, fo);
  fclose(fo);
  return 0;
}
