// emu_semidense_world_carve.cpp — TEST INFRASTRUCTURE: the carve kernel of csrc/semidense_world_carve_device.hpp, in both forms, next
// to the integration and the removal of csrc/semidense_world_device.hpp on CPU threads (hip_emu.h), with the launch geometry the
// product's launcher uses (ceil(W H / SDW_BLOCK) workgroups of SDW_NT threads per launch), before any GPU sees it; in the style of
// emu_semidense_world_reanchor.cpp.
//   emu_semidense_world_carve <reverse> <cpus> <form> <voxel> <capacity_log2> <min_obs> <z_max> <ops.raw> <out.raw>
// reverse: 1 walks the workgroups of every launch from the last to the first; cpus > 0: the process is confined to that many CPUs;
// form: 0 the pre-aggregated carve, 1 the simple one. ops.raw: per operation int32 op (0 integrate, 1 remove, 3 carve, 4 clear), w, h,
// stride, has_key; for every op but clear float K[4], T[16], margin, chi, z_near; invd, sigma (w x h floats each), n_obs (w x h
// bytes); with has_key h rows of `stride` bytes (the last without padding). A carve does what the product's launcher does: k0 is
// worked out here, on the host. out.raw: the SdwState, SdwReanchorState and SdwCarveState words, a 64-bit count, then EVERY claimed
// slot (64 bytes each; vacated ones too: the free extraction kernel with min_count 0 and no filter) sorted by key. Every buffer is
// allocated with exactly the bytes it holds, so that an address sanitizer build sees any access outside one.
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

#include "../../visual_odometry_ros_amd/csrc/semidense_world_carve_device.hpp"

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
  if (argc < 10) return 2;
  const int reverse = atoi(argv[1]), cpus = atoi(argv[2]), form = atoi(argv[3]);
  SdwArgs a;
  memset(&a, 0, sizeof(a));
  a.voxel = strtof(argv[4], nullptr);
  a.capacity_log2 = atoi(argv[5]);
  a.min_obs = atoi(argv[6]);
  a.z_max = strtof(argv[7], nullptr);
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
  std::unique_ptr<SdwCarveState> cs(new SdwCarveState);
  memset(slots.get(), 0, n_slots * sizeof(SdwSlot));
  memset(st.get(), 0, sizeof(SdwState));
  memset(rs.get(), 0, sizeof(SdwReanchorState));
  memset(cs.get(), 0, sizeof(SdwCarveState));
  a.slots = slots.get();
  a.st = st.get();
  FILE *f = fopen(argv[8], "rb");
  if (!f) return 3;
  int32_t hdr[5];
  while (fread(hdr, 4, 5, f) == 5) {
    const int op = hdr[0], w = hdr[1], h = hdr[2], stride = hdr[3], has_key = hdr[4];
    if (op == 4) {  // clear: the table, every count and the seq
      memset(slots.get(), 0, n_slots * sizeof(SdwSlot));
      memset(st.get(), 0, sizeof(SdwState));
      memset(rs.get(), 0, sizeof(SdwReanchorState));
      memset(cs.get(), 0, sizeof(SdwCarveState));
      a.seq = 0;
      continue;
    }
    float KT[23];
    if ((op != 0 && op != 1 && op != 3) || w < 1 || h < 1 || stride < w || !read_all(f, KT, sizeof(KT))) return 3;
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
    memcpy(a.T, KT + 4, sizeof(a.T));
    const dim3 grid((unsigned)((n + SDW_BLOCK - 1) / SDW_BLOCK), 1, 1);
    if (op == 1) {
      ++a.seq;
      SdwRemoveArgs ra;
      ra.a = a;
      ra.rs = rs.get();
      emu_launch_pool(semidense_world_remove_kernel, grid, dim3(SDW_NT), reverse != 0, ra);
      if (rs->ticket != 0) return 5;  // the launch's word is zero again
    } else if (op == 0) {
      ++a.seq;
      emu_launch_pool(semidense_world_integrate_kernel<true>, grid, dim3(SDW_NT), reverse != 0, a);
      if (st->ticket != 0 || st->claimed != 0) return 5;
    } else {
      SdwCarveArgs ca;
      memset(&ca, 0, sizeof(ca));
      ca.a = a;
      ca.a.Lk = nullptr;
      ca.margin = KT[20], ca.chi = KT[21], ca.z_near = KT[22];
      ca.dz = a.voxel * 0.5f;
      ca.k0 = 1;
      while (ca.k0 <= SDWC_MAX_K && !(ca.z_near <= (float)ca.k0 * ca.dz)) ++ca.k0;
      ca.cs = cs.get();
      if (form == 1)
        emu_launch_pool(semidense_world_carve_kernel<false>, grid, dim3(SDW_NT), reverse != 0, ca);
      else
        emu_launch_pool(semidense_world_carve_kernel<true>, grid, dim3(SDW_NT), reverse != 0, ca);
    }
  }
  fclose(f);
  emu_launch_pool(semidense_world_vacant_kernel, dim3((unsigned)(n_slots / SDW_NT)), dim3(SDW_NT), false, (const SdwSlot *)slots.get(), n_slots,
                  rs.get());
  // the free extraction kernel with min_count 0, min_keyframes 0, no filter: every claimed slot, vacated ones too; sorted as the host does
  SdwExtractFreeArgs e;
  memset(&e, 0, sizeof(e));
  e.e.slots = slots.get();
  e.e.n_slots = n_slots;
  e.e.cap = st->occupied;
  std::unique_ptr<SdwSlot[]> out(new SdwSlot[e.e.cap ? e.e.cap : 1]);
  e.e.out = out.get();
  e.e.st = st.get();
  emu_launch_pool(semidense_world_extract_free_kernel, dim3((unsigned)(n_slots / SDW_NT)), dim3(SDW_NT), false, e);
  if (st->n_extract != st->occupied) return 6;  // (neither a removal nor a carve frees a slot or claims one)
  std::sort(out.get(), out.get() + e.e.cap, [](const SdwSlot &x, const SdwSlot &y) { return x.key < y.key; });
  FILE *fo = fopen(argv[9], "wb");
  if (!fo) return 3;
  const unsigned long long cnt = e.e.cap;
  fwrite(st.get(), sizeof(SdwState), 1, fo);
  fwrite(rs.get(), sizeof(SdwReanchorState), 1, fo);
  fwrite(cs.get(), sizeof(SdwCarveState), 1, fo);
  fwrite(&cnt, 8, 1, fo);
  fwrite(out.get(), sizeof(SdwSlot), e.e.cap, fo);
  fclose(fo);
  return 0;
}
