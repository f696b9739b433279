// emu_semidense_map_merge.cpp — TEST INFRASTRUCTURE: the kernel of csrc/semidense_map_merge_device.hpp on CPU threads (hip_emu.h), with the
// launch geometry and the alignment rule the product's launcher uses (256 lanes a workgroup, four pixels a lane; sdm_grid,
// sdm_planes_aligned), before any GPU sees it.
//   emu_semidense_map_merge <reverse> <cpus> <w> <h> <chi: the float's 32 bits, hex> <keep_obs> <bf: hex> <map: 0 | 1> <origin: 0 | 1>
//                           <counts: 0 | 1> <alias: 0 | 1> <offset mask> <in.raw> <out.raw>
// reverse: 1 walks the workgroups from the last to the first; cpus > 0: the process is confined to that many CPUs. map: 0 none, 1 the
// three planes. alias: the outputs invd, sigma, n_obs ARE the map's planes. offset mask: bit k set puts plane k one element behind a 16-byte boundary — planes 0 map invd,
// 1 map sigma, 2 map n_obs, 3 disparity, 4 sigma_invd, 5 status, 6 invd, 7 sigma, 8 n_obs, 9 origin.
// in.raw: with a map its invd, sigma (w x h floats each) and n_obs (bytes); then disparity, sigma_invd (floats), status (bytes).
// out.raw: invd, sigma (floats), n_obs (bytes), with origin that plane (bytes), with counts six 64-bit words.
// Every plane ends exactly where its allocation ends, so that an address sanitizer build sees any access behind one.
#ifndef _GNU_SOURCE
#define _GNU_SOURCE
#endif
#include "hip_emu.h"

#include <sched.h>
#include <stdio.h>
#include <stdlib.h>

#define SDM_WAVE_SUM(v) ((unsigned)emu_wave_sum_i32((int)(v)))
#include "../../visual_odometry_ros_amd/csrc/semidense_map_merge_device.hpp"

// the threads are started once and walk the grid together (as emu_dense_speckle.cpp), forward or backward; with the wavefronts' barriers
template <class Kernel, class... Args>
static void emu_launch_pool(Kernel k, dim3 grid, dim3 block, bool reverse, Args... args) {
  gridDim = grid;
  blockDim = block;
  const unsigned nt = block.x;
  pthread_barrier_init(&emu_block_barrier, nullptr, nt);
  for (unsigned w = 0; w < (nt + 63) / 64; ++w) pthread_barrier_init(&emu_wave_barrier[w], nullptr, (nt - 64 * w) < 64 ? nt - 64 * w : 64);
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
  for (unsigned w = 0; w < (nt + 63) / 64; ++w) pthread_barrier_destroy(&emu_wave_barrier[w]);
}

// `count` elements of `size` bytes that END where the allocation ends; off: the first one sits one element behind a 16-byte boundary
struct Plane {
  void *base = nullptr;
  char *p = nullptr;
  size_t bytes = 0;
  bool make(size_t count, size_t size, bool off) {
    bytes = count * size;
    const size_t lead = off ? size : 0;
    if (posix_memalign(&base, 16, lead + bytes) != 0) return false;
    p = (char *)base + lead;
    memset(p, 0xEE, bytes);
    return true;
  }
  ~Plane() { free(base); }
};

int main(int argc, char **argv) {
  if (argc < 15) return 2;
  const int reverse = atoi(argv[1]), cpus = atoi(argv[2]), w = atoi(argv[3]), h = atoi(argv[4]);
  const float chi = __uint_as_float((unsigned)strtoul(argv[5], nullptr, 16));
  const int keep_obs = atoi(argv[6]);
  const float bf = __uint_as_float((unsigned)strtoul(argv[7], nullptr, 16));
  const int with_map = atoi(argv[8]), with_origin = atoi(argv[9]), with_counts = atoi(argv[10]), alias = atoi(argv[11]);
  const unsigned off = (unsigned)strtoul(argv[12], nullptr, 0);
  if (w < 1 || h < 1 || (long long)w * h > 0x7fffffffLL || !(chi > 0.0f) || keep_obs < 0 || keep_obs > 256 || !(bf > 0.0f)) return 2;
  if (alias && !with_map) return 2;
  if (cpus > 0) {
    cpu_set_t have, want;
    CPU_ZERO(&want);
    if (sched_getaffinity(0, sizeof(have), &have) != 0) return 4;
    int n = 0;
    for (int i = 0; i < CPU_SETSIZE && n < cpus; ++i)
      if (CPU_ISSET(i, &have)) CPU_SET(i, &want), ++n;
    if (sched_setaffinity(0, sizeof(want), &want) != 0) return 4;
  }
  const size_t n = (size_t)w * h;
  Plane pl[10], cnt;
  const size_t esz[10] = {4, 4, 1, 4, 4, 1, 4, 4, 1, 1};
  for (int k = 0; k < 10; ++k) {
    const bool need = k < 3 ? with_map != 0 : k < 6 ? true : k < 9 ? !alias : with_origin != 0;
    if (need && !pl[k].make(n, esz[k], (off >> k) & 1u)) return 4;
  }
  if (with_counts && !cnt.make(SDM_ORIGINS, sizeof(unsigned long long), false)) return 4;
  FILE *f = fopen(argv[13], "rb");
  if (!f) return 3;
  bool ok = true;
  for (int k = with_map ? 0 : 3; k < 6; ++k) ok = ok && fread(pl[k].p, esz[k], n, f) == n;
  fclose(f);
  if (!ok) return 3;
  SdmArgs a;
  memset(&a, 0, sizeof(a));
  if (with_map) a.invd_m = (const float *)pl[0].p, a.sigma_m = (const float *)pl[1].p, a.n_obs_m = (const uint8_t *)pl[2].p;
  a.disp = (const float *)pl[3].p, a.sigma_invd = (const float *)pl[4].p, a.status = (const uint8_t *)pl[5].p;
  a.bf = bf;
  a.chi2 = chi * chi;
  a.keep_obs = keep_obs;
  a.invd = (float *)pl[alias ? 0 : 6].p, a.sigma = (float *)pl[alias ? 1 : 7].p, a.n_obs = (uint8_t *)pl[alias ? 2 : 8].p;
  a.origin = with_origin ? (uint8_t *)pl[9].p : nullptr;
  a.counts = with_counts ? (unsigned long long *)cnt.p : nullptr;
  a.n = (int)n;
  a.vec = sdm_planes_aligned(a);
  if (a.counts) memset(a.counts, 0, SDM_ORIGINS * sizeof(unsigned long long));  // (the launch's predecessor)
  emu_launch_pool(semidense_map_merge_kernel, dim3(sdm_grid(a.n)), dim3(SDM_NT), reverse != 0, a);
  f = fopen(argv[14], "wb");
  if (!f) return 3;
  fwrite(a.invd, 4, n, f);
  fwrite(a.sigma, 4, n, f);
  fwrite(a.n_obs, 1, n, f);
  if (with_origin) fwrite(a.origin, 1, n, f);
  if (with_counts) fwrite(a.counts, sizeof(unsigned long long), SDM_ORIGINS, f);
  fputc(a.vec ? 1 : 0, f);  // which path ran
  fclose(f);
  return 0;
}
