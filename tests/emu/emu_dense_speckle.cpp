// emu_dense_speckle.cpp — TEST INFRASTRUCTURE: the kernels of csrc/dense_speckle_device.hpp on CPU threads (hip_emu.h), with the launch
// geometry the product's launcher uses (a workgroup per 64 x 16 tile; a lane per edge pixel; a workgroup per tile; a lane per pixel),
// before any GPU sees it.
//   emu_dense_speckle <reverse> <cpus> <w> <h> <max_size> <max_diff: the float's 32 bits, hex> <sigma: 0 | 1> <in.raw> <out.raw>
// reverse: 1 walks the workgroups of every launch from the last to the first; cpus > 0: the process is confined to that many CPUs.
// in.raw: disparity (w x h floats), with sigma = 1 sigma_invd (w x h floats), status (w x h bytes); out.raw: the same planes
// filtered, then label and size (w x h int32 each) and the two counters (n_removed, n_components). Every buffer is allocated with
// exactly the bytes it holds, so that an address sanitizer build sees any access outside one.
#ifndef _GNU_SOURCE
#define _GNU_SOURCE
#endif
#include "hip_emu.h"

#include <sched.h>
#include <stdio.h>
#include <stdlib.h>

#include <memory>

// what dense_speckle_device.hpp asks its includer for, and the two atomics hip_emu.h lacks
template <class T>
static inline T atomicMin(T *p, T v) {
  T old = __atomic_load_n(p, __ATOMIC_SEQ_CST);
  while (old > v && !__atomic_compare_exchange_n(p, &old, v, false, __ATOMIC_SEQ_CST, __ATOMIC_SEQ_CST)) {
  }
  return old;
}
template <class T>
static inline T atomicCAS(T *p, T expected, T v) {
  __atomic_compare_exchange_n(p, &expected, v, false, __ATOMIC_SEQ_CST, __ATOMIC_SEQ_CST);
  return expected;
}
#define SPK_LD_LDS(p) __atomic_load_n((p), __ATOMIC_RELAXED)
#define SPK_LD_AGENT(p) __atomic_load_n((p), __ATOMIC_RELAXED)
#include "../../visual_odometry_ros_amd/csrc/dense_speckle_device.hpp"

// the threads are started once per launch and walk the grid together (as emu_dense_stereo.cpp), forward or backward
template <class Kernel, class... Args>
static void emu_launch_pool(Kernel k, dim3 grid, dim3 block, bool reverse, Args... args) {
  gridDim = grid;
  blockDim = block;
  const unsigned nt = block.x;
  pthread_barrier_init(&emu_block_barrier, nullptr, nt);
  const unsigned nb = grid.x * grid.y;
  std::vector<std::thread> th;
  th.reserve(nt);
  for (unsigned t = 0; t < nt; ++t)
    th.emplace_back([=]() {
      threadIdx = dim3(t, 0, 0);
      for (unsigned b = 0; b < nb; ++b) {
        const unsigned bb = reverse ? nb - 1 - b : b;
        if (t == 0) blockIdx = dim3(bb % grid.x, bb / grid.x, 0);
        pthread_barrier_wait(&emu_block_barrier);
        k(args...);
        pthread_barrier_wait(&emu_block_barrier);
      }
    });
  for (auto &x : th) x.join();
  pthread_barrier_destroy(&emu_block_barrier);
}

int main(int argc, char **argv) {
  if (argc < 10) return 2;
  const int reverse = atoi(argv[1]), cpus = atoi(argv[2]), w = atoi(argv[3]), h = atoi(argv[4]), max_size = atoi(argv[5]);
  const float max_diff = __uint_as_float((unsigned)strtoul(argv[6], nullptr, 16));
  const int with_sigma = atoi(argv[7]);
  if (w < 1 || h < 1 || w > 65535 || h > 65535 || max_size < 0 || !(max_diff >= 0.0f) || !isfinite(max_diff)) return 2;
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
  std::unique_ptr<float[]> disp(new float[n]), sigma(with_sigma ? new float[n] : nullptr);
  std::unique_ptr<uint8_t[]> status(new uint8_t[n]);
  std::unique_ptr<int32_t[]> label(new int32_t[n]), size(new int32_t[n]);
  std::unique_ptr<int[]> counters(new int[2]);
  FILE *f = fopen(argv[8], "rb");
  if (!f) return 3;
  bool ok = fread(disp.get(), sizeof(float), n, f) == n;
  if (with_sigma) ok = ok && fread(sigma.get(), sizeof(float), n, f) == n;
  ok = ok && fread(status.get(), 1, n, f) == n;
  fclose(f);
  if (!ok) return 3;
  memset(label.get(), 0xEE, n * sizeof(int32_t));
  memset(size.get(), 0xEE, n * sizeof(int32_t));
  counters[0] = counters[1] = -77;
  SpkArgs a;
  memset(&a, 0, sizeof(a));
  a.disp = disp.get();
  a.sigma = sigma.get();
  a.status = status.get();
  a.label = label.get();
  a.size = size.get();
  a.counters = counters.get();
  a.W = w;
  a.H = h;
  a.n = w * h;
  a.ntx = (w + SPK_TW - 1) / SPK_TW;
  a.nty = (h + SPK_TH - 1) / SPK_TH;
  a.max_size = max_size;
  a.max_diff = max_diff;
  const int n_edge = (a.ntx - 1) * h + (a.nty - 1) * w;
  emu_launch_pool(speckle_local_kernel, dim3((unsigned)a.ntx, (unsigned)a.nty), dim3(SPK_NT), reverse != 0, a);
  if (n_edge > 0) emu_launch_pool(speckle_merge_kernel, dim3((unsigned)((n_edge + SPK_NT - 1) / SPK_NT)), dim3(SPK_NT), reverse != 0, a);
  emu_launch_pool(speckle_flatten_kernel, dim3((unsigned)a.ntx, (unsigned)a.nty), dim3(SPK_NT), reverse != 0, a);
  emu_launch_pool(speckle_apply_kernel, dim3((unsigned)((a.n + SPK_NT - 1) / SPK_NT)), dim3(SPK_NT), reverse != 0, a);
  f = fopen(argv[9], "wb");
  if (!f) return 3;
  fwrite(disp.get(), sizeof(float), n, f);
  if (with_sigma) fwrite(sigma.get(), sizeof(float), n, f);
  fwrite(status.get(), 1, n, f);
  fwrite(label.get(), sizeof(int32_t), n, f);
  fwrite(size.get(), sizeof(int32_t), n, f);
  fwrite(counters.get(), sizeof(int), 2, f);
  fclose(f);
  return 0;
}
