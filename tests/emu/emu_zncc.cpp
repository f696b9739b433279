// emu_zncc.cpp — TEST INFRASTRUCTURE: the kernel of csrc/zncc_device.hpp on CPU threads (hip_emu.h), with the launch geometry
// the product's launcher uses (zncc_plan, one wavefront per feature, ZNCC_WAVES features per workgroup, grid.y = image pairs),
// before any GPU sees it.
//   emu_zncc <w> <h> <stride> <win> <pattern> <ref> <n> <img0.raw> <img1.raw> <pts.raw> <out.raw>
// img*.raw: h rows of `stride` bytes; pts.raw: n x 2 floats pts0, then n x 2 floats pts1; out.raw: 2 x n floats — the launch has
// two pairs, (img0 at pts0, img1 at pts1) and the same with the roles swapped, as the gate's temporal + stereo launch has.
// pattern: 0 reference, 1 centred; ref: 1 = index-order sums, 0 = the tree.
#include "hip_emu.h"

#include <stdio.h>
#include <stdlib.h>

#include <vector>

// what zncc_device.hpp asks its includer for: the wavefront's cross-lane reads, through a scratch line per workgroup thread
static float emu_wave_f32[64 * 64];
static inline float emu_shfl_down(float v, int d) {
  const int tid = (int)threadIdx.x, wave = tid >> 6, lane = tid & 63;
  emu_wave_f32[tid] = v;
  pthread_barrier_wait(&emu_wave_barrier[wave]);
  const float r = lane + d < 64 ? emu_wave_f32[tid + d] : v;
  pthread_barrier_wait(&emu_wave_barrier[wave]);
  return r;
}
static inline float emu_bcast0(float v) {
  const int tid = (int)threadIdx.x, wave = tid >> 6;
  emu_wave_f32[tid] = v;
  pthread_barrier_wait(&emu_wave_barrier[wave]);
  const float r = emu_wave_f32[wave << 6];
  pthread_barrier_wait(&emu_wave_barrier[wave]);
  return r;
}
#define ZNCC_SHFL_DOWN(v, d) emu_shfl_down((v), (d))
#define ZNCC_BCAST0(v) emu_bcast0((v))
#include "../../visual_odometry_ros_amd/csrc/zncc_device.hpp"

// the threads are started once and walk the grid together (as emu_clahe.cpp: two barrier waits between workgroups)
template <class Kernel, class... Args>
static void emu_launch_pool(Kernel k, dim3 grid, dim3 block, Args... args) {
  gridDim = grid;
  blockDim = block;
  const unsigned nt = block.x;
  pthread_barrier_init(&emu_block_barrier, nullptr, nt);
  for (unsigned w = 0; w < (nt + 63) / 64; ++w) pthread_barrier_init(&emu_wave_barrier[w], nullptr, (nt - 64 * w) < 64 ? nt - 64 * w : 64);
  const unsigned nb = grid.x * grid.y * grid.z;
  std::vector<std::thread> th;
  th.reserve(nt);
  for (unsigned t = 0; t < nt; ++t)
    th.emplace_back([=]() {
      threadIdx = dim3(t, 0, 0);
      for (unsigned b = 0; b < nb; ++b) {
        if (t == 0) blockIdx = dim3(b % grid.x, (b / grid.x) % grid.y, b / (grid.x * grid.y));
        pthread_barrier_wait(&emu_block_barrier);
        k(args...);
        pthread_barrier_wait(&emu_block_barrier);
      }
    });
  for (auto &x : th) x.join();
  pthread_barrier_destroy(&emu_block_barrier);
  for (unsigned w = 0; w < (nt + 63) / 64; ++w) pthread_barrier_destroy(&emu_wave_barrier[w]);
}

static bool read_all(const char *path, void *dst, size_t bytes) {
  FILE *f = fopen(path, "rb");
  const bool ok = f && fread(dst, 1, bytes, f) == bytes;
  if (f) fclose(f);
  return ok;
}

int main(int argc, char **argv) {
  if (argc < 12) return 2;
  const int w = atoi(argv[1]), h = atoi(argv[2]), stride = atoi(argv[3]), win = atoi(argv[4]), pattern = atoi(argv[5]);
  const int ref = atoi(argv[6]), n = atoi(argv[7]);
  if (w < 2 || h < 2 || stride < w || win < ZNCC_MIN_WIN || win > ZNCC_MAX_WIN || !(win & 1) || n < 1) return 2;
  std::vector<uint8_t> img0((size_t)stride * h), img1((size_t)stride * h);
  std::vector<float> pts(4 * (size_t)n), out(2 * (size_t)n, -7.0f);
  if (!read_all(argv[8], img0.data(), img0.size()) || !read_all(argv[9], img1.data(), img1.size()) ||
      !read_all(argv[10], pts.data(), pts.size() * sizeof(float)))
    return 3;
  ZnccArgs a;
  memset(&a, 0, sizeof(a));
  zncc_plan(&a, win, pattern);
  a.W = w;
  a.H = h;
  a.n = n;
  a.pair[0] = {img0.data(), img1.data(), stride, stride, pts.data(), pts.data() + 2 * (size_t)n, out.data()};
  a.pair[1] = {img1.data(), img0.data(), stride, stride, pts.data() + 2 * (size_t)n, pts.data(), out.data() + n};
  const zncc_kernel_fn k = zncc_kernel_for(ref != 0, a.J);
  if (!k) return 2;
  emu_launch_pool(k, dim3((unsigned)((n + ZNCC_WAVES - 1) / ZNCC_WAVES), 2, 1), dim3(ZNCC_NT), a);
  FILE *f = fopen(argv[11], "wb");
  if (!f) return 3;
  fwrite(out.data(), sizeof(float), out.size(), f);
  fclose(f);
  return 0;
}
