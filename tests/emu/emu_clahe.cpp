// emu_clahe.cpp — TEST INFRASTRUCTURE: the two kernels of csrc/clahe_device.hpp on CPU threads (hip_emu.h), with the launch
// geometry the product's launcher uses (clahe_plan), before any GPU sees them.
//   emu_clahe <w> <h> <stride> <tiles_x> <tiles_y> <clip> <in.raw> <out.raw> <luts.raw> [slab_px]
// in.raw: h rows of `stride` bytes; out.raw: w x h bytes; luts.raw: tiles_y * tiles_x * 256 bytes. slab_px (default 8192, the
// product's) sets how many pixels of a tile one histogram workgroup counts: a small value makes several workgroups share a
// tile's counters and ticket; both launches then run twice on the same counters: the second run sees what the first left behind.
// Exit status 4: counters or tickets were not back at zero after a launch.
#include "hip_emu.h"

#include <stdio.h>
#include <stdlib.h>

#include <vector>

// what clahe_device.hpp asks its includer for (hip_emu.h has the ORB kernels' shims only)
#define CLAHE_LD_AGENT(p) __atomic_load_n((p), __ATOMIC_SEQ_CST)
#define CLAHE_ST_AGENT(p, v) __atomic_store_n((p), (v), __ATOMIC_SEQ_CST)
#define CLAHE_ATOMIC_ADD_AGENT(p, v) __atomic_fetch_add((p), (v), __ATOMIC_SEQ_CST)
#define CLAHE_FENCE_RELEASE() __atomic_thread_fence(__ATOMIC_SEQ_CST)
#define CLAHE_FENCE_ACQUIRE() __atomic_thread_fence(__ATOMIC_SEQ_CST)
#define CLAHE_DYN_LDS(name) uint8_t *name = emu_dyn_lds
#include "../../visual_odometry_ros_amd/csrc/clahe_device.hpp"

// emu_launch starts the threads of every workgroup anew; these grids have up to a thousand small workgroups, so the threads
// are started once and walk the grid together (two barrier waits between workgroups: all have left one, blockIdx is the next)
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

int main(int argc, char **argv) {
  if (argc < 10) return 2;
  const int w = atoi(argv[1]), h = atoi(argv[2]), stride = atoi(argv[3]), tx = atoi(argv[4]), ty = atoi(argv[5]);
  const double clip = atof(argv[6]);
  const int slab_px = argc > 10 ? atoi(argv[10]) : 8192;
  if (w <= tx || h <= ty || stride < w || tx < 1 || ty < 1 || tx > CLAHE_MAX_TILES || ty > CLAHE_MAX_TILES) return 2;
  std::vector<uint8_t> in((size_t)stride * h);
  FILE *f = fopen(argv[7], "rb");
  if (!f || fread(in.data(), 1, in.size(), f) != in.size()) return 3;
  fclose(f);
  const int dstride = (w + 63) & ~63;
  std::vector<uint32_t> out32((size_t)dstride * h / 4 + 1, 0xA5A5A5A5u), lut32((size_t)tx * ty * 64);
  std::vector<int> hist((size_t)tx * ty * 256, 0), ticket((size_t)tx * ty, 0);
  ClaheArgs a;
  memset(&a, 0, sizeof(a));
  clahe_plan(&a, w, h, tx, ty, clip, slab_px);
  a.sstride = stride;
  a.dstride = dstride;
  for (int i = 0; i < 2; ++i) a.img[i] = {in.data(), (uint8_t *)out32.data(), (uint8_t *)lut32.data(), hist.data(), ticket.data()};
  if ((size_t)a.lds_cols * a.lds_rows * 256 > sizeof(emu_dyn_lds) || !clahe_stage_fits(&a)) return 2;
  for (int rep = 0; rep < (argc > 10 ? 2 : 1); ++rep) {
    emu_launch_pool(clahe_hist_kernel, dim3(a.slabs, tx * ty, 1), dim3(CLAHE_NT), a);
    for (int v : hist)
      if (v) return 4;
    for (int v : ticket)
      if (v) return 4;
    emu_launch_pool(clahe_blend_kernel, dim3((w + CLAHE_BLEND_COLS - 1) / CLAHE_BLEND_COLS, (h + CLAHE_BLEND_ROWS - 1) / CLAHE_BLEND_ROWS, 1),
                    dim3(CLAHE_NT), a);
  }
  f = fopen(argv[8], "wb");
  if (!f) return 3;
  for (int y = 0; y < h; ++y) fwrite((const uint8_t *)out32.data() + (size_t)y * dstride, 1, (size_t)w, f);
  fclose(f);
  f = fopen(argv[9], "wb");
  if (!f) return 3;
  fwrite(lut32.data(), 1, (size_t)tx * ty * 256, f);
  fclose(f);
  return 0;
}
