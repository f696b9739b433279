// emu_semidense_temporal.cpp — TEST INFRASTRUCTURE: the kernel of csrc/semidense_temporal_device.hpp on CPU threads (hip_emu.h),
// with the launch geometry the product's launcher uses (grid = column segments x rows, SDT_NT threads), before any GPU sees it.
//   emu_semidense_temporal <w> <h> <stride> <hw> <hh> <g_min> <thres_best> <thres_peak> <peak_px> <edge_px> <eps_edge> <eps_epi>
//                          <z_min> <z_max> <max_search> <j_min> <eps_scale> <fx> <fy> <cx> <cy> <T_ck: 16 floats> <key.raw> <cur.raw>
//                          <mask.raw | -> <map.raw> <out.raw>
// key.raw / cur.raw: h rows of `stride` bytes; mask.raw: w x h bytes (0 = ignore), "-": none; map.raw: invd, sigma (w x h floats
// each), n_obs, tstatus (w x h bytes each); out.raw: the same four planes after the launch, then score (w x h floats). Every
// buffer is allocated with exactly the bytes it holds, so that an address sanitizer build sees any tap outside an image.
#include "hip_emu.h"

#include <stdio.h>
#include <stdlib.h>

#include <memory>

#include "../../visual_odometry_ros_amd/csrc/semidense_temporal_device.hpp"

// the threads are started once and walk the grid together (as emu_semidense.cpp: two barrier waits between workgroups)
template <class Kernel, class... Args>
static void emu_launch_pool(Kernel k, dim3 grid, dim3 block, Args... args) {
  gridDim = grid;
  blockDim = block;
  const unsigned nt = block.x;
  pthread_barrier_init(&emu_block_barrier, nullptr, nt);
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
}

static bool read_all(FILE *f, void *dst, size_t bytes) { return f && fread(dst, 1, bytes, f) == bytes; }
static bool read_file(const char *path, void *dst, size_t bytes) {
  FILE *f = fopen(path, "rb");
  const bool ok = read_all(f, dst, bytes);
  if (f) fclose(f);
  return ok;
}

int main(int argc, char **argv) {
  if (argc < 43) return 2;
  const int w = atoi(argv[1]), h = atoi(argv[2]), stride = atoi(argv[3]);
  SdtArgs a;
  memset(&a, 0, sizeof(a));
  a.hw = atoi(argv[4]);
  a.hh = atoi(argv[5]);
  const int g_min = atoi(argv[6]);
  a.g_min2 = g_min * g_min;
  a.thres_best = strtof(argv[7], nullptr);
  a.thres_peak = strtof(argv[8], nullptr);
  a.peak_px = atoi(argv[9]);
  a.edge_px = atoi(argv[10]);
  a.eps_edge = strtof(argv[11], nullptr);
  a.eps_epi = strtof(argv[12], nullptr);
  const float z_min = strtof(argv[13], nullptr), z_max = strtof(argv[14], nullptr);
  a.r_min = 1.0f / z_max;
  a.r_max = 1.0f / z_min;
  a.max_search = atoi(argv[15]);
  a.j_min = strtof(argv[16], nullptr);
  a.eps_scale = strtof(argv[17], nullptr);
  a.fx = strtof(argv[18], nullptr);
  a.fy = strtof(argv[19], nullptr);
  a.cx = strtof(argv[20], nullptr);
  a.cy = strtof(argv[21], nullptr);
  float T[16];
  for (int i = 0; i < 16; ++i) T[i] = strtof(argv[22 + i], nullptr);
  sdt_pose(&a, T);
  if (w < 3 || h < 3 || stride < w || a.hw < 1 || a.hw > SDT_MAX_HW || a.hh < 0 || a.hh > SDT_MAX_HH || a.max_search < 1 ||
      a.max_search > SDT_MAX_SEARCH || a.edge_px < 0)
    return 2;
  const size_t n = (size_t)w * h, nimg = (size_t)stride * (h - 1) + w;  // (the last row has no padding: exact)
  std::unique_ptr<uint8_t[]> key(new uint8_t[nimg]), cur(new uint8_t[nimg]), mask, n_obs(new uint8_t[n]), tstatus(new uint8_t[n]);
  std::unique_ptr<float[]> invd(new float[n]), sigma(new float[n]), score(new float[n]);
  if (!read_file(argv[38], key.get(), nimg) || !read_file(argv[39], cur.get(), nimg)) return 3;
  if (strcmp(argv[40], "-") != 0) {
    mask.reset(new uint8_t[n]);
    if (!read_file(argv[40], mask.get(), n)) return 3;
  }
  FILE *fm = fopen(argv[41], "rb");
  const bool ok = read_all(fm, invd.get(), 4 * n) && read_all(fm, sigma.get(), 4 * n) && read_all(fm, n_obs.get(), n) && read_all(fm, tstatus.get(), n);
  if (fm) fclose(fm);
  if (!ok) return 3;
  for (size_t i = 0; i < n; ++i) score[i] = -7.0f;
  a.Lk = key.get();
  a.Lc = cur.get();
  a.strideK = a.strideC = stride;
  a.W = w;
  a.H = h;
  a.mask = mask.get();
  a.mask_stride = w;
  a.invd = invd.get();
  a.sigma = sigma.get();
  a.n_obs = n_obs.get();
  a.tstatus = tstatus.get();
  a.score = score.get();
  emu_launch_pool(semidense_temporal_kernel, dim3((unsigned)((w + SDT_SEG - 1) / SDT_SEG), (unsigned)h, 1), dim3(SDT_NT), a);
  FILE *f = fopen(argv[42], "wb");
  if (!f) return 3;
  fwrite(invd.get(), 4, n, f);
  fwrite(sigma.get(), 4, n, f);
  fwrite(n_obs.get(), 1, n, f);
  fwrite(tstatus.get(), 1, n, f);
  fwrite(score.get(), 4, n, f);
  fclose(f);
  return 0;
}
