// emu_semidense_regularize.cpp — TEST INFRASTRUCTURE: the kernel of csrc/semidense_regularize_device.hpp on CPU threads (hip_emu.h),
// with the launch geometry the product's launcher uses (ceil(W / SDR_TW) x ceil(H / SDR_TH) workgroups of SDR_NT threads, one
// launch), before any GPU sees it.
//   emu_semidense_regularize <w> <h> <stride> <radius> <chi> <dist_sigma> <min_support> <fill_min> <g_min>
//                            <map.raw> <key.raw> <mask.raw | -> <out.raw>
// map.raw: invd, sigma (w x h floats each), n_obs (w x h bytes); key.raw: h rows of `stride` bytes (the last without padding);
// mask.raw: w x h bytes (0 = ignore), "-": none; out.raw: invd, sigma (floats), n_obs, rstatus (bytes).
// Every buffer is allocated with exactly the bytes it holds, so that an address sanitizer build sees any access outside one.
#include "hip_emu.h"

#include <stdio.h>
#include <stdlib.h>

#include <memory>

#include "../../visual_odometry_ros_amd/csrc/semidense_regularize_device.hpp"

// the threads are started once and walk the grid together (as emu_semidense_propagate.cpp: two barrier waits between workgroups)
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
  if (argc < 14) return 2;
  const int w = atoi(argv[1]), h = atoi(argv[2]), stride = atoi(argv[3]);
  SdrArgs a;
  memset(&a, 0, sizeof(a));
  a.radius = atoi(argv[4]);
  const float chi = strtof(argv[5], nullptr), dist_sigma = strtof(argv[6], nullptr);
  a.chi2 = chi * chi;
  a.dist2 = dist_sigma * dist_sigma;
  a.min_support = atoi(argv[7]);
  a.fill_min = atoi(argv[8]);
  const int g_min = atoi(argv[9]);
  a.g_min2 = g_min * g_min;
  if (w < 3 || h < 3 || stride < w || a.radius < 1 || a.radius > SDR_MAX_R) return 2;
  const size_t n = (size_t)w * h, nimg = (size_t)stride * (h - 1) + w;  // (the last row has no padding: exact)
  std::unique_ptr<uint8_t[]> key(new uint8_t[nimg]), mask, no(new uint8_t[n]), n_obs_r(new uint8_t[n]), rstatus(new uint8_t[n]);
  std::unique_ptr<float[]> invd(new float[n]), sigma(new float[n]), invd_r(new float[n]), sigma_r(new float[n]);
  FILE *fm = fopen(argv[10], "rb");
  const bool ok = read_all(fm, invd.get(), 4 * n) && read_all(fm, sigma.get(), 4 * n) && read_all(fm, no.get(), n);
  if (fm) fclose(fm);
  if (!ok || !read_file(argv[11], key.get(), nimg)) return 3;
  if (strcmp(argv[12], "-") != 0) {
    mask.reset(new uint8_t[n]);
    if (!read_file(argv[12], mask.get(), n)) return 3;
  }
  for (size_t i = 0; i < n; ++i) invd_r[i] = sigma_r[i] = -7.0f, n_obs_r[i] = rstatus[i] = 0x5A;
  a.invd = invd.get();
  a.sigma = sigma.get();
  a.n_obs = no.get();
  a.Lk = key.get();
  a.strideK = stride;
  a.W = w;
  a.H = h;
  a.mask = mask.get();
  a.mask_stride = w;
  a.invd_r = invd_r.get();
  a.sigma_r = sigma_r.get();
  a.n_obs_r = n_obs_r.get();
  a.rstatus = rstatus.get();
  emu_launch_pool(semidense_regularize_kernel, dim3((unsigned)((w + SDR_TW - 1) / SDR_TW), (unsigned)((h + SDR_TH - 1) / SDR_TH), 1), dim3(SDR_NT), a);
  FILE *f = fopen(argv[13], "wb");
  if (!f) return 3;
  fwrite(invd_r.get(), 4, n, f);
  fwrite(sigma_r.get(), 4, n, f);
  fwrite(n_obs_r.get(), 1, n, f);
  fwrite(rstatus.get(), 1, n, f);
  fclose(f);
  return 0;
}
