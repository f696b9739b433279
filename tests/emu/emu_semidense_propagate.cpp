// emu_semidense_propagate.cpp — TEST INFRASTRUCTURE: the kernels of csrc/semidense_propagate_device.hpp on CPU threads (hip_emu.h),
// with the launch geometry the product's launcher uses (ceil(W H / SDP_NT) workgroups of SDP_NT threads, the scatter, then the
// resolve), before any GPU sees them. hip_emu.h's atomicMax template serves the 64-bit keys.
//   emu_semidense_propagate <w> <h> <stride> <min_obs> <max_diff> <chi> <sigma_add> <bf> <fx> <fy> <cx> <cy> <T_ba: 16 floats>
//                           <old.raw> <key.raw> <new.raw> <mask.raw | -> <static.raw> <out.raw>
// old.raw: invd, sigma (w x h floats each), n_obs (w x h bytes); key.raw / new.raw: h rows of `stride` bytes (the last without
// padding); mask.raw: w x h bytes (0 = ignore), "-": none; static.raw: disparity, sigma_invd (floats), status (bytes); out.raw:
// invd, sigma (floats), src (int32), n_obs, tstatus, origin (bytes), then one byte: 1 where the plane of keys came back all 0.
// Every buffer is allocated with exactly the bytes it holds, so that an address sanitizer build sees any access outside one.
#include "hip_emu.h"

#include <stdio.h>
#include <stdlib.h>

#include <memory>

#include "../../visual_odometry_ros_amd/csrc/semidense_propagate_device.hpp"

// the threads are started once and walk the grid together (as emu_semidense_temporal.cpp: two barrier waits between workgroups)
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
  if (argc < 35) return 2;
  const int w = atoi(argv[1]), h = atoi(argv[2]), stride = atoi(argv[3]);
  SdpArgs a;
  memset(&a, 0, sizeof(a));
  a.min_obs = atoi(argv[4]);
  a.max_diff = atoi(argv[5]);
  const float chi = strtof(argv[6], nullptr), sigma_add = strtof(argv[7], nullptr);
  a.chi2 = chi * chi;
  a.sigma_add2 = sigma_add * sigma_add;
  a.bf = strtof(argv[8], nullptr);
  a.fx = strtof(argv[9], nullptr);
  a.fy = strtof(argv[10], nullptr);
  a.cx = strtof(argv[11], nullptr);
  a.cy = strtof(argv[12], nullptr);
  float T[16];
  for (int i = 0; i < 16; ++i) T[i] = strtof(argv[13 + i], nullptr);
  sdp_pose(&a, T);
  if (w < 3 || h < 3 || stride < w) return 2;
  const size_t n = (size_t)w * h, nimg = (size_t)stride * (h - 1) + w;  // (the last row has no padding: exact)
  std::unique_ptr<uint8_t[]> key(new uint8_t[nimg]), cur(new uint8_t[nimg]), mask, no_a(new uint8_t[n]), status(new uint8_t[n]);
  std::unique_ptr<uint8_t[]> n_obs(new uint8_t[n]), tstatus(new uint8_t[n]), origin(new uint8_t[n]);
  std::unique_ptr<float[]> invd_a(new float[n]), sigma_a(new float[n]), disp(new float[n]), sg(new float[n]), invd(new float[n]), sigma(new float[n]);
  std::unique_ptr<int32_t[]> src(new int32_t[n]);
  std::unique_ptr<unsigned long long[]> keys(new unsigned long long[n]);
  FILE *fo = fopen(argv[29], "rb");
  bool ok = read_all(fo, invd_a.get(), 4 * n) && read_all(fo, sigma_a.get(), 4 * n) && read_all(fo, no_a.get(), n);
  if (fo) fclose(fo);
  if (!ok || !read_file(argv[30], key.get(), nimg) || !read_file(argv[31], cur.get(), nimg)) return 3;
  if (strcmp(argv[32], "-") != 0) {
    mask.reset(new uint8_t[n]);
    if (!read_file(argv[32], mask.get(), n)) return 3;
  }
  FILE *fs = fopen(argv[33], "rb");
  ok = read_all(fs, disp.get(), 4 * n) && read_all(fs, sg.get(), 4 * n) && read_all(fs, status.get(), n);
  if (fs) fclose(fs);
  if (!ok) return 3;
  for (size_t i = 0; i < n; ++i) keys[i] = 0, invd[i] = sigma[i] = -7.0f, src[i] = -7, n_obs[i] = tstatus[i] = origin[i] = 0x5A;
  a.invd_a = invd_a.get();
  a.sigma_a = sigma_a.get();
  a.n_obs_a = no_a.get();
  a.La = key.get();
  a.Lb = cur.get();
  a.strideA = a.strideB = stride;
  a.W = w;
  a.H = h;
  a.mask = mask.get();
  a.mask_stride = w;
  a.keys = keys.get();
  a.disp = disp.get();
  a.sigma_invd = sg.get();
  a.status = status.get();
  a.invd = invd.get();
  a.sigma = sigma.get();
  a.n_obs = n_obs.get();
  a.tstatus = tstatus.get();
  a.origin = origin.get();
  a.src = src.get();
  const dim3 grid((unsigned)((n + SDP_NT - 1) / SDP_NT), 1, 1);
  emu_launch_pool(semidense_propagate_scatter_kernel, grid, dim3(SDP_NT), a);
  emu_launch_pool(semidense_propagate_resolve_kernel, grid, dim3(SDP_NT), a);
  uint8_t clean = 1;
  for (size_t i = 0; i < n; ++i) clean = clean && keys[i] == 0;
  FILE *f = fopen(argv[34], "wb");
  if (!f) return 3;
  fwrite(invd.get(), 4, n, f);
  fwrite(sigma.get(), 4, n, f);
  fwrite(src.get(), 4, n, f);
  fwrite(n_obs.get(), 1, n, f);
  fwrite(tstatus.get(), 1, n, f);
  fwrite(origin.get(), 1, n, f);
  fwrite(&clean, 1, 1, f);
  fclose(f);
  return 0;
}
