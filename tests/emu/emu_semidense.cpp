// emu_semidense.cpp — TEST INFRASTRUCTURE: the kernel of csrc/semidense_device.hpp on CPU threads (hip_emu.h), with the launch
// geometry the product's launcher uses (sd_plan; grid = column segments x rows, SD_NT threads), before any GPU sees it.
//   emu_semidense <w> <h> <stride> <hw> <hh> <d_min> <d_max> <g_min> <thres_best> <thres_peak> <peak_px> <edge_px> <eps_edge>
//                 <eps_epi> <bf> <left.raw> <right.raw> <mask.raw | -> <out.raw>
// left.raw / right.raw: h rows of `stride` bytes; mask.raw: w x h bytes (0 = ignore), "-": none; out.raw: disparity, score,
// sigma_invd (w x h floats each), status (w x h bytes), the sum of the workgroups' counts of accepted pixels (one int).
#include "hip_emu.h"

#include <stdio.h>
#include <stdlib.h>

#include <vector>

// what semidense_device.hpp asks its includer for: the wavefront's cross-lane operations, through a scratch line per thread
static uint32_t emu_wave_u32[64 * 64];
static inline unsigned long long emu_ballot(bool p) {
  const int tid = (int)threadIdx.x, wave = tid >> 6;
  emu_wave_u32[tid] = p ? 1u : 0u;
  pthread_barrier_wait(&emu_wave_barrier[wave]);
  unsigned long long b = 0;
  for (int l = 0; l < 64; ++l) b |= (unsigned long long)emu_wave_u32[(wave << 6) + l] << l;
  pthread_barrier_wait(&emu_wave_barrier[wave]);
  return b;
}
static inline float emu_wave_max(float v) {
  const int tid = (int)threadIdx.x, wave = tid >> 6;
  emu_wave_u32[tid] = __float_as_uint(v);
  pthread_barrier_wait(&emu_wave_barrier[wave]);
  float m = __uint_as_float(emu_wave_u32[wave << 6]);
  for (int l = 1; l < 64; ++l) {
    const float o = __uint_as_float(emu_wave_u32[(wave << 6) + l]);
    m = o > m ? o : m;
  }
  pthread_barrier_wait(&emu_wave_barrier[wave]);
  return m;
}
static inline uint32_t emu_udot4(uint32_t a, uint32_t b, uint32_t c) {
  for (int k = 0; k < 4; ++k) c += ((a >> (8 * k)) & 255u) * ((b >> (8 * k)) & 255u);
  return c;
}
static uint8_t emu_sd_lds[64 * 1024] __attribute__((aligned(16)));
#define SD_DYN_LDS(name) uint8_t *name = emu_sd_lds
#define SD_BALLOT(p) emu_ballot((p))
#define SD_WAVE_MAX_F32(v) emu_wave_max((v))
#define SD_WAVE_SYNC() pthread_barrier_wait(&emu_wave_barrier[(int)threadIdx.x >> 6])
#define SD_UDOT4(a, b, c) emu_udot4((a), (b), (c))
#include "../../visual_odometry_ros_amd/csrc/semidense_device.hpp"

// the threads are started once and walk the grid together (as emu_zncc.cpp: two barrier waits between workgroups)
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
  if (argc < 20) return 2;
  const int w = atoi(argv[1]), h = atoi(argv[2]), stride = atoi(argv[3]);
  SdArgs a;
  memset(&a, 0, sizeof(a));
  a.hw = atoi(argv[4]);
  a.hh = atoi(argv[5]);
  a.d_min = atoi(argv[6]);
  a.d_max = atoi(argv[7]);
  const int g_min = atoi(argv[8]);
  a.g_min2 = g_min * g_min;
  a.thres_best = strtof(argv[9], nullptr);
  a.thres_peak = strtof(argv[10], nullptr);
  a.peak_px = atoi(argv[11]);
  a.edge_px = atoi(argv[12]);
  a.eps_edge = strtof(argv[13], nullptr);
  a.eps_epi = strtof(argv[14], nullptr);
  a.bf = strtof(argv[15], nullptr);
  if (w < 1 || h < 1 || stride < w || a.hw < 1 || a.hw > SD_MAX_HW || a.hh < 0 || a.hh > SD_MAX_HH || a.d_min < 0 || a.d_min > a.d_max ||
      a.d_max > SD_MAX_D)
    return 2;
  const size_t n = (size_t)w * h;
  std::vector<uint8_t> left((size_t)stride * h), right((size_t)stride * h), mask, status(n, 0xEE);
  std::vector<float> disp(n, -7.0f), score(n, -7.0f), sigma(n, -7.0f);
  if (!read_all(argv[16], left.data(), left.size()) || !read_all(argv[17], right.data(), right.size())) return 3;
  if (strcmp(argv[18], "-") != 0) {
    mask.resize(n);
    if (!read_all(argv[18], mask.data(), n)) return 3;
  }
  std::vector<int> wg((size_t)((w + SD_SEG - 1) / SD_SEG) * h, -1);
  a.L = left.data();
  a.R = right.data();
  a.strideL = a.strideR = stride;
  a.W = w;
  a.H = h;
  a.mask = mask.empty() ? nullptr : mask.data();
  a.mask_stride = w;
  a.disp = disp.data();
  a.score = score.data();
  a.sigma = sigma.data();
  a.status = status.data();
  a.wg_accepted = wg.data();
  sd_plan(&a);
  if (a.lds_bytes > (int)sizeof(emu_sd_lds)) return 2;
  emu_launch_pool(semidense_kernel, dim3((unsigned)((w + SD_SEG - 1) / SD_SEG), (unsigned)h, 1), dim3(SD_NT), a);
  FILE *f = fopen(argv[19], "wb");
  if (!f) return 3;
  fwrite(disp.data(), sizeof(float), n, f);
  fwrite(score.data(), sizeof(float), n, f);
  fwrite(sigma.data(), sizeof(float), n, f);
  fwrite(status.data(), 1, n, f);
  int accepted = 0;
  for (int v : wg) accepted += v;
  fwrite(&accepted, sizeof(int), 1, f);
  fclose(f);
  return 0;
}
