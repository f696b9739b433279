// emu_dense_stereo.cpp — TEST INFRASTRUCTURE: the kernels of csrc/dense_stereo_device.hpp on CPU threads (hip_emu.h), with the launch
// geometry the product's launcher uses (census: a thread per pixel, both planes in one grid; aggregation: one launch per direction, a
// wavefront per path; decision: DS_PIX pixels per wavefront), before any GPU sees it.
//   emu_dense_stereo <reverse> <cpus> <w> <h> <stride> <d_min> <n_disp> <paths> <p1> <p2> <uniqueness> <lr_max> <eps_d> <bf>
//                    <left.raw> <right.raw> <mask.raw | -> <out.raw>
// reverse: 1 walks the workgroups of every launch from the last to the first; cpus > 0: the process is confined to that many CPUs.
// left.raw / right.raw: h rows of `stride` bytes, the last without its padding; mask.raw: w x h bytes (0 = ignore), "-": none;
// out.raw: disparity (w x h floats), cost (w x h u16), sigma_invd (w x h floats), status (w x h bytes). Every buffer is allocated
// with exactly the bytes it holds, so that an address sanitizer build sees any access outside one.
#ifndef _GNU_SOURCE
#define _GNU_SOURCE
#endif
#include "hip_emu.h"

#include <sched.h>
#include <stdio.h>
#include <stdlib.h>

#include <memory>

// what dense_stereo_device.hpp asks its includer for: the wavefront's cross-lane operations, through a scratch line per thread. The
// lines are double-buffered — every lane of a wavefront goes through the same sequence of operations, so a lane that is one
// operation ahead writes the other set — which leaves one barrier wait per operation.
static unsigned emu_ds_a[2][256];
static int emu_ds_lo[2][256], emu_ds_hi[2][256];
static thread_local unsigned emu_ds_ops;  // (threads are started per launch: 0 at a kernel's start)
static inline unsigned emu_wave_min_u32(unsigned v) {
  const int tid = (int)threadIdx.x, wave = tid >> 6;
  const unsigned p = emu_ds_ops++ & 1u;
  emu_ds_a[p][tid] = v;
  pthread_barrier_wait(&emu_wave_barrier[wave]);
  unsigned m = emu_ds_a[p][wave << 6];
  for (int l = 1; l < 64; ++l) m = emu_ds_a[p][(wave << 6) + l] < m ? emu_ds_a[p][(wave << 6) + l] : m;
  return m;
}
static inline void emu_wave_step(int m, int lo, int hi, int &mn, int &up, int &dn) {
  const int tid = (int)threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const unsigned p = emu_ds_ops++ & 1u;
  emu_ds_a[p][tid] = (unsigned)m;
  emu_ds_lo[p][tid] = lo;
  emu_ds_hi[p][tid] = hi;
  pthread_barrier_wait(&emu_wave_barrier[wave]);
  unsigned r = emu_ds_a[p][wave << 6];
  for (int l = 1; l < 64; ++l) r = emu_ds_a[p][(wave << 6) + l] < r ? emu_ds_a[p][(wave << 6) + l] : r;
  mn = (int)r;
  up = lane > 0 ? emu_ds_lo[p][tid - 1] : lo;
  dn = lane < 63 ? emu_ds_hi[p][tid + 1] : hi;
}
#define DS_WAVE_MIN_U32(v) emu_wave_min_u32((v))
#define DS_WAVE_STEP(m, lo, hi, mn, up, dn) emu_wave_step((m), (lo), (hi), (mn), (up), (dn))
#define DS_POPC64(v) __builtin_popcountll((v))
#include "../../visual_odometry_ros_amd/csrc/dense_stereo_device.hpp"

// the threads are started once per launch and walk the grid together (as emu_semidense_world.cpp), forward or backward
template <class Kernel, class... Args>
static void emu_launch_pool(Kernel k, dim3 grid, dim3 block, bool reverse, Args... args) {
  gridDim = grid;
  blockDim = block;
  const unsigned nt = block.x;
  pthread_barrier_init(&emu_block_barrier, nullptr, nt);
  for (unsigned w = 0; w < nt / 64; ++w) pthread_barrier_init(&emu_wave_barrier[w], nullptr, 64);
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
  for (unsigned w = 0; w < nt / 64; ++w) pthread_barrier_destroy(&emu_wave_barrier[w]);
}

static bool read_all(const char *path, void *dst, size_t bytes) {
  FILE *f = fopen(path, "rb");
  const bool ok = f && fread(dst, 1, bytes, f) == bytes;
  if (f) fclose(f);
  return ok;
}

template <int ND>
static void run(const DsAggArgs &agg, int paths, const DsDecideArgs &dec, bool reverse) {
  static const int dirs[8][2] = {{1, 0}, {-1, 0}, {0, 1}, {0, -1}, {1, 1}, {-1, -1}, {1, -1}, {-1, 1}};
  for (int r = 0; r < paths; ++r) {
    DsAggArgs a = agg;
    a.dx = dirs[r][0];
    a.dy = dirs[r][1];
    a.n_paths = ds_path_count(a.W, a.H, a.dx, a.dy);
    a.first = r == 0;
    emu_launch_pool(dense_aggregate_kernel<ND>, dim3((unsigned)((a.n_paths + DS_AGG_NT / 64 - 1) / (DS_AGG_NT / 64))), dim3(DS_AGG_NT), reverse, a);
  }
  const size_t np = (size_t)dec.W * (size_t)dec.H, per_wg = (size_t)DS_PIX * (DS_NT / 64);
  emu_launch_pool(dense_decide_kernel<ND>, dim3((unsigned)((np + per_wg - 1) / per_wg)), dim3(DS_NT), reverse, dec);
}

int main(int argc, char **argv) {
  if (argc < 19) return 2;
  const int reverse = atoi(argv[1]), cpus = atoi(argv[2]);
  const int w = atoi(argv[3]), h = atoi(argv[4]), stride = atoi(argv[5]);
  const int d_min = atoi(argv[6]), n_disp = atoi(argv[7]), paths = atoi(argv[8]), p1 = atoi(argv[9]), p2 = atoi(argv[10]);
  const int uniqueness = atoi(argv[11]), lr_max = atoi(argv[12]);
  const float eps_d = strtof(argv[13], nullptr), bf = strtof(argv[14], nullptr);
  if (w < 1 || h < 1 || stride < w || d_min < 0 || (n_disp != 64 && n_disp != 128 && n_disp != 192 && n_disp != 256) || (paths != 4 && paths != 8) ||
      p1 < 0 || p1 >= p2 || p2 > 8129 || uniqueness < 0 || uniqueness > 99 || lr_max < -1)
    return 2;
  if (cpus > 0) {
    cpu_set_t have, want;
    CPU_ZERO(&want);
    if (sched_getaffinity(0, sizeof(have), &have) != 0) return 4;
    int n = 0;
    for (int i = 0; i < CPU_SETSIZE && n < cpus; ++i)
      if (CPU_ISSET(i, &have)) CPU_SET(i, &want), ++n;
    if (sched_setaffinity(0, sizeof(want), &want) != 0) return 4;
  }
  const size_t n = (size_t)w * h, nimg = (size_t)stride * (h - 1) + w;  // (the last row has no padding: exact)
  std::unique_ptr<uint8_t[]> left(new uint8_t[nimg]), right(new uint8_t[nimg]), mask, status(new uint8_t[n]);
  std::unique_ptr<float[]> disp(new float[n]), sigma(new float[n]);
  std::unique_ptr<uint16_t[]> cost(new uint16_t[n]), S(new uint16_t[n * (size_t)n_disp]);
  std::unique_ptr<unsigned long long[]> cenL(new unsigned long long[n]), cenR(new unsigned long long[n]);
  if (!read_all(argv[15], left.get(), nimg) || !read_all(argv[16], right.get(), nimg)) return 3;
  if (strcmp(argv[17], "-") != 0) {
    mask.reset(new uint8_t[n]);
    if (!read_all(argv[17], mask.get(), n)) return 3;
  }
  memset(status.get(), 0xEE, n);
  memset(cost.get(), 0xEE, n * sizeof(uint16_t));
  memset(S.get(), 0xEE, n * (size_t)n_disp * sizeof(uint16_t));
  for (size_t i = 0; i < n; ++i) disp[i] = sigma[i] = -7.0f;
  DsCensusArgs ca;
  memset(&ca, 0, sizeof(ca));
  ca.img0 = left.get();
  ca.img1 = right.get();
  ca.stride0 = ca.stride1 = stride;
  ca.W = w;
  ca.H = h;
  ca.cen0 = cenL.get();
  ca.cen1 = cenR.get();
  emu_launch_pool(dense_census_kernel, dim3((unsigned)((n + DS_NT - 1) / DS_NT), 2), dim3(DS_NT), reverse != 0, ca);
  DsAggArgs ag;
  memset(&ag, 0, sizeof(ag));
  ag.cenL = cenL.get();
  ag.cenR = cenR.get();
  ag.S = S.get();
  ag.W = w;
  ag.H = h;
  ag.d_min = d_min;
  ag.p1 = p1;
  ag.p2 = p2;
  DsDecideArgs de;
  memset(&de, 0, sizeof(de));
  de.S = S.get();
  de.W = w;
  de.H = h;
  de.d_min = d_min;
  de.uniqueness = uniqueness;
  de.lr_max = lr_max;
  de.sigma = eps_d / bf;
  de.mask = mask.get();
  de.mask_stride = w;
  de.disp = disp.get();
  de.cost = cost.get();
  de.sigma_out = sigma.get();
  de.status = status.get();
  switch (n_disp / 64) {
    case 1: run<1>(ag, paths, de, reverse != 0); break;
    case 2: run<2>(ag, paths, de, reverse != 0); break;
    case 3: run<3>(ag, paths, de, reverse != 0); break;
    default: run<4>(ag, paths, de, reverse != 0); break;
  }
  FILE *f = fopen(argv[18], "wb");
  if (!f) return 3;
  fwrite(disp.get(), sizeof(float), n, f);
  fwrite(cost.get(), sizeof(uint16_t), n, f);
  fwrite(sigma.get(), sizeof(float), n, f);
  fwrite(status.get(), 1, n, f);
  fclose(f);
  return 0;
}
