// emu_semidense_align_affine.cpp — TEST INFRASTRUCTURE: the kernel of the alignment with affine brightness
// (csrc/semidense_align_affine_device.hpp) and the map pyramid's (csrc/semidense_map_pyramid_device.hpp) on CPU threads (hip_emu.h),
// with the launches the product's launcher makes: one map pyramid launch per level, then per level from the top down its iterations'
// launches at that level's planes and grid, the first of a level taking over pose and brightness of the state block. levels = 1 is
// the level-0 operator.
//   emu_semidense_align_affine <w> <h> <pad> <levels> <min_obs> <huber> <eps> <min_pixels> <iters: 6 ints> <fx> <fy> <cx> <cy>
//                              <T_ck: 16 floats> <gain0> <offset0> <key.raw> <cur.raw> <map.raw> <out.raw>
// key.raw / cur.raw: the image's levels one behind the other, level l as h_l rows of w_l + pad bytes (the last without padding);
// map.raw: invd, sigma (w x h floats each), n_obs (w x h bytes); out.raw: T_ck (16 floats), status, iters, count, start_prev, G, O
// (int32), sum w r^2, sum w, H[36], b[8] (float64), per level 0..5 status, iters, count, launches (those that did not return at
// once), G, O (int32), per level sum w r^2, sum w (float64), per level the state block's T behind the level's launches (16 floats),
// the rows of partial sums behind the very first launch (blocks of the top level x 47 int64), then per level 1 .. levels - 1 the
// map's invd, sigma (floats) and n_obs (bytes). Every buffer is allocated with exactly the bytes it holds, so that an address
// sanitizer build sees any access outside an image or a plane.
#include "hip_emu.h"

#include <stdio.h>
#include <stdlib.h>

#include <memory>
#include <vector>

static inline int sda_wave_rank(bool p, int *n) { return orb_wave_rank(p, n); }
#define SDA_DRAIN() __atomic_thread_fence(__ATOMIC_SEQ_CST)
#define SDA_ST_AGENT(p, v) __atomic_store_n((p), (v), __ATOMIC_SEQ_CST)
#define SDA_ATOMIC_ADD_AGENT(p, v) __atomic_fetch_add((p), (v), __ATOMIC_SEQ_CST)
#define SDA_FENCE_RELEASE() __atomic_thread_fence(__ATOMIC_SEQ_CST)
#define SDA_FENCE_ACQUIRE() __atomic_thread_fence(__ATOMIC_SEQ_CST)
#include "../../visual_odometry_ros_amd/csrc/semidense_align_affine_device.hpp"
#include "../../visual_odometry_ros_amd/csrc/semidense_map_pyramid_device.hpp"

static bool read_all(FILE *f, void *dst, size_t bytes) { return f && fread(dst, 1, bytes, f) == bytes; }

int main(int argc, char **argv) {
  if (argc < 41) return 2;
  const int w0 = atoi(argv[1]), h0 = atoi(argv[2]), pad = atoi(argv[3]), L = atoi(argv[4]);
  SdaaArgs aa;
  memset(&aa, 0, sizeof(aa));
  SdaArgs &a = aa.a;
  sda_params(&a, atoi(argv[5]), strtof(argv[6], nullptr), 1, strtof(argv[7], nullptr), atoi(argv[8]));
  int iters[SDA_MAX_LEVELS];
  for (int l = 0; l < SDA_MAX_LEVELS; ++l) iters[l] = atoi(argv[9 + l]);
  const float K[4] = {strtof(argv[15], nullptr), strtof(argv[16], nullptr), strtof(argv[17], nullptr), strtof(argv[18], nullptr)};
  for (int i = 0; i < 12; ++i) a.T0[i] = strtof(argv[19 + i], nullptr);
  sdaa_params(&aa, strtof(argv[35], nullptr), strtof(argv[36], nullptr));
  if (L < 1 || L > SDA_MAX_LEVELS || pad < 0) return 2;
  int w[SDA_MAX_LEVELS], h[SDA_MAX_LEVELS];
  for (int l = 0; l < L; ++l) {
    w[l] = l ? (w[l - 1] + 1) / 2 : w0;
    h[l] = l ? (h[l - 1] + 1) / 2 : h0;
    if (w[l] < 3 || h[l] < 3 || iters[l] < 1 || iters[l] > SDA_MAX_ITERS) return 2;
  }
  std::unique_ptr<uint8_t[]> key[SDA_MAX_LEVELS], cur[SDA_MAX_LEVELS], n_obs[SDA_MAX_LEVELS];
  std::unique_ptr<float[]> invd[SDA_MAX_LEVELS], sigma[SDA_MAX_LEVELS];
  FILE *fk = fopen(argv[37], "rb"), *fc = fopen(argv[38], "rb"), *fm = fopen(argv[39], "rb");
  bool ok = true;
  for (int l = 0; l < L; ++l) {
    const size_t n = (size_t)w[l] * h[l], nimg = (size_t)(w[l] + pad) * (h[l] - 1) + w[l];  // (the last row has no padding: exact)
    key[l].reset(new uint8_t[nimg]);
    cur[l].reset(new uint8_t[nimg]);
    invd[l].reset(new float[n]);
    sigma[l].reset(new float[n]);
    n_obs[l].reset(new uint8_t[n]);
    ok = ok && read_all(fk, key[l].get(), nimg) && read_all(fc, cur[l].get(), nimg);
    if (l) {  // (every coarse pixel is written before it is read)
      memset(invd[l].get(), 0xEE, 4 * n);
      memset(sigma[l].get(), 0xEE, 4 * n);
      memset(n_obs[l].get(), 0xEE, n);
    }
  }
  const size_t n0 = (size_t)w0 * h0;
  ok = ok && read_all(fm, invd[0].get(), 4 * n0) && read_all(fm, sigma[0].get(), 4 * n0) && read_all(fm, n_obs[0].get(), n0);
  for (FILE *f : {fk, fc, fm})
    if (f) fclose(f);
  if (!ok) return 3;
  // ---- the map pyramid: one launch per level ------------------------------------------------------------------------------------------
  for (int l = 1; l < L; ++l) {
    SdmArgs m;
    m.invd = invd[l - 1].get(), m.sigma = sigma[l - 1].get(), m.n_obs = n_obs[l - 1].get();
    m.w = w[l - 1], m.h = h[l - 1];
    m.o_invd = invd[l].get(), m.o_sigma = sigma[l].get(), m.o_n_obs = n_obs[l].get();
    m.wc = w[l], m.hc = h[l];
    const size_t nc = (size_t)w[l] * h[l];
    emu_launch(semidense_map_pyramid_kernel, dim3((unsigned)((nc + SDM_NT - 1) / SDM_NT)), dim3(SDM_NT), m);
  }
  // ---- the levels, from the top down ----------------------------------------------------------------------------------------------------
  const size_t max_blocks = (n0 + SDA_BLOCK - 1) / SDA_BLOCK;
  std::unique_ptr<long long[]> partial(new long long[max_blocks * SDAA_NSUM]);
  for (size_t i = 0; i < max_blocks * SDAA_NSUM; ++i) partial[i] = 0x7EEEEEEEEEEEEEEELL;  // (every row is written before it is read)
  a.partial = partial.get();
  std::unique_ptr<SdaaState> st(new SdaaState);
  memset(st.get(), 0xEE, sizeof(SdaaState));  // (the first launch overwrites whatever the block holds ...)
  st->ticket = 0;                             // (... but for the ticket, which is zero between launches)
  aa.st = st.get();
  int launches[SDA_MAX_LEVELS] = {};
  float T_level[SDA_MAX_LEVELS][16] = {};
  std::vector<long long> first_sums;
  for (int l = L - 1; l >= 0; --l) {
    const float s = 1.0f / (float)(1 << l);
    a.Lk = key[l].get();
    a.Lc = cur[l].get();
    a.strideK = a.strideC = w[l] + pad;
    a.W = w[l];
    a.H = h[l];
    a.invd = invd[l].get(), a.sigma = sigma[l].get(), a.n_obs = n_obs[l].get();
    a.fx = K[0] * s, a.fy = K[1] * s, a.cx = K[2] * s, a.cy = K[3] * s;
    a.n_blocks = (int)(((size_t)a.W * a.H + SDA_BLOCK - 1) / SDA_BLOCK);
    a.level = l;
    a.max_iters = iters[l];
    for (int it = 0; it < a.max_iters; ++it) {
      a.first = it > 0 ? 0 : (l == L - 1 ? SDA_FIRST_CALL : SDA_FIRST_LEVEL);
      launches[l] += (!a.first && st->done) ? 0 : 1;
      emu_launch(semidense_affine_kernel, dim3((unsigned)a.n_blocks), dim3(SDA_NT), aa);
      if (st->ticket != 0) return 4;  // (back to zero behind every launch)
      if (l == L - 1 && it == 0) first_sums.assign(partial.get(), partial.get() + (size_t)a.n_blocks * SDAA_NSUM);
    }
    memcpy(T_level[l], st->T, sizeof(st->T));
  }
  FILE *f = fopen(argv[40], "wb");
  if (!f) return 3;
  fwrite(st->T, 4, 16, f);
  const int32_t ints[6] = {st->status, st->iters, st->count, st->start_prev, st->G, st->O};
  fwrite(ints, 4, 6, f);
  fwrite(&st->swrr, 8, 1, f);
  fwrite(&st->sw, 8, 1, f);
  fwrite(st->H, 8, 36, f);
  fwrite(st->b, 8, 8, f);
  for (int l = 0; l < SDA_MAX_LEVELS; ++l) {
    const int32_t v[6] = {l < L ? st->lv[l].status : -1, l < L ? st->lv[l].iters : -1, l < L ? st->lv[l].count : -1, launches[l],
                          l < L ? st->lv[l].G : -1,      l < L ? st->lv[l].O : -1};
    fwrite(v, 4, 6, f);
  }
  for (int l = 0; l < SDA_MAX_LEVELS; ++l) {
    const double v[2] = {l < L ? st->lv[l].swrr : 0.0, l < L ? st->lv[l].sw : 0.0};
    fwrite(v, 8, 2, f);
  }
  fwrite(T_level, 4, SDA_MAX_LEVELS * 16, f);
  fwrite(first_sums.data(), 8, first_sums.size(), f);
  for (int l = 1; l < L; ++l) {
    const size_t n = (size_t)w[l] * h[l];
    fwrite(invd[l].get(), 4, n, f);
    fwrite(sigma[l].get(), 4, n, f);
    fwrite(n_obs[l].get(), 1, n, f);
  }
  fclose(f);
  return 0;
}
