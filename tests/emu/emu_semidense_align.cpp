// emu_semidense_align.cpp — TEST INFRASTRUCTURE: the kernel of csrc/semidense_align_device.hpp on CPU threads (hip_emu.h), with the
// launch geometry the product's launcher uses (one workgroup of SDA_NT threads per block of SDA_BLOCK raster indices, one launch
// per iteration, the last workgroup by ticket solving and updating), before any GPU sees it.
//   emu_semidense_align <w> <h> <stride> <min_obs> <huber> <max_iters> <eps> <min_pixels> <fx> <fy> <cx> <cy> <T_ck: 16 floats>
//                       <key.raw> <cur.raw> <map.raw> <out.raw>
// key.raw / cur.raw: h rows of `stride` bytes (the last without padding); map.raw: invd, sigma (w x h floats each), n_obs (w x h
// bytes); out.raw: T_ck (16 floats), status, iters, count (int32), sum w r^2, sum w, H[21], b[6] (float64), launches (int32: those
// that did not return at once). Every buffer is allocated with exactly the bytes it holds, so that an address sanitizer build sees
// any read outside an image or a plane.
#include "hip_emu.h"

#include <stdio.h>
#include <stdlib.h>

#include <memory>

static inline int sda_wave_rank(bool p, int *n) { return orb_wave_rank(p, n); }
#define SDA_DRAIN() __atomic_thread_fence(__ATOMIC_SEQ_CST)
#define SDA_ST_AGENT(p, v) __atomic_store_n((p), (v), __ATOMIC_SEQ_CST)
#define SDA_ATOMIC_ADD_AGENT(p, v) __atomic_fetch_add((p), (v), __ATOMIC_SEQ_CST)
#define SDA_FENCE_RELEASE() __atomic_thread_fence(__ATOMIC_SEQ_CST)
#define SDA_FENCE_ACQUIRE() __atomic_thread_fence(__ATOMIC_SEQ_CST)
#include "../../visual_odometry_ros_amd/csrc/semidense_align_device.hpp"

static bool read_all(FILE *f, void *dst, size_t bytes) { return f && fread(dst, 1, bytes, f) == bytes; }
static bool read_file(const char *path, void *dst, size_t bytes) {
  FILE *f = fopen(path, "rb");
  const bool ok = read_all(f, dst, bytes);
  if (f) fclose(f);
  return ok;
}

int main(int argc, char **argv) {
  if (argc < 33) return 2;
  const int w = atoi(argv[1]), h = atoi(argv[2]), stride = atoi(argv[3]);
  SdaArgs a;
  memset(&a, 0, sizeof(a));
  sda_params(&a, atoi(argv[4]), strtof(argv[5], nullptr), atoi(argv[6]), strtof(argv[7], nullptr), atoi(argv[8]));
  a.fx = strtof(argv[9], nullptr);
  a.fy = strtof(argv[10], nullptr);
  a.cx = strtof(argv[11], nullptr);
  a.cy = strtof(argv[12], nullptr);
  float T[16];
  for (int i = 0; i < 16; ++i) T[i] = strtof(argv[13 + i], nullptr);
  if (w < 3 || h < 3 || stride < w || a.max_iters < 1 || a.max_iters > SDA_MAX_ITERS) return 2;
  const size_t n = (size_t)w * h, nimg = (size_t)stride * (h - 1) + w;  // (the last row has no padding: exact)
  std::unique_ptr<uint8_t[]> key(new uint8_t[nimg]), cur(new uint8_t[nimg]), n_obs(new uint8_t[n]);
  std::unique_ptr<float[]> invd(new float[n]), sigma(new float[n]);
  if (!read_file(argv[29], key.get(), nimg) || !read_file(argv[30], cur.get(), nimg)) return 3;
  FILE *fm = fopen(argv[31], "rb");
  const bool ok = read_all(fm, invd.get(), 4 * n) && read_all(fm, sigma.get(), 4 * n) && read_all(fm, n_obs.get(), n);
  if (fm) fclose(fm);
  if (!ok) return 3;
  a.Lk = key.get();
  a.Lc = cur.get();
  a.strideK = a.strideC = stride;
  a.W = w;
  a.H = h;
  a.invd = invd.get();
  a.sigma = sigma.get();
  a.n_obs = n_obs.get();
  a.n_blocks = (int)((n + SDA_BLOCK - 1) / SDA_BLOCK);
  std::unique_ptr<long long[]> partial(new long long[(size_t)a.n_blocks * SDA_NSUM]);
  for (size_t i = 0; i < (size_t)a.n_blocks * SDA_NSUM; ++i) partial[i] = 0x7EEEEEEEEEEEEEEELL;  // (every row is written before it is read)
  a.partial = partial.get();
  std::unique_ptr<SdaState> st(new SdaState);
  memset(st.get(), 0xEE, sizeof(SdaState));  // (the first launch overwrites whatever the block holds ...)
  st->ticket = 0;                            // (... but for the ticket, which is zero between launches)
  a.st = st.get();
  for (int i = 0; i < 12; ++i) a.T0[i] = T[i];
  int launches = 0;
  for (int it = 0; it < a.max_iters; ++it) {  // the product enqueues max_iters launches back to back
    a.first = it == 0;
    launches += (!a.first && st->done) ? 0 : 1;
    emu_launch(semidense_align_kernel, dim3((unsigned)a.n_blocks), dim3(SDA_NT), a);
    if (st->ticket != 0) return 4;  // (back to zero behind every launch)
  }
  FILE *f = fopen(argv[32], "wb");
  if (!f) return 3;
  fwrite(st->T, 4, 16, f);
  const int32_t ints[3] = {st->status, st->iters, st->count};
  fwrite(ints, 4, 3, f);
  fwrite(&st->swrr, 8, 1, f);
  fwrite(&st->sw, 8, 1, f);
  fwrite(st->H, 8, 21, f);
  fwrite(st->b, 8, 6, f);
  const int32_t l = launches;
  fwrite(&l, 4, 1, f);
  fclose(f);
  return 0;
}
