// emu_mono_debug.cpp — TEST INFRASTRUCTURE ONLY. csrc/mono_debug_device.hpp compiled by g++ (-ffp-contract=off) and driven as
// mvo_debug_gather_kernel drives it: blocks of 256 lanes over max(n, 1) features, one lane per feature.
//   in : int n, need_five_point | float K[4], dT01[16] | u8 stage[n], ba_ok[n] | float pts1[2n], Xp[3n]
//   out: int ctl[MVO_DBG_WORDS] | float pts_ba[2n], pts_proj[2n] | u8 valid[n]   — every byte preset to 0xA5, so that what the
//        gather did not write shows. The output arrays hold exactly n entries: a lane past n that wrote would be out of bounds.
#include "hip_emu.h"

#include <stdio.h>

#include "../../visual_odometry_ros_amd/csrc/mono_debug_device.hpp"

__global__ __launch_bounds__(256) void mvo_debug_gather_kernel(MonoDbgArgs a) { mono_dbg_gather(a, (int)(blockIdx.x * blockDim.x + threadIdx.x)); }

int main(int argc, char **argv) {
  if (argc != 3) return 2;
  FILE *f = fopen(argv[1], "rb");
  if (!f) return 2;
  int hd[2];
  float K[4], dT[16];
  if (fread(hd, sizeof(int), 2, f) != 2 || fread(K, sizeof(float), 4, f) != 4 || fread(dT, sizeof(float), 16, f) != 16) return 3;
  const int n = hd[0], need = hd[1];
  if (n < 0 || n > (1 << 20)) return 3;
  std::vector<uint8_t> stage((size_t)n), ba_ok((size_t)n), valid((size_t)n, 0xA5);
  std::vector<float> pts1(2 * (size_t)n), Xp(3 * (size_t)n), pts_ba(2 * (size_t)n), pts_proj(2 * (size_t)n);
  if (n > 0 &&  // (an empty vector's data() may be null)
      (fread(stage.data(), 1, stage.size(), f) != stage.size() || fread(ba_ok.data(), 1, ba_ok.size(), f) != ba_ok.size() ||
      fread(pts1.data(), sizeof(float), pts1.size(), f) != pts1.size() || fread(Xp.data(), sizeof(float), Xp.size(), f) != Xp.size()))
    return 3;
  fclose(f);
  int ctl[MVO_DBG_WORDS];
  memset(ctl, 0xA5, sizeof(ctl));
  if (n) {
    memset(pts_ba.data(), 0xA5, sizeof(float) * pts_ba.size());
    memset(pts_proj.data(), 0xA5, sizeof(float) * pts_proj.size());
  }
  MonoDbgArgs a;
  memset(&a, 0, sizeof(a));
  a.n = n;
  a.stage = stage.data();
  a.ba_ok = ba_ok.data();
  a.pts1 = pts1.data();
  a.Xp = Xp.data();
  a.dT01 = dT;
  a.need_five_point = &need;
  memcpy(a.K, K, sizeof(K));
  a.ctl = ctl;
  a.pts_ba = pts_ba.data();
  a.pts_proj = pts_proj.data();
  a.valid = valid.data();
  const int lanes = n > 0 ? n : 1;
  emu_launch(mvo_debug_gather_kernel, dim3((unsigned)((lanes + 255) / 256)), dim3(256), a);
  FILE *o = fopen(argv[2], "wb");
  if (!o) return 4;
  fwrite(ctl, sizeof(int), MVO_DBG_WORDS, o);
  if (n > 0) {
    fwrite(pts_ba.data(), sizeof(float), pts_ba.size(), o);
    fwrite(pts_proj.data(), sizeof(float), pts_proj.size(), o);
    fwrite(valid.data(), 1, valid.size(), o);
  }
  fclose(o);
  return 0;
}
