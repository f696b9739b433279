// emu_orb_mask.cpp — TEST INFRASTRUCTURE: emu_orb.cpp's run of csrc/orb_tile.hpp's two kernels with an ignore mask in the
// finishing kernel's argument block (OrbFinishArgs::mask): the vote with a mask on CPU threads, before any GPU sees it.
//   emu_orb_mask <emu_orb's arguments ...> <mask.raw>      (mask.raw: w x h bytes, 0 = ignore)
// The set-up is emu_orb.cpp's own, included below with its main() renamed and its launch of orb_finish_kernel routed through
// a wrapper that fills in the mask. This relies on emu_orb.cpp naming orb_finish_kernel at its launch ONLY (the macro below renames
// every use in that file) and on its main() taking the arguments by position from the front: keep both when emu_orb.cpp changes.
#include "hip_emu.h"

#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "../../visual_odometry_ros_amd/csrc/orb_tile.hpp"

static vo_mask_view g_mask = {nullptr, 0, 0, 0};
__global__ void orb_finish_kernel_with_mask(OrbFinishArgs a) {
  a.mask = g_mask;
  orb_finish_kernel(a);
}

#define orb_finish_kernel orb_finish_kernel_with_mask
#define main emu_orb_main
#include "emu_orb.cpp"
#undef main
#undef orb_finish_kernel

int main(int argc, char **argv) {
  if (argc < 15) return 2;
  const int w = atoi(argv[1]), h = atoi(argv[2]);
  std::vector<uint8_t> mask((size_t)w * h);
  FILE *f = fopen(argv[argc - 1], "rb");
  if (!f || fread(mask.data(), 1, mask.size(), f) != mask.size()) return 3;
  fclose(f);
  g_mask = {mask.data(), w, w, h};
  return emu_orb_main(argc - 1, argv);
}
