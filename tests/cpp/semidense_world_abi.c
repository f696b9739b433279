/* The world map's handle through the C ABI alone (include/vo_hip.h, "Semi-dense world map"): what needs no device is run — the
 * defaults, and every entry refusing a null handle — and every entry is linked (tests/test_semidense_world_cpp.py). */
#include <stdio.h>
#include <string.h>

#include "include/vo_hip.h"

int main(void) {
  vo_semidense_world_params p;
  memset(&p, 0xEE, sizeof(p));
  if (vo_semidense_world_default_params(&p) != VO_OK || vo_semidense_world_default_params(NULL) != VO_ERR_INVALID) return 1;
  if (p.voxel != 0.10f || p.capacity_log2 != 22 || p.min_obs != 2 || p.z_max != 40.0f) return 2;
  vo_semidense_world *wm = NULL;
  vo_semidense_world_info info;
  int n = -1;
  const float K[4] = {1, 1, 0, 0}, T[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
  float plane[1] = {0};
  uint8_t obs[1] = {0};
  if (vo_semidense_world_create(NULL, &p, &wm) != VO_ERR_INVALID || wm != NULL) return 3;
  if (vo_semidense_world_integrate(NULL, plane, plane, obs, NULL, 0, 0, 1, 1, 0, K, T) != VO_ERR_INVALID) return 4;
  if (vo_semidense_world_stats(NULL, &info) != VO_ERR_INVALID || vo_semidense_world_clear(NULL) != VO_ERR_INVALID) return 5;
  if (vo_semidense_world_points(NULL, 1, 1, 0, NULL, NULL, NULL, NULL, NULL, NULL, NULL, &n) != VO_ERR_INVALID) return 6;
  if (vo_svo_set_semidense_world(NULL, &p, VO_SEMIDENSE_WORLD_RAW) != VO_ERR_INVALID || vo_svo_semidense_world_flush(NULL) != VO_ERR_INVALID ||
      vo_svo_semidense_world_clear(NULL) != VO_ERR_INVALID || vo_svo_get_semidense_world_stats(NULL, &info) != VO_ERR_INVALID ||
      vo_svo_get_semidense_world_points(NULL, 1, 1, 0, NULL, NULL, NULL, NULL, NULL, NULL, &n) != VO_ERR_INVALID)
    return 7;
  vo_semidense_world_destroy(NULL);
  printf("semidense world abi ok\n");
  return 0;
}
