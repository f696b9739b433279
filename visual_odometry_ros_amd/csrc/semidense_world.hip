// semidense_world.hip — the world-frame voxel map that fuses the keyframes' semi-dense maps (include/vo_hip.h, "Semi-dense world
// map"): the handle (vo_semidense_world_create / _integrate / _points / _stats / _clear / _destroy) and StereoVO's hook
// (vo_svo_set_semidense_world, vo_svo_semidense_world_flush, vo_svo_get_semidense_world_points / _stats; the launch is placed by
// vo_svo_semidense_temporal_enqueue in front of whatever overwrites the outgoing keyframe's map), and the exact removal of an
// integration and the re-anchoring built on it (vo_semidense_world_remove / _reanchor / _reanchor_stats; "Semi-dense world map:
// removal and re-anchoring"), and the free-space carving (vo_semidense_world_carve / _carve_stats / _points_free,
// vo_svo_set_semidense_world_carve; "Semi-dense world map: free-space carving"). semidense_world_device.hpp and
// semidense_world_carve_device.hpp have the kernels.
#include "stereo_vo.hpp"
#include "vo_internal.hpp"
#include "vo_kernels.hpp"

#include <math.h>

#include <algorithm>
#include <vector>

#define SDW_DRAIN() asm volatile("s_waitcnt vmcnt(0)" ::: "memory")
#define SDW_ST_AGENT(p, v) __hip_atomic_store((p), (v), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)
#define SDW_ATOMIC_ADD_AGENT(p, v) __hip_atomic_fetch_add((p), (v), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)
// (the explicit wait behind either fence, as semidense_align.hip)
#define SDW_FENCE_RELEASE()                             \
  do {                                                  \
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");  \
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");    \
  } while (0)
#define SDW_FENCE_ACQUIRE()                             \
  do {                                                  \
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");  \
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");    \
  } while (0)
__device__ __forceinline__ unsigned long long sdw_cas64(unsigned long long *p, unsigned long long cmp, unsigned long long v) {
  return atomicCAS(p, cmp, v);
}
#include "semidense_world_carve_device.hpp"

static_assert(sizeof(SdwSlot) == 64, "a slot is 64 bytes");
static_assert(sizeof(SdwState) % 8 == 0, "the removal's 64-bit words behind SdwState are aligned");
static_assert(sizeof(SdwReanchorState) % 8 == 0, "the carve's 64-bit words behind SdwReanchorState are aligned");
static_assert(offsetof(SdwSlot, free) == 60, "free is the slot's last word");
#define SDW_STATE_BYTES (sizeof(SdwState) + sizeof(SdwReanchorState) + sizeof(SdwCarveState))

struct vo_semidense_world {
  vo_ctx *c = nullptr;
  vo_semidense_world_params prm = {};
  SdwSlot *slots = nullptr;
  SdwState *st = nullptr;
  SdwReanchorState *rs = nullptr;  // the removal's words, behind *st in the same allocation
  SdwCarveState *cs = nullptr;     // the carve's words, behind *rs
  unsigned long long reanchors = 0;  // vo_semidense_world_reanchor calls that enqueued their pair
  unsigned seq = 0;             // the sequence number of the last call, refused ones included
  SdwSlot *scratch = nullptr;   // the extraction's records (grows with the first getter that needs more)
  size_t scratch_cap = 0;
};

extern "C" int vo_semidense_world_default_params(vo_semidense_world_params *p) {
  if (!p) return VO_ERR_INVALID;
  memset(p, 0, sizeof(*p));
  p->voxel = 0.10f;
  p->capacity_log2 = 22;
  p->min_obs = 2;
  p->z_max = 40.0f;
  return VO_OK;
}

static int sdw_check_params(vo_ctx *c, const vo_semidense_world_params *p) {
  if (!(p->voxel > 0.0f) || !isfinite(p->voxel)) VO_FAIL(c, VO_ERR_INVALID, "semi-dense world map: voxel must be positive and finite");
  if (p->capacity_log2 < 10 || p->capacity_log2 > 28)
    VO_FAIL(c, VO_ERR_INVALID, "semi-dense world map: capacity_log2=%d: expected 10..28", p->capacity_log2);
  if (p->min_obs < 1 || p->min_obs > 255) VO_FAIL(c, VO_ERR_INVALID, "semi-dense world map: min_obs=%d: expected 1..255", p->min_obs);
  if (!(p->z_max > 0.0f) || !isfinite(p->z_max)) VO_FAIL(c, VO_ERR_INVALID, "semi-dense world map: z_max must be positive and finite");
  return VO_OK;
}

extern "C" int vo_semidense_world_create(vo_ctx *c, const vo_semidense_world_params *prm, vo_semidense_world **out) {
  if (!c || !prm || !out) return VO_ERR_INVALID;
  *out = nullptr;
  const int rc = sdw_check_params(c, prm);
  if (rc) return rc;
  VO_CHECK_HIP(c, hipSetDevice(c->device));
  vo_semidense_world *wm = new vo_semidense_world();
  wm->c = c;
  wm->prm = *prm;
  const size_t bytes = sizeof(SdwSlot) << prm->capacity_log2;
  void *base = nullptr;
  if (vo_dev_malloc(c, &base, bytes + SDW_STATE_BYTES) != hipSuccess) {
    delete wm;
    VO_FAIL(c, VO_ERR_HIP, "semi-dense world map: no device memory for 2^%d slots of 64 bytes", prm->capacity_log2);
  }
  wm->slots = (SdwSlot *)base;
  wm->st = (SdwState *)((char *)base + bytes);
  wm->rs = (SdwReanchorState *)((char *)base + bytes + sizeof(SdwState));
  wm->cs = (SdwCarveState *)((char *)base + bytes + sizeof(SdwState) + sizeof(SdwReanchorState));
  if (hipMemsetAsync(base, 0, bytes + SDW_STATE_BYTES, c->stream) != hipSuccess || hipStreamSynchronize(c->stream) != hipSuccess) {
    (void)hipFree(base);
    delete wm;
    VO_FAIL(c, VO_ERR_HIP, "semi-dense world map: the table could not be cleared");
  }
  *out = wm;
  return VO_OK;
}

extern "C" void vo_semidense_world_destroy(vo_semidense_world *wm) {
  if (!wm) return;
  (void)hipSetDevice(wm->c->device);
  if (wm->slots) (void)hipFree(wm->slots);
  if (wm->scratch) (void)hipFree(wm->scratch);
  delete wm;
}

static int sdw_clear(vo_semidense_world *wm, hipStream_t s) {
  vo_ctx *c = wm->c;
  VO_CHECK_HIP(c, hipMemsetAsync(wm->slots, 0, (sizeof(SdwSlot) << wm->prm.capacity_log2) + SDW_STATE_BYTES, s));
  wm->seq = 0;
  wm->reanchors = 0;
  return VO_OK;
}

extern "C" int vo_semidense_world_clear(vo_semidense_world *wm) {
  if (!wm) return VO_ERR_INVALID;
  vo_ctx *c = wm->c;
  VO_CHECK_HIP(c, hipSetDevice(c->device));
  const int rc = sdw_clear(wm, c->stream);
  if (rc) return rc;
  VO_CHECK_HIP(c, hipStreamSynchronize(c->stream));
  return VO_OK;
}

// ---- the launch -------------------------------------------------------------------------------------------------------------------
static int sdw_check_launch(vo_semidense_world *wm, const uint8_t *d_key, int key_stride, int W, int H, const float K[4], const float T_wk[16]) {
  vo_ctx *c = wm->c;
  if (W < 1 || H < 1 || W > 65535 || H > 65535 || (long long)W * H > 0x7FFFFFFFll)
    VO_FAIL(c, VO_ERR_SIZE, "semi-dense world map: the map must have 1 .. 65535 pixels a side and fewer than 2^31 in all");
  if (d_key && key_stride < W) VO_FAIL(c, VO_ERR_INVALID, "semi-dense world map: key_stride %d below the width %d", key_stride, W);
  if (!(K[0] > 0.0f) || !(K[1] > 0.0f) || !isfinite(K[0]) || !isfinite(K[1]) || !isfinite(K[2]) || !isfinite(K[3]))
    VO_FAIL(c, VO_ERR_INVALID, "semi-dense world map: fx, fy must be positive, K finite");
  for (int i = 0; i < 12; ++i)
    if (!isfinite(T_wk[i])) VO_FAIL(c, VO_ERR_INVALID, "semi-dense world map: T_wk is not finite");
  return VO_OK;
}

// On stream s, DEVICE planes throughout; d_key may be null. Every call that reaches the launch takes a sequence number. remove: the
// removal kernel instead of the integration.
static int sdw_enqueue(vo_semidense_world *wm, hipStream_t s, const float *invd, const float *sigma, const uint8_t *n_obs, const uint8_t *d_key,
                       int key_stride, int W, int H, const float K[4], const float T_wk[16], bool remove = false) {
  vo_ctx *c = wm->c;
  const int rc = sdw_check_launch(wm, d_key, key_stride, W, H, K, T_wk);
  if (rc) return rc;
  SdwArgs a;
  memset(&a, 0, sizeof(a));
  a.invd = invd;
  a.sigma = sigma;
  a.n_obs = n_obs;
  a.Lk = d_key;
  a.strideK = key_stride;
  a.W = W;
  a.H = H;
  a.min_obs = wm->prm.min_obs;
  a.z_max = wm->prm.z_max;
  a.voxel = wm->prm.voxel;
  a.fx = K[0], a.fy = K[1], a.cx = K[2], a.cy = K[3];
  memcpy(a.T, T_wk, sizeof(a.T));
  a.seq = ++wm->seq;
  a.capacity_log2 = wm->prm.capacity_log2;
  a.slots = wm->slots;
  a.st = wm->st;
  const unsigned nb = (unsigned)(((size_t)W * (size_t)H + SDW_BLOCK - 1) / SDW_BLOCK);
  hipStream_t keep = c->stream;
  c->stream = s;
  vo_prof_begin(c, VO_K_AUX);
  if (remove) {
    SdwRemoveArgs ra;
    ra.a = a;
    ra.rs = wm->rs;
    hipLaunchKernelGGL(semidense_world_remove_kernel, dim3(nb), dim3(SDW_NT), 0, s, ra);
  } else if (c->dbg[VO_DBG_SDW_FORM] == 1)
    hipLaunchKernelGGL(semidense_world_integrate_kernel<false>, dim3(nb), dim3(SDW_NT), 0, s, a);
  else
    hipLaunchKernelGGL(semidense_world_integrate_kernel<true>, dim3(nb), dim3(SDW_NT), 0, s, a);
  vo_prof_end(c);
  c->stream = keep;
  VO_CHECK_HIP(c, hipGetLastError());
  return VO_OK;
}

// the operator's calls: the planes to the device where they are the host's, then one launch (T_new null), or the removal with T and the
// integration with T_new behind it; synchronous
static int sdw_operator(vo_semidense_world *wm, const float *invd, const float *sigma, const uint8_t *n_obs, const uint8_t *key_plane,
                        int key_stride, int key_on_device, int width, int height, int on_device, const float K[4], const float T_wk[16],
                        bool remove, const float *T_new) {
  if (!wm || !invd || !sigma || !n_obs || !K || !T_wk || width <= 0 || height <= 0) return VO_ERR_INVALID;
  vo_ctx *c = wm->c;
  if (width > c->cfg.max_width || height > c->cfg.max_height)
    VO_FAIL(c, VO_ERR_SIZE, "%d x %d planes exceed vo_config.max_width x max_height", width, height);
  if (key_plane && key_stride < width) VO_FAIL(c, VO_ERR_INVALID, "semi-dense world map: key_stride %d below the width %d", key_stride, width);
  VO_CHECK_HIP(c, hipSetDevice(c->device));
  hipStream_t s = c->stream;
  const int W = width, H = height;
  const size_t np = (size_t)W * (size_t)H;
  vo_sdt_buffers *b = nullptr;  // the map's and the key plane's device copies
  if ((key_plane && !key_on_device) || !on_device) {
    const int rc = vo_sdt_ctx_buffers(c, &b);
    if (rc) return rc;
  }
  const uint8_t *d_key = key_plane;
  int d_stride = key_stride;
  if (key_plane && !key_on_device) {
    VO_CHECK_HIP(c, hipMemcpy2DAsync(b->key, (size_t)W, key_plane, (size_t)key_stride, (size_t)W, (size_t)H, hipMemcpyHostToDevice, s));
    d_key = b->key;
    d_stride = W;
  }
  const float *d_invd = invd, *d_sigma = sigma;
  const uint8_t *d_no = n_obs;
  if (!on_device) {
    VO_CHECK_HIP(c, hipMemcpyAsync(b->invd, invd, np * sizeof(float), hipMemcpyHostToDevice, s));
    VO_CHECK_HIP(c, hipMemcpyAsync(b->sigma, sigma, np * sizeof(float), hipMemcpyHostToDevice, s));
    VO_CHECK_HIP(c, hipMemcpyAsync(b->n_obs, n_obs, np, hipMemcpyHostToDevice, s));
    d_invd = b->invd, d_sigma = b->sigma, d_no = b->n_obs;
  }
  int rc = T_new ? sdw_check_launch(wm, d_key, d_stride, W, H, K, T_new) : VO_OK;  // (both poses are checked before either launch)
  if (!rc) rc = sdw_enqueue(wm, s, d_invd, d_sigma, d_no, d_key, d_stride, W, H, K, T_wk, remove);
  if (!rc && T_new) {
    rc = sdw_enqueue(wm, s, d_invd, d_sigma, d_no, d_key, d_stride, W, H, K, T_new);
    if (!rc) ++wm->reanchors;
  }
  VO_CHECK_HIP(c, hipStreamSynchronize(s));  // (the copies read the caller's memory)
  return rc;
}

extern "C" int vo_semidense_world_integrate(vo_semidense_world *wm, const float *invd, const float *sigma, const uint8_t *n_obs,
                                            const uint8_t *key_plane, int key_stride, int key_on_device, int width, int height, int on_device,
                                            const float K[4], const float T_wk[16]) {
  return sdw_operator(wm, invd, sigma, n_obs, key_plane, key_stride, key_on_device, width, height, on_device, K, T_wk, false, nullptr);
}

extern "C" int vo_semidense_world_remove(vo_semidense_world *wm, const float *invd, const float *sigma, const uint8_t *n_obs,
                                         const uint8_t *key_plane, int key_stride, int key_on_device, int width, int height, int on_device,
                                         const float K[4], const float T_wk[16]) {
  return sdw_operator(wm, invd, sigma, n_obs, key_plane, key_stride, key_on_device, width, height, on_device, K, T_wk, true, nullptr);
}

extern "C" int vo_semidense_world_reanchor(vo_semidense_world *wm, const float *invd, const float *sigma, const uint8_t *n_obs,
                                           const uint8_t *key_plane, int key_stride, int key_on_device, int width, int height, int on_device,
                                           const float K[4], const float T_old[16], const float T_new[16], int *moved) {
  if (!T_old || !T_new || !moved) return VO_ERR_INVALID;
  *moved = 0;
  if (memcmp(T_old, T_new, 12 * sizeof(float)) == 0) {  // the same bits: no launch, no seq
    if (!wm || !invd || !sigma || !n_obs || !K || width <= 0 || height <= 0) return VO_ERR_INVALID;
    return VO_OK;
  }
  const int rc = sdw_operator(wm, invd, sigma, n_obs, key_plane, key_stride, key_on_device, width, height, on_device, K, T_old, true, T_new);
  if (!rc) *moved = 1;
  return rc;
}

static int sdw_reanchor_stats(vo_semidense_world *wm, hipStream_t s, vo_semidense_world_reanchor_info *info) {
  vo_ctx *c = wm->c;
  const size_t n_slots = (size_t)1 << wm->prm.capacity_log2;
  SdwReanchorState rs;
  VO_CHECK_HIP(c, hipMemsetAsync(&wm->rs->vacant, 0, sizeof(unsigned), s));
  hipLaunchKernelGGL(semidense_world_vacant_kernel, dim3((unsigned)(n_slots / SDW_NT)), dim3(SDW_NT), 0, s, wm->slots, n_slots, wm->rs);
  VO_CHECK_HIP(c, hipGetLastError());
  VO_CHECK_HIP(c, hipMemcpyAsync(&rs, wm->rs, sizeof(rs), hipMemcpyDeviceToHost, s));
  VO_CHECK_HIP(c, hipStreamSynchronize(s));
  info->removals = rs.removals;
  info->refused_removals = rs.refused_removals;
  info->removed = rs.removed;
  info->missing = rs.missing;
  info->reanchors = wm->reanchors;
  info->vacant = rs.vacant;
  return VO_OK;
}

extern "C" int vo_semidense_world_reanchor_stats(vo_semidense_world *wm, vo_semidense_world_reanchor_info *info) {
  if (!wm || !info) return VO_ERR_INVALID;
  VO_CHECK_HIP(wm->c, hipSetDevice(wm->c->device));
  return sdw_reanchor_stats(wm, wm->c->stream, info);
}

// ---- stats and extraction: synchronous on stream s ----------------------------------------------------------------------------------
// (refused_removals: the removal's word, which lies behind SdwState and comes with the same copy — StereoVO's getter settles with it)
static int sdw_stats(vo_semidense_world *wm, hipStream_t s, vo_semidense_world_info *info, unsigned long long *refused_removals = nullptr) {
  vo_ctx *c = wm->c;
  struct {
    SdwState st;
    SdwReanchorState rs;
  } both;
  static_assert(sizeof(both) + sizeof(SdwCarveState) == SDW_STATE_BYTES, "the two blocks lie back to back, the carve's behind them");
  VO_CHECK_HIP(c, hipMemcpyAsync(&both, wm->st, sizeof(both), hipMemcpyDeviceToHost, s));
  VO_CHECK_HIP(c, hipStreamSynchronize(s));
  const SdwState &st = both.st;
  if (refused_removals) *refused_removals = both.rs.refused_removals;
  info->occupied = st.occupied;
  info->capacity = 1ull << wm->prm.capacity_log2;
  info->integrations = st.integrations;
  info->refused = st.refused;
  info->inserted = st.inserted;
  info->skipped = st.skipped;
  info->out_of_range = st.out_of_range;
  return VO_OK;
}

extern "C" int vo_semidense_world_stats(vo_semidense_world *wm, vo_semidense_world_info *info) {
  if (!wm || !info) return VO_ERR_INVALID;
  VO_CHECK_HIP(wm->c, hipSetDevice(wm->c->device));
  return sdw_stats(wm, wm->c->stream, info);
}

// the free filter of vo_semidense_world_points_free; null: the extraction as it was, by its own kernel
struct SdwFreeFilter {
  unsigned num, den;
};

static int sdw_extract_launch(vo_semidense_world *wm, hipStream_t s, int min_count, int min_keyframes, const SdwFreeFilter *ff, unsigned *n) {
  vo_ctx *c = wm->c;
  SdwExtractArgs a;
  memset(&a, 0, sizeof(a));
  a.slots = wm->slots;
  a.n_slots = (size_t)1 << wm->prm.capacity_log2;
  a.min_count = (unsigned)min_count;
  a.min_keyframes = (unsigned)min_keyframes;
  a.out = wm->scratch;
  a.cap = (unsigned)wm->scratch_cap;
  a.st = wm->st;
  VO_CHECK_HIP(c, hipMemsetAsync(&wm->st->n_extract, 0, sizeof(unsigned), s));
  if (ff) {
    SdwExtractFreeArgs fa;
    fa.e = a;
    fa.free_num = ff->num;
    fa.free_den = ff->den;
    hipLaunchKernelGGL(semidense_world_extract_free_kernel, dim3((unsigned)(a.n_slots / SDW_NT)), dim3(SDW_NT), 0, s, fa);
  } else
    hipLaunchKernelGGL(semidense_world_extract_kernel, dim3((unsigned)(a.n_slots / SDW_NT)), dim3(SDW_NT), 0, s, a);
  VO_CHECK_HIP(c, hipGetLastError());
  VO_CHECK_HIP(c, hipMemcpyAsync(n, &wm->st->n_extract, sizeof(unsigned), hipMemcpyDeviceToHost, s));
  VO_CHECK_HIP(c, hipStreamSynchronize(s));
  return VO_OK;
}

static int sdw_points(vo_semidense_world *wm, hipStream_t s, int min_count, int min_keyframes, int cap, int32_t *index, float *xyz,
                      uint32_t *weight, uint32_t *count, uint32_t *keyframes, uint8_t *grey, uint64_t *sums, int *n,
                      const SdwFreeFilter *ff = nullptr, uint32_t *free_count = nullptr) {
  vo_ctx *c = wm->c;
  if (min_count < 1 || min_keyframes < 1) VO_FAIL(c, VO_ERR_INVALID, "semi-dense world map: min_count and min_keyframes are >= 1");
  unsigned k = 0;
  int rc = sdw_extract_launch(wm, s, min_count, min_keyframes, ff, &k);
  if (rc) return rc;
  *n = (int)k;
  if (cap == 0 || k == 0) return k > (unsigned)cap ? VO_ERR_CAPACITY : VO_OK;
  if ((size_t)k > wm->scratch_cap) {  // the first getter that needs more records than any before: the scratch grows, the launch repeats
    if (wm->scratch) (void)hipFree(wm->scratch);
    wm->scratch = nullptr;
    wm->scratch_cap = 0;
    VO_CHECK_HIP(c, vo_dev_malloc(c, (void **)&wm->scratch, (size_t)k * sizeof(SdwSlot)));
    wm->scratch_cap = k;
    rc = sdw_extract_launch(wm, s, min_count, min_keyframes, ff, &k);
    if (rc) return rc;
  }
  std::vector<SdwSlot> rec(k);
  VO_CHECK_HIP(c, hipMemcpyAsync(rec.data(), wm->scratch, (size_t)k * sizeof(SdwSlot), hipMemcpyDeviceToHost, s));
  VO_CHECK_HIP(c, hipStreamSynchronize(s));
  std::sort(rec.begin(), rec.end(), [](const SdwSlot &x, const SdwSlot &y) { return x.key < y.key; });
  const size_t m = k < (unsigned)cap ? k : (size_t)cap;
  const double voxel = (double)wm->prm.voxel;
  for (size_t i = 0; i < m; ++i) {
    const SdwSlot &r = rec[i];
    const sdw_u64 sxyz[3] = {r.sx, r.sy, r.sz};
    for (int ax = 0; ax < 3; ++ax) {
      const int idx = (int)((r.key >> (42 - 21 * ax)) & 0x1FFFFFull) - 1048576;
      if (index) index[3 * i + ax] = idx;
      if (xyz) {  // (host code: -ffp-contract=off, every operation rounded on its own)
        const double f = (double)sxyz[ax] / (double)r.sw + 0.5;
        const double p = (double)idx + f * (1.0 / 1024);
        xyz[3 * i + ax] = (float)(p * voxel);
      }
    }
    if (weight) weight[i] = r.sw > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)r.sw;
    if (count) count[i] = r.cnt;
    if (keyframes) keyframes[i] = r.kf_cnt;
    if (free_count) free_count[i] = r.free;
    if (grey) grey[i] = (uint8_t)((r.sg + r.sw / 2) / r.sw);
    if (sums) sums[5 * i] = r.sw, sums[5 * i + 1] = r.sx, sums[5 * i + 2] = r.sy, sums[5 * i + 3] = r.sz, sums[5 * i + 4] = r.sg;
  }
  return k > (unsigned)cap ? VO_ERR_CAPACITY : VO_OK;
}

extern "C" int vo_semidense_world_points(vo_semidense_world *wm, int min_count, int min_keyframes, int cap, int32_t *index, float *xyz,
                                         uint32_t *weight, uint32_t *count, uint32_t *keyframes, uint8_t *grey, uint64_t *sums, int *n) {
  if (!wm || !n || cap < 0) return VO_ERR_INVALID;
  VO_CHECK_HIP(wm->c, hipSetDevice(wm->c->device));
  return sdw_points(wm, wm->c->stream, min_count, min_keyframes, cap, index, xyz, weight, count, keyframes, grey, sums, n);
}

// ---- free-space carving ------------------------------------------------------------------------------------------------
extern "C" int vo_semidense_world_carve_default_params(vo_semidense_world_carve_params *p) {
  if (!p) return VO_ERR_INVALID;
  memset(p, 0, sizeof(*p));
  p->margin = 2.0f;
  p->chi = 3.0f;
  p->z_near = 0.5f;
  return VO_OK;
}

static int sdw_check_carve_params(vo_ctx *c, const vo_semidense_world_carve_params *p) {
  if (!(p->margin >= 1.0f) || !isfinite(p->margin)) VO_FAIL(c, VO_ERR_INVALID, "world map carving: margin must be >= 1 voxel and finite");
  if (!(p->chi >= 0.0f) || !isfinite(p->chi)) VO_FAIL(c, VO_ERR_INVALID, "world map carving: chi must be >= 0 and finite");
  if (!(p->z_near > 0.0f) || !isfinite(p->z_near)) VO_FAIL(c, VO_ERR_INVALID, "world map carving: z_near must be positive and finite");
  return VO_OK;
}

// On stream s, DEVICE planes. No seq, no refusal: the launch reads keys and adds to `free` words and to the carve's counters only.
static int sdw_carve_enqueue(vo_semidense_world *wm, hipStream_t s, const float *invd, const float *sigma, const uint8_t *n_obs, int W, int H,
                             const float K[4], const float T_wk[16], const vo_semidense_world_carve_params *prm) {
  vo_ctx *c = wm->c;
  int rc = sdw_check_carve_params(c, prm);
  if (!rc) rc = sdw_check_launch(wm, nullptr, 0, W, H, K, T_wk);
  if (rc) return rc;
  SdwCarveArgs ca;
  memset(&ca, 0, sizeof(ca));
  SdwArgs &a = ca.a;
  a.invd = invd;
  a.sigma = sigma;
  a.n_obs = n_obs;
  a.W = W;
  a.H = H;
  a.min_obs = wm->prm.min_obs;
  a.z_max = wm->prm.z_max;
  a.voxel = wm->prm.voxel;
  a.fx = K[0], a.fy = K[1], a.cx = K[2], a.cy = K[3];
  memcpy(a.T, T_wk, sizeof(a.T));
  a.capacity_log2 = wm->prm.capacity_log2;
  a.slots = wm->slots;
  a.st = wm->st;
  ca.margin = prm->margin;
  ca.chi = prm->chi;
  ca.z_near = prm->z_near;
  ca.dz = a.voxel * 0.5f;
  ca.k0 = 1;  // the first sample's k is the launch's: z_k does not fall with k (host code: -ffp-contract=off)
  while (ca.k0 <= SDWC_MAX_K && !(ca.z_near <= (float)ca.k0 * ca.dz)) ++ca.k0;
  ca.cs = wm->cs;
  const unsigned nb = (unsigned)(((size_t)W * (size_t)H + SDW_BLOCK - 1) / SDW_BLOCK);
  hipStream_t keep = c->stream;
  c->stream = s;
  vo_prof_begin(c, VO_K_AUX);
  // the simple form is the default: the faster of the two on a table as lightly loaded as a sequence leaves it
  if (c->dbg[VO_DBG_SDW_FORM] == 1)
    hipLaunchKernelGGL(semidense_world_carve_kernel<true>, dim3(nb), dim3(SDW_NT), 0, s, ca);
  else
    hipLaunchKernelGGL(semidense_world_carve_kernel<false>, dim3(nb), dim3(SDW_NT), 0, s, ca);
  vo_prof_end(c);
  c->stream = keep;
  VO_CHECK_HIP(c, hipGetLastError());
  return VO_OK;
}

extern "C" int vo_semidense_world_carve(vo_semidense_world *wm, const float *invd, const float *sigma, const uint8_t *n_obs, int width,
                                        int height, int on_device, const float K[4], const float T_wk[16],
                                        const vo_semidense_world_carve_params *prm) {
  if (!wm || !invd || !sigma || !n_obs || !K || !T_wk || !prm || width <= 0 || height <= 0) return VO_ERR_INVALID;
  vo_ctx *c = wm->c;
  if (width > c->cfg.max_width || height > c->cfg.max_height)
    VO_FAIL(c, VO_ERR_SIZE, "%d x %d planes exceed vo_config.max_width x max_height", width, height);
  int rc = sdw_check_carve_params(c, prm);  // (before any copy: a bad call touches nothing)
  if (!rc) rc = sdw_check_launch(wm, nullptr, 0, width, height, K, T_wk);
  if (rc) return rc;
  VO_CHECK_HIP(c, hipSetDevice(c->device));
  hipStream_t s = c->stream;
  const size_t np = (size_t)width * (size_t)height;
  const float *d_invd = invd, *d_sigma = sigma;
  const uint8_t *d_no = n_obs;
  if (!on_device) {
    vo_sdt_buffers *b = nullptr;
    rc = vo_sdt_ctx_buffers(c, &b);
    if (rc) return rc;
    VO_CHECK_HIP(c, hipMemcpyAsync(b->invd, invd, np * sizeof(float), hipMemcpyHostToDevice, s));
    VO_CHECK_HIP(c, hipMemcpyAsync(b->sigma, sigma, np * sizeof(float), hipMemcpyHostToDevice, s));
    VO_CHECK_HIP(c, hipMemcpyAsync(b->n_obs, n_obs, np, hipMemcpyHostToDevice, s));
    d_invd = b->invd, d_sigma = b->sigma, d_no = b->n_obs;
  }
  rc = sdw_carve_enqueue(wm, s, d_invd, d_sigma, d_no, width, height, K, T_wk, prm);
  VO_CHECK_HIP(c, hipStreamSynchronize(s));  // (the copies read the caller's memory)
  return rc;
}

static int sdw_carve_stats(vo_semidense_world *wm, hipStream_t s, vo_semidense_world_carve_info *info) {
  vo_ctx *c = wm->c;
  SdwCarveState cs;
  VO_CHECK_HIP(c, hipMemcpyAsync(&cs, wm->cs, sizeof(cs), hipMemcpyDeviceToHost, s));
  VO_CHECK_HIP(c, hipStreamSynchronize(s));
  info->carves = cs.carves;
  info->rays = cs.rays;
  info->short_rays = cs.short_rays;
  info->visits = cs.visits;
  info->hits = cs.hits;
  return VO_OK;
}

extern "C" int vo_semidense_world_carve_stats(vo_semidense_world *wm, vo_semidense_world_carve_info *info) {
  if (!wm || !info) return VO_ERR_INVALID;
  VO_CHECK_HIP(wm->c, hipSetDevice(wm->c->device));
  return sdw_carve_stats(wm, wm->c->stream, info);
}

static int sdw_free_filter(vo_ctx *c, int free_num, int free_den, SdwFreeFilter *ff) {
  if (free_num < 0 || free_den < 0) VO_FAIL(c, VO_ERR_INVALID, "semi-dense world map: free_num and free_den are >= 0");
  ff->num = (unsigned)free_num;
  ff->den = (unsigned)free_den;
  return VO_OK;
}

extern "C" int vo_semidense_world_points_free(vo_semidense_world *wm, int min_count, int min_keyframes, int free_num, int free_den, int cap,
                                              int32_t *index, float *xyz, uint32_t *weight, uint32_t *count, uint32_t *keyframes,
                                              uint8_t *grey, uint64_t *sums, uint32_t *free_count, int *n) {
  if (!wm || !n || cap < 0) return VO_ERR_INVALID;
  SdwFreeFilter ff;
  const int rc = sdw_free_filter(wm->c, free_num, free_den, &ff);
  if (rc) return rc;
  VO_CHECK_HIP(wm->c, hipSetDevice(wm->c->device));
  return sdw_points(wm, wm->c->stream, min_count, min_keyframes, cap, index, xyz, weight, count, keyframes, grey, sums, n, &ff, free_count);
}

// ---- StereoVO's hook ------------------------------------------------------------------------------------------------------------------
// The current keyframe's map — the temporal option's planes, or the regularised copy — into the table, on the side stream behind the
// launches that wrote it. Called by vo_svo_semidense_temporal_enqueue at the top of a keyframe change, in front of the propagation's
// scatter and the key plane's copy, and by vo_svo_semidense_world_flush; `done`: the map is marked so that it is not integrated twice.
struct SdwRing {
  float *invd, *sigma;
  uint8_t *n_obs, *key;
};

static SdwRing svo_sdw_ring(const vo_svo_semidense_world &w, int slot) {
  char *base = (char *)w.ra.ring + (size_t)slot * w.ra.np_max * 10;
  SdwRing p;
  p.invd = (float *)base;
  p.sigma = (float *)(base + 4 * w.ra.np_max);
  p.n_obs = (uint8_t *)(base + 8 * w.ra.np_max);
  p.key = p.n_obs + w.ra.np_max;
  return p;
}

static bool svo_sdw_in_window(const vo_svo *s, int kf_index) {
  for (const SvoKeyframe &k : s->keyframes)
    if (k.global == kf_index) return true;
  return false;
}

// the live anchors whose keyframe has left the window move to the frozen record, in order; their ring places are free
static void svo_sdw_freeze(vo_svo *s) {
  vo_svo_semidense_world &w = s->sdw;
  size_t keep = 0;
  for (size_t i = 0; i < w.ra.live.size(); ++i) {
    if (svo_sdw_in_window(s, w.ra.live[i].kf_index)) {
      if (keep != i) w.ra.live[keep] = w.ra.live[i];
      ++keep;
    } else {
      w.ra.live[i].slot = -1;
      w.ra.frozen.push_back(w.ra.live[i]);
    }
  }
  w.ra.live.resize(keep);
}

// (vo_svo_set_semidense_world_reanchor) what is about to be integrated — the planes and the key plane of the current keyframe's map —
// into a free place of the ring, device to device on the side stream, and the anchor: the keyframe and the pose it goes in with
static int svo_sdw_retain(vo_svo *s, const float *invd, const float *sigma, const uint8_t *n_obs) {
  vo_ctx *c = s->c;
  vo_svo_semidense_world &w = s->sdw;
  const vo_svo_semidense_temporal &t = s->sdt;
  if (!w.ra.ring) return VO_OK;
  svo_sdw_freeze(s);
  unsigned used = 0;
  for (const vo_svo_semidense_world::Anchor &an : w.ra.live) used |= 1u << an.slot;
  vo_svo_semidense_world::Anchor an;
  an.frame_id = t.frame_id;
  an.kf_index = t.kf_index;
  an.order = w.ra.n_anchors++;
  an.w = t.w;
  an.h = t.h;
  memcpy(an.T_wk, t.T_wk, sizeof(an.T_wk));
  an.slot = -1;
  if (t.kf_index < 0 || !svo_sdw_in_window(s, t.kf_index)) {  // (a window of one keyframe: the outgoing one has left it already)
    w.ra.frozen.push_back(an);
    return VO_OK;
  }
  const size_t np = (size_t)t.w * (size_t)t.h;
  if (np > w.ra.np_max) VO_FAIL(c, VO_ERR_SIZE, "world map re-anchoring: a %d x %d map exceeds vo_config.max_width x max_height", t.w, t.h);
  for (int k = 0; k < w.ra.n_slots && an.slot < 0; ++k)
    if (!(used & (1u << k))) an.slot = k;
  // (cannot happen: the window holds kf_window keyframes at most, and only keyframes of the window keep a place)
  if (an.slot < 0) VO_FAIL(c, VO_ERR_CAPACITY, "world map re-anchoring: no free place among %d for keyframe %d", w.ra.n_slots, t.kf_index);
  const SdwRing p = svo_sdw_ring(w, an.slot);
  hipStream_t side = c->stream2;
  VO_CHECK_HIP(c, hipMemcpyAsync(p.invd, invd, np * sizeof(float), hipMemcpyDeviceToDevice, side));
  VO_CHECK_HIP(c, hipMemcpyAsync(p.sigma, sigma, np * sizeof(float), hipMemcpyDeviceToDevice, side));
  VO_CHECK_HIP(c, hipMemcpyAsync(p.n_obs, n_obs, np, hipMemcpyDeviceToDevice, side));
  VO_CHECK_HIP(c, hipMemcpyAsync(p.key, t.buf.key, np, hipMemcpyDeviceToDevice, side));
  w.ra.live.push_back(an);
  return VO_OK;
}

int vo_svo_semidense_world_enqueue(vo_svo *s) {
  vo_svo_semidense_world &w = s->sdw;
  const vo_svo_semidense_temporal &t = s->sdt;
  if (!w.on || !t.have || w.done) return VO_OK;
  const float *invd = t.buf.invd, *sigma = t.buf.sigma;
  const uint8_t *n_obs = t.buf.n_obs;
  if (w.source == VO_SEMIDENSE_WORLD_REGULARIZED) {
    const vo_svo_semidense_regularize &r = s->sdr;
    if (!r.on || !r.have || r.frame_id != t.frame_id) return VO_OK;  // no regularised planes of this keyframe: nothing to integrate
    invd = r.buf.invd, sigma = r.buf.sigma, n_obs = r.buf.n_obs;
  }
  if (w.source == VO_SEMIDENSE_WORLD_DENSE || w.source == VO_SEMIDENSE_WORLD_MERGED) {
    // one merge launch into planes the option owns; what follows takes them as it takes the regularised ones. No dense result of
    // this keyframe's own pair: nothing to integrate
    bool ok = false;
    const int rcm = vo_svo_sdm_merge(s, &invd, &sigma, &n_obs, &ok);
    if (rcm) return rcm;
    if (!ok) return VO_OK;
  }
  int rc = w.ra.on ? svo_sdw_retain(s, invd, sigma, n_obs) : VO_OK;  // (in front of everything that overwrites the outgoing map)
  if (rc) return rc;
  rc = sdw_enqueue(w.wm, s->c->stream2, invd, sigma, n_obs, t.buf.key, t.w, t.w, t.h, s->prm.frame.Kl, t.T_wk);
  if (rc) return rc;
  // vo_svo_set_semidense_world_carve: the same planes with the same pose, directly behind their integration
  if (w.carve_on) rc = sdw_carve_enqueue(w.wm, s->c->stream2, invd, sigma, n_obs, t.w, t.h, s->prm.frame.Kl, t.T_wk, &w.carve);
  if (rc) return rc;
  w.done = true;
  return VO_OK;
}

// the local BA has written its poses back to kf_all: every retained map whose keyframe is still in the window moves from the pose it
// is in the table with to the keyframe's current one, where the two differ in bits and by min_move voxels at least (decided here, in
// double: move = max_r |dt_r| + z_max max_r sum_c |dR_rc|). On the side stream behind the frame's integration; nothing waits. The
// device decides whether a pair is refused, so the pair is logged with the pose it replaces (svo_sdw_settle).
int vo_svo_semidense_world_reanchor_pass(vo_svo *s) {
  vo_svo_semidense_world &w = s->sdw;
  if (!w.on || !w.ra.on || !w.ra.ring) return VO_OK;
  const double bound = w.ra.min_move * (double)w.wm->prm.voxel, z_max = (double)w.wm->prm.z_max;
  svo_sdw_freeze(s);  // (a keyframe that has left the window keeps the pose of the last pass it was in: nothing moves it any more)
  for (vo_svo_semidense_world::Anchor &an : w.ra.live) {
    const float *Tn = s->kf_all[an.kf_index].T_wc;
    if (memcmp(an.T_wk, Tn, 12 * sizeof(float)) == 0) continue;
    double dt = 0.0, dr = 0.0;
    for (int r = 0; r < 3; ++r) {
      double row = 0.0;
      for (int k = 0; k < 3; ++k) row += fabs((double)Tn[4 * r + k] - (double)an.T_wk[4 * r + k]);
      dr = std::max(dr, row);
      dt = std::max(dt, fabs((double)Tn[4 * r + 3] - (double)an.T_wk[4 * r + 3]));
    }
    if (!(dt + z_max * dr >= bound)) continue;
    const SdwRing p = svo_sdw_ring(w, an.slot);
    int rc = sdw_check_launch(w.wm, p.key, an.w, an.w, an.h, s->prm.frame.Kl, Tn);  // (both poses are checked before either launch)
    if (!rc) rc = sdw_enqueue(w.wm, s->c->stream2, p.invd, p.sigma, p.n_obs, p.key, an.w, an.w, an.h, s->prm.frame.Kl, an.T_wk, true);
    if (!rc) rc = sdw_enqueue(w.wm, s->c->stream2, p.invd, p.sigma, p.n_obs, p.key, an.w, an.w, an.h, s->prm.frame.Kl, Tn);
    if (rc) return rc;
    ++w.wm->reanchors;
    vo_svo_semidense_world::Pair pr;
    pr.frame_id = an.frame_id;
    memcpy(pr.T_prev, an.T_wk, sizeof(pr.T_prev));
    w.ra.log.push_back(pr);
    memcpy(an.T_wk, Tn, sizeof(an.T_wk));
  }
  return VO_OK;
}

void vo_svo_semidense_world_free(vo_svo *s) {
  if (s->sdw.ra.ring) {
    (void)hipSetDevice(s->c->device);
    (void)hipFree(s->sdw.ra.ring);
  }
  vo_svo_sdm_free(s);
  vo_semidense_world_destroy(s->sdw.wm);
  s->sdw = vo_svo_semidense_world();
}

// the table has been cleared: no map is in it
static void svo_sdw_forget(vo_svo_semidense_world &w) {
  w.ra.live.clear();
  w.ra.frozen.clear();
  w.ra.log.clear();
  w.ra.n_anchors = 0;
  w.ra.refused_seen = 0;
}

extern "C" int vo_svo_set_semidense_world(vo_svo *s, const vo_semidense_world_params *prm, int source) {
  if (!s) return VO_ERR_INVALID;
  vo_ctx *c = s->c;
  if (s->pending) VO_FAIL(c, VO_ERR_INVALID, "vo_svo_set_semidense_world: a frame is in flight: call vo_svo_result first");
  if (s->mono) VO_FAIL(c, VO_ERR_INVALID, "vo_svo_set_semidense_world: a stereo driver only");
  vo_svo_semidense_world &w = s->sdw;
  if (!prm) {
    w.on = false;
    w.carve_on = false;  // (the carve needs the world map)
    return VO_OK;
  }
  if (!s->sdt.on || !s->sd.on)
    VO_FAIL(c, VO_ERR_INVALID, "vo_svo_set_semidense_world: needs the temporal option: vo_svo_set_semidense_temporal first");
  if (source != VO_SEMIDENSE_WORLD_RAW && source != VO_SEMIDENSE_WORLD_REGULARIZED && source != VO_SEMIDENSE_WORLD_DENSE &&
      source != VO_SEMIDENSE_WORLD_MERGED)
    VO_FAIL(c, VO_ERR_INVALID, "vo_svo_set_semidense_world: source=%d: expected VO_SEMIDENSE_WORLD_RAW, _REGULARIZED, _DENSE or _MERGED", source);
  const bool from_dense = source == VO_SEMIDENSE_WORLD_DENSE || source == VO_SEMIDENSE_WORLD_MERGED;
  if (from_dense && !s->ds.on)
    VO_FAIL(c, VO_ERR_INVALID, "vo_svo_set_semidense_world: the dense and merged sources need vo_svo_set_dense_stereo first");
  if (source == VO_SEMIDENSE_WORLD_REGULARIZED && !s->sdr.on)
    VO_FAIL(c, VO_ERR_INVALID, "vo_svo_set_semidense_world: the regularised source needs vo_svo_set_semidense_regularize first");
  int rc = sdw_check_params(c, prm);
  if (rc) return rc;
  if (w.wm && w.wm->prm.capacity_log2 != prm->capacity_log2)
    VO_FAIL(c, VO_ERR_INVALID, "vo_svo_set_semidense_world: capacity_log2 is fixed by the first enable (%d)", w.wm->prm.capacity_log2);
  if (!w.wm) {
    rc = vo_semidense_world_create(c, prm, &w.wm);  // the option's only allocation, at the first enable
    if (rc) return rc;
  } else if (memcmp(&w.wm->prm, prm, sizeof(*prm)) != 0) {  // another voxel or gate: the sums of the old one mean nothing
    VO_CHECK_HIP(c, hipSetDevice(c->device));
    if (s->sd.have) VO_CHECK_HIP(c, hipEventSynchronize(s->sd.done));
    rc = vo_semidense_world_clear(w.wm);
    if (rc) return rc;
    w.wm->prm = *prm;
    w.done = false;
    svo_sdw_forget(w);
  }
  if (from_dense) {  // the merged planes and the keyframe's dense copy: once, at the first enable of such a source
    rc = vo_svo_sdm_alloc(s);
    if (rc) return rc;
  }
  w.source = source;
  w.on = true;
  return VO_OK;
}

// The pairs the passes have enqueued since the counters were last read: a refused pair left its map where it was, so its anchor takes
// the replaced pose back. `occupied` never falls and the driver's maps have one size, so once a launch is refused every later one is:
// the refused pairs are the LAST ones of the log, and a pair enqueued on top of a refused one was refused with it. refused_removals:
// the device's word, as the getter that calls this has just fetched it with its statistics (no copy or wait of its own).
static void svo_sdw_settle(vo_svo *s, unsigned long long refused_removals) {
  vo_svo_semidense_world &w = s->sdw;
  const unsigned long long grew = refused_removals - w.ra.refused_seen;
  w.ra.refused_seen = refused_removals;
  for (size_t k = 0; k < grew && k < w.ra.log.size(); ++k) {
    const vo_svo_semidense_world::Pair &p = w.ra.log[w.ra.log.size() - 1 - k];
    vo_svo_semidense_world::Anchor *an = nullptr;  // (by frame id: the anchor may have been frozen since)
    for (auto &a : w.ra.live)
      if (a.frame_id == p.frame_id) an = &a;
    for (size_t q = w.ra.frozen.size(); !an && q-- > 0;)
      if (w.ra.frozen[q].frame_id == p.frame_id) an = &w.ra.frozen[q];
    if (an) memcpy(an->T_wk, p.T_prev, sizeof(p.T_prev));
  }
  w.ra.log.clear();
}

static int svo_sdw_ready(vo_svo *s, const char *who) {
  vo_ctx *c = s->c;
  if (s->pending) VO_FAIL(c, VO_ERR_INVALID, "%s: a frame is in flight: call vo_svo_result first", who);
  if (!s->sdw.on || !s->sdw.wm) VO_FAIL(c, VO_ERR_INVALID, "%s: the option is off: vo_svo_set_semidense_world", who);
  VO_CHECK_HIP(c, hipSetDevice(c->device));
  if (s->sd.have) VO_CHECK_HIP(c, hipEventSynchronize(s->sd.done));  // the side stream's last launch only
  return VO_OK;
}

extern "C" int vo_svo_semidense_world_flush(vo_svo *s) {
  if (!s) return VO_ERR_INVALID;
  vo_ctx *c = s->c;
  if (s->pending) VO_FAIL(c, VO_ERR_INVALID, "vo_svo_semidense_world_flush: a frame is in flight: call vo_svo_result first");
  if (!s->sdw.on || !s->sdw.wm) VO_FAIL(c, VO_ERR_INVALID, "vo_svo_semidense_world_flush: the option is off: vo_svo_set_semidense_world");
  if (!s->sdt.on || !s->sdt.have || s->sdw.done) return VO_OK;
  VO_CHECK_HIP(c, hipSetDevice(c->device));
  const int rc = vo_svo_semidense_world_enqueue(s);
  if (rc) return rc;
  VO_CHECK_HIP(c, hipEventRecord(s->sd.done, c->stream2));
  return VO_OK;
}

extern "C" int vo_svo_semidense_world_clear(vo_svo *s) {
  if (!s) return VO_ERR_INVALID;
  int rc = svo_sdw_ready(s, "vo_svo_semidense_world_clear");
  if (rc) return rc;
  rc = vo_semidense_world_clear(s->sdw.wm);
  if (rc) return rc;
  s->sdw.done = false;
  svo_sdw_forget(s->sdw);
  return VO_OK;
}

extern "C" int vo_svo_get_semidense_world_stats(vo_svo *s, vo_semidense_world_info *info) {
  if (!s || !info) return VO_ERR_INVALID;
  int rc = svo_sdw_ready(s, "vo_svo_get_semidense_world_stats");
  if (rc) return rc;
  unsigned long long refused_removals = 0;
  rc = sdw_stats(s->sdw.wm, s->c->stream, info, &refused_removals);
  if (!rc) svo_sdw_settle(s, refused_removals);
  return rc;
}

extern "C" int vo_svo_get_semidense_world_points(vo_svo *s, int min_count, int min_keyframes, int cap, int32_t *index, float *xyz,
                                                 uint32_t *weight, uint32_t *count, uint32_t *keyframes, uint8_t *grey, int *n) {
  if (!s || !n || cap < 0) return VO_ERR_INVALID;
  const int rc = svo_sdw_ready(s, "vo_svo_get_semidense_world_points");
  if (rc) return rc;
  return sdw_points(s->sdw.wm, s->c->stream, min_count, min_keyframes, cap, index, xyz, weight, count, keyframes, grey, nullptr, n);
}

// ---- vo_svo_set_semidense_world_reanchor ----------------------------------------------------------------------------
extern "C" int vo_svo_set_semidense_world_reanchor(vo_svo *s, int on, float min_move) {
  if (!s) return VO_ERR_INVALID;
  vo_ctx *c = s->c;
  if (s->pending) VO_FAIL(c, VO_ERR_INVALID, "vo_svo_set_semidense_world_reanchor: a frame is in flight: call vo_svo_result first");
  if (s->mono) VO_FAIL(c, VO_ERR_INVALID, "vo_svo_set_semidense_world_reanchor: a stereo driver only");
  vo_svo_semidense_world &w = s->sdw;
  if (!on) {
    w.ra.on = false;
    return VO_OK;
  }
  if (!w.on || !w.wm) VO_FAIL(c, VO_ERR_INVALID, "vo_svo_set_semidense_world_reanchor: needs the world map: vo_svo_set_semidense_world first");
  if (!s->prm.local_ba) VO_FAIL(c, VO_ERR_INVALID, "vo_svo_set_semidense_world_reanchor: needs vo_svo_params.local_ba: nothing else moves a keyframe");
  if (!(min_move >= 0.0f) || !isfinite(min_move)) VO_FAIL(c, VO_ERR_INVALID, "vo_svo_set_semidense_world_reanchor: min_move must be >= 0 and finite");
  if (!w.ra.ring) {  // the option's only allocation, at the first enable: a place per keyframe of the window
    if (s->prm.kf_window < 1 || s->prm.kf_window > 32) VO_FAIL(c, VO_ERR_INVALID, "vo_svo_set_semidense_world_reanchor: a window of 1 .. 32 keyframes");
    VO_CHECK_HIP(c, hipSetDevice(c->device));
    const size_t np_max = ((size_t)c->cfg.max_width * (size_t)c->cfg.max_height + 63) / 64 * 64;
    if (vo_dev_malloc(c, &w.ra.ring, (size_t)s->prm.kf_window * np_max * 10) != hipSuccess) {
      w.ra.ring = nullptr;
      VO_FAIL(c, VO_ERR_HIP, "vo_svo_set_semidense_world_reanchor: no device memory for %d retained maps", s->prm.kf_window);
    }
    w.ra.n_slots = s->prm.kf_window;
    w.ra.np_max = np_max;
  }
  w.ra.min_move = (double)min_move;
  w.ra.on = true;
  return VO_OK;
}

extern "C" int vo_svo_get_semidense_world_anchors(vo_svo *s, int cap, int32_t *frame_id, int32_t *kf_index, float *T_wk, int32_t *in_window,
                                                  int *n) {
  if (!s || !n || cap < 0) return VO_ERR_INVALID;
  int rc = svo_sdw_ready(s, "vo_svo_get_semidense_world_anchors");
  if (rc) return rc;
  vo_svo_semidense_world &w = s->sdw;
  if (!w.ra.log.empty()) {  // (pairs have been enqueued since the last look: the counters, as the statistics getter fetches them)
    vo_semidense_world_info info;
    unsigned long long refused_removals = 0;
    rc = sdw_stats(w.wm, s->c->stream, &info, &refused_removals);
    if (rc) return rc;
    svo_sdw_settle(s, refused_removals);
  }
  // either list is in integration order: merged by `order` (an anchor integrated outside the window, which only a window of one
  // keyframe gives, goes to the frozen record at once, while older anchors may still be live)
  const size_t nf = w.ra.frozen.size(), nl = w.ra.live.size(), total = nf + nl;
  *n = (int)total;
  for (size_t i = 0, f = 0, l = 0; i < total && i < (size_t)cap; ++i) {
    const bool take_frozen = f < nf && (l >= nl || w.ra.frozen[f].order < w.ra.live[l].order);
    const vo_svo_semidense_world::Anchor &a = take_frozen ? w.ra.frozen[f++] : w.ra.live[l++];
    if (frame_id) frame_id[i] = a.frame_id;
    if (kf_index) kf_index[i] = a.kf_index;
    if (T_wk) memcpy(T_wk + 16 * i, a.T_wk, sizeof(a.T_wk));
    if (in_window) in_window[i] = a.kf_index >= 0 && svo_sdw_in_window(s, a.kf_index) ? 1 : 0;
  }
  return total > (size_t)cap ? VO_ERR_CAPACITY : VO_OK;
}

extern "C" int vo_svo_get_semidense_world_reanchor_stats(vo_svo *s, vo_semidense_world_reanchor_info *info) {
  if (!s || !info) return VO_ERR_INVALID;
  int rc = svo_sdw_ready(s, "vo_svo_get_semidense_world_reanchor_stats");
  if (rc) return rc;
  rc = sdw_reanchor_stats(s->sdw.wm, s->c->stream, info);
  if (!rc) svo_sdw_settle(s, info->refused_removals);
  return rc;
}

// ---- vo_svo_set_semidense_world_carve -------------------------------------------------------------------------------
extern "C" int vo_svo_set_semidense_world_carve(vo_svo *s, const vo_semidense_world_carve_params *prm) {
  if (!s) return VO_ERR_INVALID;
  vo_ctx *c = s->c;
  if (s->pending) VO_FAIL(c, VO_ERR_INVALID, "vo_svo_set_semidense_world_carve: a frame is in flight: call vo_svo_result first");
  if (s->mono) VO_FAIL(c, VO_ERR_INVALID, "vo_svo_set_semidense_world_carve: a stereo driver only");
  vo_svo_semidense_world &w = s->sdw;
  if (!prm) {
    w.carve_on = false;
    return VO_OK;
  }
  if (!w.on || !w.wm) VO_FAIL(c, VO_ERR_INVALID, "vo_svo_set_semidense_world_carve: needs the world map: vo_svo_set_semidense_world first");
  const int rc = sdw_check_carve_params(c, prm);
  if (rc) return rc;
  w.carve = *prm;
  w.carve_on = true;
  return VO_OK;
}

extern "C" int vo_svo_get_semidense_world_carve_stats(vo_svo *s, vo_semidense_world_carve_info *info) {
  if (!s || !info) return VO_ERR_INVALID;
  const int rc = svo_sdw_ready(s, "vo_svo_get_semidense_world_carve_stats");
  if (rc) return rc;
  return sdw_carve_stats(s->sdw.wm, s->c->stream, info);
}

extern "C" int vo_svo_get_semidense_world_points_free(vo_svo *s, int min_count, int min_keyframes, int free_num, int free_den, int cap,
                                                      int32_t *index, float *xyz, uint32_t *weight, uint32_t *count, uint32_t *keyframes,
                                                      uint8_t *grey, uint32_t *free_count, int *n) {
  if (!s || !n || cap < 0) return VO_ERR_INVALID;
  int rc = svo_sdw_ready(s, "vo_svo_get_semidense_world_points_free");
  if (rc) return rc;
  SdwFreeFilter ff;
  rc = sdw_free_filter(s->c, free_num, free_den, &ff);
  if (rc) return rc;
  return sdw_points(s->sdw.wm, s->c->stream, min_count, min_keyframes, cap, index, xyz, weight, count, keyframes, grey, nullptr, n, &ff, free_count);
}
