// semidense_map_merge.hip — a keyframe's semi-dense map merged per pixel with a disparity result of the same keyframe (include/vo_hip.h,
// "Semi-dense map merge"): the operator (vo_semidense_map_merge) and what StereoVO's world option needs of it for its
// sources VO_SEMIDENSE_WORLD_DENSE and _MERGED (vo_svo_set_semidense_world_merge, vo_svo_get_semidense_world_source; the option
// itself is in semidense_world.hip). semidense_map_merge_device.hpp has the kernel.
#include "stereo_vo.hpp"
#include "vo_internal.hpp"
#include "vo_kernels.hpp"

#include <math.h>

// the sum of an unsigned over the wavefront's 64 lanes: six exchanges, every lane ends with the sum
__device__ __forceinline__ unsigned sdm_wave_sum(unsigned v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += (unsigned)__shfl_xor((int)v, o, 64);
  return v;
}
#define SDM_WAVE_SUM(v) sdm_wave_sum(v)
#include "semidense_map_merge_device.hpp"

#define SDM_HEAD 64  // the counts' block at an allocation's start (6 x 8 bytes, padded)

extern "C" int vo_semidense_map_merge_default_params(vo_semidense_map_merge_params *p) {
  if (!p) return VO_ERR_INVALID;
  memset(p, 0, sizeof(*p));
  p->chi = 3.0f;
  p->keep_obs = 2;
  return VO_OK;
}

int vo_sdm_check_params(vo_ctx *c, const vo_semidense_map_merge_params *p) {
  if (!(p->chi > 0.0f) || !isfinite(p->chi)) VO_FAIL(c, VO_ERR_INVALID, "semi-dense map merge: chi must be finite and positive");
  if (p->keep_obs < 0 || p->keep_obs > 256) VO_FAIL(c, VO_ERR_INVALID, "semi-dense map merge: keep_obs=%d: expected 0..256", p->keep_obs);
  return VO_OK;
}

static bool sdm_shape_ok(int W, int H) { return W >= 1 && H >= 1 && (long long)W * (long long)H <= 0x7fffffffLL; }

// the launch on `s`, DEVICE planes; counts (device, may be null) is zeroed in front of it
int vo_sdm_enqueue(vo_ctx *c, hipStream_t s, const float *m_invd, const float *m_sigma, const uint8_t *m_n_obs, const float *disp,
                   const float *sigma_invd, const uint8_t *status, int W, int H, float bf, const vo_semidense_map_merge_params *p, float *invd,
                   float *sigma, uint8_t *n_obs, uint8_t *origin, unsigned long long *counts) {
  int rc = vo_sdm_check_params(c, p);
  if (rc) return rc;
  if (!disp || !sigma_invd || !status || !invd || !sigma || !n_obs) VO_FAIL(c, VO_ERR_INVALID, "semi-dense map merge: a required plane is NULL");
  const int n_map = (m_invd != nullptr) + (m_sigma != nullptr) + (m_n_obs != nullptr);
  if (n_map != 0 && n_map != 3) VO_FAIL(c, VO_ERR_INVALID, "semi-dense map merge: the map's invd, sigma and n_obs are given together or not at all");
  if (!sdm_shape_ok(W, H)) VO_FAIL(c, VO_ERR_SIZE, "semi-dense map merge: %d x %d: expected >= 1 a side and at most 2^31 - 1 pixels", W, H);
  if (!(bf > 0.0f) || !isfinite(bf)) VO_FAIL(c, VO_ERR_INVALID, "semi-dense map merge: bf (focal length x baseline) must be positive");
  SdmArgs a;
  memset(&a, 0, sizeof(a));
  a.invd_m = m_invd, a.sigma_m = m_sigma, a.n_obs_m = m_n_obs;
  a.disp = disp, a.sigma_invd = sigma_invd, a.status = status;
  a.bf = bf;
  a.chi2 = p->chi * p->chi;  // (host code: -ffp-contract=off)
  a.keep_obs = p->keep_obs;
  a.invd = invd, a.sigma = sigma, a.n_obs = n_obs, a.origin = origin;
  a.counts = counts;
  a.n = W * H;
  a.vec = sdm_planes_aligned(a);  // the wide path, or single elements
  if (counts) VO_CHECK_HIP(c, hipMemsetAsync(counts, 0, SDM_ORIGINS * sizeof(unsigned long long), s));
  const unsigned nb = sdm_grid(a.n);
  hipStream_t keep = c->stream;
  c->stream = s;
  vo_prof_begin(c, VO_K_AUX);
  hipLaunchKernelGGL(semidense_map_merge_kernel, dim3(nb), dim3(SDM_NT), 0, s, a);
  vo_prof_end(c);
  c->stream = keep;
  VO_CHECK_HIP(c, hipGetLastError());
  return VO_OK;
}

// ---- the operator's own storage: the counts and, for host planes, the ten planes' device copies, in one allocation that grows ----
struct vo_semidense_merge_state {
  void *buf = nullptr;
  size_t bytes = 0;
};
void vo_semidense_merge_free(vo_ctx *c) {
  if (!c->semidense_m) return;
  if (c->semidense_m->buf) (void)hipFree(c->semidense_m->buf);
  delete c->semidense_m;
  c->semidense_m = nullptr;
}

extern "C" int vo_semidense_map_merge(vo_ctx *c, const float *map_invd, const float *map_sigma, const uint8_t *map_n_obs, const float *disparity,
                                      const float *sigma_invd, const uint8_t *status, int width, int height, float bf,
                                      const vo_semidense_map_merge_params *prm, float *invd, float *sigma, uint8_t *n_obs, uint8_t *origin,
                                      uint64_t *counts, int on_device) {
  if (!c || !prm) return VO_ERR_INVALID;
  int rc = vo_sdm_check_params(c, prm);
  if (rc) return rc;
  if (!disparity || !sigma_invd || !status || !invd || !sigma || !n_obs) VO_FAIL(c, VO_ERR_INVALID, "semi-dense map merge: a required plane is NULL");
  const bool has_map = map_invd != nullptr;
  if ((map_sigma != nullptr) != has_map || (map_n_obs != nullptr) != has_map)
    VO_FAIL(c, VO_ERR_INVALID, "semi-dense map merge: the map's invd, sigma and n_obs are given together or not at all");
  if (!sdm_shape_ok(width, height))
    VO_FAIL(c, VO_ERR_SIZE, "semi-dense map merge: %d x %d: expected >= 1 a side and at most 2^31 - 1 pixels", width, height);
  VO_CHECK_HIP(c, hipSetDevice(c->device));
  hipStream_t s = c->stream;
  if (!c->semidense_m) c->semidense_m = new vo_semidense_merge_state();
  vo_semidense_merge_state *st = c->semidense_m;
  const size_t n = (size_t)width * (size_t)height, ne = (n + 15) & ~(size_t)15;  // a plane's place: a multiple of 16 elements
  const size_t need = SDM_HEAD + (on_device ? 0 : 28 * ne);
  if (!st->buf || st->bytes < need) {
    if (st->buf) {
      VO_CHECK_HIP(c, hipStreamSynchronize(s));
      (void)hipFree(st->buf);
      st->buf = nullptr, st->bytes = 0;
    }
    if (vo_dev_malloc(c, &st->buf, need) != hipSuccess) {
      (void)hipGetLastError();
      st->buf = nullptr;
      VO_FAIL(c, VO_ERR_HIP, "semi-dense map merge: %zu bytes could not be allocated", need);
    }
    st->bytes = need;
  }
  unsigned long long *d_counts = counts ? (unsigned long long *)st->buf : nullptr;
  if (on_device) {
    rc = vo_sdm_enqueue(c, s, map_invd, map_sigma, map_n_obs, disparity, sigma_invd, status, width, height, bf, prm, invd, sigma, n_obs, origin, d_counts);
    if (rc) return rc;
  } else {
    float *f = (float *)((char *)st->buf + SDM_HEAD);
    uint8_t *u = (uint8_t *)(f + 6 * ne);
    float *d_mi = f, *d_ms = f + ne, *d_d = f + 2 * ne, *d_sg = f + 3 * ne, *d_oi = f + 4 * ne, *d_os = f + 5 * ne;
    uint8_t *d_mn = u, *d_st = u + ne, *d_on = u + 2 * ne, *d_og = u + 3 * ne;
    if (has_map) {
      VO_CHECK_HIP(c, hipMemcpyAsync(d_mi, map_invd, n * sizeof(float), hipMemcpyHostToDevice, s));
      VO_CHECK_HIP(c, hipMemcpyAsync(d_ms, map_sigma, n * sizeof(float), hipMemcpyHostToDevice, s));
      VO_CHECK_HIP(c, hipMemcpyAsync(d_mn, map_n_obs, n, hipMemcpyHostToDevice, s));
    }
    VO_CHECK_HIP(c, hipMemcpyAsync(d_d, disparity, n * sizeof(float), hipMemcpyHostToDevice, s));
    VO_CHECK_HIP(c, hipMemcpyAsync(d_sg, sigma_invd, n * sizeof(float), hipMemcpyHostToDevice, s));
    VO_CHECK_HIP(c, hipMemcpyAsync(d_st, status, n, hipMemcpyHostToDevice, s));
    rc = vo_sdm_enqueue(c, s, has_map ? d_mi : nullptr, has_map ? d_ms : nullptr, has_map ? d_mn : nullptr, d_d, d_sg, d_st, width, height, bf, prm,
                        d_oi, d_os, d_on, origin ? d_og : nullptr, d_counts);
    if (rc) {
      (void)hipStreamSynchronize(s);  // (the copies read the caller's memory)
      return rc;
    }
    VO_CHECK_HIP(c, hipMemcpyAsync(invd, d_oi, n * sizeof(float), hipMemcpyDeviceToHost, s));
    VO_CHECK_HIP(c, hipMemcpyAsync(sigma, d_os, n * sizeof(float), hipMemcpyDeviceToHost, s));
    VO_CHECK_HIP(c, hipMemcpyAsync(n_obs, d_on, n, hipMemcpyDeviceToHost, s));
    if (origin) VO_CHECK_HIP(c, hipMemcpyAsync(origin, d_og, n, hipMemcpyDeviceToHost, s));
  }
  unsigned long long cnt[SDM_ORIGINS] = {0, 0, 0, 0, 0, 0};  // (the counts are host integers also with device planes)
  if (counts) VO_CHECK_HIP(c, hipMemcpyAsync(cnt, d_counts, sizeof(cnt), hipMemcpyDeviceToHost, s));
  VO_CHECK_HIP(c, hipStreamSynchronize(s));
  if (counts)
    for (int k = 0; k < SDM_ORIGINS; ++k) counts[k] = cnt[k];
  return VO_OK;
}

// ---- StereoVO: the world option's sources VO_SEMIDENSE_WORLD_DENSE and _MERGED ---------------------------------------------------------
// One allocation, made by vo_svo_set_semidense_world at the first enable of such a source: the counts, the outgoing keyframe's dense
// planes (9 bytes a pixel) and the merged planes with origin (10 bytes a pixel), for max_width x max_height. One rule for both values
// of the dense option's `every`: at a keyframe the dense result is copied, device to device on the side stream behind the dense
// launches (and the speckle filter's), into the option's own planes; the merge at the keyframe's end reads that copy.
struct SdmPlanes {
  unsigned long long *counts;
  float *disp, *sigma_invd, *invd, *sigma;
  uint8_t *status, *n_obs, *origin;
};
static SdmPlanes svo_sdm_planes(const vo_svo_semidense_world &w) {
  const size_t ne = w.mg.np_max;
  SdmPlanes p;
  p.counts = (unsigned long long *)w.mg.buf;
  float *f = (float *)((char *)w.mg.buf + SDM_HEAD);
  p.disp = f, p.sigma_invd = f + ne, p.invd = f + 2 * ne, p.sigma = f + 3 * ne;
  uint8_t *u = (uint8_t *)(f + 4 * ne);
  p.status = u, p.n_obs = u + ne, p.origin = u + 2 * ne;
  return p;
}

int vo_svo_sdm_alloc(vo_svo *s) {
  vo_ctx *c = s->c;
  vo_svo_semidense_world &w = s->sdw;
  if (w.mg.buf) return VO_OK;
  const size_t n = (size_t)c->cfg.max_width * (size_t)c->cfg.max_height, ne = (n + 15) & ~(size_t)15;
  VO_CHECK_HIP(c, hipSetDevice(c->device));
  if (vo_dev_malloc(c, &w.mg.buf, SDM_HEAD + 19 * ne) != hipSuccess) {
    (void)hipGetLastError();
    w.mg.buf = nullptr;
    VO_FAIL(c, VO_ERR_HIP, "vo_svo_set_semidense_world: the merged source's planes (%zu bytes) could not be allocated", SDM_HEAD + 19 * ne);
  }
  w.mg.np_max = ne;
  return VO_OK;
}

void vo_svo_sdm_free(vo_svo *s) {
  vo_svo_semidense_world &w = s->sdw;
  if (!w.mg.buf) return;
  (void)hipSetDevice(s->c->device);
  (void)hipStreamSynchronize(s->c->stream2);  // (the copy behind the last dense result has no event of its own)
  (void)hipFree(w.mg.buf);
  w.mg.buf = nullptr;
}

// called by vo_svo_dense_stereo_enqueue behind its launches, in front of its event: the frame is the temporal option's current keyframe
// and the world option's source reads the dense result — its planes are kept
int vo_svo_sdm_keep_dense(vo_svo *s, int frame_id) {
  vo_ctx *c = s->c;
  vo_svo_semidense_world &w = s->sdw;
  const vo_svo_dense_stereo &d = s->ds;
  if (!w.on || w.source < VO_SEMIDENSE_WORLD_DENSE || !w.mg.buf) return VO_OK;
  if (!s->sdt.on || !s->sdt.have || s->sdt.frame_id != frame_id) return VO_OK;  // not a keyframe of the map
  const size_t n = (size_t)d.w * (size_t)d.h;
  if (n > w.mg.np_max) VO_FAIL(c, VO_ERR_SIZE, "world map: a %d x %d dense result exceeds vo_config.max_width x max_height", d.w, d.h);
  const SdmPlanes p = svo_sdm_planes(w);
  hipStream_t side = c->stream2;
  VO_CHECK_HIP(c, hipMemcpyAsync(p.disp, d.buf.disp, n * sizeof(float), hipMemcpyDeviceToDevice, side));
  VO_CHECK_HIP(c, hipMemcpyAsync(p.sigma_invd, d.buf.sigma, n * sizeof(float), hipMemcpyDeviceToDevice, side));
  VO_CHECK_HIP(c, hipMemcpyAsync(p.status, d.buf.status, n, hipMemcpyDeviceToDevice, side));
  w.mg.ds_have = true;
  w.mg.ds_w = d.w, w.mg.ds_h = d.h, w.mg.ds_frame_id = frame_id;
  w.mg.ds_bf = d.prm.bf;
  return VO_OK;
}

// called by vo_svo_semidense_world_enqueue for the two sources: the merge launch on the side stream; *ok = false, with nothing
// launched, where the outgoing keyframe has no dense result of its own
int vo_svo_sdm_merge(vo_svo *s, const float **invd, const float **sigma, const uint8_t **n_obs, bool *ok) {
  vo_ctx *c = s->c;
  vo_svo_semidense_world &w = s->sdw;
  const vo_svo_semidense_temporal &t = s->sdt;
  *ok = false;
  if (!w.mg.buf || !s->ds.on || !w.mg.ds_have || w.mg.ds_frame_id != t.frame_id || w.mg.ds_w != t.w || w.mg.ds_h != t.h) return VO_OK;
  const SdmPlanes p = svo_sdm_planes(w);
  const bool with_map = w.source == VO_SEMIDENSE_WORLD_MERGED;
  const int rc = vo_sdm_enqueue(c, c->stream2, with_map ? t.buf.invd : nullptr, with_map ? t.buf.sigma : nullptr, with_map ? t.buf.n_obs : nullptr,
                                p.disp, p.sigma_invd, p.status, t.w, t.h, w.mg.ds_bf, &w.mg.prm, p.invd, p.sigma, p.n_obs, p.origin, p.counts);
  if (rc) return rc;
  w.mg.have = true;
  w.mg.w = t.w, w.mg.h = t.h, w.mg.frame_id = t.frame_id;
  *invd = p.invd, *sigma = p.sigma, *n_obs = p.n_obs;
  *ok = true;
  return VO_OK;
}

extern "C" int vo_svo_set_semidense_world_merge(vo_svo *s, const vo_semidense_map_merge_params *prm) {
  if (!s) return VO_ERR_INVALID;
  vo_ctx *c = s->c;
  if (s->pending) VO_FAIL(c, VO_ERR_INVALID, "vo_svo_set_semidense_world_merge: a frame is in flight: call vo_svo_result first");
  if (s->mono) VO_FAIL(c, VO_ERR_INVALID, "vo_svo_set_semidense_world_merge: a stereo driver only");
  vo_semidense_map_merge_params p;
  vo_semidense_map_merge_default_params(&p);
  if (prm) {
    const int rc = vo_sdm_check_params(c, prm);
    if (rc) return rc;
    p = *prm;
  }
  s->sdw.mg.prm = p;
  return VO_OK;
}

extern "C" int vo_svo_get_semidense_world_source(vo_svo *s, float *invd, float *sigma, uint8_t *n_obs, uint8_t *origin, int *width, int *height,
                                                 int *frame_id, uint64_t *counts) {
  if (!s || !width || !height) return VO_ERR_INVALID;
  vo_ctx *c = s->c;
  if (s->pending) VO_FAIL(c, VO_ERR_INVALID, "vo_svo_get_semidense_world_source: a frame is in flight: call vo_svo_result first");
  const vo_svo_semidense_world &w = s->sdw;
  if (!w.on || !w.wm) VO_FAIL(c, VO_ERR_INVALID, "vo_svo_get_semidense_world_source: the option is off: vo_svo_set_semidense_world");
  *width = *height = 0;
  if (frame_id) *frame_id = -1;
  if (counts) memset(counts, 0, SDM_ORIGINS * sizeof(uint64_t));
  if (!w.mg.buf || !w.mg.have) return VO_OK;  // no merge has been enqueued
  VO_CHECK_HIP(c, hipSetDevice(c->device));
  if (s->sd.have) VO_CHECK_HIP(c, hipEventSynchronize(s->sd.done));  // the side stream's last launch only
  const SdmPlanes p = svo_sdm_planes(w);
  const size_t n = (size_t)w.mg.w * (size_t)w.mg.h;
  *width = w.mg.w, *height = w.mg.h;
  if (frame_id) *frame_id = w.mg.frame_id;
  if (invd) VO_CHECK_HIP(c, hipMemcpy(invd, p.invd, n * sizeof(float), hipMemcpyDeviceToHost));
  if (sigma) VO_CHECK_HIP(c, hipMemcpy(sigma, p.sigma, n * sizeof(float), hipMemcpyDeviceToHost));
  if (n_obs) VO_CHECK_HIP(c, hipMemcpy(n_obs, p.n_obs, n, hipMemcpyDeviceToHost));
  if (origin) VO_CHECK_HIP(c, hipMemcpy(origin, p.origin, n, hipMemcpyDeviceToHost));
  if (counts) {
    unsigned long long cnt[SDM_ORIGINS];
    VO_CHECK_HIP(c, hipMemcpy(cnt, p.counts, sizeof(cnt), hipMemcpyDeviceToHost));
    for (int k = 0; k < SDM_ORIGINS; ++k) counts[k] = cnt[k];
  }
  return VO_OK;
}
