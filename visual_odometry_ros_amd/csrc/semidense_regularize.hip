// semidense_regularize.hip — outlier removal, fill and smoothing of a semi-dense map (include/vo_hip.h, "Semi-dense regularisation";
// DESIGN.md §23): the operator (vo_semidense_map_regularize) and StereoVO's hook (vo_svo_set_semidense_regularize,
// vo_svo_get_semidense_regularized*; the launch is placed by vo_svo_semidense_temporal_enqueue). semidense_regularize_device.hpp has
// the kernel.
#include "stereo_vo.hpp"
#include "vo_internal.hpp"
#include "vo_kernels.hpp"

#include <math.h>

#include "semidense_regularize_device.hpp"

extern "C" int vo_semidense_regularize_default_params(vo_semidense_regularize_params *p) {
  if (!p) return VO_ERR_INVALID;
  memset(p, 0, sizeof(*p));
  p->radius = 2;
  p->chi = 2.0f;
  p->dist_sigma = 0.01f;
  p->min_support = 1;
  p->fill_min = 8;
  p->g_min = 20;
  return VO_OK;
}

static int sdr_check_params(vo_ctx *c, const vo_semidense_regularize_params *p) {
  if (p->radius < 1 || p->radius > SDR_MAX_R) VO_FAIL(c, VO_ERR_INVALID, "semi-dense regularisation: radius=%d: expected 1..%d", p->radius, SDR_MAX_R);
  if (!(p->chi > 0.0f) || !isfinite(p->chi)) VO_FAIL(c, VO_ERR_INVALID, "semi-dense regularisation: chi must be positive and finite");
  if (!(p->dist_sigma >= 0.0f) || !isfinite(p->dist_sigma)) VO_FAIL(c, VO_ERR_INVALID, "semi-dense regularisation: dist_sigma is finite and >= 0");
  if (p->min_support < 0 || p->min_support > 48) VO_FAIL(c, VO_ERR_INVALID, "semi-dense regularisation: min_support=%d: expected 0..48", p->min_support);
  if (p->fill_min < 0 || p->fill_min > 48) VO_FAIL(c, VO_ERR_INVALID, "semi-dense regularisation: fill_min=%d: expected 0..48", p->fill_min);
  if (p->g_min < 1 || p->g_min > 360) VO_FAIL(c, VO_ERR_INVALID, "semi-dense regularisation: g_min=%d: expected 1..360", p->g_min);
  return VO_OK;
}

// ---- buffers ----------------------------------------------------------------------------------------------------------------------
// One allocation. The context's operator (host planes) has a plane for the caller's mask; a driver reads the temporal option's copy.
int vo_sdr_buffers_alloc(vo_ctx *c, vo_sdr_buffers *b, bool driver) {
  if (b->base) return VO_OK;
  const size_t n = (size_t)c->cfg.max_width * (size_t)c->cfg.max_height;
  VO_CHECK_HIP(c, hipSetDevice(c->device));
  VO_CHECK_HIP(c, vo_dev_malloc(c, &b->base, n * (2 * sizeof(float) + (driver ? 2 : 3)) + 64));
  b->invd = (float *)b->base;
  b->sigma = b->invd + n;
  b->n_obs = (uint8_t *)(b->sigma + n);
  b->rstatus = b->n_obs + n;
  if (!driver) b->mask = b->rstatus + n;
  b->npix = n;
  return VO_OK;
}
void vo_sdr_buffers_free(vo_sdr_buffers *b) {
  if (b->base) (void)hipFree(b->base);
  *b = vo_sdr_buffers();
}

struct vo_semidense_regularize_state {
  vo_sdr_buffers buf;
};
void vo_semidense_regularize_free(vo_ctx *c) {
  if (!c->semidense_r) return;
  vo_sdr_buffers_free(&c->semidense_r->buf);
  delete c->semidense_r;
  c->semidense_r = nullptr;
}

// ---- the launch -------------------------------------------------------------------------------------------------------------------
// On c->stream, DEVICE planes throughout; mask may be null.
static int sdr_enqueue(vo_ctx *c, const float *invd, const float *sigma, const uint8_t *n_obs, const uint8_t *d_key, int key_stride,
                       const uint8_t *mask, int mask_stride, int W, int H, const vo_semidense_regularize_params *p, float *invd_r, float *sigma_r,
                       uint8_t *n_obs_r, uint8_t *rstatus) {
  const int rc = sdr_check_params(c, p);
  if (rc) return rc;
  if (W < 3 || H < 3 || W > 65535 || H > 65535) VO_FAIL(c, VO_ERR_SIZE, "semi-dense regularisation: the map must have 3 .. 65535 pixels a side");
  if (key_stride < W) VO_FAIL(c, VO_ERR_INVALID, "semi-dense regularisation: key_stride %d below the width %d", key_stride, W);
  SdrArgs a;
  memset(&a, 0, sizeof(a));
  a.invd = invd;
  a.sigma = sigma;
  a.n_obs = n_obs;
  a.Lk = d_key;
  a.strideK = key_stride;
  a.W = W;
  a.H = H;
  a.mask = mask;
  a.mask_stride = mask_stride;
  a.radius = p->radius;
  a.min_support = p->min_support;
  a.fill_min = p->fill_min;
  a.g_min2 = p->g_min * p->g_min;
  a.chi2 = p->chi * p->chi;  // (host code: -ffp-contract=off)
  a.dist2 = p->dist_sigma * p->dist_sigma;
  a.invd_r = invd_r;
  a.sigma_r = sigma_r;
  a.n_obs_r = n_obs_r;
  a.rstatus = rstatus;
  vo_prof_begin(c, VO_K_AUX);
  hipLaunchKernelGGL(semidense_regularize_kernel, dim3((unsigned)((W + SDR_TW - 1) / SDR_TW), (unsigned)((H + SDR_TH - 1) / SDR_TH)), dim3(SDR_NT), 0,
                     c->stream, a);
  vo_prof_end(c);
  VO_CHECK_HIP(c, hipGetLastError());
  return VO_OK;
}

extern "C" int vo_semidense_map_regularize(vo_ctx *c, const float *invd, const float *sigma, const uint8_t *n_obs, const uint8_t *key_plane,
                                           int key_stride, int key_on_device, const uint8_t *mask, int width, int height,
                                           const vo_semidense_regularize_params *prm, float *invd_r, float *sigma_r, uint8_t *n_obs_r,
                                           uint8_t *rstatus, int on_device) {
  if (!c || !invd || !sigma || !n_obs || !key_plane || !prm || !invd_r || !sigma_r || !n_obs_r || !rstatus) return VO_ERR_INVALID;
  const void *ins[5] = {invd, sigma, n_obs, key_plane, mask}, *outs[4] = {invd_r, sigma_r, n_obs_r, rstatus};
  for (int i = 0; i < 4; ++i) {
    for (int j = 0; j < 5; ++j)
      if (outs[i] == ins[j]) VO_FAIL(c, VO_ERR_INVALID, "semi-dense regularisation: an output plane may not be an input plane");
    for (int j = 0; j < i; ++j)
      if (outs[i] == outs[j]) VO_FAIL(c, VO_ERR_INVALID, "semi-dense regularisation: the output planes may not be one another");
  }
  int rc = sdr_check_params(c, prm);
  if (rc) return rc;
  if (width < 3 || height < 3 || width > 65535 || height > 65535)
    VO_FAIL(c, VO_ERR_SIZE, "semi-dense regularisation: the map must have 3 .. 65535 pixels a side");
  if (width > c->cfg.max_width || height > c->cfg.max_height)
    VO_FAIL(c, VO_ERR_SIZE, "%d x %d planes exceed vo_config.max_width x max_height", width, height);
  if (key_stride < width) VO_FAIL(c, VO_ERR_INVALID, "semi-dense regularisation: key_stride %d below the width %d", key_stride, width);
  VO_CHECK_HIP(c, hipSetDevice(c->device));
  hipStream_t s = c->stream;
  const int W = width, H = height;
  const size_t np = (size_t)W * (size_t)H;
  vo_sdt_buffers *b = nullptr;  // the map's and the key plane's device copies
  if (!key_on_device || !on_device) {
    rc = vo_sdt_ctx_buffers(c, &b);
    if (rc) return rc;
  }
  const uint8_t *d_key = key_plane;
  int d_stride = key_stride;
  if (!key_on_device) {
    VO_CHECK_HIP(c, hipMemcpy2DAsync(b->key, (size_t)W, key_plane, (size_t)key_stride, (size_t)W, (size_t)H, hipMemcpyHostToDevice, s));
    d_key = b->key;
    d_stride = W;
  }
  if (on_device) {
    rc = sdr_enqueue(c, invd, sigma, n_obs, d_key, d_stride, mask, W, W, H, prm, invd_r, sigma_r, n_obs_r, rstatus);
    if (rc) {
      (void)hipStreamSynchronize(s);  // (the copy reads the caller's memory)
      return rc;
    }
    VO_CHECK_HIP(c, hipStreamSynchronize(s));
    return VO_OK;
  }
  if (!c->semidense_r) c->semidense_r = new vo_semidense_regularize_state();
  vo_sdr_buffers *o = &c->semidense_r->buf;
  rc = vo_sdr_buffers_alloc(c, o, false);
  if (rc) {
    (void)hipStreamSynchronize(s);
    return rc;
  }
  VO_CHECK_HIP(c, hipMemcpyAsync(b->invd, invd, np * sizeof(float), hipMemcpyHostToDevice, s));
  VO_CHECK_HIP(c, hipMemcpyAsync(b->sigma, sigma, np * sizeof(float), hipMemcpyHostToDevice, s));
  VO_CHECK_HIP(c, hipMemcpyAsync(b->n_obs, n_obs, np, hipMemcpyHostToDevice, s));
  if (mask) VO_CHECK_HIP(c, hipMemcpyAsync(o->mask, mask, np, hipMemcpyHostToDevice, s));
  rc = sdr_enqueue(c, b->invd, b->sigma, b->n_obs, d_key, d_stride, mask ? o->mask : nullptr, W, W, H, prm, o->invd, o->sigma, o->n_obs, o->rstatus);
  if (rc) {
    (void)hipStreamSynchronize(s);  // (the copies read the caller's memory)
    return rc;
  }
  VO_CHECK_HIP(c, hipMemcpyAsync(invd_r, o->invd, np * sizeof(float), hipMemcpyDeviceToHost, s));
  VO_CHECK_HIP(c, hipMemcpyAsync(sigma_r, o->sigma, np * sizeof(float), hipMemcpyDeviceToHost, s));
  VO_CHECK_HIP(c, hipMemcpyAsync(n_obs_r, o->n_obs, np, hipMemcpyDeviceToHost, s));
  VO_CHECK_HIP(c, hipMemcpyAsync(rstatus, o->rstatus, np, hipMemcpyDeviceToHost, s));
  VO_CHECK_HIP(c, hipStreamSynchronize(s));
  return VO_OK;
}

// ---- StereoVO's hook ------------------------------------------------------------------------------------------------------------------
// Called by vo_svo_semidense_temporal_enqueue behind the launch that wrote the map — the seed, the propagation's resolve (the map's
// planes are then the set that is current after its swap) or the temporal launch — and in front of the record of `sd.done`, so that
// the guard and every getter wait for it as the side stream's last launch. It reads the temporal option's map, key plane and mask
// copy and writes this option's planes; nothing reads those on the device.
int vo_svo_semidense_regularize_enqueue(vo_svo *s) {
  vo_ctx *c = s->c;
  const vo_svo_semidense_temporal &t = s->sdt;
  vo_svo_semidense_regularize &r = s->sdr;
  if (!t.have) return VO_OK;
  hipStream_t keep = c->stream;
  c->stream = c->stream2;
  const int rc = sdr_enqueue(c, t.buf.invd, t.buf.sigma, t.buf.n_obs, t.buf.key, t.w, t.mask_on ? t.buf.mask : nullptr, t.w, t.w, t.h, &r.prm,
                             r.buf.invd, r.buf.sigma, r.buf.n_obs, r.buf.rstatus);
  c->stream = keep;
  if (rc) return rc;
  r.have = true;
  r.w = t.w;
  r.h = t.h;
  r.frame_id = t.frame_id;
  r.n_fused = t.n_fused;
  memcpy(r.T_wk, t.T_wk, sizeof(r.T_wk));
  return VO_OK;
}

void vo_svo_semidense_regularize_free(vo_svo *s) {
  vo_sdr_buffers_free(&s->sdr.buf);
  s->sdr = vo_svo_semidense_regularize();
}

extern "C" int vo_svo_set_semidense_regularize(vo_svo *s, const vo_semidense_regularize_params *prm) {
  if (!s) return VO_ERR_INVALID;
  vo_ctx *c = s->c;
  if (s->pending) VO_FAIL(c, VO_ERR_INVALID, "vo_svo_set_semidense_regularize: a frame is in flight: call vo_svo_result first");
  if (s->mono) VO_FAIL(c, VO_ERR_INVALID, "vo_svo_set_semidense_regularize: a stereo driver only");
  vo_svo_semidense_regularize &r = s->sdr;
  if (!prm) {
    r.on = false;
    r.have = false;
    return VO_OK;
  }
  if (!s->sdt.on || !s->sd.on)
    VO_FAIL(c, VO_ERR_INVALID, "vo_svo_set_semidense_regularize: needs the temporal option: vo_svo_set_semidense_temporal first");
  int rc = sdr_check_params(c, prm);
  if (rc) return rc;
  rc = vo_sdr_buffers_alloc(c, &r.buf, true);  // the option's only allocation, at the first enable
  if (rc) return rc;
  r.prm = *prm;
  r.on = true;
  return VO_OK;
}

static int svo_sdr_ready(vo_svo *s, const char *who) {
  vo_ctx *c = s->c;
  if (s->pending) VO_FAIL(c, VO_ERR_INVALID, "%s: a frame is in flight: call vo_svo_result first", who);
  if (!s->sdr.on || !s->sdt.on || !s->sd.on) VO_FAIL(c, VO_ERR_INVALID, "%s: the option is off: vo_svo_set_semidense_regularize", who);
  VO_CHECK_HIP(c, hipSetDevice(c->device));
  if (s->sd.have) VO_CHECK_HIP(c, hipEventSynchronize(s->sd.done));  // the side stream's last launch only
  return VO_OK;
}

extern "C" int vo_svo_get_semidense_regularized(vo_svo *s, float *invd, float *sigma, uint8_t *n_obs, uint8_t *rstatus, int *width, int *height,
                                                int *frame_id, float T_wc[16], int *n_fused) {
  if (!s || !width || !height) return VO_ERR_INVALID;
  const int rc = svo_sdr_ready(s, "vo_svo_get_semidense_regularized");
  if (rc) return rc;
  vo_ctx *c = s->c;
  const vo_svo_semidense_regularize &r = s->sdr;
  *width = *height = 0;
  if (frame_id) *frame_id = -1;
  if (n_fused) *n_fused = 0;
  if (!r.have) return VO_OK;  // no launch since the option was switched on
  *width = r.w;
  *height = r.h;
  if (frame_id) *frame_id = r.frame_id;
  if (n_fused) *n_fused = r.n_fused;
  if (T_wc) memcpy(T_wc, r.T_wk, sizeof(r.T_wk));
  const size_t n = (size_t)r.w * (size_t)r.h;
  if (invd) VO_CHECK_HIP(c, hipMemcpy(invd, r.buf.invd, n * sizeof(float), hipMemcpyDeviceToHost));
  if (sigma) VO_CHECK_HIP(c, hipMemcpy(sigma, r.buf.sigma, n * sizeof(float), hipMemcpyDeviceToHost));
  if (n_obs) VO_CHECK_HIP(c, hipMemcpy(n_obs, r.buf.n_obs, n, hipMemcpyDeviceToHost));
  if (rstatus) VO_CHECK_HIP(c, hipMemcpy(rstatus, r.buf.rstatus, n, hipMemcpyDeviceToHost));
  return VO_OK;
}

extern "C" int vo_svo_get_semidense_regularized_points(vo_svo *s, int world, int min_obs, int cap, float *xyz, float *sigma, uint16_t *pixel, int *n,
                                                       int *frame_id) {
  if (!s || !n || cap < 0 || (cap > 0 && !xyz)) return VO_ERR_INVALID;
  const int rc = svo_sdr_ready(s, "vo_svo_get_semidense_regularized_points");
  if (rc) return rc;
  if (min_obs < 1 || min_obs > 255) VO_FAIL(s->c, VO_ERR_INVALID, "semi-dense map: min_obs=%d: expected 1..255", min_obs);
  vo_svo_semidense_regularize &r = s->sdr;
  *n = 0;
  if (frame_id) *frame_id = r.have ? r.frame_id : -1;
  if (!r.have) return VO_OK;
  return vo_sdt_points(s->c, &s->sd.buf, r.buf.invd, r.buf.sigma, r.buf.n_obs, r.w, r.h, s->prm.frame.Kl, world ? r.T_wk : nullptr, min_obs, cap,
                       xyz, sigma, pixel, n);
}
