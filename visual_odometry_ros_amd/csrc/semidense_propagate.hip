// semidense_propagate.hip — the fused semi-dense map carried over to the next keyframe (include/vo_hip.h, "Semi-dense propagation";
// DESIGN.md §19): the operator (vo_semidense_map_propagate) and StereoVO's hook (vo_svo_set_semidense_propagate,
// vo_svo_get_semidense_origin; the launches are placed by vo_svo_semidense_temporal_enqueue). semidense_propagate_device.hpp has
// the kernels.
#include "stereo_vo.hpp"
#include "vo_internal.hpp"
#include "vo_kernels.hpp"

#include <math.h>

#include "semidense_propagate_device.hpp"

extern "C" int vo_semidense_propagate_default_params(vo_semidense_propagate_params *p) {
  if (!p) return VO_ERR_INVALID;
  memset(p, 0, sizeof(*p));
  p->min_obs = 1;
  p->max_diff = 30;
  p->chi = 3.0f;
  p->sigma_add = 0.01f;
  return VO_OK;
}

static int sdp_check_params(vo_ctx *c, const vo_semidense_propagate_params *p) {
  if (p->min_obs < 1 || p->min_obs > 255) VO_FAIL(c, VO_ERR_INVALID, "semi-dense propagation: min_obs=%d: expected 1..255", p->min_obs);
  if (p->max_diff < 0 || p->max_diff > 255) VO_FAIL(c, VO_ERR_INVALID, "semi-dense propagation: max_diff=%d: expected 0..255", p->max_diff);
  if (!(p->chi > 0.0f) || !isfinite(p->chi)) VO_FAIL(c, VO_ERR_INVALID, "semi-dense propagation: chi must be positive and finite");
  if (!(p->sigma_add >= 0.0f) || !isfinite(p->sigma_add)) VO_FAIL(c, VO_ERR_INVALID, "semi-dense propagation: sigma_add is finite and >= 0");
  return VO_OK;
}

// ---- buffers ----------------------------------------------------------------------------------------------------------------------
int vo_sdp_buffers_alloc(vo_ctx *c, vo_sdp_buffers *b, bool driver) {
  if (b->base) return VO_OK;
  const size_t n = (size_t)c->cfg.max_width * (size_t)c->cfg.max_height;
  VO_CHECK_HIP(c, hipSetDevice(c->device));
  VO_CHECK_HIP(c, vo_dev_malloc(c, &b->base, n * (sizeof(unsigned long long) + (driver ? 2 : 3) * sizeof(float) + 3) + 64));
  b->keys = (unsigned long long *)b->base;
  b->invd = (float *)(b->keys + n);
  b->sigma = b->invd + n;
  float *end = b->sigma + n;
  if (!driver) b->src = (int32_t *)end, end += n;
  b->n_obs = (uint8_t *)end;
  b->tstatus = b->n_obs + n;
  b->origin = b->tstatus + n;
  b->npix = n;
  // zeroed once, and the host waits for it: every resolve launch, on whichever stream, leaves the plane clean again
  VO_CHECK_HIP(c, hipMemsetAsync(b->keys, 0, n * sizeof(unsigned long long), c->stream));
  VO_CHECK_HIP(c, hipStreamSynchronize(c->stream));
  return VO_OK;
}
void vo_sdp_buffers_free(vo_sdp_buffers *b) {
  if (b->base) (void)hipFree(b->base);
  *b = vo_sdp_buffers();
}

struct vo_semidense_propagate_state {
  vo_sdp_buffers buf;
};
void vo_semidense_propagate_free(vo_ctx *c) {
  if (!c->semidense_p) return;
  vo_sdp_buffers_free(&c->semidense_p->buf);
  delete c->semidense_p;
  c->semidense_p = nullptr;
}

// ---- the launches -------------------------------------------------------------------------------------------------------------------
// The arguments of both launches: DEVICE planes throughout. mask: the new keyframe's (p == null: none).
static int sdp_args(vo_ctx *c, SdpArgs *a, const float *old_invd, const float *old_sigma, const uint8_t *old_n_obs, const uint8_t *d_key,
                    int key_stride, int slot_new, const vo_mask_view &mask, const float *disp, const float *sigma_invd, const uint8_t *status, float bf,
                    const float K[4], const float T_ba[16], const vo_semidense_propagate_params *p, unsigned long long *keys, float *invd, float *sigma,
                    uint8_t *n_obs, uint8_t *tstatus, uint8_t *origin, int32_t *src) {
  const int rc = sdp_check_params(c, p);
  if (rc) return rc;
  if (slot_new < 0 || slot_new >= c->cfg.n_slots || c->slots[slot_new].n_levels <= 0) VO_FAIL(c, VO_ERR_INVALID, "slot holds no image");
  const vo_pyramid &P = c->slots[slot_new];
  if (P.w < 3 || P.h < 3 || P.w > 65535 || P.h > 65535 || (long long)P.w * P.h > 0x7FFFFFFFll)
    VO_FAIL(c, VO_ERR_SIZE, "semi-dense propagation: the image must have 3 .. 65535 pixels a side and fewer than 2^31 in all");
  if (key_stride < P.w) VO_FAIL(c, VO_ERR_INVALID, "semi-dense propagation: key_stride %d below the width %d", key_stride, P.w);
  if (!(K[0] > 0.0f) || !(K[1] > 0.0f)) VO_FAIL(c, VO_ERR_INVALID, "semi-dense propagation: fx, fy must be positive");
  if (!(bf > 0.0f) || !isfinite(bf)) VO_FAIL(c, VO_ERR_INVALID, "semi-dense propagation: bf (focal length x baseline) must be positive");
  for (int i = 0; i < 12; ++i)
    if (!isfinite(T_ba[i])) VO_FAIL(c, VO_ERR_INVALID, "semi-dense propagation: T_ba is not finite");
  if (mask.p && (mask.w != P.w || mask.h != P.h))
    VO_FAIL(c, VO_ERR_SIZE, "semi-dense propagation: the mask is %d x %d, the image %d x %d", mask.w, mask.h, P.w, P.h);
  memset(a, 0, sizeof(*a));
  a->invd_a = old_invd;
  a->sigma_a = old_sigma;
  a->n_obs_a = old_n_obs;
  a->La = d_key;
  a->Lb = P.lv[0].origin();
  a->strideA = key_stride;
  a->strideB = P.lv[0].stride;
  a->W = P.w;
  a->H = P.h;
  a->mask = mask.p;
  a->mask_stride = mask.stride;
  a->min_obs = p->min_obs;
  a->max_diff = p->max_diff;
  a->chi2 = p->chi * p->chi;  // (host code: -ffp-contract=off)
  a->sigma_add2 = p->sigma_add * p->sigma_add;
  a->fx = K[0], a->fy = K[1], a->cx = K[2], a->cy = K[3];
  sdp_pose(a, T_ba);
  a->keys = keys;
  a->disp = disp;
  a->sigma_invd = sigma_invd;
  a->status = status;
  a->bf = bf;
  a->invd = invd;
  a->sigma = sigma;
  a->n_obs = n_obs;
  a->tstatus = tstatus;
  a->origin = origin;
  a->src = src;
  return VO_OK;
}

static int sdp_launch(vo_ctx *c, const SdpArgs &a, bool scatter) {
  const unsigned nb = (unsigned)(((size_t)a.W * (size_t)a.H + SDP_NT - 1) / SDP_NT);
  vo_prof_begin(c, VO_K_AUX);
  if (scatter)
    hipLaunchKernelGGL(semidense_propagate_scatter_kernel, dim3(nb), dim3(SDP_NT), 0, c->stream, a);
  else
    hipLaunchKernelGGL(semidense_propagate_resolve_kernel, dim3(nb), dim3(SDP_NT), 0, c->stream, a);
  vo_prof_end(c);
  VO_CHECK_HIP(c, hipGetLastError());
  return VO_OK;
}

extern "C" int vo_semidense_map_propagate(vo_ctx *c, const float *old_invd, const float *old_sigma, const uint8_t *old_n_obs, const uint8_t *key_plane,
                                          int key_stride, int slot_new, const float *disparity, const float *sigma_invd, const uint8_t *status,
                                          float bf, const float K[4], const float T_ba[16], const vo_semidense_propagate_params *prm, float *invd,
                                          float *sigma, uint8_t *n_obs, uint8_t *tstatus, uint8_t *origin, int32_t *src, int on_device) {
  if (!c || !old_invd || !old_sigma || !old_n_obs || !key_plane || !disparity || !sigma_invd || !status || !K || !T_ba || !prm || !invd || !sigma ||
      !n_obs || !tstatus)
    return VO_ERR_INVALID;
  if (invd == old_invd || sigma == old_sigma || n_obs == old_n_obs)
    VO_FAIL(c, VO_ERR_INVALID, "semi-dense propagation: the new map's planes may not be the old map's");
  VO_CHECK_HIP(c, hipSetDevice(c->device));
  hipStream_t s = c->stream;
  if (slot_new < 0 || slot_new >= c->cfg.n_slots || c->slots[slot_new].n_levels <= 0) VO_FAIL(c, VO_ERR_INVALID, "slot holds no image");
  const int W = c->slots[slot_new].w, H = c->slots[slot_new].h;
  if (key_stride < W) VO_FAIL(c, VO_ERR_INVALID, "semi-dense propagation: key_stride %d below the width %d", key_stride, W);
  const size_t np = (size_t)W * (size_t)H;
  if (!c->semidense_p) c->semidense_p = new vo_semidense_propagate_state();
  vo_sdp_buffers *o = &c->semidense_p->buf;
  int rc = vo_sdp_buffers_alloc(c, o, false);
  if (rc) return rc;
  if (vo_slot_acquire(c, slot_new) < 0) return VO_ERR_HIP;
  vo_mask_view mv;
  rc = vo_slot_mask_acquire(c, slot_new, &mv);
  if (rc) return rc;
  SdpArgs a;
  const int stage = c->dbg[VO_DBG_SDP_STAGE];  // (measurement: one of the two launches alone)
  if (on_device) {
    rc = sdp_args(c, &a, old_invd, old_sigma, old_n_obs, key_plane, key_stride, slot_new, mv, disparity, sigma_invd, status, bf, K, T_ba, prm, o->keys,
                  invd, sigma, n_obs, tstatus, origin, src);
    if (rc) return rc;
    rc = stage != 2 ? sdp_launch(c, a, true) : VO_OK;
    if (rc >= 0 && stage != 1) rc = sdp_launch(c, a, false);
    if (rc) return rc;
    VO_CHECK_HIP(c, hipStreamSynchronize(s));
    return VO_OK;
  }
  vo_sd_buffers *in;   // the static planes' device copies
  vo_sdt_buffers *m;   // the old map's and the key plane's
  rc = vo_sd_ctx_buffers(c, &in);
  if (rc >= 0) rc = vo_sdt_ctx_buffers(c, &m);
  if (rc) return rc;
  rc = sdp_args(c, &a, m->invd, m->sigma, m->n_obs, m->key, W, slot_new, mv, in->disp, in->sigma, in->status, bf, K, T_ba, prm, o->keys, o->invd,
                o->sigma, o->n_obs, o->tstatus, origin ? o->origin : nullptr, src ? o->src : nullptr);
  if (rc) return rc;  // (before any copy reads the caller's memory)
  VO_CHECK_HIP(c, hipMemcpyAsync(m->invd, old_invd, np * sizeof(float), hipMemcpyHostToDevice, s));
  VO_CHECK_HIP(c, hipMemcpyAsync(m->sigma, old_sigma, np * sizeof(float), hipMemcpyHostToDevice, s));
  VO_CHECK_HIP(c, hipMemcpyAsync(m->n_obs, old_n_obs, np, hipMemcpyHostToDevice, s));
  VO_CHECK_HIP(c, hipMemcpy2DAsync(m->key, (size_t)W, key_plane, (size_t)key_stride, (size_t)W, (size_t)H, hipMemcpyHostToDevice, s));
  VO_CHECK_HIP(c, hipMemcpyAsync(in->disp, disparity, np * sizeof(float), hipMemcpyHostToDevice, s));
  VO_CHECK_HIP(c, hipMemcpyAsync(in->sigma, sigma_invd, np * sizeof(float), hipMemcpyHostToDevice, s));
  VO_CHECK_HIP(c, hipMemcpyAsync(in->status, status, np, hipMemcpyHostToDevice, s));
  rc = stage != 2 ? sdp_launch(c, a, true) : VO_OK;
  if (rc >= 0 && stage != 1) rc = sdp_launch(c, a, false);
  if (rc) {
    (void)hipStreamSynchronize(s);  // (the copies read the caller's memory)
    return rc;
  }
  VO_CHECK_HIP(c, hipMemcpyAsync(invd, o->invd, np * sizeof(float), hipMemcpyDeviceToHost, s));
  VO_CHECK_HIP(c, hipMemcpyAsync(sigma, o->sigma, np * sizeof(float), hipMemcpyDeviceToHost, s));
  VO_CHECK_HIP(c, hipMemcpyAsync(n_obs, o->n_obs, np, hipMemcpyDeviceToHost, s));
  VO_CHECK_HIP(c, hipMemcpyAsync(tstatus, o->tstatus, np, hipMemcpyDeviceToHost, s));
  if (origin) VO_CHECK_HIP(c, hipMemcpyAsync(origin, o->origin, np, hipMemcpyDeviceToHost, s));
  if (src) VO_CHECK_HIP(c, hipMemcpyAsync(src, o->src, np * sizeof(int32_t), hipMemcpyDeviceToHost, s));
  VO_CHECK_HIP(c, hipStreamSynchronize(s));
  return VO_OK;
}

// ---- StereoVO's hook ------------------------------------------------------------------------------------------------------------------
// Both are called by vo_svo_semidense_temporal_enqueue at a keyframe, on the side stream behind the static launch of the new pair
// (which has ordered the side stream behind the new left slot's pyramid). The old map is the temporal option's current set of planes,
// the new one this option's set; the resolve swaps them.
static int svo_sdp_args(vo_svo *s, SdpArgs *a, const vo_mask_view &mv) {
  vo_svo_semidense &d = s->sd;
  vo_svo_semidense_temporal &t = s->sdt;
  vo_svo_semidense_propagate &p = s->sdp;
  return sdp_args(s->c, a, t.buf.invd, t.buf.sigma, t.buf.n_obs, t.buf.key, d.w, d.slot_l, mv, d.buf.disp, d.buf.sigma, d.buf.status, d.prm.bf,
                  s->prm.frame.Kl, p.T_ba, &p.prm, p.buf.keys, p.buf.invd, p.buf.sigma, p.buf.n_obs, p.buf.tstatus, p.buf.origin, nullptr);
}

int vo_svo_semidense_propagate_scatter(vo_svo *s, int slot_l, const float T_wc[16]) {
  vo_ctx *c = s->c;
  vo_svo_semidense_propagate &p = s->sdp;
  float T_bw[16];
  svo_inv_se3(T_wc, T_bw);  // T_ba = inverseSE3(T_wc_new) * T_wk_old, both in float, in svo_mul44's order
  svo_mul44(T_bw, s->sdt.T_wk, p.T_ba);
  hipStream_t keep = c->stream;
  c->stream = c->stream2;
  vo_mask_view mv;
  int rc = vo_slot_mask_acquire(c, slot_l, &mv);
  SdpArgs a;
  if (rc >= 0) rc = svo_sdp_args(s, &a, mv);
  if (rc >= 0) rc = sdp_launch(c, a, true);
  c->stream = keep;
  return rc;
}

int vo_svo_semidense_propagate_resolve(vo_svo *s, bool chain) {
  vo_ctx *c = s->c;
  vo_svo_semidense_temporal &t = s->sdt;
  vo_svo_semidense_propagate &p = s->sdp;
  if (!chain) {  // no scatter ran: the keys are all 0, the pose is not used
    memset(p.T_ba, 0, sizeof(p.T_ba));
    p.T_ba[0] = p.T_ba[5] = p.T_ba[10] = p.T_ba[15] = 1.0f;
  }
  hipStream_t keep = c->stream;
  c->stream = c->stream2;
  vo_mask_view mv;  // (the resolve reads no mask)
  mv.p = nullptr;
  mv.stride = mv.w = mv.h = 0;
  SdpArgs a;
  int rc = svo_sdp_args(s, &a, mv);
  if (rc >= 0) rc = sdp_launch(c, a, false);
  c->stream = keep;
  if (rc) return rc;
  p.from_frame_id = chain ? t.frame_id : -1;
  p.chain = true;
  float *f;
  uint8_t *u;
  f = t.buf.invd, t.buf.invd = p.buf.invd, p.buf.invd = f;
  f = t.buf.sigma, t.buf.sigma = p.buf.sigma, p.buf.sigma = f;
  u = t.buf.n_obs, t.buf.n_obs = p.buf.n_obs, p.buf.n_obs = u;
  u = t.buf.tstatus, t.buf.tstatus = p.buf.tstatus, p.buf.tstatus = u;
  return VO_OK;
}

void vo_svo_semidense_propagate_free(vo_svo *s) {
  vo_sdp_buffers_free(&s->sdp.buf);
  s->sdp = vo_svo_semidense_propagate();
}

extern "C" int vo_svo_set_semidense_propagate(vo_svo *s, const vo_semidense_propagate_params *prm) {
  if (!s) return VO_ERR_INVALID;
  vo_ctx *c = s->c;
  if (s->pending) VO_FAIL(c, VO_ERR_INVALID, "vo_svo_set_semidense_propagate: a frame is in flight: call vo_svo_result first");
  if (s->mono) VO_FAIL(c, VO_ERR_INVALID, "vo_svo_set_semidense_propagate: a stereo driver only");
  vo_svo_semidense_propagate &p = s->sdp;
  if (!prm) {
    p.on = false;
    p.chain = false;
    return VO_OK;
  }
  if (!s->sdt.on || !s->sd.on)
    VO_FAIL(c, VO_ERR_INVALID, "vo_svo_set_semidense_propagate: needs the temporal option: vo_svo_set_semidense_temporal first");
  int rc = sdp_check_params(c, prm);
  if (rc) return rc;
  rc = vo_sdp_buffers_alloc(c, &p.buf, true);  // the option's only allocation, at the first enable
  if (rc) return rc;
  p.prm = *prm;
  if (!p.on) p.chain = false;  // the next keyframe seeds plainly
  p.on = true;
  return VO_OK;
}

extern "C" int vo_svo_get_semidense_origin(vo_svo *s, uint8_t *origin, int *width, int *height, int *from_frame_id) {
  if (!s || !width || !height) return VO_ERR_INVALID;
  vo_ctx *c = s->c;
  if (s->pending) VO_FAIL(c, VO_ERR_INVALID, "vo_svo_get_semidense_origin: a frame is in flight: call vo_svo_result first");
  if (!s->sdp.on || !s->sdt.on || !s->sd.on) VO_FAIL(c, VO_ERR_INVALID, "vo_svo_get_semidense_origin: the option is off: vo_svo_set_semidense_propagate");
  VO_CHECK_HIP(c, hipSetDevice(c->device));
  if (s->sd.have) VO_CHECK_HIP(c, hipEventSynchronize(s->sd.done));  // the side stream's last launch only
  const vo_svo_semidense_temporal &t = s->sdt;
  const vo_svo_semidense_propagate &p = s->sdp;
  *width = *height = 0;
  if (from_frame_id) *from_frame_id = -1;
  if (!t.have || !p.chain) return VO_OK;  // no keyframe since the option was switched on
  *width = t.w;
  *height = t.h;
  if (from_frame_id) *from_frame_id = p.from_frame_id;
  if (origin) VO_CHECK_HIP(c, hipMemcpy(origin, p.buf.origin, (size_t)t.w * (size_t)t.h, hipMemcpyDeviceToHost));
  return VO_OK;
}
