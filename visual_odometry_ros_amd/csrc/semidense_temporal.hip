// semidense_temporal.hip — the temporal semi-dense search with its per-keyframe fusion (include/vo_hip.h, "Semi-dense temporal";
// DESIGN.md §18): the operator (vo_semidense_temporal), the map from a static result (vo_semidense_map_seed), the fused map's
// points (vo_semidense_map_points) and StereoVO's hook (vo_svo_set_semidense_temporal, vo_svo_get_semidense_map*).
// semidense_temporal_device.hpp has the kernels.
#include "stereo_vo.hpp"
#include "vo_internal.hpp"
#include "vo_kernels.hpp"

#include <math.h>

#include "semidense_temporal_device.hpp"

extern "C" int vo_semidense_temporal_default_params(vo_semidense_temporal_params *p) {
  if (!p) return VO_ERR_INVALID;
  memset(p, 0, sizeof(*p));
  p->hw = 4;
  p->hh = 1;
  p->g_min = 20;
  p->thres_best = 0.95f;
  p->thres_peak = 0.9f;
  p->peak_px = 5;
  p->edge_px = 2;
  p->eps_edge = 0.5f;
  p->eps_epi = 1.0f;
  p->eps_scale = 3.0f;
  p->z_min = 3.0f;
  p->z_max = 100.0f;
  p->max_search = 128;
  p->j_min = 16.0f;
  return VO_OK;
}

static int sdt_check_params(vo_ctx *c, const vo_semidense_temporal_params *p) {
  if (p->hw < 1 || p->hw > SDT_MAX_HW || p->hh < 0 || p->hh > SDT_MAX_HH)
    VO_FAIL(c, VO_ERR_INVALID, "semi-dense temporal: window half sizes hw=%d, hh=%d: expected hw in 1..%d, hh in 0..%d", p->hw, p->hh, SDT_MAX_HW,
            SDT_MAX_HH);
  if (p->g_min < 1 || p->g_min > 360) VO_FAIL(c, VO_ERR_INVALID, "semi-dense temporal: g_min=%d: expected 1..360", p->g_min);
  if (p->peak_px < 0 || p->peak_px > SDT_MAX_SEARCH || p->edge_px < 0 || p->edge_px > SDT_MAX_SEARCH)
    VO_FAIL(c, VO_ERR_INVALID, "semi-dense temporal: peak_px and edge_px: expected 0..%d", SDT_MAX_SEARCH);
  if (p->max_search < 2 * p->edge_px + 3 || p->max_search > SDT_MAX_SEARCH)
    VO_FAIL(c, VO_ERR_INVALID, "semi-dense temporal: max_search=%d: expected 2 edge_px + 3 .. %d", p->max_search, SDT_MAX_SEARCH);
  if (isnan(p->thres_best) || isnan(p->thres_peak)) VO_FAIL(c, VO_ERR_INVALID, "semi-dense temporal: a threshold is NaN");
  if (!(p->eps_edge >= 0.0f) || !(p->eps_epi >= 0.0f) || !(p->eps_scale >= 0.0f) || !isfinite(p->eps_edge) || !isfinite(p->eps_epi) ||
      !isfinite(p->eps_scale))
    VO_FAIL(c, VO_ERR_INVALID, "semi-dense temporal: eps_edge, eps_epi and eps_scale are finite and >= 0");
  if (!(p->z_min > 0.0f) || !(p->z_max > p->z_min) || !isfinite(p->z_max))
    VO_FAIL(c, VO_ERR_INVALID, "semi-dense temporal: expected 0 < z_min < z_max < inf");
  if (!(p->j_min > 0.0f) || !isfinite(p->j_min)) VO_FAIL(c, VO_ERR_INVALID, "semi-dense temporal: j_min must be positive");
  return VO_OK;
}

// ---- buffers ----------------------------------------------------------------------------------------------------------------------
// One allocation. The context's operator (host planes) has a score plane; a driver's option has none — it never asks for the
// diagnostic — and keeps the keyframe's ignore mask instead.
int vo_sdt_buffers_alloc(vo_ctx *c, vo_sdt_buffers *b, bool driver) {
  if (b->invd) return VO_OK;
  const size_t n = (size_t)c->cfg.max_width * (size_t)c->cfg.max_height;
  VO_CHECK_HIP(c, hipSetDevice(c->device));
  VO_CHECK_HIP(c, vo_dev_malloc(c, (void **)&b->invd, n * ((driver ? 2 : 3) * sizeof(float) + (driver ? 4 : 3)) + 64));
  b->base = b->invd;
  b->sigma = b->invd + n;
  float *end = b->sigma + n;
  if (!driver) b->score = end, end += n;
  b->n_obs = (uint8_t *)end;
  b->tstatus = b->n_obs + n;
  b->key = b->tstatus + n;
  if (driver) b->mask = b->key + n;
  b->npix = n;
  return VO_OK;
}
void vo_sdt_buffers_free(vo_sdt_buffers *b) {
  if (b->base) (void)hipFree(b->base);
  *b = vo_sdt_buffers();
}

struct vo_semidense_temporal_state {
  vo_sdt_buffers buf;
};
void vo_semidense_temporal_free(vo_ctx *c) {
  if (!c->semidense_t) return;
  vo_sdt_buffers_free(&c->semidense_t->buf);
  delete c->semidense_t;
  c->semidense_t = nullptr;
}
int vo_sdt_ctx_buffers(vo_ctx *c, vo_sdt_buffers **b) {
  if (!c->semidense_t) c->semidense_t = new vo_semidense_temporal_state();
  *b = &c->semidense_t->buf;
  return vo_sdt_buffers_alloc(c, *b, false);
}

// ---- the launch ---------------------------------------------------------------------------------------------------------------------
int vo_sdt_enqueue(vo_ctx *c, const uint8_t *d_key, int key_stride, const vo_mask_view *key_mask, int slot_cur, const float K[4],
                   const float T_ck[16], const vo_semidense_temporal_params *p, float *invd, float *sigma, uint8_t *n_obs, uint8_t *tstatus,
                   float *score) {
  int rc = sdt_check_params(c, p);
  if (rc) return rc;
  if (slot_cur < 0 || slot_cur >= c->cfg.n_slots || c->slots[slot_cur].n_levels <= 0) VO_FAIL(c, VO_ERR_INVALID, "slot holds no image");
  const vo_pyramid &P = c->slots[slot_cur];
  if (P.w < 3 || P.h < 3 || P.w > 65535 || P.h > 65535) VO_FAIL(c, VO_ERR_SIZE, "semi-dense temporal: the image must have 3 .. 65535 pixels a side");
  if (key_stride < P.w) VO_FAIL(c, VO_ERR_INVALID, "semi-dense temporal: key_stride %d below the width %d", key_stride, P.w);
  if (!(K[0] > 0.0f) || !(K[1] > 0.0f)) VO_FAIL(c, VO_ERR_INVALID, "semi-dense temporal: fx, fy must be positive");
  for (int i = 0; i < 12; ++i)
    if (!isfinite(T_ck[i])) VO_FAIL(c, VO_ERR_INVALID, "semi-dense temporal: T_ck is not finite");
  if (vo_slot_acquire(c, slot_cur) < 0) return VO_ERR_HIP;
  vo_mask_view mv;  // the key pixels' mask: the caller's (a driver's copy of the keyframe's), else the one bound to the current slot
  if (key_mask) {
    mv = *key_mask;
  } else {
    rc = vo_slot_mask_acquire(c, slot_cur, &mv);
    if (rc) return rc;
  }
  if (mv.p && (mv.w != P.w || mv.h != P.h))
    VO_FAIL(c, VO_ERR_SIZE, "semi-dense temporal: the mask is %d x %d, the image %d x %d", mv.w, mv.h, P.w, P.h);
  SdtArgs a;
  memset(&a, 0, sizeof(a));
  a.Lk = d_key;
  a.Lc = P.lv[0].origin();
  a.strideK = key_stride;
  a.strideC = P.lv[0].stride;
  a.W = P.w;
  a.H = P.h;
  a.mask = mv.p;
  a.mask_stride = mv.stride;
  a.hw = p->hw;
  a.hh = p->hh;
  a.g_min2 = p->g_min * p->g_min;
  a.peak_px = p->peak_px;
  a.edge_px = p->edge_px;
  a.max_search = p->max_search;
  a.thres_best = p->thres_best;
  a.thres_peak = p->thres_peak;
  a.eps_edge = p->eps_edge;
  a.eps_epi = p->eps_epi;
  a.eps_scale = p->eps_scale;
  a.r_min = 1.0f / p->z_max;
  a.r_max = 1.0f / p->z_min;
  a.j_min = p->j_min;
  a.fx = K[0], a.fy = K[1], a.cx = K[2], a.cy = K[3];
  sdt_pose(&a, T_ck);
  a.invd = invd;
  a.sigma = sigma;
  a.n_obs = n_obs;
  a.tstatus = tstatus;
  a.score = score;
  vo_prof_begin(c, VO_K_AUX);
  hipLaunchKernelGGL(semidense_temporal_kernel, dim3((unsigned)((a.W + SDT_SEG - 1) / SDT_SEG), (unsigned)a.H), dim3(SDT_NT), 0, c->stream, a);
  vo_prof_end(c);
  VO_CHECK_HIP(c, hipGetLastError());
  return VO_OK;
}

static void sdt_seed_launch(hipStream_t s, const float *disp, const float *sigma_invd, const uint8_t *status, float bf, float *invd, float *sigma,
                            uint8_t *n_obs, uint8_t *tstatus, size_t np) {
  hipLaunchKernelGGL(semidense_map_seed_kernel, dim3((unsigned)((np + 255) / 256)), dim3(256), 0, s, disp, sigma_invd, status, bf, invd, sigma, n_obs,
                     tstatus, (int)np);
}

extern "C" int vo_semidense_map_seed(vo_ctx *c, const float *disparity, const float *sigma_invd, const uint8_t *status, int width, int height,
                                     float bf, float *invd, float *sigma, uint8_t *n_obs, uint8_t *tstatus, int on_device) {
  if (!c || !disparity || !sigma_invd || !status || !invd || !sigma || !n_obs || !tstatus || width <= 0 || height <= 0) return VO_ERR_INVALID;
  if (width > c->cfg.max_width || height > c->cfg.max_height)
    VO_FAIL(c, VO_ERR_SIZE, "%d x %d planes exceed vo_config.max_width x max_height", width, height);
  if (!(bf > 0.0f) || !isfinite(bf)) VO_FAIL(c, VO_ERR_INVALID, "semi-dense: bf (focal length x baseline) must be positive");
  VO_CHECK_HIP(c, hipSetDevice(c->device));
  hipStream_t s = c->stream;
  const size_t np = (size_t)width * (size_t)height;
  if (on_device) {
    sdt_seed_launch(s, disparity, sigma_invd, status, bf, invd, sigma, n_obs, tstatus, np);
    VO_CHECK_HIP(c, hipGetLastError());
    VO_CHECK_HIP(c, hipStreamSynchronize(s));
    return VO_OK;
  }
  vo_sd_buffers *in;
  vo_sdt_buffers *b;
  int rc = vo_sd_ctx_buffers(c, &in);
  if (rc >= 0) rc = vo_sdt_ctx_buffers(c, &b);
  if (rc) return rc;
  VO_CHECK_HIP(c, hipMemcpyAsync(in->disp, disparity, np * sizeof(float), hipMemcpyHostToDevice, s));
  VO_CHECK_HIP(c, hipMemcpyAsync(in->sigma, sigma_invd, np * sizeof(float), hipMemcpyHostToDevice, s));
  VO_CHECK_HIP(c, hipMemcpyAsync(in->status, status, np, hipMemcpyHostToDevice, s));
  sdt_seed_launch(s, in->disp, in->sigma, in->status, bf, b->invd, b->sigma, b->n_obs, b->tstatus, np);
  VO_CHECK_HIP(c, hipGetLastError());
  VO_CHECK_HIP(c, hipMemcpyAsync(invd, b->invd, np * sizeof(float), hipMemcpyDeviceToHost, s));
  VO_CHECK_HIP(c, hipMemcpyAsync(sigma, b->sigma, np * sizeof(float), hipMemcpyDeviceToHost, s));
  VO_CHECK_HIP(c, hipMemcpyAsync(n_obs, b->n_obs, np, hipMemcpyDeviceToHost, s));
  VO_CHECK_HIP(c, hipMemcpyAsync(tstatus, b->tstatus, np, hipMemcpyDeviceToHost, s));
  VO_CHECK_HIP(c, hipStreamSynchronize(s));
  return VO_OK;
}

extern "C" int vo_semidense_temporal(vo_ctx *c, const uint8_t *key_plane, int key_stride, int key_on_device, int slot_cur, const float K[4],
                                     const float T_ck[16], const vo_semidense_temporal_params *prm, float *invd, float *sigma, uint8_t *n_obs,
                                     uint8_t *tstatus, float *score, int on_device) {
  if (!c || !key_plane || !K || !T_ck || !prm || !invd || !sigma || !n_obs || !tstatus) return VO_ERR_INVALID;
  VO_CHECK_HIP(c, hipSetDevice(c->device));
  hipStream_t s = c->stream;
  if (slot_cur < 0 || slot_cur >= c->cfg.n_slots || c->slots[slot_cur].n_levels <= 0) VO_FAIL(c, VO_ERR_INVALID, "slot holds no image");
  const int W = c->slots[slot_cur].w, H = c->slots[slot_cur].h;
  if (key_stride < W) VO_FAIL(c, VO_ERR_INVALID, "semi-dense temporal: key_stride %d below the width %d", key_stride, W);
  const size_t np = (size_t)W * (size_t)H;
  vo_sdt_buffers *b = nullptr;
  if (!key_on_device || !on_device) {
    const int rc = vo_sdt_ctx_buffers(c, &b);
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
    const int rc = vo_sdt_enqueue(c, d_key, d_stride, nullptr, slot_cur, K, T_ck, prm, invd, sigma, n_obs, tstatus, score);
    if (rc) return rc;
    VO_CHECK_HIP(c, hipStreamSynchronize(s));
    return VO_OK;
  }
  VO_CHECK_HIP(c, hipMemcpyAsync(b->invd, invd, np * sizeof(float), hipMemcpyHostToDevice, s));
  VO_CHECK_HIP(c, hipMemcpyAsync(b->sigma, sigma, np * sizeof(float), hipMemcpyHostToDevice, s));
  VO_CHECK_HIP(c, hipMemcpyAsync(b->n_obs, n_obs, np, hipMemcpyHostToDevice, s));
  const int rc = vo_sdt_enqueue(c, d_key, d_stride, nullptr, slot_cur, K, T_ck, prm, b->invd, b->sigma, b->n_obs, b->tstatus, score ? b->score : nullptr);
  if (rc) {
    (void)hipStreamSynchronize(s);  // (the copies read the caller's memory)
    return rc;
  }
  VO_CHECK_HIP(c, hipMemcpyAsync(invd, b->invd, np * sizeof(float), hipMemcpyDeviceToHost, s));
  VO_CHECK_HIP(c, hipMemcpyAsync(sigma, b->sigma, np * sizeof(float), hipMemcpyDeviceToHost, s));
  VO_CHECK_HIP(c, hipMemcpyAsync(n_obs, b->n_obs, np, hipMemcpyDeviceToHost, s));
  VO_CHECK_HIP(c, hipMemcpyAsync(tstatus, b->tstatus, np, hipMemcpyDeviceToHost, s));
  if (score) VO_CHECK_HIP(c, hipMemcpyAsync(score, b->score, np * sizeof(float), hipMemcpyDeviceToHost, s));
  VO_CHECK_HIP(c, hipStreamSynchronize(s));
  return VO_OK;
}

// the pixels with n_obs >= min_obs of DEVICE planes as a list (host outputs); b: the compaction's scratch. Synchronous on c->stream.
int vo_sdt_points(vo_ctx *c, vo_sd_buffers *b, const float *d_invd, const float *d_sigma, const uint8_t *d_n_obs, int W, int H, const float K[4],
                  const float *T, int min_obs, int cap, float *xyz, float *sigma_out, uint16_t *pixel, int *n) {
  const size_t np = (size_t)W * (size_t)H;
  hipLaunchKernelGGL(semidense_map_key_kernel, dim3((unsigned)((np + 255) / 256)), dim3(256), 0, c->stream, d_n_obs, b->key, min_obs, (int)np);
  VO_CHECK_HIP(c, hipGetLastError());
  return vo_sd_points_keyed(c, b, d_invd, d_sigma, W, H, K, 1.0f, T, cap, xyz, sigma_out, pixel, n);  // (z = 1.0f / invd)
}

extern "C" int vo_semidense_map_points(vo_ctx *c, const float *invd, const float *sigma, const uint8_t *n_obs, int width, int height,
                                       int planes_on_device, const float K[4], const float *T, int min_obs, int cap, float *xyz, float *sigma_out,
                                       uint16_t *pixel, int *n) {
  if (!c || !invd || !n_obs || !K || !n || width <= 0 || height <= 0 || cap < 0 || (cap > 0 && !xyz) || (sigma_out && !sigma)) return VO_ERR_INVALID;
  if (min_obs < 1 || min_obs > 255) VO_FAIL(c, VO_ERR_INVALID, "semi-dense map: min_obs=%d: expected 1..255", min_obs);
  if (width > c->cfg.max_width || height > c->cfg.max_height || width > 65535 || height > 65535)
    VO_FAIL(c, VO_ERR_SIZE, "%d x %d planes exceed vo_config.max_width x max_height", width, height);
  VO_CHECK_HIP(c, hipSetDevice(c->device));
  vo_sd_buffers *b;
  const int rc = vo_sd_ctx_buffers(c, &b);
  if (rc) return rc;
  const size_t np = (size_t)width * (size_t)height;
  const float *d_invd = invd, *d_sig = sigma;
  const uint8_t *d_no = n_obs;
  if (!planes_on_device) {
    hipStream_t s = c->stream;
    VO_CHECK_HIP(c, hipMemcpyAsync(b->disp, invd, np * sizeof(float), hipMemcpyHostToDevice, s));
    if (sigma) VO_CHECK_HIP(c, hipMemcpyAsync(b->sigma, sigma, np * sizeof(float), hipMemcpyHostToDevice, s));
    VO_CHECK_HIP(c, hipMemcpyAsync(b->status, n_obs, np, hipMemcpyHostToDevice, s));
    d_invd = b->disp;
    d_sig = sigma ? b->sigma : nullptr;
    d_no = b->status;
  }
  return vo_sdt_points(c, b, d_invd, d_sig, d_no, width, height, K, T, min_obs, cap, xyz, sigma_out, pixel, n);
}

// ---- StereoVO's hook ------------------------------------------------------------------------------------------------------------------
// Called by vo_svo_result behind vo_svo_semidense_enqueue. At a keyframe the static launch of this frame's pair is the last work on
// the side stream: the left level-0 plane is copied into the option's key plane and the map is seeded from the static planes behind
// it. At any later frame one launch reads that frame's left slot and the key plane, behind a fork event of the main stream. `sd.done`
// is recorded again behind either, so that the guard and the getters of both options wait for the side stream's last launch.
// With vo_svo_set_semidense_propagate on, a keyframe with a predecessor runs the propagation's scatter in front of the copies and
// its resolve in place of the seed (semidense_propagate.hip); a keyframe without one runs the resolve alone, which then writes the
// seed's values.
int vo_svo_semidense_temporal_enqueue(vo_svo *s, int slot_l, int is_keyframe, int frame_id, const float T_wc[16]) {
  vo_ctx *c = s->c;
  vo_svo_semidense &d = s->sd;
  vo_svo_semidense_temporal &t = s->sdt;
  if (s->sda.on) {  // (vo_svo_set_semidense_align: no result unless one is enqueued below)
    s->sda.prev_key = s->sda.have ? s->sda.key_frame_id : -1;
    s->sda.have = false, s->sda.frame_id = frame_id;
  }
  if (!is_keyframe && !t.have) return VO_OK;
  hipStream_t side = c->stream2;
  if (is_keyframe) {
    const vo_pyramid &P = c->slots[slot_l];
    const size_t np = (size_t)d.w * (size_t)d.h;
    // vo_svo_set_semidense_world: the outgoing keyframe's map goes into the world table before anything below overwrites it or its key plane
    if (s->sdw.on) {
      const int rc = vo_svo_semidense_world_enqueue(s);
      if (rc) return rc;
    }
    // vo_svo_set_semidense_propagate: the old map is warped into this keyframe before its key plane is overwritten
    const bool propagate = s->sdp.on, chain = propagate && t.have && s->sdp.chain && t.w == d.w && t.h == d.h;
    if (chain) {
      const int rc = vo_svo_semidense_propagate_scatter(s, slot_l, T_wc);
      if (rc) return rc;
    }
    VO_CHECK_HIP(c, hipMemcpy2DAsync(t.buf.key, (size_t)d.w, P.lv[0].origin(), (size_t)P.lv[0].stride, (size_t)d.w, (size_t)d.h,
                                     hipMemcpyDeviceToDevice, side));
    if (s->sda.on && s->sda.pyr) {  // vo_svo_set_semidense_align_pyr: the keyframe's coarser levels next to its plane
      const int rc = vo_svo_semidense_align_key_levels(s, slot_l, frame_id);
      if (rc) return rc;
    }
    // the keyframe's own ignore mask goes with its plane: vo_svo_set_mask may change what later pairs carry
    vo_mask_view mv;
    hipStream_t keep = c->stream;
    c->stream = side;
    const int rc = vo_slot_mask_acquire(c, slot_l, &mv);
    c->stream = keep;
    if (rc) return rc;
    t.mask_on = mv.p != nullptr && mv.w == d.w && mv.h == d.h;
    if (t.mask_on)
      VO_CHECK_HIP(c, hipMemcpy2DAsync(t.buf.mask, (size_t)d.w, mv.p, (size_t)mv.stride, (size_t)d.w, (size_t)d.h, hipMemcpyDeviceToDevice, side));
    t.w = d.w;
    t.h = d.h;
    if (propagate) {
      const int rc2 = vo_svo_semidense_propagate_resolve(s, chain);
      if (rc2) return rc2;
    } else {
      sdt_seed_launch(side, d.buf.disp, d.buf.sigma, d.buf.status, d.prm.bf, t.buf.invd, t.buf.sigma, t.buf.n_obs, t.buf.tstatus, np);
      VO_CHECK_HIP(c, hipGetLastError());
    }
    t.have = true;
    s->sdw.done = false;
    t.frame_id = frame_id;
    t.n_fused = 0;
    memcpy(t.T_wk, T_wc, sizeof(t.T_wk));
    t.kf_index = -1;
    for (const SvoKeyframe &k : s->keyframes)
      if (k.frame_id == frame_id) t.kf_index = k.global;
  } else {
    float T_cw[16], T_ck[16];
    svo_inv_se3(T_wc, T_cw);  // T_ck = inverseSE3(T_wc) * T_wk, both in float, in svo_mul44's order
    svo_mul44(T_cw, t.T_wk, T_ck);
    VO_CHECK_HIP(c, hipEventRecord(d.fork, c->stream_main));
    VO_CHECK_HIP(c, hipStreamWaitEvent(side, d.fork, 0));
    hipStream_t keep = c->stream;
    c->stream = side;
    vo_mask_view mv;  // (no mask: a view without a plane, so that the current slot's is not taken instead)
    mv.p = t.mask_on ? t.buf.mask : nullptr;
    mv.stride = mv.w = t.w;
    mv.h = t.h;
    // vo_svo_set_semidense_align: in front of the temporal launch, so that it reads the map fused through the previous frame
    int rc = s->sda.on ? vo_svo_semidense_align_enqueue(s, slot_l, frame_id, T_ck) : VO_OK;
    if (rc >= 0)
      rc = vo_sdt_enqueue(c, t.buf.key, t.w, &mv, slot_l, s->prm.frame.Kl, T_ck, &t.prm, t.buf.invd, t.buf.sigma, t.buf.n_obs, t.buf.tstatus,
                          nullptr);
    c->stream = keep;
    if (rc) return rc;
    ++t.n_fused;
    d.busy |= 1u << slot_l;
  }
  if (s->sdr.on) {  // vo_svo_set_semidense_regularize: behind the launch that wrote the map, on the planes that are current now
    const int rc = vo_svo_semidense_regularize_enqueue(s);
    if (rc) return rc;
  }
  if (is_keyframe && s->sdw.on && s->sdw.ra.on) {  // vo_svo_set_semidense_world_reanchor: the window's maps follow the local BA
    const int rc = vo_svo_semidense_world_reanchor_pass(s);
    if (rc) return rc;
  }
  VO_CHECK_HIP(c, hipEventRecord(d.done, side));
  return VO_OK;
}

void vo_svo_semidense_temporal_free(vo_svo *s) {
  vo_svo_semidense_world_free(s);
  vo_svo_semidense_propagate_free(s);
  vo_svo_semidense_regularize_free(s);
  vo_svo_semidense_align_free(s);
  vo_sdt_buffers_free(&s->sdt.buf);
  s->sdt = vo_svo_semidense_temporal();
}

extern "C" int vo_svo_set_semidense_temporal(vo_svo *s, const vo_semidense_temporal_params *prm) {
  if (!s) return VO_ERR_INVALID;
  vo_ctx *c = s->c;
  if (s->pending) VO_FAIL(c, VO_ERR_INVALID, "vo_svo_set_semidense_temporal: a frame is in flight: call vo_svo_result first");
  if (s->mono) VO_FAIL(c, VO_ERR_INVALID, "vo_svo_set_semidense_temporal: a stereo driver only");
  vo_svo_semidense_temporal &t = s->sdt;
  if (!prm) {
    t.on = false;
    t.have = false;
    s->sdr.have = false;  // (vo_svo_set_semidense_regularize: its planes belong to a map that is gone)
    return VO_OK;
  }
  if (!s->sd.on) VO_FAIL(c, VO_ERR_INVALID, "vo_svo_set_semidense_temporal: needs the static option: vo_svo_set_semidense first");
  int rc = sdt_check_params(c, prm);
  if (rc) return rc;
  rc = vo_sdt_buffers_alloc(c, &t.buf, true);  // the option's only allocation, at the first enable (the events are the static option's)
  if (rc) return rc;
  t.prm = *prm;
  t.on = true;
  return VO_OK;
}

static int svo_sdt_ready(vo_svo *s, const char *who) {
  vo_ctx *c = s->c;
  if (s->pending) VO_FAIL(c, VO_ERR_INVALID, "%s: a frame is in flight: call vo_svo_result first", who);
  if (!s->sdt.on || !s->sd.on) VO_FAIL(c, VO_ERR_INVALID, "%s: the option is off: vo_svo_set_semidense_temporal", who);
  VO_CHECK_HIP(c, hipSetDevice(c->device));
  if (s->sd.have) VO_CHECK_HIP(c, hipEventSynchronize(s->sd.done));  // the side stream's last launch only
  return VO_OK;
}

extern "C" int vo_svo_get_semidense_map(vo_svo *s, float *invd, float *sigma, uint8_t *n_obs, uint8_t *tstatus, int *width, int *height,
                                        int *frame_id, float T_wc[16], int *n_fused) {
  if (!s || !width || !height) return VO_ERR_INVALID;
  const int rc = svo_sdt_ready(s, "vo_svo_get_semidense_map");
  if (rc) return rc;
  vo_ctx *c = s->c;
  const vo_svo_semidense_temporal &t = s->sdt;
  *width = *height = 0;
  if (frame_id) *frame_id = -1;
  if (n_fused) *n_fused = 0;
  if (!t.have) return VO_OK;  // no keyframe yet
  *width = t.w;
  *height = t.h;
  if (frame_id) *frame_id = t.frame_id;
  if (n_fused) *n_fused = t.n_fused;
  if (T_wc) memcpy(T_wc, t.T_wk, sizeof(t.T_wk));
  const size_t n = (size_t)t.w * (size_t)t.h;
  if (invd) VO_CHECK_HIP(c, hipMemcpy(invd, t.buf.invd, n * sizeof(float), hipMemcpyDeviceToHost));
  if (sigma) VO_CHECK_HIP(c, hipMemcpy(sigma, t.buf.sigma, n * sizeof(float), hipMemcpyDeviceToHost));
  if (n_obs) VO_CHECK_HIP(c, hipMemcpy(n_obs, t.buf.n_obs, n, hipMemcpyDeviceToHost));
  if (tstatus) VO_CHECK_HIP(c, hipMemcpy(tstatus, t.buf.tstatus, n, hipMemcpyDeviceToHost));
  return VO_OK;
}

extern "C" int vo_svo_get_semidense_map_points(vo_svo *s, int world, int min_obs, int cap, float *xyz, float *sigma, uint16_t *pixel, int *n,
                                               int *frame_id) {
  if (!s || !n || cap < 0 || (cap > 0 && !xyz)) return VO_ERR_INVALID;
  const int rc = svo_sdt_ready(s, "vo_svo_get_semidense_map_points");
  if (rc) return rc;
  if (min_obs < 1 || min_obs > 255) VO_FAIL(s->c, VO_ERR_INVALID, "semi-dense map: min_obs=%d: expected 1..255", min_obs);
  vo_svo_semidense_temporal &t = s->sdt;
  *n = 0;
  if (frame_id) *frame_id = t.have ? t.frame_id : -1;
  if (!t.have) return VO_OK;
  return vo_sdt_points(s->c, &s->sd.buf, t.buf.invd, t.buf.sigma, t.buf.n_obs, t.w, t.h, s->prm.frame.Kl, world ? t.T_wk : nullptr, min_obs, cap, xyz,
                       sigma, pixel, n);
}
