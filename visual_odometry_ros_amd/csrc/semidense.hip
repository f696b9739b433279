// semidense.hip — semi-dense stereo depth by an epipolar ZNCC search (include/vo_hip.h, "Semi-dense stereo"): the
// operator (vo_semidense_stereo), the points list (vo_semidense_points) and StereoVO's per-keyframe / per-frame hook
// (vo_svo_set_semidense, vo_svo_get_semidense*). semidense_device.hpp has the kernels.
#include "stereo_vo.hpp"
#include "vo_internal.hpp"
#include "vo_kernels.hpp"

#include <math.h>

#include <vector>

#define SD_DYN_LDS(name)                                 \
  extern __shared__ __attribute__((aligned(16))) uint8_t sd_dyn_lds[]; \
  uint8_t *name = sd_dyn_lds
#define SD_BALLOT(p) __ballot((p))
// (every lane of the wavefront is active wherever these are reached)
__device__ __forceinline__ float sd_wave_max_f32(float v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v = fmaxf(v, __shfl_xor(v, m, 64));
  return v;
}
#define SD_WAVE_MAX_F32(v) sd_wave_max_f32((v))
// LDS instructions of one wavefront are carried out in the order they were issued: what is left is to keep the compiler from
// moving an access across this point
#define SD_WAVE_SYNC()                                     \
  do {                                                     \
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); \
    __builtin_amdgcn_wave_barrier();                       \
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront"); \
  } while (0)
#define SD_UDOT4(a, b, c) __builtin_amdgcn_udot4((a), (b), (c), false)
#include "semidense_device.hpp"

extern "C" int vo_semidense_default_params(vo_semidense_params *p) {
  if (!p) return VO_ERR_INVALID;
  memset(p, 0, sizeof(*p));
  p->hw = 8;
  p->hh = 1;
  p->d_min = 0;
  p->d_max = 64;
  p->g_min = 20;
  p->thres_best = 0.95f;
  p->thres_peak = 0.9f;
  p->peak_px = 5;
  p->edge_px = 2;
  p->eps_edge = 0.5f;
  p->eps_epi = 1.0f;
  p->bf = 1.0f;
  return VO_OK;
}

static int sd_check_params(vo_ctx *c, const vo_semidense_params *p) {
  if (p->hw < 1 || p->hw > SD_MAX_HW || p->hh < 0 || p->hh > SD_MAX_HH)
    VO_FAIL(c, VO_ERR_INVALID, "semi-dense: window half sizes hw=%d, hh=%d: expected hw in 1..%d, hh in 0..%d", p->hw, p->hh, SD_MAX_HW, SD_MAX_HH);
  if (p->d_min < 0 || p->d_min > p->d_max || p->d_max > SD_MAX_D)
    VO_FAIL(c, VO_ERR_INVALID, "semi-dense: disparities %d..%d: expected 0 <= d_min <= d_max <= %d", p->d_min, p->d_max, SD_MAX_D);
  if (p->g_min < 1 || p->g_min > 360) VO_FAIL(c, VO_ERR_INVALID, "semi-dense: g_min=%d: expected 1..360", p->g_min);
  if (p->peak_px < 0 || p->edge_px < 0 || p->edge_px > SD_MAX_D) VO_FAIL(c, VO_ERR_INVALID, "semi-dense: peak_px and edge_px are >= 0");
  if (isnan(p->thres_best) || isnan(p->thres_peak)) VO_FAIL(c, VO_ERR_INVALID, "semi-dense: a threshold is NaN");
  if (!(p->eps_edge >= 0.0f) || !(p->eps_epi >= 0.0f) || !isfinite(p->eps_edge) || !isfinite(p->eps_epi))
    VO_FAIL(c, VO_ERR_INVALID, "semi-dense: eps_edge and eps_epi are finite and >= 0");
  if (!(p->bf > 0.0f) || !isfinite(p->bf)) VO_FAIL(c, VO_ERR_INVALID, "semi-dense: bf (focal length x baseline) must be positive");
  return VO_OK;
}

// ---- buffers: the four planes, the points list's scratch, the compaction's count and the workgroups' accepted counts -----------
int vo_sd_buffers_alloc(vo_ctx *c, vo_sd_buffers *b) {
  if (b->disp) return VO_OK;
  const size_t n = (size_t)c->cfg.max_width * (size_t)c->cfg.max_height;
  VO_CHECK_HIP(c, hipSetDevice(c->device));
  VO_CHECK_HIP(c, vo_dev_malloc(c, (void **)&b->disp, n * (3 * sizeof(float) + 2 + sizeof(int32_t)) + 64));
  b->score = b->disp + n;
  b->sigma = b->score + n;
  b->idx = (int32_t *)(b->sigma + n);
  b->status = (uint8_t *)(b->idx + n);
  b->key = b->status + n;
  b->n_wg = (size_t)((c->cfg.max_width + SD_SEG - 1) / SD_SEG) * (size_t)c->cfg.max_height;
  VO_CHECK_HIP(c, vo_dev_malloc(c, (void **)&b->cnt, (2 + b->n_wg) * sizeof(int)));
  b->npix = n;
  return VO_OK;
}
void vo_sd_buffers_free(vo_sd_buffers *b) {
  if (b->disp) (void)hipFree(b->disp);
  if (b->cnt) (void)hipFree(b->cnt);
  if (b->pts) (void)hipFree(b->pts);
  *b = vo_sd_buffers();
}
// the points list's device outputs, made at the first vo_semidense_points / vo_svo_get_semidense_points of these buffers' owner
static int sd_points_alloc(vo_ctx *c, vo_sd_buffers *b) {
  if (b->pts) return VO_OK;
  VO_CHECK_HIP(c, vo_dev_malloc(c, (void **)&b->pts, b->npix * (4 * sizeof(float) + 2 * sizeof(uint16_t))));
  return VO_OK;
}
int vo_sd_points_alloc(vo_ctx *c, vo_sd_buffers *b) { return sd_points_alloc(c, b); }

struct vo_semidense_state {
  vo_sd_buffers buf;
};
void vo_semidense_free(vo_ctx *c) {
  vo_semidense_temporal_free(c);
  vo_semidense_propagate_free(c);
  vo_semidense_regularize_free(c);
  vo_semidense_align_free(c);
  if (!c->semidense) return;
  vo_sd_buffers_free(&c->semidense->buf);
  delete c->semidense;
  c->semidense = nullptr;
}
static int sd_ctx_buffers(vo_ctx *c, vo_sd_buffers **b) {
  if (!c->semidense) c->semidense = new vo_semidense_state();
  *b = &c->semidense->buf;
  return vo_sd_buffers_alloc(c, *b);
}
int vo_sd_ctx_buffers(vo_ctx *c, vo_sd_buffers **b) { return sd_ctx_buffers(c, b); }

// the launch on c->stream: the slots' level-0 planes and the left slot's mask, ordered behind their last writers
int vo_sd_enqueue(vo_ctx *c, int slot_l, int slot_r, const vo_semidense_params *p, float *disp, float *score, float *sigma, uint8_t *status,
                  int *wg_accepted, int *W_out, int *H_out) {
  int rc = sd_check_params(c, p);
  if (rc) return rc;
  if (slot_l < 0 || slot_l >= c->cfg.n_slots || slot_r < 0 || slot_r >= c->cfg.n_slots || c->slots[slot_l].n_levels <= 0 ||
      c->slots[slot_r].n_levels <= 0)
    VO_FAIL(c, VO_ERR_INVALID, "slot holds no image");
  const vo_pyramid &Pl = c->slots[slot_l], &Pr = c->slots[slot_r];
  if (Pl.w != Pr.w || Pl.h != Pr.h) VO_FAIL(c, VO_ERR_SIZE, "image size mismatch");
  if (Pl.w > 65535 || Pl.h > 65535) VO_FAIL(c, VO_ERR_SIZE, "semi-dense: the image exceeds 65535 pixels a side");
  if (vo_slot_acquire(c, slot_l) < 0 || vo_slot_acquire(c, slot_r) < 0) return VO_ERR_HIP;
  vo_mask_view mv;
  rc = vo_slot_mask_acquire(c, slot_l, &mv);
  if (rc) return rc;
  if (mv.p && (mv.w != Pl.w || mv.h != Pl.h)) VO_FAIL(c, VO_ERR_SIZE, "semi-dense: the left slot's mask is %d x %d, its image %d x %d", mv.w, mv.h, Pl.w, Pl.h);
  SdArgs a;
  memset(&a, 0, sizeof(a));
  a.L = Pl.lv[0].origin();
  a.R = Pr.lv[0].origin();
  a.strideL = Pl.lv[0].stride;
  a.strideR = Pr.lv[0].stride;
  a.W = Pl.w;
  a.H = Pl.h;
  a.mask = mv.p;
  a.mask_stride = mv.stride;
  a.hw = p->hw;
  a.hh = p->hh;
  a.d_min = p->d_min;
  a.d_max = p->d_max;
  a.g_min2 = p->g_min * p->g_min;
  a.peak_px = p->peak_px;
  a.edge_px = p->edge_px;
  a.thres_best = p->thres_best;
  a.thres_peak = p->thres_peak;
  a.eps_edge = p->eps_edge;
  a.eps_epi = p->eps_epi;
  a.bf = p->bf;
  a.disp = disp;
  a.score = score;
  a.sigma = sigma;
  a.status = status;
  a.wg_accepted = wg_accepted;
  sd_plan(&a);
  if (a.lds_bytes > 64 * 1024) VO_FAIL(c, VO_ERR_INVALID, "semi-dense: %d bytes of LDS", a.lds_bytes);  // (cannot happen within the limits above)
  vo_prof_begin(c, VO_K_AUX);
  hipLaunchKernelGGL(semidense_kernel, dim3((unsigned)((a.W + SD_SEG - 1) / SD_SEG), (unsigned)a.H), dim3(SD_NT), (size_t)a.lds_bytes, c->stream, a);
  vo_prof_end(c);
  VO_CHECK_HIP(c, hipGetLastError());
  if (W_out) *W_out = a.W;
  if (H_out) *H_out = a.H;
  return VO_OK;
}

extern "C" int vo_semidense_stereo(vo_ctx *c, int slot_l, int slot_r, const vo_semidense_params *prm, float *disparity, float *score,
                                   float *sigma_invd, uint8_t *status, int on_device) {
  if (!c || !prm) return VO_ERR_INVALID;
  VO_CHECK_HIP(c, hipSetDevice(c->device));
  hipStream_t s = c->stream;
  int W = 0, H = 0;
  if (on_device) {
    const int rc = vo_sd_enqueue(c, slot_l, slot_r, prm, disparity, score, sigma_invd, status, nullptr, &W, &H);
    if (rc) return rc;
    VO_CHECK_HIP(c, hipStreamSynchronize(s));
    return VO_OK;
  }
  vo_sd_buffers *b;
  int rc = sd_ctx_buffers(c, &b);
  if (rc) return rc;
  rc = vo_sd_enqueue(c, slot_l, slot_r, prm, disparity ? b->disp : nullptr, score ? b->score : nullptr, sigma_invd ? b->sigma : nullptr,
                     status ? b->status : nullptr, nullptr, &W, &H);
  if (rc) return rc;
  const size_t n = (size_t)W * (size_t)H;
  if (disparity) VO_CHECK_HIP(c, hipMemcpyAsync(disparity, b->disp, n * sizeof(float), hipMemcpyDeviceToHost, s));
  if (score) VO_CHECK_HIP(c, hipMemcpyAsync(score, b->score, n * sizeof(float), hipMemcpyDeviceToHost, s));
  if (sigma_invd) VO_CHECK_HIP(c, hipMemcpyAsync(sigma_invd, b->sigma, n * sizeof(float), hipMemcpyDeviceToHost, s));
  if (status) VO_CHECK_HIP(c, hipMemcpyAsync(status, b->status, n, hipMemcpyDeviceToHost, s));
  VO_CHECK_HIP(c, hipStreamSynchronize(s));
  return VO_OK;
}

// the accepted pixels of DEVICE planes as a list (host outputs); b: the scratch (key, idx, cnt[1], pts). Synchronous on c->stream.
int vo_sd_points(vo_ctx *c, vo_sd_buffers *b, const float *d_disp, const float *d_sigma, const uint8_t *d_status, int W, int H,
                 const float K[4], float bf, const float *T, int cap, float *xyz, float *sigma_out, uint16_t *pixel, int *n) {
  const size_t np = (size_t)W * (size_t)H;
  hipLaunchKernelGGL(semidense_key_kernel, dim3((unsigned)((np + 255) / 256)), dim3(256), 0, c->stream, d_status, b->key, (int)np);
  VO_CHECK_HIP(c, hipGetLastError());
  return vo_sd_points_keyed(c, b, d_disp, d_sigma, W, H, K, bf, T, cap, xyz, sigma_out, pixel, n);
}

// the same with b->key already written on c->stream (semidense_temporal.hip: the fused map's pixels, disp = invd and bf = 1)
int vo_sd_points_keyed(vo_ctx *c, vo_sd_buffers *b, const float *d_disp, const float *d_sigma, int W, int H, const float K[4], float bf,
                       const float *T, int cap, float *xyz, float *sigma_out, uint16_t *pixel, int *n) {
  const size_t np = (size_t)W * (size_t)H;
  int rc = sd_points_alloc(c, b);
  if (rc) return rc;
  hipStream_t s = c->stream;
  CompactArgsHost h;  // the stable compaction: the accepted pixels' indices in raster order
  h.mask = b->key;
  h.n = (int)np;
  h.index_valid = b->idx;
  h.d_n_out = b->cnt + 1;
  rc = vo_compact_enqueue(c, h);
  if (rc) return rc;
  int m = 0;
  VO_CHECK_HIP(c, hipMemcpyAsync(&m, b->cnt + 1, sizeof(int), hipMemcpyDeviceToHost, s));
  VO_CHECK_HIP(c, hipStreamSynchronize(s));
  *n = m;
  const int k = m < cap ? m : cap;
  if (k > 0 && xyz) {
    SdPointArgs a;
    memset(&a, 0, sizeof(a));
    a.idx = b->idx;
    a.n = b->cnt + 1;
    a.cap = k;
    a.W = W;
    a.disp = d_disp;
    a.sigma = d_sigma;
    a.fx = K[0];
    a.fy = K[1];
    a.cx = K[2];
    a.cy = K[3];
    a.bf = bf;
    a.has_T = T != nullptr;
    if (T) memcpy(a.T, T, sizeof(a.T));
    float *d_xyz = b->pts, *d_sig = d_xyz + 3 * b->npix;
    uint16_t *d_pix = (uint16_t *)(d_sig + b->npix);
    a.xyz = d_xyz;
    a.sig = d_sig;
    a.pixel = d_pix;
    hipLaunchKernelGGL(semidense_points_kernel, dim3((unsigned)((k + 255) / 256)), dim3(256), 0, s, a);
    VO_CHECK_HIP(c, hipGetLastError());
    VO_CHECK_HIP(c, hipMemcpyAsync(xyz, d_xyz, sizeof(float) * 3 * (size_t)k, hipMemcpyDeviceToHost, s));
    if (sigma_out) VO_CHECK_HIP(c, hipMemcpyAsync(sigma_out, d_sig, sizeof(float) * (size_t)k, hipMemcpyDeviceToHost, s));
    if (pixel) VO_CHECK_HIP(c, hipMemcpyAsync(pixel, d_pix, sizeof(uint16_t) * 2 * (size_t)k, hipMemcpyDeviceToHost, s));
    VO_CHECK_HIP(c, hipStreamSynchronize(s));
  }
  if (m > cap) VO_FAIL(c, VO_ERR_CAPACITY, "%d accepted pixels, room for %d", m, cap);
  return VO_OK;
}

extern "C" int vo_semidense_points(vo_ctx *c, const float *disparity, const float *sigma_invd, const uint8_t *status, int width, int height,
                                   int planes_on_device, const float K[4], float bf, const float *T, int cap, float *xyz, float *sigma_out,
                                   uint16_t *pixel, int *n) {
  if (!c || !disparity || !status || !K || !n || width <= 0 || height <= 0 || cap < 0 || (cap > 0 && !xyz) || (sigma_out && !sigma_invd))
    return VO_ERR_INVALID;
  if (width > c->cfg.max_width || height > c->cfg.max_height || width > 65535 || height > 65535)
    VO_FAIL(c, VO_ERR_SIZE, "%d x %d planes exceed vo_config.max_width x max_height", width, height);
  if (!(bf > 0.0f)) VO_FAIL(c, VO_ERR_INVALID, "semi-dense: bf (focal length x baseline) must be positive");
  VO_CHECK_HIP(c, hipSetDevice(c->device));
  vo_sd_buffers *b;
  int rc = sd_ctx_buffers(c, &b);
  if (rc) return rc;
  const size_t np = (size_t)width * (size_t)height;
  const float *d_disp = disparity, *d_sig = sigma_invd;
  const uint8_t *d_st = status;
  if (!planes_on_device) {
    hipStream_t s = c->stream;
    VO_CHECK_HIP(c, hipMemcpyAsync(b->disp, disparity, np * sizeof(float), hipMemcpyHostToDevice, s));
    if (sigma_invd) VO_CHECK_HIP(c, hipMemcpyAsync(b->sigma, sigma_invd, np * sizeof(float), hipMemcpyHostToDevice, s));
    VO_CHECK_HIP(c, hipMemcpyAsync(b->status, status, np, hipMemcpyHostToDevice, s));
    d_disp = b->disp;
    d_sig = sigma_invd ? b->sigma : nullptr;
    d_st = b->status;
  }
  return vo_sd_points(c, b, d_disp, d_sig, d_st, width, height, K, bf, T, cap, xyz, sigma_out, pixel, n);
}

// ---- StereoVO's hook -----------------------------------------------------------------------------------------------------------
// The launch for the frame whose result the host has just taken (vo_svo_result): on the side stream, behind a fork event of the
// main stream, reading the current left / right slots. The keyframe rule is the host's (svo_keyframe_rule: acosf of the host's
// libm decides it), so the launch is enqueued where that decision is known, for the frames that produce a result only.
int vo_svo_semidense_enqueue(vo_svo *s, int slot_l, int slot_r, int frame_id, const float T_wc[16]) {
  vo_ctx *c = s->c;
  vo_svo_semidense &d = s->sd;
  VO_CHECK_HIP(c, hipEventRecord(d.fork, c->stream_main));
  VO_CHECK_HIP(c, hipStreamWaitEvent(c->stream2, d.fork, 0));
  hipStream_t keep = c->stream;
  c->stream = c->stream2;
  const int rc = vo_sd_enqueue(c, slot_l, slot_r, &d.prm, d.buf.disp, d.buf.score, d.buf.sigma, d.buf.status, d.buf.cnt + 2, &d.w, &d.h);
  c->stream = keep;
  if (rc) return rc;
  VO_CHECK_HIP(c, hipEventRecord(d.done, c->stream2));
  d.have = true;
  d.busy |= (1u << slot_l) | (1u << slot_r);  // (launches follow each other on the side stream: `done` covers every earlier one)
  d.slot_l = slot_l;
  d.slot_r = slot_r;
  d.frame_id = frame_id;
  memcpy(d.T_wc, T_wc, sizeof(d.T_wc));
  return VO_OK;
}

// An ingestion is about to overwrite slots a and b: where a launch since the last such wait read one of them, both streams an ingestion can
// run on are ordered behind the launch's event — on the device; the host does not wait.
int vo_svo_semidense_guard(vo_svo *s, int a, int b) {
  vo_svo_semidense &d = s->sd;
  if (!(d.busy & ((1u << a) | (1u << b)))) return VO_OK;
  vo_ctx *c = s->c;
  VO_CHECK_HIP(c, hipStreamWaitEvent(c->stream_main, d.done, 0));
  VO_CHECK_HIP(c, hipStreamWaitEvent(c->stream2, d.done, 0));
  d.busy = 0;
  return VO_OK;
}

void vo_svo_semidense_free(vo_svo *s) {
  vo_svo_semidense &d = s->sd;
  if (d.have) (void)hipEventSynchronize(d.done);
  vo_svo_semidense_temporal_free(s);
  vo_sd_buffers_free(&d.buf);
  if (d.fork) (void)hipEventDestroy(d.fork);
  if (d.done) (void)hipEventDestroy(d.done);
  d = vo_svo_semidense();
}

extern "C" int vo_svo_set_semidense(vo_svo *s, const vo_semidense_params *prm, int every) {
  if (!s) return VO_ERR_INVALID;
  vo_ctx *c = s->c;
  if (s->pending) VO_FAIL(c, VO_ERR_INVALID, "vo_svo_set_semidense: a frame is in flight: call vo_svo_result first");
  if (s->mono) VO_FAIL(c, VO_ERR_INVALID, "vo_svo_set_semidense: a stereo driver only");
  vo_svo_semidense &d = s->sd;
  if (!prm) {
    d.on = false;
    s->sdt.have = false;  // (the temporal option's map belongs to a keyframe of this option's results)
    return VO_OK;
  }
  if (every != VO_SEMIDENSE_KEYFRAMES && every != VO_SEMIDENSE_FRAMES)
    VO_FAIL(c, VO_ERR_INVALID, "vo_svo_set_semidense: every=%d: expected VO_SEMIDENSE_KEYFRAMES (0) or VO_SEMIDENSE_FRAMES (1)", every);
  int rc = sd_check_params(c, prm);
  if (rc) return rc;
  VO_CHECK_HIP(c, hipSetDevice(c->device));
  if (!d.buf.disp) {  // the option's only allocations
    rc = vo_sd_buffers_alloc(c, &d.buf);
    if (rc >= 0) rc = sd_points_alloc(c, &d.buf);
    if (rc) return rc;
    VO_CHECK_HIP(c, hipEventCreateWithFlags(&d.fork, hipEventDisableTiming));
    VO_CHECK_HIP(c, hipEventCreateWithFlags(&d.done, hipEventDisableTiming));
  }
  d.prm = *prm;
  d.every = every;
  d.on = true;
  return VO_OK;
}

static int svo_sd_ready(vo_svo *s, const char *who) {
  vo_ctx *c = s->c;
  if (s->pending) VO_FAIL(c, VO_ERR_INVALID, "%s: a frame is in flight: call vo_svo_result first", who);
  if (!s->sd.on) VO_FAIL(c, VO_ERR_INVALID, "%s: the option is off: vo_svo_set_semidense", who);
  VO_CHECK_HIP(c, hipSetDevice(c->device));
  if (s->sd.have) VO_CHECK_HIP(c, hipEventSynchronize(s->sd.done));  // that launch only
  return VO_OK;
}

extern "C" int vo_svo_get_semidense(vo_svo *s, float *disparity, float *score, float *sigma_invd, uint8_t *status, int *width, int *height,
                                    int *frame_id, float T_wc[16], int *n_accepted) {
  if (!s || !width || !height) return VO_ERR_INVALID;
  const int rc = svo_sd_ready(s, "vo_svo_get_semidense");
  if (rc) return rc;
  vo_ctx *c = s->c;
  const vo_svo_semidense &d = s->sd;
  *width = *height = 0;
  if (frame_id) *frame_id = -1;
  if (n_accepted) *n_accepted = 0;
  if (!d.have) return VO_OK;  // no frame has produced a result yet
  *width = d.w;
  *height = d.h;
  if (frame_id) *frame_id = d.frame_id;
  if (T_wc) memcpy(T_wc, d.T_wc, sizeof(d.T_wc));
  const size_t n = (size_t)d.w * (size_t)d.h;
  if (disparity) VO_CHECK_HIP(c, hipMemcpy(disparity, d.buf.disp, n * sizeof(float), hipMemcpyDeviceToHost));
  if (score) VO_CHECK_HIP(c, hipMemcpy(score, d.buf.score, n * sizeof(float), hipMemcpyDeviceToHost));
  if (sigma_invd) VO_CHECK_HIP(c, hipMemcpy(sigma_invd, d.buf.sigma, n * sizeof(float), hipMemcpyDeviceToHost));
  if (status) VO_CHECK_HIP(c, hipMemcpy(status, d.buf.status, n, hipMemcpyDeviceToHost));
  if (n_accepted) {  // the workgroups' counts, added here
    const size_t n_wg = (size_t)((d.w + SD_SEG - 1) / SD_SEG) * (size_t)d.h;
    std::vector<int> wg(n_wg);
    VO_CHECK_HIP(c, hipMemcpy(wg.data(), d.buf.cnt + 2, n_wg * sizeof(int), hipMemcpyDeviceToHost));
    long long sum = 0;
    for (int v : wg) sum += v;
    *n_accepted = (int)sum;
  }
  return VO_OK;
}

extern "C" int vo_svo_get_semidense_points(vo_svo *s, int world, int cap, float *xyz, float *sigma_invd, uint16_t *pixel, int *n, int *frame_id) {
  if (!s || !n || cap < 0 || (cap > 0 && !xyz)) return VO_ERR_INVALID;
  const int rc = svo_sd_ready(s, "vo_svo_get_semidense_points");
  if (rc) return rc;
  vo_svo_semidense &d = s->sd;
  *n = 0;
  if (frame_id) *frame_id = d.have ? d.frame_id : -1;
  if (!d.have) return VO_OK;
  return vo_sd_points(s->c, &d.buf, d.buf.disp, d.buf.sigma, d.buf.status, d.w, d.h, s->prm.frame.Kl, d.prm.bf, world ? d.T_wc : nullptr, cap, xyz,
                      sigma_invd, pixel, n);
}
