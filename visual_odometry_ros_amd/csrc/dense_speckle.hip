// dense_speckle.hip — the speckle filter for disparity planes (include/vo_hip.h, "Speckle filter"): connected-component
// labelling on the device and the removal of the small components. The operator (vo_disparity_speckle_filter, vo_speckle_workspace)
// and StereoVO's option behind its dense result (vo_svo_set_dense_speckle, vo_svo_get_dense_speckle_stats).
// dense_speckle_device.hpp has the kernels.
#include "stereo_vo.hpp"
#include "vo_internal.hpp"
#include "vo_kernels.hpp"

#include <math.h>

#define SPK_LD_LDS(p) __hip_atomic_load((p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP)
#define SPK_LD_AGENT(p) __hip_atomic_load((p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)
#include "dense_speckle_device.hpp"

#define SPK_HEAD 16  // the counters' block at the allocation's start, padded to 16 bytes

extern "C" int vo_speckle_default_params(vo_speckle_params *p) {
  if (!p) return VO_ERR_INVALID;
  memset(p, 0, sizeof(*p));
  p->max_size = 100;
  p->max_diff = 1.0f;
  return VO_OK;
}

static const char *spk_params_fault(const vo_speckle_params *p) {
  if (p->max_size < 0) return "max_size: expected >= 0";
  if (!(p->max_diff >= 0.0f) || !isfinite(p->max_diff)) return "max_diff is finite and >= 0";
  return nullptr;
}
int vo_spk_check_params(vo_ctx *c, const vo_speckle_params *p) {
  const char *f = spk_params_fault(p);
  if (f) VO_FAIL(c, VO_ERR_INVALID, "speckle filter: %s", f);
  return VO_OK;
}

static bool spk_shape_ok(int W, int H) { return W >= 1 && H >= 1 && W <= 65535 && H <= 65535 && (long long)W * (long long)H <= 0x7fffffffLL; }
static size_t spk_workspace_bytes(int W, int H) { return SPK_HEAD + 2 * sizeof(int32_t) * (size_t)W * (size_t)H; }

extern "C" int vo_speckle_workspace(int width, int height, size_t *bytes) {
  if (!bytes || !spk_shape_ok(width, height)) return VO_ERR_INVALID;
  *bytes = spk_workspace_bytes(width, height);
  return VO_OK;
}

// `*p` holds `bytes` at least; no launch may be reading the old one (the callers enqueue on one stream and free behind a wait)
static int spk_grow(vo_ctx *c, void **p, size_t *have, size_t bytes, const char *what) {
  if (*p && *have >= bytes) return VO_OK;
  if (*p) {
    VO_CHECK_HIP(c, hipStreamSynchronize(c->stream));
    (void)hipFree(*p);
    *p = nullptr;
    *have = 0;
  }
  if (vo_dev_malloc(c, p, bytes) != hipSuccess) {
    (void)hipGetLastError();
    *p = nullptr;
    VO_FAIL(c, VO_ERR_HIP, "speckle filter: %s of %zu bytes could not be allocated", what, bytes);
  }
  *have = bytes;
  return VO_OK;
}
int vo_spk_reserve(vo_ctx *c, vo_spk_buffers *b, int W, int H) {
  if (!spk_shape_ok(W, H)) VO_FAIL(c, VO_ERR_SIZE, "speckle filter: %d x %d: expected 1..65535 a side and at most 2^31 - 1 pixels", W, H);
  return spk_grow(c, &b->ws, &b->ws_bytes, spk_workspace_bytes(W, H), "the workspace");
}
void vo_spk_buffers_free(vo_spk_buffers *b) {
  if (b->ws) (void)hipFree(b->ws);
  *b = vo_spk_buffers();
}
int *vo_spk_counters(const vo_spk_buffers *b) { return (int *)b->ws; }
int32_t *vo_spk_label(const vo_spk_buffers *b) { return (int32_t *)((char *)b->ws + SPK_HEAD); }
int32_t *vo_spk_size(const vo_spk_buffers *b, int W, int H) { return vo_spk_label(b) + (size_t)W * (size_t)H; }

struct vo_speckle_state {
  vo_spk_buffers ws;
  void *stage = nullptr;  // host planes' device copies: disparity, sigma_invd (floats), status
  size_t stage_bytes = 0;
};
void vo_speckle_free(vo_ctx *c) {
  if (!c->speckle) return;
  vo_spk_buffers_free(&c->speckle->ws);
  if (c->speckle->stage) (void)hipFree(c->speckle->stage);
  delete c->speckle;
  c->speckle = nullptr;
}

int vo_spk_enqueue(vo_ctx *c, vo_spk_buffers *b, float *disp, float *sigma, uint8_t *status, int W, int H, const vo_speckle_params *p) {
  int rc = vo_spk_check_params(c, p);
  if (rc) return rc;
  if (!disp || !status) VO_FAIL(c, VO_ERR_INVALID, "speckle filter: disparity and status are required");
  if (!spk_shape_ok(W, H) || !b->ws || b->ws_bytes < spk_workspace_bytes(W, H)) VO_FAIL(c, VO_ERR_SIZE, "speckle filter: no workspace for %d x %d", W, H);
  SpkArgs a;
  memset(&a, 0, sizeof(a));
  a.disp = disp;
  a.sigma = sigma;
  a.status = status;
  a.label = vo_spk_label(b);
  a.size = vo_spk_size(b, W, H);
  a.counters = vo_spk_counters(b);
  a.W = W;
  a.H = H;
  a.n = W * H;
  a.ntx = (W + SPK_TW - 1) / SPK_TW;
  a.nty = (H + SPK_TH - 1) / SPK_TH;
  a.max_size = p->max_size;
  a.max_diff = p->max_diff;
  const int n_edge = (a.ntx - 1) * H + (a.nty - 1) * W;
  vo_prof_begin(c, VO_K_AUX);
  hipLaunchKernelGGL(speckle_local_kernel, dim3((unsigned)a.ntx, (unsigned)a.nty), dim3(SPK_NT), 0, c->stream, a);
  if (n_edge > 0) hipLaunchKernelGGL(speckle_merge_kernel, dim3((unsigned)((n_edge + SPK_NT - 1) / SPK_NT)), dim3(SPK_NT), 0, c->stream, a);
  hipLaunchKernelGGL(speckle_flatten_kernel, dim3((unsigned)a.ntx, (unsigned)a.nty), dim3(SPK_NT), 0, c->stream, a);
  hipLaunchKernelGGL(speckle_apply_kernel, dim3((unsigned)((a.n + SPK_NT - 1) / SPK_NT)), dim3(SPK_NT), 0, c->stream, a);
  vo_prof_end(c);
  VO_CHECK_HIP(c, hipGetLastError());
  return VO_OK;
}

extern "C" int vo_disparity_speckle_filter(vo_ctx *c, float *disparity, float *sigma_invd, uint8_t *status, int width, int height,
                                           const vo_speckle_params *prm, int32_t *label, int32_t *size, int *n_removed, int *n_components,
                                           int on_device) {
  if (!c || !prm) return VO_ERR_INVALID;
  int rc = vo_spk_check_params(c, prm);
  if (rc) return rc;
  if (!disparity || !status) VO_FAIL(c, VO_ERR_INVALID, "speckle filter: disparity and status are required");
  VO_CHECK_HIP(c, hipSetDevice(c->device));
  hipStream_t s = c->stream;
  if (!c->speckle) c->speckle = new vo_speckle_state();
  vo_speckle_state *st = c->speckle;
  rc = vo_spk_reserve(c, &st->ws, width, height);
  if (rc) return rc;
  const size_t n = (size_t)width * (size_t)height;
  float *d_disp = disparity, *d_sigma = sigma_invd;
  uint8_t *d_status = status;
  if (!on_device) {
    rc = spk_grow(c, &st->stage, &st->stage_bytes, n * (2 * sizeof(float) + 1), "the planes' device copy");
    if (rc) return rc;
    d_disp = (float *)st->stage;
    d_sigma = sigma_invd ? d_disp + n : nullptr;
    d_status = (uint8_t *)(d_disp + 2 * n);
    VO_CHECK_HIP(c, hipMemcpyAsync(d_disp, disparity, n * sizeof(float), hipMemcpyHostToDevice, s));
    if (sigma_invd) VO_CHECK_HIP(c, hipMemcpyAsync(d_sigma, sigma_invd, n * sizeof(float), hipMemcpyHostToDevice, s));
    VO_CHECK_HIP(c, hipMemcpyAsync(d_status, status, n, hipMemcpyHostToDevice, s));
  }
  rc = vo_spk_enqueue(c, &st->ws, d_disp, d_sigma, d_status, width, height, prm);
  if (rc) return rc;
  const hipMemcpyKind out = on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
  if (!on_device) {
    VO_CHECK_HIP(c, hipMemcpyAsync(disparity, d_disp, n * sizeof(float), hipMemcpyDeviceToHost, s));
    if (sigma_invd) VO_CHECK_HIP(c, hipMemcpyAsync(sigma_invd, d_sigma, n * sizeof(float), hipMemcpyDeviceToHost, s));
    VO_CHECK_HIP(c, hipMemcpyAsync(status, d_status, n, hipMemcpyDeviceToHost, s));
  }
  if (label) VO_CHECK_HIP(c, hipMemcpyAsync(label, vo_spk_label(&st->ws), n * sizeof(int32_t), out, s));
  if (size) VO_CHECK_HIP(c, hipMemcpyAsync(size, vo_spk_size(&st->ws, width, height), n * sizeof(int32_t), out, s));
  int cnt[2] = {0, 0};  // (the counters are host integers also with device planes)
  if (n_removed || n_components) VO_CHECK_HIP(c, hipMemcpyAsync(cnt, vo_spk_counters(&st->ws), sizeof(cnt), hipMemcpyDeviceToHost, s));
  VO_CHECK_HIP(c, hipStreamSynchronize(s));
  if (n_removed) *n_removed = cnt[0];
  if (n_components) *n_components = cnt[1];
  return VO_OK;
}

// ---- StereoVO's option: the filter behind the dense decision (dense_stereo.hip enqueues it), in place on the driver's dense planes --
extern "C" int vo_svo_set_dense_speckle(vo_svo *s, const vo_speckle_params *prm) {
  if (!s) return VO_ERR_INVALID;
  vo_ctx *c = s->c;
  if (s->pending) VO_FAIL(c, VO_ERR_INVALID, "vo_svo_set_dense_speckle: a frame is in flight: call vo_svo_result first");
  if (s->mono) VO_FAIL(c, VO_ERR_INVALID, "vo_svo_set_dense_speckle: a stereo driver only");
  vo_svo_dense_stereo &d = s->ds;
  if (!prm) {
    d.spk_on = false;
    return VO_OK;
  }
  if (!d.on) VO_FAIL(c, VO_ERR_INVALID, "vo_svo_set_dense_speckle: needs vo_svo_set_dense_stereo");
  int rc = vo_spk_check_params(c, prm);
  if (rc) return rc;
  VO_CHECK_HIP(c, hipSetDevice(c->device));
  if (!d.spk.ws) {  // the label and size planes for the largest pair the context takes: once
    rc = vo_spk_reserve(c, &d.spk, c->cfg.max_width, c->cfg.max_height);
    if (rc) return rc;
  }
  d.spk_prm = *prm;
  d.spk_on = true;
  return VO_OK;
}

extern "C" int vo_svo_get_dense_speckle_stats(vo_svo *s, int *n_removed, int *n_components) {
  if (!s) return VO_ERR_INVALID;
  vo_ctx *c = s->c;
  if (s->pending) VO_FAIL(c, VO_ERR_INVALID, "vo_svo_get_dense_speckle_stats: a frame is in flight: call vo_svo_result first");
  if (s->mono) VO_FAIL(c, VO_ERR_INVALID, "vo_svo_get_dense_speckle_stats: a stereo driver only");
  vo_svo_dense_stereo &d = s->ds;
  if (!d.on || !d.spk_on) VO_FAIL(c, VO_ERR_INVALID, "vo_svo_get_dense_speckle_stats: the option is off: vo_svo_set_dense_speckle");
  VO_CHECK_HIP(c, hipSetDevice(c->device));
  int cnt[2] = {0, 0};
  if (d.have && d.spk_have) {  // (before any filtered result: 0, 0)
    VO_CHECK_HIP(c, hipEventSynchronize(d.done));  // those launches only
    VO_CHECK_HIP(c, hipMemcpy(cnt, vo_spk_counters(&d.spk), sizeof(cnt), hipMemcpyDeviceToHost));
  }
  if (n_removed) *n_removed = cnt[0];
  if (n_components) *n_components = cnt[1];
  return VO_OK;
}
