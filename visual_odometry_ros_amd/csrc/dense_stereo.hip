// dense_stereo.hip — dense stereo disparity by census + semi-global matching (include/vo_hip.h, "Dense stereo"): the
// operator (vo_dense_stereo, vo_dense_stereo_workspace) and StereoVO's per-keyframe / per-frame hook (vo_svo_set_dense_stereo,
// vo_svo_get_dense_stereo, vo_svo_get_dense_points). dense_stereo_device.hpp has the kernels.
#include "stereo_vo.hpp"
#include "vo_internal.hpp"
#include "vo_kernels.hpp"

#include <math.h>

#include <vector>

// (every lane of the wavefront is active wherever these are reached)
__device__ __forceinline__ unsigned ds_wave_min_u32(unsigned v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) {
    const unsigned o = __shfl_xor(v, m, 64);
    v = o < v ? o : v;
  }
  return v;
}
#define DS_WAVE_MIN_U32(v) ds_wave_min_u32((v))
#define DS_WAVE_STEP(m, lo, hi, mn, up, dn)     \
  do {                                          \
    (mn) = (int)ds_wave_min_u32((unsigned)(m)); \
    (up) = __shfl_up((lo), 1, 64);              \
    (dn) = __shfl_down((hi), 1, 64);            \
  } while (0)
#define DS_POPC64(v) __popcll((v))
#include "dense_stereo_device.hpp"

extern "C" int vo_dense_stereo_default_params(vo_dense_stereo_params *p) {
  if (!p) return VO_ERR_INVALID;
  memset(p, 0, sizeof(*p));
  p->d_min = 0;
  p->n_disp = 64;
  p->paths = 8;
  p->p1 = 8;
  p->p2 = 64;
  p->uniqueness = 10;
  p->lr_max = 1;
  p->eps_d = 0.5f;
  p->bf = 1.0f;
  return VO_OK;
}

// null where the parameters are in range, else what is wrong with them
static const char *ds_params_fault(const vo_dense_stereo_params *p) {
  if (p->d_min < 0 || p->d_min > 65535) return "d_min: expected 0..65535";
  if (p->n_disp != 64 && p->n_disp != 128 && p->n_disp != 192 && p->n_disp != 256) return "n_disp: expected 64, 128, 192 or 256";
  if (p->paths != 4 && p->paths != 8) return "paths: expected 4 or 8";
  if (p->p1 < 0 || p->p1 >= p->p2 || p->p2 > 8129) return "expected 0 <= p1 < p2 <= 8129";
  if (p->uniqueness < 0 || p->uniqueness > 99) return "uniqueness: expected 0..99";
  if (p->lr_max < -1) return "lr_max: expected >= -1 (-1: no left-right check)";
  if (!(p->eps_d >= 0.0f) || !isfinite(p->eps_d)) return "eps_d is finite and >= 0";
  if (!(p->bf > 0.0f) || !isfinite(p->bf)) return "bf (focal length x baseline) is finite and > 0";
  return nullptr;
}
static int ds_check_params(vo_ctx *c, const vo_dense_stereo_params *p) {
  const char *f = ds_params_fault(p);
  if (f) VO_FAIL(c, VO_ERR_INVALID, "dense stereo: %s", f);
  return VO_OK;
}

static size_t ds_workspace_bytes(int W, int H, int n_disp) { return (size_t)W * (size_t)H * (2 * sizeof(unsigned long long) + sizeof(uint16_t) * (size_t)n_disp); }

extern "C" int vo_dense_stereo_workspace(int width, int height, const vo_dense_stereo_params *prm, size_t *bytes) {
  if (!prm || !bytes || width <= 0 || height <= 0 || width > 65535 || height > 65535 || ds_params_fault(prm)) return VO_ERR_INVALID;
  *bytes = ds_workspace_bytes(width, height, prm->n_disp);
  return VO_OK;
}

// the workspace holds `bytes` at least; no launch may be reading the old one (the callers enqueue on one stream and free behind a wait)
static int ds_workspace_reserve(vo_ctx *c, vo_ds_buffers *b, size_t bytes) {
  if (b->ws && b->ws_bytes >= bytes) return VO_OK;
  if (b->ws) {
    VO_CHECK_HIP(c, hipStreamSynchronize(c->stream));
    (void)hipFree(b->ws);
    b->ws = nullptr;
    b->ws_bytes = 0;
  }
  if (vo_dev_malloc(c, &b->ws, bytes) != hipSuccess) {
    (void)hipGetLastError();
    b->ws = nullptr;
    VO_FAIL(c, VO_ERR_HIP, "dense stereo: the workspace of %zu bytes could not be allocated", bytes);
  }
  b->ws_bytes = bytes;
  return VO_OK;
}
void vo_ds_buffers_free(vo_ds_buffers *b) {
  if (b->ws) (void)hipFree(b->ws);
  *b = vo_ds_buffers();
}

struct vo_dense_stereo_state {
  vo_ds_buffers ws;
};
void vo_dense_stereo_free(vo_ctx *c) {
  if (!c->dense_stereo) return;
  vo_ds_buffers_free(&c->dense_stereo->ws);
  delete c->dense_stereo;
  c->dense_stereo = nullptr;
}

template <int ND>
static void ds_launch(vo_ctx *c, const DsAggArgs &agg, int paths, const DsDecideArgs &dec) {
  static const int dirs[8][2] = {{1, 0}, {-1, 0}, {0, 1}, {0, -1}, {1, 1}, {-1, -1}, {1, -1}, {-1, 1}};
  for (int r = 0; r < paths; ++r) {
    DsAggArgs a = agg;
    a.dx = dirs[r][0];
    a.dy = dirs[r][1];
    a.n_paths = ds_path_count(a.W, a.H, a.dx, a.dy);
    a.first = r == 0;
    hipLaunchKernelGGL(dense_aggregate_kernel<ND>, dim3((unsigned)((a.n_paths + DS_AGG_NT / 64 - 1) / (DS_AGG_NT / 64))), dim3(DS_AGG_NT), 0, c->stream, a);
  }
  const size_t np = (size_t)dec.W * (size_t)dec.H, per_wg = (size_t)DS_PIX * (DS_NT / 64);
  hipLaunchKernelGGL(dense_decide_kernel<ND>, dim3((unsigned)((np + per_wg - 1) / per_wg)), dim3(DS_NT), 0, c->stream, dec);
}

// the launches on c->stream: the slots' level-0 planes and the left slot's mask, ordered behind their last writers
int vo_ds_enqueue(vo_ctx *c, vo_ds_buffers *b, int slot_l, int slot_r, const vo_dense_stereo_params *p, float *disp, uint16_t *cost, float *sigma,
                  uint8_t *status, int *W_out, int *H_out) {
  int rc = ds_check_params(c, p);
  if (rc) return rc;
  if (slot_l < 0 || slot_l >= c->cfg.n_slots || slot_r < 0 || slot_r >= c->cfg.n_slots || c->slots[slot_l].n_levels <= 0 ||
      c->slots[slot_r].n_levels <= 0)
    VO_FAIL(c, VO_ERR_INVALID, "slot holds no image");
  const vo_pyramid &Pl = c->slots[slot_l], &Pr = c->slots[slot_r];
  if (Pl.w != Pr.w || Pl.h != Pr.h) VO_FAIL(c, VO_ERR_SIZE, "image size mismatch");
  if (Pl.w > 65535 || Pl.h > 65535) VO_FAIL(c, VO_ERR_SIZE, "dense stereo: the image exceeds 65535 pixels a side");
  rc = ds_workspace_reserve(c, b, ds_workspace_bytes(Pl.w, Pl.h, p->n_disp));
  if (rc) return rc;
  if (vo_slot_acquire(c, slot_l) < 0 || vo_slot_acquire(c, slot_r) < 0) return VO_ERR_HIP;
  vo_mask_view mv;
  rc = vo_slot_mask_acquire(c, slot_l, &mv);
  if (rc) return rc;
  if (mv.p && (mv.w != Pl.w || mv.h != Pl.h)) VO_FAIL(c, VO_ERR_SIZE, "dense stereo: the left slot's mask is %d x %d, its image %d x %d", mv.w, mv.h, Pl.w, Pl.h);
  const size_t np = (size_t)Pl.w * (size_t)Pl.h;
  unsigned long long *cenL = (unsigned long long *)b->ws, *cenR = cenL + np;
  uint16_t *S = (uint16_t *)(cenR + np);
  DsCensusArgs ca;
  memset(&ca, 0, sizeof(ca));
  ca.img0 = Pl.lv[0].origin();
  ca.img1 = Pr.lv[0].origin();
  ca.stride0 = Pl.lv[0].stride;
  ca.stride1 = Pr.lv[0].stride;
  ca.W = Pl.w;
  ca.H = Pl.h;
  ca.cen0 = cenL;
  ca.cen1 = cenR;
  DsAggArgs ag;
  memset(&ag, 0, sizeof(ag));
  ag.cenL = cenL;
  ag.cenR = cenR;
  ag.S = S;
  ag.W = Pl.w;
  ag.H = Pl.h;
  ag.d_min = p->d_min;
  ag.p1 = p->p1;
  ag.p2 = p->p2;
  DsDecideArgs de;
  memset(&de, 0, sizeof(de));
  de.S = S;
  de.W = Pl.w;
  de.H = Pl.h;
  de.d_min = p->d_min;
  de.uniqueness = p->uniqueness;
  de.lr_max = p->lr_max;
  de.sigma = p->eps_d / p->bf;
  de.mask = mv.p;
  de.mask_stride = mv.stride;
  de.disp = disp;
  de.cost = cost;
  de.sigma_out = sigma;
  de.status = status;
  vo_prof_begin(c, VO_K_AUX);
  hipLaunchKernelGGL(dense_census_kernel, dim3((unsigned)((np + DS_NT - 1) / DS_NT), 2), dim3(DS_NT), 0, c->stream, ca);
  switch (p->n_disp / 64) {
    case 1: ds_launch<1>(c, ag, p->paths, de); break;
    case 2: ds_launch<2>(c, ag, p->paths, de); break;
    case 3: ds_launch<3>(c, ag, p->paths, de); break;
    default: ds_launch<4>(c, ag, p->paths, de); break;
  }
  vo_prof_end(c);
  VO_CHECK_HIP(c, hipGetLastError());
  if (W_out) *W_out = Pl.w;
  if (H_out) *H_out = Pl.h;
  return VO_OK;
}

extern "C" int vo_dense_stereo(vo_ctx *c, int slot_l, int slot_r, const vo_dense_stereo_params *prm, float *disparity, uint16_t *cost,
                               float *sigma_invd, uint8_t *status, int on_device) {
  if (!c || !prm) return VO_ERR_INVALID;
  VO_CHECK_HIP(c, hipSetDevice(c->device));
  hipStream_t s = c->stream;
  if (!c->dense_stereo) c->dense_stereo = new vo_dense_stereo_state();
  vo_ds_buffers *ws = &c->dense_stereo->ws;
  int W = 0, H = 0;
  if (on_device) {
    const int rc = vo_ds_enqueue(c, ws, slot_l, slot_r, prm, disparity, cost, sigma_invd, status, &W, &H);
    if (rc) return rc;
    VO_CHECK_HIP(c, hipStreamSynchronize(s));
    return VO_OK;
  }
  vo_sd_buffers *b;  // the context's planes (the cost in the score plane), shared with the semi-dense operator: every call is synchronous
  int rc = vo_sd_ctx_buffers(c, &b);
  if (rc) return rc;
  uint16_t *d_cost = (uint16_t *)b->score;
  rc = vo_ds_enqueue(c, ws, slot_l, slot_r, prm, disparity ? b->disp : nullptr, cost ? d_cost : nullptr, sigma_invd ? b->sigma : nullptr,
                     status ? b->status : nullptr, &W, &H);
  if (rc) return rc;
  const size_t n = (size_t)W * (size_t)H;
  if (disparity) VO_CHECK_HIP(c, hipMemcpyAsync(disparity, b->disp, n * sizeof(float), hipMemcpyDeviceToHost, s));
  if (cost) VO_CHECK_HIP(c, hipMemcpyAsync(cost, d_cost, n * sizeof(uint16_t), hipMemcpyDeviceToHost, s));
  if (sigma_invd) VO_CHECK_HIP(c, hipMemcpyAsync(sigma_invd, b->sigma, n * sizeof(float), hipMemcpyDeviceToHost, s));
  if (status) VO_CHECK_HIP(c, hipMemcpyAsync(status, b->status, n, hipMemcpyDeviceToHost, s));
  VO_CHECK_HIP(c, hipStreamSynchronize(s));
  return VO_OK;
}

// ---- StereoVO's hook: the rules of vo_svo_set_semidense (semidense.hip), with events of its own -----------------------------------
int vo_svo_dense_stereo_enqueue(vo_svo *s, int slot_l, int slot_r, int frame_id, const float T_wc[16]) {
  vo_ctx *c = s->c;
  vo_svo_dense_stereo &d = s->ds;
  VO_CHECK_HIP(c, hipEventRecord(d.fork, c->stream_main));
  VO_CHECK_HIP(c, hipStreamWaitEvent(c->stream2, d.fork, 0));
  hipStream_t keep = c->stream;
  c->stream = c->stream2;
  int rc = vo_ds_enqueue(c, &d.ws, slot_l, slot_r, &d.prm, d.buf.disp, (uint16_t *)d.buf.score, d.buf.sigma, d.buf.status, &d.w, &d.h);
  // vo_svo_set_dense_speckle: the filter's launches behind the decision, in place on the result's planes, in front of `done`
  if (!rc && d.spk_on) rc = vo_spk_enqueue(c, &d.spk, d.buf.disp, d.buf.sigma, d.buf.status, d.w, d.h, &d.spk_prm);
  c->stream = keep;
  if (rc) return rc;
  // vo_svo_set_semidense_world with a source that reads this result: a keyframe's planes are kept for the merge at its end
  if (s->sdw.on && s->sdw.source >= VO_SEMIDENSE_WORLD_DENSE) {
    rc = vo_svo_sdm_keep_dense(s, frame_id);
    if (rc) return rc;
  }
  VO_CHECK_HIP(c, hipEventRecord(d.done, c->stream2));
  d.have = true;
  d.spk_have = d.spk_on;
  d.busy |= (1u << slot_l) | (1u << slot_r);  // (launches follow each other on the side stream: `done` covers every earlier one)
  d.frame_id = frame_id;
  memcpy(d.T_wc, T_wc, sizeof(d.T_wc));
  return VO_OK;
}

// An ingestion is about to overwrite slots a and b: where launches since the last such wait read one of them, both streams an
// ingestion can run on are ordered behind their event — on the device; the host does not wait.
int vo_svo_dense_stereo_guard(vo_svo *s, int a, int b) {
  vo_svo_dense_stereo &d = s->ds;
  if (!(d.busy & ((1u << a) | (1u << b)))) return VO_OK;
  vo_ctx *c = s->c;
  VO_CHECK_HIP(c, hipStreamWaitEvent(c->stream_main, d.done, 0));
  VO_CHECK_HIP(c, hipStreamWaitEvent(c->stream2, d.done, 0));
  d.busy = 0;
  return VO_OK;
}

void vo_svo_dense_stereo_free(vo_svo *s) {
  vo_svo_dense_stereo &d = s->ds;
  if (d.have) (void)hipEventSynchronize(d.done);
  vo_ds_buffers_free(&d.ws);
  vo_spk_buffers_free(&d.spk);
  vo_sd_buffers_free(&d.buf);
  if (d.fork) (void)hipEventDestroy(d.fork);
  if (d.done) (void)hipEventDestroy(d.done);
  d = vo_svo_dense_stereo();
}

extern "C" int vo_svo_set_dense_stereo(vo_svo *s, const vo_dense_stereo_params *prm, int every) {
  if (!s) return VO_ERR_INVALID;
  vo_ctx *c = s->c;
  if (s->pending) VO_FAIL(c, VO_ERR_INVALID, "vo_svo_set_dense_stereo: a frame is in flight: call vo_svo_result first");
  if (s->mono) VO_FAIL(c, VO_ERR_INVALID, "vo_svo_set_dense_stereo: a stereo driver only");
  vo_svo_dense_stereo &d = s->ds;
  if (!prm) {
    d.on = false;
    return VO_OK;
  }
  if (every != VO_SEMIDENSE_KEYFRAMES && every != VO_SEMIDENSE_FRAMES)
    VO_FAIL(c, VO_ERR_INVALID, "vo_svo_set_dense_stereo: every=%d: expected VO_SEMIDENSE_KEYFRAMES (0) or VO_SEMIDENSE_FRAMES (1)", every);
  int rc = ds_check_params(c, prm);
  if (rc) return rc;
  VO_CHECK_HIP(c, hipSetDevice(c->device));
  if (!d.buf.disp) {  // the planes, the points list's scratch and the events: once
    rc = vo_sd_buffers_alloc(c, &d.buf);
    if (rc >= 0) rc = vo_sd_points_alloc(c, &d.buf);
    if (rc) return rc;
    VO_CHECK_HIP(c, hipEventCreateWithFlags(&d.fork, hipEventDisableTiming));
    VO_CHECK_HIP(c, hipEventCreateWithFlags(&d.done, hipEventDisableTiming));
  }
  // the workspace for the largest pair the context takes, here and not under a frame (it grows only when n_disp does; a launch that
  // still reads the old one is waited for first)
  if (d.have) VO_CHECK_HIP(c, hipEventSynchronize(d.done));
  rc = ds_workspace_reserve(c, &d.ws, ds_workspace_bytes(c->cfg.max_width, c->cfg.max_height, prm->n_disp));
  if (rc) return rc;
  d.prm = *prm;
  d.every = every;
  d.on = true;
  return VO_OK;
}

static int svo_ds_ready(vo_svo *s, const char *who) {
  vo_ctx *c = s->c;
  if (s->pending) VO_FAIL(c, VO_ERR_INVALID, "%s: a frame is in flight: call vo_svo_result first", who);
  if (s->mono) VO_FAIL(c, VO_ERR_INVALID, "%s: a stereo driver only", who);
  if (!s->ds.on) VO_FAIL(c, VO_ERR_INVALID, "%s: the option is off: vo_svo_set_dense_stereo", who);
  VO_CHECK_HIP(c, hipSetDevice(c->device));
  if (s->ds.have) VO_CHECK_HIP(c, hipEventSynchronize(s->ds.done));  // those launches only
  return VO_OK;
}

extern "C" int vo_svo_get_dense_stereo(vo_svo *s, float *disparity, uint16_t *cost, float *sigma_invd, uint8_t *status, int *width, int *height,
                                       int *frame_id, float T_wc[16], int *n_accepted) {
  if (!s || !width || !height) return VO_ERR_INVALID;
  const int rc = svo_ds_ready(s, "vo_svo_get_dense_stereo");
  if (rc) return rc;
  vo_ctx *c = s->c;
  const vo_svo_dense_stereo &d = s->ds;
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
  if (cost) VO_CHECK_HIP(c, hipMemcpy(cost, d.buf.score, n * sizeof(uint16_t), hipMemcpyDeviceToHost));
  if (sigma_invd) VO_CHECK_HIP(c, hipMemcpy(sigma_invd, d.buf.sigma, n * sizeof(float), hipMemcpyDeviceToHost));
  if (status) VO_CHECK_HIP(c, hipMemcpy(status, d.buf.status, n, hipMemcpyDeviceToHost));
  if (n_accepted) {  // counted here, from the status plane
    std::vector<uint8_t> st;
    const uint8_t *p = status;
    if (!p) {
      st.resize(n);
      VO_CHECK_HIP(c, hipMemcpy(st.data(), d.buf.status, n, hipMemcpyDeviceToHost));
      p = st.data();
    }
    int m = 0;
    for (size_t i = 0; i < n; ++i) m += p[i] == 1;
    *n_accepted = m;
  }
  return VO_OK;
}

extern "C" int vo_svo_get_dense_points(vo_svo *s, int world, int cap, float *xyz, float *sigma_invd, uint16_t *pixel, int *n, int *frame_id) {
  if (!s || !n || cap < 0 || (cap > 0 && !xyz)) return VO_ERR_INVALID;
  const int rc = svo_ds_ready(s, "vo_svo_get_dense_points");
  if (rc) return rc;
  vo_svo_dense_stereo &d = s->ds;
  *n = 0;
  if (frame_id) *frame_id = d.have ? d.frame_id : -1;
  if (!d.have) return VO_OK;
  return vo_sd_points(s->c, &d.buf, d.buf.disp, d.buf.sigma, d.buf.status, d.w, d.h, s->prm.frame.Kl, d.prm.bf, world ? d.T_wc : nullptr, cap, xyz,
                      sigma_invd, pixel, n);
}
