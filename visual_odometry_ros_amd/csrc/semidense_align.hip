// semidense_align.hip — direct image alignment on the semi-dense map (include/vo_hip.h, "Semi-dense alignment"): the
// operator (vo_semidense_align) and StereoVO's hook (vo_svo_set_semidense_align, vo_svo_get_semidense_align; the launches are
// placed by vo_svo_semidense_temporal_enqueue in front of the frame's temporal launch). semidense_align_device.hpp has the kernel.
// Below them the same alignment coarse to fine on a map pyramid ("Semi-dense alignment on a map pyramid"):
// vo_semidense_map_pyramid, vo_semidense_align_pyr, vo_svo_set_semidense_align_pyr, vo_svo_get_semidense_align_pyr;
// semidense_map_pyramid_device.hpp has the map pyramid's kernel. At the end either with affine brightness ("Semi-dense alignment with
// affine brightness"): vo_semidense_align_affine, vo_semidense_align_pyr_affine, vo_svo_set_semidense_align_affine,
// vo_svo_get_semidense_align_affine; semidense_align_affine_device.hpp has that kernel.
#include "stereo_vo.hpp"
#include "vo_internal.hpp"
#include "vo_kernels.hpp"

#include <math.h>

__device__ __forceinline__ int sda_wave_rank(bool p, int *n) {
  const unsigned long long m = __ballot(p);
  *n = __popcll(m);
  return __popcll(m & ((1ull << (threadIdx.x & 63)) - 1ull));
}
#define SDA_DRAIN() asm volatile("s_waitcnt vmcnt(0)" ::: "memory")
#define SDA_ST_AGENT(p, v) __hip_atomic_store((p), (v), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)
#define SDA_ATOMIC_ADD_AGENT(p, v) __hip_atomic_fetch_add((p), (v), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)
// (the explicit wait behind either fence: the release has been performed before the ticket is taken, the invalidate before the
// barrier that lets the other wavefronts load)
#define SDA_FENCE_RELEASE()                             \
  do {                                                  \
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");  \
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");    \
  } while (0)
#define SDA_FENCE_ACQUIRE()                             \
  do {                                                  \
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");  \
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");    \
  } while (0)
#include "semidense_align_device.hpp"
#include "semidense_align_affine_device.hpp"
#include "semidense_map_pyramid_device.hpp"

extern "C" int vo_semidense_align_default_params(vo_semidense_align_params *p) {
  if (!p) return VO_ERR_INVALID;
  memset(p, 0, sizeof(*p));
  p->min_obs = 1;
  p->huber = 10.0f;
  p->max_iters = 10;
  p->eps = 1e-4f;
  p->min_pixels = 100;
  return VO_OK;
}

static int sda_check_params(vo_ctx *c, const vo_semidense_align_params *p) {
  if (p->min_obs < 1 || p->min_obs > 255) VO_FAIL(c, VO_ERR_INVALID, "semi-dense alignment: min_obs=%d: expected 1..255", p->min_obs);
  if (!(p->huber > 0.0f) || !(p->huber <= 255.0f)) VO_FAIL(c, VO_ERR_INVALID, "semi-dense alignment: huber: expected 0 < huber <= 255 grey levels");
  if (p->max_iters < 1 || p->max_iters > SDA_MAX_ITERS)
    VO_FAIL(c, VO_ERR_INVALID, "semi-dense alignment: max_iters=%d: expected 1..%d", p->max_iters, SDA_MAX_ITERS);
  if (!(p->eps >= 0.0f) || !isfinite(p->eps)) VO_FAIL(c, VO_ERR_INVALID, "semi-dense alignment: eps is finite and >= 0");
  if (p->min_pixels < 6) VO_FAIL(c, VO_ERR_INVALID, "semi-dense alignment: min_pixels=%d: expected >= 6", p->min_pixels);
  return VO_OK;
}

// ---- buffers ----------------------------------------------------------------------------------------------------------------------
// One allocation: the state block and the blocks' rows of partial sums, sized by vo_config.max_width x max_height. The ticket
// starts at zero and every launch leaves it there.
static int sda_buffers_alloc(vo_ctx *c, vo_sda_buffers *b, size_t state_bytes, size_t nsum) {
  if (b->base) return VO_OK;
  const size_t n = (size_t)c->cfg.max_width * (size_t)c->cfg.max_height, nb = (n + SDA_BLOCK - 1) / SDA_BLOCK;
  const size_t head = (state_bytes + 255) & ~(size_t)255;
  VO_CHECK_HIP(c, hipSetDevice(c->device));
  VO_CHECK_HIP(c, vo_dev_malloc(c, &b->base, head + nb * nsum * sizeof(long long)));
  b->state = b->base;
  b->partial = (long long *)((uint8_t *)b->base + head);
  b->n_blocks = nb;
  VO_CHECK_HIP(c, hipMemsetAsync(b->base, 0, head, c->stream));
  VO_CHECK_HIP(c, hipStreamSynchronize(c->stream));  // (the launches may run on another stream)
  return VO_OK;
}
int vo_sda_buffers_alloc(vo_ctx *c, vo_sda_buffers *b) { return sda_buffers_alloc(c, b, sizeof(SdaState), SDA_NSUM); }
int vo_sdaa_buffers_alloc(vo_ctx *c, vo_sda_buffers *b) { return sda_buffers_alloc(c, b, sizeof(SdaaState), SDAA_NSUM); }
void vo_sda_buffers_free(vo_sda_buffers *b) {
  if (b->base) (void)hipFree(b->base);
  *b = vo_sda_buffers();
}

struct vo_semidense_align_state {
  vo_sda_buffers buf;
  vo_sdm_pyramid py;  // vo_semidense_align_pyr / vo_semidense_map_pyramid: levels 1..5 of the map
  vo_sda_buffers abuf;  // vo_semidense_align_affine / vo_semidense_align_pyr_affine
};
void vo_semidense_align_free(vo_ctx *c) {
  if (!c->semidense_a) return;
  vo_sda_buffers_free(&c->semidense_a->buf);
  vo_sda_buffers_free(&c->semidense_a->abuf);
  vo_sdm_pyramid_free(&c->semidense_a->py);
  delete c->semidense_a;
  c->semidense_a = nullptr;
}

// ---- the launches -------------------------------------------------------------------------------------------------------------------
// max_iters launches on c->stream, back to back: DEVICE planes throughout. Nothing waits.
int vo_sda_enqueue(vo_ctx *c, vo_sda_buffers *b, const uint8_t *d_key, int key_stride, int slot_cur, const float K[4], const float T_ck[16],
                   const vo_semidense_align_params *p, const float *invd, const float *sigma, const uint8_t *n_obs) {
  int rc = sda_check_params(c, p);
  if (rc) return rc;
  if (slot_cur < 0 || slot_cur >= c->cfg.n_slots || c->slots[slot_cur].n_levels <= 0) VO_FAIL(c, VO_ERR_INVALID, "slot holds no image");
  const vo_pyramid &P = c->slots[slot_cur];
  if (P.w < 3 || P.h < 3 || P.w > 65535 || P.h > 65535 || (long long)P.w * P.h > 0x7FFFFFFFll)
    VO_FAIL(c, VO_ERR_SIZE, "semi-dense alignment: the image must have 3 .. 65535 pixels a side and fewer than 2^31 in all");
  if (key_stride < P.w) VO_FAIL(c, VO_ERR_INVALID, "semi-dense alignment: key_stride %d below the width %d", key_stride, P.w);
  if (!(K[0] > 0.0f) || !(K[1] > 0.0f) || !isfinite(K[0]) || !isfinite(K[1]) || !isfinite(K[2]) || !isfinite(K[3]))
    VO_FAIL(c, VO_ERR_INVALID, "semi-dense alignment: fx, fy must be positive, K finite");
  for (int i = 0; i < 12; ++i)
    if (!isfinite(T_ck[i])) VO_FAIL(c, VO_ERR_INVALID, "semi-dense alignment: T_ck is not finite");
  SdaArgs a;
  memset(&a, 0, sizeof(a));
  a.n_blocks = (int)(((size_t)P.w * (size_t)P.h + SDA_BLOCK - 1) / SDA_BLOCK);
  if ((size_t)a.n_blocks > b->n_blocks) VO_FAIL(c, VO_ERR_SIZE, "%d x %d planes exceed vo_config.max_width x max_height", P.w, P.h);
  if (vo_slot_acquire(c, slot_cur) < 0) return VO_ERR_HIP;
  a.Lk = d_key;
  a.Lc = P.lv[0].origin();
  a.strideK = key_stride;
  a.strideC = P.lv[0].stride;
  a.W = P.w;
  a.H = P.h;
  a.invd = invd;
  a.sigma = sigma;
  a.n_obs = n_obs;
  sda_params(&a, p->min_obs, p->huber, p->max_iters, p->eps, p->min_pixels);
  a.fx = K[0], a.fy = K[1], a.cx = K[2], a.cy = K[3];
  for (int i = 0; i < 12; ++i) a.T0[i] = T_ck[i];
  a.partial = b->partial;
  a.st = (SdaState *)b->state;
  vo_prof_begin(c, VO_K_AUX);
  for (int it = 0; it < p->max_iters; ++it) {
    a.first = it == 0;
    hipLaunchKernelGGL(semidense_align_kernel, dim3((unsigned)a.n_blocks), dim3(SDA_NT), 0, c->stream, a);
  }
  vo_prof_end(c);
  VO_CHECK_HIP(c, hipGetLastError());
  return VO_OK;
}

// the state block (the caller has waited for its launches) as a result
static int sda_fetch(vo_ctx *c, const vo_sda_buffers *b, vo_semidense_align_result *res) {
  SdaState st;
  VO_CHECK_HIP(c, hipMemcpy(&st, b->state, sizeof(st), hipMemcpyDeviceToHost));
  memcpy(res->T_ck, st.T, sizeof(st.T));
  res->status = st.status;
  res->iters = st.iters;
  res->count = st.count;
  res->rms = st.sw > 0.0 ? sqrt(st.swrr / st.sw) / 16.0 : 0.0;
  memcpy(res->H, st.H, sizeof(st.H));
  memcpy(res->b, st.b, sizeof(st.b));
  return VO_OK;
}

extern "C" int vo_semidense_align(vo_ctx *c, const uint8_t *key_plane, int key_stride, int key_on_device, int slot_cur, const float K[4],
                                  const float T_ck[16], const vo_semidense_align_params *prm, const float *invd, const float *sigma,
                                  const uint8_t *n_obs, int on_device, vo_semidense_align_result *res) {
  if (!c || !key_plane || !K || !T_ck || !prm || !invd || !sigma || !n_obs || !res) return VO_ERR_INVALID;
  VO_CHECK_HIP(c, hipSetDevice(c->device));
  hipStream_t s = c->stream;
  if (slot_cur < 0 || slot_cur >= c->cfg.n_slots || c->slots[slot_cur].n_levels <= 0) VO_FAIL(c, VO_ERR_INVALID, "slot holds no image");
  const int W = c->slots[slot_cur].w, H = c->slots[slot_cur].h;
  if (key_stride < W) VO_FAIL(c, VO_ERR_INVALID, "semi-dense alignment: key_stride %d below the width %d", key_stride, W);
  int rc = sda_check_params(c, prm);  // (before any copy reads the caller's memory)
  if (rc) return rc;
  const size_t np = (size_t)W * (size_t)H;
  if (!c->semidense_a) c->semidense_a = new vo_semidense_align_state();
  vo_sda_buffers *b = &c->semidense_a->buf;
  rc = vo_sda_buffers_alloc(c, b);
  if (rc) return rc;
  vo_sdt_buffers *m = nullptr;  // the device copies of host planes
  if (!key_on_device || !on_device) {
    rc = vo_sdt_ctx_buffers(c, &m);
    if (rc) return rc;
  }
  const uint8_t *d_key = key_plane;
  int d_stride = key_stride;
  if (!key_on_device) {
    VO_CHECK_HIP(c, hipMemcpy2DAsync(m->key, (size_t)W, key_plane, (size_t)key_stride, (size_t)W, (size_t)H, hipMemcpyHostToDevice, s));
    d_key = m->key;
    d_stride = W;
  }
  if (!on_device) {
    VO_CHECK_HIP(c, hipMemcpyAsync(m->invd, invd, np * sizeof(float), hipMemcpyHostToDevice, s));
    VO_CHECK_HIP(c, hipMemcpyAsync(m->sigma, sigma, np * sizeof(float), hipMemcpyHostToDevice, s));
    VO_CHECK_HIP(c, hipMemcpyAsync(m->n_obs, n_obs, np, hipMemcpyHostToDevice, s));
    invd = m->invd, sigma = m->sigma, n_obs = m->n_obs;
  }
  rc = vo_sda_enqueue(c, b, d_key, d_stride, slot_cur, K, T_ck, prm, invd, sigma, n_obs);
  VO_CHECK_HIP(c, hipStreamSynchronize(s));  // (the copies read the caller's memory)
  if (rc) return rc;
  return sda_fetch(c, b, res);
}

// ---- StereoVO's hook ------------------------------------------------------------------------------------------------------------------
// Called by vo_svo_semidense_temporal_enqueue at a frame that is not a keyframe, on the side stream behind the fork event and in
// front of that frame's temporal launch: the alignment reads the map as the previous frames left it.
static int svo_sda_enqueue_pyr(vo_svo *s, int slot_l, const float T_ck[16]);
static int svo_sdaa_enqueue_level0(vo_svo *s, int slot_l, const float T_ck[16]);
static int sdaa_fetch_plain(vo_ctx *c, const vo_sda_buffers *b, int levels, vo_semidense_align_pyr_result *res);
int vo_svo_semidense_align_enqueue(vo_svo *s, int slot_l, int frame_id, const float T_ck[16]) {
  vo_ctx *c = s->c;
  vo_svo_semidense_temporal &t = s->sdt;
  vo_svo_semidense_align &g = s->sda;
  g.have = false;  // (should the launch be refused, this frame has no result)
  const int rc = g.pyr      ? svo_sda_enqueue_pyr(s, slot_l, T_ck)
                 : g.affine ? svo_sdaa_enqueue_level0(s, slot_l, T_ck)
                            : vo_sda_enqueue(c, &g.buf, t.buf.key, t.w, slot_l, s->prm.frame.Kl, T_ck, &g.prm, t.buf.invd, t.buf.sigma, t.buf.n_obs);
  if (rc > 0) return VO_OK;  // (the coarse-to-fine option came on behind this keyframe: no result until the next one)
  if (rc) return rc;
  g.have = true;
  g.frame_id = frame_id;
  g.key_frame_id = t.frame_id;
  memcpy(g.T_wk, t.T_wk, sizeof(g.T_wk));
  return VO_OK;
}

void vo_svo_semidense_align_free(vo_svo *s) {
  vo_sda_buffers_free(&s->sda.buf);
  vo_sda_buffers_free(&s->sda.abuf);
  vo_sdm_pyramid_free(&s->sda.py);
  s->sda = vo_svo_semidense_align();
}

extern "C" int vo_svo_set_semidense_align(vo_svo *s, const vo_semidense_align_params *prm) {
  if (!s) return VO_ERR_INVALID;
  vo_ctx *c = s->c;
  if (s->pending) VO_FAIL(c, VO_ERR_INVALID, "vo_svo_set_semidense_align: a frame is in flight: call vo_svo_result first");
  if (s->mono) VO_FAIL(c, VO_ERR_INVALID, "vo_svo_set_semidense_align: a stereo driver only");
  vo_svo_semidense_align &g = s->sda;
  if (!prm) {
    g.on = g.pyr = g.affine = false;
    g.have = false;
    return VO_OK;
  }
  if (!s->sdt.on || !s->sd.on)
    VO_FAIL(c, VO_ERR_INVALID, "vo_svo_set_semidense_align: needs the temporal option: vo_svo_set_semidense_temporal first");
  int rc = sda_check_params(c, prm);
  if (rc) return rc;
  rc = vo_sda_buffers_alloc(c, &g.buf);  // the option's only allocation, at the first enable
  if (rc) return rc;
  g.prm = *prm;
  if (!g.on || g.pyr) g.have = false, g.frame_id = -1;
  g.on = true;
  g.pyr = false;
  return VO_OK;
}

extern "C" int vo_svo_get_semidense_align(vo_svo *s, vo_semidense_align_result *res, float T_wc[16], int *frame_id, int *key_frame_id) {
  if (!s || !res) return VO_ERR_INVALID;
  vo_ctx *c = s->c;
  if (s->pending) VO_FAIL(c, VO_ERR_INVALID, "vo_svo_get_semidense_align: a frame is in flight: call vo_svo_result first");
  if (!s->sda.on || !s->sdt.on || !s->sd.on) VO_FAIL(c, VO_ERR_INVALID, "vo_svo_get_semidense_align: the option is off: vo_svo_set_semidense_align");
  VO_CHECK_HIP(c, hipSetDevice(c->device));
  const vo_svo_semidense_align &g = s->sda;
  memset(res, 0, sizeof(*res));
  res->status = VO_SEMIDENSE_ALIGN_NONE;
  res->T_ck[0] = res->T_ck[5] = res->T_ck[10] = res->T_ck[15] = 1.0f;
  if (frame_id) *frame_id = g.frame_id;
  if (key_frame_id) *key_frame_id = g.have ? g.key_frame_id : -1;
  if (T_wc)
    for (int i = 0; i < 16; ++i) T_wc[i] = (i % 5 == 0) ? 1.0f : 0.0f;
  if (!g.have) return VO_OK;  // a keyframe frame, or no frame yet
  if (s->sd.have) VO_CHECK_HIP(c, hipEventSynchronize(s->sd.done));  // the side stream's last launch only
  int rc;
  if (g.affine) {  // vo_svo_set_semidense_align_affine: the affine run's result, H and b cut to the pose's rows and columns
    vo_semidense_align_pyr_result full;
    rc = sdaa_fetch_plain(c, &g.abuf, 1, &full);
    memcpy(res->T_ck, full.T_ck, sizeof(res->T_ck));
    res->status = full.status, res->iters = full.iters, res->count = full.count, res->rms = full.rms;
    memcpy(res->H, full.H, sizeof(res->H));
    memcpy(res->b, full.b, sizeof(res->b));
  } else {
    rc = sda_fetch(c, &g.buf, res);
  }
  if (rc) return rc;
  if (T_wc) {  // T_wk * inverseSE3(T_ck), on the host in float, in svo_mul44's order
    float T_kc[16];
    svo_inv_se3(res->T_ck, T_kc);
    svo_mul44(g.T_wk, T_kc, T_wc);
  }
  return VO_OK;
}

// ==== coarse to fine on a map pyramid (include/vo_hip.h, "Semi-dense alignment on a map pyramid") ======================
static inline void sdm_level_size(int l, int *w, int *h) {
  for (int i = 0; i < l; ++i) *w = (*w + 1) / 2, *h = (*h + 1) / 2;
}

extern "C" int vo_semidense_align_pyr_default_params(vo_semidense_align_pyr_params *p) {
  if (!p) return VO_ERR_INVALID;
  memset(p, 0, sizeof(*p));
  p->min_obs = 1;
  p->huber = 10.0f;
  p->max_iters = 10;
  p->eps = 1e-4f;
  p->min_pixels = 100;
  p->levels = 4;  // max_iters_level: 0 = max_iters
  return VO_OK;
}

static inline int sda_level_iters(const vo_semidense_align_pyr_params *p, int l) { return p->max_iters_level[l] > 0 ? p->max_iters_level[l] : p->max_iters; }

static int sda_check_pyr_params(vo_ctx *c, const vo_semidense_align_pyr_params *p) {
  vo_semidense_align_params q = {p->min_obs, p->huber, p->max_iters, p->eps, p->min_pixels};
  const int rc = sda_check_params(c, &q);
  if (rc) return rc;
  if (p->levels < 1 || p->levels > SDA_MAX_LEVELS) VO_FAIL(c, VO_ERR_INVALID, "semi-dense alignment: levels=%d: expected 1..%d", p->levels, SDA_MAX_LEVELS);
  for (int l = 0; l < p->levels; ++l)
    if (p->max_iters_level[l] < 0 || p->max_iters_level[l] > SDA_MAX_ITERS)
      VO_FAIL(c, VO_ERR_INVALID, "semi-dense alignment: max_iters_level[%d]=%d: expected 0..%d", l, p->max_iters_level[l], SDA_MAX_ITERS);
  return VO_OK;
}

extern "C" int vo_semidense_map_pyramid_size(int width, int height, int levels, long long *elements) {
  if (!elements || width < 1 || height < 1 || levels < 1 || levels > SDM_MAX_LEVELS) return VO_ERR_INVALID;
  long long n = 0;
  for (int l = 1; l < levels; ++l) {
    int w = width, h = height;
    sdm_level_size(l, &w, &h);
    n += (long long)w * h;
  }
  *elements = n;
  return VO_OK;
}

// One allocation: per level 1..5 of vo_config.max_width x max_height the map's three planes and, for a driver, the key image's.
int vo_sdm_pyramid_alloc(vo_ctx *c, vo_sdm_pyramid *py, bool with_key) {
  if (py->base) return VO_OK;
  size_t off[SDM_MAX_LEVELS][4], total = 0;
  for (int l = 1; l < SDM_MAX_LEVELS; ++l) {
    int w = c->cfg.max_width, h = c->cfg.max_height;
    sdm_level_size(l, &w, &h);
    const size_t n = (size_t)w * (size_t)h;
    const size_t bytes[4] = {n * sizeof(float), n * sizeof(float), n, with_key ? n : 0};
    for (int k = 0; k < 4; ++k) {
      off[l][k] = total;
      total += (bytes[k] + 255) & ~(size_t)255;
    }
  }
  VO_CHECK_HIP(c, hipSetDevice(c->device));
  VO_CHECK_HIP(c, vo_dev_malloc(c, &py->base, total));
  uint8_t *base = (uint8_t *)py->base;
  for (int l = 1; l < SDM_MAX_LEVELS; ++l) {
    py->invd[l] = (float *)(base + off[l][0]);
    py->sigma[l] = (float *)(base + off[l][1]);
    py->n_obs[l] = base + off[l][2];
    py->key[l] = with_key ? base + off[l][3] : nullptr;
  }
  return VO_OK;
}
void vo_sdm_pyramid_free(vo_sdm_pyramid *py) {
  if (py->base) (void)hipFree(py->base);
  *py = vo_sdm_pyramid();
}

int vo_sdm_enqueue(vo_ctx *c, int w, int h, int levels, float *const invd[], float *const sigma[], uint8_t *const n_obs[]) {
  if (levels < 1 || levels > SDM_MAX_LEVELS) VO_FAIL(c, VO_ERR_INVALID, "semi-dense map pyramid: levels=%d: expected 1..%d", levels, SDM_MAX_LEVELS);
  if (w < 1 || h < 1 || (long long)w * h > 0x7FFFFFFFll) VO_FAIL(c, VO_ERR_SIZE, "semi-dense map pyramid: %d x %d planes", w, h);
  vo_prof_begin(c, VO_K_AUX);
  for (int l = 1; l < levels; ++l) {
    SdmArgs a;
    a.invd = invd[l - 1], a.sigma = sigma[l - 1], a.n_obs = n_obs[l - 1];
    a.w = w, a.h = h;
    w = (w + 1) / 2, h = (h + 1) / 2;
    a.o_invd = invd[l], a.o_sigma = sigma[l], a.o_n_obs = n_obs[l];
    a.wc = w, a.hc = h;
    const size_t nc = (size_t)w * (size_t)h;
    hipLaunchKernelGGL(semidense_map_pyramid_kernel, dim3((unsigned)((nc + SDM_NT - 1) / SDM_NT)), dim3(SDM_NT), 0, c->stream, a);
  }
  vo_prof_end(c);
  VO_CHECK_HIP(c, hipGetLastError());
  return VO_OK;
}

// the operators' buffers: the level-0 operator's state, and levels 1..5 of a map
static int sda_ctx_state(vo_ctx *c, bool pyramid) {
  if (!c->semidense_a) c->semidense_a = new vo_semidense_align_state();
  return pyramid ? vo_sdm_pyramid_alloc(c, &c->semidense_a->py, false) : VO_OK;
}

extern "C" int vo_semidense_map_pyramid(vo_ctx *c, const float *invd, const float *sigma, const uint8_t *n_obs, int width, int height, int levels,
                                        float *invd_pyr, float *sigma_pyr, uint8_t *n_obs_pyr, int on_device) {
  if (!c || !invd || !sigma || !n_obs || !invd_pyr || !sigma_pyr || !n_obs_pyr) return VO_ERR_INVALID;
  VO_CHECK_HIP(c, hipSetDevice(c->device));
  if (levels < 2 || levels > SDM_MAX_LEVELS) VO_FAIL(c, VO_ERR_INVALID, "semi-dense map pyramid: levels=%d: expected 2..%d", levels, SDM_MAX_LEVELS);
  if (width < 1 || height < 1 || width > c->cfg.max_width || height > c->cfg.max_height)
    VO_FAIL(c, VO_ERR_SIZE, "semi-dense map pyramid: %d x %d planes: expected 1 x 1 .. vo_config.max_width x max_height", width, height);
  hipStream_t s = c->stream;
  const size_t np = (size_t)width * (size_t)height;
  float *pi[SDM_MAX_LEVELS] = {}, *ps[SDM_MAX_LEVELS] = {};
  uint8_t *pn[SDM_MAX_LEVELS] = {};
  int rc;
  if (on_device) {
    pi[0] = (float *)invd, ps[0] = (float *)sigma, pn[0] = (uint8_t *)n_obs;  // (level 0 is read only)
    size_t off = 0;
    for (int l = 1; l < levels; ++l) {
      int w = width, h = height;
      sdm_level_size(l, &w, &h);
      pi[l] = invd_pyr + off, ps[l] = sigma_pyr + off, pn[l] = n_obs_pyr + off;
      off += (size_t)w * (size_t)h;
    }
    rc = vo_sdm_enqueue(c, width, height, levels, pi, ps, pn);
    VO_CHECK_HIP(c, hipStreamSynchronize(s));
    return rc;
  }
  rc = sda_ctx_state(c, true);
  if (rc) return rc;
  vo_sdt_buffers *m = nullptr;  // the device copies of host planes
  rc = vo_sdt_ctx_buffers(c, &m);
  if (rc) return rc;
  const vo_sdm_pyramid &py = c->semidense_a->py;
  VO_CHECK_HIP(c, hipMemcpyAsync(m->invd, invd, np * sizeof(float), hipMemcpyHostToDevice, s));
  VO_CHECK_HIP(c, hipMemcpyAsync(m->sigma, sigma, np * sizeof(float), hipMemcpyHostToDevice, s));
  VO_CHECK_HIP(c, hipMemcpyAsync(m->n_obs, n_obs, np, hipMemcpyHostToDevice, s));
  pi[0] = m->invd, ps[0] = m->sigma, pn[0] = m->n_obs;
  for (int l = 1; l < levels; ++l) pi[l] = py.invd[l], ps[l] = py.sigma[l], pn[l] = py.n_obs[l];
  rc = vo_sdm_enqueue(c, width, height, levels, pi, ps, pn);
  size_t off = 0;
  for (int l = 1; l < levels && !rc; ++l) {
    int w = width, h = height;
    sdm_level_size(l, &w, &h);
    const size_t n = (size_t)w * (size_t)h;
    VO_CHECK_HIP(c, hipMemcpyAsync(invd_pyr + off, pi[l], n * sizeof(float), hipMemcpyDeviceToHost, s));
    VO_CHECK_HIP(c, hipMemcpyAsync(sigma_pyr + off, ps[l], n * sizeof(float), hipMemcpyDeviceToHost, s));
    VO_CHECK_HIP(c, hipMemcpyAsync(n_obs_pyr + off, pn[l], n, hipMemcpyDeviceToHost, s));
    off += n;
  }
  VO_CHECK_HIP(c, hipStreamSynchronize(s));
  return rc;
}

int vo_sda_enqueue_pyr(vo_ctx *c, vo_sda_buffers *b, const uint8_t *const key[], const int key_stride[], int slot_cur, const float K[4],
                       const float T_ck[16], const vo_semidense_align_pyr_params *p, const float *const invd[], const float *const sigma[],
                       const uint8_t *const n_obs[], int first) {
  int rc = sda_check_pyr_params(c, p);
  if (rc) return rc;
  if (slot_cur < 0 || slot_cur >= c->cfg.n_slots || c->slots[slot_cur].n_levels <= 0) VO_FAIL(c, VO_ERR_INVALID, "slot holds no image");
  const vo_pyramid &P = c->slots[slot_cur];
  const int L = p->levels;
  VO_NEED_LEVELS(c, P, L - 1);
  if (P.w > 65535 || P.h > 65535 || (long long)P.w * P.h > 0x7FFFFFFFll)
    VO_FAIL(c, VO_ERR_SIZE, "semi-dense alignment: the image must have 3 .. 65535 pixels a side and fewer than 2^31 in all");
  for (int l = 0; l < L; ++l) {
    int w = P.w, h = P.h;
    sdm_level_size(l, &w, &h);
    if (w != P.lv[l].w || h != P.lv[l].h) VO_FAIL(c, VO_ERR_INVALID, "semi-dense alignment: level %d of the slot is %d x %d, expected %d x %d", l, P.lv[l].w, P.lv[l].h, w, h);
    if (w < 3 || h < 3) VO_FAIL(c, VO_ERR_SIZE, "semi-dense alignment: level %d is %d x %d: every used level needs 3 pixels a side", l, w, h);
    if (key_stride[l] < w) VO_FAIL(c, VO_ERR_INVALID, "semi-dense alignment: level %d: key_stride %d below the width %d", l, key_stride[l], w);
  }
  if (!(K[0] > 0.0f) || !(K[1] > 0.0f) || !isfinite(K[0]) || !isfinite(K[1]) || !isfinite(K[2]) || !isfinite(K[3]))
    VO_FAIL(c, VO_ERR_INVALID, "semi-dense alignment: fx, fy must be positive, K finite");
  for (int i = 0; i < 12; ++i)
    if (!isfinite(T_ck[i])) VO_FAIL(c, VO_ERR_INVALID, "semi-dense alignment: T_ck is not finite");
  if (((size_t)P.w * (size_t)P.h + SDA_BLOCK - 1) / SDA_BLOCK > b->n_blocks)
    VO_FAIL(c, VO_ERR_SIZE, "%d x %d planes exceed vo_config.max_width x max_height", P.w, P.h);
  if (vo_slot_acquire(c, slot_cur) < 0) return VO_ERR_HIP;
  SdaArgs a;
  memset(&a, 0, sizeof(a));
  sda_params(&a, p->min_obs, p->huber, p->max_iters, p->eps, p->min_pixels);
  for (int i = 0; i < 12; ++i) a.T0[i] = T_ck[i];
  a.partial = b->partial;
  a.st = (SdaState *)b->state;
  vo_prof_begin(c, VO_K_AUX);
  for (int l = L - 1; l >= 0; --l) {
    const float s = 1.0f / (float)(1 << l);  // (a power of two: the products are exact)
    a.Lk = key[l];
    a.Lc = P.lv[l].origin();
    a.strideK = key_stride[l];
    a.strideC = P.lv[l].stride;
    a.W = P.lv[l].w;
    a.H = P.lv[l].h;
    a.invd = invd[l], a.sigma = sigma[l], a.n_obs = n_obs[l];
    a.fx = K[0] * s, a.fy = K[1] * s, a.cx = K[2] * s, a.cy = K[3] * s;
    a.n_blocks = (int)(((size_t)a.W * (size_t)a.H + SDA_BLOCK - 1) / SDA_BLOCK);
    a.level = l;
    a.max_iters = sda_level_iters(p, l);
    for (int it = 0; it < a.max_iters; ++it) {
      a.first = it > 0 ? 0 : (l == L - 1 ? first : SDA_FIRST_LEVEL);
      hipLaunchKernelGGL(semidense_align_kernel, dim3((unsigned)a.n_blocks), dim3(SDA_NT), 0, c->stream, a);
    }
  }
  vo_prof_end(c);
  VO_CHECK_HIP(c, hipGetLastError());
  return VO_OK;
}

static int sda_fetch_pyr(vo_ctx *c, const vo_sda_buffers *b, int levels, vo_semidense_align_pyr_result *res) {
  SdaState st;
  VO_CHECK_HIP(c, hipMemcpy(&st, b->state, sizeof(st), hipMemcpyDeviceToHost));
  memset(res, 0, sizeof(*res));
  memcpy(res->T_ck, st.T, sizeof(st.T));
  res->status = st.status;
  res->iters = st.iters;
  res->count = st.count;
  res->rms = st.sw > 0.0 ? sqrt(st.swrr / st.sw) / 16.0 : 0.0;
  memcpy(res->H, st.H, sizeof(st.H));
  memcpy(res->b, st.b, sizeof(st.b));
  res->levels = levels;
  res->start_prev = st.start_prev;
  for (int l = 0; l < levels; ++l) {
    res->level_status[l] = st.lv[l].status;
    res->level_iters[l] = st.lv[l].iters;
    res->level_count[l] = st.lv[l].count;
    res->level_rms[l] = st.lv[l].sw > 0.0 ? sqrt(st.lv[l].swrr / st.lv[l].sw) / 16.0 : 0.0;
  }
  return VO_OK;
}

extern "C" int vo_semidense_align_pyr(vo_ctx *c, int slot_key, int slot_cur, const float K[4], const float T_ck[16],
                                      const vo_semidense_align_pyr_params *prm, const float *invd, const float *sigma, const uint8_t *n_obs,
                                      int on_device, vo_semidense_align_pyr_result *res) {
  if (!c || !K || !T_ck || !prm || !invd || !sigma || !n_obs || !res) return VO_ERR_INVALID;
  VO_CHECK_HIP(c, hipSetDevice(c->device));
  hipStream_t s = c->stream;
  for (int slot : {slot_key, slot_cur})
    if (slot < 0 || slot >= c->cfg.n_slots || c->slots[slot].n_levels <= 0) VO_FAIL(c, VO_ERR_INVALID, "slot %d holds no image", slot);
  const vo_pyramid &Pk = c->slots[slot_key], &Pc = c->slots[slot_cur];
  if (Pk.w != Pc.w || Pk.h != Pc.h) VO_FAIL(c, VO_ERR_SIZE, "semi-dense alignment: the slots' images differ in size");
  int rc = sda_check_pyr_params(c, prm);  // (before any copy reads the caller's memory)
  if (rc) return rc;
  const int L = prm->levels;
  VO_NEED_LEVELS(c, Pk, L - 1);
  VO_NEED_LEVELS(c, Pc, L - 1);
  const size_t np = (size_t)Pc.w * (size_t)Pc.h;
  rc = sda_ctx_state(c, L > 1);
  if (rc) return rc;
  vo_sda_buffers *b = &c->semidense_a->buf;
  rc = vo_sda_buffers_alloc(c, b);
  if (rc) return rc;
  if (!on_device) {
    vo_sdt_buffers *m = nullptr;  // the device copies of host planes
    rc = vo_sdt_ctx_buffers(c, &m);
    if (rc) return rc;
    VO_CHECK_HIP(c, hipMemcpyAsync(m->invd, invd, np * sizeof(float), hipMemcpyHostToDevice, s));
    VO_CHECK_HIP(c, hipMemcpyAsync(m->sigma, sigma, np * sizeof(float), hipMemcpyHostToDevice, s));
    VO_CHECK_HIP(c, hipMemcpyAsync(m->n_obs, n_obs, np, hipMemcpyHostToDevice, s));
    invd = m->invd, sigma = m->sigma, n_obs = m->n_obs;
  }
  const vo_sdm_pyramid &py = c->semidense_a->py;
  float *pi[SDM_MAX_LEVELS] = {(float *)invd}, *ps[SDM_MAX_LEVELS] = {(float *)sigma};  // (level 0 is read only)
  uint8_t *pn[SDM_MAX_LEVELS] = {(uint8_t *)n_obs};
  const uint8_t *key[SDM_MAX_LEVELS] = {};
  int stride[SDM_MAX_LEVELS] = {};
  for (int l = 0; l < L; ++l) {
    if (l) pi[l] = py.invd[l], ps[l] = py.sigma[l], pn[l] = py.n_obs[l];
    key[l] = Pk.lv[l].origin();
    stride[l] = Pk.lv[l].stride;
  }
  rc = vo_slot_acquire(c, slot_key) < 0 ? VO_ERR_HIP : VO_OK;
  if (!rc) rc = vo_sdm_enqueue(c, Pc.w, Pc.h, L, pi, ps, pn);
  if (!rc) rc = vo_sda_enqueue_pyr(c, b, key, stride, slot_cur, K, T_ck, prm, pi, ps, pn, SDA_FIRST_CALL);
  VO_CHECK_HIP(c, hipStreamSynchronize(s));  // (the copies read the caller's memory)
  if (rc) return rc;
  return sda_fetch_pyr(c, b, L, res);
}

// ---- StereoVO's hook ------------------------------------------------------------------------------------------------------------------
// At a keyframe, behind the key plane's copy on the side stream: the slot's levels 1 .. levels - 1, device to device, tight.
int vo_svo_semidense_align_key_levels(vo_svo *s, int slot_l, int frame_id) {
  vo_ctx *c = s->c;
  vo_svo_semidense_align &g = s->sda;
  const vo_pyramid &P = c->slots[slot_l];
  const int L = g.pprm.levels < P.n_levels ? g.pprm.levels : P.n_levels;
  for (int l = 1; l < L; ++l)
    VO_CHECK_HIP(c, hipMemcpy2DAsync(g.py.key[l], (size_t)P.lv[l].w, P.lv[l].origin(), (size_t)P.lv[l].stride, (size_t)P.lv[l].w, (size_t)P.lv[l].h,
                                     hipMemcpyDeviceToDevice, c->stream2));
  g.key_levels = L;
  g.key_levels_of = frame_id;
  return VO_OK;
}

// the coarse-to-fine launches of vo_svo_semidense_align_enqueue
static int svo_sda_enqueue_pyr(vo_svo *s, int slot_l, const float T_ck[16]) {
  vo_ctx *c = s->c;
  vo_svo_semidense_temporal &t = s->sdt;
  vo_svo_semidense_align &g = s->sda;
  const int L = g.pprm.levels;
  if (g.key_levels_of != t.frame_id) return 1;  // (the option came on behind this keyframe: its levels were not kept; no result)
  if (g.key_levels < L) VO_FAIL(c, VO_ERR_INVALID, "semi-dense alignment: the keyframe's pyramid held %d levels, the option needs %d", g.key_levels, L);
  float *pi[SDM_MAX_LEVELS] = {t.buf.invd}, *ps[SDM_MAX_LEVELS] = {t.buf.sigma};
  uint8_t *pn[SDM_MAX_LEVELS] = {t.buf.n_obs};
  const uint8_t *key[SDM_MAX_LEVELS] = {t.buf.key};
  int stride[SDM_MAX_LEVELS] = {t.w};
  int w = t.w, h = t.h;
  for (int l = 1; l < L; ++l) {
    w = (w + 1) / 2, h = (h + 1) / 2;
    pi[l] = g.py.invd[l], ps[l] = g.py.sigma[l], pn[l] = g.py.n_obs[l];
    key[l] = g.py.key[l];
    stride[l] = w;
  }
  int rc = vo_sdm_enqueue(c, t.w, t.h, L, pi, ps, pn);
  if (rc) return rc;
  float I[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
  const float *T0 = T_ck;
  int first = SDA_FIRST_CALL;
  if (g.start == VO_SEMIDENSE_ALIGN_START_PREVIOUS) {
    if (t.n_fused == 0)
      T0 = I;  // the first frame after the keyframe
    else if (g.prev_key == t.frame_id)
      first = SDA_FIRST_PREV;  // the previous frame's result where its status is 0 or 1 (the kernel looks), else T_ck
  }
  if (g.affine) return vo_sdaa_enqueue_pyr(c, &g.abuf, key, stride, slot_l, s->prm.frame.Kl, T0, &g.pprm, &g.aprm, pi, ps, pn, first);
  return vo_sda_enqueue_pyr(c, &g.buf, key, stride, slot_l, s->prm.frame.Kl, T0, &g.pprm, pi, ps, pn, first);
}

extern "C" int vo_svo_set_semidense_align_pyr(vo_svo *s, const vo_semidense_align_pyr_params *prm, int start) {
  if (!s) return VO_ERR_INVALID;
  vo_ctx *c = s->c;
  if (s->pending) VO_FAIL(c, VO_ERR_INVALID, "vo_svo_set_semidense_align_pyr: a frame is in flight: call vo_svo_result first");
  if (s->mono) VO_FAIL(c, VO_ERR_INVALID, "vo_svo_set_semidense_align_pyr: a stereo driver only");
  vo_svo_semidense_align &g = s->sda;
  if (!prm) return vo_svo_set_semidense_align(s, nullptr);
  if (!s->sdt.on || !s->sd.on)
    VO_FAIL(c, VO_ERR_INVALID, "vo_svo_set_semidense_align_pyr: needs the temporal option: vo_svo_set_semidense_temporal first");
  if (start != VO_SEMIDENSE_ALIGN_START_ODOMETRY && start != VO_SEMIDENSE_ALIGN_START_PREVIOUS)
    VO_FAIL(c, VO_ERR_INVALID, "vo_svo_set_semidense_align_pyr: start=%d: expected 0 (odometry) or 1 (previous)", start);
  int rc = sda_check_pyr_params(c, prm);
  if (rc) return rc;
  rc = vo_sda_buffers_alloc(c, &g.buf);  // the option's allocations, at the first enable: the state block (unless the level-0 option made it) ...
  if (rc) return rc;
  rc = vo_sdm_pyramid_alloc(c, &g.py, true);  // ... and the key levels with the map pyramid's planes
  if (rc) return rc;
  g.pprm = *prm;
  g.start = start;
  if (!g.on || !g.pyr) g.have = false, g.frame_id = -1, g.prev_key = -1, g.key_levels_of = -1;
  g.on = g.pyr = true;
  return VO_OK;
}

extern "C" int vo_svo_get_semidense_align_pyr(vo_svo *s, vo_semidense_align_pyr_result *res, float T_wc[16], int *frame_id, int *key_frame_id) {
  if (!s || !res) return VO_ERR_INVALID;
  vo_ctx *c = s->c;
  if (s->pending) VO_FAIL(c, VO_ERR_INVALID, "vo_svo_get_semidense_align_pyr: a frame is in flight: call vo_svo_result first");
  if (!s->sda.on || !s->sdt.on || !s->sd.on)
    VO_FAIL(c, VO_ERR_INVALID, "vo_svo_get_semidense_align_pyr: the option is off: vo_svo_set_semidense_align_pyr");
  VO_CHECK_HIP(c, hipSetDevice(c->device));
  const vo_svo_semidense_align &g = s->sda;
  memset(res, 0, sizeof(*res));
  res->status = VO_SEMIDENSE_ALIGN_NONE;
  res->T_ck[0] = res->T_ck[5] = res->T_ck[10] = res->T_ck[15] = 1.0f;
  res->levels = g.pyr ? g.pprm.levels : 1;
  for (int l = 0; l < res->levels; ++l) res->level_status[l] = VO_SEMIDENSE_ALIGN_NONE;
  if (frame_id) *frame_id = g.frame_id;
  if (key_frame_id) *key_frame_id = g.have ? g.key_frame_id : -1;
  if (T_wc)
    for (int i = 0; i < 16; ++i) T_wc[i] = (i % 5 == 0) ? 1.0f : 0.0f;
  if (!g.have) return VO_OK;  // a keyframe frame, or no frame yet
  if (s->sd.have) VO_CHECK_HIP(c, hipEventSynchronize(s->sd.done));  // the side stream's last launch only
  const int rc = g.affine ? sdaa_fetch_plain(c, &g.abuf, g.pyr ? g.pprm.levels : 1, res) : sda_fetch_pyr(c, &g.buf, g.pyr ? g.pprm.levels : 1, res);
  if (rc) return rc;
  if (T_wc) {  // T_wk * inverseSE3(T_ck), on the host in float, in svo_mul44's order
    float T_kc[16];
    svo_inv_se3(res->T_ck, T_kc);
    svo_mul44(g.T_wk, T_kc, T_wc);
  }
  return VO_OK;
}

// ==== with affine brightness (include/vo_hip.h, "Semi-dense alignment with affine brightness") ==========================
extern "C" int vo_semidense_affine_default_params(vo_semidense_affine_params *p) {
  if (!p) return VO_ERR_INVALID;
  memset(p, 0, sizeof(*p));
  p->gain0 = 1.0f;
  return VO_OK;
}

static int sdaa_check_params(vo_ctx *c, const vo_semidense_affine_params *p) {
  if (!(p->gain0 >= 0.125f) || !(p->gain0 <= 8.0f)) VO_FAIL(c, VO_ERR_INVALID, "semi-dense alignment: gain0: expected 1/8 <= gain0 <= 8");
  if (!(fabsf(p->offset0) <= 255.0f)) VO_FAIL(c, VO_ERR_INVALID, "semi-dense alignment: offset0: expected |offset0| <= 255 grey levels");
  return VO_OK;
}

int vo_sdaa_enqueue_pyr(vo_ctx *c, vo_sda_buffers *b, const uint8_t *const key[], const int key_stride[], int slot_cur, const float K[4],
                        const float T_ck[16], const vo_semidense_align_pyr_params *p, const vo_semidense_affine_params *ap,
                        const float *const invd[], const float *const sigma[], const uint8_t *const n_obs[], int first) {
  int rc = sda_check_pyr_params(c, p);
  if (rc) return rc;
  rc = sdaa_check_params(c, ap);
  if (rc) return rc;
  if (slot_cur < 0 || slot_cur >= c->cfg.n_slots || c->slots[slot_cur].n_levels <= 0) VO_FAIL(c, VO_ERR_INVALID, "slot holds no image");
  const vo_pyramid &P = c->slots[slot_cur];
  const int L = p->levels;
  VO_NEED_LEVELS(c, P, L - 1);
  if (P.w > 65535 || P.h > 65535 || (long long)P.w * P.h > 0x7FFFFFFFll)
    VO_FAIL(c, VO_ERR_SIZE, "semi-dense alignment: the image must have 3 .. 65535 pixels a side and fewer than 2^31 in all");
  for (int l = 0; l < L; ++l) {
    int w = P.w, h = P.h;
    sdm_level_size(l, &w, &h);
    if (w != P.lv[l].w || h != P.lv[l].h) VO_FAIL(c, VO_ERR_INVALID, "semi-dense alignment: level %d of the slot is %d x %d, expected %d x %d", l, P.lv[l].w, P.lv[l].h, w, h);
    if (w < 3 || h < 3) VO_FAIL(c, VO_ERR_SIZE, "semi-dense alignment: level %d is %d x %d: every used level needs 3 pixels a side", l, w, h);
    if (key_stride[l] < w) VO_FAIL(c, VO_ERR_INVALID, "semi-dense alignment: level %d: key_stride %d below the width %d", l, key_stride[l], w);
  }
  if (!(K[0] > 0.0f) || !(K[1] > 0.0f) || !isfinite(K[0]) || !isfinite(K[1]) || !isfinite(K[2]) || !isfinite(K[3]))
    VO_FAIL(c, VO_ERR_INVALID, "semi-dense alignment: fx, fy must be positive, K finite");
  for (int i = 0; i < 12; ++i)
    if (!isfinite(T_ck[i])) VO_FAIL(c, VO_ERR_INVALID, "semi-dense alignment: T_ck is not finite");
  if (((size_t)P.w * (size_t)P.h + SDA_BLOCK - 1) / SDA_BLOCK > b->n_blocks)
    VO_FAIL(c, VO_ERR_SIZE, "%d x %d planes exceed vo_config.max_width x max_height", P.w, P.h);
  if (vo_slot_acquire(c, slot_cur) < 0) return VO_ERR_HIP;
  SdaaArgs aa;
  memset(&aa, 0, sizeof(aa));
  SdaArgs &a = aa.a;
  sda_params(&a, p->min_obs, p->huber, p->max_iters, p->eps, p->min_pixels);
  sdaa_params(&aa, ap->gain0, ap->offset0);
  for (int i = 0; i < 12; ++i) a.T0[i] = T_ck[i];
  a.partial = b->partial;
  aa.st = (SdaaState *)b->state;
  vo_prof_begin(c, VO_K_AUX);
  for (int l = L - 1; l >= 0; --l) {
    const float s = 1.0f / (float)(1 << l);  // (a power of two: the products are exact)
    a.Lk = key[l];
    a.Lc = P.lv[l].origin();
    a.strideK = key_stride[l];
    a.strideC = P.lv[l].stride;
    a.W = P.lv[l].w;
    a.H = P.lv[l].h;
    a.invd = invd[l], a.sigma = sigma[l], a.n_obs = n_obs[l];
    a.fx = K[0] * s, a.fy = K[1] * s, a.cx = K[2] * s, a.cy = K[3] * s;
    a.n_blocks = (int)(((size_t)a.W * (size_t)a.H + SDA_BLOCK - 1) / SDA_BLOCK);
    a.level = l;
    a.max_iters = sda_level_iters(p, l);
    for (int it = 0; it < a.max_iters; ++it) {
      a.first = it > 0 ? 0 : (l == L - 1 ? first : SDA_FIRST_LEVEL);
      hipLaunchKernelGGL(semidense_affine_kernel, dim3((unsigned)a.n_blocks), dim3(SDA_NT), 0, c->stream, aa);
    }
  }
  vo_prof_end(c);
  VO_CHECK_HIP(c, hipGetLastError());
  return VO_OK;
}

static inline vo_semidense_align_pyr_params sdaa_one_level(const vo_semidense_align_params *p) {
  vo_semidense_align_pyr_params q;
  memset(&q, 0, sizeof(q));
  q.min_obs = p->min_obs, q.huber = p->huber, q.max_iters = p->max_iters, q.eps = p->eps, q.min_pixels = p->min_pixels;
  q.levels = 1;
  return q;
}

static int sdaa_fetch(vo_ctx *c, const vo_sda_buffers *b, int levels, vo_semidense_align_affine_result *res) {
  SdaaState st;
  VO_CHECK_HIP(c, hipMemcpy(&st, b->state, sizeof(st), hipMemcpyDeviceToHost));
  memset(res, 0, sizeof(*res));
  memcpy(res->T_ck, st.T, sizeof(st.T));
  res->status = st.status;
  res->iters = st.iters;
  res->count = st.count;
  res->rms = st.sw > 0.0 ? sqrt(st.swrr / st.sw) / 16.0 : 0.0;
  memcpy(res->H, st.H, sizeof(st.H));
  memcpy(res->b, st.b, sizeof(st.b));
  res->G = st.G, res->O = st.O;
  res->gain = (double)st.G / 65536.0, res->offset = (double)st.O / 16.0;
  res->levels = levels;
  res->start_prev = st.start_prev;
  for (int l = 0; l < levels; ++l) {
    res->level_status[l] = st.lv[l].status;
    res->level_iters[l] = st.lv[l].iters;
    res->level_count[l] = st.lv[l].count;
    res->level_rms[l] = st.lv[l].sw > 0.0 ? sqrt(st.lv[l].swrr / st.lv[l].sw) / 16.0 : 0.0;
    res->level_G[l] = st.lv[l].G, res->level_O[l] = st.lv[l].O;
  }
  return VO_OK;
}

// the affine run's result as the getters without gain and offset report it: H, b cut to the pose's rows and columns of the 8 x 8
static int sdaa_fetch_plain(vo_ctx *c, const vo_sda_buffers *b, int levels, vo_semidense_align_pyr_result *res) {
  vo_semidense_align_affine_result r;
  const int rc = sdaa_fetch(c, b, levels, &r);
  if (rc) return rc;
  memset(res, 0, sizeof(*res));
  memcpy(res->T_ck, r.T_ck, sizeof(r.T_ck));
  res->status = r.status, res->iters = r.iters, res->count = r.count, res->rms = r.rms;
  for (int i = 0, n = 0, m = 0; i < 8; ++i)
    for (int j = i; j < 8; ++j, ++m)
      if (j < 6) res->H[n++] = r.H[m];
  memcpy(res->b, r.b, sizeof(res->b));
  res->levels = levels, res->start_prev = r.start_prev;
  for (int l = 0; l < levels; ++l) {
    res->level_status[l] = r.level_status[l], res->level_iters[l] = r.level_iters[l], res->level_count[l] = r.level_count[l];
    res->level_rms[l] = r.level_rms[l];
  }
  return VO_OK;
}

extern "C" int vo_semidense_align_affine(vo_ctx *c, const uint8_t *key_plane, int key_stride, int key_on_device, int slot_cur, const float K[4],
                                         const float T_ck[16], const vo_semidense_align_params *prm, const vo_semidense_affine_params *ap,
                                         const float *invd, const float *sigma, const uint8_t *n_obs, int on_device,
                                         vo_semidense_align_affine_result *res) {
  if (!c || !key_plane || !K || !T_ck || !prm || !ap || !invd || !sigma || !n_obs || !res) return VO_ERR_INVALID;
  VO_CHECK_HIP(c, hipSetDevice(c->device));
  hipStream_t s = c->stream;
  if (slot_cur < 0 || slot_cur >= c->cfg.n_slots || c->slots[slot_cur].n_levels <= 0) VO_FAIL(c, VO_ERR_INVALID, "slot holds no image");
  const int W = c->slots[slot_cur].w, H = c->slots[slot_cur].h;
  if (key_stride < W) VO_FAIL(c, VO_ERR_INVALID, "semi-dense alignment: key_stride %d below the width %d", key_stride, W);
  if (W < 3 || H < 3) VO_FAIL(c, VO_ERR_SIZE, "semi-dense alignment: the image must have 3 .. 65535 pixels a side and fewer than 2^31 in all");
  int rc = sda_check_params(c, prm);  // (before any copy reads the caller's memory)
  if (!rc) rc = sdaa_check_params(c, ap);
  if (rc) return rc;
  const size_t np = (size_t)W * (size_t)H;
  if (!c->semidense_a) c->semidense_a = new vo_semidense_align_state();
  vo_sda_buffers *b = &c->semidense_a->abuf;
  rc = vo_sdaa_buffers_alloc(c, b);
  if (rc) return rc;
  vo_sdt_buffers *m = nullptr;  // the device copies of host planes
  if (!key_on_device || !on_device) {
    rc = vo_sdt_ctx_buffers(c, &m);
    if (rc) return rc;
  }
  const uint8_t *d_key = key_plane;
  int d_stride = key_stride;
  if (!key_on_device) {
    VO_CHECK_HIP(c, hipMemcpy2DAsync(m->key, (size_t)W, key_plane, (size_t)key_stride, (size_t)W, (size_t)H, hipMemcpyHostToDevice, s));
    d_key = m->key;
    d_stride = W;
  }
  if (!on_device) {
    VO_CHECK_HIP(c, hipMemcpyAsync(m->invd, invd, np * sizeof(float), hipMemcpyHostToDevice, s));
    VO_CHECK_HIP(c, hipMemcpyAsync(m->sigma, sigma, np * sizeof(float), hipMemcpyHostToDevice, s));
    VO_CHECK_HIP(c, hipMemcpyAsync(m->n_obs, n_obs, np, hipMemcpyHostToDevice, s));
    invd = m->invd, sigma = m->sigma, n_obs = m->n_obs;
  }
  const vo_semidense_align_pyr_params one = sdaa_one_level(prm);
  rc = vo_sdaa_enqueue_pyr(c, b, &d_key, &d_stride, slot_cur, K, T_ck, &one, ap, &invd, &sigma, &n_obs, SDA_FIRST_CALL);
  VO_CHECK_HIP(c, hipStreamSynchronize(s));  // (the copies read the caller's memory)
  if (rc) return rc;
  return sdaa_fetch(c, b, 1, res);
}

extern "C" int vo_semidense_align_pyr_affine(vo_ctx *c, int slot_key, int slot_cur, const float K[4], const float T_ck[16],
                                             const vo_semidense_align_pyr_params *prm, const vo_semidense_affine_params *ap, const float *invd,
                                             const float *sigma, const uint8_t *n_obs, int on_device, vo_semidense_align_affine_result *res) {
  if (!c || !K || !T_ck || !prm || !ap || !invd || !sigma || !n_obs || !res) return VO_ERR_INVALID;
  VO_CHECK_HIP(c, hipSetDevice(c->device));
  hipStream_t s = c->stream;
  for (int slot : {slot_key, slot_cur})
    if (slot < 0 || slot >= c->cfg.n_slots || c->slots[slot].n_levels <= 0) VO_FAIL(c, VO_ERR_INVALID, "slot %d holds no image", slot);
  const vo_pyramid &Pk = c->slots[slot_key], &Pc = c->slots[slot_cur];
  if (Pk.w != Pc.w || Pk.h != Pc.h) VO_FAIL(c, VO_ERR_SIZE, "semi-dense alignment: the slots' images differ in size");
  int rc = sda_check_pyr_params(c, prm);  // (before any copy reads the caller's memory)
  if (!rc) rc = sdaa_check_params(c, ap);
  if (rc) return rc;
  const int L = prm->levels;
  VO_NEED_LEVELS(c, Pk, L - 1);
  VO_NEED_LEVELS(c, Pc, L - 1);
  const size_t np = (size_t)Pc.w * (size_t)Pc.h;
  rc = sda_ctx_state(c, L > 1);
  if (rc) return rc;
  vo_sda_buffers *b = &c->semidense_a->abuf;
  rc = vo_sdaa_buffers_alloc(c, b);
  if (rc) return rc;
  if (!on_device) {
    vo_sdt_buffers *m = nullptr;  // the device copies of host planes
    rc = vo_sdt_ctx_buffers(c, &m);
    if (rc) return rc;
    VO_CHECK_HIP(c, hipMemcpyAsync(m->invd, invd, np * sizeof(float), hipMemcpyHostToDevice, s));
    VO_CHECK_HIP(c, hipMemcpyAsync(m->sigma, sigma, np * sizeof(float), hipMemcpyHostToDevice, s));
    VO_CHECK_HIP(c, hipMemcpyAsync(m->n_obs, n_obs, np, hipMemcpyHostToDevice, s));
    invd = m->invd, sigma = m->sigma, n_obs = m->n_obs;
  }
  const vo_sdm_pyramid &py = c->semidense_a->py;
  float *pi[SDM_MAX_LEVELS] = {(float *)invd}, *ps[SDM_MAX_LEVELS] = {(float *)sigma};  // (level 0 is read only)
  uint8_t *pn[SDM_MAX_LEVELS] = {(uint8_t *)n_obs};
  const uint8_t *key[SDM_MAX_LEVELS] = {};
  int stride[SDM_MAX_LEVELS] = {};
  for (int l = 0; l < L; ++l) {
    if (l) pi[l] = py.invd[l], ps[l] = py.sigma[l], pn[l] = py.n_obs[l];
    key[l] = Pk.lv[l].origin();
    stride[l] = Pk.lv[l].stride;
  }
  rc = vo_slot_acquire(c, slot_key) < 0 ? VO_ERR_HIP : VO_OK;
  if (!rc) rc = vo_sdm_enqueue(c, Pc.w, Pc.h, L, pi, ps, pn);
  if (!rc) rc = vo_sdaa_enqueue_pyr(c, b, key, stride, slot_cur, K, T_ck, prm, ap, pi, ps, pn, SDA_FIRST_CALL);
  VO_CHECK_HIP(c, hipStreamSynchronize(s));  // (the copies read the caller's memory)
  if (rc) return rc;
  return sdaa_fetch(c, b, L, res);
}

// ---- StereoVO's hook ------------------------------------------------------------------------------------------------------------------
// the level-0 option's launches of vo_svo_semidense_align_enqueue with the modifier on
static int svo_sdaa_enqueue_level0(vo_svo *s, int slot_l, const float T_ck[16]) {
  vo_svo_semidense_temporal &t = s->sdt;
  vo_svo_semidense_align &g = s->sda;
  const vo_semidense_align_pyr_params one = sdaa_one_level(&g.prm);
  const uint8_t *key = t.buf.key, *pn = t.buf.n_obs;
  const float *pi = t.buf.invd, *ps = t.buf.sigma;
  const int stride = t.w;
  return vo_sdaa_enqueue_pyr(s->c, &g.abuf, &key, &stride, slot_l, s->prm.frame.Kl, T_ck, &one, &g.aprm, &pi, &ps, &pn, SDA_FIRST_CALL);
}

extern "C" int vo_svo_set_semidense_align_affine(vo_svo *s, const vo_semidense_affine_params *ap) {
  if (!s) return VO_ERR_INVALID;
  vo_ctx *c = s->c;
  if (s->pending) VO_FAIL(c, VO_ERR_INVALID, "vo_svo_set_semidense_align_affine: a frame is in flight: call vo_svo_result first");
  if (s->mono) VO_FAIL(c, VO_ERR_INVALID, "vo_svo_set_semidense_align_affine: a stereo driver only");
  vo_svo_semidense_align &g = s->sda;
  if (!ap) {
    if (g.affine) g.have = false;  // (the state block changes: the next frame has no previous result)
    g.affine = false;
    return VO_OK;
  }
  if (!g.on || !s->sdt.on || !s->sd.on)
    VO_FAIL(c, VO_ERR_INVALID, "vo_svo_set_semidense_align_affine: needs an alignment option: vo_svo_set_semidense_align or vo_svo_set_semidense_align_pyr first");
  int rc = sdaa_check_params(c, ap);
  if (rc) return rc;
  rc = vo_sdaa_buffers_alloc(c, &g.abuf);  // the modifier's only allocation, at the first enable
  if (rc) return rc;
  g.aprm = *ap;
  if (!g.affine) g.have = false;
  g.affine = true;
  return VO_OK;
}

extern "C" int vo_svo_get_semidense_align_affine(vo_svo *s, vo_semidense_align_affine_result *res, float T_wc[16], int *frame_id, int *key_frame_id) {
  if (!s || !res) return VO_ERR_INVALID;
  vo_ctx *c = s->c;
  if (s->pending) VO_FAIL(c, VO_ERR_INVALID, "vo_svo_get_semidense_align_affine: a frame is in flight: call vo_svo_result first");
  if (!s->sda.on || !s->sda.affine || !s->sdt.on || !s->sd.on)
    VO_FAIL(c, VO_ERR_INVALID, "vo_svo_get_semidense_align_affine: the modifier is off: vo_svo_set_semidense_align_affine");
  VO_CHECK_HIP(c, hipSetDevice(c->device));
  const vo_svo_semidense_align &g = s->sda;
  memset(res, 0, sizeof(*res));
  res->status = VO_SEMIDENSE_ALIGN_NONE;
  res->T_ck[0] = res->T_ck[5] = res->T_ck[10] = res->T_ck[15] = 1.0f;
  res->levels = g.pyr ? g.pprm.levels : 1;
  for (int l = 0; l < res->levels; ++l) res->level_status[l] = VO_SEMIDENSE_ALIGN_NONE;
  res->G = (int)floorf(65536.0f * g.aprm.gain0 + 0.5f), res->O = (int)floorf(16.0f * g.aprm.offset0 + 0.5f);
  res->gain = (double)res->G / 65536.0, res->offset = (double)res->O / 16.0;
  if (frame_id) *frame_id = g.frame_id;
  if (key_frame_id) *key_frame_id = g.have ? g.key_frame_id : -1;
  if (T_wc)
    for (int i = 0; i < 16; ++i) T_wc[i] = (i % 5 == 0) ? 1.0f : 0.0f;
  if (!g.have) return VO_OK;  // a keyframe frame, or no frame yet
  if (s->sd.have) VO_CHECK_HIP(c, hipEventSynchronize(s->sd.done));  // the side stream's last launch only
  const int rc = sdaa_fetch(c, &g.abuf, g.pyr ? g.pprm.levels : 1, res);
  if (rc) return rc;
  if (T_wc) {  // T_wk * inverseSE3(T_ck), on the host in float, in svo_mul44's order
    float T_kc[16];
    svo_inv_se3(res->T_ck, T_kc);
    svo_mul44(g.T_wk, T_kc, T_wc);
  }
  return VO_OK;
}
