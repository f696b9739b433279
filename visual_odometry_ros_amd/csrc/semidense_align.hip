// semidense_align.hip — direct image alignment on the semi-dense map (include/vo_hip.h, "Semi-dense alignment"): the
// operator (vo_semidense_align) and StereoVO's hook (vo_svo_set_semidense_align, vo_svo_get_semidense_align; the launches are
// placed by vo_svo_semidense_temporal_enqueue in front of the frame's temporal launch). semidense_align_device.hpp has the kernel.
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
int vo_sda_buffers_alloc(vo_ctx *c, vo_sda_buffers *b) {
  if (b->base) return VO_OK;
  const size_t n = (size_t)c->cfg.max_width * (size_t)c->cfg.max_height, nb = (n + SDA_BLOCK - 1) / SDA_BLOCK;
  const size_t head = (sizeof(SdaState) + 255) & ~(size_t)255;
  VO_CHECK_HIP(c, hipSetDevice(c->device));
  VO_CHECK_HIP(c, vo_dev_malloc(c, &b->base, head + nb * SDA_NSUM * sizeof(long long)));
  b->state = b->base;
  b->partial = (long long *)((uint8_t *)b->base + head);
  b->n_blocks = nb;
  VO_CHECK_HIP(c, hipMemsetAsync(b->base, 0, head, c->stream));
  VO_CHECK_HIP(c, hipStreamSynchronize(c->stream));  // (the launches may run on another stream)
  return VO_OK;
}
void vo_sda_buffers_free(vo_sda_buffers *b) {
  if (b->base) (void)hipFree(b->base);
  *b = vo_sda_buffers();
}

struct vo_semidense_align_state {
  vo_sda_buffers buf;
};
void vo_semidense_align_free(vo_ctx *c) {
  if (!c->semidense_a) return;
  vo_sda_buffers_free(&c->semidense_a->buf);
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
int vo_svo_semidense_align_enqueue(vo_svo *s, int slot_l, int frame_id, const float T_ck[16]) {
  vo_ctx *c = s->c;
  vo_svo_semidense_temporal &t = s->sdt;
  vo_svo_semidense_align &g = s->sda;
  g.have = false;  // (should the launch be refused, this frame has no result)
  const int rc = vo_sda_enqueue(c, &g.buf, t.buf.key, t.w, slot_l, s->prm.frame.Kl, T_ck, &g.prm, t.buf.invd, t.buf.sigma, t.buf.n_obs);
  if (rc) return rc;
  g.have = true;
  g.frame_id = frame_id;
  g.key_frame_id = t.frame_id;
  memcpy(g.T_wk, t.T_wk, sizeof(g.T_wk));
  return VO_OK;
}

void vo_svo_semidense_align_free(vo_svo *s) {
  vo_sda_buffers_free(&s->sda.buf);
  s->sda = vo_svo_semidense_align();
}

extern "C" int vo_svo_set_semidense_align(vo_svo *s, const vo_semidense_align_params *prm) {
  if (!s) return VO_ERR_INVALID;
  vo_ctx *c = s->c;
  if (s->pending) VO_FAIL(c, VO_ERR_INVALID, "vo_svo_set_semidense_align: a frame is in flight: call vo_svo_result first");
  if (s->mono) VO_FAIL(c, VO_ERR_INVALID, "vo_svo_set_semidense_align: a stereo driver only");
  vo_svo_semidense_align &g = s->sda;
  if (!prm) {
    g.on = false;
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
  if (!g.on) g.have = false, g.frame_id = -1;
  g.on = true;
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
  const int rc = sda_fetch(c, &g.buf, res);
  if (rc) return rc;
  if (T_wc) {  // T_wk * inverseSE3(T_ck), on the host in float, in svo_mul44's order
    float T_kc[16];
    svo_inv_se3(res->T_ck, T_kc);
    svo_mul44(g.T_wk, T_kc, T_wc);
  }
  return VO_OK;
}
