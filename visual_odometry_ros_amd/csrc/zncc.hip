// zncc.hip — image_processing::calcZNCC on the device (include/vo_hip.h, "ZNCC"): the operator (vo_zncc), the
// drivers' gate state, and the launch the frame operators put in front of the BA launch (zncc_device.hpp has the kernel).
#include "vo_internal.hpp"
#include "vo_kernels.hpp"

#include <math.h>

#define ZNCC_SHFL_DOWN(v, d) __shfl_down((v), (d), 64)
// (every lane of the wavefront is active wherever this is reached: the first active lane is lane 0)
#define ZNCC_BCAST0(v) __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, (v))))
#include "zncc_device.hpp"

static int zncc_check_window(vo_ctx *c, int win, int pattern) {
  if (win < ZNCC_MIN_WIN || win > ZNCC_MAX_WIN || !(win & 1))
    VO_FAIL(c, VO_ERR_INVALID, "ZNCC window %d: expected an odd size in %d..%d", win, ZNCC_MIN_WIN, ZNCC_MAX_WIN);
  if (pattern != VO_ZNCC_PATTERN_REFERENCE && pattern != VO_ZNCC_PATTERN_CENTERED)
    VO_FAIL(c, VO_ERR_INVALID, "ZNCC pattern %d: expected VO_ZNCC_PATTERN_REFERENCE (0) or VO_ZNCC_PATTERN_CENTERED (1)", pattern);
  return VO_OK;
}

static int zncc_pair(vo_ctx *c, int slot0, int slot1, ZnccPair *p, int *W, int *H) {
  if (slot0 < 0 || slot0 >= c->cfg.n_slots || slot1 < 0 || slot1 >= c->cfg.n_slots || c->slots[slot0].n_levels <= 0 ||
      c->slots[slot1].n_levels <= 0)
    VO_FAIL(c, VO_ERR_INVALID, "slot holds no image");
  const vo_pyramid &P0 = c->slots[slot0], &P1 = c->slots[slot1];
  if (P0.w != P1.w || P0.h != P1.h) VO_FAIL(c, VO_ERR_SIZE, "image size mismatch");
  if (*W && (*W != P0.w || *H != P0.h)) VO_FAIL(c, VO_ERR_SIZE, "image size mismatch");
  if (P0.w < 2 || P0.h < 2) VO_FAIL(c, VO_ERR_SIZE, "ZNCC needs an image of at least 2 x 2 pixels");
  if (vo_slot_acquire(c, slot0) < 0 || vo_slot_acquire(c, slot1) < 0) return VO_ERR_HIP;
  p->I0 = P0.lv[0].origin();
  p->stride0 = P0.lv[0].stride;
  p->I1 = P1.lv[0].origin();
  p->stride1 = P1.lv[0].stride;
  *W = P0.w;
  *H = P0.h;
  return VO_OK;
}

// n_pairs launches' worth in ONE launch: grid (ceil(n / ZNCC_WAVES), n_pairs), on c->stream
static int zncc_launch(vo_ctx *c, ZnccArgs &a, int n_pairs, int win, int pattern) {
  if (a.n <= 0) return VO_OK;
  zncc_plan(&a, win, pattern);
  const dim3 grid((unsigned)((a.n + ZNCC_WAVES - 1) / ZNCC_WAVES), (unsigned)n_pairs);
  const zncc_kernel_fn k = zncc_kernel_for(c->sum_order == VO_SUM_ORDER_REFERENCE, a.J);
  if (!k) VO_FAIL(c, VO_ERR_INVALID, "ZNCC: no kernel for a %d x %d window", win, win);  // (a missing kernel is an error)
  vo_prof_begin(c, VO_K_AUX);
  hipLaunchKernelGGL(k, grid, dim3(ZNCC_NT), 0, c->stream, a);
  vo_prof_end(c);
  VO_CHECK_HIP(c, hipGetLastError());
  return VO_OK;
}

extern "C" int vo_zncc(vo_ctx *c, int slot0, int slot1, const float *pts0, const float *pts1, int n, int win, int pattern, float *out) {
  if (!c || n < 0 || (n > 0 && (!pts0 || !pts1 || !out))) return VO_ERR_INVALID;
  int rc = zncc_check_window(c, win, pattern);
  if (rc) return rc;
  if (n > c->cfg.max_points) VO_FAIL(c, VO_ERR_CAPACITY, "n=%d exceeds vo_config.max_points=%d", n, c->cfg.max_points);
  VO_CHECK_HIP(c, hipSetDevice(c->device));
  ZnccArgs a;
  memset(&a, 0, sizeof(a));
  rc = zncc_pair(c, slot0, slot1, &a.pair[0], &a.W, &a.H);
  if (rc) return rc;
  if (n == 0) return VO_OK;
  hipStream_t s = c->stream;
  VO_CHECK_HIP(c, hipMemcpyAsync(c->d_pts0, pts0, sizeof(float) * 2 * (size_t)n, hipMemcpyHostToDevice, s));
  VO_CHECK_HIP(c, hipMemcpyAsync(c->d_pts1, pts1, sizeof(float) * 2 * (size_t)n, hipMemcpyHostToDevice, s));
  a.pair[0].pts0 = c->d_pts0;
  a.pair[0].pts1 = c->d_pts1;
  a.pair[0].out = c->d_err;
  a.n = n;
  rc = zncc_launch(c, a, 1, win, pattern);
  if (rc) return rc;
  VO_CHECK_HIP(c, hipMemcpyAsync(out, c->d_err, sizeof(float) * (size_t)n, hipMemcpyDeviceToHost, s));
  VO_CHECK_HIP(c, hipStreamSynchronize(s));
  return VO_OK;
}

// ---- the drivers' gate -------------------------------------------------------------------------------------------------------
int vo_zncc_gate_set(vo_ctx *c, vo_zncc_gate *g, int pairs, int win, int pattern, float thres, bool stereo, int cap) {
  if (pairs & ~(VO_ZNCC_TEMPORAL | VO_ZNCC_STEREO)) VO_FAIL(c, VO_ERR_INVALID, "ZNCC gate: unknown pair bits 0x%x", pairs);
  if ((pairs & VO_ZNCC_STEREO) && !stereo) VO_FAIL(c, VO_ERR_INVALID, "ZNCC gate: VO_ZNCC_STEREO needs a stereo driver");
  if (pairs == 0) {
    g->pairs = 0;
    return VO_OK;
  }
  const int rc = zncc_check_window(c, win, pattern);
  if (rc) return rc;
  if (isnan(thres)) VO_FAIL(c, VO_ERR_INVALID, "ZNCC gate: the threshold is NaN");
  if (!g->d) {  // the option's only allocation
    VO_CHECK_HIP(c, hipSetDevice(c->device));
    VO_CHECK_HIP(c, vo_dev_malloc(c, (void **)&g->d, sizeof(float) * 2 * (size_t)cap));
    g->cap = cap;
  }
  g->pairs = pairs;
  g->win = win;
  g->pattern = pattern;
  g->thres = thres;
  return VO_OK;
}

void vo_zncc_gate_free(vo_zncc_gate *g) {
  if (g->d) (void)hipFree(g->d);
  *g = vo_zncc_gate();
}

int vo_zncc_gate_get(vo_ctx *c, const vo_zncc_gate *g, float *zncc_t, float *zncc_s, int cap, int *n) {
  if (!n || cap < 0) return VO_ERR_INVALID;
  if (!g->pairs || !g->d) VO_FAIL(c, VO_ERR_INVALID, "the ZNCC gate is off: vo_svo_set_zncc_gate / vo_mvo_set_zncc_gate");
  *n = g->last_n;
  const int m = g->last_n < cap ? g->last_n : cap;
  if (m <= 0) return VO_OK;
  VO_CHECK_HIP(c, hipSetDevice(c->device));
  // (behind the frame's result: the launch that wrote the values has finished)
  if (zncc_t && (g->last_pairs & VO_ZNCC_TEMPORAL)) VO_CHECK_HIP(c, hipMemcpy(zncc_t, g->d, sizeof(float) * (size_t)m, hipMemcpyDeviceToHost));
  if (zncc_s && (g->last_pairs & VO_ZNCC_STEREO))
    VO_CHECK_HIP(c, hipMemcpy(zncc_s, g->d + g->cap, sizeof(float) * (size_t)m, hipMemcpyDeviceToHost));
  return VO_OK;
}

int vo_zncc_gate_enqueue(vo_ctx *c, vo_zncc_gate *g, int slot_l0, int slot_l1, int slot_r1, const float *d_pts_l0, const float *d_pts_l1,
                         const float *d_pts_r1, int n, vo_zncc_view *view) {
  view->t = view->s = nullptr;
  view->thres = 0.0f;
  view->on = 0;
  if (!g || !g->pairs || n <= 0) return VO_OK;
  if (n > g->cap) VO_FAIL(c, VO_ERR_CAPACITY, "ZNCC gate: %d features exceed the %d the gate's storage holds", n, g->cap);
  int pairs = g->pairs;
  if (slot_r1 < 0 || !d_pts_r1) pairs &= ~VO_ZNCC_STEREO;
  ZnccArgs a;
  memset(&a, 0, sizeof(a));
  int k = 0;
  if (pairs & VO_ZNCC_TEMPORAL) {
    const int rc = zncc_pair(c, slot_l0, slot_l1, &a.pair[k], &a.W, &a.H);
    if (rc) return rc;
    a.pair[k].pts0 = d_pts_l0;
    a.pair[k].pts1 = d_pts_l1;
    a.pair[k].out = g->d;
    view->t = g->d;
    ++k;
  }
  if (pairs & VO_ZNCC_STEREO) {
    const int rc = zncc_pair(c, slot_l1, slot_r1, &a.pair[k], &a.W, &a.H);
    if (rc) return rc;
    a.pair[k].pts0 = d_pts_l1;
    a.pair[k].pts1 = d_pts_r1;
    a.pair[k].out = g->d + g->cap;
    view->s = g->d + g->cap;
    ++k;
  }
  if (k == 0) return VO_OK;
  a.n = n;
  const int rc = zncc_launch(c, a, k, g->win, g->pattern);
  if (rc) return rc;
  view->thres = g->thres;
  view->on = 1;
  g->last_n = n;
  g->last_pairs = pairs;
  return VO_OK;
}
