// orb_describe.hip — FeatureExtractor::extractAndComputeORB (core/visual_odometry/feature_extractor.cpp:321-332) on the
// device: orientation and 256-bit steered-BRIEF descriptors of ORB keypoints (cv::ORB::compute restated, semantics in
// include/vo_hip.h), two descriptor sets resident on the device and the matcher on them. The kernel is orb_describe.hpp;
// the pyramid and the detection are orb_detect.hip's (vo_orb_levels_enqueue).
#include "vo_internal.hpp"
#include "vo_kernels.hpp"

// what orb_describe.hpp asks its includer for (tests/emu/emu_describe.cpp provides CPU stand-ins of the same names)
__device__ __forceinline__ int orb_wave_sum(int v) { return wave_sum_i32(v); }
__device__ __forceinline__ int orb_wave_get(int v, int lane) { return __shfl(v, lane); }
#include "orb_describe.hpp"

struct vo_orb_desc_set {
  uint8_t *desc = nullptr;  // 32 bytes per keypoint
  float *angle = nullptr;
  uint8_t *valid = nullptr;
  int cap = 0, n = 0;
};
struct vo_orb_desc_state {
  int8_t pattern[1024];
  bool pattern_on_device = false;
  int8_t *d_pattern = nullptr;
  OrbDescLevel *d_levels = nullptr;
  OrbDescLevel h_levels[12];  // what the last launch's table was copied from (stays valid until that call has synchronised)
  vo_orb_desc_set set[2];
  vo_orb_desc_set own;  // vo_orb_compute: the caller's keypoints
  float *d_xy = nullptr;
  int32_t *d_oct = nullptr;
  int32_t *d_best = nullptr;  // vo_orb_match_sets
  uint16_t *d_bd = nullptr, *d_sd = nullptr;
  int match_cap = 0;
};

static uint64_t orbd_mix(uint64_t z) {
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
extern "C" int vo_orb_default_pattern(int8_t pattern[1024]) {
  if (!pattern) return VO_ERR_INVALID;
  for (uint64_t k = 0; k < 1024; ++k) {
    const uint64_t z = orbd_mix(0x4F52423331ull + (k + 1) * 0x9E3779B97F4A7C15ull);
    pattern[k] = (int8_t)((int)(((z >> 32) * 31) >> 32) - 15);
  }
  return VO_OK;
}

static void free_set(vo_orb_desc_set &s) {
  if (s.desc) (void)hipFree(s.desc);
  if (s.angle) (void)hipFree(s.angle);
  if (s.valid) (void)hipFree(s.valid);
  s = vo_orb_desc_set();
}
void vo_orb_describe_free(vo_ctx *c) {
  vo_orb_desc_state *D = c->orb_desc;
  if (!D) return;
  free_set(D->set[0]);
  free_set(D->set[1]);
  free_set(D->own);
  void *bufs[] = {D->d_pattern, D->d_levels, D->d_xy, D->d_oct, D->d_best, D->d_bd, D->d_sd};
  for (void *b : bufs)
    if (b) (void)hipFree(b);
  delete D;
  c->orb_desc = nullptr;
}

static int desc_state(vo_ctx *c) {
  if (c->orb_desc) return VO_OK;
  vo_orb_desc_state *D = new vo_orb_desc_state();
  vo_orb_default_pattern(D->pattern);
  c->orb_desc = D;
  VO_CHECK_HIP(c, vo_dev_malloc(c, (void **)&D->d_pattern, 1024));
  VO_CHECK_HIP(c, vo_dev_malloc(c, (void **)&D->d_levels, sizeof(OrbDescLevel) * 12));
  return VO_OK;
}
static int ensure_set(vo_ctx *c, vo_orb_desc_set &s, int cap) {
  if (cap <= s.cap) return VO_OK;
  free_set(s);
  VO_CHECK_HIP(c, vo_dev_malloc(c, (void **)&s.desc, (size_t)cap * 32));
  VO_CHECK_HIP(c, vo_dev_malloc(c, (void **)&s.angle, sizeof(float) * (size_t)cap));
  VO_CHECK_HIP(c, vo_dev_malloc(c, (void **)&s.valid, (size_t)cap));
  s.cap = cap;
  return VO_OK;
}

extern "C" int vo_orb_get_pattern(vo_ctx *c, int8_t pattern[1024]) {
  if (!c || !pattern) return VO_ERR_INVALID;
  if (c->orb_desc)
    memcpy(pattern, c->orb_desc->pattern, 1024);
  else
    vo_orb_default_pattern(pattern);
  return VO_OK;
}
extern "C" int vo_orb_set_pattern(vo_ctx *c, const int8_t pattern[1024]) {
  if (!c || !pattern) return VO_ERR_INVALID;
  for (int k = 0; k < 1024; ++k)
    if (pattern[k] < -15 || pattern[k] > 15) VO_FAIL(c, VO_ERR_INVALID, "pattern coordinate %d is %d: outside [-15, 15]", k, (int)pattern[k]);
  VO_CHECK_HIP(c, hipSetDevice(c->device));
  int rc = desc_state(c);
  if (rc) return rc;
  memcpy(c->orb_desc->pattern, pattern, 1024);
  c->orb_desc->pattern_on_device = false;
  return VO_OK;
}

// descriptors of n keypoints (n_dev: counted on the device, at most n) on the levels of `v`, into `out`, on c->stream
static int describe_enqueue(vo_ctx *c, const vo_orb_view &v, const float *d_xy, const int32_t *d_oct, int n, const int *n_dev, int steer,
                            vo_orb_desc_set &out) {
  vo_orb_desc_state *D = c->orb_desc;
  hipStream_t s = c->stream;
  if (!D->pattern_on_device) {
    // (a synchronous copy: the table may be replaced by the host right after this call)
    VO_CHECK_HIP(c, hipStreamSynchronize(s));
    VO_CHECK_HIP(c, hipMemcpy(D->d_pattern, D->pattern, 1024, hipMemcpyHostToDevice));
    D->pattern_on_device = true;
  }
  OrbDescLevel *L = D->h_levels;
  memset(L, 0, sizeof(D->h_levels));
  for (int l = 0; l < v.n_levels; ++l) {
    L[l].img = v.img[l];
    L[l].w = v.w[l];
    L[l].h = v.h[l];
    L[l].stride = v.stride[l];
    L[l].inv_scale = 1.0f / v.scale[l];
  }
  VO_CHECK_HIP(c, hipMemcpyAsync(D->d_levels, L, sizeof(D->h_levels), hipMemcpyHostToDevice, s));
  OrbDescArgs a;
  memset(&a, 0, sizeof(a));
  a.levels = D->d_levels;
  a.n_levels = v.n_levels;
  a.edge = v.edge;
  a.steer = steer ? 1 : 0;
  a.n = n;
  a.n_dev = n_dev;
  a.n_cap = n;
  a.kp_xy = d_xy;
  a.kp_oct = d_oct;
  a.pattern = D->d_pattern;
  a.angle = out.angle;
  a.desc = (uint32_t *)out.desc;
  a.valid = out.valid;
  vo_prof_begin(c, VO_K_AUX);
  hipLaunchKernelGGL(orb_describe_kernel, dim3((n + ORBD_KP - 1) / ORBD_KP), dim3(64 * ORBD_KP), 0, s, a);
  vo_prof_end(c);
  VO_CHECK_HIP(c, hipGetLastError());
  return VO_OK;
}

extern "C" int vo_orb_compute(vo_ctx *c, int slot, const vo_orb_params *p, const float *kp_xy, const int32_t *kp_octave, int n, int steer,
                              float *angle_out, uint8_t *desc_out, uint8_t *valid_out) {
  if (!c || !p || n < 0 || (n > 0 && (!kp_xy || !kp_octave))) return VO_ERR_INVALID;
  VO_CHECK_HIP(c, hipSetDevice(c->device));
  int rc = desc_state(c);
  if (rc) return rc;
  vo_orb_view v;
  rc = vo_orb_levels_enqueue(c, slot, p, false, &v);
  if (rc) return rc;
  if (n == 0) return VO_OK;
  vo_orb_desc_state *D = c->orb_desc;
  if (n > D->own.cap) {
    if (D->d_xy) (void)hipFree(D->d_xy);
    if (D->d_oct) (void)hipFree(D->d_oct);
    D->d_xy = nullptr;
    D->d_oct = nullptr;
    const int cap = n;
    VO_CHECK_HIP(c, vo_dev_malloc(c, (void **)&D->d_xy, sizeof(float) * 2 * (size_t)cap));
    VO_CHECK_HIP(c, vo_dev_malloc(c, (void **)&D->d_oct, sizeof(int32_t) * (size_t)cap));
    rc = ensure_set(c, D->own, cap);
    if (rc) return rc;
  }
  hipStream_t s = c->stream;
  VO_CHECK_HIP(c, hipMemcpyAsync(D->d_xy, kp_xy, sizeof(float) * 2 * (size_t)n, hipMemcpyHostToDevice, s));
  VO_CHECK_HIP(c, hipMemcpyAsync(D->d_oct, kp_octave, sizeof(int32_t) * (size_t)n, hipMemcpyHostToDevice, s));
  rc = describe_enqueue(c, v, D->d_xy, D->d_oct, n, nullptr, steer, D->own);
  if (rc) return rc;
  if (angle_out) VO_CHECK_HIP(c, hipMemcpyAsync(angle_out, D->own.angle, sizeof(float) * (size_t)n, hipMemcpyDeviceToHost, s));
  if (desc_out) VO_CHECK_HIP(c, hipMemcpyAsync(desc_out, D->own.desc, (size_t)n * 32, hipMemcpyDeviceToHost, s));
  if (valid_out) VO_CHECK_HIP(c, hipMemcpyAsync(valid_out, D->own.valid, (size_t)n, hipMemcpyDeviceToHost, s));
  VO_CHECK_HIP(c, hipStreamSynchronize(s));
  return VO_OK;
}

extern "C" int vo_orb_detect_and_compute(vo_ctx *c, int slot, const vo_orb_params *p, int steer, int set, float *kp_xy, float *kp_response,
                                         int32_t *kp_octave, float *kp_angle, uint8_t *desc, int max_kp, int *n_out) {
  if (!c || !p || !n_out || max_kp < 0 || set < 0 || set > 1) return VO_ERR_INVALID;
  VO_CHECK_HIP(c, hipSetDevice(c->device));
  int rc = desc_state(c);
  if (rc) return rc;
  vo_orb_view v;
  rc = vo_orb_levels_enqueue(c, slot, p, true, &v);
  if (rc) return rc;
  vo_orb_desc_set &S = c->orb_desc->set[set];
  S.n = 0;
  rc = ensure_set(c, S, v.max_out);
  if (rc) return rc;
  rc = describe_enqueue(c, v, v.xy, v.oct, v.max_out, v.n_dev, steer, S);
  if (rc) return rc;
  hipStream_t s = c->stream;
  int n = 0, flags = 0;
  VO_CHECK_HIP(c, hipMemcpyAsync(&n, v.n_dev, sizeof(int), hipMemcpyDeviceToHost, s));
  VO_CHECK_HIP(c, hipMemcpyAsync(&flags, v.flags_dev, sizeof(int), hipMemcpyDeviceToHost, s));
  VO_CHECK_HIP(c, hipStreamSynchronize(s));
  rc = vo_orb_check_flags(c, flags);
  if (rc) return rc;
  if (n > max_kp) VO_FAIL(c, VO_ERR_CAPACITY, "%d keypoints, the caller's buffers hold %d", n, max_kp);
  S.n = n;
  if (n > 0) {
    if (kp_xy) VO_CHECK_HIP(c, hipMemcpy(kp_xy, v.xy, sizeof(float) * 2 * (size_t)n, hipMemcpyDeviceToHost));
    if (kp_response) VO_CHECK_HIP(c, hipMemcpy(kp_response, v.resp, sizeof(float) * (size_t)n, hipMemcpyDeviceToHost));
    if (kp_octave) VO_CHECK_HIP(c, hipMemcpy(kp_octave, v.oct, sizeof(int32_t) * (size_t)n, hipMemcpyDeviceToHost));
    if (kp_angle) VO_CHECK_HIP(c, hipMemcpy(kp_angle, S.angle, sizeof(float) * (size_t)n, hipMemcpyDeviceToHost));
    if (desc) VO_CHECK_HIP(c, hipMemcpy(desc, S.desc, (size_t)n * 32, hipMemcpyDeviceToHost));
  }
  *n_out = n;
  return VO_OK;
}

extern "C" int vo_orb_match_sets(vo_ctx *c, int set_a, int set_b, int th_low, float ratio, int32_t *best_idx, uint16_t *best_dist,
                                 uint16_t *second_dist) {
  if (!c || !best_idx || !best_dist || !second_dist || set_a < 0 || set_a > 1 || set_b < 0 || set_b > 1) return VO_ERR_INVALID;
  vo_orb_desc_state *D = c->orb_desc;
  if (!D) VO_FAIL(c, VO_ERR_INVALID, "no descriptor set: call vo_orb_detect_and_compute first");
  const int na = D->set[set_a].n, nb = D->set[set_b].n;
  if (na == 0) return VO_OK;
  VO_CHECK_HIP(c, hipSetDevice(c->device));
  if (na > D->match_cap) {
    void *old[] = {D->d_best, D->d_bd, D->d_sd};
    for (void *b : old)
      if (b) (void)hipFree(b);
    D->d_best = nullptr;
    D->d_bd = D->d_sd = nullptr;
    D->match_cap = 0;
    const int cap = D->set[set_a].cap;  // (a set's capacity: no growth from call to call)
    VO_CHECK_HIP(c, vo_dev_malloc(c, (void **)&D->d_best, sizeof(int32_t) * (size_t)cap));
    VO_CHECK_HIP(c, vo_dev_malloc(c, (void **)&D->d_bd, sizeof(uint16_t) * (size_t)cap));
    VO_CHECK_HIP(c, vo_dev_malloc(c, (void **)&D->d_sd, sizeof(uint16_t) * (size_t)cap));
    D->match_cap = cap;
  }
  int rc = vo_match_enqueue(c, D->set[set_a].desc, na, D->set[set_b].desc, nb, th_low, ratio, D->d_best, D->d_bd, D->d_sd);
  if (rc < 0) return rc;
  hipStream_t s = c->stream;
  VO_CHECK_HIP(c, hipMemcpyAsync(best_idx, D->d_best, sizeof(int32_t) * (size_t)na, hipMemcpyDeviceToHost, s));
  VO_CHECK_HIP(c, hipMemcpyAsync(best_dist, D->d_bd, sizeof(uint16_t) * (size_t)na, hipMemcpyDeviceToHost, s));
  VO_CHECK_HIP(c, hipMemcpyAsync(second_dist, D->d_sd, sizeof(uint16_t) * (size_t)na, hipMemcpyDeviceToHost, s));
  VO_CHECK_HIP(c, hipStreamSynchronize(s));
  return VO_OK;
}
