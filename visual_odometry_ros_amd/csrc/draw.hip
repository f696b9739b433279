// draw.hip — the drivers' debug image on the device. Reference: showTracking / showTrackingBA of both drivers
// (stereo_vo.cpp:685-688, mono_vo.cpp:554-555, :626-627, :903-904 draw into img_debug_ on every tracked frame). The current
// image and the final track set are on the device when a frame ends, so the picture is made there:
//   1. draw_cover_kernel    one wavefront per primitive: atomicMax of (primitive number + 1) over the pixels it covers, into a
//                           W x H uint32 plane (0 = none). Stamps span at most 15 x 15 pixels; a line is walked over the
//                           part of its major axis that lies inside the image, so no loop is longer than max(W, H) / 64.
//   2. draw_resolve_kernel  four pixels per lane: level 0 of the slot replicated into three channels (CV_GRAY2RGB) or the
//                           colour of the pixel's highest primitive; 12 bytes = three dword stores.
// A driver's job may leave the sizes of its point sets, and whether it is drawn at all, to words in device memory (DrawDev).
// The rules themselves (numbering, coverage, colours) are csrc/draw_device.hpp; include/vo_hip.h states them.
#include "vo_internal.hpp"
#include "vo_kernels.hpp"
#include "draw_device.hpp"

struct vo_draw_state {
  vo_draw_buffers b;
  float *pts;       // 3 sets x max_points x 2: the operators' points
};

#define DRAW_WAVES 4
// What a driver's job leaves to the device (any pointer may be null: the host's value holds). n0 / n1: the sizes of p0 / p1 of a
// tracking_ba job, clamped to [0, cap] (the grid is sized for them). go: *go == 0 skips the job as a whole — no pixel of the
// picture is written, so the device picture stays the previous one.
struct DrawDev {
  const int *n0, *n1, *go;
  int cap;
};
__device__ __forceinline__ bool draw_dev_apply(DrawJob &j, const DrawDev &d) {
  if (d.go && *d.go == 0) return false;
  if (d.n0) {
    const int n = *d.n0;
    j.n0 = n < 0 ? 0 : (n < d.cap ? n : d.cap);
  }
  if (d.n1) {
    const int n = *d.n1;
    j.n1 = n < 0 ? 0 : (n < d.cap ? n : d.cap);
  }
  return true;
}
__global__ __launch_bounds__(64 * DRAW_WAVES) void draw_cover_kernel(DrawJob j, DrawDev d, uint32_t *__restrict__ idx) {
  const int prim = blockIdx.x * DRAW_WAVES + (threadIdx.x >> 6);
  if (!draw_dev_apply(j, d)) return;
  if (prim >= draw_prim_count(j)) return;
  const uint32_t tag = (uint32_t)prim + 1u;
  draw_cover(j, prim, threadIdx.x & 63, 64, [&](int x, int y) { atomicMax(idx + (size_t)y * j.w + x, tag); });
}

__global__ __launch_bounds__(256) void draw_resolve_kernel(DrawJob j, DrawDev d, const uint32_t *__restrict__ idx,
                                                           const uint8_t *__restrict__ lv0, int lstride,
                                                           uint32_t *__restrict__ out) {
  const int g = blockIdx.x * blockDim.x + threadIdx.x, total = j.w * j.h;
  const int i = 4 * g;
  if (i >= total) return;
  if (!draw_dev_apply(j, d)) return;
  int y = i / j.w, x = i - y * j.w;
  uint32_t c[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    c[q] = 0u;
    if (i + q < total) {
      const uint32_t tag = idx[i + q];
      c[q] = tag ? draw_colour(j, (int)tag - 1) : 0x00010101u * lv0[(size_t)y * lstride + x];
      if (++x == j.w) {
        x = 0;
        ++y;
      }
    }
  }
  out[3 * (size_t)g + 0] = c[0] | (c[1] << 24);
  out[3 * (size_t)g + 1] = (c[1] >> 8) | (c[2] << 16);
  out[3 * (size_t)g + 2] = (c[2] >> 16) | (c[3] << 8);
}

int vo_draw_buffers_alloc(vo_ctx *c, vo_draw_buffers *b) {
  const size_t px = (size_t)c->cfg.max_width * c->cfg.max_height;
  b->img_bytes = (px + 3) / 4 * 12;  // (the resolve pass stores 12 bytes per four pixels)
  VO_CHECK_HIP(c, vo_dev_malloc(c, (void **)&b->idx, px * sizeof(uint32_t)));
  VO_CHECK_HIP(c, vo_dev_malloc(c, (void **)&b->img, b->img_bytes));
  VO_CHECK_HIP(c, vo_host_malloc(c, (void **)&b->h_img, b->img_bytes, hipHostMallocDefault));
  return VO_OK;
}
void vo_draw_buffers_free(vo_draw_buffers *b) {
  if (b->idx) (void)hipFree(b->idx);
  if (b->img) (void)hipFree(b->img);
  if (b->h_img) (void)hipHostFree(b->h_img);
  memset(b, 0, sizeof(*b));
}

void vo_draw_free(vo_ctx *c) {
  vo_draw_state *s = c->draw;
  if (!s) return;
  vo_draw_buffers_free(&s->b);
  if (s->pts) (void)hipFree(s->pts);
  free(s);
  c->draw = nullptr;
}

// the context's drawing buffers, allocated by the first call that needs them
static int draw_ensure(vo_ctx *c) {
  if (c->draw) return VO_OK;
  vo_draw_state *s = (vo_draw_state *)calloc(1, sizeof(vo_draw_state));
  if (!s) VO_FAIL(c, VO_ERR_INVALID, "out of host memory");
  c->draw = s;
  const int rc = vo_draw_buffers_alloc(c, &s->b);
  if (rc) return rc;
  VO_CHECK_HIP(c, vo_dev_malloc(c, (void **)&s->pts, sizeof(float) * 6 * (size_t)c->cfg.max_points));
  return VO_OK;
}

// the two launches on `st`: j's point sets are DEVICE pointers, the picture goes to s->img and, behind it, to s->h_img.
// d: see DrawDev (with a device-side count the grid is sized for d.cap points per such set). A job skipped by *d.go leaves
// s->img as it was; the copy behind it then moves the same bytes into s->h_img again.
static int draw_enqueue(vo_ctx *c, hipStream_t st, int slot, DrawJob j, vo_draw_buffers *s, DrawDev d = DrawDev{nullptr, nullptr, nullptr, 0}) {
  const vo_level &L = c->slots[slot].lv[0];
  j.w = L.w;
  j.h = L.h;
  const size_t px = (size_t)L.w * L.h;
  VO_CHECK_HIP(c, hipMemsetAsync(s->idx, 0, px * sizeof(uint32_t), st));
  DrawJob most = j;  // (the largest job the device may make of it)
  if (d.n0) most.n0 = d.cap;
  if (d.n1) most.n1 = d.cap;
  const int n_prims = draw_prim_count(most);
  if (n_prims > 0)
    hipLaunchKernelGGL(draw_cover_kernel, dim3((n_prims + DRAW_WAVES - 1) / DRAW_WAVES), dim3(64 * DRAW_WAVES), 0, st, j, d, s->idx);
  const int lanes = (int)((px + 3) / 4);
  hipLaunchKernelGGL(draw_resolve_kernel, dim3((lanes + 255) / 256), dim3(256), 0, st, j, d, s->idx, L.origin(), L.stride, (uint32_t *)s->img);
  VO_CHECK_HIP(c, hipGetLastError());
  VO_CHECK_HIP(c, hipMemcpyAsync(s->h_img, s->img, px * 3, hipMemcpyDeviceToHost, st));
  return VO_OK;
}

int vo_draw_ba_enqueue(vo_ctx *c, hipStream_t st, int slot, const float *d_pts_proj, const int *d_n, int cap, vo_draw_buffers *b) {
  DrawJob j;
  memset(&j, 0, sizeof(j));
  j.mode = 1;
  j.p1 = d_pts_proj;
  return draw_enqueue(c, st, slot, j, b, DrawDev{nullptr, d_n, nullptr, cap});
}

int vo_draw_ba_sets_enqueue(vo_ctx *c, hipStream_t st, int slot, const float *d_pts, const float *d_pts_proj, const int *d_n, int cap,
                            const int *d_go, vo_draw_buffers *b) {
  DrawJob j;
  memset(&j, 0, sizeof(j));
  j.mode = 1;
  j.p0 = d_pts;
  j.p1 = d_pts_proj;
  return draw_enqueue(c, st, slot, j, b, DrawDev{d_n, d_n, d_go, cap});
}

int vo_draw_tracking_enqueue(vo_ctx *c, hipStream_t st, int slot, const float *d_pts0, int n0, const float *d_pts1, int n1,
                             const float *d_pts_new, int n_new, vo_draw_buffers *b) {
  DrawJob j;
  memset(&j, 0, sizeof(j));
  j.mode = 0;
  j.n0 = n0;
  j.n1 = n1;
  j.n2 = n_new;
  j.p0 = d_pts0;
  j.p1 = d_pts1;
  j.p2 = d_pts_new;
  return draw_enqueue(c, st, slot, j, b);
}

static int draw_host(vo_ctx *c, int slot, DrawJob j, const float *const sets[3], const int n[3], uint8_t *out, int out_stride) {
  if (slot < 0 || slot >= c->cfg.n_slots) VO_FAIL(c, VO_ERR_INVALID, "slot out of range");
  const vo_pyramid &P = c->slots[slot];
  if (P.n_levels < 1) VO_FAIL(c, VO_ERR_INVALID, "slot %d holds no image", slot);
  for (int k = 0; k < 3; ++k) {
    if (n[k] < 0 || (n[k] > 0 && !sets[k])) VO_FAIL(c, VO_ERR_INVALID, "point set %d: n = %d, pointer %p", k, n[k], (const void *)sets[k]);
    if (n[k] > c->cfg.max_points) VO_FAIL(c, VO_ERR_CAPACITY, "n=%d exceeds vo_config.max_points=%d", n[k], c->cfg.max_points);
  }
  if (out_stride < 3 * P.w) VO_FAIL(c, VO_ERR_INVALID, "out_stride %d is below 3 x width = %d", out_stride, 3 * P.w);
  VO_CHECK_HIP(c, hipSetDevice(c->device));
  int rc = draw_ensure(c);
  if (rc) return rc;
  vo_draw_state *s = c->draw;
  vo_draw_buffers *b = &s->b;
  if (vo_slot_acquire(c, slot) < 0) return VO_ERR_HIP;
  const float *dev[3];
  for (int k = 0; k < 3; ++k) {
    dev[k] = s->pts + 2 * (size_t)k * c->cfg.max_points;
    if (n[k] > 0)
      VO_CHECK_HIP(c, hipMemcpyAsync((void *)dev[k], sets[k], sizeof(float) * 2 * (size_t)n[k], hipMemcpyHostToDevice, c->stream));
  }
  j.p0 = dev[0];
  j.p1 = dev[1];
  j.p2 = dev[2];
  rc = draw_enqueue(c, c->stream, slot, j, b);
  if (rc) return rc;
  VO_CHECK_HIP(c, hipStreamSynchronize(c->stream));
  for (int y = 0; y < P.h; ++y) memcpy(out + (size_t)y * out_stride, b->h_img + (size_t)y * 3 * P.w, (size_t)3 * P.w);
  return VO_OK;
}

extern "C" int vo_draw_tracking(vo_ctx *c, int slot, const float *pts0, int n0, const float *pts1, int n1, const float *pts_new,
                                int n_new, uint8_t *out, int out_stride) {
  if (!c || !out) return VO_ERR_INVALID;
  if (n1 > n0) VO_FAIL(c, VO_ERR_INVALID, "vo_draw_tracking: n1 = %d exceeds n0 = %d (a line joins pts0[i] and pts1[i])", n1, n0);
  DrawJob j;
  memset(&j, 0, sizeof(j));
  j.mode = 0;
  j.n0 = n0;
  j.n1 = n1;
  j.n2 = n_new;
  const float *const sets[3] = {pts0, pts1, pts_new};
  const int n[3] = {n0, n1, n_new};
  return draw_host(c, slot, j, sets, n, out, out_stride);
}

extern "C" int vo_draw_tracking_ba(vo_ctx *c, int slot, const float *pts, int n, const float *pts_proj, int n_proj, uint8_t *out,
                                   int out_stride) {
  if (!c || !out) return VO_ERR_INVALID;
  DrawJob j;
  memset(&j, 0, sizeof(j));
  j.mode = 1;
  j.n0 = n;
  j.n1 = n_proj;
  const float *const sets[3] = {pts, pts_proj, nullptr};
  const int nn[3] = {n, n_proj, 0};
  return draw_host(c, slot, j, sets, nn, out, out_stride);
}
