// clahe.hip — CLAHE equalisation in front of the image ingestion (include/vo_hip.h: vo_set_equalize): the option's
// state and storage, the two launches (clahe_device.hpp) and the operator on its own (vo_equalize_image).
//
// Hook: pyramid.hip's build() — the one place every ingestion entry point goes through — calls vo_equalize_enqueue in front of the
// rectifying remap / the pyramid launch, on the stream of the ingestion chain, and reads on from the slot's equalised plane. The
// caller's image is only read. With the option off nothing here is reached.
#include "vo_internal.hpp"
#include "vo_kernels.hpp"

#include <math.h>

#define CLAHE_LD_AGENT(p) __hip_atomic_load((p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)
#define CLAHE_ST_AGENT(p, v) __hip_atomic_store((p), (v), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)
#define CLAHE_ATOMIC_ADD_AGENT(p, v) __hip_atomic_fetch_add((p), (v), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)
// (the explicit wait behind the release: the counts of this thread have left before the barrier in front of the ticket)
#define CLAHE_FENCE_RELEASE()                             \
  do {                                                    \
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");    \
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");      \
  } while (0)
#define CLAHE_FENCE_ACQUIRE() __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent")
#define CLAHE_DYN_LDS(name) extern __shared__ __attribute__((aligned(16))) uint8_t name[]
#include "clahe_device.hpp"

// ---- storage: [plane | tables | counters | tickets] per slot, sized for vo_config's largest image and 32 x 32 tiles ------------------
static size_t eq_plane_stride(const vo_ctx *c) { return ((size_t)c->cfg.max_width + 63) & ~(size_t)63; }
static size_t eq_plane_bytes(const vo_ctx *c) { return (eq_plane_stride(c) * (size_t)c->cfg.max_height + 255) & ~(size_t)255; }
static const size_t EQ_TILES = (size_t)CLAHE_MAX_TILES * CLAHE_MAX_TILES;
static const size_t EQ_LUT_BYTES = EQ_TILES * 256, EQ_HIST_BYTES = EQ_TILES * 256 * sizeof(int), EQ_TICKET_BYTES = EQ_TILES * sizeof(int);

static int eq_alloc_one(vo_ctx *c, uint8_t **p, size_t planes) {
  const size_t head = planes * eq_plane_bytes(c) + EQ_LUT_BYTES;
  VO_CHECK_HIP(c, vo_dev_malloc(c, (void **)p, head + EQ_HIST_BYTES + EQ_TICKET_BYTES));
  VO_CHECK_HIP(c, hipMemsetAsync(*p + head, 0, EQ_HIST_BYTES + EQ_TICKET_BYTES, c->stream_main));  // counters and tickets start at zero
  return VO_OK;
}

void vo_equalize_free(vo_ctx *c) {
  if (c->slots)
    for (int s = 0; s < c->cfg.n_slots; ++s)
      if (c->slots[s].eq) {
        (void)hipFree(c->slots[s].eq);
        c->slots[s].eq = nullptr;
      }
  if (c->eq_op) (void)hipFree(c->eq_op);
  c->eq_op = nullptr;
}

extern "C" int vo_set_equalize(vo_ctx *c, int mode, double clip_limit, int tiles_x, int tiles_y) {
  if (!c) return VO_ERR_INVALID;
  if (mode != VO_EQ_OFF && mode != VO_EQ_CLAHE) VO_FAIL(c, VO_ERR_INVALID, "equalisation mode %d: expected VO_EQ_OFF (0) or VO_EQ_CLAHE (1)", mode);
  if (tiles_x < 1 || tiles_x > CLAHE_MAX_TILES || tiles_y < 1 || tiles_y > CLAHE_MAX_TILES)
    VO_FAIL(c, VO_ERR_INVALID, "%d x %d tiles: both counts must be in 1..%d", tiles_x, tiles_y, CLAHE_MAX_TILES);
  if (!(clip_limit >= 0.0) || !isfinite(clip_limit)) VO_FAIL(c, VO_ERR_INVALID, "the clip limit must be finite and >= 0 (0: no clipping)");
  if (mode == VO_EQ_CLAHE && c->input_format != VO_PIX_MONO8)
    VO_FAIL(c, VO_ERR_INVALID, "equalisation takes 8-bit grey images: the context's input format is not VO_PIX_MONO8");
  if (vo_frame_in_flight(c)) VO_FAIL(c, VO_ERR_INVALID, "a frame is in flight: collect its result before changing the equalisation");
  if (mode == VO_EQ_CLAHE && !c->eq_op) {  // every allocation of the option, the first time it is turned on
    VO_CHECK_HIP(c, hipSetDevice(c->device));
    for (int s = 0; s < c->cfg.n_slots; ++s)
      if (!c->slots[s].eq) {
        const int rc = eq_alloc_one(c, &c->slots[s].eq, 1);
        if (rc) return rc;
      }
    const int rc = eq_alloc_one(c, &c->eq_op, 2);
    if (rc) return rc;
    // the counters are zero before anything on either ingest stream counts into them
    VO_CHECK_HIP(c, hipStreamSynchronize(c->stream_main));
  }
  c->eq_mode = mode;
  c->eq_clip = clip_limit;
  c->eq_tiles_x = tiles_x;
  c->eq_tiles_y = tiles_y;
  return VO_OK;
}

extern "C" int vo_get_equalize(vo_ctx *c, int *mode, double *clip_limit, int *tiles_x, int *tiles_y) {
  if (!c || !mode || !clip_limit || !tiles_x || !tiles_y) return VO_ERR_INVALID;
  *mode = c->eq_mode;
  *clip_limit = c->eq_clip;
  *tiles_x = c->eq_tiles_x;
  *tiles_y = c->eq_tiles_y;
  return VO_OK;
}

int vo_equalize_check(vo_ctx *c, int w, int h) {
  if (c->input_format != VO_PIX_MONO8) VO_FAIL(c, VO_ERR_INVALID, "equalisation takes 8-bit grey images");
  if (w <= c->eq_tiles_x || h <= c->eq_tiles_y)  // (the reflected extension reads up to tiles_x columns / tiles_y rows back)
    VO_FAIL(c, VO_ERR_SIZE, "a %d x %d image is not larger than the %d x %d tiles of the equalisation", w, h, c->eq_tiles_x, c->eq_tiles_y);
  return VO_OK;
}

// both launches for one image or a pair; store[i]: the [plane | tables | counters | tickets] block of image i, `skip` planes in
static int eq_launch(vo_ctx *c, int nimg, const uint8_t *const *src, int stride, uint8_t *const *store, size_t skip, int w, int h) {
  ClaheArgs a;
  memset(&a, 0, sizeof(a));
  const size_t pb = eq_plane_bytes(c);
  for (int i = 0; i < 2; ++i) {
    const int k = i < nimg ? i : 0;
    uint8_t *base = store[k] + skip * pb;
    a.img[i].src = src[k];
    a.img[i].dst = base;
    a.img[i].lut = base + pb;
    a.img[i].hist = (int *)(base + pb + EQ_LUT_BYTES);
    a.img[i].ticket = (int *)(base + pb + EQ_LUT_BYTES + EQ_HIST_BYTES);
  }
  const int tx = c->eq_tiles_x, ty = c->eq_tiles_y;
  clahe_plan(&a, w, h, tx, ty, c->eq_clip, 8192);
  a.sstride = stride;
  a.dstride = (int)eq_plane_stride(c);
  const size_t lds = (size_t)a.lds_cols * a.lds_rows * 256;
  if (!clahe_stage_fits(&a))  // (a sizing bug would otherwise leave the plane unwritten without a word)
    VO_FAIL(c, VO_ERR_INVALID, "equalisation: the blend's LDS stage (%d x %d tables) does not hold a workgroup's tables at %d x %d, %d x %d tiles",
            a.lds_cols, a.lds_rows, w, h, tx, ty);
  hipLaunchKernelGGL(clahe_hist_kernel, dim3(a.slabs, tx * ty, nimg), dim3(CLAHE_NT), 0, c->stream, a);
  hipLaunchKernelGGL(clahe_blend_kernel, dim3((w + CLAHE_BLEND_COLS - 1) / CLAHE_BLEND_COLS, (h + CLAHE_BLEND_ROWS - 1) / CLAHE_BLEND_ROWS, nimg),
                     dim3(CLAHE_NT), lds, c->stream, a);
  VO_CHECK_HIP(c, hipGetLastError());
  return VO_OK;
}

int vo_equalize_enqueue(vo_ctx *c, int nimg, const int *slots, const uint8_t *const *src, int stride, int w, int h, const uint8_t **eq,
                        int *eq_stride) {
  uint8_t *store[2] = {nullptr, nullptr};
  for (int i = 0; i < nimg; ++i) {
    store[i] = c->slots[slots[i]].eq;
    if (!store[i]) VO_FAIL(c, VO_ERR_INVALID, "slot %d has no equalisation storage", slots[i]);
    eq[i] = store[i];
  }
  *eq_stride = (int)eq_plane_stride(c);
  return eq_launch(c, nimg, src, stride, store, 0, w, h);
}

extern "C" int vo_equalize_image(vo_ctx *c, const void *src, int stride, int width, int height, void *dst, int dst_stride, uint8_t *luts,
                                 int on_device) {
  if (!c || !src || !dst) return VO_ERR_INVALID;
  if (c->eq_mode != VO_EQ_CLAHE) VO_FAIL(c, VO_ERR_INVALID, "vo_equalize_image: equalisation is off (vo_set_equalize)");
  if (width <= 0 || height <= 0 || width > c->cfg.max_width || height > c->cfg.max_height)
    VO_FAIL(c, VO_ERR_CAPACITY, "image %dx%d exceeds vo_config %dx%d", width, height, c->cfg.max_width, c->cfg.max_height);
  if (stride < width || dst_stride < width) VO_FAIL(c, VO_ERR_INVALID, "a stride is below the image width %d", width);
  if (on_device != VO_EQ_HOST && on_device != VO_EQ_DEVICE && on_device != VO_EQ_DEVICE_TO_HOST)
    VO_FAIL(c, VO_ERR_INVALID, "on_device %d: expected VO_EQ_HOST (0), VO_EQ_DEVICE (1) or VO_EQ_DEVICE_TO_HOST (2)", on_device);
  const bool src_dev = on_device != VO_EQ_HOST, dst_dev = on_device == VO_EQ_DEVICE;
  int rc = vo_equalize_check(c, width, height);
  if (rc) return rc;
  VO_CHECK_HIP(c, hipSetDevice(c->device));
  const uint8_t *in = (const uint8_t *)src;
  int in_stride = stride;
  if (!src_dev) {  // a host image goes through the operator's staging plane
    VO_CHECK_HIP(c, hipMemcpy2DAsync(c->eq_op, (size_t)width, src, (size_t)stride, (size_t)width, (size_t)height, hipMemcpyHostToDevice, c->stream));
    in = c->eq_op;
    in_stride = width;
  }
  uint8_t *store[2] = {c->eq_op, nullptr};
  rc = eq_launch(c, 1, &in, in_stride, store, 1, width, height);
  if (rc) return rc;
  const uint8_t *out = c->eq_op + eq_plane_bytes(c);
  const hipMemcpyKind kind = dst_dev ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
  VO_CHECK_HIP(c, hipMemcpy2DAsync(dst, (size_t)dst_stride, out, eq_plane_stride(c), (size_t)width, (size_t)height, kind, c->stream));
  if (luts)
    VO_CHECK_HIP(c, hipMemcpyAsync(luts, out + eq_plane_bytes(c), (size_t)c->eq_tiles_x * c->eq_tiles_y * 256, kind, c->stream));
  VO_CHECK_HIP(c, hipStreamSynchronize(c->stream));
  return VO_OK;
}
