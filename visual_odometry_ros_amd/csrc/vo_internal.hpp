// vo_internal.hpp — context layout and device helpers shared by the gfx950 kernels.
// Wave width is 64 everywhere (CDNA4); reductions use DPP butterflies whose
// summation tree is the balanced binary tree over lanes in natural order
// (adjacent pairs first) — the order oracle/ calls VO_SUM_TREE.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "../../include/vo_hip.h"

#define VO_ALIGNBYTE(hi, lo, n) __builtin_amdgcn_alignbyte((hi), (lo), (n))
#include "vo_layout.hpp"   // VO_PAD, VO_MAX_LEVELS, vo_level, vo_reflect101
#define VO_WAVE 64

struct vo_pyramid {
  vo_level lv[VO_MAX_LEVELS];
  int n_levels;    // levels built (0..n_levels-1 valid)
  int w, h;
  uint8_t *mem;    // one allocation for all levels
  size_t bytes;
  // ordering across the context's two streams: `ready` is recorded behind every build of the slot, on the stream
  // that built it; a consumer on the other stream waits for it once (vo_slot_acquire)
  hipEvent_t ready;
  uint8_t seen[2];  // [0] main stream / [1] side stream is already ordered behind the last build
  unsigned gen;     // counts the builds of this slot: what was computed from a slot names the build it read
  uint8_t *stage;  // device staging for an image that arrives from the host asynchronously (allocated on demand)
  // the ignore mask of the image in this slot (vo_set_slot_mask, the drivers' ingestion): a tightly packed mask_w x mask_h plane,
  // allocated at the first set (vo_config.max_width x max_height bytes), read by the detector's vote and the track gate while
  // mask_on. Ordered across the two streams like the pyramid: mask_ready behind every write, mask_seen per stream.
  uint8_t *mask;
  int mask_w, mask_h, mask_on;
  hipEvent_t mask_ready;
  uint8_t mask_seen[2];
  unsigned mask_ver;  // the drivers: version of their master plane this copy was made from (0: none)
  // vo_set_equalize (clahe.hip): the equalised image of this slot, the look-up tables and the histogram counters behind it in one
  // allocation, made when the option is first turned on. Written and read by the slot's ingestion chain only, on its stream.
  uint8_t *eq;
};

struct vo_gn_dev_info {
  int iterations;
  float err, delta_err, delta_norm;
  int cnt_invalid;
  int is_nan;
};

struct vo_prof_rec {
  hipEvent_t a, b;
  int cls;
};

struct vo_ctx {
  vo_config cfg;
  int device;
  hipStream_t stream;      // the stream launchers enqueue on (= stream_main, except while a side-stream chain is built)
  hipStream_t stream_main;
  hipStream_t stream2;     // side stream: work that does not depend on the main chain of a frame
  hipStream_t stream3;     // the strict-border replay of the frame in flight (runs next to the frame kernel)
  int ingest_side;         // vo_set_ingest_side_stream: image ingestion (H2D, pyramids) runs on the side stream
  // StereoVO's synchronous call with host images: the detection of the LEFT image is started from its staging plane as soon
  // as that upload is queued (vo_set_stereo_pair_host_async), not behind the pair's pyramids; armed per call, consumed there
  const vo_bin_params *early_bins;
  int early_table, early_issued;
  hipEvent_t ev_fork, ev_join;
  hipEvent_t ev_pyr;       // recorded behind every pyramid build: what side-stream consumers of a slot wait for
  char err[512];
  vo_pyramid *slots;
  // per-point device buffers (capacity cfg.max_points)
  float *d_pts0, *d_pts1, *d_pts2, *d_pts3, *d_err, *d_err2, *d_scale, *d_X, *d_X2;
  uint8_t *d_status, *d_status2, *d_mask, *d_mask2;
  int32_t *d_idx;
  int *d_count;
  float *d_mat;            // small matrices / scalars
  vo_gn_dev_info *d_gninfo;
  int *d_flags;            // error flags raised by kernels
  // pinned host staging
  uint8_t *h_stage;
  size_t h_stage_bytes;
  uint8_t *d_img_stage;    // device staging for host images
  // vo_set_input_format (rectify.hip): what the rectifying entry points take; both staging buffers hold stage_bpp bytes per pixel
  int input_format;        // VO_PIX_*, 0 = VO_PIX_MONO8
  int stage_bpp;
  // hamming
  uint8_t *d_desc_a, *d_desc_b;
  uint16_t *d_dist;
  size_t desc_cap, dist_cap;
  // frame pipeline state
  void *ic_rec;            // tap records of the IC strict replay (ic_refine.hip)
  struct vo_frame_state *frame;
  int frame_strict_ic;     // replay border-touching points with the reference's sticky tap state (as requested: 0..4)
  int frame_strict_now;    // the stereo frame in flight: 4 (automatic) resolved to 1 or 3
  int frame_recoveries;    // frames issued again after such a time-out (vo_stereo_frame_recoveries)
  int frame_conc_off;      // a device-side join timed out once: the concurrent arrangements (3, 5, 4 -> 3) are off for good
  int frame_slots_busy;    // a frame is in flight and reads frame_slot[0..2]
  int frame_slot[3];
  int sum_order;           // VO_SUM_ORDER_*: read by every launch of the IC and GN kernels (0: tree, the default)
  // profiling
  vo_prof_rec *prof;
  int prof_cap, prof_n;
  unsigned prof_mask;      // bit per kernel class; 0 = all
  int prof_open;           // begin() recorded an event that end() must close
  int pyr_win_hint;        // > 0: build only the levels calcOpticalFlowPyrLK would use for this window
  // undistortion / rectification maps (rectify.hip): camera 0 = left or mono, 1 = right
  float *rect_u[2], *rect_v[2];
  int rect_w[2], rect_h[2];
  // per-stream ID counters: Landmark::landmark_counter_ (landmark.h:64) and Frame::frame_counter_ (frame.h:53) are
  // process-global in the reference; one pair per context keeps the streams of a batch from interleaving
  int32_t next_landmark_id, next_frame_id;
  struct vo_sba_state *sba;  // device arena of the sparse local BA (sba.hip)
  struct vo_orb_state *orb;  // pyramid, score planes and candidate lists of the keypoint detector (orb_detect.hip)
  struct vo_orb_desc_state *orb_desc;  // pattern table, resident descriptor sets (orb_describe.hip)
  struct vo_draw_state *draw;          // index plane and picture of the debug image (draw.hip), allocated on first use
  // every device / pinned allocation made on behalf of this context (vo_dev_malloc / vo_host_malloc): what
  // vo_debug_allocation_count reports, so that a test can assert that a steady-state frame allocates nothing
  long long n_allocs;
  // vo_debug_set: test / measurement switches of THIS context (never read from the environment inside the library)
  int dbg[VO_DBG_COUNT];
  // versions of the drivers' mask masters (vo_driver_mask_set): drawn from ONE counter per context, so that a slot's copy made
  // from one driver's master is never taken for a copy of another driver's (several drivers follow each other on a context)
  unsigned mask_ver_next;
  // vo_set_equalize (clahe.hip): every 8-bit image that enters a slot is equalised first. eq_mode == VO_EQ_OFF: nothing of it runs.
  int eq_mode, eq_tiles_x, eq_tiles_y;
  double eq_clip;
  uint8_t *eq_op;  // vo_equalize_image's own storage: a staging plane in front of what a slot has
  // the ZNCC gate of the driver whose frame is in flight (zncc.hip); null: none — the frame operators then launch nothing
  struct vo_zncc_gate *zncc_gate;
  struct vo_semidense_temporal_state *semidense_t;  // vo_semidense_temporal / vo_semidense_map_seed with host planes: their device copies
  struct vo_semidense_state *semidense;  // vo_semidense_stereo / vo_semidense_points: their planes and scratch (semidense.hip), made on first use
  struct vo_semidense_propagate_state *semidense_p;  // vo_semidense_map_propagate: its keys and, for host planes, the new map's device copies
  struct vo_semidense_align_state *semidense_a;  // vo_semidense_align: its state block and partial sums
  struct vo_semidense_regularize_state *semidense_r;  // vo_semidense_map_regularize with host planes: the mask's and the outputs' device copies
  struct vo_dense_stereo_state *dense_stereo;  // vo_dense_stereo: its workspace and, for host outputs, the planes (dense_stereo.hip), made on first use
  struct vo_speckle_state *speckle;  // vo_disparity_speckle_filter: its workspace and, for host planes, their device copies (dense_speckle.hip), made on first use
  struct vo_semidense_merge_state *semidense_m;  // vo_semidense_map_merge: its counts and, for host planes, their device copies (semidense_map_merge.hip), made on first use
};

static inline hipError_t vo_dev_malloc(vo_ctx *c, void **p, size_t bytes) {
  if (c) ++c->n_allocs;
  return hipMalloc(p, bytes);
}
static inline hipError_t vo_host_malloc(vo_ctx *c, void **p, size_t bytes, unsigned flags) {
  if (c) ++c->n_allocs;
  return hipHostMalloc(p, bytes, flags);
}

#define VO_CHECK_HIP(ctx, expr)                                                            \
  do {                                                                                     \
    hipError_t _e = (expr);                                                                \
    if (_e != hipSuccess) {                                                                \
      snprintf((ctx)->err, sizeof((ctx)->err), "%s:%d: %s -> %s", __FILE__, __LINE__, #expr, \
               hipGetErrorString(_e));                                                     \
      return VO_ERR_HIP;                                                                   \
    }                                                                                      \
  } while (0)

#define VO_FAIL(ctx, code, ...)                                \
  do {                                                         \
    snprintf((ctx)->err, sizeof((ctx)->err), __VA_ARGS__);     \
    return (code);                                             \
  } while (0)

// The entry points without a remap take u8 planes only (vo_set_input_format).
#define VO_NEED_MONO8(ctx, name)                                                                                      \
  do {                                                                                                               \
    if ((ctx)->input_format != VO_PIX_MONO8)                                                                          \
      VO_FAIL(ctx, VO_ERR_INVALID,                                                                                   \
              name ": the context's input format is not VO_PIX_MONO8 and this entry point does not convert; use the " \
                   "rectifying entry points (identity maps via vo_rectify_set_maps for undistorted data)");          \
  } while (0)

// A call needs pyramid levels 0..eff of a slot. Fewer were built when vo_config.max_level is below the call's
// maxLevel or when vo_set_pyramid_window_hint() named a LARGER window than the call uses (a larger window stops
// the pyramid earlier): tracking with fewer levels than cv::buildOpticalFlowPyramid would build diverges from the
// reference, so it is an error, not a clamp.
#define VO_NEED_LEVELS(ctx, P, eff)                                                                                  \
  do {                                                                                                               \
    if ((eff) > (P).n_levels - 1)                                                                                    \
      VO_FAIL(ctx, VO_ERR_INVALID,                                                                                   \
              "the slot's pyramid holds levels 0..%d, this call needs 0..%d: raise vo_config.max_level, or give "    \
              "vo_set_pyramid_window_hint the SMALLEST window in use",                                               \
              (P).n_levels - 1, (eff));                                                                              \
  } while (0)

// Work about to be enqueued on c->stream reads the pyramid of `slot`: order it behind the slot's last build if that
// ran on the other stream (one hipStreamWaitEvent per build and stream, nothing when both are the same stream).
static inline int vo_slot_acquire(vo_ctx *c, int slot) {
  vo_pyramid &P = c->slots[slot];
  const int k = c->stream == c->stream2 ? 1 : 0;
  if (!P.seen[k]) {
    VO_CHECK_HIP(c, hipStreamWaitEvent(c->stream, P.ready, 0));
    P.seen[k] = 1;
  }
  return VO_OK;
}

// Work about to be enqueued on c->stream reads the slot's ignore mask: the view (p == null without a mask), ordered behind the
// mask's last write if that ran on the other stream.
static inline int vo_slot_mask_acquire(vo_ctx *c, int slot, vo_mask_view *v) {
  v->p = nullptr;
  v->stride = v->w = v->h = 0;
  if (slot < 0 || slot >= c->cfg.n_slots) return VO_OK;
  vo_pyramid &P = c->slots[slot];
  if (!P.mask_on || !P.mask) return VO_OK;
  const int k = c->stream == c->stream2 ? 1 : 0;
  if (!P.mask_seen[k]) {
    VO_CHECK_HIP(c, hipStreamWaitEvent(c->stream, P.mask_ready, 0));
    P.mask_seen[k] = 1;
  }
  v->p = P.mask;
  v->stride = v->w = P.mask_w;
  v->h = P.mask_h;
  return VO_OK;
}
// vo_capi.hip: the slot's plane exists (the only allocation of a slot's mask) / a w x h mask copied into it on c->stream
// (src == null: the slot has no mask from here on); kind: hipMemcpyHostToDevice or hipMemcpyDeviceToDevice
int vo_slot_mask_reserve(vo_ctx *c, int slot);
int vo_slot_mask_write(vo_ctx *c, int slot, const void *src, int stride, int w, int h, hipMemcpyKind kind);
// the mask a driver (StereoVO, MonoVO) gives to the pairs it ingests (vo_capi.hip)
struct vo_driver_mask {
  uint8_t *master = nullptr;  // w x h, tightly packed
  unsigned ver = 0;           // the context-wide version of the master's content (vo_ctx::mask_ver_next; never 0 once set)
  int on = 0;
};
int vo_driver_mask_set(vo_ctx *c, vo_driver_mask *m, const int *slots, int n_slots, const void *mask, int stride, int on_device,
                       int w, int h);
int vo_driver_mask_bind(vo_ctx *c, const vo_driver_mask *m, int slot, int w, int h);  // at ingestion, before the pair's detection
void vo_driver_mask_free(vo_driver_mask *m);
// a driver takes or gives up its image slots: none of them carries a mask any longer (the planes stay allocated)
void vo_driver_mask_release_slots(vo_ctx *c, const int *slots, int n_slots);

// The ZNCC gate of a driver (vo_svo_set_zncc_gate / vo_mvo_set_zncc_gate; zncc.hip). The driver points vo_ctx::zncc_gate at its
// own state for the time its frame is in flight (enqueue .. result): the frame operators launch the kernel in front of the BA
// launch and hand the BA launch the view. pairs == 0: off.
struct vo_zncc_gate {
  int pairs = 0, win = 15, pattern = 0;
  float thres = 0.0f;
  float *d = nullptr;  // [2][cap] floats: temporal values, stereo values — the option's only allocation, at the first enable
  int cap = 0;
  int last_n = 0, last_pairs = 0;  // the last frame the kernel ran for: its input count and pairs
};
int vo_zncc_gate_set(vo_ctx *c, vo_zncc_gate *g, int pairs, int win, int pattern, float thres, bool stereo, int cap);
void vo_zncc_gate_free(vo_zncc_gate *g);
int vo_zncc_gate_get(vo_ctx *c, const vo_zncc_gate *g, float *zncc_t, float *zncc_s, int cap, int *n);
// the frame operators: the launch on c->stream (slot_r1 < 0 / pts_r1 == null: no stereo pair) and the BA launch's view
int vo_zncc_gate_enqueue(vo_ctx *c, vo_zncc_gate *g, int slot_l0, int slot_l1, int slot_r1, const float *d_pts_l0, const float *d_pts_l1,
                         const float *d_pts_r1, int n, vo_zncc_view *view);

// Semi-dense stereo depth (semidense.hip; include/vo_hip.h, "Semi-dense stereo"): the four planes of one result, the points
// list's scratch (key, idx, cnt[1]) and, from the first points call, its device outputs (pts); sized by vo_config.max_width x
// max_height. cnt[1]: the compaction's count; cnt[2 ..]: the kernel's workgroups' counts of accepted pixels (n_wg of them).
struct vo_sd_buffers {
  float *disp = nullptr, *score = nullptr, *sigma = nullptr;
  int32_t *idx = nullptr;
  uint8_t *status = nullptr, *key = nullptr;
  int *cnt = nullptr;
  float *pts = nullptr;
  size_t npix = 0, n_wg = 0;
};
int vo_sd_buffers_alloc(vo_ctx *c, vo_sd_buffers *b);
void vo_sd_buffers_free(vo_sd_buffers *b);
void vo_semidense_free(vo_ctx *c);
// the launch on c->stream, into device planes (any may be null); wg_accepted (device, may be null): a count per workgroup
int vo_sd_enqueue(vo_ctx *c, int slot_l, int slot_r, const vo_semidense_params *p, float *disp, float *score, float *sigma, uint8_t *status,
                  int *wg_accepted, int *W_out, int *H_out);

int vo_sd_ctx_buffers(vo_ctx *c, vo_sd_buffers **b);  // the context's own buffers, made on first use
int vo_sd_points_alloc(vo_ctx *c, vo_sd_buffers *b);  // the points list's device outputs, ahead of its first call
// the points of DEVICE planes (host outputs), synchronous on c->stream; vo_sd_points_keyed: b->key is written already (the caller's rule)
int vo_sd_points(vo_ctx *c, vo_sd_buffers *b, const float *d_disp, const float *d_sigma, const uint8_t *d_status, int W, int H,
                 const float K[4], float bf, const float *T, int cap, float *xyz, float *sigma_out, uint16_t *pixel, int *n);
int vo_sd_points_keyed(vo_ctx *c, vo_sd_buffers *b, const float *d_disp, const float *d_sigma, int W, int H, const float K[4], float bf,
                       const float *T, int cap, float *xyz, float *sigma_out, uint16_t *pixel, int *n);

// Dense stereo disparity (dense_stereo.hip; include/vo_hip.h, "Dense stereo"): the workspace (two census planes and the summed
// volume, in one allocation that grows when a call needs more). A result's four planes live in a vo_sd_buffers (the u16 cost plane in
// its score plane), whose scratch the points list needs anyway.
struct vo_ds_buffers {
  void *ws = nullptr;
  size_t ws_bytes = 0;
};
void vo_ds_buffers_free(vo_ds_buffers *b);
void vo_dense_stereo_free(vo_ctx *c);
// the launches on c->stream, into device planes (any may be null)
int vo_ds_enqueue(vo_ctx *c, vo_ds_buffers *b, int slot_l, int slot_r, const vo_dense_stereo_params *p, float *disp, uint16_t *cost, float *sigma,
                  uint8_t *status, int *W_out, int *H_out);

// The speckle filter for disparity planes (dense_speckle.hip; include/vo_hip.h, "Speckle filter"): the workspace — the counters, the
// label plane and the size plane in one allocation that grows when a call needs more.
struct vo_spk_buffers {
  void *ws = nullptr;
  size_t ws_bytes = 0;
};
int vo_spk_reserve(vo_ctx *c, vo_spk_buffers *b, int W, int H);
void vo_spk_buffers_free(vo_spk_buffers *b);
void vo_speckle_free(vo_ctx *c);
int vo_spk_check_params(vo_ctx *c, const vo_speckle_params *p);
int32_t *vo_spk_label(const vo_spk_buffers *b);
int32_t *vo_spk_size(const vo_spk_buffers *b, int W, int H);
int *vo_spk_counters(const vo_spk_buffers *b);  // [0] n_removed, [1] n_components
// the four launches on c->stream, in place on DEVICE planes (sigma may be null); b holds the shape (vo_spk_reserve)
int vo_spk_enqueue(vo_ctx *c, vo_spk_buffers *b, float *disp, float *sigma, uint8_t *status, int W, int H, const vo_speckle_params *p);

// The map merge (semidense_map_merge.hip; include/vo_hip.h, "Semi-dense map merge"): the launch on `s` over DEVICE planes (the map's
// three null together: no map; origin and counts may be null; counts — 6 device words — is zeroed on `s` in front of the launch)
void vo_semidense_merge_free(vo_ctx *c);
int vo_sdm_check_params(vo_ctx *c, const vo_semidense_map_merge_params *p);
int vo_sdm_enqueue(vo_ctx *c, hipStream_t s, const float *m_invd, const float *m_sigma, const uint8_t *m_n_obs, const float *disp,
                   const float *sigma_invd, const uint8_t *status, int W, int H, float bf, const vo_semidense_map_merge_params *p, float *invd,
                   float *sigma, uint8_t *n_obs, uint8_t *origin, unsigned long long *counts);

// The temporal semi-dense search (semidense_temporal.hip; include/vo_hip.h, "Semi-dense temporal"): a key plane, the four planes of a
// map and — the context's operator — the score plane or — a driver's option — the keyframe's ignore mask: one allocation sized by
// vo_config.max_width x max_height.
struct vo_sdt_buffers {
  float *invd = nullptr, *sigma = nullptr, *score = nullptr;
  uint8_t *n_obs = nullptr, *tstatus = nullptr, *key = nullptr, *mask = nullptr;
  size_t npix = 0;
  void *base = nullptr;  // the allocation (a driver's propagation swaps the map's four planes with those of its own set)
};
int vo_sdt_buffers_alloc(vo_ctx *c, vo_sdt_buffers *b, bool driver);
void vo_sdt_buffers_free(vo_sdt_buffers *b);
void vo_semidense_temporal_free(vo_ctx *c);
int vo_sdt_ctx_buffers(vo_ctx *c, vo_sdt_buffers **b);  // the context's own buffers, made on first use
// the launch on c->stream: a DEVICE key plane against the slot's level-0 plane, the map's DEVICE planes updated in place; key_mask:
// the key pixels' ignore mask (p == null: none), null: the one bound to slot_cur
int vo_sdt_enqueue(vo_ctx *c, const uint8_t *d_key, int key_stride, const vo_mask_view *key_mask, int slot_cur, const float K[4],
                   const float T_ck[16], const vo_semidense_temporal_params *p, float *invd, float *sigma, uint8_t *n_obs, uint8_t *tstatus,
                   float *score);
// the pixels with n_obs >= min_obs of DEVICE planes as a list (host outputs); b: the compaction's scratch. Synchronous on c->stream.
int vo_sdt_points(vo_ctx *c, vo_sd_buffers *b, const float *d_invd, const float *d_sigma, const uint8_t *d_n_obs, int W, int H, const float K[4],
                  const float *T, int min_obs, int cap, float *xyz, float *sigma_out, uint16_t *pixel, int *n);

// The semi-dense propagation (semidense_propagate.hip; include/vo_hip.h, "Semi-dense propagation"): the plane of keys (all 0 between
// calls: zeroed at allocation, every resolve launch stores 0 back), a set of map planes, origin and — the context's operator — src:
// one allocation sized by vo_config.max_width x max_height.
struct vo_sdp_buffers {
  void *base = nullptr;
  unsigned long long *keys = nullptr;
  float *invd = nullptr, *sigma = nullptr;
  int32_t *src = nullptr;
  uint8_t *n_obs = nullptr, *tstatus = nullptr, *origin = nullptr;
  size_t npix = 0;
};
int vo_sdp_buffers_alloc(vo_ctx *c, vo_sdp_buffers *b, bool driver);
void vo_sdp_buffers_free(vo_sdp_buffers *b);
void vo_semidense_propagate_free(vo_ctx *c);

// The semi-dense regularisation (semidense_regularize.hip; include/vo_hip.h, "Semi-dense regularisation"): the four planes of a
// regularised map and — the context's operator — a copy of the caller's mask: one allocation sized by vo_config.max_width x
// max_height.
struct vo_sdr_buffers {
  void *base = nullptr;
  float *invd = nullptr, *sigma = nullptr;
  uint8_t *n_obs = nullptr, *rstatus = nullptr, *mask = nullptr;
  size_t npix = 0;
};
int vo_sdr_buffers_alloc(vo_ctx *c, vo_sdr_buffers *b, bool driver);
void vo_sdr_buffers_free(vo_sdr_buffers *b);
void vo_semidense_regularize_free(vo_ctx *c);

// The semi-dense alignment (semidense_align.hip; include/vo_hip.h, "Semi-dense alignment"): the small state block (pose, status, the
// "done" word and the ticket, zero between launches; the last evaluated system) and a row of 30 integer sums per block of 1024
// raster indices: one allocation sized by vo_config.max_width x max_height.
struct vo_sda_buffers {
  void *base = nullptr, *state = nullptr;
  long long *partial = nullptr;
  size_t n_blocks = 0;
};
int vo_sda_buffers_alloc(vo_ctx *c, vo_sda_buffers *b);
void vo_sda_buffers_free(vo_sda_buffers *b);
void vo_semidense_align_free(vo_ctx *c);
// max_iters launches on c->stream, back to back: a DEVICE key plane and the map's DEVICE planes against the slot's level-0 plane
int vo_sda_enqueue(vo_ctx *c, vo_sda_buffers *b, const uint8_t *d_key, int key_stride, int slot_cur, const float K[4], const float T_ck[16],
                   const vo_semidense_align_params *p, const float *invd, const float *sigma, const uint8_t *n_obs);
// The coarse-to-fine alignment (include/vo_hip.h, "Semi-dense alignment on a map pyramid"): levels 1..5 of a map and, for a driver,
// of the keyframe's left image, tight planes in one allocation sized by vo_config.max_width x max_height ([0] stays null).
struct vo_sdm_pyramid {
  void *base = nullptr;
  float *invd[6] = {}, *sigma[6] = {};
  uint8_t *n_obs[6] = {}, *key[6] = {};
};
int vo_sdm_pyramid_alloc(vo_ctx *c, vo_sdm_pyramid *py, bool with_key);
void vo_sdm_pyramid_free(vo_sdm_pyramid *py);
// levels - 1 launches on c->stream: level l of the map (DEVICE planes, [0] the w x h level 0) from level l - 1, l = 1 .. levels - 1
int vo_sdm_enqueue(vo_ctx *c, int w, int h, int levels, float *const invd[], float *const sigma[], uint8_t *const n_obs[]);
// per level, from levels - 1 down, its iterations' launches on c->stream: DEVICE planes per level ([l]: the key's level with its
// stride, the map's level) against the slot's pyramid. first: SDA_FIRST_CALL or SDA_FIRST_PREV (semidense_align_device.hpp)
int vo_sda_enqueue_pyr(vo_ctx *c, vo_sda_buffers *b, const uint8_t *const key[], const int key_stride[], int slot_cur, const float K[4],
                       const float T_ck[16], const vo_semidense_align_pyr_params *p, const float *const invd[], const float *const sigma[],
                       const uint8_t *const n_obs[], int first);
// The alignment with affine brightness (include/vo_hip.h, "Semi-dense alignment with affine brightness"): a state block of its own
// kind and 47 sums per block in a vo_sda_buffers of its own; the launches of vo_sda_enqueue_pyr with that block's kernel (levels = 1
// with the key plane as key[0]: the level-0 operator).
int vo_sdaa_buffers_alloc(vo_ctx *c, vo_sda_buffers *b);
int vo_sdaa_enqueue_pyr(vo_ctx *c, vo_sda_buffers *b, const uint8_t *const key[], const int key_stride[], int slot_cur, const float K[4],
                        const float T_ck[16], const vo_semidense_align_pyr_params *p, const vo_semidense_affine_params *ap,
                        const float *const invd[], const float *const sigma[], const uint8_t *const n_obs[], int first);

// Image ingestion (H2D + pyramid chain) enqueues on the side stream when vo_set_ingest_side_stream is on: launchers
// use c->stream, which this scope points at the ingest stream and restores on exit.
struct vo_ingest_scope {
  vo_ctx *c;
  hipStream_t saved;
  explicit vo_ingest_scope(vo_ctx *ctx) : c(ctx), saved(ctx->stream) {
    if (c->ingest_side && c->stream == c->stream_main) c->stream = c->stream2;
  }
  ~vo_ingest_scope() { c->stream = saved; }
};

// The cumulative hand-shake targets (features past pass 1, finished fallback workgroups, candidate workgroups, DLT workers)
// grow by a few thousand per frame for the life of a stream and are compared by wrapped difference on the device; on the
// host they wrap the same way — through unsigned arithmetic, a signed `+=` would be undefined behaviour after ~5e5 frames.
static inline void vo_wrap_add(int &x, int n) { x = (int)((unsigned)x + (unsigned)n); }

// ---- profiling brackets (no-ops unless vo_profile_enable was called) --------
static inline void vo_prof_begin(vo_ctx *c, int cls) {
  c->prof_open = 0;
  if (c->prof && c->prof_n < c->prof_cap && (!c->prof_mask || (c->prof_mask & (1u << cls)))) {
    c->prof[c->prof_n].cls = cls;
    (void)hipEventRecord(c->prof[c->prof_n].a, c->stream);
    c->prof_open = 1;
  }
}
static inline void vo_prof_end(vo_ctx *c) {
  if (c->prof_open) {
    (void)hipEventRecord(c->prof[c->prof_n].b, c->stream);
    ++c->prof_n;
    c->prof_open = 0;
  }
}

#ifdef __HIPCC__
// ---- DPP cross-lane helpers ---------------------------------------------------
// dpp_ctrl: quad_perm [1,0,3,2] = 0xB1, quad_perm [2,3,0,1] = 0x4E,
//           row_half_mirror = 0x141, row_mirror = 0x140.
template <int CTRL>
__device__ __forceinline__ float dpp_f32(float v) {
  return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, 0xF, 0xF, true));
}
template <int CTRL>
__device__ __forceinline__ int dpp_i32(int v) {
  return __builtin_amdgcn_update_dpp(0, v, CTRL, 0xF, 0xF, true);
}

// Sum over the 64 lanes; every lane returns the same bits.
// Tree: ((l0+l1)+(l2+l3)) ... within rows of 16 (quad_perm, half_mirror, mirror), then
// row_bcast15 (rows 1,3 += previous row), row_bcast31 (rows 2,3 += row 1) and one readlane(63):
// (r3+r2)+(r1+r0), the same additions as the balanced tree (r0+r1)+(r2+r3) since + commutes.
__device__ __forceinline__ float wave_sum_f32(float v) {
  v = v + dpp_f32<0xB1>(v);
  v = v + dpp_f32<0x4E>(v);
  v = v + dpp_f32<0x141>(v);
  v = v + dpp_f32<0x140>(v);
  v = v + __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x142, 0xA, 0xF, false));
  v = v + __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x143, 0xC, 0xF, false));
  return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), 63));
}
// Four independent sums, stepped together so that each DPP's wait states are filled by the other
// three chains (a lone wavefront otherwise stalls on every dependent DPP). Same tree as wave_sum_f32.
__device__ __forceinline__ void wave_sum4_f32(float &a, float &b, float &c, float &d) {
#define VO_STEP4(CTRL)                                    \
  {                                                       \
    const float ta = dpp_f32<CTRL>(a), tb = dpp_f32<CTRL>(b), tc = dpp_f32<CTRL>(c), td = dpp_f32<CTRL>(d); \
    a = a + ta;                                           \
    b = b + tb;                                           \
    c = c + tc;                                           \
    d = d + td;                                           \
  }
  VO_STEP4(0xB1)
  VO_STEP4(0x4E)
  VO_STEP4(0x141)
  VO_STEP4(0x140)
#undef VO_STEP4
#define VO_BC4(CTRL, RM)                                                                                   \
  {                                                                                                        \
    const float ta = __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, a), CTRL, RM, 0xF, false)); \
    const float tb = __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, b), CTRL, RM, 0xF, false)); \
    const float tc = __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, c), CTRL, RM, 0xF, false)); \
    const float td = __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, d), CTRL, RM, 0xF, false)); \
    a = a + ta;                                                                                            \
    b = b + tb;                                                                                            \
    c = c + tc;                                                                                            \
    d = d + td;                                                                                            \
  }
  VO_BC4(0x142, 0xA)
  VO_BC4(0x143, 0xC)
#undef VO_BC4
  a = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, a), 63));
  b = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, b), 63));
  c = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, c), 63));
  d = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, d), 63));
}
__device__ __forceinline__ int wave_sum_i32(int v) {
  v = v + dpp_i32<0xB1>(v);
  v = v + dpp_i32<0x4E>(v);
  v = v + dpp_i32<0x141>(v);
  v = v + dpp_i32<0x140>(v);
  v = v + __builtin_amdgcn_update_dpp(0, v, 0x142, 0xA, 0xF, false);
  v = v + __builtin_amdgcn_update_dpp(0, v, 0x143, 0xC, 0xF, false);
  return __builtin_amdgcn_readlane(v, 63);
}
__device__ __forceinline__ void wave_sum4_i32(int &a, int &b, int &c, int &d) {
#define VO_STEP4I(CTRL)                                                                       \
  {                                                                                           \
    const int ta = dpp_i32<CTRL>(a), tb = dpp_i32<CTRL>(b), tc = dpp_i32<CTRL>(c), td = dpp_i32<CTRL>(d); \
    a += ta;                                                                                  \
    b += tb;                                                                                  \
    c += tc;                                                                                  \
    d += td;                                                                                  \
  }
  VO_STEP4I(0xB1)
  VO_STEP4I(0x4E)
  VO_STEP4I(0x141)
  VO_STEP4I(0x140)
#undef VO_STEP4I
#define VO_BC4I(CTRL, RM)                                                  \
  {                                                                        \
    const int ta = __builtin_amdgcn_update_dpp(0, a, CTRL, RM, 0xF, false); \
    const int tb = __builtin_amdgcn_update_dpp(0, b, CTRL, RM, 0xF, false); \
    const int tc = __builtin_amdgcn_update_dpp(0, c, CTRL, RM, 0xF, false); \
    const int td = __builtin_amdgcn_update_dpp(0, d, CTRL, RM, 0xF, false); \
    a += ta;                                                               \
    b += tb;                                                               \
    c += tc;                                                               \
    d += td;                                                               \
  }
  VO_BC4I(0x142, 0xA)
  VO_BC4I(0x143, 0xC)
#undef VO_BC4I
  a = __builtin_amdgcn_readlane(a, 63);
  b = __builtin_amdgcn_readlane(b, 63);
  c = __builtin_amdgcn_readlane(c, 63);
  d = __builtin_amdgcn_readlane(d, 63);
}
// two exact (float)(int64 sum) at once: 16/16 split of both partials, one interleaved 4-way butterfly
__device__ __forceinline__ void wave_sum2_i32_to_f32(int p, int q, float &fp, float &fq) {
  // When every lane's partials are below 2^25 in magnitude (the usual case) the 64-lane sums fit int32: two chains
  // instead of four, and (float)(int32) rounds once exactly like (float)(int64).
  if (__builtin_expect(!__any((((unsigned)p + (1u << 25)) | ((unsigned)q + (1u << 25))) >> 26), 1)) {
#define VO_STEP2I(EXPR_P, EXPR_Q) \
  {                               \
    const int tp = EXPR_P, tq = EXPR_Q; \
    p += tp;                      \
    q += tq;                      \
  }
    VO_STEP2I(dpp_i32<0xB1>(p), dpp_i32<0xB1>(q))
    VO_STEP2I(dpp_i32<0x4E>(p), dpp_i32<0x4E>(q))
    VO_STEP2I(dpp_i32<0x141>(p), dpp_i32<0x141>(q))
    VO_STEP2I(dpp_i32<0x140>(p), dpp_i32<0x140>(q))
    VO_STEP2I(__builtin_amdgcn_update_dpp(0, p, 0x142, 0xA, 0xF, false), __builtin_amdgcn_update_dpp(0, q, 0x142, 0xA, 0xF, false))
    VO_STEP2I(__builtin_amdgcn_update_dpp(0, p, 0x143, 0xC, 0xF, false), __builtin_amdgcn_update_dpp(0, q, 0x143, 0xC, 0xF, false))
#undef VO_STEP2I
    fp = (float)__builtin_amdgcn_readlane(p, 63);
    fq = (float)__builtin_amdgcn_readlane(q, 63);
    return;
  }
  int plo = p & 0xFFFF, phi = p >> 16, qlo = q & 0xFFFF, qhi = q >> 16;
  wave_sum4_i32(plo, phi, qlo, qhi);
  fp = (float)((double)phi * 65536.0 + (double)plo);
  fq = (float)((double)qhi * 65536.0 + (double)qlo);
}
// three at once: six interleaved chains (16/16 halves of p, q, r), same butterfly
__device__ __forceinline__ void wave_sum3_i32_to_f32(int p, int q, int r, float &fp, float &fq, float &fr) {
  int v[6] = {p & 0xFFFF, p >> 16, q & 0xFFFF, q >> 16, r & 0xFFFF, r >> 16};
#define VO_STEP6(CTRL)                                      \
  {                                                         \
    int t[6];                                               \
    _Pragma("unroll") for (int k = 0; k < 6; ++k) t[k] = dpp_i32<CTRL>(v[k]); \
    _Pragma("unroll") for (int k = 0; k < 6; ++k) v[k] += t[k];               \
  }
  VO_STEP6(0xB1)
  VO_STEP6(0x4E)
  VO_STEP6(0x141)
  VO_STEP6(0x140)
#undef VO_STEP6
#pragma unroll
  for (int k = 0; k < 6; ++k) v[k] += __builtin_amdgcn_update_dpp(0, v[k], 0x142, 0xA, 0xF, false);
#pragma unroll
  for (int k = 0; k < 6; ++k) v[k] += __builtin_amdgcn_update_dpp(0, v[k], 0x143, 0xC, 0xF, false);
#pragma unroll
  for (int k = 0; k < 6; ++k) v[k] = __builtin_amdgcn_readlane(v[k], 63);
  fp = (float)((double)v[1] * 65536.0 + (double)v[0]);
  fq = (float)((double)v[3] * 65536.0 + (double)v[2]);
  fr = (float)((double)v[5] * 65536.0 + (double)v[4]);
}
// Exact 64-bit sum of 64 int32 lane values (each |v| < 2^30): split 16/16 so the
// two int32 wave sums cannot overflow, recombine in int64.
__device__ __forceinline__ long long wave_sum_i32_to_i64(int v) {
  int lo = v & 0xFFFF;
  int hi = v >> 16;
  int slo = wave_sum_i32(lo);
  int shi = wave_sum_i32(hi);
  return (long long)shi * 65536LL + (long long)slo;
}
// (float)(exact int64 sum): the sum is < 2^53, so hi*65536 + lo is exact in double and the
// double -> float conversion rounds once, exactly like (float)(int64_t).
__device__ __forceinline__ float wave_sum_i32_to_f32(int v) {
  int lo = v & 0xFFFF;
  int hi = v >> 16;
  int slo = wave_sum_i32(lo);
  int shi = wave_sum_i32(hi);
  return (float)((double)shi * 65536.0 + (double)slo);
}

__device__ __forceinline__ int reflect101_dev(int p, int n) { return vo_reflect101(p, n); }
#endif  // __HIPCC__

