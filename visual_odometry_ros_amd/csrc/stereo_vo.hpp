// stereo_vo.hpp — state of the StereoVO driver (stereo_vo.hip, stereo_vo_lba.hip)
#pragma once
#include <vector>

#include "pose_covariance.hpp"
#include "svo_device.hpp"
#include "vo_internal.hpp"
#include "vo_kernels.hpp"

// Keyframe-centric storage of what the reference keeps per landmark (getObservationsOnKeyframes / getRelatedKeyframePtr):
// a keyframe holds its related landmarks' ids and both pixels. The ids of a track set are ASCENDING and dense (survivors
// keep their order, new landmarks get the next ids and are appended), so every container is a direct-address array.
struct SvoKeyframe {
  int serial, frame_id;
  float T_wc[16];
  // the keyframe's related landmarks live in slot `ring` of the device-side keyframe ring (ids, pixels)
  int ring = 0, n = 0, id_min = 0;  // entries, smallest (= first) landmark id
  int global = 0;                   // index among all keyframes of the stream (stats_keyframe)
};

// vo_svo_set_semidense (semidense.hip): the option's state. One result at most is in flight: `done` is recorded behind its launch on
// the side stream; an ingestion that reuses a slot the launch reads is ordered behind `done` on the device (guard).
struct vo_svo_semidense {
  bool on = false, have = false;
  unsigned busy = 0;  // slots (bits) a launch has read since the last guard wait
  int every = 0;
  vo_semidense_params prm = {};
  vo_sd_buffers buf;
  hipEvent_t fork = nullptr, done = nullptr;
  int slot_l = -1, slot_r = -1, w = 0, h = 0, frame_id = -1;
  float T_wc[16] = {};
};

// vo_svo_set_dense_stereo (dense_stereo.hip): the option's state, with the rules of vo_svo_semidense and events of its own. `buf`:
// the result's planes (cost in the score plane) and the points list's scratch; `ws`: the workspace. Both made at the first enable.
struct vo_svo_dense_stereo {
  bool on = false, have = false;
  unsigned busy = 0;
  int every = 0;
  vo_dense_stereo_params prm = {};
  vo_ds_buffers ws;
  vo_sd_buffers buf;
  hipEvent_t fork = nullptr, done = nullptr;
  int w = 0, h = 0, frame_id = -1;
  float T_wc[16] = {};
  // vo_svo_set_dense_speckle (dense_speckle.hip): the filter behind the decision, in place on `buf`; `spk`: its label and size planes
  // and counters, made at the first enable; spk_have: the last result went through it
  bool spk_on = false, spk_have = false;
  vo_speckle_params spk_prm = {};
  vo_spk_buffers spk;
};

// vo_svo_set_semidense_temporal (semidense_temporal.hip): the last keyframe's left plane and its map. The launches run on the side
// stream behind the static option's, one after the other (the map needs no second copy), and share its events: `sd.done` is
// recorded behind each, `sd.busy` takes the current left slot.
struct vo_svo_semidense_temporal {
  bool on = false, have = false, mask_on = false;  // switched on; a keyframe has seeded the map; that keyframe carried a mask (buf.mask)
  vo_semidense_temporal_params prm = {};
  vo_sdt_buffers buf;
  int w = 0, h = 0, frame_id = -1, n_fused = 0;
  int kf_index = -1;  // the keyframe's index among all keyframes of the stream (kf_all)
  float T_wk[16] = {};
};

// vo_svo_set_semidense_propagate (semidense_propagate.hip): at a keyframe the temporal option's map is warped into the new keyframe
// and fused with its static result instead of being seeded afresh. `buf` holds the keys, the map's other set of planes (resolve
// reads the old map while it writes the new one; the sets are swapped behind it) and origin. chain: the map on the device has been
// written by a keyframe since the option was switched on, so the next keyframe has a predecessor.
struct vo_svo_semidense_propagate {
  bool on = false, chain = false;
  vo_semidense_propagate_params prm = {};
  vo_sdp_buffers buf;
  int from_frame_id = -1;
  float T_ba[16] = {};
};

// vo_svo_set_semidense_regularize (semidense_regularize.hip): behind every launch that writes the temporal option's map one launch
// writes a regularised copy into `buf`; the map itself is never touched. have: `buf` holds the regularised map of the keyframe
// frame_id after n_fused temporal launches.
struct vo_svo_semidense_regularize {
  bool on = false, have = false;
  vo_semidense_regularize_params prm = {};
  vo_sdr_buffers buf;
  int w = 0, h = 0, frame_id = -1, n_fused = 0;
  float T_wk[16] = {};
};

// vo_svo_set_semidense_world (semidense_world.hip): the outgoing keyframe's map goes into a world-frame voxel table when the next
// keyframe replaces it (or at vo_svo_semidense_world_flush). done: the current keyframe's map is in the table already.
struct vo_svo_semidense_world {
  bool on = false, done = false;
  int source = 0;
  struct vo_semidense_world *wm = nullptr;
  // vo_svo_set_semidense_world_carve: every integration of a keyframe's map is followed by the carve of the same planes
  bool carve_on = false;
  vo_semidense_world_carve_params carve = {};
  // vo_svo_set_semidense_world_reanchor: the planes of every map integrated while its keyframe sits in the local BA's
  // window are kept in a ring on the device, so that the map can be taken out of the table and put back where the BA moves the
  // keyframe. An anchor per integrated keyframe: `live` those whose keyframe is in the window (kf_window at most, each with a ring
  // place; what the pass and the retaining walk), `frozen` the record of those that have left it (slot -1; 88 bytes per keyframe of
  // the stream, like kf_all; only the anchors getter reads it). Each list is in integration order (`order`); the getter merges them.
  // log: the pairs enqueued since the counters were last read, with the pose each replaced — a refused pair (the device decides) is
  // taken back then.
  struct Anchor {
    int frame_id, kf_index, slot, w, h;
    int order;       // its place among the integrations since the table was last cleared
    float T_wk[16];  // the pose the map is in the table with ("applied")
  };
  struct Pair {
    int frame_id;  // the anchor's
    float T_prev[16];
  };
  struct {
    bool on = false;
    double min_move = 0.0;  // [voxels]
    void *ring = nullptr;   // n_slots x (invd f32, sigma f32, n_obs u8, key u8) at max_width x max_height
    int n_slots = 0;
    size_t np_max = 0;
    std::vector<Anchor> live, frozen;
    std::vector<Pair> log;
    unsigned long long refused_seen = 0;  // refused_removals when the log was last settled
    int n_anchors = 0;                    // anchors recorded since the table was last cleared
  } ra;
  // the sources VO_SEMIDENSE_WORLD_DENSE and _MERGED (semidense_map_merge.hip): `buf` — the counts, the keyframe's own
  // dense planes (copied behind its dense launches: ds_*) and the merged planes with origin, at max_width x max_height — is made at the
  // first enable of such a source; have: a merge has been enqueued, of keyframe frame_id
  struct {
    vo_semidense_map_merge_params prm = {3.0f, 2};
    void *buf = nullptr;
    size_t np_max = 0;
    bool ds_have = false, have = false;
    int ds_w = 0, ds_h = 0, ds_frame_id = -1;
    float ds_bf = 0.0f;
    int w = 0, h = 0, frame_id = -1;
  } mg;
};

// vo_svo_set_semidense_align (semidense_align.hip): at every frame that is not a keyframe the frame's left image is aligned against
// the keyframe's map, on the side stream in front of the frame's temporal launch. `have`: the last frame has a result in `buf`.
struct vo_svo_semidense_align {
  bool on = false, have = false;
  vo_semidense_align_params prm = {};
  vo_sda_buffers buf;
  int frame_id = -1, key_frame_id = -1;
  float T_wk[16] = {};
  // vo_svo_set_semidense_align_pyr: coarse to fine on the keyframe's levels (copied at the keyframe `key_levels_of`) and a map pyramid
  bool pyr = false;
  int start = 0;
  vo_semidense_align_pyr_params pprm = {};
  vo_sdm_pyramid py;
  int key_levels = 0, key_levels_of = -1;
  int prev_key = -1;  // the keyframe the PREVIOUS frame's result is against (-1: it has none)
  // vo_svo_set_semidense_align_affine: either option's launches run the kernel with affine brightness on a state block of its own
  bool affine = false;
  vo_semidense_affine_params aprm = {};
  vo_sda_buffers abuf;
};

struct vo_svo {
  vo_ctx *c = nullptr;
  vo_svo_params prm;
  int cap = 0;
  SvoTrackSet ts[2] = {};
  int cur = 0, n = 0;
  uint8_t *d_accept = nullptr;
  int *d_acc_bin = nullptr;
  SvoHdr *d_hdr = nullptr, *h_hdr = nullptr;
  int seq = 0;
  SvoCam cam;
  float T_rl[16];
  float T_wp[16], dT01[16];  // pose of the previous left frame; its getPoseDiff01()
  float kf_rot = 0.f;
  bool first = true, pending = false, pending_first = false, prefetched = false;
  const void *pre_l = nullptr, *pre_r = nullptr;
  int slot[5];
  int tab_cur = 0, tab_next = 0;
  int frame_id = 0, first_n_cand = 0;
  // keyframes
  std::vector<SvoKeyframe> keyframes;  // the window (stereo_kfs_list_)
  int n_keyframes = 0, n_kf_lms = 0;
  // landmark table, keyframe ring, window scratch and the solver's arena, all on the device (stereo_vo_lba.hip)
  struct vo_svo_lba *lba = nullptr;
  // vo_svo_set_debug_image: img_debug_ of the reference (stereo_vo.cpp:685-688), drawn on the side stream behind every frame
  struct {
    bool on = false, have = false;  // switched on; a picture has been enqueued (dbg.done says when it is there)
    vo_draw_buffers buf = {};
    hipEvent_t fork = nullptr, done = nullptr;
    int w = 0, h = 0, recoveries = 0;
  } dbg;
  // vo_svo_set_pose_covariance (MonoVO: vo_mvo_set_pose_covariance): one launch of pose_covariance.hip behind every frame's BA
  // launch, in stream order
  VoPoseCovState cov;
  vo_driver_mask mask;  // vo_svo_set_mask (MonoVO: vo_mvo_set_mask): the ignore mask the pairs ingested from now on carry
  vo_zncc_gate zncc;    // vo_svo_set_zncc_gate (MonoVO: vo_mvo_set_zncc_gate): the appearance gate of the steady-state frames
  vo_svo_semidense sd;  // vo_svo_set_semidense: semi-dense stereo depth of the keyframes' (or every frame's) own pair
  vo_svo_semidense_temporal sdt;  // vo_svo_set_semidense_temporal: the keyframe's map, fused with every later frame
  vo_svo_semidense_propagate sdp;  // vo_svo_set_semidense_propagate: that map carried over to the next keyframe
  vo_svo_semidense_align sda;  // vo_svo_set_semidense_align: every later frame's left image aligned against that map
  vo_svo_semidense_regularize sdr;  // vo_svo_set_semidense_regularize: a regularised copy of that map behind every launch that writes it
  vo_svo_semidense_world sdw;  // vo_svo_set_semidense_world: the keyframes' maps fused into one world-frame voxel table
  vo_svo_dense_stereo ds;  // vo_svo_set_dense_stereo: dense disparity of the keyframes' (or every frame's) own pair
  int mono = 0;  // the keyframe storage serves a MonoVO (mono_vo.hip): one observation per keyframe entry, bundled flags
  // all_stkeyframes_ (stats_keyframe): every keyframe's current pose (host) and where its related landmarks' ids are kept
  // on the device (a pool that only grows)
  struct SvoKfAll {
    float T_wc[16];
    int n;
    const int32_t *d_ids;
  };
  std::vector<SvoKfAll> kf_all;
  // VO_SVO_TRACE=1: where the host's time goes per frame (per StereoVO; averages on stderr every 200 frames)
  struct {
    double t_ret = 0, acc[5] = {0, 0, 0, 0, 0};  // caller between result and enqueue, enqueue, prefetch, wait in result, rest of result
    int n = 0, n_all = 0;                        // ordinary frames, all steady-state frames
  } ht;
#ifdef GN_STAMP
  double gn_acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  int gn_nacc = 0;
#endif
};

int vo_svo_lba_init(vo_svo *s);  // stereo_vo_lba.hip: landmark table, keyframe ring, window scratch, solver arena — all at construction
int vo_svo_local_ba(vo_svo *s, vo_svo_frame_info *info, int id_min);
void vo_svo_lba_free(vo_svo *s);
size_t vo_svo_lba_bytes(const vo_svo *s);
int vo_svo_lba_update_points(vo_svo *s, const SvoTrackSet &ts, int n);  // a landmark got its 3-D point outside a keyframe

int vo_svo_semidense_enqueue(vo_svo *s, int slot_l, int slot_r, int frame_id, const float T_wc[16]);  // semidense.hip
int vo_svo_semidense_guard(vo_svo *s, int a, int b);
void vo_svo_semidense_free(vo_svo *s);
int vo_svo_dense_stereo_enqueue(vo_svo *s, int slot_l, int slot_r, int frame_id, const float T_wc[16]);  // dense_stereo.hip
int vo_svo_dense_stereo_guard(vo_svo *s, int a, int b);
void vo_svo_dense_stereo_free(vo_svo *s);
int vo_svo_semidense_temporal_enqueue(vo_svo *s, int slot_l, int is_keyframe, int frame_id, const float T_wc[16]);  // semidense_temporal.hip
void vo_svo_semidense_temporal_free(vo_svo *s);
// semidense_propagate.hip, both on the side stream at a keyframe with the option on: the scatter in front of the key-plane copy
// (chain only; it reads the old map and key plane), the resolve in place of the seed (it swaps the map sets)
int vo_svo_semidense_propagate_scatter(vo_svo *s, int slot_l, const float T_wc[16]);
int vo_svo_semidense_propagate_resolve(vo_svo *s, bool chain);
void vo_svo_semidense_propagate_free(vo_svo *s);
// semidense_regularize.hip: one launch on the side stream behind the launch that wrote the map (seed, resolve or temporal)
int vo_svo_semidense_regularize_enqueue(vo_svo *s);
void vo_svo_semidense_regularize_free(vo_svo *s);
// semidense_world.hip: the current keyframe's map into the table, on the side stream, unless it is there already
int vo_svo_semidense_world_enqueue(vo_svo *s);
// (vo_svo_set_semidense_world_reanchor) behind a keyframe frame's integration, on the side stream: the window's maps follow the poses
// the local BA has just written back
int vo_svo_semidense_world_reanchor_pass(vo_svo *s);
void vo_svo_semidense_world_free(vo_svo *s);
// semidense_map_merge.hip, for the world option's sources that read the dense result: the planes' one allocation; a keyframe's dense
// planes kept (called behind the dense launches); the merge launch in front of the integration (*ok false: no dense result of the
// outgoing keyframe, nothing launched)
int vo_svo_sdm_alloc(vo_svo *s);
void vo_svo_sdm_free(vo_svo *s);
int vo_svo_sdm_keep_dense(vo_svo *s, int frame_id);
int vo_svo_sdm_merge(vo_svo *s, const float **invd, const float **sigma, const uint8_t **n_obs, bool *ok);
// semidense_align.hip: on the side stream (c->stream points at it) in front of a non-keyframe frame's temporal launch
int vo_svo_semidense_align_enqueue(vo_svo *s, int slot_l, int frame_id, const float T_ck[16]);
// (vo_svo_set_semidense_align_pyr) at a keyframe, behind the key plane's copy: the slot's coarser levels next to it
int vo_svo_semidense_align_key_levels(vo_svo *s, int slot_l, int frame_id);
void vo_svo_semidense_align_free(vo_svo *s);

void svo_mul44(const float A[16], const float B[16], float C[16]);
void svo_inv_se3(const float T[16], float Ti[16]);
