// vo_kernels.hpp — host-side launchers of the gfx950 kernels (one .hip file each).
// Every launcher only ENQUEUES on ctx->stream (no synchronisation, no allocation),
// so callers can chain them without returning to the host.
#pragma once
#include "vo_internal.hpp"

// gn_pose.hip
// frame mode of the GN launch (fused frame path): compaction prologue + result copy-out epilogue
struct vo_gn_frame {
  int n;                    // features in input index space
  const uint8_t *stage;
  const uint8_t *lm_flags;  // stereo: bit 0 = landmark triangulated (null: all are); BA set = stage 3 && triangulated
  const float *X, *pl1, *pr1;
  const float *T_pw;        // non-null: X holds WORLD points, the BA takes Xp = T_pw * X (stereo_vo.cpp:605)
  float *C_X, *C_pl1, *C_pr1;
  int32_t *C_orig;
  int *cnt;
  int *ctl;                 // null (general path): no control block to report / reset
  int ctl_words, nt_word;
  int *hdr_flags;
  const int *join_word;     // non-null: before anything else wait until *join_word has reached join_target (cumulative
  int join_target;          // count of the concurrent strict-border replay's finished workgroups; bounded wait)
  const void *res_dev;
  void *res_host;           // pinned, device-visible; null = no copy-out
  size_t res_bytes;
  int seq;                  // != 0: written to the host block's header (word seq_word) after everything else, system scope
  int seq_word;
  size_t res_late_bytes;    // leading part (header + stage bytes, multiple of 16) the GN launch itself still writes
  // mono frame (frame_mono.hip): the BA set is m1 && m2 && m3 instead of stage >= 3 (counts: m1, m1 && m2, the set),
  // and the epilogue is mono_gate_body(*mono_gate) — a MonoGateArgs, copied into the kernel arguments
  const uint8_t *m1, *m2, *m3;
  const struct MonoGateArgs *mono_gate;
  // stereo: the ignore mask of the current left image (p == null: none) — a feature is promoted to stage 4 only where the lookup
  // at its current left pixel is non-zero (the general form of the y > 660 gate). Mono: MonoGateArgs::ign.
  vo_mask_view ign;
  // stereo: the ZNCC gate's values of this frame (vo_zncc_gate_enqueue; on == 0: none) — stage 4 also needs vo_zncc_pass at the
  // feature's input index. Mono: MonoGateArgs::zn.
  vo_zncc_view zn;
  // closed step [10] (stereo): updateWeightBin(lmtrack_final.pts_l1) + the emission of the bucketed candidates of the
  // bins left empty, from the speculative per-bin results of the frame kernel
  int np_bins;              // > 0: enabled; n_bins_u * n_bins_v
  int np_bins_u, np_u_step, np_v_step;
  const uint8_t *np_has;    // [np_bins] table: the bin holds a keypoint
  const float *np_xy;       // [np_bins][2] table: its pixel
  const float *np_bin_r;    // [np_bins][2] frame kernel: forward result of the bin's candidate
  const uint8_t *np_bin_m;  // [np_bins]    frame kernel: trackBidirection mask of the bin's candidate
  float *np_out_l, *np_out_r;  // compacted, bins ascending (inside the result block)
  uint8_t *np_out_m;
  float *np_host_l, *np_host_r;  // the same places in the pinned host block (written entry by entry, not copied)
  uint8_t *np_host_m;
  const int *np_cand_done;  // VoNpArgs::cand_done / cand_target
  int np_cand_target;
  const struct VoAdvArgs *adv;   // StereoVO: the epilogue also builds the next track set (svo_device.hpp)
};
int vo_gn_enqueue(vo_ctx *c, bool stereo, bool mono_general_inverse, const float *dX, const float *dP1,
                  const float *dP2, int n, const int *d_n, const float Kl[4], const float Kr[4],
                  const float T_lr[16], float thres, int variant, const float T01_init[16],
                  float *d_Tout, uint8_t *d_mask, vo_gn_dev_info *d_info, bool write_init_on_nan = false,
                  uint8_t *d_stage = nullptr, const int32_t *d_orig = nullptr, int stage_val = 0,
                  float gate_thres = 0.f, const vo_gn_frame *frame = nullptr);

// pyramid.hip
int vo_pyr_levels_host(int w, int h, int win, int max_level);
int vo_pyramid_build(vo_ctx *c, int slot, const uint8_t *d_img, int w, int h, int stride);
int vo_pyramid_build_pair(vo_ctx *c, int slot_l, const uint8_t *d_l, int slot_r, const uint8_t *d_r, int w, int h,
                          int stride);

int vo_pyramid_build_rectified(vo_ctx *c, int slot, const uint8_t *d_img, int w, int h, int stride, int cam);
int vo_pyramid_build_pair_rectified(vo_ctx *c, int slot_l, const uint8_t *d_l, int slot_r, const uint8_t *d_r, int w,
                                    int h, int stride);

// rectify.hip
void vo_rectify_free(vo_ctx *c);

// clahe.hip
void vo_equalize_free(vo_ctx *c);
// the ingestion's hook (pyramid.hip), with equalisation on: src[i] (w x h, stride bytes per row) equalised into slots[i]'s plane on
// c->stream; eq[i] / *eq_stride: where the chain reads on. VO_ERR_SIZE for an image not larger than the tile counts.
int vo_equalize_check(vo_ctx *c, int w, int h);
int vo_equalize_enqueue(vo_ctx *c, int nimg, const int *slots, const uint8_t *const *src, int stride, int w, int h, const uint8_t **eq,
                        int *eq_stride);

// frame_pipeline.hip
bool vo_frame_in_flight(const vo_ctx *c);

// draw.hip
void vo_draw_free(vo_ctx *c);
struct vo_draw_buffers {  // what one picture needs: the index plane, the picture on the device and its pinned copy
  uint32_t *idx;
  uint8_t *img, *h_img;
  size_t img_bytes;
};
int vo_draw_buffers_alloc(vo_ctx *c, vo_draw_buffers *b);  // sized by vo_config.max_width x max_height
void vo_draw_buffers_free(vo_draw_buffers *b);
// The drivers' form of showTrackingBA(level 0 of `slot`, {}, d_pts_proj[0 .. min(*d_n, cap))): both launches and the copy into
// b->h_img on stream `st`. Points and count are DEVICE memory — the count need not be known to the host when this is enqueued.
int vo_draw_ba_enqueue(vo_ctx *c, hipStream_t st, int slot, const float *d_pts_proj, const int *d_n, int cap, vo_draw_buffers *b);
// showTrackingBA(level 0 of `slot`, d_pts[0 .. n), d_pts_proj[0 .. n)) with n = min(*d_n, cap) read on the device, drawn only
// when *d_go != 0: a skipped job writes no pixel of b->img, and the copy behind it leaves b->h_img with the bytes it had.
int vo_draw_ba_sets_enqueue(vo_ctx *c, hipStream_t st, int slot, const float *d_pts, const float *d_pts_proj, const int *d_n, int cap,
                            const int *d_go, vo_draw_buffers *b);
// showTracking(level 0 of `slot`, pts0, pts1, pts_new) from DEVICE point sets whose sizes the host knows (n1 <= n0)
int vo_draw_tracking_enqueue(vo_ctx *c, hipStream_t st, int slot, const float *d_pts0, int n0, const float *d_pts1, int n1,
                             const float *d_pts_new, int n_new, vo_draw_buffers *b);

// sba.hip
void vo_sba_free(vo_ctx *c);

// orb_detect.hip
void vo_orb_free(vo_ctx *c);
struct vo_orb_view {  // the ORB pyramid and the last detection's results on the device
  int n_levels, edge, max_out;
  const uint8_t *img[12];
  int w[12], h[12], stride[12];
  float scale[12];
  const float *xy, *resp;
  const int32_t *oct;
  const int *n_dev, *flags_dev;
};
int vo_orb_levels_enqueue(vo_ctx *c, int slot, const vo_orb_params *p, bool detect, vo_orb_view *v);
int vo_orb_check_flags(vo_ctx *c, int flags);

// orb_describe.hip
void vo_orb_describe_free(vo_ctx *c);

// klt_track.hip
int vo_klt_enqueue(vo_ctx *c, int slot0, int slot1, const float *d_pts0, const float *d_pts1_init,
                   float *d_pts1, int n_max,
                   const int *d_n, int win, int max_level, int flags, int max_iter, double eps,
                   float min_eig, uint8_t *d_status, float *d_err);
int vo_klt_mask_enqueue(vo_ctx *c, int mode, int n_max, const int *d_n, int n_cols, int n_rows,
                        float thres_err, float thres_bidir, const float *pts0, const float *pts_track,
                        const float *pts_back, const uint8_t *st_f, const uint8_t *st_b,
                        const float *err_f, const float *err_b, const uint8_t *mask_in, uint8_t *mask);

// ic_refine.hip
int vo_ic_enqueue(vo_ctx *c, int slot0, int slot1, const float *d_pts0, const float *d_scale,
                  const float *d_prior, float *d_pts_track, const uint8_t *d_mask_in, uint8_t *d_mask,
                  uint8_t *d_touched, uint8_t *d_cls, float *d_last_pu, int n_max, const int *d_n,
                  int *d_flags = nullptr, bool with_records = false);
int vo_ic_strict_enqueue(vo_ctx *c, int slot0, int slot1, const float *d_pts0, const float *d_scale,
                         const float *d_prior, float *d_pts_track, uint8_t *d_mask, uint8_t *d_touched,
                         uint8_t *d_cls, float *d_last_pu, int n_max, const int *d_n, int *d_flags = nullptr,
                         bool sequential_only = false);

// the frame kernel's view of the IC state (ic_refine.hip); IcArgs lives in ic_device.hpp
struct IcArgs;
size_t vo_ic_ctl_bytes();
int vo_ic_ctl_nt_word();
int vo_ic_frame_args(vo_ctx *c, int slot0, int slot1, IcArgs *a, int *ctl, bool with_records);
void vo_ic_strict_launch(vo_ctx *c, const IcArgs &a);

// frame_fused.hip
struct vo_frame_fused_bufs {
  float *scale, *k1, *pr_prior, *pl1, *pr1, *ref, *lastpu;
  uint8_t *stage, *m2, *touched, *cls;
  float *new_r;    // new-point candidates: forward result / mask
  uint8_t *m_new;
  const uint8_t *cand_has;  // closed step [10]: candidate j is bin j of a table, present where cand_has[j] != 0
  int *ctl;        // control block (vo_ic_ctl_bytes): error flags + replay control words
  int *sync;       // [0] features past pass 1, [1] replay workgroups finished: cumulative over the frames
  int *sync_p1_target, *sync_done_target;  // host-side running totals (updated by the enqueue)
  int conc_grid;   // concurrent replay: workgroups of the pool
  int split_cands; // phase 0 launches the features only; the candidates follow as phase 2 (behind a detection still in flight)
  int *cand_done;  // phase 2: cumulative count of finished candidate workgroups (the BA launch joins on it), or null
  int *hdr_flags;  // where the frame's error flags are reported
  float *C_X, *C_pl1, *C_pr1;
  int32_t *C_orig;
  int *cnt;
};
int vo_frame_fused_supported(int win);
int vo_frame_fused_enqueue(vo_ctx *c, const vo_stereo_params *prm, int slot_l0, int slot_l1, int slot_r1,
                           const float *d_l0, const float *d_r0, const float *d_X, const uint8_t *d_flags, int n,
                           const float T_cp[16],
                           const float T_rl[16], const float *d_new, int n_new, const vo_frame_fused_bufs &b,
                           int phase, const float *T_pw = nullptr);
// the candidate role alone, n_bins workgroups on c->stream: L1 / R1 from the two slots, results written through to
// new_r / m_new, every workgroup counts itself in cand_done
int vo_frame_fused_candidates_enqueue(vo_ctx *c, const vo_stereo_params *prm, int slot_l, int slot_r, const float *d_xy,
                                      const uint8_t *d_has, int n_bins, float *new_r, uint8_t *m_new, int *cand_done);

// misc_kernels.hip
int vo_hamming_enqueue(vo_ctx *c, const uint8_t *d_a, int na, const uint8_t *d_b, int nb, uint16_t *d_dist);
int vo_match_enqueue(vo_ctx *c, const uint8_t *d_a, int na, const uint8_t *d_b, int nb, int th_low, float ratio,
                     int32_t *d_best, uint16_t *d_bd, uint16_t *d_sd);
struct CompactArgsHost {
  const uint8_t *mask = nullptr, *alive = nullptr, *tracked = nullptr;
  const uint8_t *lm_flags = nullptr;  // drop where (lm_flags[i] & lm_reject) != 0
  int lm_reject = 0;
  int n = 0;
  const int *d_n = nullptr;
  int32_t *index_valid = nullptr;
  int *d_n_out = nullptr;
  const float *in2[4] = {nullptr, nullptr, nullptr, nullptr};
  float *out2[4] = {nullptr, nullptr, nullptr, nullptr};
  const float *in3 = nullptr;
  float *out3 = nullptr;
  const float *in1 = nullptr;
  float *out1 = nullptr;
  const int32_t *in_i = nullptr;
  int32_t *out_i = nullptr;
  uint8_t *stage = nullptr;
  int stage_val = 0;
  const float *sc_src = nullptr;
  float *sc_dst = nullptr;
  const float *gate_pts = nullptr;
  float gate_thres = 0.f;
  const uint8_t *klt_status = nullptr;
  const float *klt_err = nullptr;
  const float *klt_pts = nullptr;
  float klt_thres_err = 0.f;
  int klt_W = 0, klt_H = 0;
};
int vo_compact_enqueue(vo_ctx *c, const CompactArgsHost &h);
int vo_calc_prior_enqueue(vo_ctx *c, const float *d_pts0, int n_pts0, const float *d_Xw, int n,
                          const float T1w[16], const float K[9], float *d_out);
int vo_stereo_prior_enqueue(vo_ctx *c, const float *d_Xp, const float *d_pl0, const float *d_pr0,
                            const uint8_t *d_flags, int n,
                            const float T_cp[16], const float T_rl[16], const float Kl[4], const float Kr[4],
                            int W, int H, float *d_pl1, float *d_pr1, float *d_scale, int32_t *d_orig,
                            uint8_t *d_stage);

int vo_epi_distance_enqueue(vo_ctx *c, int mode, const float *d_pts0, const float *d_pts1, int n, const float F10[9],
                            float *d_dist);

int vo_weight_bin_update_enqueue(vo_ctx *c, const float *d_pts, int n, int u_step, int v_step, int n_bins_u,
                                 int n_bins_v, int32_t *d_weight);
int vo_bucket_argmax_enqueue(vo_ctx *c, const float *d_xy, const float *d_response, int n, float inv_u, float inv_v,
                             int n_bins_u, int n_bins_v, const int32_t *d_weight, unsigned long long *d_key,
                             float *d_pts_out, int32_t *d_idx_out, int *d_n_out, const int *d_n = nullptr,
                             const vo_mask_view *mask = nullptr);

int vo_bucket_table_enqueue(vo_ctx *c, const float *d_xy, const float *d_response, int n_max, float inv_u, float inv_v,
                            int n_bins_u, int n_bins_v, unsigned long long *d_key, float *d_tab_xy, uint8_t *d_tab_has,
                            const int *d_n, const vo_mask_view *mask = nullptr);

// orb_detect.hip: per-bin candidate tables of the closed step [10] (vo_new_point_candidates_enqueue)
struct vo_cand_table {
  float *xy;        // [n_bins][2] best keypoint of the bin (level-0 pixels)
  uint8_t *has;     // [n_bins]    the bin holds a keypoint
  int n_bins;       // 0 = never filled
  hipEvent_t ready; // recorded on the side stream behind the table's kernels and the copy of its flags
  int *h_flags;     // pinned: the detector's capacity flags of this table's detection
  int dbg_filled;   // (VO_DBG_SKIP_DETECT only)
  // The look-ahead loop tracks the table's candidates AHEAD of the frame that will use them (vo_frame_candidates_enqueue:
  // the candidate role of the frame kernel as a launch of its own on the side stream, behind the table's detection). The
  // results live with the table — the BA launch of the frame before reads the OTHER table's while these are written.
  float *new_r;     // [n_bins][2] forward result of the bin's candidate
  uint8_t *m_new;   // [n_bins]    its trackBidirection mask
  hipEvent_t tracked_ev;  // recorded on the side stream behind that launch (the stream-ordered consumers: re-issue, abandonment)
  int tracked;      // new_r / m_new hold the results described by `trk`; cleared by every detection into this table
  struct {
    int slot_l, slot_r;           // the pair's two slots and the builds of them that were read (vo_pyramid::gen)
    unsigned gen_l, gen_r;
    int win, max_level, width, height, sum_order;
    float thres_err, thres_bidir;
    int target;                   // what vo_frame_state::cand_done reads when that launch has finished (cumulative)
  } trk;
};
const vo_cand_table *vo_orb_cand_table(vo_ctx *c, int table);
vo_cand_table *vo_orb_cand_table_mut(vo_ctx *c, int table);
// the table of an image that is not (yet) a pyramid slot: `dev_img` is the image itself (device memory, `stride` bytes per row), read by
// the tile kernels on the side stream with NO wait for anything — the caller orders the side stream behind whatever fills the
// image. Returns 1 (nothing enqueued) where the tile kernels do not apply: the caller detects from the slot as usual.
int vo_set_image_host_async(vo_ctx *c, int slot, const uint8_t *host, int width, int height, int stride);  // vo_capi.hip
// mask_slot: the slot the image is on its way into — its ignore mask (vo_set_slot_mask) is the image's; < 0: none
int vo_new_point_candidates_enqueue_image(vo_ctx *c, const uint8_t *dev_img, int stride, int w, int h, const vo_bin_params *bp, int table,
                                          int mask_slot);

// frame_pipeline.hip
void vo_frame_free(vo_ctx *c);
// the candidates of table `table` (detected from slot_l) tracked slot_l -> slot_r -> slot_l on the side stream, for a pair that
// is not a frame yet; touches no per-frame state. VO_OK with nothing enqueued where the frame would not use it.
int vo_frame_candidates_enqueue(vo_ctx *c, const vo_stereo_params *prm, int slot_l, int slot_r, const vo_bin_params *bp, int table);
// the pair the table was tracked for is not going to be that table's frame: the main stream is ordered behind the launch
// (it may rebuild the slots that launch reads) and the table is no longer `tracked`
int vo_frame_candidates_abandon(vo_ctx *c, int table);
