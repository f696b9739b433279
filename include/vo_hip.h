/*
 * vo_hip.h — C ABI of libvo_hip.so, the MI355X (gfx950) implementation of the
 * per-frame visual-odometry hot path of ChanghyeonKim93/visual_odometry_ros.
 *
 * This is the drop-in boundary: plain pointers and sizes, no C++/torch types,
 * no exceptions across the ABI. Every entry point names the reference
 * interface it replaces (paths relative to the reference repository root).
 * The C++ classes in visual_odometry_ros_amd/core/visual_odometry/ (same class
 * and method names as the reference) sit directly on top of these calls; see
 * INTEGRATION.md for the reference-side binding.
 *
 * Conventions
 *  - Pixels are float pairs (x,y), row i at pts[2*i], pts[2*i+1]
 *    (cv::Point2f layout, core/defines/define_type.h:16).
 *  - 3-D points are float triples (Eigen::Vector3f layout, define_type.h:17).
 *  - Masks are one uint8_t per element (the adapter converts the reference's
 *    bit-packed std::vector<bool>, define_type.h:33).
 *  - 4x4 / 3x3 matrices are ROW-MAJOR here; Eigen::Matrix4f (PoseSE3,
 *    define_type.h:41) is column-major, the adapter transposes explicitly.
 *  - Unless a parameter is documented as a device pointer, pointers are HOST
 *    pointers; the call is synchronous at return (like the reference methods).
 *  - Return value: VO_OK (0) or a negative vo_status. vo_last_error() gives
 *    the message. Codes VO_ERR_NAN_* mirror the reference's
 *    `throw std::runtime_error` sites; VO_ERR_SIZE its size-mismatch throws.
 *  - There is NO CPU fallback: every compute entry point fails with
 *    VO_ERR_NO_DEVICE when no gfx950 device is usable.
 */
#ifndef VO_HIP_H_
#define VO_HIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VO_HIP_ABI_VERSION 3

typedef enum {
  VO_OK = 0,
  VO_ERR_INVALID = -1,    /* bad argument */
  VO_ERR_HIP = -2,        /* HIP runtime error */
  VO_ERR_NO_DEVICE = -3,  /* no usable gfx950 device */
  VO_ERR_SIZE = -4,       /* reference: throw on size mismatch (feature_tracker.cpp:283, motion_estimator.cpp:670,873) */
  VO_ERR_NAN_AXAY = -5,   /* feature_tracker.cpp:414 "ax ay nan" */
  VO_ERR_NAN_PATCH = -6,  /* feature_tracker.cpp:443,447 */
  VO_ERR_NAN_UPDATE = -7, /* feature_tracker.cpp:465 "dtu dtv nan" */
  VO_ERR_CAPACITY = -8,   /* more points / larger image than vo_config allows */
  VO_ERR_GN_FAILED = -9,  /* stereo_vo.cpp:626 "PoseOnlyStereoBA is failed!" */
  VO_ERR_LBA_NAN = -10    /* sparse_bundle_adjustment.cpp:318,:413 "In LBA, pose becomes nan!", :613, :764 "Local BA NAN!" */
} vo_status;

/* cv::OPTFLOW_USE_INITIAL_FLOW */
#define VO_KLT_USE_INITIAL_FLOW 4

/* mono GN variant: core/visual_odometry/motion_estimator.cpp:793-799 (core)
 * vs standalone/motion_estimator/motion_estimator.cpp:135 (standalone) */
#define VO_GN_VARIANT_CORE 0
#define VO_GN_VARIANT_STANDALONE 1

typedef struct vo_ctx vo_ctx;

typedef struct {
  int device;      /* HIP device ordinal */
  int max_width;   /* largest image accepted by vo_set_image */
  int max_height;
  int max_points;  /* capacity of every per-point buffer */
  int n_slots;     /* image slots (each holds an image pyramid), >= 3 for stereo */
  int max_level;   /* deepest pyramid level ever requested (OpenCV maxLevel) */
} vo_config;

typedef struct {
  int iterations;   /* GN iterations executed */
  float err;        /* last err_curr (motion_estimator.cpp:812 / :1042-1043) */
  float delta_err;
  float delta_norm; /* ||delta_xi|| of the last step */
  int cnt_invalid;  /* outliers in the last iteration */
  int is_nan;       /* pose went NaN: reference returns false, pose untouched */
} vo_gn_info;

/* ---- context ------------------------------------------------------------ */
int vo_abi_version(void);
int vo_device_count(void);
int vo_create(const vo_config *cfg, vo_ctx **out);
void vo_destroy(vo_ctx *ctx);
const char *vo_last_error(const vo_ctx *ctx);
/* hipStream_t of the context, as void* (for event timing by the caller). */
void *vo_stream(vo_ctx *ctx);
int vo_synchronize(vo_ctx *ctx);

/* Summation order of the float reductions of the IC refinement (trackWithScale: A11, A12, A22, b1, b2 and the squared
 * error over the 264 taps) and of the pose-only Gauss-Newton (the 21 + 6 entries of JtWJ / mJtWr and the error).
 * VO_SUM_ORDER_TREE (the default): per-lane or per-thread partials and a balanced tree. Exact against the oracle's
 * VO_SUM_TREE, and the fast form.
 * VO_SUM_ORDER_REFERENCE: every such sum adds its terms one after the other in the reference's order (taps in index
 * order, feature_tracker.cpp:426-458; points in order and, within a point, rows in order, motion_estimator.cpp:713-810,
 * :920-1040). The device then equals the oracle's VO_SUM_SEQ bit for bit, per operator and over free-running loops,
 * so its track ids and poses follow the reference's own float arithmetic. Cost: the sums become chains of dependent
 * adds — about 4 N adds per GN iteration for N stereo points — so a frame is several times slower (README has the
 * measured frames/s). Meant for validation runs.
 * It applies to every entry that runs IC or GN on this context: vo_track_with_scale, vo_gn_pose_mono /_stereo, the
 * stereo and mono frame operators (the _closed forms included), vo_svo_* and vo_mvo_*. The order is read when work is
 * enqueued: a change between two frames of a running stream takes effect at the next frame's enqueue. vo_batch
 * streams stay in tree order (and unequalised: vo_set_equalize is a property of a context, and a batch's contexts are
 * its own). Any other value returns VO_ERR_INVALID and changes nothing. */
enum { VO_SUM_ORDER_TREE = 0, VO_SUM_ORDER_REFERENCE = 1 };
int vo_set_sum_order(vo_ctx *ctx, int order);
int vo_get_sum_order(const vo_ctx *ctx); /* VO_SUM_ORDER_*, or VO_ERR_INVALID for a NULL context */

/* ---- images & pyramids ---------------------------------------------------
 * Replaces what cv::calcOpticalFlowPyrLK does internally on every call
 * (buildOpticalFlowPyramid: pyrDown 5-tap, REFLECT_101 borders; reference call
 * sites core/visual_odometry/feature_tracker.cpp:29,60,69,108,117,186). A slot
 * keeps its pyramid device-resident so the 4 PyrLK calls of a frame and the
 * next frame reuse it. */
int vo_set_image(vo_ctx *ctx, int slot, const uint8_t *host, int width, int height, int stride);
/* same, `dev` is a DEVICE pointer (image already resident in HBM) */
int vo_set_image_device(vo_ctx *ctx, int slot, const void *dev, int width, int height, int stride);
int vo_swap_slots(vo_ctx *ctx, int slot_a, int slot_b);
/* Both images of a stereo pair in one call (one launch per pyramid level for the pair). */
int vo_set_stereo_pair_device(vo_ctx *ctx, int slot_l, const void *dev_l, int slot_r, const void *dev_r,
                              int width, int height, int stride);
/* Image ingestion on the context's SIDE stream (on != 0): vo_set_image* / vo_set_stereo_pair* enqueue their copies
 * and pyramid chains there, concurrent with whatever the main stream runs (the frame in flight); the operators
 * that read a slot wait for it on the device. A slot may then be rebuilt only after the result of every frame that
 * read it has been collected (VO_ERR_INVALID otherwise). Default off: everything on one stream. */
int vo_set_ingest_side_stream(vo_ctx *ctx, int on);
/* Both images of a stereo pair from HOST memory without a host synchronisation (vo_set_image is synchronous):
 * asynchronous H2D + the pyramid chain on the ingest stream. Pinned host buffers give a true asynchronous copy;
 * the buffers must stay untouched until the frame that reads the slots has returned its result. */
int vo_set_stereo_pair_host_async(vo_ctx *ctx, int slot_l, const uint8_t *host_l, int slot_r, const uint8_t *host_r,
                                  int width, int height, int stride);
/* win > 0: build only levels 0..vo_pyramid_levels(w,h,win,max_level) (what PyrLK with that window
 * can use); 0 (default): every level down to vo_config.max_level. */
int vo_set_pyramid_window_hint(vo_ctx *ctx, int win);
/* effective OpenCV maxLevel for (width,height,win,max_level) */
int vo_pyramid_levels(int width, int height, int win, int max_level);
/* test hook: copy unpadded level `level` of a slot back to host (tightly packed) */
int vo_get_level(vo_ctx *ctx, int slot, int level, uint8_t *host, int *width, int *height);

/* ---- pyramidal LK -------------------------------------------------------
 * cv::calcOpticalFlowPyrLK(prev, next, prevPts, nextPts, status, err, winSize,
 * maxLevel, criteria, flags, minEigThreshold) on two slots. max_iter <= 0 and
 * eps <= 0 select what the reference's `{}` TermCriteria yields (30, 0.01).
 * pts1 is in/out when flags has VO_KLT_USE_INITIAL_FLOW. */
int vo_klt_track(vo_ctx *ctx, int slot0, int slot1, const float *pts0, float *pts1, int n,
                 int win, int max_level, int flags, int max_iter, double eps, float min_eig_thr,
                 uint8_t *status, float *err);

/* ---- FeatureTracker (core/visual_odometry/feature_tracker.h:44-104) ------ */
/* FeatureTracker::track, feature_tracker.cpp:13-37 */
int vo_track(vo_ctx *ctx, int slot0, int slot1, const float *pts0, int n, int win, int max_level,
             float thres_err, float *pts_track, uint8_t *mask_valid);
/* FeatureTracker::trackBidirection, feature_tracker.cpp:39-86 */
int vo_track_bidirection(vo_ctx *ctx, int slot0, int slot1, const float *pts0, int n, int win,
                         int max_level, float thres_err, float thres_bidirection,
                         float *pts_track, uint8_t *mask_valid);
/* FeatureTracker::trackBidirectionWithPrior, feature_tracker.cpp:88-169 (pts_track in/out) */
int vo_track_bidirection_with_prior(vo_ctx *ctx, int slot0, int slot1, const float *pts0, int n,
                                    int win, int max_level, float thres_err,
                                    float thres_bidirection, float *pts_track,
                                    uint8_t *mask_valid);
/* FeatureTracker::trackWithPrior, feature_tracker.cpp:171-206 (pts_track in/out) */
int vo_track_with_prior(vo_ctx *ctx, int slot0, int slot1, const float *pts0, int n, int win,
                        int max_level, float thres_err, float *pts_track, uint8_t *mask_valid);
/* FeatureTracker::calcPrior, feature_tracker.cpp:208-234 (K row-major 3x3, Tw1 row-major 4x4) */
int vo_calc_prior(vo_ctx *ctx, const float *pts0, int n_pts0, const float *Xw, int n,
                  const float Tw1[16], const float K[9], float *pts1_prior);
/* FeatureTracker::trackWithScale, feature_tracker.cpp:236-504, fused with the
 * cv::Sobel(ksize 3, CV_32F) pair the drivers compute first
 * (stereo_vo.cpp:549-552, mono_vo.cpp:779-782). pts_track and mask_valid are
 * in/out. strict_border != 0 reproduces the reference's never-reset tap masks
 * for points whose taps leave the image; 0 excludes such taps.
 * 1 = parallel fixed-point replay with a sequential fallback, 2 = sequential
 * replay only (validation of the fallback; same results, slower). */
int vo_track_with_scale(vo_ctx *ctx, int slot0, int slot1, const float *pts0,
                        const float *scale_est, int n, float *pts_track, uint8_t *mask_valid,
                        int strict_border);

/* ---- MotionEstimator (core/visual_odometry/motion_estimator.h:117-120) --- */
/* poseOnlyBundleAdjustment, motion_estimator.cpp:665-861. K = (fx,fy,cx,cy).
 * Returns 1 = true, 0 = false (NaN pose, R01/t01 untouched), <0 = error. */
int vo_gn_pose_mono(vo_ctx *ctx, const float *X, const float *pts1, int n, const float K[4],
                    int thres_reproj_outlier, float R01[9], float t01[3], uint8_t *mask_inlier,
                    int variant, vo_gn_info *info);
/* poseOnlyBundleAdjustment_Stereo, motion_estimator.cpp:863-1088. */
int vo_gn_pose_stereo(vo_ctx *ctx, const float *X, const float *pts_l1, const float *pts_r1,
                      int n, const float Kl[4], const float Kr[4], const float T_lr[16],
                      float thres_reproj_outlier, float T01[16], uint8_t *mask_inlier,
                      vo_gn_info *info);

/* Covariance of the pose a pose-only BA returned (the reference has no counterpart: it never fills
 * nav_msgs::Odometry::pose.covariance). Inputs: the set the BA ran on and the T01 it returned. Everything is evaluated in
 * f64 from the f32 inputs, with T10 = the SE(3) inverse of T01: the Jacobian rows of the projections under T10 <- exp(delta) T10,
 * order xi = [rho; phi] — the reference's rows for the left / mono camera (motion_estimator.cpp:976-998, :755-789); for the right
 * camera [a | Xl x a] with a = (d proj / d Xr) R_rl, the exact derivative (the reference's :1009-1031, the left-frame formula at
 * Xr, is not: DESIGN.md §13) —, the estimator's own
 * Huber weight w at that pose (a = 0.5 * sum |r| stereo, |rx| + |ry| mono; w = 1 if a < 0.5, else 0.5 / a), all n points.
 *   H      = sum_i w_i sum_rows J J^T (row-major 6x6, no (1 + lambda) factor)
 *   s2     = sum_i w_i |r_i|^2 / (rows * sum_i w_i - 6), rows = 4 stereo / 2 mono, px^2
 *   Sigma  = s2 * H^-1, or sigma_px^2 * H^-1 when sigma_px > 0: T10_true ~ exp(eps) * T10_est, eps ~ N(0, Sigma)
 *   valid  = 0 when n < 3, the denominator is <= 0, anything is non-finite or the diagonally scaled H = S H S,
 *            S = diag(H)^-1/2, is not positive definite: a pivot of its Cholesky factorisation is <= 0 up to rounding
 *            (<= 36 * 2^-53 / the smallest earlier pivot; the diagonal is 1). Sigma and s2 are then zero. The inverse is that factorisation's, unscaled.
 * The summation order is fixed: two calls give the same bits. Returns VO_OK or an error. */
int vo_gn_pose_information_stereo(vo_ctx *ctx, const float *X, const float *pts_l1, const float *pts_r1, int n,
                                  const float Kl[4], const float Kr[4], const float T_lr[16], const float T01[16],
                                  double sigma_px, double H[36], double Sigma[36], double *s2, int *valid);
int vo_gn_pose_information_mono(vo_ctx *ctx, const float *X, const float *pts1, int n, const float K[4],
                                const float R01[9], const float t01[3], double sigma_px, double H[36], double Sigma[36],
                                double *s2, int *valid);

/* geometry::se3Exp_f (core/util/geometry_library.cpp:386-440, incl. the theta < 1e-7 branch) and inverseSE3_f
 * (:554-560) exactly as the GN kernel evaluates them on the device, on their own: T = exp(xi), xi = (v, w);
 * Tinv (may be NULL) = inverseSE3_f(T). Row-major. A test hook: the estimator never needs the host to call it. */
int vo_se3_exp(vo_ctx *ctx, const float xi[6], float T[16], float Tinv[16]);

/* Epipolar gates. MotionEstimator::calcSampsonDistance(pts0, pts1, F10, out)
 * (motion_estimator.cpp:572-599) and calcSymmetricEpipolarDistance (:621-653, its per-point part):
 * F10 row-major 3x3. The camera/pose overloads (:538-570) build F10 = Kinv^T [t10]x R10 Kinv on the
 * host and call these. */
int vo_sampson_distance(vo_ctx *ctx, const float *pts0, const float *pts1, int n, const float F10[9],
                        float *dist);
int vo_symmetric_epipolar_distance(vo_ctx *ctx, const float *pts0, const float *pts1, int n,
                                   const float F10[9], float *dist);

/* ---- FeatureExtractor bucketing (the reference-owned part; cv::ORB::detect stays on the host) */
/* WeightBin::reset + update, feature_extractor.h:120-135: weight[v*n_bins_u+u] = 0 for bins that hold a
 * point (u = floor(x / u_step), only the flattened index is range-tested, as in the reference), else 1. */
int vo_weight_bin_update(vo_ctx *ctx, const float *pts, int n, int u_step, int v_step, int n_bins_u,
                         int n_bins_v, int32_t *weight);
/* The flag_nonmax_ branch of extractORBwithBinning_fast, feature_extractor.cpp:241-277: per bin with
 * weight > 0 the FIRST keypoint (detector order) of largest response; bins ascending. kp_xy / kp_response:
 * the n keypoints cv::ORB::detect returned (n <= vo_config.max_points). idx_out may be NULL. */
int vo_bucket_argmax(vo_ctx *ctx, const float *kp_xy, const float *kp_response, int n, float inv_u_step,
                     float inv_v_step, int n_bins_u, int n_bins_v, const int32_t *weight, float *pts_out,
                     int32_t *idx_out, int *n_out);

/* ---- FeatureExtractor::extractORBwithBinning_fast: detection ----------------------
 * `extractor_orb_->detect(img, fts)` (feature_extractor.cpp:241) on the image held by `slot`. cv::ORB is
 * OpenCV 4 (not in the reference tree); its detection pipeline — 8-level INTER_LINEAR_EXACT pyramid, FAST-9/16
 * with non-max suppression, runByImageBorder, retainBest on the FAST score, HarrisResponses, retainBest on the
 * Harris response, pt *= scale — is restated (oracle/oracle_orb.c says what could not be verified here).
 * Keypoints come back as level-0 pixel coordinates, Harris response and octave, ordered by level and then
 * raster order (cv's own order is unspecified). Orientation and descriptors: vo_orb_compute / vo_orb_detect_and_compute
 * below. */
typedef struct {
  int nfeatures;        /* setMaxFeatures(10000), feature_extractor.cpp:48 */
  double scale_factor;  /* 1.2 */
  int n_levels;         /* 8 */
  int edge_threshold;   /* 31 */
  int fast_threshold;   /* THRES_FAST */
} vo_orb_params;
int vo_orb_detect(vo_ctx *ctx, int slot, const vo_orb_params *prm, float *kp_xy, float *kp_response,
                  int32_t *kp_octave, int max_kp, int *n_out);
/* test hook: pyramid level >= 1 of the last detection, tightly packed */
int vo_orb_get_level(vo_ctx *ctx, int level, uint8_t *host, int *width, int *height);
/* detection + the flag_nonmax_ bucketing of feature_extractor.cpp:244-277 (vo_bucket_argmax) chained on the
 * device: only the bucketed pixels are copied back. n_detected (may be NULL) = number of keypoints before bucketing. */
int vo_extract_orb_with_binning(vo_ctx *ctx, int slot, const vo_orb_params *prm, float inv_u_step, float inv_v_step,
                                int n_bins_u, int n_bins_v, const int32_t *weight, float *pts_out, int *n_out,
                                int *n_detected);

/* The same, asynchronous: the kernels run on the context's side stream behind the last pyramid build (vo_set_image*),
 * so that the detection of an image overlaps the frame operator working on it. One detection in flight per
 * context; the image slot must stay untouched until _result() has returned. */
int vo_extract_orb_with_binning_enqueue(vo_ctx *ctx, int slot, const vo_orb_params *prm, float inv_u_step,
                                        float inv_v_step, int n_bins_u, int n_bins_v, const int32_t *weight);
int vo_extract_orb_with_binning_result(vo_ctx *ctx, float *pts_out, int *n_out, int *n_detected);

/* ---- FeatureExtractor::descriptorDistance (feature_extractor.cpp:338-357) - */
/* all-pairs 256-bit Hamming distance, dist is na x nb row-major */
int vo_orb_hamming(vo_ctx *ctx, const uint8_t *a, int na, const uint8_t *b, int nb,
                   uint16_t *dist);
/* nearest / second-nearest + the test/test_orbmatching.cpp:87-137 accept rule */
int vo_orb_match(vo_ctx *ctx, const uint8_t *a, int na, const uint8_t *b, int nb, int th_low,
                 float ratio, int32_t *best_idx, uint16_t *best_dist, uint16_t *second_dist);

/* ---- ORB orientation and descriptors: FeatureExtractor::extractAndComputeORB ----------------------------------------
 * feature_extractor.cpp:321-332: extractor_orb_->detectAndCompute(...) with the settings of initParams (:49-57: WTA_K 2,
 * patch 31, Harris score). cv::ORB::compute is OpenCV (not in the reference tree): restated here as far as it is known to
 * the author (orb.cpp ICAngles / computeOrbDescriptors, fastAtan2), unpinned like the detector; what is this library's own
 * choice is marked (own). Everything is integer arithmetic or individually rounded float operations (no fused
 * multiply-add), so a restatement written from this text reproduces the bits (csrc/orb_describe.hpp is the device text).
 *
 * For one keypoint (x, y, octave) — level-0 pixels and octave as vo_orb_detect returns them — on the ORB pyramid of the
 * image in `slot` (the detector's levels: vo_orb_get_level), with edge = vo_orb_params.edge_threshold:
 *  1. Level and centre. s = the float scale of the level ((float)pow(scale_factor, octave)); inv = 1.f / s;
 *     xf = rint(x * inv), yf = rint(y * inv) (float product, round half to even). The keypoint is VALID when
 *     0 <= octave < n_levels and edge <= xf < w - edge and edge <= yf < h - edge (float compares; w x h = the level's size).
 *     An invalid keypoint gets valid = 0, angle = 0 and 32 zero bytes (own: OpenCV drops it; the detector returns none).
 *     cx = (int)xf, cy = (int)yf. A pixel outside the level is BORDER_REFLECT_101 of the level, iterated
 *     (p < 0 -> -p, p >= n -> 2n - 2 - p, until inside).
 *  2. Orientation (ICAngles) on the unblurred level: m10 = sum u I(cx + u, cy + v), m01 = sum v I(cx + u, cy + v) over
 *     v = -15 .. 15, |u| <= umax[|v|], umax = 15 15 15 15 14 14 14 13 13 12 11 10 9 8 6 3 (integers: any order).
 *     angle = fastAtan2((float)m01, (float)m10), degrees in [0, 360), in float: K = (float)(180 / pi);
 *     p1 = 0.9997878412794807f * K, p3 = -0.3258083974640975f * K, p5 = 0.1555786518463281f * K,
 *     p7 = -0.04432655554792128f * K (each a float product); ax = |x|, ay = |y|, eps = (float)DBL_EPSILON;
 *     ax >= ay: c = ay / (ax + eps), c2 = c * c, a = (((p7 * c2 + p5) * c2 + p3) * c2 + p1) * c;
 *     else:     c = ax / (ay + eps), c2 = c * c, a = 90.f - (((p7 * c2 + p5) * c2 + p3) * c2 + p1) * c;
 *     x < 0: a = 180.f - a; then y < 0: a = 360.f - a.   steer = 0: the moments are skipped and angle = 0 (plain BRIEF).
 *  3. Smoothing: GaussianBlur(7 x 7, sigma 2, BORDER_REFLECT_101) in fixed point with the 8-bit kernel
 *     k = 18 34 49 54 49 34 18 (sum 256): B(q) = (sum_ij k_i k_j I(q + (i - 3, j - 3)) + 2^15) >> 16, for any position q,
 *     also outside the level, I being the reflected level of 1. (own where a sample leaves the level: OpenCV blurs the level
 *     only; with the reference's edge threshold 31 no sample does).
 *  4. Steered BRIEF, WTA_K 2: r = (double)(angle * (float)(pi / 180)); a = (float)cos(r), b = (float)sin(r) (double
 *     functions, rounded once). Pattern point (px, py): ix = rint(px * a - py * b), iy = rint(px * b + py * a) (float products,
 *     one float subtraction / addition). Bit j of byte i = B(c + rot(pattern[16 i + 2 j])) < B(c + rot(pattern[16 i + 2 j + 1])).
 *  5. Pattern: 512 points x (x, y), int8 in [-15, 15], pattern[2 p] = x, pattern[2 p + 1] = y of point p. OpenCV's learned
 *     table (bit_pattern_31_) is not reproduced (own). The default, vo_orb_default_pattern: entry k = 0 .. 1023 from the
 *     splitmix64 stream of the 5-point sampler (below), z = 0x4F52423331 + (k + 1) * 0x9E3779B97F4A7C15, the same three
 *     mixing lines, value = (int)(((z >> 32) * 31) >> 32) - 15. vo_orb_set_pattern replaces the table of a context (an
 *     integrator with OpenCV loads bit_pattern_31_ and gets that table's descriptors). Descriptors are comparable only
 *     between sets made with the same table and the same `steer`.
 * On an upright stereo pair steering costs recall (fewer accepted matches at equal precision): `steer` is the caller's choice.
 *
 * All calls run on the context's main stream and allocate only when a capacity grows. */
int vo_orb_default_pattern(int8_t pattern[1024]);
int vo_orb_get_pattern(vo_ctx *ctx, int8_t pattern[1024]);
/* VO_ERR_INVALID (nothing changes) when a coordinate is outside [-15, 15] */
int vo_orb_set_pattern(vo_ctx *ctx, const int8_t pattern[1024]);
/* descriptors of the caller's n keypoints on the image in `slot` (builds the slot's ORB pyramid). angle_out[n],
 * desc_out[32 n], valid_out[n]; each may be NULL. */
int vo_orb_compute(vo_ctx *ctx, int slot, const vo_orb_params *prm, const float *kp_xy, const int32_t *kp_octave, int n,
                   int steer, float *angle_out, uint8_t *desc_out, uint8_t *valid_out);
/* extractAndComputeORB: the detection of vo_orb_detect (same order, same bits) and the descriptors of all its keypoints,
 * which do not leave the device in between. `set` (0 / 1): one of two descriptor sets that stay resident on the device for
 * vo_orb_match_sets. kp_* / desc (32 bytes per keypoint) may each be NULL. */
int vo_orb_detect_and_compute(vo_ctx *ctx, int slot, const vo_orb_params *prm, int steer, int set, float *kp_xy,
                              float *kp_response, int32_t *kp_octave, float *kp_angle, uint8_t *desc, int max_kp, int *n_out);
/* vo_orb_match on two resident sets (no upload, not limited by max_points): outputs hold one entry per keypoint of set_a
 * (the n_out of its vo_orb_detect_and_compute) */
int vo_orb_match_sets(vo_ctx *ctx, int set_a, int set_b, int th_low, float ratio, int32_t *best_idx, uint16_t *best_dist,
                      uint16_t *second_dist);

/* ---- landmark mask compaction (landmark.cpp:291-332, :194-231) ----------- */
/* stable compaction indices of mask && alive && tracked; returns count in *n_out */
int vo_compact_indices(vo_ctx *ctx, const uint8_t *mask, const uint8_t *alive,
                       const uint8_t *tracked, int n, int32_t *index_valid, int *n_out);

/* ---- track IDs (landmark.h:64, landmark.cpp:6,:29; frame.h:53, frame.cpp:15,:35) ----------------
 * The reference numbers landmarks and frames with two process-global counters (inline static
 * Landmark::landmark_counter_, Frame::frame_counter_). Here every vo_ctx — one image stream — owns its pair, so the
 * streams of a batch-of-sequences process get the IDs each would get in a process of its own.
 * Both start at 0 (vo_create). */
int vo_ids_reset(vo_ctx *ctx, int32_t next_landmark_id, int32_t next_frame_id);
int vo_ids_peek(const vo_ctx *ctx, int32_t *next_landmark_id, int32_t *next_frame_id);
/* n Frame constructions in order: ids[i] = frame_counter_++. StereoFrame(cam_l, cam_r, t) is two of them, left
 * first (frame.cpp:176-180). */
int vo_ids_new_frames(vo_ctx *ctx, int n, int32_t *ids);
/* Landmark constructions for the candidates i = 0..n-1 in order, where accept[i] != 0 (NULL = all), e.g. step [10]'s
 * `mask_new[i] && Xl(2) > 0 && Xr(2) > 0` (stereo_vo.cpp:716-729): ids[i] = landmark_counter_++, -1 where rejected. */
int vo_ids_new_landmarks(vo_ctx *ctx, const uint8_t *accept, int n, int32_t *ids, int *n_created);
/* StereoLandmarkTracking(src, mask) / LandmarkTracking(src, mask) with their side effect (landmark.cpp:291-332,
 * :194-231): index_valid = stable compaction of mask && alive && tracked (as vo_compact_indices), every other
 * landmark is setUntracked() — tracked[] is in/out —, and ids_out[k] = ids[index_valid[k]] (both may be NULL). */
int vo_compact_tracks(vo_ctx *ctx, const uint8_t *mask, const uint8_t *alive, uint8_t *tracked, const int32_t *ids,
                      int n, int32_t *index_valid, int32_t *ids_out, int *n_out);

/* ---- steady-state stereo frame -------------------------------------------
 * The operator sequence of StereoVO::trackStereoImages, steps [3]-[7] and the
 * tracking part of [10] (core/visual_odometry/stereo_vo/stereo_vo.cpp:483-711),
 * chained on the device with no host round trip. */
typedef struct {
  int width, height;
  int win, max_level;
  float thres_err, thres_bidirection, thres_poseba;
  float Kl[4], Kr[4];
  float T_lr[16];
  float thres_sampson;  /* feature_tracker.thres_sampson (stereo_vo.cpp:245, :395): step [7] keeps a feature whose "distance" —
                           100 for pts_l1.y > 660, else 0 (:653-668: the epipolar distance itself is commented out in the reference) —
                           is below it. 60 in kitti_00_stereo.yaml, 0.5 in most others: the same gate; above 100 it never fires */
} vo_stereo_params;

typedef struct {
  int n_l0l1, n_refine, n_l1r1, n_inlier, n_new_ok;
  int gn_iterations;
  int n_replayed; /* strict border: features whose refinement was replayed (their IC window left the image) */
  int n_ba;       /* size of the pose-only BA set: survivors of [5] whose landmark is triangulated (stereo_vo.cpp:599) */
} vo_frame_counts;

/* flags[i] of a tracked feature in the stereo frame: bit 0 = lm->isTriangulated(); bit 1 = the landmark is no
 * longer alive or tracked (!(lm->isAlive() && lm->isTracked())): the first compaction of the frame drops it
 * whatever the tracker says (landmark.cpp:305), so it never reaches trackWithScale or the BA. */
#define VO_LM_TRIANGULATED 1
#define VO_LM_DROPPED 2
/* flags[i] in the mono frame: bit 0 = lm->isBundled(), bit 1 = member of the pose-only BA class, bit 2 = no longer
 * alive or tracked (landmark.cpp:207) */
#define VO_MONO_LM_BUNDLED 1
#define VO_MONO_LM_BA_CLASS 2
#define VO_MONO_LM_DROPPED 4

/* strict != 0: the frame's trackWithScale step replays border-touching points
 * with the reference's never-reset tap state (same as vo_track_with_scale's
 * strict_border; 2 = sequential replay only, for validation). Default 0.
 * 3 (stereo and mono frames) = the parallel replay runs on a stream of its own NEXT TO the frame kernel, as a pool of
 * resident workgroups that pick the border-touching features up as the frame kernel lists them; a dependency chain
 * starts when its members are past their first refinement instead of behind the frame kernel's last wavefront. Joined
 * on the device (no HIP event). The pool costs the frame kernel room, so it pays only when there is something to
 * replay. It needs the two queues to really run concurrently: under a tool that serialises kernels across queues
 * (rocprofv3 --pmc) its bounded waits run out; the frame is then issued again with the stream-ordered replay and the
 * context stays on it (vo_stereo_frame_recoveries).
 * 5 (stereo frame only; the mono frame takes 1) = the stream-ordered replay of mode 1, but on the replay stream behind a one-wavefront gate that
 * waits for the frame kernel's last pass 1: its (normally idle) launches run under the frame kernel's tail instead of
 * between it and the BA launch. Same conditions as 3.
 * 4 (stereo and mono frames) = 3 or 1, chosen per frame: 3 when the previous frame replayed at least 16 features and the
 * frame kernel is small enough (at most 4096 features + candidates) to leave the chip mostly idle in its second half.
 * Every non-zero value gives the same results (DESIGN.md §4.3 has the measurements). */
int vo_stereo_frame_set_strict_border(vo_ctx *ctx, int strict);

/* Frames of this context that vo_stereo_frame_result had to issue again because the device-side join of modes 3 / 5
 * timed out (the replay stream did not run next to the frame kernel: a serialising tool, a shared GPU). Such a frame
 * is re-run with the stream-ordered replay (its inputs are still on the device) and delivers the normal results; the
 * context then stays on the stream-ordered arrangement. 0 in normal operation. */
int vo_stereo_frame_recoveries(const vo_ctx *ctx);

/* ---- test / measurement hooks of one context ----------------------------------------------------------------
 * The library reads no switch from the environment (VO_SVO_TRACE, which only prints timings, is the exception); a test or
 * a measurement script sets these per context. Every value defaults to 0 = normal operation.
 *   VO_DBG_FAIL_JOIN      != 0: the device-side join of strict-border modes 3 / 5 waits for a count that never comes
 *                         (as under a tool that serialises the queues) — exercises the re-issue path
 *   VO_DBG_CONC_GRID      > 0: workgroups of the concurrent replay's pool (a pool smaller than the list)
 *   VO_DBG_SBA_LDS_SOLVE  != 0: the local BA's general dense solve (matrix in LDS) for every window size
 *   VO_DBG_SKIP_DETECT    != 0: a candidate table filled twice keeps its content (what a frame costs without the
 *                         detection under it; the results are those of a stale table)
 *   VO_OPT_POLL_YIELD     != 0: the result polls (a pinned word written last by the frame's BA launch / the local BA) give the
 *                         CPU up between looks (sched_yield) instead of spinning — for hosts where the ranks or streams
 *                         outnumber the idle cores (8 ranks on a few cores: a spinning rank keeps another one's launches waiting)
 *   VO_DBG_STAGED_DETECT  != 0: the per-bin candidate table of the closed step [10] by the per-stage detector kernels (19
 *                         launches) instead of the two tile kernels — the same table, bit for bit (tests compare the two)
 *   VO_DBG_MVO_HOST_ADVANCE != 0: MonoVO launches a frame's advance step (the next track set) from vo_mvo_result, behind the
 *                         frame's result, instead of chaining it behind the BA launch in vo_mvo_enqueue (measurement)
 *   VO_DBG_CANDS_IN_FRAME != 0: StereoVO's look-ahead loop keeps the new-point candidates of a prefetched pair inside that pair's
 *                         frame kernel instead of tracking them ahead, on the side stream, behind the pair's detection — the
 *                         same results, bit for bit (tests compare the two; the A/B lever of the measurement)
 *   VO_DBG_SBA_SPLIT      0: the local BA's steady-state iteration runs its dense solve inside the point-update launch (two
 *                         launches per iteration); 1: three launches per iteration (solve and point update apart) — the same
 *                         results, bit for bit (tests compare the two; the A/B lever of the measurement); >= 2: the fused launch
 *                         with at most that many workgroups (tests: every workgroup strides over several landmark groups)
 *   VO_DBG_SDP_STAGE      vo_semidense_map_propagate launches 1: its scatter only (the plane of keys stays as the launch leaves
 *                         it), 2: its resolve only (on the keys an earlier call left) — what each launch costs (measurement)
 *   VO_DBG_SDW_FORM       1: the world map's integrations of this context run the simple kernel form (every point probes the global
 *                         table itself) instead of the pre-aggregated one — the same table contents, bit for bit (tests compare the
 *                         two; the A/B lever of the measurement); the carves of this context run the form that is not their default,
 *                         the pre-aggregated one ("Semi-dense world map: free-space carving") */
enum { VO_DBG_FAIL_JOIN = 0, VO_DBG_CONC_GRID = 1, VO_DBG_SBA_LDS_SOLVE = 2, VO_DBG_SKIP_DETECT = 3, VO_OPT_POLL_YIELD = 4,
       VO_DBG_MVO_HOST_ADVANCE = 5, VO_DBG_STAGED_DETECT = 6, VO_DBG_CANDS_IN_FRAME = 7, VO_DBG_SBA_SPLIT = 8,
       VO_DBG_SDP_STAGE = 9, VO_DBG_SDW_FORM = 10, VO_DBG_COUNT = 11 };
int vo_debug_set(vo_ctx *ctx, int key, int value);
/* Device and pinned-host allocations made on behalf of this context so far (vo_create included). A steady-state frame —
 * keyframes and their local BA included — makes none: tests/test_stereo_vo_gpu.py asserts it. */
int vo_debug_allocation_count(const vo_ctx *ctx, long long *count);

/* Asynchronous: enqueues one frame on the context stream. slot_l0 must hold the
 * previous left pyramid, slot_l1 / slot_r1 the current pair. Track-set inputs
 * are DEVICE pointers when `inputs_on_device` != 0, else host pointers.
 * flags[i] bit 0 (VO_LM_TRIANGULATED) = lm->isTriangulated() of feature i; NULL = every landmark is
 * triangulated. New stereo landmarks stay untriangulated until the next keyframe (stereo_vo.cpp:736, :794), so a
 * real track set is a mix: an untriangulated feature takes pts_l0 / pts_r0 as prior and patch scale 1
 * (stereo_vo.cpp:490, :515-519), goes through [4], [4-1], [5] like every other, stays out of the pose-only BA
 * (:599) with mask_motion = true (:582) and meets the y > 660 gate of [7] (:653-668). Xp[i] (the landmark in the
 * previous left camera frame, T_pw * X) is read only where the bit is set. Bit 1 (VO_LM_DROPPED): see above.
 * One frame in flight per context (VO_ERR_INVALID otherwise). */
int vo_stereo_frame_enqueue(vo_ctx *ctx, const vo_stereo_params *prm, int slot_l0, int slot_l1,
                            int slot_r1, const float *pts_l0, const float *pts_r0,
                            const float *Xp, const uint8_t *flags, int n, const float dT_prior[16],
                            const float *pts_new, int n_new, int inputs_on_device);
/* ---- step [10] closed on the device ------------------------------------------------------------------------
 * In the reference the new-point candidates of a frame are extractORBwithBinning_fast(I1_left) AFTER
 * updateWeightBin(lmtrack_final.pts_l1) (stereo_vo.cpp:691-693), i.e. they depend on this frame's BA. What depends on
 * the BA is only WHICH bins ask for a point; the detection and the best keypoint of each bin depend on the image
 * alone. So: vo_new_point_candidates_enqueue runs cv::ORB::detect's restatement and the per-bin arg-max for EVERY bin
 * as soon as the image is in its slot (side stream, next to the previous frame), vo_stereo_frame_enqueue_closed
 * tracks every bin's candidate bidirectionally next to the features (speculatively), and the BA launch's epilogue
 * applies updateWeightBin and emits, bins ascending, exactly the candidates the reference would have extracted and
 * tracked — no host round trip and no dependent launch behind the BA. Two tables (0 / 1) so that the detection of
 * pair k+1 can run while frame k is in flight. */
typedef struct {
  int n_bins_u, n_bins_v;        /* FeatureExtractor::initParams */
  int u_step, v_step;            /* WeightBin::init, feature_extractor.h:103-104: (int)floor(n_cols / n_bins_u), ... */
  float inv_u_step, inv_v_step;  /* :106-107 */
  vo_orb_params orb;
} vo_bin_params;
int vo_new_point_candidates_enqueue(vo_ctx *ctx, int slot, const vo_bin_params *bins, int table);
/* test hook: waits for the table; xy[n_bins][2], has[n_bins] (either may be NULL), keypoints detected */
int vo_new_point_candidates_get(vo_ctx *ctx, int table, float *xy, uint8_t *has, int *n_detected);
/* vo_stereo_frame_enqueue with the candidates taken from `table` (which must hold the detection of the image in
 * slot_l1). n must be > 0 and prm->win one of 13, 15, 21, 31. Results: vo_stereo_frame_result (pts_new_r, mask_new:
 * room for n_bins entries; counts->n_new_ok) and vo_stereo_frame_new_points. */
int vo_stereo_frame_enqueue_closed(vo_ctx *ctx, const vo_stereo_params *prm, int slot_l0, int slot_l1, int slot_r1,
                                   const float *pts_l0, const float *pts_r0, const float *Xp, const uint8_t *flags,
                                   int n, const float dT_prior[16], const vo_bin_params *bins, int table,
                                   int inputs_on_device);
/* The closed frame on the reference's own data flow (stereo_vo.cpp:475-522, :595-613): Xw holds the landmarks in the
 * WORLD frame (lm->get3DPoint()), T_pw = stframe_prev->getLeft()->getPoseInv(), T_cw_prior = inverseSE3_f(T_wp *
 * dT_pc_prev), dT_prior = dT_pc_prev (the BA's initial value, :585). X_l1 = T_cw_prior X, the patch scale is
 * (T_pw X)(2) / X_l1(2) and the BA takes Xp = T_pw X, each in Eigen's evaluation order of `R * X + t`. */
int vo_stereo_frame_enqueue_closed_world(vo_ctx *ctx, const vo_stereo_params *prm, int slot_l0, int slot_l1, int slot_r1,
                                         const float *pts_l0, const float *pts_r0, const float *Xw, const uint8_t *flags,
                                         int n, const float dT_prior[16], const float T_pw[16], const float T_cw_prior[16],
                                         const vo_bin_params *bins, int table, int inputs_on_device);
/* after vo_stereo_frame_result of a closed frame: the candidates' left pixels (pts_l1_new; room for n_bins) */
int vo_stereo_frame_new_points(vo_ctx *ctx, float *pts_new, int *n_new);

/* Waits for the last enqueued frame and copies its results to host buffers
 * (any of which may be NULL). stage[i] = number of gates point i passed (0..4):
 * 1 [4], 2 [4-1], 3 [5], 4 = in lmtrack_final (BA inlier or untriangulated, and past the gate of [7]). */
int vo_stereo_frame_result(vo_ctx *ctx, float *pts_l1, float *pts_r1, uint8_t *stage,
                           float dT[16], float *pts_new_r, uint8_t *mask_new,
                           vo_frame_counts *counts, vo_gn_info *gn);

/* ---- StereoVO: the closed loop around the frame ---------------------------------------------------------------
 * StereoVO::trackStereoImages (core/visual_odometry/stereo_vo/stereo_vo.cpp:392-989, class surface stereo_vo.h:233-249)
 * with the track set carried ON THE DEVICE from frame to frame: what enters frame k+1 is what frame k left behind —
 * lmtrack_final (the stage-4 survivors in index order, :670) followed by the new landmarks of step [10] (:714-739:
 * trackBidirection mask and both DLT depths positive, mapping::triangulateDLT = core/util/triangulate_3d.cpp:91-130
 * with Eigen's 4x4 JacobiSVD restated), landmark ids from the context's counter (landmark.cpp:29), the previous pose
 * and the constant-velocity prior (:475-480, frame.cpp:50-54), the keyframe rule (keyframes.cpp:217-303) and, at a
 * keyframe, the reconstruction of lmtrack_final (:763-797) and the local bundle adjustment over the keyframe window
 * (:802 -> motion_estimator.cpp:1207-1340, sparse_ba_parameters.h:292-466, sparse_bundle_adjustment.cpp:624-722).
 * The first pair is the reference's initialisation (:842-949). The host sees one small result block per frame.
 * Needs a context with >= 5 image slots (previous left, current pair, next pair) and prm.frame.win in {13,15,21,31}. */
typedef struct vo_svo vo_svo;
typedef struct {
  vo_stereo_params frame;   /* Camera.*, feature_tracker.*, motion_estimator.thres_poseba_error */
  vo_bin_params bins;       /* feature_extractor.* as FeatureExtractor::initParams derives them */
  float kf_overlap_ratio;   /* keyframe_update.thres_alive_ratio   (StereoKeyframes::setThresOverlapRatio) */
  float kf_rotation_deg;    /* keyframe_update.thres_rotation      (degrees; the reference multiplies by D2R) */
  float kf_translation;     /* keyframe_update.thres_trans */
  int kf_window;            /* keyframe_update.n_max_keyframes_in_window (with local_ba: at most 16) */
  int strict_border;        /* vo_stereo_frame_set_strict_border */
  int local_ba;             /* != 0: localBundleAdjustmentSparseSolver_Stereo at every keyframe (the reference's behaviour);
                               the window may span at most 2^24 landmark ids — the distance from the oldest landmark
                               still tracked at the window's oldest keyframe to the newest, ~80 000 frames of a track
                               that never dies (VO_ERR_CAPACITY beyond). Landmark table, keyframe window and the BA
                               problem live on the device, allocated by vo_svo_create (vo_svo_device_bytes: ~32 MB at
                               configs[1]); the table doubles with the ids handed out (17 B per landmark ever created,
                               like the reference's all_landmarks_; beyond 2^24 the oldest read as the origin) */
  int rectify;              /* != 0: flagDoUndistortion (stereo_vo.cpp:414-427) — every incoming pair goes through the
                               context's stereo rectification maps (vo_rectify_init_stereo / vo_rectify_set_maps first) on
                               its way into the pyramids; frame.Kl / Kr / T_lr are then the RECTIFIED camera and extrinsics */
} vo_svo_params;
typedef struct {
  int frame_id;             /* id of the left Frame of this pair (the right one is frame_id + 1, frame.cpp:176-180) */
  int is_first, is_keyframe, lba_ran;
  int n_tracks_in;          /* size of the track set that entered the frame */
  int n_final;              /* lmtrack_final.n_pts: stage-4 survivors */
  int n_new;                /* landmarks created in step [10] */
  int n_tracks_out;         /* n_final + n_new: the next frame's track set */
  int n_kf_tracked;         /* survivors that belong to the last keyframe (numerator of the overlap ratio) */
  int n_new_candidates;     /* candidates step [10] extracted (bins left empty that hold a keypoint) */
  vo_frame_counts counts;
  vo_gn_info gn;
  float dT[16];             /* dT_pc_poBA */
  float T_wc[16];           /* pose of the left camera after this call (after the local BA at a keyframe) */
  double lba_err_first, lba_err_last; /* average pixel error of the local BA's first / last iteration */
  int lba_landmarks, lba_observations;
} vo_svo_frame_info;
int vo_svo_create(vo_ctx *ctx, const vo_svo_params *prm, vo_svo **out);
void vo_svo_destroy(vo_svo *svo);
/* StereoVO::trackStereoImages(img_left, img_right, timestamp): synchronous. Images: tightly addressed u8, `stride`
 * bytes per row; device pointers when on_device != 0, else host pointers (pinned memory gives a true asynchronous
 * copy). Errors: VO_ERR_GN_FAILED = the reference's throw "PoseOnlyStereoBA is failed!" (:626), VO_ERR_LBA_NAN. */
int vo_svo_track(vo_svo *svo, const void *left, const void *right, int stride, int on_device, double timestamp,
                 vo_svo_frame_info *info);
/* The same in two halves, so that a caller that already holds the NEXT pair (a recorded sequence) can hand it over
 * while this frame is in flight: vo_svo_enqueue(k); vo_svo_prefetch(k+1); vo_svo_result(k). The prefetch builds the
 * pair's pyramids and the per-bin candidate table on the side stream; the following vo_svo_enqueue / vo_svo_track with
 * the SAME two pointers uses them (other pointers: the prefetch is dropped and the pair is ingested as usual). Host
 * buffers of a prefetched pair must stay untouched until that pair's frame has returned. */
int vo_svo_enqueue(vo_svo *svo, const void *left, const void *right, int stride, int on_device, double timestamp);
int vo_svo_prefetch(vo_svo *svo, const void *left, const void *right, int stride, int on_device);
int vo_svo_result(vo_svo *svo, vo_svo_frame_info *info);
/* A recorded sequence through the same three calls, the loop on this side of the ABI: collects frames k_begin .. k_end - 1
 * of the n_total pairs left[k] / right[k] — vo_svo_result(k), then at once vo_svo_enqueue(k + 1) and vo_svo_prefetch(k + 2).
 * k_begin == 0 starts the sequence; otherwise frame k_begin is the one a previous call left in flight, and frame k_end is
 * in flight on return (when there is one; collect it with vo_svo_result or the next vo_svo_run). infos (may be NULL):
 * [k_end - k_begin]; stamps (may be NULL): CLOCK_MONOTONIC seconds at which each frame's result was in hand. */
int vo_svo_run(vo_svo *svo, const void *const *left, const void *const *right, int n_total, int stride, int on_device,
               int k_begin, int k_end, vo_svo_frame_info *infos, double *stamps);
/* The track set the next frame will start from (stframe_prev_'s pts seen + related landmarks): ids, left / right
 * pixels, world points, flags (VO_LM_TRIANGULATED, VO_LM_DROPPED, VO_LM_KF_MEMBER). Any pointer may be NULL; *n
 * receives the size. A device-to-host copy with a synchronisation: a test / inspection hook, not part of the loop. */
#define VO_LM_KF_MEMBER 4
int vo_svo_get_tracks(vo_svo *svo, int32_t *ids, float *pts_l, float *pts_r, float *Xw, uint8_t *flags, int cap, int *n);
/* step [10] of the last frame: the extracted candidates (left / right pixels, trackBidirection mask) and which of them
 * became landmarks (stereo_vo.cpp:716-725). Capacity n_bins each. */
int vo_svo_get_new_points(vo_svo *svo, float *pts_l, float *pts_r, uint8_t *mask_new, uint8_t *accept, int *n);
/* mapping::triangulateDLT (triangulate_3d.cpp:91-130) for n pixel pairs on the device: X0 (first camera), X1 = R10 X0 +
 * t10. T_10 row-major 4x4 (e.g. T_rl); K0 / K1 = fx, fy, cx, cy. */
int vo_triangulate_dlt(vo_ctx *ctx, const float *pts0, const float *pts1, int n, const float T_10[16], const float K0[4],
                       const float K1[4], float *X0, float *X1);

/* ---- batch of sequences on one device ---------------------------------------------------------------------
 * S independent stereo streams on ONE GPU, each with its own context (HIP streams, slots, landmark / frame id counters:
 * SURVEY F11), its own StereoVO and its own host thread inside the library. (BASELINE's batch mode proper is one stream
 * per GPU; a single sequential stream is latency-bound and leaves most of an MI355X idle.) The streams share nothing.
 * vo_batch_run: stream s tracks the pairs left[s * n_frames + k], right[...] (k = 0..n_frames-1; device pointers when
 * on_device != 0) in order, pair k+1 handed over while frame k is in flight; the first `warmup` frames of every stream are
 * untimed and all streams start the timed part together. Outputs (each may be NULL): T_wc [n_streams][n_frames][16],
 * last_ids [n_streams][ids_cap] + n_ids [n_streams] (every stream's final track-set ids), seconds [n_streams] (timed
 * wall time per stream), *wall (first start to last end). */
typedef struct vo_batch vo_batch;
/* (The batch's streams run in tree summation order: vo_set_sum_order does not reach them.) */
int vo_batch_create(const vo_config *cfg, const vo_svo_params *prm, int n_streams, vo_batch **out);
void vo_batch_destroy(vo_batch *batch);
const char *vo_batch_last_error(const vo_batch *batch);
/* vo_debug_set on every stream's context (measurement switches, e.g. VO_DBG_SKIP_DETECT) */
int vo_batch_debug_set(vo_batch *batch, int key, int value);
/* The strict-border arrangement the batch's streams run with: prm->strict_border, except that the arrangements with a
 * replay next to the frame kernel (3, 4, 5) become the stream-ordered one (1, same results) when n_streams > 1. */
int vo_batch_strict_border(const vo_batch *batch);
int vo_batch_run(vo_batch *batch, const void *const *left, const void *const *right, int n_frames, int stride, int on_device,
                 int warmup, float *T_wc, int32_t *last_ids, int ids_cap, int *n_ids, double *seconds, double *wall);

/* AlgorithmStatistics::stats_keyframe as trackStereoImages refreshes it at every keyframe (stereo_vo.cpp:805-821; read by
 * the ROS 2 node for its trajectory and map-point topics, ros2/visual_odometry/stereo_vo_ros2.cpp:141-166): every
 * keyframe so far, j = 0 .. count-1, with its CURRENT pose and the current 3-D points of its related landmarks (the local
 * BA keeps changing both). mappoints may be NULL (count only); cap = room for that many points. */
int vo_svo_keyframe_count(vo_svo *svo, int *n_keyframes);
int vo_svo_get_keyframe(vo_svo *svo, int j, float T_wc[16], float *mappoints, int cap, int *n_points);
/* all of them at once (what trackStereoImages rewrites at every keyframe): T_wc [n_keyframes][16], n_points [n_keyframes],
 * mappoints [total][3] in keyframe order; any of the three may be NULL; *total_points = sum of n_points */
int vo_svo_get_keyframes(vo_svo *svo, float *T_wc, int32_t *n_points, float *mappoints, size_t cap_points, size_t *total_points);
/* Device memory this StereoVO holds for its keyframes (landmark table, keyframe ring, keyframe pool, the local BA's window
 * scratch and arena): ~32 MB at BASELINE configs[1] (max_points 4024, window of 9), all of it allocated by vo_svo_create. */
int vo_svo_device_bytes(const vo_svo *svo, size_t *bytes);
/* img_debug_ of the reference's StereoVO: with the option on, every tracked frame draws what stereo_vo.cpp:685-688 draws,
 * showTrackingBA(I1_left, {}, lmtrack_final.pts_l1) = vo_draw_tracking_ba (below) on level 0 of the current left image with
 * pts empty and pts_proj = the frame's surviving landmarks' left pixels (the first n_final entries of the track set the frame
 * leaves behind). Off by default; with it off no launch, allocation or result differs from a driver without the option.
 * vo_svo_set_debug_image(svo, 1) allocates an index plane, the picture on the device and a pinned host picture — the
 * option's only allocation; VO_ERR_INVALID while a frame is in flight. The rendering is enqueued behind the frame's last
 * launch on the context's side stream, with the copy to the host behind it; vo_svo_result does not wait for it, and poses,
 * ids, flags and keyframe decisions are the same bits with the option on and off.
 * vo_svo_get_debug_image waits for the last picture only and copies it into `out` (height x width x 3 bytes, row pitch
 * out_stride >= 3 * width; NULL: the size only). A frame that does not draw (the first pair of a stream) keeps the previous
 * picture; before the first one *width = *height = 0 and the call returns VO_OK.
 * MonoVO's form of the option is vo_mvo_set_debug_image / vo_mvo_get_debug_image (below). */
int vo_svo_set_debug_image(vo_svo *svo, int on);
int vo_svo_get_debug_image(vo_svo *svo, uint8_t *out, int out_stride, int *width, int *height);
/* Covariance of StereoVO's pose, what a node puts into nav_msgs::Odometry::pose.covariance. Off by default;
 * with it off no launch, allocation or result differs from a driver without the option. vo_svo_set_pose_covariance(svo, 1,
 * sigma_px) makes the option's only allocations (two result blocks on the device, one in pinned host memory) and starts the
 * chain at P = 0; VO_ERR_INVALID while a frame is in flight. sigma_px > 0 scales by sigma_px^2 instead of the a-posteriori s2.
 * Behind every frame's BA launch, in stream order, one launch of the operator above (vo_gn_pose_information_stereo) reads the
 * launch's compacted set and the T01 it wrote on the device, and chains
 *   P_k = Ad(T10,k) P_k-1 Ad(T10,k)^T + Sigma_xi,k,   Ad(T) = [[R, [t]x R], [0, R]],   T_wc_true ~ T_wc_est exp(-e), e ~ N(0, P_k).
 * A frame whose pose did not come from the BA (the first pair, a block that is not valid) only carries P with its T10 and counts
 * in n_unknown_steps. The local BA moves T_wc at a keyframe and leaves P alone. vo_svo_result does not wait for the launch;
 * vo_svo_get_pose_covariance does (any output may be NULL; VO_ERR_INVALID while a frame is in flight or with the option off). */
int vo_svo_set_pose_covariance(vo_svo *svo, int on, double sigma_px);
int vo_svo_get_pose_covariance(vo_svo *svo, double P[36], double Sigma_xi[36], double *s2, int *valid, int *n_points,
                               int *n_unknown_steps);
/* test hook: what the last frame's covariance launch read — the BA set (X in the previous left camera's frame, both pixel
 * sets; cap entries of room, NULL: the count only) and the T01 the BA returned */
int vo_svo_get_pose_covariance_inputs(vo_svo *svo, float *X, float *pts_l, float *pts_r, int cap, int *n, float T01[16]);

/* ---- Ignore mask: where keypoint detection and the track gate do not look ----------
 * A mask is a width x height plane of bytes (`stride` bytes per row, host or device memory) in the pixels of the LEFT / mono
 * image as the tracker sees it — after rectification, if any. 0 = ignore, non-zero = usable. The lookup of a float pixel
 * (x, y) is mask[(int)(y + 0.5f)][(int)(x + 0.5f)] (cv::KeyPointsFilter::runByPixelsMask's rounding); an index outside the
 * plane reads as 0. Two places read it:
 *   detection   a keypoint whose (level-scaled) position reads 0 does not vote for its bucket: the result is "detect, drop the
 *               masked keypoints, then bucket". The detection itself is not masked: the count of detected keypoints
 *               (n_detected) is that of the unmasked image, and vo_orb_detect's list never reads a mask.
 *   track gate  the BA launch promotes a feature to stage 4 only where the lookup at its current left pixel is non-zero (the
 *               general form of the reference's y > 660 gate, stereo_vo.cpp:653-668). A masked feature stays at stage 3: it
 *               took part in this frame's BA, is not in the next track set, and its bucket is free for this frame's new points.
 * Without a mask (the default; NULL) every kernel runs exactly what it ran before the option existed, and a mask of all 255
 * gives the same bits as none.
 *
 * vo_set_slot_mask: the mask of the image in `slot` (which must hold one: the mask has its dimensions), copied into storage the
 * context owns (allocated at the slot's first mask); NULL clears it. It stays with the slot (vo_swap_slots moves it along) until
 * cleared or replaced, or until an image of another size is put into the slot (the mask is dropped then). Read by vo_new_point_candidates_enqueue, vo_extract_orb_with_binning[_enqueue] and the frame operators'
 * gate (the mask of slot_l1 / slot1); NOT by vo_orb_detect. VO_ERR_INVALID while a frame is in flight. Returns when the caller's
 * buffer is free again. */
int vo_set_slot_mask(vo_ctx *ctx, int slot, const void *mask, int stride, int on_device);
/* the size of the image in `slot` (0 x 0: the slot holds none) — what a mask for it must measure. Host state only: no device work. */
int vo_slot_image_size(vo_ctx *ctx, int slot, int *width, int *height);
/* The drivers: the mask that pairs / images ingested FROM NOW ON carry (frame.width x frame.height; VO_ERR_INVALID for a stride
 * below the width); NULL: none. Legal between any two of track / enqueue / prefetch / result — a per-frame mask is set before its
 * pair is handed over. A pair keeps the mask it was ingested with: its detection (side stream, possibly a frame ahead) and the
 * gate of its own frame read the same plane, whatever is set afterwards. vo_svo_run / vo_mvo_run use the mask current at the
 * call. The call copies into library-owned storage and returns when the caller's buffer is free again. Storage: one master
 * plane and one plane per left / mono image slot, all allocated at the FIRST set (vo_debug_allocation_count does not move
 * afterwards); at ingestion a slot's plane is refreshed — one device copy in front of the detector — only when the master
 * changed since. Creating and destroying a driver clears the masks of the slots it uses: a driver never sees its predecessor's
 * mask, and operator calls on those slots do not see a destroyed driver's. MonoVO's first two images and its 5-point-fallback frames are host-driven and have no stage-4 gate: there the
 * mask acts on the detection only. */
int vo_svo_set_mask(vo_svo *svo, const void *mask, int stride, int on_device);
/* (MonoVO: vo_mvo_set_mask, below) */

/* ---- ZNCC: image_processing::calcZNCC and the appearance gate ---------------------------------------
 * core/util/image_processing.cpp:195-266 with interpImage (:28-77). The reference has the function and, commented out in
 * FeatureTracker::trackWithPrior (feature_tracker.cpp:198-202), the place for it: calcZNCC(img0, img1, pts0[i], pts_track[i],
 * 15) > 0.5f. ZNCC does not change under gain and offset: the one test of a track that keeps its meaning under auto-exposure
 * and between two cameras of different gain.
 *
 * vo_zncc: n values, out[i] = ZNCC of the win x win patch of slot0's image at pts0[i] and of slot1's image at pts1[i] (level 0 as
 * the tracker sees it: after rectification / equalisation; both images of one size, VO_ERR_SIZE otherwise). Host pointers;
 * synchronous. n == 0 is legal. The arithmetic, all in float32, every operation rounded on its own (no FMA):
 *   window   win odd, 3 .. 31 (VO_ERR_INVALID otherwise; the reference throws on even).
 *   taps     n_elem = win * win; tap k = i * win + j has the offset (i - o, j - o) in (x, y).
 *            VO_ZNCC_PATTERN_REFERENCE: o = win. This is the reference's own text (patt[ind] = (i - win_sz, j - win_sz); win_half
 *            is computed and not used): the patch lies up-left of the point, its nearest corner at (-1, -1). Restated as written.
 *            VO_ZNCC_PATTERN_CENTERED:  o = win / 2: the patch the commented-out call presumably meant.
 *   position pt + offset, one float add per coordinate.
 *   sample   u0 = (int)u, v0 = (int)v (toward zero); valid iff 0 <= u0 < W - 1 and 0 <= v0 < H - 1 (the image, not the padded
 *            plane); ax = u - u0, ay = v - v0; value = ((axay * (((I1 - I2) - I3) + I4) + ax * (-I1 + I2)) + ay * (-I1 + I3)) + I1
 *            with I1 = I[v0][u0], I2 = I[v0][u0 + 1], I3 = I[v0 + 1][u0], I4 = I[v0 + 1][u0 + 1]. An invalid tap reads -2.0f
 *            (interpImage's resize(n, -2.0f)). A NaN coordinate, and one beyond the int range, is invalid. u in (-1, 0) gives
 *            u0 = 0 and a negative ax, as the text does.
 *   result   mean = sum / (float)n_elem per patch; numer = sum (I0 - mean_l)(I1 - mean_r), denom_l = sum (I0 - mean_l)^2,
 *            denom_r = sum (I1 - mean_r)^2; numer / sqrtf(denom_l * denom_r). A flat pair gives 0 / 0 = NaN.
 *   sums     vo_set_sum_order decides. VO_SUM_ORDER_REFERENCE: index order k = 0 .. n_elem - 1. VO_SUM_ORDER_TREE (default): the
 *            terms zero-padded to P, the next power of two >= max(n_elem, 64); for stride = P/2 .. 1: s[i] += s[i + stride]
 *            (i < stride); s[0]. One wavefront per feature: lane l holds taps l, l + 64, ...
 *
 * The gate (StereoVO / MonoVO; off by default — with it off no launch, wait, allocation or result bit differs): a feature the
 * BA launch would promote to stage 4 additionally needs zncc > thres (NaN fails), in the same place and with the same
 * consequences as the ignore mask's track gate, and combined with it by AND: a failing feature stays at stage 3 — it took
 * part in this frame's BA, is not in the next track set, and its bucket is free for this frame's new points.
 *   VO_ZNCC_TEMPORAL  the previous left / mono image at the feature's input pixel against the current left / mono image at its
 *                     final pixel
 *   VO_ZNCC_STEREO    (StereoVO only) the current left image at the final left pixel against the current right image at the
 *                     final right pixel
 * The values come from one launch of the operator's kernel in front of the BA launch, over the whole input track set, behind
 * everything that writes the final pixels: with the gate on, a strict-border replay that would run on its own stream next to
 * the frame kernel (vo_stereo_frame_set_strict_border 3, 4, 5) runs stream-ordered instead — the results are the same. A feature that was lost
 * on the way has whatever its pixels give (often NaN); it is not promoted anyway. MonoVO's host-driven frames (the first two
 * images, a 5-point fallback) have no gate, as with the mask. vo_batch streams have no gate.
 * vo_svo_set_zncc_gate: pairs = a bit set of VO_ZNCC_*, 0 = off (win, pattern, thres are then not looked at). The first call
 * with pairs != 0 allocates the per-feature floats (vo_debug_allocation_count does not move afterwards). VO_ERR_INVALID while a
 * frame is in flight, for a bad window or pattern, a NaN threshold, unknown bits, and VO_ZNCC_STEREO on a MonoVO.
 * vo_svo_get_zncc: inspection, like vo_svo_get_new_points — the values the last steady-state frame computed, per input feature
 * (*n = that frame's input count, 0 before any; at most cap are written; zncc_s is written only where VO_ZNCC_STEREO was on;
 * either pointer may be NULL). VO_ERR_INVALID while a frame is in flight or with the gate off. */
enum { VO_ZNCC_PATTERN_REFERENCE = 0, VO_ZNCC_PATTERN_CENTERED = 1 };
enum { VO_ZNCC_TEMPORAL = 1, VO_ZNCC_STEREO = 2 };
int vo_zncc(vo_ctx *ctx, int slot0, int slot1, const float *pts0, const float *pts1, int n, int win, int pattern, float *out);
int vo_svo_set_zncc_gate(vo_svo *svo, int pairs, int win, int pattern, float thres);
int vo_svo_get_zncc(vo_svo *svo, float *zncc_t, float *zncc_s, int cap, int *n);
/* (MonoVO: vo_mvo_set_zncc_gate / vo_mvo_get_zncc, below) */

/* ---- Semi-dense stereo: depth of the high-gradient pixels by an epipolar ZNCC search -----------------------
 * The static stereo part of the reference author's semi-dense prototype, as an operator on a rectified pair (epipolar lines
 * are rows) and as an option of StereoVO. Inputs: the level-0 u8 planes L, R of two slots of one size W x H, the left slot's
 * ignore mask where one is bound, and vo_semidense_params. All taps sit at integer pixels: the window sums are exact integers
 * and no summation order enters the result.
 *   params     hw 1..15, hh 0..3: the window is (2 hw + 1) x (2 hh + 1), n taps; 0 <= d_min <= d_max <= 1023; g_min 1..360;
 *              thres_best, thres_peak; peak_px, edge_px >= 0; eps_edge, eps_epi >= 0; bf = focal length x baseline [pixel m] > 0.
 *   candidate  (x, y) with m_x <= x <= W-1-m_x, m_y <= y <= H-1-m_y (m_x = max(hw, 1), m_y = max(hh, 1)); with the integers
 *              gx = L(x+1,y) - L(x-1,y), gy = L(x,y+1) - L(x,y-1): gx^2 + gy^2 >= g_min^2 and 3 gx^2 >= gy^2 (the gradient lies
 *              within 60 degrees of the epipolar line); not masked (mask byte != 0).
 *   scores     for d = d_min .. d_last = min(d_max, x - hw), over |k| <= hw, |v| <= hh with l = L(x+k, y+v), r = R(x-d+k, y+v):
 *              S_l, S_ll, S_r, S_rr, S_lr; A = n S_ll - S_l^2, B = n S_rr - S_r^2, num = n S_lr - S_l S_r as exact (64-bit)
 *              integers; s(d) = -1 where A == 0 or B == 0, else (float)num / sqrtf((float)A * (float)B), every operation
 *              rounded to float on its own (no FMA).
 *   status     in this order: 0 no candidate; 5 fewer than 2 edge_px + 3 disparities in the range, or A == 0; with d_best the
 *              disparity of the largest s (ties: the smallest d): 2 s(d_best) <= thres_best; 3 some d with s(d) > thres_peak has
 *              |d - d_best| > peak_px; 4 not (d_min + edge_px < d_best < d_last - edge_px); 1 accepted.
 *   accepted   s0 = s(d_best), sm = s(d_best - 1), sp = s(d_best + 1); den = (sm + sp) - (s0 + s0);
 *              off = den != 0 ? (0.5f * (sm - sp)) / den : 0; disparity = (float)d_best + off;
 *              g = sqrtf((float)(gx^2 + gy^2)); du = (float)gx / g; dv = (float)gy / g; e = eps_epi * dv;
 *              sigma_invd = (sqrtf(eps_edge * eps_edge + e * e) / fabsf(du)) / bf — in this order, each operation rounded.
 *   outputs    four W x H planes, tightly packed: disparity f32 (0 where status != 1), score f32 (s(d_best) for status 1..4,
 *              else 0), sigma_invd f32 (standard deviation of the inverse depth; 0 where status != 1), status u8.
 * vo_semidense_stereo: any output may be NULL; on_device: the outputs are device memory. Synchronous.
 * vo_semidense_points: the accepted pixels of such planes (host, or device with planes_on_device) in raster order, by the
 * library's stable compaction: z = bf / disparity, X = (((float)x - cx) / fx * z, ((float)y - cy) / fy * z, z) with K = fx, fy,
 * cx, cy; with T (row-major 4 x 4, may be NULL) X' [r] = (T[r][0] X + (T[r][1] Y + T[r][2] Z)) + T[r][3]. Host outputs xyz [cap][3],
 * sigma_out [cap] (may be NULL), pixel [cap][2] (x, y; may be NULL); *n = the true count, also with VO_ERR_CAPACITY (n > cap: the
 * first cap entries are written). The planes may not exceed vo_config.max_width x max_height.
 *
 * StereoVO (off by default; with it off no launch, wait, allocation or result bit differs; with it on the odometry's results
 * are the same bits): vo_svo_set_semidense(svo, prm, every) — prm NULL = off — makes the option's only allocations at the first
 * enable. every = VO_SEMIDENSE_KEYFRAMES: a result per keyframe; VO_SEMIDENSE_FRAMES: per frame (the first pair included). The
 * launch for a frame is enqueued by vo_svo_result, where the keyframe decision and the pose after the local BA are known, on the
 * side stream behind a fork event of the main stream; it reads the frame's own left and right slots; vo_svo_result never waits
 * for it. A later ingestion into a slot the launch reads is ordered behind the launch's event on the device. A frame that
 * produces no result leaves the previous one in place. vo_svo_get_semidense: the last result's planes (any may be NULL), size,
 * frame_id (-1 and 0 x 0 before any), T_wc and the number of accepted pixels; waits for that launch's event only.
 * vo_svo_get_semidense_points: vo_semidense_points of the last result with the left camera's K, in the world frame (world != 0:
 * T = the frame's T_wc) or the camera frame. All three: VO_ERR_INVALID while a frame is in flight; the getters also with the
 * option off. Not for MonoVO or vo_batch streams. */
typedef struct {
  int hw, hh;          /* 8, 1 */
  int d_min, d_max;    /* 0, 64 */
  int g_min;           /* 20 */
  float thres_best;    /* 0.95 */
  float thres_peak;    /* 0.9 */
  int peak_px;         /* 5 */
  int edge_px;         /* 2 */
  float eps_edge;      /* 0.5 */
  float eps_epi;       /* 1.0 */
  float bf;            /* 1.0: set it */
} vo_semidense_params;
enum { VO_SEMIDENSE_KEYFRAMES = 0, VO_SEMIDENSE_FRAMES = 1 };
int vo_semidense_default_params(vo_semidense_params *prm);
int vo_semidense_stereo(vo_ctx *ctx, int slot_l, int slot_r, const vo_semidense_params *prm, float *disparity, float *score,
                        float *sigma_invd, uint8_t *status, int on_device);
int vo_semidense_points(vo_ctx *ctx, const float *disparity, const float *sigma_invd, const uint8_t *status, int width, int height,
                        int planes_on_device, const float K[4], float bf, const float *T, int cap, float *xyz, float *sigma_out,
                        uint16_t *pixel, int *n);
int vo_svo_set_semidense(vo_svo *svo, const vo_semidense_params *prm, int every);
int vo_svo_get_semidense(vo_svo *svo, float *disparity, float *score, float *sigma_invd, uint8_t *status, int *width, int *height,
                         int *frame_id, float T_wc[16], int *n_accepted);
int vo_svo_get_semidense_points(vo_svo *svo, int world, int cap, float *xyz, float *sigma_invd, uint16_t *pixel, int *n, int *frame_id);

/* ---- Dense stereo: a disparity for every pixel by census + semi-global matching ----------------------------
 * Coverage, not precision: the semi-dense operator above measures the high-gradient pixels more exactly; this one gives walls,
 * road and weakly textured surfaces a disparity too. Inputs: the level-0 u8 planes L, R of two slots of one size W x H (both
 * <= 65535), the left slot's ignore mask where one is bound, and vo_dense_stereo_params. Everything up to the parabola is an
 * integer, and min and + do not depend on an order: tests/dense_stereo_restatement.py restates it.
 *   params     d_min >= 0; n_disp 64, 128, 192 or 256: the disparities searched are d_min + d, d = 0 .. n_disp-1; paths 4 or 8;
 *              0 <= p1 < p2 <= 8129 (S below fits 16 bits: 8 (62 + p2) <= 65535); uniqueness 0..99; lr_max >= -1 (-1: no
 *              left-right check); eps_d >= 0 [pixel] and bf = focal length x baseline [pixel m] > 0, both finite.
 *   census     cen(x, y): 62 bits of a 64-bit word over the 9 x 7 window without its centre. Taps in raster order, v = -3..3
 *              (rows, outer), k = -4..4 (columns, inner), the centre skipped: the t-th tap sets bit t (t = 0..61) where
 *              I(clamp(x+k, 0, W-1), clamp(y+v, 0, H-1)) < I(x, y).
 *   cost       C(x, y, d) = popcount(cenL(x, y) ^ cenR(x - d_min - d, y)); 62 where x - d_min - d < 0.
 *   paths      directions r = (dx, dy): (1,0), (-1,0), (0,1), (0,-1), and with paths = 8 also (1,1), (-1,-1), (1,-1), (-1,1).
 *              L_r(p, d) = C(p, d) where p - r lies outside the image, else with m = min_k L_r(p-r, k):
 *              C(p, d) + min(L_r(p-r, d), min(L_r(p-r, d-1), L_r(p-r, d+1)) + p1, m + p2) - m; a neighbour d-1 < 0 or
 *              d+1 > n_disp-1 does not take part. p2 is constant. S = the sum of L_r over the directions (<= 65535).
 *   decision   d_best = the d of the smallest S(x, y, d) (ties: the smallest d); S2 = the smallest S(x, y, d) over |d - d_best| > 1;
 *              x_r = x - d_min - d_best; d_R(x_r) = the d of the smallest S(x_r + d_min + d, y, d) over the d with
 *              x_r + d_min + d <= W-1 (ties: the smallest d): the right view's disparity from the same volume.
 *   status     in this order of precedence: 0 masked (mask byte == 0); 4 d_best == 0 or d_best == n_disp-1; 2 S2 (100 - uniqueness) <
 *              100 S(d_best) (64-bit integers); 3 with lr_max >= 0: x_r < 0 or |d_R(x_r) - d_best| > lr_max; 1 accepted. The mask
 *              touches the outputs only: masked pixels take part in the aggregation.
 *   accepted   Sm, S0, Sp = (float)S(x, y, d_best - 1), .. (d_best), .. (d_best + 1); den = (Sm + Sp) - (S0 + S0);
 *              off = den != 0 ? (0.5f * (Sm - Sp)) / den : 0; disparity = (float)(d_min + d_best) + off; sigma_invd = eps_d / bf —
 *              float32, each operation rounded on its own (no FMA).
 *   outputs    four W x H planes, tightly packed: disparity f32 (0 where status != 1), cost u16 (S(d_best); 0 where masked),
 *              sigma_invd f32 (0 where status != 1), status u8. disparity, sigma_invd and status mean what vo_semidense_stereo's
 *              planes mean: vo_semidense_points, vo_semidense_map_seed, the regularisation and vo_semidense_world_integrate take
 *              them unchanged.
 * vo_dense_stereo: any output may be NULL; on_device: the outputs are device memory. Synchronous. The workspace — two census
 * planes (8 bytes a pixel each) and S (2 n_disp bytes a pixel) — belongs to the context, is allocated at the first call and grows
 * when a later call needs more; vo_dense_stereo_workspace reports its size for a shape. An allocation that fails is VO_ERR_HIP.
 *
 * StereoVO (off by default; with it off no launch, wait, allocation or result bit differs; with it on the odometry's and every
 * semi-dense option's results are the same bits): vo_svo_set_dense_stereo(svo, prm, every) — prm NULL = off, every as in
 * vo_svo_set_semidense — with exactly that option's rules: the option's only allocations at the first enable; the launches for a
 * frame are enqueued by vo_svo_result on the side stream behind a fork event of the main stream and read the frame's own slots;
 * vo_svo_result never waits; a later ingestion into a slot they read is ordered behind their event on the device.
 * vo_svo_get_dense_stereo: the last result's planes (any may be NULL), size, frame_id (-1 and 0 x 0 before any), T_wc and the
 * number of accepted pixels; vo_svo_get_dense_points: vo_semidense_points of it with the left camera's K. Both wait for that
 * result's event only. All three: VO_ERR_INVALID while a frame is in flight and on a MonoVO's driver; the getters also with the
 * option off. Independent of vo_svo_set_semidense: either, both or neither may be on.
 * Out of scope: the driver's world map, temporal map or propagation taking this result as their source (the operators above take
 * the planes; the world map's driver option since added: "Semi-dense map merge"); gradient-adaptive p2; speckle and median filters; hole filling; a right-image mask;
 * sub-pixel costs; more than 256 disparities; MonoVO and vo_batch; any use of the disparity in the odometry. */
typedef struct {
  int d_min;        /* 0 */
  int n_disp;       /* 64 */
  int paths;        /* 8 */
  int p1, p2;       /* 8, 64 */
  int uniqueness;   /* 10 */
  int lr_max;       /* 1 */
  float eps_d;      /* 0.5 */
  float bf;         /* 1.0: set it */
} vo_dense_stereo_params;
int vo_dense_stereo_default_params(vo_dense_stereo_params *prm);
int vo_dense_stereo_workspace(int width, int height, const vo_dense_stereo_params *prm, size_t *bytes);
int vo_dense_stereo(vo_ctx *ctx, int slot_l, int slot_r, const vo_dense_stereo_params *prm, float *disparity, uint16_t *cost,
                    float *sigma_invd, uint8_t *status, int on_device);
int vo_svo_set_dense_stereo(vo_svo *svo, const vo_dense_stereo_params *prm, int every);
int vo_svo_get_dense_stereo(vo_svo *svo, float *disparity, uint16_t *cost, float *sigma_invd, uint8_t *status, int *width, int *height,
                            int *frame_id, float T_wc[16], int *n_accepted);
int vo_svo_get_dense_points(vo_svo *svo, int world, int cap, float *xyz, float *sigma_invd, uint16_t *pixel, int *n, int *frame_id);

/* ---- Speckle filter: small connected components of a disparity plane removed --------------------------------
 * Small islands of wrong disparity survive the dense operator's uniqueness and left-right checks; in a point cloud or the voxel
 * map they are floating blobs. This operator labels the connected components of (disparity, sigma_invd, status) planes — W x H,
 * tightly packed, with the meaning they have under "Semi-dense stereo" and "Dense stereo" — and removes the small ones, in
 * place. 1 <= W, H <= 65535 and W H <= 2^31 - 1. tests/dense_speckle_restatement.py restates it.
 *   valid      a pixel with status == 1.
 *   joined     two 4-neighbours p, q (left/right, up/down) that are both valid with fabsf(disparity[p] - disparity[q]) <= max_diff:
 *              float32, one subtraction, rounded; a NaN result fails the comparison (so a NaN or an infinite disparity under
 *              status 1 joins nothing).
 *   component  a connected component of the graph of joined pairs over the valid pixels; its label is the smallest raster index
 *              y W + x among its pixels, its size the number of its pixels. Neither depends on any order of arrival.
 *   removal    every pixel of a component with size <= max_size: status = VO_DISPARITY_SPECKLE (6), disparity = 0 and (where the
 *              plane is given) sigma_invd = 0. Every other pixel, valid or not, keeps every bit; a cost or score plane is not
 *              touched. max_size = 0 removes nothing (the labels, sizes and counts are still computed).
 *   params     0 <= max_size; max_diff >= 0, finite [pixel].
 * vo_disparity_speckle_filter: disparity and status are required; sigma_invd, label, size, n_removed and n_components may be
 * NULL. label, size: W x H int32 planes describing the components BEFORE the removal — a pixel's label and its component's size;
 * -1 and 0 on invalid pixels. n_components: the number of components (all of them); n_removed: the number of removed pixels (host
 * integers also with on_device). on_device: the planes, label and size are device memory. Synchronous. The workspace — 16 bytes
 * of counters and two int32 planes: 16 + 8 W H bytes, what vo_speckle_workspace reports — belongs to the context, is allocated at
 * the first call and grows when a later call needs more; host planes also take a device copy of 9 W H bytes that grows likewise.
 * An allocation that fails is VO_ERR_HIP.
 *
 * StereoVO (off by default; with it off no launch, wait, allocation or result bit differs): vo_svo_set_dense_speckle(svo, prm) —
 * prm NULL = off — needs vo_svo_set_dense_stereo to be on. Its only allocation, at the first enable: the workspace for
 * max_width x max_height. The filter's launches follow the dense decision on the side stream, in front of that result's event,
 * in place on the driver's dense planes: vo_svo_get_dense_stereo returns the filtered planes (n_accepted counts status 1, so it
 * falls by the pixels removed), vo_svo_get_dense_points leaves the speckles out, and the guard of the slots covers them
 * unchanged. vo_svo_get_dense_speckle_stats: n_removed and n_components of the last result (0, 0 before any that went through
 * the filter; either may be NULL); waits for that result's event only. Both: VO_ERR_INVALID while a frame is in flight and on a
 * MonoVO's driver; the getter also with the option off.
 * Out of scope: the driver's world map taking the dense result as its source (since added: "Semi-dense map merge" below);
 * its temporal map or propagation doing so; a median filter; hole filling; 8-connectivity; fixed-point disparities as
 * OpenCV's filterSpeckles takes; the filter on the driver's semi-dense result (the operator takes any planes, but a map of thin
 * edges would lose most of itself); MonoVO and vo_batch. */
#define VO_DISPARITY_SPECKLE 6 /* status of a removed pixel (the semi-dense operator uses 0..5) */
typedef struct {
  int max_size;   /* 100 */
  float max_diff; /* 1.0 */
} vo_speckle_params;
int vo_speckle_default_params(vo_speckle_params *prm);
int vo_speckle_workspace(int width, int height, size_t *bytes);
int vo_disparity_speckle_filter(vo_ctx *ctx, float *disparity, float *sigma_invd, uint8_t *status, int width, int height,
                                const vo_speckle_params *prm, int32_t *label, int32_t *size, int *n_removed, int *n_components,
                                int on_device);
int vo_svo_set_dense_speckle(vo_svo *svo, const vo_speckle_params *prm);
int vo_svo_get_dense_speckle_stats(vo_svo *svo, int *n_removed, int *n_components);

/* ---- Semi-dense map merge: a keyframe's map and a disparity result of the same keyframe, per pixel --------------
 * The semi-dense chain measures edges well and covers little; the dense operator covers nearly everything and measures an edge worse.
 * The merge takes, per pixel, the better of what the two have: the fusion where they agree, the map where several frames outvote one
 * dense decision, the dense value where it is the only one. float32, every operation rounded on its own (no FMA), in the order
 * written; the counts are integers. tests/semidense_map_merge_restatement.py restates it.
 *   inputs     a map: invd, sigma f32, n_obs u8 (all three NULL: no map); a disparity result — a dense or a semi-dense one, filtered or
 *              not —: disparity, sigma_invd f32, status u8, with bf > 0; all W x H, tightly packed, W, H >= 1, W H <= 2^31 - 1.
 *   params     chi > 0, finite (default 3, the propagation's); keep_obs in 0..256 (default 2). chi2 = chi chi.
 *   m          the map has an entry at pixel j: a map is given and n_obs[j] >= 1.
 *   s          the result has one: rho_d, sig_d and the count n_d are what vo_semidense_map_seed writes for the pixel (rho_d =
 *              disparity[j] / bf, sig_d = sigma_invd[j], n_d = 1 where status[j] == 1; else 0, 0, 0 — the same device function), and
 *              s is n_d >= 1. Status 6 (VO_DISPARITY_SPECKLE) and every other status but 1 therefore give no entry, whatever bits
 *              their disparity and sigma_invd hold; a disparity of 0 under status 1 is an entry like any other (the seed makes one).
 *   neither    invd = sigma = 0, n_obs = 0, origin 0.
 *   m only     the map's three values, every bit, origin 1.
 *   s only     rho_d, sig_d, n_d, origin 2.
 *   both       the test and the fusion of the propagation's resolve (the same device function), the map in the warped source's
 *              role and the result in the static one's: dd = invd - rho_d, s2 = sigma sigma, m2 = sig_d sig_d, sum = s2 + m2.
 *              agree iff sum > 0 and dd dd <= chi2 sum (a NaN anywhere fails): invd = (invd m2 + rho_d s2) / sum,
 *              sigma = sqrtf((s2 m2) / sum), n_obs = min(255, n_obs + 1), origin 3.
 *              Otherwise, where the map's n_obs >= keep_obs: the map's three values, every bit, origin 4 (several frames outvote
 *              one decision); else invd = sigma = 0, n_obs = 0, origin 5 (one of two single measurements is grossly wrong and
 *              nothing says which). keep_obs = 0 always keeps the map, 256 never.
 *   counts     counts[k], k = 0..5: the number of pixels with origin k; they sum to W H.
 * vo_semidense_map_merge: the outputs invd, sigma, n_obs are required, origin and counts may be NULL; host planes, or all device
 * planes with on_device (counts is a host array of 6 either way). An output plane may be the input plane of the same kind (invd on
 * the map's invd, sigma on its sigma, n_obs on its n_obs): the operator is per pixel and the lane that writes a pixel is the only one
 * that reads it. A device pointer may have any alignment: planes that are not all 16-byte (f32) and 4-byte (u8) aligned take a path
 * that moves single elements, with the same bits. One launch; synchronous. VO_ERR_INVALID: chi not finite or <= 0, keep_obs outside
 * 0..256, bf not positive, a missing plane, a partial map trio. The context keeps 64 bytes of counts and, for host planes, a device copy
 * of 28 bytes a pixel that grows when a call needs more.
 *
 * StereoVO: vo_svo_set_semidense_world(svo, prm, source) also takes source = VO_SEMIDENSE_WORLD_DENSE (the merge without a map: the
 * dense result seeded) and VO_SEMIDENSE_WORLD_MERGED (the keyframe's fused map merged with the dense result of the keyframe's own
 * pair). Both need vo_svo_set_dense_stereo on next to the temporal option — VO_ERR_INVALID otherwise — and make one allocation at the
 * first enable of such a source: 64 bytes of counts, the keyframe's dense planes (9 bytes a pixel) and the merged planes with origin
 * (10 bytes a pixel) for max_width x max_height. One rule for either `every` of the dense option: behind the dense launches of a
 * keyframe (and the speckle filter's, whose planes the merge then sees) the result is copied device to device on the side stream
 * into the option's planes. When the keyframe is replaced (or at the flush) ONE merge launch on the side stream writes the merged
 * planes, and the re-anchoring's ring, the integration and the carve take those exactly as they take the regularised ones. A keyframe
 * without a dense result of its own pair (the source or the dense option switched on after it, the dense option off, another size)
 * is not integrated, and a later flush does not integrate it either. vo_svo_set_semidense_world_merge(svo, prm) sets chi and
 * keep_obs for the merges enqueued from then on (prm NULL: the defaults). vo_svo_get_semidense_world_source: the planes, origin and
 * counts (any may be NULL) of the last merge the driver enqueued, its size (0 x 0 where there is none) and keyframe; waits for the
 * side stream's last launch only. Both: VO_ERR_INVALID while a frame is in flight; the getter also with the world option off. With
 * these sources on, the odometry's results, the semi-dense and dense results and the keyframes' poses are the same bits.
 * Out of scope: the world option without the temporal option; the temporal search, the propagation or the alignment reading the merged
 * map; the dense value as a prior of the temporal search; trimming dense pixels at depth discontinuities, a median filter, hole
 * filling; decimating the dense input; a tighter refusal bound or a growing table; re-merging when the map changes after its
 * integration; MonoVO and vo_batch. */
typedef struct {
  float chi;     /* 3.0 */
  int keep_obs;  /* 2 */
} vo_semidense_map_merge_params;
int vo_semidense_map_merge_default_params(vo_semidense_map_merge_params *prm);
int vo_semidense_map_merge(vo_ctx *ctx, const float *map_invd, const float *map_sigma, const uint8_t *map_n_obs, const float *disparity,
                           const float *sigma_invd, const uint8_t *status, int width, int height, float bf,
                           const vo_semidense_map_merge_params *prm, float *invd, float *sigma, uint8_t *n_obs, uint8_t *origin,
                           uint64_t *counts, int on_device);
int vo_svo_set_semidense_world_merge(vo_svo *svo, const vo_semidense_map_merge_params *prm);
int vo_svo_get_semidense_world_source(vo_svo *svo, float *invd, float *sigma, uint8_t *n_obs, uint8_t *origin, int *width, int *height,
                                      int *frame_id, uint64_t *counts);

/* ---- Semi-dense temporal: the keyframe's pixels searched in the following left images, fused per keyframe ----
 * The second half of the reference author's semi-dense prototype, read for intent only: a pixel of the keyframe's left image is
 * searched in a later left image along the epipolar line the odometry's pose gives, and the inverse depths are fused as
 * Gaussians. Only + - x / sqrtf floorf fabsf in float32, every operation rounded on its own (no FMA), in the order written here;
 * the samples and the five sums are integers, so no summation order enters. tests/semidense_temporal_restatement.py restates it.
 *   inputs     Lk: the keyframe's left level-0 u8 plane; Lc: the current left plane (a slot's level 0), both W x H, 3 <= W, H <=
 *              65535; an ignore mask over the key pixels (the operator, which has no key slot, takes the one bound to slot_cur;
 *              the driver takes the keyframe left slot's, copied when the map is seeded); K = fx, fy, cx, cy; T_ck row-major 4 x 4, X_c = R X_k + t; the map: four W x H
 *              planes invd f32, sigma f32 (both 0 where there is nothing yet), n_obs u8, tstatus u8 (the last launch's decision).
 *   params     hw 1..15, hh 0..3; g_min 1..360; thres_best, thres_peak; peak_px, edge_px 0..512; eps_edge, eps_epi, eps_scale >= 0;
 *              0 < z_min < z_max [m]; 2 edge_px + 3 <= max_search <= 512; j_min > 0 [pixel per 1/m].
 *              r_min = 1.0f / z_max, r_max = 1.0f / z_min. C[i] = -((R[0][i] t0 + R[1][i] t1) + R[2][i] t2).
 *   candidate  (x, y) with 1 <= x <= W-2, 1 <= y <= H-2; gx, gy as in the static block, gx^2 + gy^2 >= g_min^2; not masked. Then
 *              xc = (float)x - cx, yc = (float)y - cy, u = xc / fx, v = yc / fy, a_i = (R[i][0] u + R[i][1] v) + R[i][2];
 *              d_k = (fx C0 - xc C2, fy C1 - yc C2), dk2 = d_kx^2 + d_ky^2. dk2 < 1e-6: the pixel sits on the epipole, status 7
 *              (so that an identity pose gives every candidate that status). dot = (float)gx d_kx + (float)gy d_ky,
 *              g2 = (float)(gx^2 + gy^2): (4 dot) dot < g2 dk2 (the gradient lies more than 60 degrees off the key epipolar
 *              line): no candidate. (ux, uy) = d_k / sqrtf(dk2). A key tap (below) outside the image: no candidate.
 *   range      prior (sigma > 0): lo = max(invd - 2 sigma, r_min), hi = min(invd + 2 sigma, r_max); else lo = r_min, hi = r_max.
 *              D(rho) = a2 + rho t2; p(rho) = (fx ((a0 + rho t0) / D(rho)) + cx, fy ((a1 + rho t1) / D(rho)) + cy).
 *              not (lo < hi), or D(lo) <= 0.1 or D(hi) <= 0.1 (an end not in front of the current camera): status 8.
 *              P0 = p(lo), e = p(hi) - P0, len = sqrtf(ex^2 + ey^2), J = len / (hi - lo). not (J >= j_min): status 7 (no
 *              parallax: the depth is not observable, the pixel must not enter the map). l = e / len.
 *              npos = (int)floorf(len + 0.5f) + 2 edge_px + 3 positions p_j = P0 + (float)j l, j = j0 .. j0 + npos - 1 with
 *              j0 = -(edge_px + 1). npos > max_search: status 6 (range too long), nothing is searched.
 *   taps       t = (v, k), v = -hh..hh outer, k = -hw..hw inner. The key direction d = +-(ux, uy), + where
 *              lx (fx (b0 D(lo) - N0 b2)) + ly (fy (b1 D(lo) - N1 b2)) >= 0 with b_i = R[i][0] (ux / fx) + R[i][1] (uy / fy),
 *              N_i = a_i + lo t_i (the derivative of p(lo) along the key direction, times D(lo)^2: the key direction that
 *              corresponds to l). Key tap: ((float)x + (float)k dx) + (float)v (-dy), ((float)y + (float)k dy) + (float)v dx.
 *              Current tap of position j: (p_jx + (float)k lx) + (float)v (-ly), (p_jy + (float)k ly) + (float)v lx.
 *              A coordinate c becomes X = (int)floorf(32 c + 0.5f) where that lies in [-2^20, 2^22], else -2^20; cell X >> 5,
 *              weight X & 31. The tap is inside where 0 <= cell_x <= W-2 and 0 <= cell_y <= H-2 — decided on the integers
 *              before any load. Value: ((32-wy) ((32-wx) I00 + wx I10) + wy ((32-wx) I01 + wx I11) + 32) >> 6, 0 .. 4080.
 *   scores     S_k, S_kk, S_c, S_cc, S_kc over the n taps (n <= 217: they fit 32 bits unsigned); A = n S_kk - S_k^2,
 *              B = n S_cc - S_c^2, num = n S_kc - S_k S_c (64-bit); s(j) = -1 where A == 0 or B == 0, else
 *              (float)num / sqrtf((float)A * (float)B). A position with a tap outside has no score.
 *   run        the positions searched: the maximal run of inside positions that contains the prior's position
 *              jp = (int)floorf(((p(invd)_x - P0x) lx + (p(invd)_y - P0y) ly) + 0.5f) (a prior with D(invd) > 0.1 and jp among
 *              the positions), or else the first maximal run.
 *   status     0 no candidate; 7, 8, 6 as above; then 5: no run, fewer than 2 edge_px + 3 positions in it, or A == 0; with j_best
 *              the run's largest s (ties: the smallest j): 2 s(j_best) <= thres_best; 3 some j of the run with s(j) > thres_peak
 *              has |j - j_best| > peak_px; 4 not (first + edge_px < j_best < last - edge_px); else the parabola offset off of the
 *              static block on s(j_best - 1), s(j_best), s(j_best + 1), j* = (float)j_best + off, and with |lx| >= |ly|:
 *              w = ((P0x + j* lx) - cx) / fx, rho* = (a0 - w a2) / (w t2 - t0); else w = ((P0y + j* ly) - cy) / fy,
 *              rho* = (a1 - w a2) / (w t2 - t1). not (r_min <= rho* <= r_max) or D(rho*) <= 0.1: status 8. Else 1, accepted.
 *   sigma*     cs = dot / (sqrtf(g2) sqrtf(dk2)); sn2 = max(1 - cs cs, 0); st = (eps_scale (float)hw) fabsf(1 - 1 / D(rho*));
 *              sigma* = (sqrtf((eps_edge^2 + (eps_epi^2) sn2) + st^2) / fabsf(cs)) / J: the static formula with bf replaced by the
 *              local J, plus st: the patch is not rescaled, and 1 / D(rho*) is the factor by which a fronto-parallel surface is
 *              magnified in the current image (DESIGN.md §18 has the measurement that asked for this term).
 *   fusion     by the same lane, in the same launch. Without a prior: invd = rho*, sigma = sigma*, n_obs = 1. With one:
 *              s2 = sigma^2, m2 = sigma*^2: invd = (invd m2 + rho* s2) / (s2 + m2), sigma = sqrtf((s2 m2) / (s2 + m2)), n_obs
 *              saturates at 255. A pixel that is not accepted keeps its map entry; tstatus is written for every pixel.
 *   score      (diagnostic, may be NULL) s(j_best) wherever a best was taken (status 1..4, and 8 after the search), else 0.
 * vo_semidense_map_seed: a map from a static result (host planes, or all device with on_device): where status == 1
 * invd = disparity / bf, sigma = sigma_invd, n_obs = 1; elsewhere 0; tstatus = 0. Synchronous.
 * vo_semidense_temporal: one launch; key_plane (host, or device with key_on_device) has key_stride bytes per row; the map is
 * updated in place (host planes, or all device with on_device). Synchronous.
 * vo_semidense_map_points: vo_semidense_points of a map: the pixels with n_obs >= min_obs (1..255) in raster order, z = 1 / invd.
 *
 * StereoVO: vo_svo_set_semidense_temporal(svo, prm) — NULL = off — needs vo_svo_set_semidense on (any `every`) and makes its only
 * allocation (the key plane, the keyframe's mask and the map) at the first enable; with it off nothing changes, with it on the odometry's results are
 * the same bits. At a keyframe, behind the static launch on the side stream: the left level-0 plane is copied into the key
 * plane and the left slot's mask next to it, the map is seeded, the keyframe's T_wc and frame_id are kept. At every later frame until the next keyframe
 * vo_svo_result enqueues one launch on the side stream behind a fork event, with T_ck = inverseSE3(T_wc) * T_wk formed on the host
 * in float (inverseSE3: t' = ((-r0) t0 + (-r1) t1) + (-r2) t2 per row of R^T; the product: r = a0 b0, r = a_k b_k + r) from the
 * poses vo_svo_result returns; it never waits for it. The launch reads that frame's left slot, which a later ingestion is
 * ordered behind on the device. vo_svo_get_semidense_map: the planes (any may be NULL), size (0 x 0 before a keyframe), the
 * keyframe's frame_id and T_wc, n_fused = the launches since the keyframe. vo_svo_get_semidense_map_points: the map's points with
 * the left camera's K, world != 0: in the world frame. Both wait for the side stream's last launch only; VO_ERR_INVALID while a
 * frame is in flight or with the option off. Not for MonoVO or vo_batch streams. */
typedef struct {
  int hw, hh;          /* 4, 1 */
  int g_min;           /* 20 */
  float thres_best;    /* 0.95 */
  float thres_peak;    /* 0.9 */
  int peak_px;         /* 5 */
  int edge_px;         /* 2 */
  float eps_edge;      /* 0.5 */
  float eps_epi;       /* 1.0 */
  float eps_scale;     /* 3.0 */
  float z_min, z_max;  /* 3, 100 [m] */
  int max_search;      /* 128 */
  float j_min;         /* 16 */
} vo_semidense_temporal_params;
int vo_semidense_temporal_default_params(vo_semidense_temporal_params *prm);
int vo_semidense_map_seed(vo_ctx *ctx, const float *disparity, const float *sigma_invd, const uint8_t *status, int width, int height,
                          float bf, float *invd, float *sigma, uint8_t *n_obs, uint8_t *tstatus, int on_device);
int vo_semidense_temporal(vo_ctx *ctx, const uint8_t *key_plane, int key_stride, int key_on_device, int slot_cur, const float K[4],
                          const float T_ck[16], const vo_semidense_temporal_params *prm, float *invd, float *sigma, uint8_t *n_obs,
                          uint8_t *tstatus, float *score, int on_device);
int vo_semidense_map_points(vo_ctx *ctx, const float *invd, const float *sigma, const uint8_t *n_obs, int width, int height,
                            int planes_on_device, const float K[4], const float *T, int min_obs, int cap, float *xyz, float *sigma_out,
                            uint16_t *pixel, int *n);
int vo_svo_set_semidense_temporal(vo_svo *svo, const vo_semidense_temporal_params *prm);
int vo_svo_get_semidense_map(vo_svo *svo, float *invd, float *sigma, uint8_t *n_obs, uint8_t *tstatus, int *width, int *height,
                             int *frame_id, float T_wc[16], int *n_fused);
int vo_svo_get_semidense_map_points(vo_svo *svo, int world, int min_obs, int cap, float *xyz, float *sigma, uint16_t *pixel, int *n,
                                    int *frame_id);

/* ---- Semi-dense propagation: the old keyframe's fused map carried over to the new keyframe ---------------------
 * A forward warp of the map's pixels into the new keyframe's left image under the odometry's pose, with an occlusion rule, and
 * a fusion with the new pair's static result. What it gains is coverage and continuity — pixels static refuses, n_obs >= 2 and
 * narrowed variances survive the keyframe change — not precision on the pixels static measures itself (§19 has the figures).
 * Only + - x / sqrtf floorf fabsf in float32, every operation rounded on its own (no FMA), in the order written here.
 * tests/semidense_propagate_restatement.py restates it.
 *   inputs     the old map: three W x H planes invd f32, sigma f32, n_obs u8, and the old keyframe's left level-0 u8 plane La;
 *              the new keyframe's left plane Lb (a slot's level 0), 3 <= W, H <= 65535, W H < 2^31, and the ignore mask bound to
 *              that slot, if any; the new pair's static planes disparity, sigma_invd, status and bf > 0; K = fx, fy, cx, cy;
 *              T_ba row-major 4 x 4, X_b = R X_a + t.
 *   params     min_obs 1..255; max_diff 0..255 (255: no gate); chi > 0; sigma_add >= 0 [1/m], all finite.
 *   source     every pixel (x, y) of the old map, raster index i = y W + x, with n_obs >= min_obs, sigma > 0 and invd > 0. With
 *              xc, yc, u, v, a_i as in the temporal block: D = a2 + invd t2. not (D > 0.1): dropped. invd_b = invd / D;
 *              p = (fx ((a0 + invd t0) / D) + cx, fy ((a1 + invd t1) / D) + cy); sigma_w = (sigma fabsf(a2)) / (D D) (the
 *              derivative of invd / (a2 + invd t2)); sigma_b = sqrtf(sigma_w sigma_w + sigma_add sigma_add). A source whose invd_b
 *              or sigma_b is not in (0, FLT_MAX] is dropped (so that the new map's entries are sources again, and NaN never
 *              enters it).
 *   target     X = (int)floorf(p_x + 0.5f) where that value lies in [-2^20, 2^22], else -2^20; Y likewise. The source is kept
 *              where, tested in this order, 1 <= X <= W-2 and 1 <= Y <= H-2; the mask byte at (X, Y) is not 0;
 *              |La(x, y) - Lb(X, Y)| <= max_diff as integers.
 *   occlusion  among the sources kept for one target the largest invd_b (the nearest) wins; on equal bits the smallest i. This
 *              is a property of the set of sources, not of any order of arrival.
 *   resolve    per pixel j of the new map, static where status == 1 with rho_s = disparity / bf, sig_s = sigma_invd (as
 *              vo_semidense_map_seed forms them):
 *                neither            invd = sigma = 0, n_obs = 0, origin 0
 *                static only        rho_s, sig_s, n_obs = 1, origin 1
 *                winner only        invd_b, sigma_b, the source's n_obs, origin 2
 *                both               dd = invd_b - rho_s, s2 = sigma_b sigma_b, m2 = sig_s sig_s, sum = s2 + m2. Consistent where
 *                                   sum > 0 and dd dd <= (chi chi) sum: the temporal block's product with the winner as the prior,
 *                                   invd = (invd_b m2 + rho_s s2) / sum, sigma = sqrtf((s2 m2) / sum), n_obs = min(n_obs + 1, 255),
 *                                   origin 3. Else the fresh measurement replaces the stale one: rho_s, sig_s, n_obs = 1, origin 4.
 *              tstatus = 0 everywhere. origin u8 and src i32 (the winner's i, -1 where there is none) are diagnostic planes.
 * vo_semidense_map_propagate: the operator, synchronous. old_* and key_plane (key_stride bytes per row), the static planes and
 * the outputs are host planes, or all device planes with on_device; the new planes may not be the old ones (resolve reads the
 * old map while it writes the new one). origin and src may be NULL. The planes may not exceed vo_config.max_width x max_height.
 *
 * StereoVO: vo_svo_set_semidense_propagate(svo, prm) — NULL = off — needs vo_svo_set_semidense_temporal on and makes its only
 * allocation (the plane of keys, a second set of map planes, origin) at the first enable; VO_ERR_INVALID while a frame is in
 * flight or on a mono driver. With it off nothing changes; with it on the odometry's results are the same bits. At a keyframe
 * that has a predecessor since the option was switched on, T_ba = inverseSE3(T_wc_new) * T_wk_old is formed on the host as the
 * temporal block forms T_ck, and on the side stream behind the static launch: the scatter (old map, old key plane, the new left
 * slot's level 0 and mask), the key-plane and mask copies, the resolve in place of the seed; then the map sets are swapped. The
 * first keyframe, and the first after the option (or the temporal one) was off, seed the map from the static result alone — the
 * same values as without the option, origin 0 / 1. The map is not re-anchored when the local BA moves a keyframe.
 * vo_svo_get_semidense_origin: the map's origin plane (may be NULL), size (0 x 0 before the first keyframe since the option was
 * switched on), from_frame_id = the frame_id
 * of the keyframe the map was propagated from, -1 where it was seeded without a predecessor; waits for the side stream's last
 * launch only; VO_ERR_INVALID while a frame is in flight or with the option off. Not for MonoVO or vo_batch streams. */
typedef struct {
  int min_obs;      /* 1 */
  int max_diff;     /* 30 */
  float chi;        /* 3.0 */
  float sigma_add;  /* 0.01 */
} vo_semidense_propagate_params;
int vo_semidense_propagate_default_params(vo_semidense_propagate_params *prm);
int vo_semidense_map_propagate(vo_ctx *ctx, const float *old_invd, const float *old_sigma, const uint8_t *old_n_obs, const uint8_t *key_plane,
                               int key_stride, int slot_new, const float *disparity, const float *sigma_invd, const uint8_t *status, float bf,
                               const float K[4], const float T_ba[16], const vo_semidense_propagate_params *prm, float *invd, float *sigma,
                               uint8_t *n_obs, uint8_t *tstatus, uint8_t *origin, int32_t *src, int on_device);
int vo_svo_set_semidense_propagate(vo_svo *svo, const vo_semidense_propagate_params *prm);
int vo_svo_get_semidense_origin(vo_svo *svo, uint8_t *origin, int *width, int *height, int *from_frame_id);

/* ---- Semi-dense alignment: a left image aligned photometrically against the keyframe's semi-dense map ----------
 * The step LSD-SLAM and SVO take: inverse compositional Gauss-Newton on level 0 over the map's pixels, from a start that is already
 * close (the odometry's pose); no pyramid, so the basin is a few pixels wide. It yields a second pose estimate, independent of the
 * feature tracks, with its residual statistic and 6 x 6 normal matrix. float32 + - x / floorf sqrtf, every operation rounded on its
 * own (no FMA), in the order written here; the Jacobian entries, weights and residuals are integers and their sums exact, the
 * solve is float64 in a written order. tests/semidense_align_restatement.py restates it.
 *   inputs     Lk: the keyframe's left level-0 u8 plane; Lc: the current left plane (a slot's level 0), both W x H, 3 <= W, H <=
 *              65535, W H < 2^31; the map's planes invd f32, sigma f32, n_obs u8; K = fx, fy, cx, cy; the start T_ck row-major
 *              4 x 4, X_c = R X_k + t (rows 0..2 are read; row 3 is 0 0 0 1).
 *   params     min_obs 1..255; 0 < huber <= 255 [grey levels]; max_iters 1..32; eps >= 0; min_pixels >= 6.
 *   pixel set  (x, y), raster index i = y W + x, with n_obs >= min_obs, sigma > 0, invd > 0, 1 <= x <= W-2, 1 <= y <= H-2. No mask is
 *              consulted: the map respects the keyframe's.
 *   constants  gx = Lk(x+1, y) - Lk(x-1, y), gy = Lk(x, y+1) - Lk(x, y-1) (integers, as the static block forms them); Z = 1 / invd,
 *              u = ((float)x - cx) / fx, v = ((float)y - cy) / fy, X = u Z, Y = v Z; fu = fx u, fv = fy v;
 *                Ju = (fx invd, 0, -(fu invd), -(fu v), fx + fu u, -(fx v))    (the derivative of the pixel column by xi = (v, omega),
 *                Jv = (0, fy invd, -(fv invd), -(fy + fv v), fv u, fy u)        the order of se3Exp_f, at xi = 0)
 *              J_i = 0.5 ((float)gx Ju_i + (float)gy Jv_i) — 0.5: the central difference spans two pixels;
 *              q_i = (int)floorf(16 J_i + 0.5f). A pixel with a non-finite X, Y, Z or 16 J_i, or any |16 J_i| >= 2^22, is dropped.
 *   iteration  with R, t of the current T: X_c = ((R[i][0] X + R[i][1] Y) + R[i][2] Z) + t_i. not (Z_c > 0.1): the pixel is out for
 *              this iteration. p = (fx (X_c / Z_c) + cx, fy (Y_c / Z_c) + cy), sampled as the temporal block samples a tap (1/32
 *              pixel, the integer inside test before any load, the 12-bit value 0..4080); not inside: out. r = sample - 16 Lk(x, y),
 *              an integer in 1/16 grey level. kq = (int)floorf(16 huber + 0.5f); w = 256 where |r| <= kq, else (256 kq) / |r| by
 *              integer division (Huber's weight in 1/256).
 *   sums       30 integers held in int64: the 21 sums of w q_i q_j (i <= j, row by row), the 6 of w q_i r, sum w r^2, sum w and
 *              the count of pixels that are not out — per block of 1024 consecutive raster indices, a constant of the definition
 *              and not of any launch. Bound: w <= 2^8, |q_i| <= 2^22, |r| < 2^12, 2^10 pixels: a block's sum stays below
 *              2^8 2^44 2^10 = 2^62. (With the 2^23 of a 24-bit mantissa the bound would be 2^64: hence 2^22.) Inside a block
 *              the sums are exact, so their order is free. The blocks' sums are converted to f64 and added in block order,
 *              block 0 first, then scaled by exact powers of two: H = 2^-16 sum w q_i q_j, b = 2^-16 sum w q_i r.
 *   solve      count < min_pixels: status 2. H xi = b by LDL^T in f64, for j = 0..5: d_j = H_jj - sum_k<j (L_jk L_jk) d_k (k
 *              ascending, one subtraction per k); not (0 < d_j <= DBL_MAX) or not (d_j > 2^-20 H_jj): status 3;
 *              L_ij = (H_ij - sum_k<j (L_ik L_jk) d_k) / d_j. (d_j / H_jj is the share of column j the columns before it do not
 *              explain. A map of one image row at one depth leaves 1e-9 .. 4e-8 of the rotation about x next to the translation
 *              along y, passes a test on the sign alone and walks metres away; the test stream's maps, crops of 31 x 29 included,
 *              stay above 2e-4. 2^-20 is also where the entries' own rounding to 1/16 ends: |q| <= 2^22 with an error of 1/2.)
 *              y_i = b_i - sum_k<i L_ik y_k; x_i = y_i / d_i - sum_k>i L_ki x_k (k ascending), i = 5..0. A non-finite x: status 3.
 *   update     T <- T exp(-xi), xi = (float)x: the exponential is geometry::se3Exp_f as the pose-only BA's kernel evaluates it
 *              (float32; the three coefficients through float64, below 0.25 rad by the Taylor series written in
 *              csrc/semidense_align_device.hpp), the product in the temporal block's order (r = a0 b0, r = a_k b_k + r). Then stop
 *              with status 0 where ((((x0^2 + x1^2) + x2^2) + x3^2) + x4^2) + x5^2 < (double)eps (double)eps, in f64 (the square of
 *              a float is exact); with status 1 after max_iters iterations. After status 2 or 3 T is the pose they were met at.
 *              The samples sit on a 1/32 pixel grid, so the cost is piecewise constant in T: the iteration ends in a fixed point
 *              or in a small cycle (steps of 1e-6 .. 2e-5 on the 640 x 240 test stream). eps = 1e-4 (0.1 mm, 0.006 degrees) lies
 *              above that floor and below the quantum itself: 1/32 pixel of a point 3 m away is 0.25 mm at fx = 370.
 *   result     T_ck, status, iters; from the last evaluated system: count, rms = sqrt(sum w r^2 / sum w) / 16 [grey levels] (0
 *              where sum w = 0), H (21 entries, the upper triangle row by row) and b. H is what a caller turns into an
 *              information matrix (divide by a residual variance in grey levels squared).
 * vo_semidense_align: the operator, synchronous: at most max_iters launches, back to back without a host turn. key_plane (host,
 * or device with key_on_device) has key_stride bytes per row; the map's planes are host planes, or all device planes with
 * on_device; they are not modified. The planes may not exceed vo_config.max_width x max_height.
 *
 * StereoVO: vo_svo_set_semidense_align(svo, prm) — NULL = off — needs vo_svo_set_semidense_temporal on and makes its only allocation
 * (the state block and the blocks' partial sums) at the first enable; VO_ERR_INVALID while a frame is in flight or on a mono driver.
 * With it off nothing changes; with it on the odometry's results, the semi-dense results and the map are the same bits. At every
 * frame that is not a keyframe and has a keyframe map, vo_svo_result enqueues the launches on the side stream IN FRONT OF that
 * frame's temporal launch, with the T_ck the temporal launch gets as the start: the alignment reads the map fused through the
 * previous frame. It never waits for them. vo_svo_get_semidense_align: the last frame's result, T_wc = T_wk inverseSE3(T_ck) formed
 * on the host in float (may be NULL), that frame's id and the keyframe's; at a keyframe frame (and before the first frame)
 * status = VO_SEMIDENSE_ALIGN_NONE, key_frame_id = -1, the poses are the identity. It waits for the side stream's last launch only;
 * VO_ERR_INVALID while a frame is in flight or with the option off. The aligned pose is not fed back anywhere. Not for MonoVO or
 * vo_batch streams. */
enum { VO_SEMIDENSE_ALIGN_CONVERGED = 0, VO_SEMIDENSE_ALIGN_MAX_ITERS = 1, VO_SEMIDENSE_ALIGN_FEW_PIXELS = 2, VO_SEMIDENSE_ALIGN_SINGULAR = 3,
       VO_SEMIDENSE_ALIGN_NONE = 4 };
typedef struct {
  int min_obs;     /* 1 */
  float huber;     /* 10.0 [grey levels] */
  int max_iters;   /* 10 */
  float eps;       /* 1e-4 */
  int min_pixels;  /* 100 */
} vo_semidense_align_params;
typedef struct {
  float T_ck[16];
  int status, iters, count;
  double rms;
  double H[21], b[6];
} vo_semidense_align_result;
int vo_semidense_align_default_params(vo_semidense_align_params *prm);
int vo_semidense_align(vo_ctx *ctx, const uint8_t *key_plane, int key_stride, int key_on_device, int slot_cur, const float K[4],
                       const float T_ck[16], const vo_semidense_align_params *prm, const float *invd, const float *sigma, const uint8_t *n_obs,
                       int on_device, vo_semidense_align_result *result);
int vo_svo_set_semidense_align(vo_svo *svo, const vo_semidense_align_params *prm);
int vo_svo_get_semidense_align(vo_svo *svo, vo_semidense_align_result *result, float T_wc[16], int *frame_id, int *key_frame_id);

/* ---- Semi-dense alignment on a map pyramid: the block above, coarse to fine ----------
 * The level-0 block converges from a few pixels; run level by level on the images' pyrDown pyramids and a pyramid of the map it
 * converges from a frame's motion and more (from the identity, 0.8 - 2.4 m off on the 640 x 240 test stream) and ends where the
 * level-0 block ends from a close start. tests/semidense_align_pyr_restatement.py restates both parts.
 *   level sizes  the slot pyramid's: W_0 = W, W_(l+1) = (W_l + 1) / 2, the same for H.
 *   map pyramid  level l + 1 from level l's RESULT (not from level 0). cv::pyrDown centres the coarse pixel (X, Y) on the finer
 *              pixel (2X, 2Y): its children are the 3 x 3 finer cells (2X + dx, 2Y + dy) that lie inside the finer plane, visited
 *              dy = -1, 0, 1 outer, dx = -1, 0, 1 inner. A child counts iff n_obs >= 1, sigma > 0, invd > 0 and both are finite.
 *              float32, every operation rounded on its own, no FMA: per counted child w = 1 / (sigma sigma), S = S + w,
 *              N = N + w invd (S = N = 0 at the start). With n counted children, n >= 1 and 0 < S <= FLT_MAX:
 *              invd = N / S, sigma = sqrtf((float)n / S) — the children's weighted-mean variance, not the fused one: neighbours
 *              are not independent measurements —, n_obs = the largest counted child's n_obs. Otherwise all three are 0.
 *   params     the level-0 block's five; levels 1..6; max_iters_level[l] 0..32 for l < levels: a level's iterations, 0 = max_iters.
 *              Every used level exists in both slots (VO_ERR_INVALID otherwise) and has W_l, H_l >= 3 (VO_ERR_SIZE).
 *   levels     for l = levels - 1 down to 0 the level-0 block's definition verbatim — pixel set, blocks of 1024 raster indices of
 *              THAT level's plane, integer sums, the f64 block order, LDL^T, the 2^-20 pivot, update and stop — applied to level l
 *              of the key slot's and the current slot's pyramid, level l of the map pyramid, K_l = (fx, fy, cx, cy) 2^-l (exact;
 *              pyrDown's centre alignment: x_l = 2^-l x_0) and the pose the level above left (the top level: the start). After
 *              status 0 or 1 a level hands its pose down; after status 2 or 3 the pose that status was met at, and the next level
 *              runs all the same. Translations are metric at every level, so the pose needs no rescaling.
 *   result     level 0's T_ck, status, iters, count, rms, H, b — with levels = 1 every one of them is vo_semidense_align's, bit for
 *              bit — and status, iters, count, rms per level (index = level); start_prev (StereoVO only, below).
 * vo_semidense_map_pyramid: levels 1 .. levels - 1 of a w x h map, each plane kind into ONE tightly packed buffer, level 1 first
 * (vo_semidense_map_pyramid_size: its elements). One launch per level. Host planes, or all device planes with on_device. 2 <= levels
 * <= 6; the planes may not exceed vo_config.max_width x max_height.
 * vo_semidense_align_pyr: the operator, synchronous: the map pyramid's launches, then per level at most its iterations' launches,
 * back to back without a host turn (a launch that finds its level done returns at once). Both images are slots; the map's level-0
 * planes are host planes or, with on_device, device planes; they are not modified.
 *
 * StereoVO: vo_svo_set_semidense_align_pyr(svo, prm, start) — NULL = off — needs vo_svo_set_semidense_temporal on; it replaces
 * vo_svo_set_semidense_align's launches while it is on (either setter with NULL turns the alignment off). Its allocations are made
 * at the first enable only: the keyframe's levels 1..5 with the map pyramid's planes (one allocation) and, unless
 * vo_svo_set_semidense_align made it, the state block. VO_ERR_INVALID while a frame is in flight or on a mono driver. At a keyframe
 * the slot's levels 1 .. levels - 1 are copied next to the key plane, device to device; at every other frame the map pyramid's
 * launches and the alignment's go on the side stream in front of the frame's temporal launch. Nothing waits. With it off no launch,
 * wait, allocation or result bit differs; with it on the odometry's results, the static result and the map are the same bits.
 *   start = VO_SEMIDENSE_ALIGN_START_ODOMETRY  the T_ck the temporal launch gets, as vo_svo_set_semidense_align.
 *   start = VO_SEMIDENSE_ALIGN_START_PREVIOUS  an odometry of its own: at the first frame after a keyframe the identity; otherwise the
 *              previous frame's aligned T_ck where that frame has a result against the same keyframe with status 0 or 1 — read from
 *              the state block on the device by the top level's first launch: no host turn —, else the odometry's T_ck, which the
 *              launch carries in its arguments. result.start_prev = 1 where the previous result was used.
 * vo_svo_get_semidense_align_pyr: as vo_svo_get_semidense_align, with the per-level fields; either getter serves either setter (the
 * level-0 getter leaves the per-level fields out). The aligned pose is not fed back anywhere. */
#define VO_SEMIDENSE_ALIGN_MAX_LEVELS 6
enum { VO_SEMIDENSE_ALIGN_START_ODOMETRY = 0, VO_SEMIDENSE_ALIGN_START_PREVIOUS = 1 };
typedef struct {
  int min_obs;     /* 1 */
  float huber;     /* 10.0 [grey levels] */
  int max_iters;   /* 10: a level's iterations where max_iters_level[l] = 0 */
  float eps;       /* 1e-4 */
  int min_pixels;  /* 100 */
  int levels;      /* 4 */
  int max_iters_level[VO_SEMIDENSE_ALIGN_MAX_LEVELS]; /* 0 */
} vo_semidense_align_pyr_params;
typedef struct {
  float T_ck[16];
  int status, iters, count;
  double rms;
  double H[21], b[6];
  int levels, start_prev;
  int level_status[VO_SEMIDENSE_ALIGN_MAX_LEVELS], level_iters[VO_SEMIDENSE_ALIGN_MAX_LEVELS], level_count[VO_SEMIDENSE_ALIGN_MAX_LEVELS];
  double level_rms[VO_SEMIDENSE_ALIGN_MAX_LEVELS];
} vo_semidense_align_pyr_result;
int vo_semidense_align_pyr_default_params(vo_semidense_align_pyr_params *prm);
int vo_semidense_map_pyramid_size(int width, int height, int levels, long long *elements);
int vo_semidense_map_pyramid(vo_ctx *ctx, const float *invd, const float *sigma, const uint8_t *n_obs, int width, int height, int levels,
                             float *invd_pyr, float *sigma_pyr, uint8_t *n_obs_pyr, int on_device);
int vo_semidense_align_pyr(vo_ctx *ctx, int slot_key, int slot_cur, const float K[4], const float T_ck[16],
                           const vo_semidense_align_pyr_params *prm, const float *invd, const float *sigma, const uint8_t *n_obs, int on_device,
                           vo_semidense_align_pyr_result *result);
int vo_svo_set_semidense_align_pyr(vo_svo *svo, const vo_semidense_align_pyr_params *prm, int start);
int vo_svo_get_semidense_align_pyr(vo_svo *svo, vo_semidense_align_pyr_result *result, float T_wc[16], int *frame_id, int *key_frame_id);

/* ---- Semi-dense alignment with affine brightness: gain and offset estimated next to the pose ----------
 * The two blocks above compare raw grey levels of two images, r = sample - 16 Lk(x, y): an exposure change between the keyframe and
 * the current image biases the pose (+15 grey levels: 0.7 mm -> 8 mm on the 640 x 240 test stream, status 0 or 1 all the same) and
 * makes rms meaningless. This block estimates, jointly with the pose, a gain g and an offset o that map the KEYFRAME's grey levels
 * into the current image's exposure. It is the "Semi-dense alignment" block but for what is written here; opt-in; the blocks above
 * keep their bits. tests/semidense_align_affine_restatement.py restates it.
 *   params     the block's own, and gain0, offset0 [grey levels]: 1/8 <= gain0 <= 8, |offset0| <= 255 (VO_ERR_INVALID otherwise).
 *   state      next to T two integers: G, the gain in 2^-16, and O, the offset in 1/16 grey level. They start at
 *              G0 = (int)floorf(65536 gain0 + 0.5f), O0 = (int)floorf(16 offset0 + 0.5f).
 *   iteration  model = ((G (16 Lk(x, y)) + 2^15) >> 16) + O, formed in int64; r = sample - model, an integer in 1/16 grey level;
 *              Huber's weight from this r as above.
 *   unknowns   eight: xi, then dg and do. q_0..q_5 are the integers above, NOT scaled by the gain (the iteration converges without:
 *              DESIGN.md §22 has the iterations it costs); q_6 = 16 Lk(x, y) (0..4080), q_7 = 16: with H and b scaled as above dg
 *              multiplies the key's grey level and do comes out in grey levels.
 *   sums       47 integers held in int64 per block of 1024 raster indices: the 36 sums of w q_i q_j (i <= j, row by row over the 8
 *              columns), the 8 of w q_i r, sum w r^2, sum w and the count. Bound: G in [2^13, 2^19] and |O| <= 4080 (the update
 *              keeps them there) give model <= 8 x 4080 + 4080 and |r| <= 40800 < 2^16; w <= 2^8, |q_i| <= 2^22, 2^10 pixels:
 *              w q_i r <= 2^8 2^22 2^16 2^10 = 2^56, w q_i q_j <= 2^62 as above, w r^2 <= 2^8 2^32 2^10 = 2^50. Exact inside a
 *              block; the blocks' sums are converted to f64 and added in block order, block 0 first; H = 2^-16 sum w q_i q_j,
 *              b = 2^-16 sum w q_i r.
 *   solve      count < min_pixels: status 2. H x = b by the LDL^T above in the same written order over j = 0..7, the 2^-20 pivot
 *              test on every column: status 3; x_i for i = 7..0; a non-finite x: status 3. (The smallest d_j / H_jj on the test
 *              stream's maps: 1.3e-3 on the 97 x 45 crop.)
 *   update     in f64: G' = G + floor(65536 x_6 + 0.5), O' = O + floor(16 x_7 + 0.5). Not (2^13 <= G' <= 2^19 and |O'| <= 4080) —
 *              which a NaN fails —: status VO_SEMIDENSE_ALIGN_AFFINE_RANGE, and T, G, O stay those the iteration started with.
 *              Otherwise T <- T exp(-xi) from x_0..x_5 as above, G <- G', O <- O' (r = sample - model: raising G or O lowers r, as
 *              T exp(-xi) does along q_0..q_5, so the signs of the eight components agree). The stop test is the one above, on
 *              x_0..x_5 alone; statuses 0..4 keep their meaning. After status 2 or 3 the state is the one they were met at.
 *              At the end point G and O move by a few quanta per iteration like the pose does.
 *   pyramid    "Semi-dense alignment on a map pyramid" with this block per level: G and O are handed from level to level with the
 *              pose, after any status (grey levels do not scale with the level); every level's record keeps the G, O it left.
 *   result     T_ck, status, iters, count, rms; H (36 entries, the upper triangle of the 8 x 8 row by row) and b (8); G, O,
 *              gain = G / 65536, offset = O / 16 (doubles); levels, start_prev and the per-level fields with level_G, level_O
 *              (the level-0 operator: levels = 1).
 * vo_semidense_align_affine / vo_semidense_align_pyr_affine: vo_semidense_align's / vo_semidense_align_pyr's arguments and the
 * affine parameters (not NULL); synchronous, the same launches with the kernel of this block.
 *
 * StereoVO: vo_svo_set_semidense_align_affine(svo, affine) — NULL = off — is a modifier of whichever alignment option is on
 * (vo_svo_set_semidense_align or vo_svo_set_semidense_align_pyr; VO_ERR_INVALID with neither; turning the alignment off turns it off
 * too): the option's launches, at their place on the side stream in front of the temporal launch, run this block's kernel on a
 * state block of their own, allocated at the first enable. VO_ERR_INVALID while a frame is in flight or on a mono driver. With it off
 * no launch, allocation, wait or result bit differs; with it on the odometry's results, the static result and the map are the same
 * bits. start = VO_SEMIDENSE_ALIGN_START_PREVIOUS takes G and O from the previous frame's result wherever it takes the pose (status
 * 0 or 1, read on the device), else G0, O0 with the odometry's pose; the first frame after a keyframe starts from G0, O0. Turning
 * the modifier on or off forgets the previous frame's result: the next frame has none to start from.
 * vo_svo_get_semidense_align_affine: as vo_svo_get_semidense_align_pyr, VO_ERR_INVALID with the modifier off. While it is on, the
 * two getters above return the affine run's T_ck, status (5 included), iters, count, rms and per-level fields; their H is the 21
 * entries of the upper-left 6 x 6 and their b the first 6 — the pose's rows and columns of the 8 x 8 system, not its Schur
 * complement. Neither the pose nor the gain is fed back anywhere. Not for MonoVO or vo_batch streams. */
enum { VO_SEMIDENSE_ALIGN_AFFINE_RANGE = 5 };
typedef struct {
  float gain0;    /* 1.0 */
  float offset0;  /* 0.0 [grey levels] */
} vo_semidense_affine_params;
typedef struct {
  float T_ck[16];
  int status, iters, count;
  double rms;
  double H[36], b[8];
  double gain, offset;
  int G, O;
  int levels, start_prev;
  int level_status[VO_SEMIDENSE_ALIGN_MAX_LEVELS], level_iters[VO_SEMIDENSE_ALIGN_MAX_LEVELS], level_count[VO_SEMIDENSE_ALIGN_MAX_LEVELS];
  double level_rms[VO_SEMIDENSE_ALIGN_MAX_LEVELS];
  int level_G[VO_SEMIDENSE_ALIGN_MAX_LEVELS], level_O[VO_SEMIDENSE_ALIGN_MAX_LEVELS];
} vo_semidense_align_affine_result;
int vo_semidense_affine_default_params(vo_semidense_affine_params *prm);
int vo_semidense_align_affine(vo_ctx *ctx, const uint8_t *key_plane, int key_stride, int key_on_device, int slot_cur, const float K[4],
                              const float T_ck[16], const vo_semidense_align_params *prm, const vo_semidense_affine_params *affine,
                              const float *invd, const float *sigma, const uint8_t *n_obs, int on_device,
                              vo_semidense_align_affine_result *result);
int vo_semidense_align_pyr_affine(vo_ctx *ctx, int slot_key, int slot_cur, const float K[4], const float T_ck[16],
                                  const vo_semidense_align_pyr_params *prm, const vo_semidense_affine_params *affine, const float *invd,
                                  const float *sigma, const uint8_t *n_obs, int on_device, vo_semidense_align_affine_result *result);
int vo_svo_set_semidense_align_affine(vo_svo *svo, const vo_semidense_affine_params *affine);
int vo_svo_get_semidense_align_affine(vo_svo *svo, vo_semidense_align_affine_result *result, float T_wc[16], int *frame_id, int *key_frame_id);

/* ---- Semi-dense regularisation: outlier removal, fill and smoothing of a map over each pixel's neighbourhood ----
 * Every block above treats a map pixel on its own. This one asks whether a pixel agrees with the pixels next to it (LSD-SLAM's
 * regularizeDepthMap / regularizeDepthMapFillHoles): an entry without consistent neighbours, or with more inconsistent than
 * consistent ones, is removed; a high-gradient pixel without an entry whose neighbours agree with each other is filled; every kept
 * value is replaced by a weighted mean of its consistent neighbours. What it gains is robustness and coverage, not precision on good
 * pixels (§23 has the figures). Opt-in; it writes planes of its own and the blocks above keep their bits.
 * Only + - x / sqrtf in float32, every operation rounded on its own (no FMA), in the order written here. All sums are per pixel, over
 * the neighbours (x + dx, y + dy) in the order dy = -r .. r outer, dx = -r .. r inner, r = radius; neighbours outside the image do
 * not exist. tests/semidense_regularize_restatement.py restates it.
 *   inputs     a map: three W x H planes invd f32, sigma f32, n_obs u8, 3 <= W, H <= 65535; the keyframe's left level-0 u8 plane
 *              Lk; an optional W x H u8 ignore mask (0 = ignore).
 *   params     radius 1..3; chi > 0; dist_sigma >= 0 [1/m per pixel]; min_support 0..48; fill_min 0..48 (0: no filling);
 *              g_min 1..360; all finite (VO_ERR_INVALID otherwise).
 *   entry      a pixel with n_obs >= 1, 0 < sigma <= FLT_MAX and 0 < invd <= FLT_MAX (NaN and inf fail these tests: they never
 *              enter a sum). var = sigma sigma.
 *   stage A    fill. A candidate is a pixel that has no entry, with 1 <= x <= W-2 and 1 <= y <= H-2, whose mask byte is not 0,
 *              with gx, gy as in the static block on Lk: gx^2 + gy^2 >= g_min^2 (integers), and fill_min > 0. Over its neighbours
 *              that have an entry: w_n = 1 / var_n; S += invd_n w_n; Wt += w_n; V += var_n; cnt = their count; mean = S / Wt;
 *              vmean = V / (float)cnt. It is filled where cnt >= fill_min and EVERY counted neighbour has dd = invd_n - mean,
 *              dd dd <= (chi chi) (var_n + vmean): one neighbour off the mean refuses the fill, so that nothing is invented across a
 *              depth step. A filled pixel carries invd = mean, var = vmean, n_obs = 1. (The mean variance, not 1 / Wt: neighbouring
 *              pixels share taps — the map pyramid's stance.)
 *   stage B    over map A = the entries and the filled pixels. For a pixel c of A and every neighbour n of A, c itself included:
 *              dd = invd_n - invd_c; n is consistent where dd dd <= (chi chi) (var_c + var_n). Over the consistent ones:
 *              w_n = 1 / (var_n + (dist_sigma dist_sigma) (float)(dx^2 + dy^2)); S += invd_n w_n; Wt += w_n. Two counts over the
 *              ORIGINAL entries other than c (filled pixels vote in the mean, but neither support nor conflict): support = the
 *              consistent ones, conflict = the others. c is kept where support >= min_support and conflict <= support.
 *   outputs    four planes of their own. A kept pixel: invd_r = S / Wt, sigma_r = sqrtf(var_c) — the pixel's own: the regularised
 *              map claims no information the filter did not have —, n_obs_r = its n_obs (a filled pixel's: 1). Everything else 0.
 *              rstatus u8: 0 nothing (a filled pixel that is not kept included), 1 an entry kept and smoothed, 2 an entry removed,
 *              3 filled and kept.
 * vo_semidense_map_regularize: the operator, one launch, synchronous. The map, the mask (may be NULL) and the outputs are host
 * planes, or all device planes with on_device; key_plane (key_stride bytes per row) is a host plane, or a device plane with
 * key_on_device. No output may be an input or another output (VO_ERR_INVALID). The planes may not exceed vo_config.max_width x
 * max_height. The result is a map: vo_semidense_align*, vo_semidense_map_pyramid and vo_semidense_map_points take it.
 *
 * StereoVO: vo_svo_set_semidense_regularize(svo, prm) — NULL = off — needs vo_svo_set_semidense_temporal on and makes its only
 * allocation (the four planes) at the first enable; VO_ERR_INVALID while a frame is in flight or on a mono driver. With it off no
 * launch, allocation, wait or result bit differs; with it on the odometry's results, the static result and the map are the same
 * bits: the alignment, the propagation and the temporal search keep reading the raw map. vo_svo_result enqueues one launch on the
 * side stream behind every launch that writes the map — at a keyframe the seed or the propagation's resolve (it then reads the set
 * of planes that is current after the swap), at every other frame the temporal launch — with the key plane and the keyframe's mask
 * copy the temporal option keeps; nothing waits for it. vo_svo_get_semidense_regularized: the planes (any may be NULL), size (0 x 0
 * before the first launch since the option was switched on), the keyframe's frame_id and T_wc, n_fused as vo_svo_get_semidense_map.
 * vo_svo_get_semidense_regularized_points: as vo_svo_get_semidense_map_points, of the regularised map. Both wait for the side
 * stream's last launch only; VO_ERR_INVALID while a frame is in flight or with the option off. Not for MonoVO or vo_batch streams. */
typedef struct {
  int radius;        /* 2 */
  float chi;         /* 2.0 */
  float dist_sigma;  /* 0.01 [1/m per pixel] */
  int min_support;   /* 1 */
  int fill_min;      /* 8 */
  int g_min;         /* 20 */
} vo_semidense_regularize_params;
int vo_semidense_regularize_default_params(vo_semidense_regularize_params *prm);
int vo_semidense_map_regularize(vo_ctx *ctx, const float *invd, const float *sigma, const uint8_t *n_obs, const uint8_t *key_plane,
                                int key_stride, int key_on_device, const uint8_t *mask, int width, int height,
                                const vo_semidense_regularize_params *prm, float *invd_r, float *sigma_r, uint8_t *n_obs_r, uint8_t *rstatus,
                                int on_device);
int vo_svo_set_semidense_regularize(vo_svo *svo, const vo_semidense_regularize_params *prm);
int vo_svo_get_semidense_regularized(vo_svo *svo, float *invd, float *sigma, uint8_t *n_obs, uint8_t *rstatus, int *width, int *height,
                                     int *frame_id, float T_wc[16], int *n_fused);
int vo_svo_get_semidense_regularized_points(vo_svo *svo, int world, int min_obs, int cap, float *xyz, float *sigma, uint16_t *pixel, int *n,
                                            int *frame_id);

/* ---- Semi-dense world map: the keyframes' semi-dense maps fused into one sparse voxel table in the world frame ----
 * Every block above ends at one keyframe's map. This one adds the map of a sequence: a sparse set of voxels of edge `voxel` [m] in the
 * world frame, held in an open-addressing hash table of 2^capacity_log2 slots of 64 bytes on the device, into which a keyframe's map
 * is integrated once, when the next keyframe replaces it. A voxel keeps a weighted mean position and grey value, the number of points
 * and the number of integrations (keyframes) that reached it; "seen by k keyframes" is the filter a single cloud cannot give.
 * Opt-in; the blocks above keep their bits. float32 with every operation rounded on its own (no FMA), in the order written here, up
 * to the voxel index; every accumulator is an integer, so the order in which points arrive changes no bit of any voxel.
 * tests/semidense_world_restatement.py restates it.
 *   inputs     of one integration: a map, three W x H planes invd f32, sigma f32, n_obs u8 (the entry test is the regularisation
 *              block's); optionally the keyframe's left level-0 u8 plane Lk (key_stride bytes per row); K = fx, fy, cx, cy; T_wk
 *              row-major 4 x 4; seq, 1 for the first integration into a table (or since its last clear) and one more per call, refused
 *              calls included.
 *   params     voxel > 0 [m]; capacity_log2 10..28; min_obs 1..255; z_max > 0 [m]; all finite (VO_ERR_INVALID otherwise).
 *   point      an entry at (x, y): z = 1.0f / invd. It is SKIPPED (and counted so) where n_obs < min_obs or z > z_max. Else
 *              X = (((float)x - cx) / fx * z, ((float)y - cy) / fy * z, z) and X'[r] = (T[r][0] X + (T[r][1] Y + T[r][2] Z)) + T[r][3]
 *              as vo_semidense_map_points forms them.
 *   voxel      per axis a: u = X'[a] / voxel, i = floorf(u). Unless -2^20 <= i < 2^20 on all three axes — tested on the float, so
 *              that NaN and inf fail — the point is dropped and counted as OUT OF RANGE. q = min((int)((u - i) * 1024.0f), 1023):
 *              u - i is exact except for a negative u so close to an integer that it rounds to 1.0f, which the clamp takes.
 *              key (64 bits) = 2^63 | (i_x + 2^20) << 42 | (i_y + 2^20) << 21 | (i_z + 2^20); 0 means "empty".
 *   weight     sz = (sigma * z) * z (the depth's standard deviation), r = voxel / sz, w = r * r,
 *              wq = w >= 65535.0f ? 65536 : (uint32)w + 1.
 *   sums       per voxel, all integers: sw += wq, sx / sy / sz += wq * q_a, sg += wq * Lk(x, y) (64 bits; sg stays 0 without a
 *              plane), cnt += 1 (32 bits); kf_cnt with last_seq: old = atomicMax(&last_seq, seq), the one point that sees old < seq
 *              adds 1 to kf_cnt. Points inserted are counted.
 *   slot       home = (key * 0x9E3779B97F4A7C15 mod 2^64) >> (64 - capacity_log2), then linear probing; an empty slot is claimed with
 *              a 64-bit compare-and-swap on its key word. Which slot a voxel sits in is the one thing that depends on arrival order.
 *   refusal    all or nothing: an integration is refused as a whole where occupied + W H > 2^capacity_log2 / 2, with `occupied` the
 *              count the previous accepted integration published — decided on the device, the same in every workgroup, no host turn.
 *              A refused integration leaves every slot and every count but `refused` (+ 1) untouched; it still takes its seq. An
 *              accepted one therefore always finds a free slot within half a table; `integrations` counts the accepted ones.
 *   extraction the voxels with cnt >= min_count and kf_cnt >= min_keyframes (both >= 1) in ASCENDING KEY order (compacted on the
 *              device in arrival order, sorted on the host: the getter is not on a hot path, and may allocate device scratch the first
 *              time it needs more records than before). Per record: index i32[3]; xyz f32[3], per axis
 *              (float)(((double)i + ((double)s_a / (double)sw + 0.5) * (1.0 / 1024)) * (double)voxel), each operation rounded on its
 *              own; weight u32 = min(sw, 2^32 - 1); count = cnt; keyframes = kf_cnt; grey u8 = (sg + sw / 2) / sw (integer division);
 *              sums u64[5] = sw, sx, sy, sz, sg (the operator only). Every output may be NULL. *n = the true count, also with
 *              VO_ERR_CAPACITY (n > cap: the first cap records in key order are written).
 * vo_semidense_world_create makes the handle's one allocation (64 bytes x 2^capacity_log2: 268 MB at the default 22) on the
 * context's device; destroy it before the context. vo_semidense_world_integrate: one launch, synchronous; the map is host planes, or
 * device planes with on_device; key_plane may be NULL, a host plane, or a device plane with key_on_device. The planes may not exceed
 * vo_config.max_width x max_height (VO_ERR_SIZE). vo_semidense_world_clear empties the table and zeroes every count and seq.
 *
 * StereoVO: vo_svo_set_semidense_world(svo, prm, source) — prm NULL = off — needs vo_svo_set_semidense_temporal on and, for
 * source = VO_SEMIDENSE_WORLD_REGULARIZED, vo_svo_set_semidense_regularize; VO_ERR_INVALID otherwise, while a frame is in flight or
 * on a mono driver. Its only allocation (the table) happens at the first enable; capacity_log2 is fixed from then on, and a later
 * enable with another voxel, min_obs or z_max clears the table. With it off no launch, allocation, wait or result bit differs; with
 * it on the odometry's results, the static result, the map, the alignment and the regularised planes are the same bits. At a keyframe
 * change vo_svo_result enqueues ONE launch on the side stream that integrates the OUTGOING keyframe's map (raw, or its regularised
 * copy; with the regularised source a keyframe without such a copy is not integrated) with that keyframe's T_wc, K of the left camera
 * and key plane — in front of the propagation's scatter, the key plane's copy and the seed, which overwrite them; nothing waits for
 * it. vo_svo_semidense_world_flush integrates the CURRENT keyframe's map now (the end of a sequence) and marks it, so that the next
 * keyframe change does not integrate it again. vo_svo_get_semidense_world_points / _stats wait for the side stream's last launch
 * only; vo_svo_semidense_world_clear empties the table. All: VO_ERR_INVALID while a frame is in flight or with the option off.
 *
 * Out of scope: re-anchoring voxels after the local BA moves a keyframe (since added: DESIGN §25, the block below; without that option
 * a keyframe stays integrated with the pose it had when it was replaced); free-space carving (since added: DESIGN §26, the block below that) and the removal of moving objects; a TSDF, surfaces or meshes; growing or rehashing the table; a
 * tighter refusal bound than W H; streaming the map out in tiles; MonoVO and vo_batch streams; any use of the map in the odometry.
 * With vo_svo_set_semidense_propagate on a propagated pixel re-enters every keyframe that carries it, so kf_cnt counts carried
 * surfaces too: min_keyframes then asks for less than independent confirmation. */
typedef struct {
  float voxel;        /* 0.10 [m] */
  int capacity_log2;  /* 22 */
  int min_obs;        /* 2 */
  float z_max;        /* 40 [m] */
} vo_semidense_world_params;
typedef struct {
  unsigned long long occupied, capacity, integrations, refused, inserted, skipped, out_of_range;
} vo_semidense_world_info;
enum { VO_SEMIDENSE_WORLD_RAW = 0, VO_SEMIDENSE_WORLD_REGULARIZED = 1, VO_SEMIDENSE_WORLD_DENSE = 2, VO_SEMIDENSE_WORLD_MERGED = 3 };  /* 2, 3: "Semi-dense map merge" */
typedef struct vo_semidense_world vo_semidense_world;
int vo_semidense_world_default_params(vo_semidense_world_params *prm);
int vo_semidense_world_create(vo_ctx *ctx, const vo_semidense_world_params *prm, vo_semidense_world **wm);
void vo_semidense_world_destroy(vo_semidense_world *wm);
int vo_semidense_world_clear(vo_semidense_world *wm);
int vo_semidense_world_integrate(vo_semidense_world *wm, const float *invd, const float *sigma, const uint8_t *n_obs,
                                 const uint8_t *key_plane, int key_stride, int key_on_device, int width, int height, int on_device,
                                 const float K[4], const float T_wk[16]);
int vo_semidense_world_stats(vo_semidense_world *wm, vo_semidense_world_info *info);
int vo_semidense_world_points(vo_semidense_world *wm, int min_count, int min_keyframes, int cap, int32_t *index, float *xyz,
                              uint32_t *weight, uint32_t *count, uint32_t *keyframes, uint8_t *grey, uint64_t *sums, int *n);
int vo_svo_set_semidense_world(vo_svo *svo, const vo_semidense_world_params *prm, int source);
int vo_svo_semidense_world_flush(vo_svo *svo);
int vo_svo_semidense_world_clear(vo_svo *svo);
int vo_svo_get_semidense_world_stats(vo_svo *svo, vo_semidense_world_info *info);
int vo_svo_get_semidense_world_points(vo_svo *svo, int min_count, int min_keyframes, int cap, int32_t *index, float *xyz,
                                      uint32_t *weight, uint32_t *count, uint32_t *keyframes, uint8_t *grey, int *n);

/* ---- Semi-dense world map: removal and re-anchoring -----------------------------------------------------------------
 * Every accumulator of the table above is an integer, so an integration can be taken out again EXACTLY and put back under another
 * pose: afterwards every live voxel holds the bits it would hold had the map been integrated with the new pose in the first place —
 * no float drift, no dependence on arrival order. tests/semidense_world_reanchor_restatement.py restates it.
 *   removal    of one earlier integration, given the SAME planes, K, T_wk, key plane and parameters: the points, keys, q, wq and grey
 *              are those of the integration (the same text forms them). It takes a seq of its own, like an integration.
 *   lookup     home slot and linear probing as above, but the key words are only READ, never compare-and-swapped: a probe that
 *              meets key 0 ends, the point is counted as MISSING and nothing is subtracted. Otherwise the point counts as REMOVED.
 *   sums       sw, sx, sy, sz, sg get the two's complement added (0 - v modulo 2^64), cnt gets 0u - c; kf_cnt with last_seq:
 *              old = atomicMax(&last_seq, seq), the one arrival that sees old < seq adds 0u - 1u. Removing what was never integrated
 *              into a voxel that exists wraps its sums: the caller's business, as is removing twice.
 *   vacated    a voxel whose cnt reaches 0 KEEPS its key, so that the probe chains of its neighbours stay intact. The extraction
 *              skips it (min_count >= 1); `occupied` keeps meaning "claimed slots", and a removal never changes it. `vacant` is the
 *              number of slots with key != 0 and cnt == 0, counted by a small launch of its own when the statistics are asked for.
 *              A later integration that reaches a vacated voxel finds its slot and fills it again.
 *   refusal    all or nothing, by the integration's own test on the same word: occupied + W H > 2^capacity_log2 / 2. A refused
 *              removal touches `refused_removals` (+ 1) only (and takes its seq). A removal and the integration enqueued behind it
 *              therefore decide alike, without a host turn.
 *   re-anchor  vo_semidense_world_reanchor(planes, K, T_old, T_new): where the first 12 floats of the two poses have equal BITS,
 *              *moved = 0, no launch, no seq. Otherwise *moved = 1 and it enqueues the removal with T_old, then the integration
 *              above with T_new, back to back (two seqs); both poses are validated before either launch. `integrations`,
 *              `inserted`, `skipped` and `out_of_range` of vo_semidense_world_info therefore count re-integrations too.
 *   counters   vo_semidense_world_reanchor_info: removals (accepted), refused_removals, removed and missing (points), reanchors
 *              (calls that enqueued their pair, refused pairs included), vacant. vo_semidense_world_info keeps its layout; clear
 *              zeroes these too.
 * vo_semidense_world_remove takes the arguments of _integrate and is synchronous like it. The launch has the integration's geometry
 * (ceil(W H / 1024) workgroups of 256) and its pre-aggregated shape: one global update per distinct voxel of a workgroup.
 *
 *
 * StereoVO: vo_svo_set_semidense_world_reanchor(svo, on, min_move) — needs vo_svo_set_semidense_world on and vo_svo_params.local_ba;
 * VO_ERR_INVALID otherwise, with a negative or non-finite min_move, while a frame is in flight or on a mono driver. Without it a
 * keyframe's map stays in the table with the pose it had when the next keyframe replaced it, while the local BA goes on moving that
 * keyframe for as long as it sits in the window: vo_svo_get_keyframes publishes the current poses, the world map the stale ones. With
 * it the map follows. The first enable makes the option's one allocation, a ring of kf_window places of 10 bytes per pixel of
 * max_width x max_height (invd f32, sigma f32, n_obs u8, the key plane u8). Wherever the driver integrates a keyframe's map (the
 * keyframe change, the flush) it first copies what it integrates into a free place, device to device on the side stream in front of
 * everything that overwrites the outgoing map, and records an ANCHOR: the keyframe's frame_id, its index among vo_svo_get_keyframes'
 * keyframes and the pose the map goes in with, the "applied" pose. The integration itself is unchanged. In vo_svo_result of a
 * keyframe frame, behind that frame's integration on the side stream, every anchor whose keyframe is still in the window is re-anchored
 * from its applied pose to the keyframe's current one where their first 12 floats differ in bits and
 *   move = max_r |dt_r| + z_max * max_r sum_c |dR_rc| >= min_move * voxel   (in double, from the two float poses; min_move in voxels,
 * 0: any difference), and the current pose becomes the applied one. Nothing waits. An anchor whose keyframe has left the window is
 * frozen and its place reused. The device decides whether a pair is refused; a refused pair leaves the map where it was, so the next
 * call of vo_svo_get_semidense_world_stats, _anchors or _reanchor_stats — refused_removals comes with the counters they fetch, no
 * copy or wait of its own; _points does not look — gives the anchor its previous pose back (a table never gets emptier and the
 * driver's maps have one size, so the refused pairs are the last ones enqueued). The invariant: after one of these three the
 * table holds the bits of a fresh table fed, in order, every anchor's map with its applied pose. With min_move 0 every applied pose
 * equals the keyframe's pose of vo_svo_get_keyframes to the bit. vo_svo_get_semidense_world_anchors returns the anchors in
 * integration order (*n the true count, VO_ERR_CAPACITY where n > cap; every output may be NULL; in_window: the keyframe is still
 * in the window), vo_svo_get_semidense_world_reanchor_stats the counters above. vo_svo_semidense_world_clear forgets the anchors.
 * While the option is off integrated maps get no anchor. With it off no launch, allocation, wait or result bit differs; with it on
 * the odometry, every semi-dense result and the keyframe poses keep every bit.
 *
 * Out of scope: a fused remove-and-add launch; a compact per-keyframe point list instead of retained planes; reclaiming vacated
 * slots or rehashing; re-anchoring the per-keyframe map, the propagation or the alignment; re-anchoring keyframes that have left the
 * window; MonoVO and vo_batch; any use of the map in the odometry. */
typedef struct {
  unsigned long long removals, refused_removals, removed, missing, reanchors, vacant;
} vo_semidense_world_reanchor_info;
int vo_semidense_world_remove(vo_semidense_world *wm, const float *invd, const float *sigma, const uint8_t *n_obs,
                              const uint8_t *key_plane, int key_stride, int key_on_device, int width, int height, int on_device,
                              const float K[4], const float T_wk[16]);
int vo_semidense_world_reanchor(vo_semidense_world *wm, const float *invd, const float *sigma, const uint8_t *n_obs,
                                const uint8_t *key_plane, int key_stride, int key_on_device, int width, int height, int on_device,
                                const float K[4], const float T_old[16], const float T_new[16], int *moved);
int vo_semidense_world_reanchor_stats(vo_semidense_world *wm, vo_semidense_world_reanchor_info *info);
int vo_svo_set_semidense_world_reanchor(vo_svo *svo, int on, float min_move);
int vo_svo_get_semidense_world_anchors(vo_svo *svo, int cap, int32_t *frame_id, int32_t *kf_index, float *T_wk, int32_t *in_window, int *n);
int vo_svo_get_semidense_world_reanchor_stats(vo_svo *svo, vo_semidense_world_reanchor_info *info);

/* ---- Semi-dense world map: free-space carving -----------------------------------------------------------------------
 * The two blocks above only ever add evidence that something is there. This one adds the complement of a hit: a voxel that a
 * keyframe's ray has passed through on its way to a surface behind counts as SEEN TO BE EMPTY, in a 32-bit count `free` per voxel —
 * the word of the 64-byte slot that was padding. It is an integer like every other accumulator, so it is as independent of arrival
 * order and as reproducible to the bit. Opt-in; with it off no launch, allocation, wait or result bit differs, with it on every other
 * field of every voxel keeps its bits. float32, every operation rounded on its own (no FMA), in the order written here.
 * tests/semidense_world_carve_restatement.py restates it.
 *   inputs     of one carve: a map (invd, sigma, n_obs, W x H), K and T_wk exactly as vo_semidense_world_integrate takes them, without a
 *              key plane. The table supplies voxel, min_obs and z_max.
 *   params     vo_semidense_world_carve_params: margin [voxels] 2.0, >= 1; chi 3.0, >= 0; z_near [m] 0.5, > 0; all finite
 *              (VO_ERR_INVALID otherwise).
 *   ray        a pixel casts a ray where it passes the integration's entry test and is not SKIPPED (n_obs >= min_obs, z <= z_max,
 *              z = 1.0f / invd) — whether or not its own point was out of range. sz = (sigma * z) * z, m = fmaxf(margin * voxel,
 *              chi * sz), z_end = z - m, dz = voxel * 0.5f.
 *   samples    the k in 1 .. 4096 with z_k = (float)k * dz, z_near <= z_k and z_k < z_end. 4096 is a constant of the definition: a
 *              longer ray is carved over its near part only. A ray with no sample is counted as a SHORT ray.
 *   position   sdw_point's text with z_k in the place of z: X = ((float)x - cx) / fx * z_k, Y = ((float)y - cy) / fy * z_k,
 *              X'[r] = (T[r][0] X + (T[r][1] Y + T[r][2] z_k)) + T[r][3], per axis i = floorf(X' / voxel) with the integration's range
 *              test and key. A sample with any axis out of range has key_k = 0.
 *   visit      sample k is a VISIT where key_k != 0 and either k is the ray's first sample or key_k != key_{k-1}. A line meets a cube
 *              in one interval, so suppressing consecutive duplicates is all the de-duplication a ray needs; the definition is the
 *              consecutive rule itself, whatever rounding does.
 *   lookup     the removal's: home slot, then linear probing; the key words are only read. A probe that meets key 0 ends with
 *              nothing done; a match is a HIT and adds 1 to the slot's `free` (32 bits, wraps). A vacated voxel (cnt == 0, key kept)
 *              collects `free` like any other: `free` belongs to the cell in space, not to an integration. The removal and the
 *              re-anchoring do not touch it (the invariant of the block above holds for every field but `free`: a re-anchor does not
 *              re-carve); clear zeroes it.
 *   no seq     a carve takes no sequence number and is never refused; it writes no key and leaves occupied, cnt, kf_cnt and last_seq
 *              alone.
 *   counters   vo_semidense_world_carve_info: carves, rays, short_rays, visits, hits. The infos above keep their layouts; clear
 *              zeroes these too.
 *   extraction vo_semidense_world_points is unchanged. vo_semidense_world_points_free returns `free` per record as well, and with
 *              free_den >= 1 keeps a voxel only where (u64)free * free_den <= (u64)cnt * free_num (free_num >= 0); free_den == 0: no
 *              filter. Key order, cap and VO_ERR_CAPACITY as above.
 * vo_semidense_world_carve is synchronous like _integrate and validates like it: a bad K, T or size touches nothing. The launch has the
 * integration's geometry (ceil(W H / 1024) workgroups of 256); the block's (ray, k) pairs are shared out over the lanes, no lane owns
 * a ray. In the default form every visit looks its voxel up itself (the simple form: hits are rare, the cost is the key reads);
 * VO_DBG_SDW_FORM = 1 selects the OTHER form of the carve, which first combines a round's visits per workgroup in an LDS hash and
 * looks every distinct voxel up once. Both leave the same bytes.
 *
 * StereoVO: vo_svo_set_semidense_world_carve(svo, prm) — prm NULL = off — needs vo_svo_set_semidense_world on; VO_ERR_INVALID
 * otherwise, while a frame is in flight or on a mono driver. It allocates nothing. Wherever the driver integrates a keyframe's map (the
 * keyframe change, the flush) it enqueues the carve of the same planes with the same pose directly behind that integration on the
 * side stream: in front of whatever overwrites those planes and in front of the re-anchoring pass. Nothing waits. With it on the
 * odometry, every semi-dense result, the keyframe poses and every other field of every voxel keep their bits.
 *
 * Out of scope: voxels for free space, an occupancy or TSDF grid; an exact 3-D DDA (the half-voxel sampling may miss a corner cut
 * shorter than the step, by definition); re-carving on re-anchor; undoing a carve; deleting carved voxels or reclaiming their slots;
 * carving from frames that are not keyframes; MonoVO and vo_batch; any use of `free` in the odometry. */
typedef struct {
  float margin; /* 2.0 [voxels] */
  float chi;    /* 3.0 */
  float z_near; /* 0.5 [m] */
} vo_semidense_world_carve_params;
typedef struct {
  unsigned long long carves, rays, short_rays, visits, hits;
} vo_semidense_world_carve_info;
int vo_semidense_world_carve_default_params(vo_semidense_world_carve_params *prm);
int vo_semidense_world_carve(vo_semidense_world *wm, const float *invd, const float *sigma, const uint8_t *n_obs, int width, int height,
                             int on_device, const float K[4], const float T_wk[16], const vo_semidense_world_carve_params *prm);
int vo_semidense_world_carve_stats(vo_semidense_world *wm, vo_semidense_world_carve_info *info);
int vo_semidense_world_points_free(vo_semidense_world *wm, int min_count, int min_keyframes, int free_num, int free_den, int cap,
                                   int32_t *index, float *xyz, uint32_t *weight, uint32_t *count, uint32_t *keyframes, uint8_t *grey,
                                   uint64_t *sums, uint32_t *free_count, int *n);
int vo_svo_set_semidense_world_carve(vo_svo *svo, const vo_semidense_world_carve_params *prm);
int vo_svo_get_semidense_world_carve_stats(vo_svo *svo, vo_semidense_world_carve_info *info);
int vo_svo_get_semidense_world_points_free(vo_svo *svo, int min_count, int min_keyframes, int free_num, int free_den, int cap,
                                           int32_t *index, float *xyz, uint32_t *weight, uint32_t *count, uint32_t *keyframes,
                                           uint8_t *grey, uint32_t *free_count, int *n);

/* ---- undistortion / stereo rectification in front of the trackers ----------
 * core/visual_odometry/camera.cpp. A context holds the maps of two cameras
 * (cam 0 = left or the mono camera, cam 1 = right), device-resident. */
/* Camera::generateImageUndistortMaps (camera.cpp:56-90): K = fx,fy,cx,cy ; D = k1,k2,p1,p2,k3 */
int vo_rectify_init_mono(vo_ctx *ctx, int cam, int width, int height, const float K[4], const float D[5]);
/* StereoCamera::generateStereoImagesUndistortAndRectifyMaps (camera.cpp:364-546): maps of cam 0 and 1;
 * returns the rectified camera K_rect = f,f,cu,cv (getRectifiedCamera) and the rectified extrinsics
 * (getRectifiedStereoPoseLeft2Right / Right2Left; row-major 4x4; T_rl_rect may be NULL) */
int vo_rectify_init_stereo(vo_ctx *ctx, int width, int height, const float Kl[4], const float Dl[5],
                           const float Kr[4], const float Dr[5], const float T_lr[16], float K_rect[4],
                           float T_lr_rect[16], float T_rl_rect[16]);
/* caller-made maps (what cv::remap takes as map1 / map2, CV_32FC1, width x height, tightly packed) */
int vo_rectify_set_maps(vo_ctx *ctx, int cam, const float *map_u, const float *map_v, int width, int height);
int vo_rectify_get_maps(vo_ctx *ctx, int cam, float *map_u, float *map_v, int *width, int *height);
/* Where camera `cam`'s rectified image shows the source, as an ignore mask (above): cv::remap fills the rest with 0, and FAST
 * fires along the edge. valid(x, y) iff 0 <= map_u <= width - 1 and 0 <= map_v <= height - 1 (float compares; NaN is invalid);
 * out(x, y) = 255 iff every pixel of the (2 erode + 1)^2 square around it, clipped to the image, is valid, else 0. erode: 0..31.
 * out: width x height bytes, `stride` per row, host or device memory. */
int vo_rectify_validity_mask(vo_ctx *ctx, int cam, int erode, void *out, int stride, int on_device);
/* Camera::undistortImage / StereoCamera::rectifyStereoImages (camera.cpp:166-183, :300-336) +
 * convertTo(CV_8UC1) (stereo_vo.cpp:420-421, mono_vo.cpp:512), fused into the pyramid build of the slot:
 * vo_set_image* with the raw image and the camera whose map applies. The image must have the map's
 * size (VO_ERR_SIZE otherwise, as the reference throws). */
int vo_set_image_rectified(vo_ctx *ctx, int slot, const uint8_t *host, int width, int height, int stride, int cam);
int vo_set_image_rectified_device(vo_ctx *ctx, int slot, const void *dev, int width, int height, int stride,
                                  int cam);
/* left image through cam 0's map, right image through cam 1's, one launch chain */
int vo_set_stereo_pair_rectified_device(vo_ctx *ctx, int slot_l, const void *dev_l, int slot_r, const void *dev_r,
                                        int width, int height, int stride);
/* The pixel format of the images given to the three entry points above and, through them, to vo_svo_* / vo_mvo_*
 * created with rectify = 1 (synchronous call, prefetch / enqueue, run; host and device images). It is a property of the
 * context; the default is VO_PIX_MONO8, with which nothing changes. `stride` stays in BYTES for every format and need
 * not be a multiple of the sample size; `host` / `dev` point at the first byte of the image whatever its type.
 *
 * The reference's ingestion with flagDoUndistortion (camera.cpp:163-183, :300-336; stereo_vo.cpp:414-421;
 * mono_vo.cpp:509-513) takes any cv::Mat: a 3-channel image goes through cvtColor(COLOR_RGB2GRAY), any depth through
 * convertTo(CV_32FC1), cv::remap (INTER_LINEAR, BORDER_CONSTANT 0) and convertTo(CV_8UC1). Per format, one output byte is:
 *   VO_PIX_RGB8     every tap is gray = (c0*9798 + c1*19235 + c2*3735 + 16384) >> 15 of its three bytes c0 c1 c2 — OpenCV
 *                   4.5's 8-bit RGB2Gray with 15-bit coefficients, restated from memory and NOT pinned against an OpenCV
 *                   build (like every third-party restatement here). Channel 0 is weighted as R whatever
 *                   the message called it: that is what the reference's COLOR_RGB2GRAY does to a bgr8 image, so this is
 *                   the format for every 3-channel image of an unmodified node. The u8 gray taps then go through the
 *                   integer remap of VO_PIX_MONO8 unchanged (pyramid.hip / ingest_formats.hpp: remap_sample).
 *   VO_PIX_BGR8     the same with c0 and c2 exchanged. For callers who know their data; not the reference's behaviour.
 *   VO_PIX_MONO16U / VO_PIX_MONO16S / VO_PIX_F32
 *                   a tap is a float (16-bit values convert exactly). The map coordinates are quantised to 1/32 px as
 *                   for u8: fx = cvRound(map_u*32), sx = fx >> 5, ax = fx & 31 (the same for y; a NaN coordinate is far
 *                   outside). Taps outside the source are 0. Weights w00 = (32-ay)(32-ax)/1024, w01 = (32-ay)ax/1024,
 *                   w10 = ay(32-ax)/1024, w11 = ay*ax/1024, exact in float. The sum is
 *                   ((v00*w00 + v01*w01) + v10*w10) + v11*w11 with every product and every sum rounded to float on its
 *                   own (no FMA): OpenCV's scalar remapBilinear<float>. convertTo(CV_8UC1) of that sum s: NaN gives 0;
 *                   |s| >= 2^31 gives 0 (x86 cvRound returns the integer-indefinite value, the convention the
 *                   coordinates already follow — unpinned as well); anything else is rounded half to even and clamped
 *                   to [0, 255].
 * vo_set_input_format grows the context's pinned-host and device staging images to 3 (RGB8, BGR8), 2 (16-bit) or 4 (F32)
 * bytes per pixel the first time a format needs it; it is the only place that allocates for this. It returns
 * VO_ERR_INVALID for an unknown format and while a frame is in flight.
 * The entry points WITHOUT a remap — vo_set_image, vo_set_image_device, vo_set_stereo_pair_device,
 * vo_set_stereo_pair_host_async, and the drivers created with rectify = 0 — return VO_ERR_INVALID while the format is not
 * VO_PIX_MONO8: in the reference a colour image on that path reaches the trackers unconverted, there is no behaviour to
 * mirror. Undistorted colour / 16-bit / float data goes through the rectifying entry points with identity maps
 * (vo_rectify_set_maps with map_u[v][u] = u, map_v[v][u] = v: integer coordinates sample one tap with weight 1). */
enum { VO_PIX_MONO8 = 0, VO_PIX_RGB8 = 1, VO_PIX_BGR8 = 2, VO_PIX_MONO16U = 3, VO_PIX_MONO16S = 4, VO_PIX_F32 = 5 };
int vo_set_input_format(vo_ctx *ctx, int format);
int vo_get_input_format(vo_ctx *ctx, int *format);

/* ---- CLAHE equalisation in front of the ingestion ----------------------------------------------------------
 * An opt-in property of the context, off by default. While it is on, every 8-bit grey image that enters a slot — vo_set_image,
 * vo_set_image_device, vo_set_stereo_pair_device, vo_set_stereo_pair_host_async, the three *_rectified* entry points and,
 * through them, vo_svo_* / vo_mvo_* (synchronous call, enqueue / prefetch / result, run; host and device images) — is first
 * equalised as cv::createCLAHE(clip_limit, Size(tiles_x, tiles_y))->apply would, and everything downstream (the rectifying
 * remap, the pyramid, the detector, KLT / IC / the frame kernels, the debug image) reads the equalised image. The two images of
 * a pair are equalised independently. Under rectification the RAW image is equalised, then remapped: cv::remap's zero fill never
 * enters a histogram. The caller's device image is never written: the result goes into a plane per slot that the context owns.
 * With the option off no kernel, launch, allocation or result bit differs from a context that never had it.
 *
 * The arithmetic (OpenCV 4.x imgproc/src/clahe.cpp, 8-bit path; restated from knowledge of upstream and NOT pinned against an
 * OpenCV build, like every third-party restatement here), for an image w x h:
 *   extension  if w % tiles_x == 0 and h % tiles_y == 0 the histograms are taken from the image itself; otherwise from the image
 *              extended to the right by tiles_x - w % tiles_x columns and at the bottom by tiles_y - h % tiles_y rows with
 *              BORDER_REFLECT_101 — both amounts whenever either remainder is non-zero, so a dimension that divides evenly is
 *              then extended by a full tiles_x / tiles_y (upstream's behaviour). tw = w_ext / tiles_x, th = h_ext / tiles_y.
 *   per tile   the int histogram of its tw x th pixels. If clip_limit > 0: limit = max((int)(clip_limit * tw*th / 256), 1) in
 *              double; every bin above limit is cut to it, clipped = the sum of what was cut, batch = clipped / 256,
 *              residual = clipped - 256 * batch; every bin += batch; if residual != 0, step = max(256 / residual, 1) and bins
 *              0, step, 2 step, ... each += 1 until residual increments are made or the index reaches 256.
 *   table      lut[i] = saturate_cast<uchar>((float)(running sum up to bin i) * ((float)255 / (float)(tw*th))) — rounded
 *              half to even, clamped to 0..255.
 *   blend      per column x: txf = (float)x * (1.0f / tw) - 0.5f, tx1 = floor(txf), xa = txf - tx1, xa1 = 1.0f - xa (weights from
 *              the unclamped tx1), then tx2 = min(tx1 + 1, tiles_x - 1), tx1 = max(tx1, 0); rows alike with th. Per pixel of
 *              value v: res = (L[ty1][tx1][v]*xa1 + L[ty1][tx2][v]*xa)*ya1 + (L[ty2][tx1][v]*xa1 + L[ty2][tx2][v]*xa)*ya in float,
 *              every product and every sum rounded on its own (no FMA); out = saturate_cast<uchar>(res).
 *
 * vo_set_equalize: mode VO_EQ_OFF / VO_EQ_CLAHE; tiles_x, tiles_y in 1..32; clip_limit finite and >= 0 (0: no clipping);
 * anything else returns VO_ERR_INVALID and changes nothing. VO_ERR_INVALID as well while the input format is not VO_PIX_MONO8
 * (and vo_set_input_format to another format is refused while equalisation is on), and while a frame is in flight. The first call
 * that turns the option on makes every allocation of it (per slot: the plane, the tables and the histogram counters; one more
 * set for vo_equalize_image); vo_debug_allocation_count does not move on any later call or frame. At an ingestion entry point an
 * image with width <= tiles_x or height <= tiles_y returns VO_ERR_SIZE (the reflected extension needs more). The launches run on
 * the stream of the ingestion chain (vo_set_ingest_side_stream). While the option is on the drivers' synchronous call starts the
 * keypoint detection from the slot, behind the pyramid, instead of from the caller's image next to it: the same table.
 * vo_batch streams stay unequalised (their contexts are the batch's own).
 * vo_get_equalize: the current values (the defaults before any set: VO_EQ_OFF, 40.0, 8 x 8 — cv::createCLAHE's). */
enum { VO_EQ_OFF = 0, VO_EQ_CLAHE = 1 };
int vo_set_equalize(vo_ctx *ctx, int mode, double clip_limit, int tiles_x, int tiles_y);
int vo_get_equalize(vo_ctx *ctx, int *mode, double *clip_limit, int *tiles_x, int *tiles_y);
/* the operator on its own: dst = CLAHE(src) with the context's current parameters (mode must be VO_EQ_CLAHE);
 * luts may be NULL, else tiles_y*tiles_x*256 bytes, row-major by tile; src/dst/luts host (on_device 0) or device (1);
 * VO_EQ_DEVICE_TO_HOST (2): src in device memory, dst and luts in host memory. Any other value is VO_ERR_INVALID. Both strides
 * are at least the width; VO_ERR_SIZE as at ingestion. Returns when dst is written.
 * The work is queued on the context's stream behind whatever is queued there, and the call waits for it: called while a frame is
 * in flight it is correct (stream order; its staging is the operator's own, not a slot's) but returns only after that frame's
 * device work. One call at a time per context, like every other call on a vo_ctx. */
enum { VO_EQ_HOST = 0, VO_EQ_DEVICE = 1, VO_EQ_DEVICE_TO_HOST = 2 };
int vo_equalize_image(vo_ctx *ctx, const void *src, int stride, int width, int height,
                      void *dst, int dst_stride, uint8_t *luts, int on_device);

/* ---- the drivers' debug image: showTracking / showTrackingBA -----------------------------------------------------
 * Both drivers share one text for each (stereo_vo.cpp:685-688 -> showTrackingBA; mono_vo.cpp:554-555, :626-627 ->
 * showTracking, :903-904 -> showTrackingBA) and draw into img_debug_, which the ROS 1 nodes publish as bgr8
 * (stereo_vo_ros1.cpp:199-203, mono_vo_ros1.cpp:245-248). `out` is a HOST image of height x width x 3 bytes (row pitch
 * out_stride >= 3 * width) of the size of the slot's image: level 0 of `slot` replicated into the three channels
 * (CV_GRAY2RGB) with the primitives on top. Channel k receives component k of the reference's cv::Scalar, so in the
 * published bgr8 buffer (0,255,0) is green and (0,0,255) is red. Points are x y pairs in HOST memory; n <=
 * vo_config.max_points per set; a NULL set with n = 0 is an empty set.
 *   vo_draw_tracking, primitives in this order:
 *     for i < n1: the line pts0[i] -> pts1[i] in (0,255,255); n1 <= n0, VO_ERR_INVALID otherwise
 *     for each of pts0:    circle(3, 2) in (0,0,0), then circle(2, 1) in (255,0,255)
 *     for each of pts1:    circle(3, 2) in (0,0,0), then circle(2, 1) in (0,255,0)
 *     for each of pts_new: circle(3, 2) in (0,0,0), then circle(2, 1) in (255,0,0)
 *   vo_draw_tracking_ba:
 *     for each of pts:      circle(1, 4) in (0,0,255)
 *     for each of pts_proj: rect(6, 2) in (0,255,0)
 * The rasterisation is the library's OWN: it is modelled on the look of cv::line / cv::circle / cv::rectangle and is NOT
 * pixel parity with them (as §10's RANSAC is not OpenCV's). Its rules, all in integers:
 *   centre      c = (rint(x), rint(y)), halves to even. A point with a NaN coordinate or with |coordinate| >= 2^30 is
 *               skipped; a line is skipped when either of its end points is.
 *   circle(r,t) the pixels c + (dx, dy) with max(0, 2r - t)^2 <= 4 (dx^2 + dy^2) <= (2r + t)^2
 *   rect(h,t)   the pixels c + (dx, dy) with 2h - t <= 2 max(|dx|, |dy|) <= 2h + t
 *   line a -> b between the two centres: n = max(|bx - ax|, |by - ay|); the pixels
 *               (ax + floor((2k(bx - ax) + n) / (2n)), ay + floor((2k(by - ay) + n) / (2n))) for k = 0 .. n, floor
 *               division; for n = 0 the one pixel a.
 *   clipping    pixels outside the image are dropped, primitive by primitive.
 *   overlap     primitives are numbered from 0 in the order above; a pixel takes the colour of the highest-numbered
 *               primitive that covers it, else its gray value. The result does not depend on scheduling.
 * The first call allocates the context's drawing buffers (an index plane, the picture on the device and pinned). */
int vo_draw_tracking(vo_ctx *ctx, int slot, const float *pts0, int n0, const float *pts1, int n1, const float *pts_new,
                     int n_new, uint8_t *out, int out_stride);
int vo_draw_tracking_ba(vo_ctx *ctx, int slot, const float *pts, int n, const float *pts_proj, int n_proj, uint8_t *out,
                        int out_stride);

/* ---- steady-state mono frame ----------------------------------------------
 * The operator sequence of MonoVO::trackImage
 * (core/visual_odometry/mono_vo/mono_vo.cpp:739-963): prior pixel + patch scale
 * (:739-761), trackBidirectionWithPrior (:768), trackWithScale (:779-788), the
 * selection of the pose-only BA set (:799-826), poseOnlyBundleAdjustment
 * (:856-867), mask_motion (:872-879) and the Sampson gate (:954-963), chained on
 * the device. The 5-point fallback (:905-935, OpenCV calib3d) stays with the
 * caller: counts.need_five_point says when it is due (fewer than 11 BA points,
 * or the BA failed); stages then stop at 2 and dT01 is the prior. */
typedef struct {
  int width, height;
  int win, max_level;
  float thres_err, thres_bidirection;
  int thres_poseba;      /* int, as the reference's poseOnlyBundleAdjustment takes it */
  float thres_sampson;
  float K[4];
} vo_mono_params;

typedef struct {
  int n_klt, n_refine, n_ba, n_motion, n_final;
  int gn_iterations;
  int need_five_point;
  int n_replayed;
} vo_mono_counts;

/* flags[i]: bit 0 = lm->isBundled() (prior pixel and patch scale come from the
 * 3-D point), bit 1 = the landmark is in the class this frame hands to the
 * pose-only BA (mono_vo.cpp:800-826), bit 2 = VO_MONO_LM_DROPPED (fails the first
 * compaction, mono_vo.cpp:773 -> landmark.cpp:207). Xw is read only where bit 0 or 1 is set.
 * Tcw_prev = inverse pose of the previous frame, Tcw_prior = inverse of the
 * predicted current pose, dT01_prior = predicted motion (all row-major 4x4).
 * The strict-border mode is the context's (vo_stereo_frame_set_strict_border). */
int vo_mono_frame_enqueue(vo_ctx *ctx, const vo_mono_params *prm, int slot0, int slot1,
                          const float *pts0, const float *Xw, const uint8_t *flags, int n,
                          const float Tcw_prev[16], const float Tcw_prior[16],
                          const float dT01_prior[16], int inputs_on_device);
/* stage[i] = gates passed: 1 tracked, 2 refined, 3 motion inlier (or not in the
 * BA set), 4 passed the Sampson gate. pts1 = refined pixel (stage >= 2), else the
 * forward KLT result. */
int vo_mono_frame_result(vo_ctx *ctx, float *pts1, float *scale, uint8_t *stage, float dT01[16],
                         vo_mono_counts *counts, vo_gn_info *gn);
/* The mono frame with its new-point step closed on the device (MonoVO::trackImage, mono_vo.cpp:977-1001:
 * extractor_->updateWeightBin(lmtrack_final.pts1), extractORBwithBinning_fast(I1, ...), trackBidirection(I1, I0, ...)):
 * `table` holds the best keypoint of every bin of the image in slot1 (vo_new_point_candidates_enqueue, from the image
 * alone, any time before), the frame kernel back-tracks every bin's candidate, and the BA launch's epilogue emits the
 * candidates of the bins that lmtrack_final (stage 4) leaves empty — the reference's result in the reference's order.
 * When the BA gives no pose (counts.need_five_point) no new points are reported: that path is the caller's. */
int vo_mono_frame_enqueue_closed(vo_ctx *ctx, const vo_mono_params *prm, int slot0, int slot1,
                                 const float *pts0, const float *Xw, const uint8_t *flags, int n,
                                 const float Tcw_prev[16], const float Tcw_prior[16],
                                 const float dT01_prior[16], const vo_bin_params *bins, int table,
                                 int inputs_on_device);
/* After vo_mono_frame_result of a closed frame: pts1_new = the new points' pixels in I1 (bins ascending), pts0_new =
 * their back-tracked pixels in I0, mask_new = trackBidirection's mask. Capacity: n_bins_u * n_bins_v each. */
int vo_mono_frame_new_points(vo_ctx *ctx, float *pts1_new, float *pts0_new, uint8_t *mask_new, int *n_new);

/* ---- MonoVO: the closed loop around the mono frame -------------------------------------------------------------
 * MonoVO::trackImage (core/visual_odometry/mono_vo/mono_vo.cpp:496-1194, class surface mono_vo.h:235-243, :267) with the
 * track set carried ON THE DEVICE: per landmark the pixel seen, id, world point, flags (VO_LM_TRIANGULATED | VO_LM_DROPPED |
 * VO_LM_KF_MEMBER | VO_LM_BUNDLED), its first observation and frame, age, the parallax of its newest observation
 * (landmark.cpp:76-135), its first keyframe observation and their number. The first image creates one landmark per bucketed
 * keypoint (:528-561); the second is the initialisation (:562-696); then the steady state (:698-1019: prior and patch scale
 * from bundled landmarks, trackBidirectionWithPrior, trackWithScale, pose-only BA on the bundled / triangulated
 * landmarks, Sampson gate, new points back-tracked into the previous image); at the end of every call the keyframe rule
 * (keyframes.cpp:47-126), and at a keyframe addNewKeyframe (:30-45), the reconstruction of landmarks seen on more than
 * two keyframes (:1032-1076) and the mono local BA (motion_estimator.cpp:1090-1205, sparse_ba_parameters.h:292-466 with
 * one observation per keyframe and at least two window keyframes per landmark; setBundled / setDead on the way back).
 * The 5-point / essential-matrix pose (MotionEstimator::calcPose5PointsAlgorithm, motion_estimator.cpp:21-203) is a HOOK
 * (the library's own: vo_mvo_params_set_five_point + vo_five_point_*, below; or the caller's): called at the initialisation and whenever the pose-only BA
 * yields no pose (:909-949). pts0 / pts1: n pixel pairs (previous, current image); K = fx, fy, cx, cy; outputs R10
 * (row-major 3x3), t10 (any length; the driver rescales it as the reference does) and mask[n] (inliers). Return non-zero
 * on success; 0 ends the call with VO_ERR_GN_FAILED (the reference throws).
 * Needs a context with >= 3 image slots and prm.frame.win in {13, 15, 21, 31}. */
#define VO_LM_BUNDLED 8
typedef int (*vo_five_point_fn)(void *user, const float *pts0, const float *pts1, int n, const float K[4], float R10[9],
                                float t10[3], uint8_t *mask);
typedef struct vo_mvo vo_mvo;
typedef struct {
  vo_mono_params frame;     /* Camera.*, feature_tracker.* (incl. thres_sampson), motion_estimator.thres_poseba_error */
  vo_bin_params bins;       /* feature_extractor.* as FeatureExtractor::initParams derives them */
  float kf_overlap_ratio;   /* keyframe_update.thres_overlap_ratio */
  float kf_rotation_deg;    /* keyframe_update.thres_rotation (degrees) */
  float kf_translation;     /* keyframe_update.thres_translation */
  int kf_window;            /* keyframe_update.n_max_keyframes_in_window (at most 16) */
  float thres_parallax_deg; /* map_update.thres_parallax (degrees; the reference multiplies by D2R) */
  int strict_border;        /* trackWithScale's never-reset tap state: 0 masked taps; 1..4 reference-exact — 1 the replay stream-ordered
                               behind the frame kernel, 2 sequential replay only (validation), 3 the replay next to the frame
                               kernel joined on the device, 4 = 3 or 1 per frame (vo_stereo_frame_set_strict_border); same results */
  int local_ba;             /* != 0: localBundleAdjustmentSparseSolver at every keyframe */
  int rectify;              /* != 0: flagDoUndistortion (mono_vo.cpp:509-513) — images go through camera 0's undistortion
                               map (vo_rectify_init_mono first) on their way into the pyramid */
  vo_five_point_fn five_point;
  void *five_point_user;
} vo_mvo_params;
typedef struct {
  int frame_id;             /* Frame id of this image (the context's frame counter) */
  int is_first, is_init, is_keyframe, lba_ran, used_five_point;
  int n_tracks_in, n_final, n_new, n_tracks_out, n_kf_tracked, n_reconstructed;
  vo_mono_counts counts;
  vo_gn_info gn;
  float dT01[16];           /* motion previous -> current camera as the frame used it */
  float T_wc[16];           /* pose after this call (after the local BA at a keyframe) */
  double lba_err_first, lba_err_last;
  int lba_landmarks, lba_observations;
} vo_mvo_frame_info;
int vo_mvo_create(vo_ctx *ctx, const vo_mvo_params *prm, vo_mvo **out);
void vo_mvo_destroy(vo_mvo *mvo);
/* MonoVO::trackImage(img, timestamp): synchronous. Image: u8, `stride` bytes per row, device pointer when on_device != 0. */
int vo_mvo_track(vo_mvo *mvo, const void *img, int stride, int on_device, double timestamp, vo_mvo_frame_info *info);
/* A recorded sequence through vo_mvo_result(k) / vo_mvo_enqueue(k + 1) / vo_mvo_prefetch(k + 2), the loop on this side of the ABI
 * (see vo_svo_run). The 5-point hook is called from inside as usual. */
int vo_mvo_run(vo_mvo *mvo, const void *const *img, int n_total, int stride, int on_device, int k_begin, int k_end,
               vo_mvo_frame_info *infos, double *stamps);
/* the same in halves, and the next image handed over early (pyramid + per-bin candidate table on the side stream). A host image is
 * uploaded asynchronously: its buffer must stay untouched until that image's frame has returned (as for vo_svo_prefetch). A refused
 * vo_mvo_enqueue leaves the driver as it was (the image can be handed over again); an error return of vo_mvo_result ENDS the
 * stream, as the reference's throw ends its node (mono_vo.cpp:909-949): the frame is no longer in flight and the track set / pose
 * are where the failing step left them. */
int vo_mvo_enqueue(vo_mvo *mvo, const void *img, int stride, int on_device, double timestamp);
int vo_mvo_prefetch(vo_mvo *mvo, const void *img, int stride, int on_device);
int vo_mvo_result(vo_mvo *mvo, vo_mvo_frame_info *info);
/* frame_prev_'s related landmarks (test / inspection hook): any pointer may be NULL. cos_parallax: cosine of
 * Landmark::getLastParallax() (2 = no second observation yet) */
int vo_mvo_get_tracks(vo_mvo *mvo, int32_t *ids, float *pts, float *Xw, uint8_t *flags, int32_t *age, float *cos_parallax, int cap,
                      int *n);
/* stats_keyframe (mono_vo.cpp:1130-1155), as vo_svo_keyframe_count / vo_svo_get_keyframes */
int vo_mvo_keyframe_count(vo_mvo *mvo, int *n_keyframes);
int vo_mvo_get_keyframes(vo_mvo *mvo, float *T_wc, int32_t *n_points, float *mappoints, size_t cap_points, size_t *total_points);
/* img_debug_ of the reference's MonoVO: with the option on, every frame draws what trackImage draws, on level 0 of the
 * current image slot (with rectify the undistorted image, which is what the reference draws on):
 *   first image      mono_vo.cpp:555  showTracking(I1, lmtrack_curr.pts1, {}, {}) = vo_draw_tracking with pts0 = the new
 *                    landmarks' pixels in landmark order, n1 = n_new = 0                                            (kind 1)
 *   initialisation   :627  showTracking(I1, lmtrack_final.pts0, lmtrack_final.pts1, pts1_new): the survivors of the 5-point
 *                    mask and the Sampson gate, in order, previous and current pixels; pts_new = EVERY candidate of the
 *                    bucketed extraction of :624, accepted by the back-tracking gate of :634 or not                 (kind 1)
 *   steady state     :904  showTrackingBA(I1, pts1_ba, pts1_proj_ba) = vo_draw_tracking_ba when the pose-only BA gave the
 *                    pose. index_ba (:799-826) = the features i with stage >= 2 and the BA class and Xp(2) > 0.1, in index
 *                    order (Xp = Rcw_prev X + tcw_prev, the frame kernel's own value). pts1_ba[i] = the refined pixel
 *                    pts1[i], also for features the BA or the Sampson gate reject afterwards. pts1_proj_ba[i] =
 *                    projectToPixel(dR10 Xp + dt10) (:893-897, camera.cpp:208-213) with dT10 = inverseSE3_f(dT01) of the
 *                    pose the frame returns, in float, every operation rounded on its own:
 *                      Xc_r = ((R[r][0]*Xp0 + R[r][1]*Xp1) + R[r][2]*Xp2) + t_r;  invz = 1.0f / Xc_2;
 *                      u = (fx * Xc_0) * invz + cx;  v = (fy * Xc_1) * invz + cy
 *                    (a depth Xc_2 <= 0 gives negative, infinite or NaN pixels: the drawing rules skip or clip them) (kind 2)
 *   steady state, 5-point fallback (too few BA points, or a failed BA): nothing, as in the reference — the picture, its size,
 *                    its kind and its points stay as they were.
 * Off by default; with it off no launch, allocation or result differs from a driver without the option.
 * vo_mvo_set_debug_image(mvo, 1) makes the option's only allocations, five of them: an index plane, the picture on the device,
 * a pinned host picture, and a device and a pinned block for the point sets. VO_ERR_INVALID while a frame is in flight.
 * The steady-state sets are gathered on the device by one small launch on the main stream behind the frame's last launch —
 * the frame's arrays are the next frame's to overwrite — and whether the frame draws is decided there, from the frame's
 * need_five_point word. Coverage, resolve and the copies to the host follow on the context's side stream. At most one picture
 * is in flight: vo_mvo_result waits for the PREVIOUS frame's picture before it enqueues its own, never for its own. Poses,
 * ids, pixels, flags, keyframe decisions and the local BA are the same bits with the option on and off.
 * vo_mvo_get_debug_image waits for the last picture only and copies it into `out` (height x width x 3 bytes, row pitch
 * out_stride >= 3 * width, VO_ERR_INVALID otherwise; NULL: the size only). Before the first picture *width = *height = 0 and
 * the call returns VO_OK.
 * vo_mvo_get_debug_points is a test / inspection hook: what the last picture was drawn from. *kind = 0 (none yet), 1
 * (showTracking), 2 (showTrackingBA). kind 1: set0 = pts0, set1 = pts1, set2 = pts_new. kind 2: set0 = pts1_ba, set1 =
 * pts1_proj_ba (both compacted, index order), n[2] = 0. x y pairs; any pointer may be NULL; VO_ERR_CAPACITY when a requested
 * set exceeds cap. */
int vo_mvo_set_debug_image(vo_mvo *mvo, int on);
int vo_mvo_get_debug_image(vo_mvo *mvo, uint8_t *out, int out_stride, int *width, int *height);
int vo_mvo_get_debug_points(vo_mvo *mvo, int *kind, float *set0, float *set1, float *set2, int n[3], int cap);
/* Covariance of MonoVO's pose, in map units (up to the stream's scale): vo_svo_set_pose_covariance's twin. The launch behind a
 * steady-state frame's BA launch is vo_gn_pose_information_mono on the launch's compacted set and its R01, t01. The first
 * image, the initialisation frame and a frame that took the 5-point fallback have no BA pose: they carry P with their own T10
 * (for the fallback the step is issued again from vo_mvo_result, where that pose becomes known) and count in n_unknown_steps.
 * The scale's own uncertainty is not part of P. */
int vo_mvo_set_pose_covariance(vo_mvo *mvo, int on, double sigma_px);
int vo_mvo_get_pose_covariance(vo_mvo *mvo, double P[36], double Sigma_xi[36], double *s2, int *valid, int *n_points,
                               int *n_unknown_steps);
/* test hook: the last steady-state frame's BA set (X in the previous camera's frame, pixels) and the R01, t01 the BA returned */
int vo_mvo_get_pose_covariance_inputs(vo_mvo *mvo, float *X, float *pts, int cap, int *n, float R01[9], float t01[3]);
/* the ignore mask of the images ingested from now on: vo_svo_set_mask's rules ("Ignore mask" above) */
int vo_mvo_set_mask(vo_mvo *mvo, const void *mask, int stride, int on_device);
/* the ZNCC gate of the steady-state frames ("ZNCC" above): VO_ZNCC_TEMPORAL only, VO_ZNCC_STEREO is VO_ERR_INVALID */
int vo_mvo_set_zncc_gate(vo_mvo *mvo, int pairs, int win, int pattern, float thres);
int vo_mvo_get_zncc(vo_mvo *mvo, float *zncc_t, int cap, int *n);

/* ---- 5-point RANSAC pose: MotionEstimator::calcPose5PointsAlgorithm ------------------------------------------------
 * motion_estimator.cpp:21-123 + findCorrectRT (:205-263): cv::findEssentialMat(pts0, pts1, K, RANSAC, confidence, thres_px)
 * followed by the reference's SVD decomposition and chirality test, on the device (csrc/five_point.hip). The library's
 * replacement for the caller hook of MonoVO (vo_mvo_params_set_five_point).
 *
 * One call (vo_five_point_pose), n pixel pairs pts0 (previous image) / pts1 (current), K = fx, fy, cx, cy:
 *  1. n < 5: VO_ERR_GN_FAILED (findEssentialMat has no model there).
 *  2. n == 5: the minimal solver once; its first solution; all five points inliers (OpenCV's count == modelPoints branch).
 *     No solution: VO_ERR_GN_FAILED.
 *  3. Points are normalised in double: ((u - cx) / fx, (v - cy) / fy); t = thres_px / ((fx + fy) / 2). A point is an inlier of
 *     E when its Sampson error, in double and rounded to float, is <= (float)(t * t). The arithmetic, in this order:
 *       a = (E0 x0 + E1 y0) + E2, b = (E3 x0 + E4 y0) + E5, c = (E6 x0 + E7 y0) + E8, d = (E0 x1 + E3 y1) + E6,
 *       e = (E1 x1 + E4 y1) + E7, r = (x1 a + y1 b) + c, err = (float)((r r) / (((a a + b b) + d d) + e e))  (E row-major).
 *  4. Samples s = 0 .. max_iters - 1 (all of them are evaluated, in one batch). Sample s draws indices until it has five
 *     distinct ones, at most 256 draws; draw j (j = 0, 1, ...; repeats rejected) is, in uint64 arithmetic,
 *       k = s * 256 + j;  z = seed + (k + 1) * 0x9E3779B97F4A7C15;
 *       z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9;  z = (z ^ (z >> 27)) * 0x94D049BB133111EB;  z ^= z >> 31;
 *       index = ((z >> 32) * n) >> 32
 *     (splitmix64 of a counter). The stream depends on (seed, s, n) only: a call carries nothing over from earlier calls.
 *  5. The minimal solver (Nister's 5-point method, in double) gives each sample at most 10 unit-Frobenius essential
 *     matrices: the null space of the 5x9 epipolar system, the ten cubic constraints det E = 0 and 2 EE^T E - tr(EE^T) E = 0,
 *     Gauss-Jordan, the hidden-variable 3x3 in z, the real roots of its degree-10 determinant (derivative-separated
 *     bisection on [-1, 1] for z and for 1/z, so ascending z in [-1, 1] first, then ascending 1/z), back substitution. A
 *     root whose E leaves a constraint residual above 1e-8 is dropped.
 *  6. Selection is OpenCV's sequential rule over that stream: samples in order, models in solver order; a model becomes
 *     the best when its inlier count is > max(best, 4); after each replacement niters = RANSACUpdateNumIters(p, (n -
 *     best) / n, 5, niters) with p = (double)confidence: d = 1 - (1 - ep)^5 (as ((q q)(q q)) q), d < DBL_MIN -> 0;
 *     num = log(max(1 - p, DBL_MIN)), den = log(d); niters if den >= 0 or -num >= niters (-den), else rint(num / den).
 *     The walk stops once s + 1 >= niters. The result does not depend on how the work is batched or launched.
 *  7. The best E is rounded to float (cv::cv2eigen into Mat33): E10. mask_5p = its inliers (3.), all five for n == 5.
 *  8. motion_estimator.cpp:64-127: Eigen's JacobiSVD of E10 in f32 (full U, V; restated as svo_svd4_nullvec restates the
 *     4x4), the last column of U / V negated where its determinant is negative, R = U W V^T, U W^T V^T, t = +-U.col(2) in
 *     the reference's order, mapping::triangulateDLT of EVERY point under each, the first candidate with a strictly larger
 *     count of points with both depths > 0 wins. mask = chirality AND mask_5p. Success even when fewer than half the points
 *     pass (findCorrectRT only warns); when no point passes under any candidate, VO_ERR_GN_FAILED (the reference's (R, t)
 *     would be uninitialised).
 *  9. Out: R10 (row-major), t10 (unit length), mask[n], info (may be NULL).
 * Bit parity with OpenCV is not the goal and cannot be had: OpenCV's random stream and its polynomial solver are its own.
 * Everything from 7. on is the reference's arithmetic.
 *
 * The solver owns its device workspace and pinned staging, sized at creation from max_points (<= 0: the context's) and
 * max_iters (1 .. 4096) through the context's counted allocations; a call allocates nothing. A call runs on the context's
 * main stream (one upload, three launches, one download) and waits for that stream only. It does not read the context's
 * summation order (its sums are integer counts or per-lane sequential arithmetic). Destroy it before its context. */
typedef struct {
  float thres_px;       /* motion_estimator.thres_5p_error (pixels) */
  float confidence;     /* 0.999 in the reference */
  int max_iters;        /* OpenCV's default 1000 */
  unsigned long long seed;
} vo_five_point_params;
typedef struct {
  float E10[9];         /* the selected essential matrix as the decomposition used it (float, row-major) */
  int n_inliers_5p;     /* |mask_5p| */
  int n_inliers;        /* |mask| = |mask_5p AND chirality| */
  int iterations;       /* samples walked: the stop index */
  int models;           /* models of those samples */
  int best_sample;      /* sample of the selected model (-1: none) */
} vo_five_point_info;
typedef struct vo_five_point vo_five_point;
int vo_five_point_create(vo_ctx *ctx, const vo_five_point_params *prm, int max_points, vo_five_point **out);
void vo_five_point_destroy(vo_five_point *fp);
/* VO_OK, VO_ERR_GN_FAILED where the reference has no pose (see above), VO_ERR_CAPACITY for n > max_points */
int vo_five_point_pose(vo_five_point *fp, const float *pts0, const float *pts1, int n, const float K[4], float R10[9],
                       float t10[3], uint8_t *mask, vo_five_point_info *info);
/* fills prm->five_point / five_point_user with the library's own hook bound to fp (no host callback on that path); fp must
 * outlive the vo_mvo created from prm */
int vo_mvo_params_set_five_point(vo_mvo_params *prm, vo_five_point *fp);
/* test hooks. minimal: n_sets sets of five NORMALISED pairs (x0, x1: n_sets x 5 x 2 doubles) through the minimal solver:
 * E[s * 90 + m * 9 + k] for m < n_sol[s]. samples: of the last vo_five_point_pose call (0 samples for n == 5, or after
 * vo_five_point_minimal): the five indices of every sample (-1 where it was given up), its number of models and its largest
 * inlier count (-1: no model); all three may be NULL to ask for *n_samples only; VO_ERR_CAPACITY when cap is too small. */
int vo_five_point_minimal(vo_five_point *fp, const double *x0, const double *x1, int n_sets, double *E, int *n_sol);
int vo_five_point_samples(const vo_five_point *fp, int32_t *subsets, int32_t *n_models, int32_t *best_count, int cap,
                          int *n_samples);
/* test hook: the inlier count of every model of every sample of the last vo_five_point_pose call, counts[s * 10 + m] in
 * solver order, -1 past the sample's models (so that the sequential rule can be walked model by model); NULL counts asks for
 * *n_samples only; VO_ERR_CAPACITY when cap (in samples) is too small */
int vo_five_point_counts(const vo_five_point *fp, int32_t *counts, int cap, int *n_samples);

/* ---- sparse local bundle adjustment -----------------------------------------
 * SparseBundleAdjustmentSolver::solveForFiniteIterations
 * (core/visual_odometry/ba_solver/sparse_bundle_adjustment.cpp:150-643; called from
 * MotionEstimator::localBundleAdjustmentSparseSolver[_Stereo], motion_estimator.cpp:1090-1340, with
 * MAX_ITER 10 and THRES_HUBER 0.5). The problem is what SparseBAParameters holds after
 * setPosesAndPoints (sparse_ba_parameters.h:283-440), as flat arrays, in double:
 *   T_jw      n_frames x 16   poses (row-major 4x4) of the frames that carry one - mono keyframes or the LEFT
 *                             frames of stereo keyframes - in the window's reference frame, translations scaled
 *   opt_index n_frames        index in [0, n_opt) of the pose in the optimisation, or -1 when it is fixed
 *   X         n_points x 3    landmarks (same frame and scale)
 *   obs_ptr   n_points + 1    observations of landmark i are obs_ptr[i] .. obs_ptr[i+1]-1, in the order of
 *                             LandmarkBA::kfs_seen
 *   obs_frame / obs_right / obs_px   frame index (the left frame for a right-image observation), seen in the
 *                             right image, pixel
 * T_jw (optimised poses) and X are updated in place. avg_err (max_iter doubles, may be NULL) receives the
 * average pixel error the reference prints per iteration. Returns 1 = flag_success, 0 = average error of the
 * last iteration above 1 px, VO_ERR_LBA_NAN where the reference throws. n_opt <= 20. */
typedef struct {
  int n_frames, n_opt, n_points, n_obs;
  int stereo;
  int max_iter;
  double Kl[4], Kr[4];
  double T_lr[16]; /* stereo pose left -> right as SparseBAParameters::getStereoPose gives it (scaled) */
  double thres_huber;
} vo_sba_problem;
int vo_sba_solve(vo_ctx *ctx, const vo_sba_problem *prm, double *T_jw, const int32_t *opt_index, double *X,
                 const int32_t *obs_ptr, const int32_t *obs_frame, const uint8_t *obs_right,
                 const double *obs_px, double *avg_err);

/* ---- kernel timing (HIP events on the context stream) --------------------- */
enum { VO_K_PYRAMID = 0, VO_K_KLT = 1, VO_K_IC = 2, VO_K_GN = 3, VO_K_HAMMING = 4, VO_K_AUX = 5, VO_K_COUNT = 6 };
int vo_profile_enable(vo_ctx *ctx, int max_records);
int vo_profile_reset(vo_ctx *ctx);
/* restrict the event brackets to a set of kernel classes: mask = OR of (1 << VO_K_*); 0 = all */
int vo_profile_set_classes(vo_ctx *ctx, unsigned mask);
/* after vo_synchronize(): launches and summed device time (ms) of one kernel class */
int vo_profile_get(vo_ctx *ctx, int kernel_class, int *launches, double *total_ms);

#ifdef __cplusplus
}
#endif
#endif /* VO_HIP_H_ */
