// stereo_vo.h — StereoVO (core/visual_odometry/stereo_vo/stereo_vo.h:45-273) on the C ABI (include/vo_hip.h: vo_svo_*).
//
// Same public surface as the reference's class: trackStereoImages(left, right, timestamp), getStatistics(); the
// statistics structs carry the reference's field names. The constructor takes numbers instead of (mode, YAML directory):
// loading the YAML (cv::FileStorage, stereo_vo.cpp:118-392) stays with the caller. What trackStereoImages does — the
// track set carried from frame to frame, new landmarks, keyframes, reconstruction, local bundle adjustment — runs inside
// libvo_hip.so with the track set on the device (csrc/stereo_vo.hip).
// SURVEY F9 / F12 behind switches: the reference's destructor writes /home/kch/frame_poses.txt and throws when it cannot
// (here: only when trajectory_path is set, never throwing from the destructor); the ROS1 node reads
// stats_execution.back() / stats_landmark.back(), which the reference never pushes (here: pushed every frame).
#ifndef VO_AMD_STEREO_VO_H_
#define VO_AMD_STEREO_VO_H_

#include <chrono>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "../defines/define_type.h"
#include "trajectory_io.h"
#include "vo_context.h"
#include "pose_covariance.h"

namespace vo {

struct StereoVOParams {
  // Camera.* / T_lr of the YAML (rectified pair)
  int width = 1241, height = 376;
  float Kl[4] = {718.856f, 718.856f, 607.1928f, 185.2157f}, Kr[4] = {718.856f, 718.856f, 607.1928f, 185.2157f};
  PoseSE3 T_lr = {1, 0, 0, 0.5371657189f, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
  // StereoVO::AlgorithmParameters (stereo_vo.h:57-103), defaults of the reference
  struct FeatureTrackerParameters {
    float thres_error = 125.0f, thres_bidirection = 1.0f, thres_sampson = 10.0f;
    int window_size = 15, max_level = 6;
  } feature_tracker;
  struct FeatureExtractorParameters {
    int n_features = 100, n_bins_u = 16, n_bins_v = 8;
    float thres_fastscore = 25.0f, radius = 15.0f;
  } feature_extractor;
  struct MotionEstimatorParameters {
    float thres_1p_error = 10.0f, thres_5p_error = 2.0f, thres_poseba_error = 5.0f;
  } motion_estimator;
  struct KeyframeUpdateParameters {
    float thres_alive_ratio = 0.7f;
    float thres_trans = 1.0f;     // metres
    float thres_rotation = 3.0f;  // DEGREES as in the YAML (the reference multiplies by D2R in its constructor)
    int n_max_keyframes_in_window = 9;
  } keyframe_update;
  // system_flags_.flagDoUndistortion (stereo_vo.cpp:239, :414-427): Kl / Kr / T_lr above are then the RAW cameras with the
  // distortion below (k1, k2, p1, p2, k3); the constructor makes the rectification maps on the context
  // (StereoCamera::initStereoCameraToRectify) and the loop runs on getRectifiedCamera / getRectifiedStereoPoseLeft2Right
  bool flagDoUndistortion = false;
  float Dl[5] = {0, 0, 0, 0, 0}, Dr[5] = {0, 0, 0, 0, 0};
  // not in the reference
  // stats_keyframe: the reference rewrites EVERY keyframe's pose and map points at every keyframe (stereo_vo.cpp:805-821,
  // a cost that grows with the length of the run). true: the same here (one gather + copy per keyframe so far, at every
  // keyframe); false: stats_keyframe stays empty and refreshKeyframeStatistics() fills it when the caller wants it
  bool keyframe_statistics = false;
  int strict_border = 4;        // vo_stereo_frame_set_strict_border
  bool local_ba = true;         // localBundleAdjustmentSparseSolver_Stereo at keyframes (the reference always does)
  std::string trajectory_path;  // F9: non-empty = write the frame poses there on destruction (the reference's format)
};

class StereoVO {
 public:
  struct AlgorithmStatistics {
    struct LandmarkStatistics {
      int n_initial = 0, n_pass_bidirection = 0, n_pass_1p = 0, n_pass_5p = 0, n_new = 0, n_final = 0;
      int max_age = 0, min_age = 0;
      float avg_age = 0.0f;
      int n_ok_parallax = 0;
      float min_parallax = 0.0f, max_parallax = 0.0f, avg_parallax = 0.0f;
    };
    struct FrameStatistics {
      PoseSE3 Twc, Tcw, dT_01, dT_10;
    };
    struct ExecutionStatistics {
      float time_track = 0.0f, time_1p = 0.0f, time_5p = 0.0f, time_localba = 0.0f, time_new = 0.0f, time_total = 0.0f;  // [ms]
    };
    struct KeyframeStatistics {  // what the ROS 2 node publishes as trajectory and map points (stereo_vo_ros2.cpp:141-166)
      PoseSE3 Twc;
      PointVec mappoints;
    };
    std::vector<KeyframeStatistics> stats_keyframe;
    std::vector<LandmarkStatistics> stats_landmark;
    std::vector<FrameStatistics> stats_frame;
    std::vector<ExecutionStatistics> stats_execution;
  };

  StereoVO(ContextPtr ctx, const StereoVOParams &p) : ctx_(std::move(ctx)), prm_(p) {
    vo_svo_params q;
    std::memset(&q, 0, sizeof(q));
    q.frame.width = p.width;
    q.frame.height = p.height;
    q.frame.win = p.feature_tracker.window_size;
    q.frame.max_level = p.feature_tracker.max_level;
    q.frame.thres_err = p.feature_tracker.thres_error;
    q.frame.thres_bidirection = p.feature_tracker.thres_bidirection;
    q.frame.thres_poseba = p.motion_estimator.thres_poseba_error;
    q.frame.thres_sampson = p.feature_tracker.thres_sampson;
    for (int k = 0; k < 4; ++k) {
      q.frame.Kl[k] = p.Kl[k];
      q.frame.Kr[k] = p.Kr[k];
    }
    for (int k = 0; k < 16; ++k) q.frame.T_lr[k] = p.T_lr[(size_t)k];
    if (p.flagDoUndistortion) {
      float K_rect[4], T_lr_rect[16];
      ctx_->check(vo_rectify_init_stereo(ctx_->get(), p.width, p.height, p.Kl, p.Dl, p.Kr, p.Dr, q.frame.T_lr, K_rect, T_lr_rect, nullptr));
      for (int k = 0; k < 4; ++k) q.frame.Kl[k] = q.frame.Kr[k] = K_rect[k];
      for (int k = 0; k < 16; ++k) q.frame.T_lr[k] = T_lr_rect[k];
      q.rectify = 1;
    }
    // FeatureExtractor::initParams -> WeightBin::init (feature_extractor.h:90-118, feature_extractor.cpp:48-56)
    q.bins.n_bins_u = p.feature_extractor.n_bins_u;
    q.bins.n_bins_v = p.feature_extractor.n_bins_v;
    q.bins.u_step = (int)std::floor((float)p.width / (float)p.feature_extractor.n_bins_u);
    q.bins.v_step = (int)std::floor((float)p.height / (float)p.feature_extractor.n_bins_v);
    q.bins.inv_u_step = 1.0f / (float)q.bins.u_step;
    q.bins.inv_v_step = 1.0f / (float)q.bins.v_step;
    q.bins.orb.nfeatures = 10000;
    q.bins.orb.scale_factor = 1.2;
    q.bins.orb.n_levels = 8;
    q.bins.orb.edge_threshold = 31;
    q.bins.orb.fast_threshold = (int)p.feature_extractor.thres_fastscore;
    q.kf_overlap_ratio = p.keyframe_update.thres_alive_ratio;
    q.kf_rotation_deg = p.keyframe_update.thres_rotation;
    q.kf_translation = p.keyframe_update.thres_trans;
    q.kf_window = p.keyframe_update.n_max_keyframes_in_window;
    q.strict_border = p.strict_border;
    q.local_ba = p.local_ba ? 1 : 0;
    ctx_->check(vo_svo_create(ctx_->get(), &q, &svo_));
  }
  ~StereoVO() {
    if (!prm_.trajectory_path.empty()) {
      try {
        std::vector<int> ids;
        std::vector<PoseSE3> poses;
        for (size_t k = 0; k < stat_.stats_frame.size(); ++k) {
          ids.push_back(frame_ids_[k]);
          poses.push_back(stat_.stats_frame[k].Twc);
        }
        writeTrajectory(prm_.trajectory_path, ids, poses);
      } catch (...) {  // (the reference's destructor is noexcept(false) and throws: not reproduced)
      }
    }
    if (svo_) vo_svo_destroy(svo_);
  }
  StereoVO(const StereoVO &) = delete;
  StereoVO &operator=(const StereoVO &) = delete;

  // StereoVO::trackStereoImages (stereo_vo.cpp:392-989). Throws std::runtime_error where the reference throws.
  void trackStereoImages(const Image &img_left, const Image &img_right, const double &timestamp) {
    if (img_left.width != prm_.width || img_left.height != prm_.height || img_right.width != prm_.width ||
        img_right.height != prm_.height || img_left.stride != img_right.stride)
      throw std::runtime_error("StereoVO: image size differs from the camera model");
    ctx_->checkFormat(img_left.format, prm_.flagDoUndistortion);
    ctx_->checkFormat(img_right.format, prm_.flagDoUndistortion);
    const auto t0 = std::chrono::steady_clock::now();
    vo_svo_frame_info info;
    ctx_->check(vo_svo_track(svo_, img_left.data, img_right.data, img_left.stride, 0, timestamp, &info));
    push_statistics(info, std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count());
  }
  // NOT in the reference: a caller that already holds the next pair (a recorded sequence) may hand it over before
  // trackStereoImages of the current one returns its result — see vo_svo_prefetch. The buffers must stay untouched
  // until that pair has been tracked.
  void enqueueStereoImages(const Image &l, const Image &r, const double &timestamp) {
    t_enq_ = std::chrono::steady_clock::now();
    ctx_->checkFormat(l.format, prm_.flagDoUndistortion);
    ctx_->checkFormat(r.format, prm_.flagDoUndistortion);
    ctx_->check(vo_svo_enqueue(svo_, l.data, r.data, l.stride, 0, timestamp));
  }
  void prefetchStereoImages(const Image &l, const Image &r) { ctx_->check(vo_svo_prefetch(svo_, l.data, r.data, l.stride, 0)); }
  void resultStereoImages() {
    vo_svo_frame_info info;
    ctx_->check(vo_svo_result(svo_, &info));
    push_statistics(info, std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t_enq_).count());
  }

  // A recorded sequence (host images, all of one stride) through the three calls above, the loop inside the library
  // (vo_svo_run): every pair is handed over one frame early. One statistics record per frame, as trackStereoImages leaves it.
  void trackSequence(const std::vector<Image> &left, const std::vector<Image> &right) {
    const size_t n = left.size() < right.size() ? left.size() : right.size();
    if (n == 0) return;
    std::vector<const void *> L(n), R(n);
    for (size_t k = 0; k < n; ++k) {
      L[k] = left[k].data;
      R[k] = right[k].data;
    }
    std::vector<vo_svo_frame_info> &infos = sequence_infos_;
    infos.assign(n, vo_svo_frame_info());
    std::vector<double> stamps(n);
    const auto t0 = std::chrono::steady_clock::now();
    ctx_->check(vo_svo_run(svo_, L.data(), R.data(), (int)n, left[0].stride, 0, 0, (int)n, infos.data(), stamps.data()));
    const float total = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
    for (size_t k = 0; k < n; ++k)
      push_statistics(infos[k], k == 0 ? total - (float)(1e3 * (stamps[n - 1] - stamps[0])) : (float)(1e3 * (stamps[k] - stamps[k - 1])));
  }

  const std::vector<vo_svo_frame_info> &sequenceInfos() const { return sequence_infos_; }  // (of the last trackSequence)

  const AlgorithmStatistics &getStatistics() const { return stat_; }
  // stats_keyframe as of now: every keyframe's current pose and the current 3-D points of its related landmarks
  void refreshKeyframeStatistics() {
    int nk = 0;
    ctx_->check(vo_svo_keyframe_count(svo_, &nk));
    stat_.stats_keyframe.resize((size_t)nk);
    if (nk == 0) return;
    std::vector<float> T((size_t)nk * 16);
    std::vector<std::int32_t> cnt((size_t)nk);
    std::size_t total = 0;
    ctx_->check(vo_svo_get_keyframes(svo_, T.data(), cnt.data(), nullptr, 0, &total));
    std::vector<Point> all(total);  // one gather + one copy for all keyframes
    if (total) ctx_->check(vo_svo_get_keyframes(svo_, nullptr, nullptr, reinterpret_cast<float *>(all.data()), total, &total));
    std::size_t off = 0;
    for (int j = 0; j < nk; ++j) {
      AlgorithmStatistics::KeyframeStatistics &k = stat_.stats_keyframe[(size_t)j];
      for (int q = 0; q < 16; ++q) k.Twc[(size_t)q] = T[(size_t)j * 16 + (size_t)q];
      k.mappoints.assign(all.begin() + (std::ptrdiff_t)off, all.begin() + (std::ptrdiff_t)(off + (std::size_t)cnt[(size_t)j]));
      off += (std::size_t)cnt[(size_t)j];
    }
  }
  const vo_svo_frame_info &lastFrameInfo() const { return last_; }
  // NOT in the reference (which leaves nav_msgs::Odometry::pose.covariance empty): the covariance of the pose, chained on the
  // device behind every frame's BA launch (vo_svo_set_pose_covariance), off by default. sigma_px > 0 scales by that pixel
  // noise instead of the a-posteriori variance.
  void setPoseCovariance(bool on, double sigma_px = 0.0) { ctx_->check(vo_svo_set_pose_covariance(svo_, on ? 1 : 0, sigma_px)); }
  // NOT in the reference (whose only such device is the y > 660 row gate): the ignore mask of the pairs handed over FROM NOW ON
  // (vo_svo_set_mask; include/vo_hip.h, "Ignore mask") — width x height bytes in the left image as the tracker sees it, 0 =
  // ignore; nullptr: none. on_device: the plane is device memory (a segmentation network's output). The library copies.
  void setMask(const std::uint8_t *mask, int stride, bool on_device = false) {
    ctx_->check(vo_svo_set_mask(svo_, mask, stride, on_device ? 1 : 0));
  }
  // In the reference only as a commented-out line (feature_tracker.cpp:198-202): the ZNCC appearance gate of the frames tracked
  // FROM NOW ON (vo_svo_set_zncc_gate; include/vo_hip.h, "ZNCC"). pairs: VO_ZNCC_TEMPORAL | VO_ZNCC_STEREO, 0 = off. A feature is
  // promoted to the next track set only where the ZNCC of its win x win patches exceeds thres. Throws while a frame is in flight.
  void setZnccGate(int pairs, float thres = 0.5f, int win = 15, int pattern = VO_ZNCC_PATTERN_CENTERED) {
    ctx_->check(vo_svo_set_zncc_gate(svo_, pairs, win, pattern, thres));
  }
  // The static stereo part of the reference author's semi-dense prototype (vo_svo_set_semidense; include/vo_hip.h, "Semi-dense
  // stereo"): depth of the high-gradient pixels of every keyframe's (every = VO_SEMIDENSE_FRAMES: every frame's) own rectified
  // pair, on the side stream behind the frame; the odometry does not change. prm = nullptr: off. defaultSemiDenseParams(bf)
  // fills in the defaults for a focal length x baseline. Throws while a frame is in flight.
  static vo_semidense_params defaultSemiDenseParams(float bf, int d_max = 64) {
    vo_semidense_params p;
    vo_semidense_default_params(&p);
    p.bf = bf;
    p.d_max = d_max;
    return p;
  }
  void setSemiDense(const vo_semidense_params *prm, int every = VO_SEMIDENSE_KEYFRAMES) { ctx_->check(vo_svo_set_semidense(svo_, prm, every)); }
  // the accepted pixels of the last result as points in the world frame (its frame's T_wc) or the left camera's, raster order;
  // waits for that result's launch only. false (and empty vectors) before the first result.
  bool getSemiDensePoints(PointVec &xyz, std::vector<float> *sigma_invd = nullptr, bool world = true, int *frame_id = nullptr) {
    int n = 0, fid = -1;
    const int rc = vo_svo_get_semidense_points(svo_, world ? 1 : 0, 0, nullptr, nullptr, nullptr, &n, &fid);
    if (rc != VO_ERR_CAPACITY) ctx_->check(rc);  // (room for none: the count is what was asked for)
    xyz.resize((size_t)n);
    if (sigma_invd) sigma_invd->resize((size_t)n);
    if (frame_id) *frame_id = fid;
    if (n) ctx_->check(vo_svo_get_semidense_points(svo_, world ? 1 : 0, n, reinterpret_cast<float *>(xyz.data()),
                                                   sigma_invd ? sigma_invd->data() : nullptr, nullptr, &n, &fid));
    return fid >= 0;
  }
  // Dense stereo disparity (vo_svo_set_dense_stereo; include/vo_hip.h, "Dense stereo"): census + semi-global matching on every
  // keyframe's (every = VO_SEMIDENSE_FRAMES: every frame's) own rectified pair, on the side stream behind the frame — a disparity
  // for walls and road too, less exact than the semi-dense one; the odometry does not change. Independent of setSemiDense.
  // prm = nullptr: off. defaultDenseStereoParams(bf) fills in the defaults for a focal length x baseline: the disparities
  // d_min .. d_min + n_disp - 1 (n_disp 64, 128, 192 or 256) are searched. Throws while a frame is in flight.
  static vo_dense_stereo_params defaultDenseStereoParams(float bf, int n_disp = 64, int d_min = 0) {
    vo_dense_stereo_params p;
    vo_dense_stereo_default_params(&p);
    p.bf = bf;
    p.n_disp = n_disp;
    p.d_min = d_min;
    return p;
  }
  void setDenseStereo(const vo_dense_stereo_params *prm, int every = VO_SEMIDENSE_KEYFRAMES) { ctx_->check(vo_svo_set_dense_stereo(svo_, prm, every)); }
  // The speckle filter behind every dense result (vo_svo_set_dense_speckle; include/vo_hip.h, "Speckle filter"): the connected
  // components of at most max_size pixels (4-neighbours, |disparity difference| <= max_diff) are removed on the side stream, in
  // place, so that getDensePoints leaves them out. Needs setDenseStereo. prm = nullptr: off. Throws while a frame is in flight.
  static vo_speckle_params defaultSpeckleParams() {
    vo_speckle_params p;
    vo_speckle_default_params(&p);
    return p;
  }
  void setDenseSpeckle(const vo_speckle_params *prm) { ctx_->check(vo_svo_set_dense_speckle(svo_, prm)); }
  // the last result's number of removed pixels and of components (0, 0 before any); waits for that result's launches only
  void getDenseSpeckleStats(int *n_removed, int *n_components) { ctx_->check(vo_svo_get_dense_speckle_stats(svo_, n_removed, n_components)); }
  // the accepted pixels of the last dense result as points, as getSemiDensePoints; waits for that result's launches only
  bool getDensePoints(PointVec &xyz, std::vector<float> *sigma_invd = nullptr, bool world = true, int *frame_id = nullptr) {
    int n = 0, fid = -1;
    const int rc = vo_svo_get_dense_points(svo_, world ? 1 : 0, 0, nullptr, nullptr, nullptr, &n, &fid);
    if (rc != VO_ERR_CAPACITY) ctx_->check(rc);  // (room for none: the count is what was asked for)
    xyz.resize((size_t)n);
    if (sigma_invd) sigma_invd->resize((size_t)n);
    if (frame_id) *frame_id = fid;
    if (n) ctx_->check(vo_svo_get_dense_points(svo_, world ? 1 : 0, n, reinterpret_cast<float *>(xyz.data()),
                                               sigma_invd ? sigma_invd->data() : nullptr, nullptr, &n, &fid));
    return fid >= 0;
  }
  // The temporal half of that prototype (vo_svo_set_semidense_temporal; include/vo_hip.h, "Semi-dense temporal"): every keyframe's
  // static result seeds a map that each later frame until the next keyframe updates on the side stream (an epipolar search along
  // the odometry's pose, Gaussian fusion of the inverse depths). Needs setSemiDense. prm = nullptr: off. Throws while a frame is in flight.
  static vo_semidense_temporal_params defaultSemiDenseTemporalParams() {
    vo_semidense_temporal_params p;
    vo_semidense_temporal_default_params(&p);
    return p;
  }
  void setSemiDenseTemporal(const vo_semidense_temporal_params *prm) { ctx_->check(vo_svo_set_semidense_temporal(svo_, prm)); }
  // the last keyframe's map as points (the pixels with n_obs >= min_obs, z = 1 / invd) in the world frame (the keyframe's T_wc) or
  // the left camera's, raster order; waits for the side stream's last launch only. false (and empty vectors) before a keyframe.
  bool getSemiDenseMapPoints(PointVec &xyz, std::vector<float> *sigma = nullptr, bool world = true, int min_obs = 2, int *frame_id = nullptr) {
    int n = 0, fid = -1;
    const int rc = vo_svo_get_semidense_map_points(svo_, world ? 1 : 0, min_obs, 0, nullptr, nullptr, nullptr, &n, &fid);
    if (rc != VO_ERR_CAPACITY) ctx_->check(rc);  // (room for none: the count is what was asked for)
    xyz.resize((size_t)n);
    if (sigma) sigma->resize((size_t)n);
    if (frame_id) *frame_id = fid;
    if (n) ctx_->check(vo_svo_get_semidense_map_points(svo_, world ? 1 : 0, min_obs, n, reinterpret_cast<float *>(xyz.data()),
                                                       sigma ? sigma->data() : nullptr, nullptr, &n, &fid));
    return fid >= 0;
  }
  // The map carried over to the next keyframe (vo_svo_set_semidense_propagate; include/vo_hip.h, "Semi-dense propagation"): at a
  // keyframe the old map is warped into the new one under the odometry's pose and fused with its static result, so that
  // getSemiDenseMapPoints has points on a keyframe frame too. Needs setSemiDenseTemporal. prm = nullptr: off. Throws while a frame
  // is in flight.
  static vo_semidense_propagate_params defaultSemiDensePropagateParams() {
    vo_semidense_propagate_params p;
    vo_semidense_propagate_default_params(&p);
    return p;
  }
  void setSemiDensePropagate(const vo_semidense_propagate_params *prm) { ctx_->check(vo_svo_set_semidense_propagate(svo_, prm)); }
  // the map's origin plane (0 nothing, 1 static, 2 propagated, 3 fused, 4 static replaced a propagated value), width x height;
  // from_frame_id: the keyframe the map was propagated from, -1: seeded without a predecessor. false (and empty) before a keyframe.
  bool getSemiDenseOrigin(std::vector<uint8_t> &origin, int *width = nullptr, int *height = nullptr, int *from_frame_id = nullptr) {
    int w = 0, h = 0, from = -1;
    ctx_->check(vo_svo_get_semidense_origin(svo_, nullptr, &w, &h, &from));
    origin.resize((size_t)w * (size_t)h);
    if (w > 0) ctx_->check(vo_svo_get_semidense_origin(svo_, origin.data(), &w, &h, &from));
    if (width) *width = w;
    if (height) *height = h;
    if (from_frame_id) *from_frame_id = from;
    return w > 0;
  }
  // A regularised copy of the map (vo_svo_set_semidense_regularize; include/vo_hip.h, "Semi-dense regularisation"): behind every
  // launch that writes the map one launch on the side stream removes the entries their neighbours contradict, fills high-gradient
  // holes whose neighbours agree and smooths the rest, into planes of its own; the map itself keeps its bits. Needs
  // setSemiDenseTemporal. prm = nullptr: off. Throws while a frame is in flight.
  static vo_semidense_regularize_params defaultSemiDenseRegularizeParams() {
    vo_semidense_regularize_params p;
    vo_semidense_regularize_default_params(&p);
    return p;
  }
  void setSemiDenseRegularize(const vo_semidense_regularize_params *prm) { ctx_->check(vo_svo_set_semidense_regularize(svo_, prm)); }
  // the regularised map as points (the pixels with n_obs >= min_obs; a filled pixel has n_obs 1), as getSemiDenseMapPoints. false (and
  // empty vectors) before the first frame since the option was switched on.
  bool getSemiDenseRegularizedPoints(PointVec &xyz, std::vector<float> *sigma = nullptr, bool world = true, int min_obs = 1,
                                     int *frame_id = nullptr) {
    int n = 0, fid = -1;
    const int rc = vo_svo_get_semidense_regularized_points(svo_, world ? 1 : 0, min_obs, 0, nullptr, nullptr, nullptr, &n, &fid);
    if (rc != VO_ERR_CAPACITY) ctx_->check(rc);  // (room for none: the count is what was asked for)
    xyz.resize((size_t)n);
    if (sigma) sigma->resize((size_t)n);
    if (frame_id) *frame_id = fid;
    if (n) ctx_->check(vo_svo_get_semidense_regularized_points(svo_, world ? 1 : 0, min_obs, n, reinterpret_cast<float *>(xyz.data()),
                                                               sigma ? sigma->data() : nullptr, nullptr, &n, &fid));
    return fid >= 0;
  }
  // The keyframes' maps fused into one world-frame voxel map (vo_svo_set_semidense_world; include/vo_hip.h, "Semi-dense world map"):
  // when a keyframe is replaced one launch on the side stream integrates its map (source VO_SEMIDENSE_WORLD_RAW, or _REGULARIZED:
  // its regularised copy) into a hash table of voxels; the odometry's results and every semi-dense result keep their bits. Needs
  // setSemiDenseTemporal (and setSemiDenseRegularize for the regularised source). prm = nullptr: off. Throws while a frame is in flight.
  static vo_semidense_world_params defaultSemiDenseWorldParams() {
    vo_semidense_world_params p;
    vo_semidense_world_default_params(&p);
    return p;
  }
  void setSemiDenseWorld(const vo_semidense_world_params *prm, int source = VO_SEMIDENSE_WORLD_RAW) {
    ctx_->check(vo_svo_set_semidense_world(svo_, prm, source));
  }
  // The world map follows the local BA (vo_svo_set_semidense_world_reanchor; include/vo_hip.h, "Semi-dense world map: removal and
  // re-anchoring"): the maps of the keyframes in the BA's window are retained, and at every keyframe each one whose keyframe has moved
  // by min_move voxels or more is taken out of the table and put back with the keyframe's current pose. Needs setSemiDenseWorld and
  // local_ba. Throws while a frame is in flight.
  void setSemiDenseWorldReanchor(bool on, float min_move = 0.0f) { ctx_->check(vo_svo_set_semidense_world_reanchor(svo_, on ? 1 : 0, min_move)); }
  vo_semidense_world_reanchor_info getSemiDenseWorldReanchorStats() {
    vo_semidense_world_reanchor_info info;
    ctx_->check(vo_svo_get_semidense_world_reanchor_stats(svo_, &info));
    return info;
  }
  // per integrated keyframe, in integration order: its frame id, its index among the keyframes, the pose its map is in the table with
  // (row-major 4 x 4, 16 floats each) and whether it is still in the window; returns their number
  int getSemiDenseWorldAnchors(std::vector<int32_t> *frame_id, std::vector<int32_t> *kf_index, std::vector<float> *T_wk,
                               std::vector<int32_t> *in_window = nullptr) {
    int n = 0;
    const int rc = vo_svo_get_semidense_world_anchors(svo_, 0, nullptr, nullptr, nullptr, nullptr, &n);
    if (rc != VO_ERR_CAPACITY) ctx_->check(rc);  // (room for none: the count is what was asked for)
    if (frame_id) frame_id->resize((size_t)n);
    if (kf_index) kf_index->resize((size_t)n);
    if (T_wk) T_wk->resize((size_t)n * 16);
    if (in_window) in_window->resize((size_t)n);
    if (n) ctx_->check(vo_svo_get_semidense_world_anchors(svo_, n, frame_id ? frame_id->data() : nullptr, kf_index ? kf_index->data() : nullptr,
                                                          T_wk ? T_wk->data() : nullptr, in_window ? in_window->data() : nullptr, &n));
    return n;
  }
  // the current keyframe's map into the world map now (the end of a sequence); the next keyframe change does not integrate it again
  void flushSemiDenseWorld() { ctx_->check(vo_svo_semidense_world_flush(svo_)); }
  void clearSemiDenseWorld() { ctx_->check(vo_svo_semidense_world_clear(svo_)); }
  vo_semidense_world_info getSemiDenseWorldStats() {
    vo_semidense_world_info info;
    ctx_->check(vo_svo_get_semidense_world_stats(svo_, &info));
    return info;
  }
  // the voxels with at least min_count points seen by at least min_keyframes keyframes, in ascending key order: their weighted mean
  // positions and, where asked for, point counts, keyframe counts and grey values. Returns their number.
  int getSemiDenseWorldPoints(PointVec &xyz, int min_count = 1, int min_keyframes = 1, std::vector<uint32_t> *count = nullptr,
                              std::vector<uint32_t> *keyframes = nullptr, std::vector<uint8_t> *grey = nullptr) {
    int n = 0;
    const int rc = vo_svo_get_semidense_world_points(svo_, min_count, min_keyframes, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, &n);
    if (rc != VO_ERR_CAPACITY) ctx_->check(rc);  // (room for none: the count is what was asked for)
    xyz.resize((size_t)n);
    if (count) count->resize((size_t)n);
    if (keyframes) keyframes->resize((size_t)n);
    if (grey) grey->resize((size_t)n);
    if (n) ctx_->check(vo_svo_get_semidense_world_points(svo_, min_count, min_keyframes, n, nullptr, reinterpret_cast<float *>(xyz.data()), nullptr,
                                                         count ? count->data() : nullptr, keyframes ? keyframes->data() : nullptr,
                                                         grey ? grey->data() : nullptr, &n));
    return n;
  }
  // Free-space carving on the world map (vo_svo_set_semidense_world_carve; include/vo_hip.h, "Semi-dense world map: free-space
  // carving"): directly behind every integration of a keyframe's map its rays are marched through the table, and every voxel a ray
  // passes through on its way to a surface behind gets 1 added to its `free` count. Needs setSemiDenseWorld. prm = nullptr: off.
  // Throws while a frame is in flight.
  static vo_semidense_world_carve_params defaultSemiDenseWorldCarveParams() {
    vo_semidense_world_carve_params p;
    vo_semidense_world_carve_default_params(&p);
    return p;
  }
  void setSemiDenseWorldCarve(const vo_semidense_world_carve_params *prm) { ctx_->check(vo_svo_set_semidense_world_carve(svo_, prm)); }
  // The world map fed from the dense result (include/vo_hip.h, "Semi-dense map merge"): setSemiDenseWorld(prm, VO_SEMIDENSE_WORLD_DENSE
  // or _MERGED) needs setDenseStereo; setSemiDenseWorldMerge sets chi and keep_obs of the merges enqueued from then on (nullptr: the
  // defaults 3, 2); getSemiDenseWorldSource returns what the last merge wrote — the planes sized width x height, origin and the six
  // counts; any vector may be null — and its keyframe's frame id, -1 and 0 x 0 where there is none. Both throw while a frame is in flight.
  static vo_semidense_map_merge_params defaultSemiDenseWorldMergeParams() {
    vo_semidense_map_merge_params p;
    vo_semidense_map_merge_default_params(&p);
    return p;
  }
  void setSemiDenseWorldMerge(const vo_semidense_map_merge_params *prm) { ctx_->check(vo_svo_set_semidense_world_merge(svo_, prm)); }
  int getSemiDenseWorldSource(std::vector<float> *invd, std::vector<float> *sigma, std::vector<uint8_t> *n_obs, std::vector<uint8_t> *origin,
                              int *width, int *height, uint64_t counts[6] = nullptr) {
    int w = 0, h = 0, frame_id = -1;
    ctx_->check(vo_svo_get_semidense_world_source(svo_, nullptr, nullptr, nullptr, nullptr, &w, &h, &frame_id, nullptr));
    const size_t n = (size_t)w * (size_t)h;
    if (invd) invd->assign(n, 0.0f);
    if (sigma) sigma->assign(n, 0.0f);
    if (n_obs) n_obs->assign(n, 0);
    if (origin) origin->assign(n, 0);
    ctx_->check(vo_svo_get_semidense_world_source(svo_, invd ? invd->data() : nullptr, sigma ? sigma->data() : nullptr,
                                                  n_obs ? n_obs->data() : nullptr, origin ? origin->data() : nullptr, &w, &h, &frame_id, counts));
    if (width) *width = w;
    if (height) *height = h;
    return frame_id;
  }
  vo_semidense_world_carve_info getSemiDenseWorldCarveStats() {
    vo_semidense_world_carve_info info;
    ctx_->check(vo_svo_get_semidense_world_carve_stats(svo_, &info));
    return info;
  }
  // getSemiDenseWorldPoints with the free count per voxel; with free_den >= 1 only the voxels with free * free_den <= count *
  // free_num (free_den 0: all of them). Returns their number.
  int getSemiDenseWorldFree(PointVec &xyz, std::vector<uint32_t> &free_count, int free_num = 0, int free_den = 0, int min_count = 1,
                            int min_keyframes = 1, std::vector<uint32_t> *count = nullptr, std::vector<uint32_t> *keyframes = nullptr,
                            std::vector<uint8_t> *grey = nullptr) {
    int n = 0;
    const int rc = vo_svo_get_semidense_world_points_free(svo_, min_count, min_keyframes, free_num, free_den, 0, nullptr, nullptr, nullptr, nullptr,
                                                          nullptr, nullptr, nullptr, &n);
    if (rc != VO_ERR_CAPACITY) ctx_->check(rc);  // (room for none: the count is what was asked for)
    xyz.resize((size_t)n);
    free_count.resize((size_t)n);
    if (count) count->resize((size_t)n);
    if (keyframes) keyframes->resize((size_t)n);
    if (grey) grey->resize((size_t)n);
    if (n) ctx_->check(vo_svo_get_semidense_world_points_free(svo_, min_count, min_keyframes, free_num, free_den, n, nullptr,
                                                              reinterpret_cast<float *>(xyz.data()), nullptr, count ? count->data() : nullptr,
                                                              keyframes ? keyframes->data() : nullptr, grey ? grey->data() : nullptr,
                                                              free_count.data(), &n));
    return n;
  }
  // Direct image alignment on the keyframe's map (vo_svo_set_semidense_align; include/vo_hip.h, "Semi-dense alignment"): every frame
  // that is not a keyframe aligns its left image against the map from the odometry's pose, on the side stream in front of the
  // frame's temporal launch; nothing uses the aligned pose. Needs setSemiDenseTemporal. prm = nullptr: off. Throws while a frame is
  // in flight.
  static vo_semidense_align_params defaultSemiDenseAlignParams() {
    vo_semidense_align_params p;
    vo_semidense_align_default_params(&p);
    return p;
  }
  void setSemiDenseAlign(const vo_semidense_align_params *prm) { ctx_->check(vo_svo_set_semidense_align(svo_, prm)); }
  // the last frame's alignment: result (T_ck, status, iters, count, rms, H, b), T_wc = the keyframe's pose times inverseSE3(T_ck)
  // (row-major 4 x 4, may be nullptr), the frame's id and the keyframe's. false at a keyframe frame, which has none (status
  // VO_SEMIDENSE_ALIGN_NONE). Waits for the side stream's last launch only.
  bool getSemiDenseAlign(vo_semidense_align_result &result, float *T_wc = nullptr, int *frame_id = nullptr, int *key_frame_id = nullptr) {
    ctx_->check(vo_svo_get_semidense_align(svo_, &result, T_wc, frame_id, key_frame_id));
    return result.status != VO_SEMIDENSE_ALIGN_NONE;
  }
  // The same alignment coarse to fine on a map pyramid (vo_svo_set_semidense_align_pyr; include/vo_hip.h, "Semi-dense alignment on a
  // map pyramid"): it converges from a frame's motion and more. start = VO_SEMIDENSE_ALIGN_START_PREVIOUS: an odometry of its own —
  // the identity at the first frame after a keyframe, then the previous frame's aligned pose where that frame converged, else the
  // odometry's. Takes effect with the next keyframe; replaces setSemiDenseAlign's launches while it is on. prm = nullptr: off.
  static vo_semidense_align_pyr_params defaultSemiDenseAlignPyramidParams() {
    vo_semidense_align_pyr_params p;
    vo_semidense_align_pyr_default_params(&p);
    return p;
  }
  void setSemiDenseAlignPyramid(const vo_semidense_align_pyr_params *prm, int start = VO_SEMIDENSE_ALIGN_START_ODOMETRY) {
    ctx_->check(vo_svo_set_semidense_align_pyr(svo_, prm, start));
  }
  // getSemiDenseAlign with the per-level fields (index = level) and start_prev: the previous frame's aligned pose was the start
  bool getSemiDenseAlign(vo_semidense_align_pyr_result &result, float *T_wc = nullptr, int *frame_id = nullptr, int *key_frame_id = nullptr) {
    ctx_->check(vo_svo_get_semidense_align_pyr(svo_, &result, T_wc, frame_id, key_frame_id));
    return result.status != VO_SEMIDENSE_ALIGN_NONE;
  }
  // A modifier of whichever alignment is on (vo_svo_set_semidense_align_affine; include/vo_hip.h, "Semi-dense alignment with affine
  // brightness"): a gain and an offset of the keyframe's grey levels are estimated next to the pose, so that an exposure change
  // between the keyframe and the frame does not bias it. affine = nullptr: off. Needs setSemiDenseAlign or setSemiDenseAlignPyramid.
  static vo_semidense_affine_params defaultSemiDenseAffineParams() {
    vo_semidense_affine_params p;
    vo_semidense_affine_default_params(&p);
    return p;
  }
  void setSemiDenseAlignAffine(const vo_semidense_affine_params *affine) { ctx_->check(vo_svo_set_semidense_align_affine(svo_, affine)); }
  // getSemiDenseAlign with gain, offset, G, O, the 8 x 8 system and G, O per level; refused while the modifier is off (the two
  // getters above then serve, and while it is on return the affine run's pose, status, iters, count and rms)
  bool getSemiDenseAlign(vo_semidense_align_affine_result &result, float *T_wc = nullptr, int *frame_id = nullptr, int *key_frame_id = nullptr) {
    ctx_->check(vo_svo_get_semidense_align_affine(svo_, &result, T_wc, frame_id, key_frame_id));
    return result.status != VO_SEMIDENSE_ALIGN_NONE;
  }
  // NOT in the reference: CLAHE on every image before the tracker (vo::Context::setEqualize on this driver's context): legal
  // between frames, applies to the images handed over from now on
  void setEqualize(int mode, double clip_limit = 40.0, int tiles_x = 8, int tiles_y = 8) { ctx_->setEqualize(mode, clip_limit, tiles_x, tiles_y); }
  int width() const { return prm_.width; }
  int height() const { return prm_.height; }
  // of the last tracked frame: waits for that frame's covariance launch only
  PoseCovariance getPoseCovariance() {
    PoseCovariance c;
    int valid = 0;
    ctx_->check(vo_svo_get_pose_covariance(svo_, c.P.data(), c.Sigma_xi.data(), &c.s2, &valid, &c.n_points, &c.n_unknown_steps));
    c.valid = valid != 0;
    return c;
  }
  // the 36 doubles of pose.covariance for the last frame's pose: (x, y, z, rot x, rot y, rot z), row-major
  std::array<double, 36> getPoseCovarianceRos() { return poseCovarianceRos(getPoseCovariance().P, last_.T_wc); }
  // img_debug_ of the reference (stereo_vo.cpp:685-688), drawn on the device (vo_svo_set_debug_image): off by default
  void setDebugImage(bool on) { ctx_->check(vo_svo_set_debug_image(svo_, on ? 1 : 0)); }
  // the last picture: rows of width x 3 bytes (cv::Scalar component k in channel k: published as bgr8, (0,255,0) is green);
  // returns false and leaves `rgb` empty before the first drawn frame
  bool getDebugImage(std::vector<std::uint8_t> &rgb, int &width, int &height) {
    ctx_->check(vo_svo_get_debug_image(svo_, nullptr, 0, &width, &height));
    rgb.assign((size_t)width * (size_t)height * 3, 0);
    if (rgb.empty()) return false;
    ctx_->check(vo_svo_get_debug_image(svo_, rgb.data(), 3 * width, &width, &height));
    return true;
  }
  // stframe_prev_'s tracked pixels and landmarks (ids, flags: VO_LM_*), for inspection
  void getTracks(std::vector<std::int32_t> &ids, PixelVec &pts_l, PixelVec &pts_r, PointVec &Xw, std::vector<std::uint8_t> &flags) {
    int n = 0;
    ctx_->check(vo_svo_get_tracks(svo_, nullptr, nullptr, nullptr, nullptr, nullptr, 0, &n));
    ids.resize((size_t)n);
    pts_l.resize((size_t)n);
    pts_r.resize((size_t)n);
    Xw.resize((size_t)n);
    flags.resize((size_t)n);
    if (n)
      ctx_->check(vo_svo_get_tracks(svo_, ids.data(), reinterpret_cast<float *>(pts_l.data()), reinterpret_cast<float *>(pts_r.data()),
                                    reinterpret_cast<float *>(Xw.data()), flags.data(), n, &n));
  }

 private:
  static PoseSE3 inverse_se3(const PoseSE3 &T) {  // geometry::inverseSE3_f
    PoseSE3 o{};
    for (int i = 0; i < 3; ++i) {
      for (int j = 0; j < 3; ++j) o[(size_t)(i * 4 + j)] = T[(size_t)(j * 4 + i)];
      o[(size_t)(i * 4 + 3)] = ((-T[(size_t)(0 * 4 + i)]) * T[3] + (-T[(size_t)(1 * 4 + i)]) * T[7]) + (-T[(size_t)(2 * 4 + i)]) * T[11];
    }
    o[15] = 1.0f;
    return o;
  }
  void push_statistics(const vo_svo_frame_info &info, float ms) {
    last_ = info;
    AlgorithmStatistics::FrameStatistics f;
    for (int k = 0; k < 16; ++k) {
      f.Twc[(size_t)k] = info.T_wc[k];
      f.dT_01[(size_t)k] = info.dT[k];
    }
    f.Tcw = inverse_se3(f.Twc);
    f.dT_10 = inverse_se3(f.dT_01);
    stat_.stats_frame.push_back(f);  // stereo_vo.cpp:979-980
    frame_ids_.push_back(info.frame_id);
    AlgorithmStatistics::LandmarkStatistics l;  // F12: the ROS1 node reads .back() of these two
    l.n_initial = info.n_tracks_in;
    l.n_pass_bidirection = info.counts.n_l1r1;
    l.n_pass_1p = l.n_pass_5p = info.counts.n_inlier;
    l.n_new = info.n_new;
    l.n_final = info.n_tracks_out;
    stat_.stats_landmark.push_back(l);
    AlgorithmStatistics::ExecutionStatistics e;
    e.time_total = e.time_track = ms;
    stat_.stats_execution.push_back(e);
    if (prm_.keyframe_statistics && info.is_keyframe) refreshKeyframeStatistics();
  }

  ContextPtr ctx_;
  StereoVOParams prm_;
  vo_svo *svo_ = nullptr;
  AlgorithmStatistics stat_;
  std::vector<int> frame_ids_;
  vo_svo_frame_info last_{};
  std::chrono::steady_clock::time_point t_enq_;
  std::vector<vo_svo_frame_info> sequence_infos_;
};

}  // namespace vo
#endif
