// feature_extractor.h — FeatureExtractor::descriptorDistance
// (core/visual_odometry/feature_extractor.cpp:338-357) for descriptor sets, and the bucketing around
// cv::ORB::detect (feature_extractor.h:58-135, feature_extractor.cpp:241-277), and extractAndComputeORB (:321-332).
#ifndef VO_AMD_FEATURE_EXTRACTOR_H_
#define VO_AMD_FEATURE_EXTRACTOR_H_

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <stdexcept>
#include <vector>

#include "../defines/define_type.h"
#include "vo_context.h"

namespace vo {

class FeatureExtractor {
 public:
  explicit FeatureExtractor(ContextPtr ctx) : ctx_(std::move(ctx)) {}
  // single pair, same contract as the reference (two 32-byte ORB descriptors -> [0,256])
  int descriptorDistance(const std::uint8_t *a, const std::uint8_t *b) {
    std::uint16_t d = 0;
    ctx_->check(vo_orb_hamming(ctx_->get(), a, 1, b, 1, &d));
    return (int)d;
  }
  // ---- bucketing around cv::ORB::detect (the detector itself stays OpenCV's, on the host) ----
  // feature_extractor.cpp:26-69 / WeightBin::init (feature_extractor.h:90-118)
  void initParams(int n_cols, int n_rows, int n_bins_u, int n_bins_v, int /*THRES_FAST*/ = 15, int /*radius*/ = 5) {
    n_bins_u_ = n_bins_u;
    n_bins_v_ = n_bins_v;
    u_step_ = (int)std::floor((float)n_cols / (float)n_bins_u);
    v_step_ = (int)std::floor((float)n_rows / (float)n_bins_v);
    inv_u_step_ = 1.0f / (float)u_step_;
    inv_v_step_ = 1.0f / (float)v_step_;
    weight_.assign((size_t)n_bins_u * n_bins_v, 1);
  }
  // extractor_orb_ settings of initParams (:48-56); THRES_FAST of the call above
  void setOrbParams(int fast_threshold, int nfeatures = 10000, double scale_factor = 1.2, int n_levels = 8,
                    int edge_threshold = 31) {
    orb_ = vo_orb_params{nfeatures, scale_factor, n_levels, edge_threshold, fast_threshold};
  }
  // extractor_orb_->detect(img, fts) (:241) on the image in `slot`
  void detect(int slot, PixelVec &kp, std::vector<float> &response, std::vector<std::int32_t> &octave,
              int max_kp = 60000) {
    kp.assign((size_t)max_kp, Pixel{0.f, 0.f});
    response.assign((size_t)max_kp, 0.f);
    octave.assign((size_t)max_kp, 0);
    int n = 0;
    ctx_->check(vo_orb_detect(ctx_->get(), slot, &orb_, &kp.data()->x, response.data(), octave.data(), max_kp, &n));
    kp.resize((size_t)n);
    response.resize((size_t)n);
    octave.resize((size_t)n);
  }
  // extractAndComputeORB (:321-332): detect() and the descriptors of all its keypoints (cv::ORB::compute restated, include/vo_hip.h);
  // angle in degrees, size = 31 * scale (cv::KeyPoint::size), desc 32 bytes per keypoint. The descriptors also stay on the
  // device as set 0 / 1 for matchSets.
  void extractAndComputeORB(int slot, PixelVec &kp, std::vector<float> &response, std::vector<std::int32_t> &octave,
                            std::vector<float> &angle, std::vector<float> &size, std::vector<std::uint8_t> &desc, int set = 0,
                            bool steer = true, int max_kp = 60000) {
    kp.assign((size_t)max_kp, Pixel{0.f, 0.f});
    response.assign((size_t)max_kp, 0.f);
    octave.assign((size_t)max_kp, 0);
    angle.assign((size_t)max_kp, 0.f);
    desc.assign((size_t)max_kp * 32, 0);
    int n = 0;
    ctx_->check(vo_orb_detect_and_compute(ctx_->get(), slot, &orb_, steer ? 1 : 0, set, &kp.data()->x, response.data(), octave.data(),
                                          angle.data(), desc.data(), max_kp, &n));
    kp.resize((size_t)n);
    response.resize((size_t)n);
    octave.resize((size_t)n);
    angle.resize((size_t)n);
    desc.resize((size_t)n * 32);
    size.resize((size_t)n);
    for (int i = 0; i < n; ++i) size[(size_t)i] = 31.0f * (float)std::pow(orb_.scale_factor, (double)octave[(size_t)i]);
    set_size_[set] = n;
  }
  // descriptors of the caller's keypoints; valid[i] = 0 (angle 0, zero descriptor) for a keypoint too close to its level's border
  void compute(int slot, const PixelVec &kp, const std::vector<std::int32_t> &octave, std::vector<float> &angle,
               std::vector<std::uint8_t> &desc, std::vector<std::uint8_t> &valid, bool steer = true) {
    if (kp.size() != octave.size()) throw std::runtime_error("keypoint positions / octaves differ in length");
    const int n = (int)kp.size();
    angle.assign((size_t)n, 0.f);
    desc.assign((size_t)n * 32, 0);
    valid.assign((size_t)n, 0);
    ctx_->check(vo_orb_compute(ctx_->get(), slot, &orb_, n ? &kp.data()->x : zero_, octave.data(), n, steer ? 1 : 0, angle.data(),
                               desc.data(), valid.data()));
  }
  void getPattern(std::int8_t pattern[1024]) { ctx_->check(vo_orb_get_pattern(ctx_->get(), pattern)); }
  void setPattern(const std::int8_t pattern[1024]) { ctx_->check(vo_orb_set_pattern(ctx_->get(), pattern)); }
  // the accept rule of test/test_orbmatching.cpp:87-137 on two resident sets: one entry per keypoint of set a
  void matchSets(int a, int b, std::vector<std::int32_t> &best_idx, std::vector<std::uint16_t> &best_dist,
                 std::vector<std::uint16_t> &second_dist, int th_low = 50, float ratio = 0.6f) {
    if (a < 0 || a > 1 || b < 0 || b > 1 || set_size_[a] < 0 || set_size_[b] < 0)
      throw std::runtime_error("matchSets: extractAndComputeORB has not filled both sets through this object");
    const size_t na = (size_t)set_size_[a];
    best_idx.assign(na + 1, -1);
    best_dist.assign(na + 1, 0);
    second_dist.assign(na + 1, 0);
    ctx_->check(vo_orb_match_sets(ctx_->get(), a, b, th_low, ratio, best_idx.data(), best_dist.data(), second_dist.data()));
    best_idx.resize(na);
    best_dist.resize(na);
    second_dist.resize(na);
  }
  // extractORBwithBinning_fast (:211-318) with flag_nonmax_ (set by initParams, :37): detection and the per-bin
  // arg-max chained on the device. The image is the one held by `slot`.
  void extractORBwithBinning_fast(int slot, PixelVec &pts_extracted) {
    pts_extracted.assign(weight_.size() + 1, Pixel{0.f, 0.f});
    int m = 0;
    ctx_->check(vo_extract_orb_with_binning(ctx_->get(), slot, &orb_, inv_u_step_, inv_v_step_, n_bins_u_, n_bins_v_,
                                            weight_.data(), &pts_extracted.data()->x, &m, nullptr));
    pts_extracted.resize((size_t)m);
  }
  void resetWeightBin() { std::fill(weight_.begin(), weight_.end(), 1); }  // :71-74
  void suppressCenterBins() {                                              // :76-92
    const int u_cent = (int)(n_bins_u_ * 0.5), v_cent = (int)(n_bins_v_ * 0.5);
    const int wu = (int)(0.15f * n_bins_u_), wv = (int)(0.30f * n_bins_v_), wv2 = (int)(0.15f * n_bins_v_);
    for (int w = -wv; w <= wv; ++w) {
      const int v_idx = n_bins_u_ * (w + v_cent - wv2);
      for (int u = -wu; u <= wu; ++u) weight_[(size_t)(v_idx + u + u_cent)] = 0;
    }
  }
  void updateWeightBin(const PixelVec &fts) {  // :94-98
    ctx_->check(vo_weight_bin_update(ctx_->get(), fts.empty() ? zero_ : &fts.data()->x, (int)fts.size(), u_step_, v_step_,
                                     n_bins_u_, n_bins_v_, weight_.data()));
  }
  // the flag_nonmax_ branch of extractORBwithBinning_fast (:241-277) on the detector's keypoints
  void bucketKeypoints(const PixelVec &kp, const std::vector<float> &response, PixelVec &pts_extracted) {
    if (kp.size() != response.size()) throw std::runtime_error("keypoint positions / responses differ in length");
    pts_extracted.assign(weight_.size(), Pixel{0.f, 0.f});
    int m = 0;
    ctx_->check(vo_bucket_argmax(ctx_->get(), kp.empty() ? zero_ : &kp.data()->x, response.empty() ? zero_ : response.data(),
                                 (int)kp.size(), inv_u_step_, inv_v_step_, n_bins_u_, n_bins_v_, weight_.data(),
                                 &pts_extracted.data()->x, nullptr, &m));
    pts_extracted.resize((size_t)m);
  }
  const std::vector<std::int32_t> &weightBin() const { return weight_; }

  // all pairs: dist[i*nb + j]
  void descriptorDistance(const std::uint8_t *a, int na, const std::uint8_t *b, int nb,
                          std::vector<std::uint16_t> &dist) {
    dist.assign((size_t)na * nb, 0);
    if (na && nb) ctx_->check(vo_orb_hamming(ctx_->get(), a, na, b, nb, dist.data()));
  }

 private:
  ContextPtr ctx_;
  int n_bins_u_ = 0, n_bins_v_ = 0, u_step_ = 1, v_step_ = 1;
  float inv_u_step_ = 1.f, inv_v_step_ = 1.f;
  std::vector<std::int32_t> weight_;
  vo_orb_params orb_{10000, 1.2, 8, 31, 15};
  float zero_[2] = {0.f, 0.f};
  int set_size_[2] = {-1, -1};
};

}  // namespace vo
#endif
