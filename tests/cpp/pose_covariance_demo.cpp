// pose_covariance_demo.cpp — drives vo::StereoVO (core/visual_odometry/stereo_vo.h) with setPoseCovariance(true) over a short stereo
// sequence and prints, per frame, what a node puts into nav_msgs::Odometry::pose.covariance: the three lines of INTEGRATION.md.
// Input (argv[1]): the file of stereo_vo_demo.cpp. Output (argv[2]): one text line per frame: frame id, the 36 values of
// getPoseCovarianceRos() (row-major, %.17g), valid, n_unknown_steps.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "visual_odometry_ros_amd/core/visual_odometry/stereo_vo.h"

int main(int argc, char **argv) {
  if (argc < 3) return 1;
  FILE *f = fopen(argv[1], "rb");
  if (!f) return 1;
  int hdr[9];
  float fl[26];
  if (fread(hdr, sizeof(int), 9, f) != 9 || fread(fl, sizeof(float), 26, f) != 26) return 2;
  const int n = hdr[0], w = hdr[1], h = hdr[2];
  std::vector<std::vector<unsigned char>> L(n), R(n);
  for (int k = 0; k < n; ++k) {
    L[k].resize((size_t)w * h);
    R[k].resize((size_t)w * h);
    if (fread(L[k].data(), 1, L[k].size(), f) != L[k].size() || fread(R[k].data(), 1, R[k].size(), f) != R[k].size()) return 2;
  }
  fclose(f);
  vo::StereoVOParams p;
  p.width = w;
  p.height = h;
  for (int k = 0; k < 4; ++k) p.Kl[k] = p.Kr[k] = fl[k];
  for (int k = 0; k < 16; ++k) p.T_lr[(size_t)k] = fl[4 + k];
  p.feature_extractor.n_bins_u = hdr[3];
  p.feature_extractor.n_bins_v = hdr[4];
  p.feature_extractor.thres_fastscore = 15.0f;
  p.feature_tracker.window_size = hdr[5];
  p.feature_tracker.max_level = hdr[6];
  p.feature_tracker.thres_error = fl[20];
  p.feature_tracker.thres_bidirection = fl[21];
  p.motion_estimator.thres_poseba_error = fl[22];
  p.keyframe_update.thres_alive_ratio = fl[23];
  p.keyframe_update.thres_trans = fl[24];
  p.keyframe_update.thres_rotation = fl[25];
  p.local_ba = hdr[8] != 0;
  FILE *o = fopen(argv[2], "w");
  if (!o) return 1;
  try {
    auto ctx = std::make_shared<vo::Context>(0, w, h, 4096, 5, p.feature_tracker.max_level);
    vo::StereoVO stereo_vo(ctx, p);
    stereo_vo.setPoseCovariance(true);
    for (int k = 0; k < n; ++k) {
      stereo_vo.trackStereoImages(vo::Image(L[k].data(), w, h, w), vo::Image(R[k].data(), w, h, w), 0.1 * k);
      const vo::PoseCovariance cov = stereo_vo.getPoseCovariance();
      const std::array<double, 36> ros = stereo_vo.getPoseCovarianceRos();  // -> msg.pose.covariance
      fprintf(o, "%d", stereo_vo.lastFrameInfo().frame_id);
      for (double v : ros) fprintf(o, " %.17g", v);
      fprintf(o, " %d %d\n", cov.valid ? 1 : 0, cov.n_unknown_steps);
    }
  } catch (const std::exception &e) {
    fprintf(stderr, "pose_covariance_demo: %s\n", e.what());
    fclose(o);
    return 4;
  }
  fclose(o);
  return 0;
}
