// orb_describe_demo.cpp — vo::FeatureExtractor::extractAndComputeORB / matchSets through the C++ surface alone: the
// detect -> describe -> match chain of the reference's test/test_orbmatching.cpp on a stereo pair.
// argv: raw file (left then right image, w x h u8), w, h, FAST threshold, output file. Output: int n, then xy, octave,
// angle, size, descriptors of the left image and best index / best distance of every left keypoint in the right image.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "visual_odometry_ros_amd/core/visual_odometry/feature_extractor.h"

template <typename T>
static void wr(FILE *f, const std::vector<T> &v) {
  if (!v.empty()) fwrite(v.data(), sizeof(T), v.size(), f);
}

int main(int argc, char **argv) {
  if (argc < 6) return 1;
  const int w = atoi(argv[2]), h = atoi(argv[3]), thr = atoi(argv[4]);
  FILE *f = fopen(argv[1], "rb");
  if (!f) return 1;
  std::vector<unsigned char> buf((size_t)w * h * 2);
  if (fread(buf.data(), 1, buf.size(), f) != buf.size()) return 2;
  fclose(f);
  try {
    auto ctx = std::make_shared<vo::Context>(0, w, h, 2048, 2, 4);
    vo::FeatureExtractor fe(ctx);
    fe.initParams(w, h, 20, 12, thr);
    fe.setOrbParams(thr);
    vo::PixelVec kp[2];
    std::vector<float> resp[2], angle[2], size[2];
    std::vector<std::int32_t> oct[2], best;
    std::vector<std::uint8_t> desc[2];
    std::vector<std::uint16_t> bd, sd;
    for (int k = 0; k < 2; ++k) {
      ctx->check(vo_set_image(ctx->get(), k, buf.data() + (size_t)k * w * h, w, h, w));
      fe.extractAndComputeORB(k, kp[k], resp[k], oct[k], angle[k], size[k], desc[k], k);
    }
    fe.matchSets(0, 1, best, bd, sd);
    int accepted = 0;
    for (int b : best) accepted += b >= 0;
    printf("left %zu right %zu accepted %d\n", kp[0].size(), kp[1].size(), accepted);
    FILE *o = fopen(argv[5], "wb");
    if (!o) return 1;
    const int n = (int)kp[0].size();
    fwrite(&n, sizeof(int), 1, o);
    if (n) fwrite(kp[0].data(), sizeof(vo::Pixel), kp[0].size(), o);
    wr(o, oct[0]);
    wr(o, angle[0]);
    wr(o, size[0]);
    wr(o, desc[0]);
    wr(o, best);
    wr(o, bd);
    fclose(o);
  } catch (const std::exception &e) {
    printf("error %s\n", e.what());
    return 3;
  }
  return 0;
}
