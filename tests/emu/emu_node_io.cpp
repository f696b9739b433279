// emu_node_io.cpp — TEST INFRASTRUCTURE: the text of csrc/ingest_formats.hpp (one output byte of the rectifying ingestion per
// pixel format) and of csrc/draw_device.hpp (the debug image's primitives, coverage and colours) compiled by g++ and run on the
// CPU, driven as pyramid.hip / draw.hip drive them.
//   emu_node_io <in.bin> <out.bin>
// in.bin, ingestion: int 0, format, w, h, stride; h * stride source bytes; w * h float map_u; w * h float map_v
//         -> w * h bytes (level 0 without its border)
// in.bin, drawing:   int 1, mode, n0, n1, n2, w, h; 2 n0 + 2 n1 + 2 n2 floats; w * h gray bytes
//         -> h * w * 3 bytes
#include "hip_emu.h"

#include <stdio.h>
#include <stdlib.h>

#include "../../visual_odometry_ros_amd/csrc/draw_device.hpp"
#include "../../visual_odometry_ros_amd/csrc/ingest_formats.hpp"

template <int FMT>
static void ingest(const uint8_t *src, int w, int h, int stride, const float *mu, const float *mv, uint8_t *out) {
  for (int i = 0; i < w * h; ++i) out[i] = (uint8_t)ingest_sample<FMT>(src, w, h, stride, mu[i], mv[i]);
}

int main(int argc, char **argv) {
  if (argc < 3) return 2;
  FILE *f = fopen(argv[1], "rb");
  if (!f) return 3;
  int mode;
  if (fread(&mode, sizeof(int), 1, f) != 1) return 3;
  std::vector<uint8_t> out;
  if (mode == 0) {
    int hd[4];
    if (fread(hd, sizeof(int), 4, f) != 4) return 3;
    const int fmt = hd[0], w = hd[1], h = hd[2], stride = hd[3];
    if (w < 1 || h < 1 || stride < w) return 3;
    std::vector<uint8_t> src((size_t)h * stride);
    std::vector<float> mu((size_t)w * h), mv((size_t)w * h);
    if (fread(src.data(), 1, src.size(), f) != src.size() || fread(mu.data(), sizeof(float), mu.size(), f) != mu.size() ||
        fread(mv.data(), sizeof(float), mv.size(), f) != mv.size())
      return 3;
    out.resize((size_t)w * h);
    switch (fmt) {
      case VO_PIX_MONO8: ingest<VO_PIX_MONO8>(src.data(), w, h, stride, mu.data(), mv.data(), out.data()); break;
      case VO_PIX_RGB8: ingest<VO_PIX_RGB8>(src.data(), w, h, stride, mu.data(), mv.data(), out.data()); break;
      case VO_PIX_BGR8: ingest<VO_PIX_BGR8>(src.data(), w, h, stride, mu.data(), mv.data(), out.data()); break;
      case VO_PIX_MONO16U: ingest<VO_PIX_MONO16U>(src.data(), w, h, stride, mu.data(), mv.data(), out.data()); break;
      case VO_PIX_MONO16S: ingest<VO_PIX_MONO16S>(src.data(), w, h, stride, mu.data(), mv.data(), out.data()); break;
      case VO_PIX_F32: ingest<VO_PIX_F32>(src.data(), w, h, stride, mu.data(), mv.data(), out.data()); break;
      default: return 3;
    }
  } else if (mode == 1) {
    int hd[6];
    if (fread(hd, sizeof(int), 6, f) != 6) return 3;
    DrawJob j;
    memset(&j, 0, sizeof(j));
    j.mode = hd[0];
    j.n0 = hd[1];
    j.n1 = hd[2];
    j.n2 = hd[3];
    j.w = hd[4];
    j.h = hd[5];
    if (j.n0 < 0 || j.n1 < 0 || j.n2 < 0 || j.w < 1 || j.h < 1) return 3;
    std::vector<float> p0(2 * (size_t)j.n0 + 2), p1(2 * (size_t)j.n1 + 2), p2(2 * (size_t)j.n2 + 2);
    std::vector<uint8_t> gray((size_t)j.w * j.h);
    if (fread(p0.data(), sizeof(float), 2 * (size_t)j.n0, f) != 2 * (size_t)j.n0 || fread(p1.data(), sizeof(float), 2 * (size_t)j.n1, f) != 2 * (size_t)j.n1 ||
        fread(p2.data(), sizeof(float), 2 * (size_t)j.n2, f) != 2 * (size_t)j.n2 || fread(gray.data(), 1, gray.size(), f) != gray.size())
      return 3;
    j.p0 = p0.data();
    j.p1 = p1.data();
    j.p2 = p2.data();
    std::vector<uint32_t> idx(gray.size(), 0u);
    const int n_prims = draw_prim_count(j);
    for (int prim = 0; prim < n_prims; ++prim)
      for (int lane = 0; lane < 64; ++lane)
        draw_cover(j, prim, lane, 64, [&](int x, int y) {
          if (x < 0 || x >= j.w || y < 0 || y >= j.h) abort();  // the coverage must clip
          uint32_t &t = idx[(size_t)y * j.w + x];
          if (t < (uint32_t)prim + 1u) t = (uint32_t)prim + 1u;
        });
    out.resize(gray.size() * 3);
    for (size_t i = 0; i < gray.size(); ++i) {
      const uint32_t c = idx[i] ? draw_colour(j, (int)idx[i] - 1) : 0x00010101u * gray[i];
      out[3 * i] = (uint8_t)c;
      out[3 * i + 1] = (uint8_t)(c >> 8);
      out[3 * i + 2] = (uint8_t)(c >> 16);
    }
  } else {
    return 3;
  }
  fclose(f);
  FILE *o = fopen(argv[2], "wb");
  if (!o) return 4;
  fwrite(out.data(), 1, out.size(), o);
  fclose(o);
  return 0;
}
