// vo_context.h — RAII owner of a vo_ctx shared by the host-side classes.
#ifndef VO_AMD_CONTEXT_H_
#define VO_AMD_CONTEXT_H_

#include <memory>
#include <stdexcept>
#include <string>

#include "../../../include/vo_hip.h"

namespace vo {

class Context {
 public:
  explicit Context(int device = 0, int max_width = 1241, int max_height = 376, int max_points = 4096,
                   int n_slots = 4, int max_level = 6) {
    vo_config cfg{device, max_width, max_height, max_points, n_slots, max_level};
    const int rc = vo_create(&cfg, &ctx_);
    if (rc != VO_OK) {
      std::string msg = vo_last_error(ctx_);
      if (ctx_) vo_destroy(ctx_);
      ctx_ = nullptr;
      throw std::runtime_error("libvo_hip: " + msg);  // no CPU fallback
    }
    n_slots_ = n_slots;
  }
  ~Context() {
    if (ctx_) vo_destroy(ctx_);
  }
  Context(const Context &) = delete;
  Context &operator=(const Context &) = delete;
  vo_ctx *get() const { return ctx_; }
  int n_slots() const { return n_slots_; }
  // summation order of the IC and GN reductions (vo_set_sum_order): VO_SUM_ORDER_TREE (the default) or
  // VO_SUM_ORDER_REFERENCE; every class that shares this context follows it from its next call or frame
  void setSumOrder(int order) { check(vo_set_sum_order(ctx_, order)); }
  int sumOrder() const { return check(vo_get_sum_order(ctx_)); }
  // pixel format of the images the undistorting / rectifying ingestion takes (vo_set_input_format): VO_PIX_MONO8 (the
  // default) .. VO_PIX_F32. Camera::undistortImage, StereoCamera::rectifyStereoImages and StereoVO / MonoVO with
  // flagDoUndistortion then take vo::Image of that format; everything else keeps taking u8 planes.
  void setInputFormat(int format) {
    check(vo_set_input_format(ctx_, format));
    format_ = format;
  }
  int inputFormat() const { return format_; }
  // CLAHE equalisation in front of every ingestion of this context (vo_set_equalize): mode VO_EQ_CLAHE / VO_EQ_OFF, OpenCV's
  // defaults. Refused (throws) while the input format is not VO_PIX_MONO8 and while a frame is in flight.
  void setEqualize(int mode, double clip_limit = 40.0, int tiles_x = 8, int tiles_y = 8) {
    check(vo_set_equalize(ctx_, mode, clip_limit, tiles_x, tiles_y));
  }
  // an image handed to the rectifying ingestion (rectifying = true) must be of the context's format, any other a u8 plane
  void checkFormat(int image_format, bool rectifying) const {
    if (image_format != (rectifying ? format_ : (int)VO_PIX_MONO8))
      throw std::runtime_error(rectifying ? "libvo_hip: the image's pixel format differs from the context's (Context::setInputFormat)"
                                          : "libvo_hip: only the undistorting / rectifying ingestion converts pixel formats: a u8 plane expected");
  }
  // maps the reference's throw sites / return-false onto the C status codes
  int check(int rc) const {
    if (rc < 0) throw std::runtime_error(vo_last_error(ctx_));
    return rc;
  }

 private:
  vo_ctx *ctx_ = nullptr;
  int n_slots_ = 0;
  int format_ = VO_PIX_MONO8;
};
using ContextPtr = std::shared_ptr<Context>;

}  // namespace vo
#endif
