// downscale_unit.h -- the downscale the reference's reader applies to every frame
// (VideoReaderOptions::downscale, video_framework/video_reader_unit.{h,cpp}:155-206, :374) as a unit
// of its own on top of libvsg_resize.so (include/vsg_resize.h).  It follows a root unit
// (RawVideoReaderUnit, a synthetic source) where the reference's reader does its own scaling, and
// records the size before the downscale in the stream, which the writer scales its vectorization
// back to (segmentation_unit.cpp:379-395).  The output size is the reference's rule; the resampling
// is the one tests/resize_model.py defines (parity with swscale is unpinned), computed on the device.
#ifndef VSG_HOST_DOWNSCALE_UNIT_H_
#define VSG_HOST_DOWNSCALE_UNIT_H_

#include <string>

#include "video_framework.h"

struct vsg_resize;

namespace video_framework {

struct DownscaleUnitOptions {
  enum DownScale { DOWNSCALE_NONE, DOWNSCALE_BY_FACTOR, DOWNSCALE_TO_MIN_SIZE, DOWNSCALE_TO_MAX_SIZE };
  DownScale downscale = DOWNSCALE_NONE;
  float downscale_factor = 0.5f;   // DOWNSCALE_BY_FACTOR
  int downscale_size = 0;          // the two size modes: the length of the smaller / larger side
  std::string stream_name = "VideoStream";
  int device = -1;                 // not in the reference: HIP device, -1 = current
};

class DownscaleUnit : public VideoUnit {
 public:
  explicit DownscaleUnit(const DownscaleUnitOptions& options) : options_(options) {}
  ~DownscaleUnit() override;
  bool OpenStreams(StreamSet* set) override;
  void ProcessFrame(FrameSetPtr input, std::list<FrameSetPtr>* output) override;
  bool PostProcess(std::list<FrameSetPtr>* append) override { return false; }

  int output_width() const { return output_width_; }
  int output_height() const { return output_height_; }

 private:
  DownscaleUnitOptions options_;
  int video_stream_idx_ = -1;
  int frame_width_ = 0, frame_height_ = 0;
  int output_width_ = 0, output_height_ = 0, output_width_step_ = 0;
  vsg_resize* resize_ = nullptr;
};

}  // namespace video_framework

#endif  // VSG_HOST_DOWNSCALE_UNIT_H_
