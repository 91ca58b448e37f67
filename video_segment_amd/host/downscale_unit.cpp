// downscale_unit.cpp -- see downscale_unit.h.
#include "downscale_unit.h"

#include <cstdio>

#include "../../include/vsg_resize.h"

namespace video_framework {

DownscaleUnit::~DownscaleUnit() {
  if (resize_) vsg_resize_destroy(resize_);
}

bool DownscaleUnit::OpenStreams(StreamSet* set) {
  auto fail = [](const char* what) {
    std::fprintf(stderr, "ERROR: DownscaleUnit: %s\n", what);
    return false;
  };
  video_stream_idx_ = FindStreamIdx(options_.stream_name, set);
  if (video_stream_idx_ < 0) return fail("could not find video stream");
  const VideoStream& vid_stream = set->at(video_stream_idx_)->As<VideoStream>();
  if (vid_stream.pixel_format() != PIXEL_FORMAT_BGR24) return fail("only BGR24 input is supported");
  frame_width_ = vid_stream.frame_width();
  frame_height_ = vid_stream.frame_height();
  if (options_.downscale == DownscaleUnitOptions::DOWNSCALE_BY_FACTOR && options_.downscale_factor > 1.0f) {
    return fail("Only downscaling is supported.");   // video_reader_unit.cpp:163-166
  }

  vsg_resize_options ro;
  vsg_resize_default_options(&ro);
  switch (options_.downscale) {
    case DownscaleUnitOptions::DOWNSCALE_NONE: ro.mode = VSG_RESIZE_NONE; break;
    case DownscaleUnitOptions::DOWNSCALE_BY_FACTOR: ro.mode = VSG_RESIZE_BY_FACTOR; break;
    case DownscaleUnitOptions::DOWNSCALE_TO_MIN_SIZE: ro.mode = VSG_RESIZE_TO_MIN_SIZE; break;
    case DownscaleUnitOptions::DOWNSCALE_TO_MAX_SIZE: ro.mode = VSG_RESIZE_TO_MAX_SIZE; break;
  }
  ro.factor = options_.downscale_factor;
  ro.size = options_.downscale_size;
  ro.device = options_.device;
  if (vsg_resize_create(&ro, frame_width_, frame_height_, &resize_) != VSG_OK) return fail(vsg_resize_last_error());
  if (vsg_resize_get_output_size(resize_, &output_width_, &output_height_, &output_width_step_) != VSG_OK) {
    return fail(vsg_resize_last_error());
  }

  // The stream of the downscaled frames takes the place of the incoming one.  An original size the
  // incoming stream already carries (a source that was downscaled before) is kept.
  std::shared_ptr<VideoStream> scaled(new VideoStream(output_width_, output_height_, output_width_step_,
                                                      vid_stream.fps(), PIXEL_FORMAT_BGR24, options_.stream_name));
  scaled->set_original_size(vid_stream.original_width(), vid_stream.original_height());
  set->at(video_stream_idx_) = scaled;
  return true;
}

void DownscaleUnit::ProcessFrame(FrameSetPtr input, std::list<FrameSetPtr>* output) {
  const VideoFrame& frame = input->at(video_stream_idx_)->As<VideoFrame>();
  VF_CHECK(frame.width() == frame_width_ && frame.height() == frame_height_ && frame.channels() == 3,
           "DownscaleUnit: the frame is not of the stream's size");
  std::shared_ptr<VideoFrame> scaled(new VideoFrame(output_width_, output_height_, 3, output_width_step_, frame.pts()));
  VF_CHECK(vsg_resize_process(resize_, frame.data(), (size_t)frame.width_step(), VSG_MEM_HOST, scaled->mutable_data(),
                              (size_t)output_width_step_, VSG_MEM_HOST) == VSG_OK,
           vsg_resize_last_error());
  input->at(video_stream_idx_) = scaled;   // every other stream of the frame set stays as it is
  output->push_back(input);
}

}  // namespace video_framework
