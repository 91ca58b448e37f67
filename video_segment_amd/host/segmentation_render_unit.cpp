// segmentation_render_unit.cpp -- see segmentation_render_unit.h.  Stream handling restated from the
// reference's SegmentationRenderUnit (segmentation/segmentation_unit.cpp:478-655); the hierarchy
// state, the colours and every pixel are the library's (include/vsg_render.h).
#include "segmentation_render_unit.h"

#include <cstdio>

namespace segmentation {

SegmentationRenderUnit::SegmentationRenderUnit(const SegmentationRenderUnitOptions& options)
    : options_(options) {}

SegmentationRenderUnit::~SegmentationRenderUnit() { vsg_render_destroy(render_); }

bool SegmentationRenderUnit::OpenStreams(StreamSet* set) {
  if (options_.draw_shape_descriptors) {
    std::fprintf(stderr, "ERROR: draw_shape_descriptors is not supported by the HIP renderer\n");
    return false;
  }
  float fps = 0;
  if (options_.video_stream_name.empty()) {
    if (options_.blend_alpha != 1.f) {
      options_.blend_alpha = 1.f;
      std::fprintf(stderr, "WARNING: No video stream request. Fixing blend alpha to 1.\n");
    }
    fps = 25;   // standard value
    vid_stream_idx_ = -1;
  } else {
    vid_stream_idx_ = FindStreamIdx(options_.video_stream_name, set);
    if (vid_stream_idx_ < 0) {
      std::fprintf(stderr, "ERROR: Could not find Video stream!\n");
      return false;
    }
    const VideoStream& vid_stream = set->at(vid_stream_idx_)->As<VideoStream>();
    if (vid_stream.pixel_format() != PIXEL_FORMAT_BGR24) {
      std::fprintf(stderr, "ERROR: Expecting video format to be BGR24.\n");
      return false;
    }
    frame_width_ = vid_stream.frame_width();
    frame_height_ = vid_stream.frame_height();
    frame_width_step_ = vid_stream.width_step();
    fps = vid_stream.fps();
  }
  seg_stream_idx_ = FindStreamIdx(options_.segment_stream_name, set);
  if (seg_stream_idx_ < 0) {
    std::fprintf(stderr, "ERROR: SegmentationRenderUnit::OpenStreams: Could not find Segmentation stream!\n");
    return false;
  }
  if (frame_width_ == 0) {   // dimensions from the segmentation stream
    const SegmentationStream& seg_stream = set->at(seg_stream_idx_)->As<SegmentationStream>();
    frame_width_ = seg_stream.frame_width();
    frame_height_ = seg_stream.frame_height();
    frame_width_step_ = (int)vsg_render_default_stride(frame_width_);
  }
  if (options_.concat_with_source && vid_stream_idx_ < 0) {
    std::fprintf(stderr, "ERROR: Request concatenation with source but no video stream present.\n");
    return false;
  }
  const int actual_height = frame_height_ * (options_.concat_with_source ? 2 : 1);
  set->push_back(std::shared_ptr<DataStream>(new VideoStream(
      frame_width_, actual_height, frame_width_step_, fps, PIXEL_FORMAT_BGR24, options_.out_stream_name)));

  vsg_render_options o;
  vsg_render_default_options(&o);
  o.blend_alpha = options_.blend_alpha;
  o.hierarchy_level = options_.hierarchy_level;
  o.highlight_edges = options_.highlight_edges ? 1 : 0;
  o.concat_with_source = options_.concat_with_source ? 1 : 0;
  o.has_video = vid_stream_idx_ >= 0 ? 1 : 0;
  o.device = options_.device;
  if (vsg_render_create(&o, frame_width_, frame_height_, &render_) != VSG_OK) {
    render_ = nullptr;
    std::fprintf(stderr, "ERROR: could not create the HIP renderer: %s\n", vsg_render_last_error());
    return false;
  }
  if (options_.volume_level >= 0 &&
      vsg_render_volume_begin(render_, options_.volume_level, vid_stream_idx_ >= 0 ? 1 : 0, 0) != VSG_OK) {
    std::fprintf(stderr, "ERROR: could not begin the volume session: %s\n", vsg_render_last_error());
    return false;
  }
  return true;
}

void SegmentationRenderUnit::ProcessFrame(FrameSetPtr input, std::list<FrameSetPtr>* output) {
  int64_t pts = (int64_t)frame_number_ * 100;   // dummy pts, if no video frame present
  const uint8_t* bgr = nullptr;
  size_t stride = 0;
  if (vid_stream_idx_ >= 0) {
    VF_CHECK(input->at(vid_stream_idx_) != nullptr, "the video frame was freed before the render unit");
    const VideoFrame& frame = input->at(vid_stream_idx_)->As<VideoFrame>();
    bgr = frame.data();
    stride = (size_t)frame.width_step();
    pts = frame.pts();
  }
  const SegmentationDesc& desc = input->at(seg_stream_idx_)->As<PointerFrame<SegmentationDesc>>().Ref();
  std::shared_ptr<VideoFrame> render_frame(new VideoFrame(
      frame_width_, frame_height_ * (options_.concat_with_source ? 2 : 1), 3, frame_width_step_, pts));
  VF_CHECK(vsg_render_frame(render_, reinterpret_cast<const uint8_t*>(desc.wire.data()), desc.wire.size(), bgr,
                            stride, VSG_MEM_HOST, render_frame->mutable_data(), (size_t)frame_width_step_,
                            VSG_MEM_HOST) == VSG_OK,
           vsg_render_last_error());
  if (options_.volume_level >= 0) {   // after the render: a desc without a hierarchy uses the kept one
    VF_CHECK(vsg_render_volume_add(render_, reinterpret_cast<const uint8_t*>(desc.wire.data()), desc.wire.size(),
                                   frame_number_, bgr, stride, VSG_MEM_HOST, nullptr, 0, VSG_MEM_HOST) == VSG_OK,
             vsg_render_last_error());
  }
  input->push_back(render_frame);
  output->push_back(input);
  ++frame_number_;
}

int SegmentationRenderUnit::hierarchy_level() const {
  int level = -1;
  if (!render_ || vsg_render_level(render_, &level) != VSG_OK) return -1;
  return level;
}

bool SegmentationRenderUnit::VolumeTable(std::vector<vsg_render_volume_row>* rows,
                                         std::vector<vsg_render_volume_col>* cols,
                                         std::vector<vsg_render_volume_pair>* pairs) const {
  if (!render_ || options_.volume_level < 0) return false;
  size_t nr = 0, nc = 0, np = 0;
  if (vsg_render_volume_table(render_, nullptr, 0, &nr, nullptr, 0, &nc, nullptr, 0, &np, VSG_MEM_HOST) != VSG_OK) {
    return false;
  }
  rows->resize(nr);
  cols->resize(nc);
  pairs->resize(np);
  if (nr + nc + np == 0) return true;
  return vsg_render_volume_table(render_, rows->data(), nr, &nr, cols->data(), nc, &nc, pairs->data(), np, &np,
                                 VSG_MEM_HOST) == VSG_OK;
}

}  // namespace segmentation
