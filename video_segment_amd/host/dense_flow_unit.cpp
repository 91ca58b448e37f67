// dense_flow_unit.cpp -- see dense_flow_unit.h.
#include "dense_flow_unit.h"

#include <cstdio>

#include "../../include/vsg_flow.h"

namespace video_framework {

bool LuminanceUnit::OpenStreams(StreamSet* set) {
  video_stream_idx_ = FindStreamIdx(options_.video_stream_name, set);
  if (video_stream_idx_ < 0) {
    std::fprintf(stderr, "ERROR: LuminanceUnit: could not find video stream\n");
    return false;
  }
  const VideoStream& vid_stream = set->at(video_stream_idx_)->As<VideoStream>();
  frame_width_ = vid_stream.frame_width();
  frame_height_ = vid_stream.frame_height();
  if (vid_stream.pixel_format() != PIXEL_FORMAT_BGR24) {
    std::fprintf(stderr, "ERROR: LuminanceUnit: only BGR24 input is supported\n");
    return false;
  }
  width_step_ = frame_width_;   // conversion_units.cpp:59-63
  if (width_step_ % 4) width_step_ += 4 - width_step_ % 4;
  set->push_back(std::make_shared<VideoStream>(frame_width_, frame_height_, width_step_, vid_stream.fps(),
                                               PIXEL_FORMAT_LUMINANCE, options_.luminance_stream_name));
  return true;
}

void LuminanceUnit::ProcessFrame(FrameSetPtr input, std::list<FrameSetPtr>* output) {
  const VideoFrame& frame = input->at(video_stream_idx_)->As<VideoFrame>();
  std::shared_ptr<VideoFrame> lum(new VideoFrame(frame_width_, frame_height_, 1, width_step_, frame.pts()));
  // vsg_flow_luminance writes packed rows; the stream's rows are width_step_ apart
  std::vector<uint8_t> packed((size_t)frame_width_ * frame_height_);
  VF_CHECK(vsg_flow_luminance(frame.data(), (size_t)frame.width_step(), frame_width_, frame_height_,
                              packed.data()) == VSG_OK,
           vsg_flow_last_error());
  for (int y = 0; y < frame_height_; ++y) {
    std::copy(packed.begin() + (size_t)y * frame_width_, packed.begin() + (size_t)(y + 1) * frame_width_,
              lum->mutable_data() + (size_t)y * width_step_);
  }
  input->push_back(lum);
  output->push_back(input);
}

DenseFlowUnit::~DenseFlowUnit() {
  if (flow_) vsg_flow_destroy(flow_);
}

bool DenseFlowUnit::OpenStreams(StreamSet* set) {
  auto fail = [](const char* what) {
    std::fprintf(stderr, "ERROR: DenseFlowUnit: %s\n", what);
    return false;
  };
  video_stream_idx_ = FindStreamIdx(options_.input_stream_name, set);
  if (video_stream_idx_ < 0) return fail("could not find video stream");
  if (!options_.video_out_stream_name.empty()) {
    return fail("video_out_stream_name (the HSV picture of the flow) is not supported: leave it empty");
  }
  const VideoStream& vid_stream = set->at(video_stream_idx_)->As<VideoStream>();
  if (vid_stream.pixel_format() != PIXEL_FORMAT_LUMINANCE) return fail("expecting luminance input");
  const int width = vid_stream.frame_width(), height = vid_stream.frame_height();
  const bool forward = options_.flow_type == FLOW_FORWARD || options_.flow_type == FLOW_BOTH;
  const bool backward = options_.flow_type == FLOW_BACKWARD || options_.flow_type == FLOW_BOTH;

  vsg_flow_options fo;
  vsg_flow_default_options(&fo);
  fo.flow_type = options_.flow_type == FLOW_BOTH ? VSG_FLOW_BOTH : (forward ? VSG_FLOW_FORWARD : VSG_FLOW_BACKWARD);
  fo.iterations = options_.flow_iterations;
  fo.warps = options_.num_warps;
  fo.device = options_.device;
  if (vsg_flow_create(&fo, width, height, &flow_) != VSG_OK) return fail(vsg_flow_last_error());
  frame_number_ = 0;

  // forward before backward (flow_reader.cpp:215-226)
  if (forward) {
    if (options_.forward_flow_stream_name.empty()) return fail("forward flow stream is empty");
    set->push_back(std::make_shared<DataStream>(options_.forward_flow_stream_name));
  }
  if (backward) {
    if (options_.backward_flow_stream_name.empty()) return fail("backward flow stream is empty");
    set->push_back(std::make_shared<DataStream>(options_.backward_flow_stream_name));
  }
  if (!options_.flow_output_file.empty()) {   // flow_reader.cpp:240-249
    writer_.reset(new DenseFlowWriter(options_.flow_output_file));
    if (!writer_->OpenAndWriteHeader(width, height, options_.flow_type)) return fail("can not open flow_output_file");
  }
  return true;
}

void DenseFlowUnit::ProcessFrame(FrameSetPtr input, std::list<FrameSetPtr>* output) {
  const VideoFrame& frame = input->at(video_stream_idx_)->As<VideoFrame>();
  const int width = frame.width(), height = frame.height();
  const int64_t pts = frame.pts();
  const bool forward = options_.flow_type == FLOW_FORWARD || options_.flow_type == FLOW_BOTH;
  const bool backward = options_.flow_type == FLOW_BACKWARD || options_.flow_type == FLOW_BOTH;
  // The first frame gets zero fields marked as forward ones (flow_reader.cpp:331-345).
  std::shared_ptr<DenseFlowFrame> ff, bf;
  if (forward) ff.reset(new DenseFlowFrame(width, height, false, pts));
  if (backward) bf.reset(new DenseFlowFrame(width, height, frame_number_ > 0, pts));
  int has_flow = 0;
  VF_CHECK(vsg_flow_process_luminance(flow_, frame.data(), (size_t)frame.width_step(), VSG_MEM_HOST,
                                      bf ? bf->mutable_flow() : nullptr, ff ? ff->mutable_flow() : nullptr,
                                      VSG_MEM_HOST, &has_flow) == VSG_OK,
           vsg_flow_last_error());
  VF_CHECK(has_flow == (frame_number_ > 0 ? 1 : 0), "DenseFlowUnit: the library lost track of the first frame");
  if (ff) {
    input->push_back(ff);
    if (writer_ && has_flow) writer_->AddFlowFrame(ff->flow());
  }
  if (bf) {
    input->push_back(bf);
    if (writer_ && has_flow) writer_->AddFlowFrame(bf->flow());
  }
  output->push_back(input);
  ++frame_number_;
}

bool DenseFlowUnit::PostProcess(std::list<FrameSetPtr>* append) {
  if (writer_) writer_->Close();
  return false;
}

}  // namespace video_framework
