// dense_flow_unit.h -- LuminanceUnit (video_framework/conversion_units.{h,cpp}:40-109) and
// DenseFlowUnit (video_framework/flow_reader.{h,cpp}:141-371) on top of libvsg_flow.so
// (include/vsg_flow.h): the pair seg_tree.cpp:170-187 inserts in front of the DenseSegmentationUnit
// when --flow is on and no .flow file exists.  The flow is Dual TV-L1 as tests/flow_model.py defines
// it, computed on the device; the unit's streams, first-frame behaviour and .flow output are the
// reference's.
#ifndef VSG_HOST_DENSE_FLOW_UNIT_H_
#define VSG_HOST_DENSE_FLOW_UNIT_H_

#include <memory>
#include <string>

#include "flow_reader.h"
#include "video_framework.h"

struct vsg_flow;

namespace video_framework {

struct LuminanceUnitOptions {
  std::string video_stream_name = "VideoStream";
  std::string luminance_stream_name = "LuminanceStream";
};

// BGR24 -> 8-bit luminance, cvtColor(CV_BGR2GRAY) (conversion_units.cpp:75-109); the other pixel
// formats the reference converts are refused.
class LuminanceUnit : public VideoUnit {
 public:
  explicit LuminanceUnit(const LuminanceUnitOptions& options = LuminanceUnitOptions()) : options_(options) {}
  bool OpenStreams(StreamSet* set) override;
  void ProcessFrame(FrameSetPtr input, std::list<FrameSetPtr>* output) override;
  bool PostProcess(std::list<FrameSetPtr>* append) override { return false; }

 private:
  LuminanceUnitOptions options_;
  int video_stream_idx_ = -1;
  int frame_width_ = 0, frame_height_ = 0, width_step_ = 0;
};

struct DenseFlowOptions {
  DenseFlowType flow_type = FLOW_BACKWARD;
  int flow_iterations = 10;
  int num_warps = 2;
  std::string input_stream_name = "LuminanceStream";
  std::string backward_flow_stream_name = "BackwardFlowStream";
  std::string forward_flow_stream_name = "ForwardFlowStream";
  std::string video_out_stream_name;   // the HSV picture of the flow: refused
  std::string flow_output_file;
  int device = -1;                     // not in the reference: HIP device, -1 = current
};

class DenseFlowUnit : public VideoUnit {
 public:
  explicit DenseFlowUnit(const DenseFlowOptions& options) : options_(options) {}
  ~DenseFlowUnit() override;
  bool OpenStreams(StreamSet* set) override;
  void ProcessFrame(FrameSetPtr input, std::list<FrameSetPtr>* output) override;
  bool PostProcess(std::list<FrameSetPtr>* append) override;

 private:
  DenseFlowOptions options_;
  int video_stream_idx_ = -1;
  int frame_number_ = 0;
  vsg_flow* flow_ = nullptr;
  std::unique_ptr<DenseFlowWriter> writer_;
};

}  // namespace video_framework

#endif  // VSG_HOST_DENSE_FLOW_UNIT_H_
