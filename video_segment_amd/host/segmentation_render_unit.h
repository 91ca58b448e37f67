// segmentation_render_unit.h -- SegmentationRenderUnit: drop-in for the reference's unit of the same
// name (segmentation/segmentation_unit.h:281-326, segmentation_unit.cpp:478-655), rendering on an
// MI355X through the C ABI in include/vsg_render.h.
//
// Same stream contract: reads "SegmentationStream" and, unless video_stream_name is empty, the BGR24
// "VideoStream"; appends a BGR24 "RenderedRegionStream" of H rows (2 * H with concat_with_source).
// Not drawn: shape descriptors (draw_shape_descriptors is refused) and the two cv::putText overlays.
#ifndef VSG_HOST_SEGMENTATION_RENDER_UNIT_H_
#define VSG_HOST_SEGMENTATION_RENDER_UNIT_H_

#include <list>
#include <string>
#include <vector>

#include "../../include/vsg_render.h"
#include "segmentation_unit.h"
#include "video_framework.h"

namespace segmentation {

// Same fields and defaults as the reference (segmentation_unit.h:281-297).
struct SegmentationRenderUnitOptions {
  // Optional when blend_alpha == 1.
  std::string video_stream_name = "VideoStream";
  std::string segment_stream_name = "SegmentationStream";
  std::string out_stream_name = "RenderedRegionStream";
  float blend_alpha = 0.5f;
  // >= 1: absolute level, 0: over-segmentation, (0, 1): fraction of the first chunk's levels.
  float hierarchy_level = 0;
  bool highlight_edges = true;
  bool draw_shape_descriptors = false;   // not offered: OpenStreams fails when set
  bool concat_with_source = false;
  int device = -1;                       // HIP device ordinal (-1: current)
  // Not in the reference.  >= 0: a volume session (vsg_render_volume_begin) at this hierarchy level accumulates
  // every frame the unit renders, with the colour sums when there is a video stream and without labels; the
  // frame index is the unit's frame number.  < 0: none.
  int volume_level = -1;
};

class SegmentationRenderUnit : public VideoUnit {
 public:
  explicit SegmentationRenderUnit(const SegmentationRenderUnitOptions& options);
  virtual ~SegmentationRenderUnit();

  virtual bool OpenStreams(StreamSet* set);
  virtual void ProcessFrame(FrameSetPtr input, std::list<FrameSetPtr>* output);

  // The level resolved on the first frame (-1 before it).
  int hierarchy_level() const;

  // The table of the volume session over the frames rendered so far (options.volume_level >= 0): one row per
  // supervoxel; cols and pairs stay empty, the session has no labels.  false without a session or on a failure.
  bool VolumeTable(std::vector<vsg_render_volume_row>* rows, std::vector<vsg_render_volume_col>* cols,
                   std::vector<vsg_render_volume_pair>* pairs) const;

 private:
  SegmentationRenderUnitOptions options_;
  int vid_stream_idx_ = -1, seg_stream_idx_ = -1;
  int frame_width_ = 0, frame_height_ = 0, frame_width_step_ = 0;
  int frame_number_ = 0;
  vsg_render* render_ = nullptr;
};

}  // namespace segmentation

#endif  // VSG_HOST_SEGMENTATION_RENDER_UNIT_H_
