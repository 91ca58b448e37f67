// seg_tree_synth.cpp -- the caller of the hot path, mirroring seg_tree_sample's over-segmentation
// wiring (seg_tree_sample/seg_tree.cpp:85-367): root unit -> [flow] -> DenseSegmentationUnit ->
// sink, as a threaded pipeline (--use_pipeline, the default as in the reference) or single threaded.  The H.264 reader and the .flow reader of the reference are replaced
// by an in-process synthetic source (no codec is available in this image).
//
//   seg_tree_synth --width 64 --height 48 --frames 45 --flow --input probe [--nouse_pipeline]
// prints the number of over-segmented frames, Region2D counts and the FNV-1a-32 hash of all region
// id images (the quantity pinned in SURVEY.md App. B), then __SEGMENTATION_FINISHED__.
//
//   --render_level <float> [--render_concat] [--render_blend_alpha <float>]
// puts a SegmentationRenderUnit (seg_tree.cpp --render_and_save) behind the segmentation and prints a
// second line, render_frames=N render_fnv1a32=<FNV-1a-32 of the rendered frames' pixel bytes>.
//
//   --level_regions <level>
// asks vsg_render_level_regions for that hierarchy level's regions of every frame and prints a line
// level_regions=<sum over frames> level_intervals=<sum> level_fnv1a32=<hash of both lists' bytes>.
//
//   --level_components <level> [--components_n8]
// asks vsg_render_level_components for the connected components (N4, or N8) of that level's regions of
// every frame and prints a line
// level_components=<sum> component_intervals=<sum> component_fnv1a32=<hash of both lists' bytes>.
//
//   --level_boundaries <level> [--boundaries_outer] [--boundaries_components [--components_n8]]
// asks vsg_render_level_boundaries for the inner (or outer) N4 boundary points of that level's regions,
// or of their connected components (N4, or N8), of every frame and prints a line
// level_boundaries=<sum> boundary_points=<sum> boundary_fnv1a32=<hash of both lists' bytes>.
//
//   --level_adjacency <level> [--adjacency_n8] [--adjacency_components [--components_n8]]
// asks vsg_render_level_adjacency for the adjacency graph (pixel sides, or with --adjacency_n8 also
// diagonal contacts) of that level's regions, or of their connected components (N4, or N8), of every
// frame and prints a line
// level_adjacency_nodes=<sum> adjacency_edges=<sum> adjacency_fnv1a32=<hash of both lists' bytes, nodes first>.
//
//   --level_overlap <level> [--overlap_components [--components_n8]]
// asks vsg_render_level_overlap, for every frame after the first, for the overlap table of that level's
// regions, or of their connected components (N4, or N8), with the previous frame's id image at that level
// (fetched with vsg_render_id_image into host memory) and prints a line
// level_overlap_rows=<sum> overlap_cols=<sum> overlap_pairs=<sum> overlap_fnv1a32=<hash of the three lists'
// bytes, rows, cols and pairs of every compared frame in that order>.
//
//   --persistence [--adjacency_n8]
// asks vsg_render_persistence_image and vsg_render_persistence_graph (pixel sides, or with --adjacency_n8 also
// diagonal contacts) for the boundary persistence of every frame's hierarchy and prints a line
// persistence_levels=<L of the last frame> persistence_edge_pixels=<sum> persistence_edges=<sum>
// persistence_fnv1a32=<hash of every frame's plane, then persistence, then level_sides bytes>.
//
//   --tree_cut <penalty>
// asks vsg_render_tree_cut, for every frame after the first, for the best cut of the frame's hierarchy against
// the previous frame's level-0 id image (fetched with vsg_render_id_image into host memory) with that penalty
// and prints a line
// tree_cut_nodes=<sum> tree_cut_total=<sum> tree_cut_fnv1a32=<hash of every compared frame's records, then plane>.
//
//   --level_pool <level> [--pool_components [--components_n8]]
// asks vsg_render_level_pool for the sums, sums of squares, minima and maxima of five planar f32 channels (the
// frame's B, G, R, then x and y) over that level's regions, or their connected components, in every frame, and
// prints level_pool_groups=<sum> level_pool_sums=<the five channels' sums over all groups, comma separated>
// level_pool_fnv1a32=<hash of every frame's groups and four matrices>.
//
//   --level_colors <level> [--colors_components [--components_n8]]
// asks vsg_render_level_colors for the colour sums of that level's regions, or of their connected components
// (N4, or N8), in every frame of the video, and vsg_render_mean_frame for the level painted in their mean
// colours (default options: edges, blend 0.5), and prints a line
// level_colors_groups=<sum> level_colors_fnv1a32=<hash of every frame's records, then its mean frame bytes>.
//
//   --level_contours <level> [--contours_components [--components_n8]]
// asks vsg_render_level_contours for the traced outlines of that level's regions, or of their connected
// components, for every frame and prints
// level_contours_count=<sum> level_contours_fnv1a32=<hash of every frame's records, then its vertices' bytes>.
//
//   --level_mesh <level> [--mesh_components [--components_n8]]
// asks vsg_render_level_mesh for the shared-segment mesh of that level's regions, or of their connected
// components, for every frame and prints
// level_mesh_count=<segments over all frames> level_mesh_fnv1a32=<hash of every frame's segments, vertices,
// loops and refs bytes, in that order>.
//
//   --level_mesh <level> --mesh_max_error <e> [--mesh_min_segment_points <n>]
// asks vsg_render_level_mesh_simplified instead (n: 4 when absent; e finite and >= 0, n >= 0; either flag without
// the one before it is refused) and prints
// level_mesh_simplified_count=<segments over all frames> level_mesh_simplified_fnv1a32=<the same hash of its lists>.
//
//   --boundary_distance <level>
// asks vsg_render_boundary_distance for the exact squared distance of every pixel to that level's nearest
// edge pixel, for every frame, and prints a line
// boundary_distance_level=<level> boundary_distance_edge_pixels=<sum> boundary_distance_max=<largest finite
// distance of any frame> boundary_distance_fnv1a32=<hash of every frame's plane bytes>.
//
//   --boundary_benchmark <tolerance_sq>
// asks vsg_render_boundary_benchmark, for every frame after the first, for the boundary records of every
// hierarchy level against the previous frame's level-0 id image (fetched with vsg_render_id_image into host
// memory), boundaries matching within sqrt(tolerance_sq) pixels, and prints a line
// boundary_benchmark_levels=<L of the last frame> boundary_seg_edges=<sum> boundary_seg_matched=<sum>
// boundary_gt_edges=<sum> boundary_gt_matched=<sum> boundary_benchmark_fnv1a32=<hash of every compared
// frame's records>.
//
//   --volume_level <level> [--volume_out FILE]
// gives the SegmentationRenderUnit a volume session at that hierarchy level (--render_level 0 is implied when no
// render level was given): every rendered frame is accumulated on the device, and after the last frame one line
// volume_level=<level> volume_frames=<adds> volume_supervoxels=<rows> volume_voxels=<sum of the volumes>
// volume_fnv1a32=<hash of the rows' bytes> is printed, and one text line per supervoxel,
// "id first_frame last_frame frames volume min_x min_y max_x max_y sum_x sum_y sum_t sum_b sum_g sum_r",
// is written to FILE (to stdout, each line beginning with "supervoxel ", without --volume_out).
//
//   --write_to_file --remove_rasterization [--original_width W --original_height H]
// writes vector-only descs as seg_tree_sample does (seg_tree.cpp:308), scaled to the video's original
// size where the source says it was downscaled; a render unit in the same run is then put behind the
// writer and given the same vector-only descs (at the stream's size), which is what a consumer of the
// file renders.  --rewrite_pb FILE applies the writer's edit to a container (no GPU).
//
//   --downscale_min_size N
// puts a DownscaleUnit (the reader's DOWNSCALE_TO_MIN_SIZE, seg_tree.cpp:136-139) directly behind the
// source: everything after it sees the smaller frames, and the writer scales its vectorization back to
// the source's size.  --run_on_server applies the overrides of seg_tree.cpp:90-98 that exist here:
// use_pipeline on, write_to_file on, downscale_min_size 360, no render unit.
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <string>

#include "dense_flow_unit.h"
#include "../../include/vsg_resize.h"
#include "downscale_unit.h"
#include "flow_reader.h"
#include "raw_video_reader.h"
#include "segmentation_io.h"
#include "segmentation_render_unit.h"
#include "segmentation_unit.h"
#include "video_pipeline.h"

using namespace video_framework;
using namespace segmentation;

namespace {

uint32_t PcgHash(uint32_t v) {
  const uint32_t state = v * 747796405u + 2891336453u;
  const uint32_t word = ((state >> ((state >> 28u) + 4u)) ^ state) * 277803737u;
  return (word >> 22u) ^ word;
}

// Same generators as tests/synth.py (probe_frame / bench_frame / const_flow).
class SyntheticVideoUnit : public VideoUnit {
 public:
  // kind: 0 probe, 1 bench, 2 soft (tests/synth.py: soft_frame, the input of the hierarchical stage)
  SyntheticVideoUnit(int width, int height, int frames, bool flow, int kind,
                     const std::string& save_flow = std::string(), int original_width = 0, int original_height = 0,
                     int flow_width = 0, int flow_height = 0)
      : width_(width), height_(height), frames_(frames), flow_(flow), bench_(kind != 0), soft_(kind == 2),
        save_flow_(save_flow), original_width_(original_width), original_height_(original_height),
        flow_width_(flow_width > 0 ? flow_width : width), flow_height_(flow_height > 0 ? flow_height : height) {}

  bool OpenStreams(StreamSet* set) override {
    width_step_ = (width_ * 3 + 3) / 4 * 4;   // padded like video_reader_unit.cpp:200-206
    std::shared_ptr<VideoStream> video(
        new VideoStream(width_, height_, width_step_, 25.0f, PIXEL_FORMAT_BGR24, "VideoStream"));
    if (original_width_ > 0 && original_height_ > 0) video->set_original_size(original_width_, original_height_);
    set->push_back(video);
    if (flow_) {
      set->push_back(std::shared_ptr<DataStream>(
          new DenseFlowStream(flow_width_, flow_height_, "BackwardFlowStream")));
    }
    if (!save_flow_.empty()) {   // what DenseFlowUnit does with --save_flow (flow_reader.cpp:240-248)
      flow_writer_.reset(new DenseFlowWriter(save_flow_));
      if (!flow_writer_->OpenAndWriteHeader(flow_width_, flow_height_, FLOW_BACKWARD)) return false;
    }
    return true;
  }

  bool PostProcess(std::list<FrameSetPtr>* append) override {
    if (k_ >= frames_) {
      if (flow_writer_) flow_writer_->Close();
      return false;
    }
    FrameSetPtr fs(new FrameSet);
    std::shared_ptr<VideoFrame> vf(new VideoFrame(width_, height_, 3, width_step_, (int64_t)k_ * 40000));
    uint8_t* d = vf->mutable_data();
    const int cw = bench_ ? std::max(1, 16 * width_ / 64) : 16;
    const int ch = bench_ ? std::max(1, 12 * width_ / 64) : 12;
    const uint32_t base = PcgHash((uint32_t)(1234 + k_));
    for (int y = 0; y < height_; ++y) {
      uint8_t* row = d + (size_t)y * width_step_;
      for (int x = 0; x < width_; ++x) {
        int b = soft_ ? 96 + x * 64 / width_ : x * 255 / width_;
        int g = soft_ ? 96 + y * 64 / height_ : y * 255 / height_;
        const int chk = (((x + 2 * k_) / cw) % 2) ^ ((y / ch) % 2);
        int r = soft_ ? chk * 30 + 110 : (bench_ ? chk * 160 + 40 : (chk ? 200 : 40));
        if (bench_) {
          const uint32_t i = (uint32_t)((y * width_ + x) * 3);
          b += (int)(PcgHash(i + base) % 7u) - 3;
          g += (int)(PcgHash(i + 1 + base) % 7u) - 3;
          r += (int)(PcgHash(i + 2 + base) % 7u) - 3;
        }
        row[3 * x] = (uint8_t)std::min(255, std::max(0, b));
        row[3 * x + 1] = (uint8_t)std::min(255, std::max(0, g));
        row[3 * x + 2] = (uint8_t)std::min(255, std::max(0, r));
      }
    }
    fs->push_back(vf);
    if (flow_ || flow_writer_) {
      std::shared_ptr<DenseFlowFrame> ff(new DenseFlowFrame(flow_width_, flow_height_, true, vf->pts()));
      float* f = ff->mutable_flow();
      for (size_t i = 0; i < (size_t)flow_width_ * flow_height_; ++i) {
        f[2 * i] = -2.0f;
        f[2 * i + 1] = 0.0f;
      }
      if (flow_writer_ && k_ > 0) flow_writer_->AddFlowFrame(f);   // no field for frame 0
      if (flow_) fs->push_back(ff);
    }
    append->push_back(fs);
    ++k_;
    return true;
  }

 private:
  int width_, height_, frames_;
  bool flow_, bench_, soft_;
  std::string save_flow_;
  std::unique_ptr<DenseFlowWriter> flow_writer_;
  int original_width_, original_height_;
  int flow_width_, flow_height_;   // the frame size behind a downscale: the flow belongs to those frames
  int width_step_ = 0;
  int k_ = 0;
};

// Replaces the stream's desc by its vector-only form (RemoveRasterization): what a reader of a file
// written with remove_rasterization hands to the units behind it.
class RemoveRasterizationUnit : public VideoUnit {
 public:
  bool OpenStreams(StreamSet* set) override {
    seg_idx_ = FindStreamIdx("SegmentationStream", set);
    return seg_idx_ >= 0;
  }
  void ProcessFrame(FrameSetPtr input, std::list<FrameSetPtr>* output) override {
    const PointerFrame<SegmentationDesc>& frame = input->at(seg_idx_)->As<PointerFrame<SegmentationDesc>>();
    std::unique_ptr<SegmentationDesc> desc(new SegmentationDesc(frame.Ref()));
    VF_CHECK(HasVectorMesh(desc->wire), "--remove_rasterization needs a vectorization (--over_segment)");
    VF_CHECK(RemoveRasterization(&desc->wire), "malformed SegmentationDesc");
    input->at(seg_idx_).reset(new PointerFrame<SegmentationDesc>(std::move(desc), frame.pts()));
    output->push_back(input);
  }

 private:
  int seg_idx_ = -1;
};

// Consumes "SegmentationStream" like the reference's writer / renderer units do
// (segmentation_unit.cpp:376-379, 562-565).
class HashSinkUnit : public VideoUnit {
 public:
  bool OpenStreams(StreamSet* set) override {
    seg_idx_ = FindStreamIdx("SegmentationStream", set);
    if (seg_idx_ < 0) return false;
    const SegmentationStream& s = set->at(seg_idx_)->As<SegmentationStream>();
    width_ = s.frame_width();
    height_ = s.frame_height();
    return true;
  }
  void ProcessFrame(FrameSetPtr input, std::list<FrameSetPtr>* output) override {
    const SegmentationDesc& desc = input->at(seg_idx_)->As<PointerFrame<SegmentationDesc>>().Ref();
    std::vector<int32_t> ids;
    VF_CHECK(desc.ToIdImage(width_, height_, &ids), "malformed SegmentationDesc");
    for (int32_t v : ids) {
      for (int b = 0; b < 4; ++b) {
        hash_ ^= (uint32_t)((uint32_t)v >> (8 * b)) & 0xffu;
        hash_ *= 16777619u;
      }
    }
    if (frames_ == 0) {
      first_regions_ = desc.NumRegions();
      first_levels_ = desc.NumHierarchyLevels();
    }
    total_regions_ += desc.NumRegions();
    bytes_ += desc.wire.size();
    ++frames_;
    output->push_back(input);
  }
  uint32_t hash() const { return hash_; }
  int frames() const { return frames_; }
  int first_regions() const { return first_regions_; }
  int first_levels() const { return first_levels_; }
  long total_regions() const { return total_regions_; }
  size_t bytes() const { return bytes_; }

 private:
  int seg_idx_ = -1, width_ = 0, height_ = 0, frames_ = 0, first_regions_ = 0, first_levels_ = 0;
  long total_regions_ = 0;
  size_t bytes_ = 0;
  uint32_t hash_ = 2166136261u;
};

// Hashes the pixel bytes (3 * width per row, no padding) of every "RenderedRegionStream" frame.
class RenderHashSinkUnit : public VideoUnit {
 public:
  bool OpenStreams(StreamSet* set) override {
    idx_ = FindStreamIdx("RenderedRegionStream", set);
    return idx_ >= 0;
  }
  void ProcessFrame(FrameSetPtr input, std::list<FrameSetPtr>* output) override {
    const VideoFrame& f = input->at(idx_)->As<VideoFrame>();
    for (int y = 0; y < f.height(); ++y) {
      const uint8_t* row = f.data() + (size_t)y * f.width_step();
      for (int x = 0; x < f.width() * 3; ++x) {
        hash_ ^= row[x];
        hash_ *= 16777619u;
      }
    }
    ++frames_;
    output->push_back(input);
  }
  uint32_t hash() const { return hash_; }
  int frames() const { return frames_; }

 private:
  int idx_ = -1, frames_ = 0;
  uint32_t hash_ = 2166136261u;
};

// --level_regions: asks the renderer library for the regions of one hierarchy level of every
// "SegmentationStream" frame (vsg_render_level_regions) and hashes both lists' bytes, regions first.
class LevelRegionsSinkUnit : public VideoUnit {
 public:
  LevelRegionsSinkUnit(int level, int device) : level_(level), device_(device) {}
  ~LevelRegionsSinkUnit() override { vsg_render_destroy(render_); }
  bool OpenStreams(StreamSet* set) override {
    seg_idx_ = FindStreamIdx("SegmentationStream", set);
    if (seg_idx_ < 0) return false;
    const SegmentationStream& s = set->at(seg_idx_)->As<SegmentationStream>();
    vsg_render_options o;
    vsg_render_default_options(&o);
    o.has_video = 0;
    o.device = device_;
    if (vsg_render_create(&o, s.frame_width(), s.frame_height(), &render_) != VSG_OK) {
      render_ = nullptr;
      std::fprintf(stderr, "ERROR: could not create the HIP renderer: %s\n", vsg_render_last_error());
      return false;
    }
    return true;
  }
  void ProcessFrame(FrameSetPtr input, std::list<FrameSetPtr>* output) override {
    const SegmentationDesc& desc = input->at(seg_idx_)->As<PointerFrame<SegmentationDesc>>().Ref();
    const uint8_t* seg = reinterpret_cast<const uint8_t*>(desc.wire.data());
    size_t nr = 0, ni = 0;
    VF_CHECK(vsg_render_level_regions(render_, seg, desc.wire.size(), level_, nullptr, 0, &nr, nullptr, 0, &ni,
                                      VSG_MEM_HOST) == VSG_OK,
             vsg_render_last_error());
    regions_buf_.resize(nr);
    intervals_buf_.resize(4 * ni);
    VF_CHECK(vsg_render_level_regions(render_, seg, desc.wire.size(), level_, regions_buf_.data(), nr, &nr,
                                      intervals_buf_.data(), ni, &ni, VSG_MEM_HOST) == VSG_OK,
             vsg_render_last_error());
    Hash(regions_buf_.data(), nr * sizeof(vsg_render_level_region));
    Hash(intervals_buf_.data(), ni * 4 * sizeof(int32_t));
    regions_ += (long)nr;
    intervals_ += (long)ni;
    output->push_back(input);
  }
  uint32_t hash() const { return hash_; }
  long regions() const { return regions_; }
  long intervals() const { return intervals_; }

 private:
  void Hash(const void* p, size_t n) {
    const uint8_t* b = static_cast<const uint8_t*>(p);
    for (size_t k = 0; k < n; ++k) {
      hash_ ^= b[k];
      hash_ *= 16777619u;
    }
  }
  int level_, device_, seg_idx_ = -1;
  vsg_render* render_ = nullptr;
  std::vector<vsg_render_level_region> regions_buf_;
  std::vector<int32_t> intervals_buf_;
  long regions_ = 0, intervals_ = 0;
  uint32_t hash_ = 2166136261u;
};

// --level_components: the same for the connected components of a level's regions
// (vsg_render_level_components), components first.
class LevelComponentsSinkUnit : public VideoUnit {
 public:
  LevelComponentsSinkUnit(int level, bool n8, int device)
      : level_(level), connect_(n8 ? VSG_RENDER_CONNECT_N8 : VSG_RENDER_CONNECT_N4), device_(device) {}
  ~LevelComponentsSinkUnit() override { vsg_render_destroy(render_); }
  bool OpenStreams(StreamSet* set) override {
    seg_idx_ = FindStreamIdx("SegmentationStream", set);
    if (seg_idx_ < 0) return false;
    const SegmentationStream& s = set->at(seg_idx_)->As<SegmentationStream>();
    vsg_render_options o;
    vsg_render_default_options(&o);
    o.has_video = 0;
    o.device = device_;
    if (vsg_render_create(&o, s.frame_width(), s.frame_height(), &render_) != VSG_OK) {
      render_ = nullptr;
      std::fprintf(stderr, "ERROR: could not create the HIP renderer: %s\n", vsg_render_last_error());
      return false;
    }
    return true;
  }
  void ProcessFrame(FrameSetPtr input, std::list<FrameSetPtr>* output) override {
    const SegmentationDesc& desc = input->at(seg_idx_)->As<PointerFrame<SegmentationDesc>>().Ref();
    const uint8_t* seg = reinterpret_cast<const uint8_t*>(desc.wire.data());
    size_t nc = 0, ni = 0;
    VF_CHECK(vsg_render_level_components(render_, seg, desc.wire.size(), level_, connect_, nullptr, 0, &nc, nullptr,
                                         0, &ni, nullptr, VSG_MEM_HOST) == VSG_OK,
             vsg_render_last_error());
    components_buf_.resize(nc);
    intervals_buf_.resize(4 * ni);
    VF_CHECK(vsg_render_level_components(render_, seg, desc.wire.size(), level_, connect_, components_buf_.data(), nc,
                                         &nc, intervals_buf_.data(), ni, &ni, nullptr, VSG_MEM_HOST) == VSG_OK,
             vsg_render_last_error());
    Hash(components_buf_.data(), nc * sizeof(vsg_render_level_component));
    Hash(intervals_buf_.data(), ni * 4 * sizeof(int32_t));
    components_ += (long)nc;
    intervals_ += (long)ni;
    output->push_back(input);
  }
  uint32_t hash() const { return hash_; }
  long components() const { return components_; }
  long intervals() const { return intervals_; }

 private:
  void Hash(const void* p, size_t n) {
    const uint8_t* b = static_cast<const uint8_t*>(p);
    for (size_t k = 0; k < n; ++k) {
      hash_ ^= b[k];
      hash_ *= 16777619u;
    }
  }
  int level_, connect_, device_, seg_idx_ = -1;
  vsg_render* render_ = nullptr;
  std::vector<vsg_render_level_component> components_buf_;
  std::vector<int32_t> intervals_buf_;
  long components_ = 0, intervals_ = 0;
  uint32_t hash_ = 2166136261u;
};

// --level_boundaries: the same for the boundary point lists of a level's regions or of their connected
// components (vsg_render_level_boundaries), records first.
class LevelBoundariesSinkUnit : public VideoUnit {
 public:
  LevelBoundariesSinkUnit(int level, int connectedness, bool outer, int device)
      : level_(level), connect_(connectedness),
        which_(outer ? VSG_RENDER_BOUNDARY_OUTER : VSG_RENDER_BOUNDARY_INNER), device_(device) {}
  ~LevelBoundariesSinkUnit() override { vsg_render_destroy(render_); }
  bool OpenStreams(StreamSet* set) override {
    seg_idx_ = FindStreamIdx("SegmentationStream", set);
    if (seg_idx_ < 0) return false;
    const SegmentationStream& s = set->at(seg_idx_)->As<SegmentationStream>();
    vsg_render_options o;
    vsg_render_default_options(&o);
    o.has_video = 0;
    o.device = device_;
    if (vsg_render_create(&o, s.frame_width(), s.frame_height(), &render_) != VSG_OK) {
      render_ = nullptr;
      std::fprintf(stderr, "ERROR: could not create the HIP renderer: %s\n", vsg_render_last_error());
      return false;
    }
    return true;
  }
  void ProcessFrame(FrameSetPtr input, std::list<FrameSetPtr>* output) override {
    const SegmentationDesc& desc = input->at(seg_idx_)->As<PointerFrame<SegmentationDesc>>().Ref();
    const uint8_t* seg = reinterpret_cast<const uint8_t*>(desc.wire.data());
    size_t nb = 0, np = 0;
    VF_CHECK(vsg_render_level_boundaries(render_, seg, desc.wire.size(), level_, connect_, which_, nullptr, 0, &nb,
                                         nullptr, 0, &np, VSG_MEM_HOST) == VSG_OK,
             vsg_render_last_error());
    records_buf_.resize(nb);
    points_buf_.resize(2 * np);
    VF_CHECK(vsg_render_level_boundaries(render_, seg, desc.wire.size(), level_, connect_, which_, records_buf_.data(),
                                         nb, &nb, points_buf_.data(), np, &np, VSG_MEM_HOST) == VSG_OK,
             vsg_render_last_error());
    Hash(records_buf_.data(), nb * sizeof(vsg_render_level_boundary));
    Hash(points_buf_.data(), np * 2 * sizeof(int32_t));
    boundaries_ += (long)nb;
    points_ += (long)np;
    output->push_back(input);
  }
  uint32_t hash() const { return hash_; }
  long boundaries() const { return boundaries_; }
  long points() const { return points_; }

 private:
  void Hash(const void* p, size_t n) {
    const uint8_t* b = static_cast<const uint8_t*>(p);
    for (size_t k = 0; k < n; ++k) {
      hash_ ^= b[k];
      hash_ *= 16777619u;
    }
  }
  int level_, connect_, which_, device_, seg_idx_ = -1;
  vsg_render* render_ = nullptr;
  std::vector<vsg_render_level_boundary> records_buf_;
  std::vector<int32_t> points_buf_;
  long boundaries_ = 0, points_ = 0;
  uint32_t hash_ = 2166136261u;
};

// --level_contours: the same for the traced contours of a level's regions or of their connected components
// (vsg_render_level_contours), records first.
class LevelContoursSinkUnit : public VideoUnit {
 public:
  LevelContoursSinkUnit(int level, int connectedness, int device)
      : level_(level), connect_(connectedness), device_(device) {}
  ~LevelContoursSinkUnit() override { vsg_render_destroy(render_); }
  bool OpenStreams(StreamSet* set) override {
    seg_idx_ = FindStreamIdx("SegmentationStream", set);
    if (seg_idx_ < 0) return false;
    const SegmentationStream& s = set->at(seg_idx_)->As<SegmentationStream>();
    vsg_render_options o;
    vsg_render_default_options(&o);
    o.has_video = 0;
    o.device = device_;
    if (vsg_render_create(&o, s.frame_width(), s.frame_height(), &render_) != VSG_OK) {
      render_ = nullptr;
      std::fprintf(stderr, "ERROR: could not create the HIP renderer: %s\n", vsg_render_last_error());
      return false;
    }
    return true;
  }
  void ProcessFrame(FrameSetPtr input, std::list<FrameSetPtr>* output) override {
    const SegmentationDesc& desc = input->at(seg_idx_)->As<PointerFrame<SegmentationDesc>>().Ref();
    const uint8_t* seg = reinterpret_cast<const uint8_t*>(desc.wire.data());
    size_t nc = 0, nv = 0;
    VF_CHECK(vsg_render_level_contours(render_, seg, desc.wire.size(), level_, connect_, nullptr, 0, &nc, nullptr, 0,
                                       &nv, VSG_MEM_HOST) == VSG_OK,
             vsg_render_last_error());
    records_buf_.resize(nc);
    vertices_buf_.resize(2 * nv);
    if (nc) {
      VF_CHECK(vsg_render_level_contours(render_, seg, desc.wire.size(), level_, connect_, records_buf_.data(), nc,
                                         &nc, vertices_buf_.data(), nv, &nv, VSG_MEM_HOST) == VSG_OK,
               vsg_render_last_error());
    }
    Hash(records_buf_.data(), nc * sizeof(vsg_render_level_contour));
    Hash(vertices_buf_.data(), nv * 2 * sizeof(int32_t));
    contours_ += (long)nc;
    output->push_back(input);
  }
  uint32_t hash() const { return hash_; }
  long contours() const { return contours_; }

 private:
  void Hash(const void* p, size_t n) {
    const uint8_t* b = static_cast<const uint8_t*>(p);
    for (size_t k = 0; k < n; ++k) {
      hash_ ^= b[k];
      hash_ *= 16777619u;
    }
  }
  int level_, connect_, device_, seg_idx_ = -1;
  vsg_render* render_ = nullptr;
  std::vector<vsg_render_level_contour> records_buf_;
  std::vector<int32_t> vertices_buf_;
  long contours_ = 0;
  uint32_t hash_ = 2166136261u;
};

// --level_mesh: the same for the shared-segment mesh of a level's regions or of their connected components
// (vsg_render_level_mesh): segments, vertices, loops, refs.  max_error >= 0: vsg_render_level_mesh_simplified.
class LevelMeshSinkUnit : public VideoUnit {
 public:
  LevelMeshSinkUnit(int level, int connectedness, int device, float max_error, int min_segment_points)
      : level_(level), connect_(connectedness), device_(device), max_error_(max_error),
        min_segment_points_(min_segment_points) {}
  ~LevelMeshSinkUnit() override { vsg_render_destroy(render_); }
  bool OpenStreams(StreamSet* set) override {
    seg_idx_ = FindStreamIdx("SegmentationStream", set);
    if (seg_idx_ < 0) return false;
    const SegmentationStream& s = set->at(seg_idx_)->As<SegmentationStream>();
    vsg_render_options o;
    vsg_render_default_options(&o);
    o.has_video = 0;
    o.device = device_;
    if (vsg_render_create(&o, s.frame_width(), s.frame_height(), &render_) != VSG_OK) {
      render_ = nullptr;
      std::fprintf(stderr, "ERROR: could not create the HIP renderer: %s\n", vsg_render_last_error());
      return false;
    }
    return true;
  }
  void ProcessFrame(FrameSetPtr input, std::list<FrameSetPtr>* output) override {
    const SegmentationDesc& desc = input->at(seg_idx_)->As<PointerFrame<SegmentationDesc>>().Ref();
    const uint8_t* seg = reinterpret_cast<const uint8_t*>(desc.wire.data());
    size_t ns = 0, nv = 0, nl = 0, nr = 0;
    auto mesh = [&](vsg_render_mesh_segment* segments, int32_t* vertices, vsg_render_mesh_loop* loops, int32_t* refs) {
      if (max_error_ >= 0) {
        return vsg_render_level_mesh_simplified(render_, seg, desc.wire.size(), level_, connect_, max_error_,
                                                min_segment_points_, segments, ns, &ns, vertices, nv, &nv, loops, nl,
                                                &nl, refs, nr, &nr, VSG_MEM_HOST);
      }
      return vsg_render_level_mesh(render_, seg, desc.wire.size(), level_, connect_, segments, ns, &ns, vertices, nv, &nv,
                                   loops, nl, &nl, refs, nr, &nr, VSG_MEM_HOST);
    };
    VF_CHECK(mesh(nullptr, nullptr, nullptr, nullptr) == VSG_OK, vsg_render_last_error());
    segments_buf_.resize(ns);
    vertices_buf_.resize(2 * nv);
    loops_buf_.resize(nl);
    refs_buf_.resize(nr);
    if (ns) {
      VF_CHECK(mesh(segments_buf_.data(), vertices_buf_.data(), loops_buf_.data(), refs_buf_.data()) == VSG_OK,
               vsg_render_last_error());
    }
    Hash(segments_buf_.data(), ns * sizeof(vsg_render_mesh_segment));
    Hash(vertices_buf_.data(), nv * 2 * sizeof(int32_t));
    Hash(loops_buf_.data(), nl * sizeof(vsg_render_mesh_loop));
    Hash(refs_buf_.data(), nr * sizeof(int32_t));
    segments_ += (long)ns;
    output->push_back(input);
  }
  uint32_t hash() const { return hash_; }
  long segments() const { return segments_; }

 private:
  void Hash(const void* p, size_t n) {
    const uint8_t* b = static_cast<const uint8_t*>(p);
    for (size_t k = 0; k < n; ++k) {
      hash_ ^= b[k];
      hash_ *= 16777619u;
    }
  }
  int level_, connect_, device_, seg_idx_ = -1;
  float max_error_;
  int min_segment_points_;
  vsg_render* render_ = nullptr;
  std::vector<vsg_render_mesh_segment> segments_buf_;
  std::vector<int32_t> vertices_buf_;
  std::vector<vsg_render_mesh_loop> loops_buf_;
  std::vector<int32_t> refs_buf_;
  long segments_ = 0;
  uint32_t hash_ = 2166136261u;
};

// --level_adjacency: the same for the adjacency graph of a level's regions or of their connected
// components (vsg_render_level_adjacency), nodes first.
class LevelAdjacencySinkUnit : public VideoUnit {
 public:
  LevelAdjacencySinkUnit(int level, int connectedness, bool n8, int device)
      : level_(level), connect_(connectedness),
        neighbourhood_(n8 ? VSG_RENDER_ADJACENT_N8 : VSG_RENDER_ADJACENT_N4), device_(device) {}
  ~LevelAdjacencySinkUnit() override { vsg_render_destroy(render_); }
  bool OpenStreams(StreamSet* set) override {
    seg_idx_ = FindStreamIdx("SegmentationStream", set);
    if (seg_idx_ < 0) return false;
    const SegmentationStream& s = set->at(seg_idx_)->As<SegmentationStream>();
    vsg_render_options o;
    vsg_render_default_options(&o);
    o.has_video = 0;
    o.device = device_;
    if (vsg_render_create(&o, s.frame_width(), s.frame_height(), &render_) != VSG_OK) {
      render_ = nullptr;
      std::fprintf(stderr, "ERROR: could not create the HIP renderer: %s\n", vsg_render_last_error());
      return false;
    }
    return true;
  }
  void ProcessFrame(FrameSetPtr input, std::list<FrameSetPtr>* output) override {
    const SegmentationDesc& desc = input->at(seg_idx_)->As<PointerFrame<SegmentationDesc>>().Ref();
    const uint8_t* seg = reinterpret_cast<const uint8_t*>(desc.wire.data());
    size_t nn = 0, ne = 0;
    VF_CHECK(vsg_render_level_adjacency(render_, seg, desc.wire.size(), level_, connect_, neighbourhood_, nullptr, 0,
                                        &nn, nullptr, 0, &ne, VSG_MEM_HOST) == VSG_OK,
             vsg_render_last_error());
    nodes_buf_.resize(nn);
    edges_buf_.resize(ne);
    if (nn) {
      VF_CHECK(vsg_render_level_adjacency(render_, seg, desc.wire.size(), level_, connect_, neighbourhood_,
                                          nodes_buf_.data(), nn, &nn, edges_buf_.data(), ne, &ne,
                                          VSG_MEM_HOST) == VSG_OK,
               vsg_render_last_error());
    }
    Hash(nodes_buf_.data(), nn * sizeof(vsg_render_level_node));
    Hash(edges_buf_.data(), ne * sizeof(vsg_render_level_edge));
    nodes_ += (long)nn;
    edges_ += (long)ne;
    output->push_back(input);
  }
  uint32_t hash() const { return hash_; }
  long nodes() const { return nodes_; }
  long edges() const { return edges_; }

 private:
  void Hash(const void* p, size_t n) {
    const uint8_t* b = static_cast<const uint8_t*>(p);
    for (size_t k = 0; k < n; ++k) {
      hash_ ^= b[k];
      hash_ *= 16777619u;
    }
  }
  int level_, connect_, neighbourhood_, device_, seg_idx_ = -1;
  vsg_render* render_ = nullptr;
  std::vector<vsg_render_level_node> nodes_buf_;
  std::vector<vsg_render_level_edge> edges_buf_;
  long nodes_ = 0, edges_ = 0;
  uint32_t hash_ = 2166136261u;
};

// --persistence: the boundary persistence of every frame's hierarchy: the plane of
// vsg_render_persistence_image, then the edges' persistences and the levels' sides of
// vsg_render_persistence_graph.
class PersistenceSinkUnit : public VideoUnit {
 public:
  PersistenceSinkUnit(bool n8, int device)
      : neighbourhood_(n8 ? VSG_RENDER_ADJACENT_N8 : VSG_RENDER_ADJACENT_N4), device_(device) {}
  ~PersistenceSinkUnit() override { vsg_render_destroy(render_); }
  bool OpenStreams(StreamSet* set) override {
    seg_idx_ = FindStreamIdx("SegmentationStream", set);
    if (seg_idx_ < 0) return false;
    const SegmentationStream& s = set->at(seg_idx_)->As<SegmentationStream>();
    vsg_render_options o;
    vsg_render_default_options(&o);
    o.has_video = 0;
    o.device = device_;
    if (vsg_render_create(&o, s.frame_width(), s.frame_height(), &render_) != VSG_OK) {
      render_ = nullptr;
      std::fprintf(stderr, "ERROR: could not create the HIP renderer: %s\n", vsg_render_last_error());
      return false;
    }
    plane_.resize((size_t)s.frame_width() * s.frame_height());
    return true;
  }
  void ProcessFrame(FrameSetPtr input, std::list<FrameSetPtr>* output) override {
    const SegmentationDesc& desc = input->at(seg_idx_)->As<PointerFrame<SegmentationDesc>>().Ref();
    const uint8_t* seg = reinterpret_cast<const uint8_t*>(desc.wire.data());
    VF_CHECK(vsg_render_persistence_image(render_, seg, desc.wire.size(), plane_.data(), &levels_, VSG_MEM_HOST) ==
                 VSG_OK,
             vsg_render_last_error());
    vsg_render_persistence_stats st;
    VF_CHECK(vsg_render_last_persistence_stats(render_, &st) == VSG_OK, vsg_render_last_error());
    edge_pixels_ += (long)st.edge_pixels;
    size_t nn = 0, ne = 0, nl = 0;
    VF_CHECK(vsg_render_persistence_graph(render_, seg, desc.wire.size(), neighbourhood_, nullptr, 0, &nn, nullptr, 0,
                                          &ne, nullptr, nullptr, 0, &nl, VSG_MEM_HOST) == VSG_OK,
             vsg_render_last_error());
    nodes_buf_.resize(std::max<size_t>(nn, 1));
    edges_buf_.resize(std::max<size_t>(ne, 1));
    persistence_.resize(std::max<size_t>(ne, 1));
    sides_.resize(nl);
    VF_CHECK(vsg_render_persistence_graph(render_, seg, desc.wire.size(), neighbourhood_, nodes_buf_.data(), nn, &nn,
                                          edges_buf_.data(), ne, &ne, persistence_.data(), sides_.data(), nl, &nl,
                                          VSG_MEM_HOST) == VSG_OK,
             vsg_render_last_error());
    Hash(plane_.data(), plane_.size() * sizeof(int32_t));
    Hash(persistence_.data(), ne * sizeof(int32_t));
    Hash(sides_.data(), nl * sizeof(int64_t));
    edges_ += (long)ne;
    output->push_back(input);
  }
  uint32_t hash() const { return hash_; }
  int levels() const { return levels_; }
  long edge_pixels() const { return edge_pixels_; }
  long edges() const { return edges_; }

 private:
  void Hash(const void* p, size_t n) {
    const uint8_t* b = static_cast<const uint8_t*>(p);
    for (size_t k = 0; k < n; ++k) {
      hash_ ^= b[k];
      hash_ *= 16777619u;
    }
  }
  int neighbourhood_, device_, seg_idx_ = -1, levels_ = 0;
  vsg_render* render_ = nullptr;
  std::vector<int32_t> plane_, persistence_;
  std::vector<int64_t> sides_;
  std::vector<vsg_render_level_node> nodes_buf_;
  std::vector<vsg_render_level_edge> edges_buf_;
  long edge_pixels_ = 0, edges_ = 0;
  uint32_t hash_ = 2166136261u;
};

// --level_overlap: the same for the overlap table of a level's regions, or of their connected components,
// with the previous frame's id image at that level (vsg_render_level_overlap): rows, cols, pairs of every
// frame after the first.
class LevelOverlapSinkUnit : public VideoUnit {
 public:
  LevelOverlapSinkUnit(int level, int connectedness, int device)
      : level_(level), connect_(connectedness), device_(device) {}
  ~LevelOverlapSinkUnit() override { vsg_render_destroy(render_); }
  bool OpenStreams(StreamSet* set) override {
    seg_idx_ = FindStreamIdx("SegmentationStream", set);
    if (seg_idx_ < 0) return false;
    const SegmentationStream& s = set->at(seg_idx_)->As<SegmentationStream>();
    vsg_render_options o;
    vsg_render_default_options(&o);
    o.has_video = 0;
    o.device = device_;
    if (vsg_render_create(&o, s.frame_width(), s.frame_height(), &render_) != VSG_OK) {
      render_ = nullptr;
      std::fprintf(stderr, "ERROR: could not create the HIP renderer: %s\n", vsg_render_last_error());
      return false;
    }
    previous_.resize((size_t)s.frame_width() * s.frame_height());
    return true;
  }
  void ProcessFrame(FrameSetPtr input, std::list<FrameSetPtr>* output) override {
    const SegmentationDesc& desc = input->at(seg_idx_)->As<PointerFrame<SegmentationDesc>>().Ref();
    const uint8_t* seg = reinterpret_cast<const uint8_t*>(desc.wire.data());
    if (have_previous_) {
      size_t nr = 0, nc = 0, np = 0;
      VF_CHECK(vsg_render_level_overlap(render_, seg, desc.wire.size(), level_, connect_, previous_.data(), 0,
                                        VSG_MEM_HOST, nullptr, 0, &nr, nullptr, 0, &nc, nullptr, 0, &np,
                                        VSG_MEM_HOST) == VSG_OK,
               vsg_render_last_error());
      rows_buf_.resize(nr);
      cols_buf_.resize(nc);
      pairs_buf_.resize(np);
      if (nr || nc) {
        VF_CHECK(vsg_render_level_overlap(render_, seg, desc.wire.size(), level_, connect_, previous_.data(), 0,
                                          VSG_MEM_HOST, rows_buf_.data(), nr, &nr, cols_buf_.data(), nc, &nc,
                                          pairs_buf_.data(), np, &np, VSG_MEM_HOST) == VSG_OK,
                 vsg_render_last_error());
      }
      Hash(rows_buf_.data(), nr * sizeof(vsg_render_overlap_row));
      Hash(cols_buf_.data(), nc * sizeof(vsg_render_overlap_col));
      Hash(pairs_buf_.data(), np * sizeof(vsg_render_overlap_pair));
      rows_ += (long)nr;
      cols_ += (long)nc;
      pairs_ += (long)np;
    }
    VF_CHECK(vsg_render_id_image(render_, seg, desc.wire.size(), level_, previous_.data(), VSG_MEM_HOST) == VSG_OK,
             vsg_render_last_error());
    have_previous_ = true;
    output->push_back(input);
  }
  uint32_t hash() const { return hash_; }
  long rows() const { return rows_; }
  long cols() const { return cols_; }
  long pairs() const { return pairs_; }

 private:
  void Hash(const void* p, size_t n) {
    const uint8_t* b = static_cast<const uint8_t*>(p);
    for (size_t k = 0; k < n; ++k) {
      hash_ ^= b[k];
      hash_ *= 16777619u;
    }
  }
  int level_, connect_, device_, seg_idx_ = -1;
  vsg_render* render_ = nullptr;
  bool have_previous_ = false;
  std::vector<int32_t> previous_;
  std::vector<vsg_render_overlap_row> rows_buf_;
  std::vector<vsg_render_overlap_col> cols_buf_;
  std::vector<vsg_render_overlap_pair> pairs_buf_;
  long rows_ = 0, cols_ = 0, pairs_ = 0;
  uint32_t hash_ = 2166136261u;
};

// --tree_cut: the best non-horizontal cut of every frame's hierarchy after the first against the previous
// frame's level-0 id image (vsg_render_tree_cut with labels): the records, then the plane.
class TreeCutSinkUnit : public VideoUnit {
 public:
  TreeCutSinkUnit(int64_t penalty, int device) : penalty_(penalty), device_(device) {}
  ~TreeCutSinkUnit() override { vsg_render_destroy(render_); }
  bool OpenStreams(StreamSet* set) override {
    seg_idx_ = FindStreamIdx("SegmentationStream", set);
    if (seg_idx_ < 0) return false;
    const SegmentationStream& s = set->at(seg_idx_)->As<SegmentationStream>();
    vsg_render_options o;
    vsg_render_default_options(&o);
    o.has_video = 0;
    o.device = device_;
    if (vsg_render_create(&o, s.frame_width(), s.frame_height(), &render_) != VSG_OK) {
      render_ = nullptr;
      std::fprintf(stderr, "ERROR: could not create the HIP renderer: %s\n", vsg_render_last_error());
      return false;
    }
    previous_.resize((size_t)s.frame_width() * s.frame_height());
    plane_.resize(previous_.size());
    return true;
  }
  void ProcessFrame(FrameSetPtr input, std::list<FrameSetPtr>* output) override {
    const SegmentationDesc& desc = input->at(seg_idx_)->As<PointerFrame<SegmentationDesc>>().Ref();
    const uint8_t* seg = reinterpret_cast<const uint8_t*>(desc.wire.data());
    if (have_previous_) {
      size_t n = 0;
      int64_t total = 0;
      VF_CHECK(vsg_render_tree_cut(render_, seg, desc.wire.size(), previous_.data(), 0, VSG_MEM_HOST, penalty_,
                                   nullptr, 0, VSG_MEM_HOST, nullptr, 0, &n, nullptr, &total, VSG_MEM_HOST) == VSG_OK,
               vsg_render_last_error());
      nodes_buf_.resize(std::max<size_t>(n, 1));
      VF_CHECK(vsg_render_tree_cut(render_, seg, desc.wire.size(), previous_.data(), 0, VSG_MEM_HOST, penalty_,
                                   nullptr, 0, VSG_MEM_HOST, nodes_buf_.data(), n, &n, plane_.data(), &total,
                                   VSG_MEM_HOST) == VSG_OK,
               vsg_render_last_error());
      Hash(nodes_buf_.data(), n * sizeof(vsg_render_cut_node));
      Hash(plane_.data(), plane_.size() * sizeof(int32_t));
      nodes_ += (long)n;
      total_ += (long long)total;
    }
    VF_CHECK(vsg_render_id_image(render_, seg, desc.wire.size(), 0, previous_.data(), VSG_MEM_HOST) == VSG_OK,
             vsg_render_last_error());
    have_previous_ = true;
    output->push_back(input);
  }
  uint32_t hash() const { return hash_; }
  long nodes() const { return nodes_; }
  long long total() const { return total_; }

 private:
  void Hash(const void* p, size_t n) {
    const uint8_t* b = static_cast<const uint8_t*>(p);
    for (size_t k = 0; k < n; ++k) {
      hash_ ^= b[k];
      hash_ *= 16777619u;
    }
  }
  int64_t penalty_;
  int device_, seg_idx_ = -1;
  vsg_render* render_ = nullptr;
  bool have_previous_ = false;
  std::vector<int32_t> previous_, plane_;
  std::vector<vsg_render_cut_node> nodes_buf_;
  long nodes_ = 0;
  long long total_ = 0;
  uint32_t hash_ = 2166136261u;
};

// --boundary_distance and --boundary_benchmark: the squared distance to a level's edges of every frame
// (vsg_render_boundary_distance), and the boundary records of all levels of every frame after the first
// against the previous frame's level-0 id image (vsg_render_boundary_benchmark).  level < 0 or
// tolerance_sq < 0: that half is off.
class BoundaryDistanceSinkUnit : public VideoUnit {
 public:
  BoundaryDistanceSinkUnit(int level, int tolerance_sq, int device)
      : level_(level), tolerance_sq_(tolerance_sq), device_(device) {}
  ~BoundaryDistanceSinkUnit() override { vsg_render_destroy(render_); }
  bool OpenStreams(StreamSet* set) override {
    seg_idx_ = FindStreamIdx("SegmentationStream", set);
    if (seg_idx_ < 0) return false;
    const SegmentationStream& s = set->at(seg_idx_)->As<SegmentationStream>();
    vsg_render_options o;
    vsg_render_default_options(&o);
    o.has_video = 0;
    o.device = device_;
    if (vsg_render_create(&o, s.frame_width(), s.frame_height(), &render_) != VSG_OK) {
      render_ = nullptr;
      std::fprintf(stderr, "ERROR: could not create the HIP renderer: %s\n", vsg_render_last_error());
      return false;
    }
    plane_.resize((size_t)s.frame_width() * s.frame_height());
    previous_.resize(plane_.size());
    return true;
  }
  void ProcessFrame(FrameSetPtr input, std::list<FrameSetPtr>* output) override {
    const SegmentationDesc& desc = input->at(seg_idx_)->As<PointerFrame<SegmentationDesc>>().Ref();
    const uint8_t* seg = reinterpret_cast<const uint8_t*>(desc.wire.data());
    if (level_ >= 0) {
      VF_CHECK(vsg_render_boundary_distance(render_, seg, desc.wire.size(), level_, plane_.data(), VSG_MEM_HOST) ==
                   VSG_OK,
               vsg_render_last_error());
      vsg_render_distance_stats st;
      VF_CHECK(vsg_render_last_distance_stats(render_, &st) == VSG_OK, vsg_render_last_error());
      edge_pixels_ += (long)st.edge_pixels;
      max_distance_ = std::max(max_distance_, (long)st.max_distance);
      Hash(&distance_hash_, plane_.data(), plane_.size() * sizeof(int32_t));
    }
    if (tolerance_sq_ >= 0) {
      if (have_previous_) {
        // one call while the records fit: a call whose capacity is too small has done most of its work
        // already, and says how many levels there are
        size_t nl = 0;
        if (scores_.size() < 32) scores_.resize(32);
        int rc = vsg_render_boundary_benchmark(render_, seg, desc.wire.size(), previous_.data(), 0, VSG_MEM_HOST,
                                               tolerance_sq_, scores_.data(), scores_.size(), &nl, VSG_MEM_HOST);
        if (rc != VSG_OK && nl > scores_.size()) {
          scores_.resize(nl);
          rc = vsg_render_boundary_benchmark(render_, seg, desc.wire.size(), previous_.data(), 0, VSG_MEM_HOST,
                                             tolerance_sq_, scores_.data(), scores_.size(), &nl, VSG_MEM_HOST);
        }
        VF_CHECK(rc == VSG_OK, vsg_render_last_error());
        for (size_t l = 0; l < nl; ++l) {
          sums_[0] += (long)scores_[l].seg_edges;
          sums_[1] += (long)scores_[l].seg_matched;
          sums_[2] += (long)scores_[l].gt_edges;
          sums_[3] += (long)scores_[l].gt_matched;
        }
        levels_ = (int)nl;
        Hash(&benchmark_hash_, scores_.data(), nl * sizeof(vsg_render_boundary_score));
      }
      VF_CHECK(vsg_render_id_image(render_, seg, desc.wire.size(), 0, previous_.data(), VSG_MEM_HOST) == VSG_OK,
               vsg_render_last_error());
      have_previous_ = true;
    }
    output->push_back(input);
  }
  int level() const { return level_; }
  int tolerance_sq() const { return tolerance_sq_; }
  int levels() const { return levels_; }
  long edge_pixels() const { return edge_pixels_; }
  long max_distance() const { return max_distance_; }
  const long* sums() const { return sums_; }
  uint32_t distance_hash() const { return distance_hash_; }
  uint32_t benchmark_hash() const { return benchmark_hash_; }

 private:
  static void Hash(uint32_t* hash, const void* p, size_t n) {
    const uint8_t* b = static_cast<const uint8_t*>(p);
    for (size_t k = 0; k < n; ++k) {
      *hash ^= b[k];
      *hash *= 16777619u;
    }
  }
  int level_, tolerance_sq_, device_, seg_idx_ = -1, levels_ = 0;
  vsg_render* render_ = nullptr;
  bool have_previous_ = false;
  std::vector<int32_t> plane_, previous_;
  std::vector<vsg_render_boundary_score> scores_;
  long edge_pixels_ = 0, max_distance_ = 0, sums_[4] = {0, 0, 0, 0};
  uint32_t distance_hash_ = 2166136261u, benchmark_hash_ = 2166136261u;
};

// --level_colors: the colour table of a level's regions, or of their connected components, in the video's
// frame (vsg_render_level_colors) and the level painted in mean colours (vsg_render_mean_frame): the
// records, then the 3 * width pixel bytes of every picture row, of every frame.
class LevelColorsSinkUnit : public VideoUnit {
 public:
  LevelColorsSinkUnit(int level, int connectedness, int device)
      : level_(level), connect_(connectedness), device_(device) {}
  ~LevelColorsSinkUnit() override { vsg_render_destroy(render_); }
  bool OpenStreams(StreamSet* set) override {
    seg_idx_ = FindStreamIdx("SegmentationStream", set);
    vid_idx_ = FindStreamIdx("VideoStream", set);
    if (seg_idx_ < 0 || vid_idx_ < 0) return false;
    const VideoStream& v = set->at(vid_idx_)->As<VideoStream>();
    if (v.pixel_format() != PIXEL_FORMAT_BGR24) {
      std::fprintf(stderr, "ERROR: --level_colors needs a BGR24 video stream\n");
      return false;
    }
    width_ = v.frame_width();
    height_ = v.frame_height();
    vsg_render_options o;
    vsg_render_default_options(&o);
    o.device = device_;
    if (vsg_render_create(&o, width_, height_, &render_) != VSG_OK) {
      render_ = nullptr;
      std::fprintf(stderr, "ERROR: could not create the HIP renderer: %s\n", vsg_render_last_error());
      return false;
    }
    stride_ = vsg_render_default_stride(width_);
    picture_.resize(stride_ * height_);
    return true;
  }
  void ProcessFrame(FrameSetPtr input, std::list<FrameSetPtr>* output) override {
    const SegmentationDesc& desc = input->at(seg_idx_)->As<PointerFrame<SegmentationDesc>>().Ref();
    const uint8_t* seg = reinterpret_cast<const uint8_t*>(desc.wire.data());
    VF_CHECK(input->at(vid_idx_) != nullptr, "the video frame was freed before the colour sink");
    const VideoFrame& frame = input->at(vid_idx_)->As<VideoFrame>();
    size_t n = 0;
    VF_CHECK(vsg_render_level_colors(render_, seg, desc.wire.size(), level_, connect_, frame.data(),
                                     (size_t)frame.width_step(), VSG_MEM_HOST, nullptr, 0, &n, VSG_MEM_HOST) == VSG_OK,
             vsg_render_last_error());
    colors_buf_.resize(n);
    if (n) {
      VF_CHECK(vsg_render_level_colors(render_, seg, desc.wire.size(), level_, connect_, frame.data(),
                                       (size_t)frame.width_step(), VSG_MEM_HOST, colors_buf_.data(), n, &n,
                                       VSG_MEM_HOST) == VSG_OK,
               vsg_render_last_error());
    }
    Hash(colors_buf_.data(), n * sizeof(vsg_render_level_color));
    groups_ += (long)n;
    VF_CHECK(vsg_render_mean_frame(render_, seg, desc.wire.size(), level_, connect_, frame.data(),
                                   (size_t)frame.width_step(), VSG_MEM_HOST, picture_.data(), stride_,
                                   VSG_MEM_HOST) == VSG_OK,
             vsg_render_last_error());
    for (int y = 0; y < height_; ++y) Hash(picture_.data() + (size_t)y * stride_, (size_t)width_ * 3);
    output->push_back(input);
  }
  uint32_t hash() const { return hash_; }
  long groups() const { return groups_; }

 private:
  void Hash(const void* p, size_t n) {
    const uint8_t* b = static_cast<const uint8_t*>(p);
    for (size_t k = 0; k < n; ++k) {
      hash_ ^= b[k];
      hash_ *= 16777619u;
    }
  }
  int level_, connect_, device_, seg_idx_ = -1, vid_idx_ = -1, width_ = 0, height_ = 0;
  size_t stride_ = 0;
  vsg_render* render_ = nullptr;
  std::vector<vsg_render_level_color> colors_buf_;
  std::vector<uint8_t> picture_;
  long groups_ = 0;
  uint32_t hash_ = 2166136261u;
};

// --level_pool: a planar f32 feature map of five channels, the frame's B, G, R, then x and y, pooled by a level's
// regions or by their connected components (vsg_render_level_pool): the groups and the four matrices of every
// frame are hashed, the sums of every channel over all groups added up.
class LevelPoolSinkUnit : public VideoUnit {
 public:
  static constexpr int kChannels = 5;
  LevelPoolSinkUnit(int level, int connectedness, int device)
      : level_(level), connect_(connectedness), device_(device) {}
  ~LevelPoolSinkUnit() override { vsg_render_destroy(render_); }
  bool OpenStreams(StreamSet* set) override {
    seg_idx_ = FindStreamIdx("SegmentationStream", set);
    vid_idx_ = FindStreamIdx("VideoStream", set);
    if (seg_idx_ < 0 || vid_idx_ < 0) return false;
    const VideoStream& v = set->at(vid_idx_)->As<VideoStream>();
    if (v.pixel_format() != PIXEL_FORMAT_BGR24) {
      std::fprintf(stderr, "ERROR: --level_pool needs a BGR24 video stream\n");
      return false;
    }
    width_ = v.frame_width();
    height_ = v.frame_height();
    vsg_render_options o;
    vsg_render_default_options(&o);
    o.device = device_;
    if (vsg_render_create(&o, width_, height_, &render_) != VSG_OK) {
      render_ = nullptr;
      std::fprintf(stderr, "ERROR: could not create the HIP renderer: %s\n", vsg_render_last_error());
      return false;
    }
    features_.resize((size_t)kChannels * width_ * height_);
    return true;
  }
  void ProcessFrame(FrameSetPtr input, std::list<FrameSetPtr>* output) override {
    const SegmentationDesc& desc = input->at(seg_idx_)->As<PointerFrame<SegmentationDesc>>().Ref();
    const uint8_t* seg = reinterpret_cast<const uint8_t*>(desc.wire.data());
    VF_CHECK(input->at(vid_idx_) != nullptr, "the video frame was freed before the pool sink");
    const VideoFrame& frame = input->at(vid_idx_)->As<VideoFrame>();
    const size_t plane = (size_t)width_ * height_;
    for (int y = 0; y < height_; ++y) {
      const uint8_t* row = frame.data() + (size_t)y * frame.width_step();
      for (int x = 0; x < width_; ++x) {
        const size_t at = (size_t)y * width_ + x;
        for (int c = 0; c < 3; ++c) features_[c * plane + at] = (float)row[3 * x + c];
        features_[3 * plane + at] = (float)x;
        features_[4 * plane + at] = (float)y;
      }
    }
    auto pool = [&](vsg_render_pool_group* g, double* s, double* q, float* lo, float* hi, size_t cap, size_t* n) {
      VF_CHECK(vsg_render_level_pool(render_, seg, desc.wire.size(), level_, connect_, features_.data(), VSG_POOL_F32,
                                     kChannels, (ptrdiff_t)plane, (ptrdiff_t)width_, 1, VSG_MEM_HOST, g, s, q, lo, hi,
                                     cap, n, VSG_MEM_HOST) == VSG_OK,
               vsg_render_last_error());
    };
    size_t n = 0;
    pool(nullptr, nullptr, nullptr, nullptr, nullptr, 0, &n);
    groups_buf_.resize(n);
    sum_.resize(n * kChannels);
    sum_sq_.resize(n * kChannels);
    min_.resize(n * kChannels);
    max_.resize(n * kChannels);
    if (n) pool(groups_buf_.data(), sum_.data(), sum_sq_.data(), min_.data(), max_.data(), n, &n);
    Hash(groups_buf_.data(), n * sizeof(vsg_render_pool_group));
    Hash(sum_.data(), n * kChannels * sizeof(double));
    Hash(sum_sq_.data(), n * kChannels * sizeof(double));
    Hash(min_.data(), n * kChannels * sizeof(float));
    Hash(max_.data(), n * kChannels * sizeof(float));
    for (size_t k = 0; k < n; ++k) {
      for (int c = 0; c < kChannels; ++c) totals_[c] += sum_[k * kChannels + c];   // integers: exact
    }
    groups_ += (long)n;
    output->push_back(input);
  }
  uint32_t hash() const { return hash_; }
  long groups() const { return groups_; }
  const double* totals() const { return totals_; }

 private:
  void Hash(const void* p, size_t n) {
    const uint8_t* b = static_cast<const uint8_t*>(p);
    for (size_t k = 0; k < n; ++k) {
      hash_ ^= b[k];
      hash_ *= 16777619u;
    }
  }
  int level_, connect_, device_, seg_idx_ = -1, vid_idx_ = -1, width_ = 0, height_ = 0;
  vsg_render* render_ = nullptr;
  std::vector<float> features_, min_, max_;
  std::vector<double> sum_, sum_sq_;
  std::vector<vsg_render_pool_group> groups_buf_;
  double totals_[kChannels] = {0, 0, 0, 0, 0};
  long groups_ = 0;
  uint32_t hash_ = 2166136261u;
};

}  // namespace

// --read_pb FILE: reads a segmentation container back with SegmentationReader and prints what the
// sink prints for a live run (frames, regions, label hash), without touching the GPU.
int ReadBack(const std::string& file) {
  SegmentationReader reader(file);
  if (!reader.OpenFileAndReadHeaders()) return 1;
  int width = 0, height = 0;
  if (reader.NumFrames() > 0 && !reader.SegmentationResolution(&width, &height)) return 1;
  uint32_t hash = 2166136261u;
  long total_regions = 0;
  int first_regions = 0;
  size_t bytes = 0;
  std::vector<int32_t> ids;
  for (int k = 0; reader.RemainingFrames() > 0; ++k) {
    SegmentationDesc desc;
    if (!reader.ReadNextFrame(&desc) || !desc.ToIdImage(width, height, &ids)) return 1;
    for (int32_t v : ids) {
      for (int b = 0; b < 4; ++b) {
        hash ^= (uint32_t)((uint32_t)v >> (8 * b)) & 0xffu;
        hash *= 16777619u;
      }
    }
    if (k == 0) first_regions = desc.NumRegions();
    total_regions += desc.NumRegions();
    bytes += desc.wire.size();
  }
  std::printf("frames=%d first_frame_regions=%d total_regions=%ld label_fnv1a32=%08x bytes=%zu "
              "width=%d height=%d header_flags=%zu last_pts=%lld\n",
              reader.NumFrames(), first_regions, total_regions, hash, bytes, width, height,
              reader.GetHeaderFlags().size(),
              reader.NumFrames() ? (long long)reader.TimeStamps().back() : 0ll);
  return 0;
}

// --rewrite_pb FILE --output_file OUT [--remove_rasterization] [--original_width W --original_height H]:
// every desc of FILE through the writer unit's edit (PrepareDescForWriting) into OUT.  No GPU.
int Rewrite(const std::string& file, const std::string& out_file, bool remove_rasterization, int original_width,
            int original_height) {
  SegmentationReader reader(file);
  if (!reader.OpenFileAndReadHeaders() || out_file.empty()) return 1;
  SegmentationWriterUnitOptions wo;
  wo.filename = out_file;
  wo.remove_rasterization = remove_rasterization;
  SegmentationWriter writer(out_file);
  if (!writer.OpenFile(std::vector<int>{1, 0})) return 1;
  for (int k = 0; reader.RemainingFrames() > 0; ++k) {
    SegmentationDesc desc;
    if (!reader.ReadNextFrame(&desc)) return 1;
    if (!PrepareDescForWriting(wo, original_width, original_height, &desc.wire)) return 1;
    writer.AddSegmentationDataToChunk(desc.wire, reader.TimeStamps()[k]);
  }
  writer.WriteTermHeaderAndClose();
  return 0;
}

// Flags: the reference's names where it has them (seg_tree.cpp:52-72, dense_segmentation.cpp:39-46),
// gflags syntax (--flag=value, --flag value, --flag / --noflag for booleans).
struct Flags {
  // seg_tree_sample
  bool flow = true;
  std::string input_file;
  bool use_pipeline = true;
  bool over_segment = false;       // as in the reference: also turns the vectorization on (this
                                   // driver always stops after the dense over-segmentation)
  bool write_to_file = false;      // writes <input_file>.pb (or --output_file)
  bool save_flow = false;          // writes <input base>.flow from the synthetic source
  bool compute_flow = false;       // opt-in: with --flow and no .flow file, LuminanceUnit -> DenseFlowUnit
                                   // compute the flow (seg_tree.cpp:170-187) instead of the source
  // dense_segmentation.cpp
  std::string dense_smoothing = "bilateral";   // none | bilateral
  std::string dense_color_dist = "l2";         // l1 | l2
  double dense_min_region_size = 0.01;         // frac_min_region_size
  // this driver only
  int width = 64, height = 48, frames = 45, chunk_size = 20, device = -1;
  std::string input = "probe";     // synthetic generator: probe | bench | soft
  // seg_tree.cpp:219-241 runs the RegionSegmentationUnit unless --over_segment is given; here it is
  // opt-in, so that the over-segmentation hashes of the default run stay what the pins say
  bool region_segmentation = false;
  int chunk_set_size = 6, chunk_set_overlap = 2, min_region_num = 10;
  std::string output_file, flow_file, read_pb;
  std::string flow_output_file;    // DenseFlowOptions::flow_output_file: explicit path for --save_flow
  double pipeline_max_rate = 0;    // seg_tree.cpp:349 uses 20 frames/s for its root
  bool two_stage_oversegment = false;
  // SegmentationRenderUnit behind the segmentation (seg_tree.cpp --render_and_save); < 0: no render
  double render_level = -1;
  bool render_concat = false;
  double render_blend_alpha = 0.5;
  // vsg_render_level_regions at this level for every frame; < 0: off
  int level_regions = -1;
  // vsg_render_level_components at this level for every frame; < 0: off.  N4, or N8 with --components_n8
  int level_components = -1;
  bool components_n8 = false;
  // vsg_render_level_boundaries at this level for every frame; < 0: off.  Inner points of the regions, or
  // outer points with --boundaries_outer, of the components (N4, or N8 with --components_n8) with
  // --boundaries_components
  int level_boundaries = -1;
  bool boundaries_outer = false, boundaries_components = false;
  // vsg_render_level_adjacency at this level for every frame; < 0: off.  Pixel sides of the regions, or
  // with --adjacency_n8 also diagonal contacts, of the components (N4, or N8 with --components_n8) with
  // --adjacency_components
  int level_adjacency = -1;
  bool adjacency_n8 = false, adjacency_components = false;
  // vsg_render_level_overlap at this level for every frame after the first, with the previous frame's id
  // image at this level; < 0: off.  Of the regions, or of the components (N4, or N8 with --components_n8)
  // with --overlap_components
  int level_overlap = -1;
  bool overlap_components = false;
  // vsg_render_persistence_image and vsg_render_persistence_graph for every frame; the graph's
  // neighbourhood is --adjacency_n8's
  bool persistence = false;
  // vsg_render_tree_cut with this penalty for every frame after the first, against the previous frame's
  // level-0 id image; < 0: off
  long long tree_cut = -1;
  // vsg_render_level_colors and vsg_render_mean_frame at this level for every frame; < 0: off.  Of the
  // regions, or of the components (N4, or N8 with --components_n8) with --colors_components
  int level_colors = -1;
  bool colors_components = false;
  // vsg_render_level_pool at this level for every frame; < 0: off.  Of the regions, or of the components (N4, or
  // N8 with --components_n8) with --pool_components
  int level_pool = -1;
  bool pool_components = false;
  // vsg_render_level_contours at this level for every frame; < 0: off.  Of the regions, or of the components
  // (N4, or N8 with --components_n8) with --contours_components
  int level_contours = -1;
  bool contours_components = false;
  // vsg_render_level_mesh at this level for every frame; < 0: off.  Of the regions, or of the components
  // (N4, or N8 with --components_n8) with --mesh_components
  int level_mesh = -1;
  bool mesh_components = false;
  // mesh_simplified (--mesh_max_error was given): vsg_render_level_mesh_simplified with this max_error and
  // mesh_min_segment_points instead
  bool mesh_simplified = false, mesh_min_segment_points_given = false;
  float mesh_max_error = 1.0f;
  int mesh_min_segment_points = 4;
  // vsg_render_boundary_distance at this level for every frame; < 0: off
  int boundary_distance = -1;
  // vsg_render_boundary_benchmark with this tolerance_sq for every frame after the first, against the
  // previous frame's level-0 id image; < 0: off
  int boundary_benchmark = -1;
  // SegmentationRenderUnitOptions::volume_level; < 0: off.  The supervoxel lines go to volume_out, or to stdout
  int volume_level = -1;
  std::string volume_out;
  // SegmentationWriterUnitOptions::remove_rasterization (seg_tree.cpp:308 sets it for --write_to_file;
  // here it is opt-in, so that the files of existing runs stay what they were)
  bool remove_rasterization = false;
  int original_width = 0, original_height = 0;   // the video's size before a downscale; 0 = the frame size
  std::string rewrite_pb;
  // VideoReaderOptions::DOWNSCALE_TO_MIN_SIZE with this size (seg_tree.cpp:136-139); 0: no downscale
  int downscale_min_size = 0;
  // seg_tree.cpp:90-98: sets use_pipeline, write_to_file, downscale_min_size = 360 and switches the
  // render unit off (this driver has no display, logging or display_flow to override)
  bool run_on_server = false;
};

bool ParseFlags(int argc, char** argv, Flags* f) {
  auto as_bool = [](const std::string& v) { return !(v == "0" || v == "false" || v == "no"); };
  for (int i = 1; i < argc; ++i) {
    std::string a = argv[i];
    if (a.rfind("--", 0) != 0) {
      std::fprintf(stderr, "unexpected argument %s\n", a.c_str());
      return false;
    }
    a = a.substr(2);
    std::string v;
    bool has_v = false;
    const size_t eq = a.find('=');
    if (eq != std::string::npos) {
      v = a.substr(eq + 1);
      a = a.substr(0, eq);
      has_v = true;
    }
    static const char* kBools[] = {"flow", "use_pipeline", "over_segment", "write_to_file", "save_flow",
                                   "two_stage_oversegment", "region_segmentation", "render_concat",
                                   "compute_flow", "remove_rasterization", "run_on_server", "components_n8",
                                   "boundaries_outer", "boundaries_components", "adjacency_n8",
                                   "adjacency_components", "overlap_components", "persistence", "colors_components",
                                   "pool_components",
                                   "contours_components", "mesh_components",
                                   "help"};
    bool is_bool = false, negated = false;
    for (const char* b : kBools) {
      if (a == b) is_bool = true;
      if (a == std::string("no") + b) {
        is_bool = negated = true;
        a = b;
      }
    }
    if (!has_v && !(is_bool && (i + 1 >= argc || std::string(argv[i + 1]).rfind("--", 0) == 0)) &&
        !negated) {
      if (i + 1 >= argc) {
        std::fprintf(stderr, "flag --%s needs a value\n", a.c_str());
        return false;
      }
      v = argv[++i];
      has_v = true;
    }
    const bool bv = negated ? false : (has_v ? as_bool(v) : true);
    if (a == "flow") f->flow = bv;
    else if (a == "use_pipeline") f->use_pipeline = bv;
    else if (a == "over_segment") f->over_segment = bv;
    else if (a == "write_to_file") f->write_to_file = bv;
    else if (a == "save_flow") f->save_flow = bv;
    else if (a == "compute_flow") f->compute_flow = bv;
    else if (a == "two_stage_oversegment") f->two_stage_oversegment = bv;
    else if (a == "region_segmentation") f->region_segmentation = bv;
    else if (a == "render_concat") f->render_concat = bv;
    else if (a == "remove_rasterization") f->remove_rasterization = bv;
    else if (a == "run_on_server") f->run_on_server = bv;
    else if (a == "downscale_min_size") f->downscale_min_size = atoi(v.c_str());
    else if (a == "help") {
      std::printf(
          "seg_tree_synth: see the head of seg_tree_synth.cpp for the flags.\n"
          "  --downscale_min_size N  downscale every frame so that its smaller side is N (0: off)\n"
          "  --run_on_server         sets --use_pipeline, --write_to_file, --downscale_min_size 360 and\n"
          "                          switches --render_level off (seg_tree.cpp:90-98)\n");
      std::exit(0);
    }
    else if (a == "original_width") f->original_width = atoi(v.c_str());
    else if (a == "original_height") f->original_height = atoi(v.c_str());
    else if (a == "rewrite_pb") f->rewrite_pb = v;
    else if (a == "render_level") f->render_level = atof(v.c_str());
    else if (a == "render_blend_alpha") f->render_blend_alpha = atof(v.c_str());
    else if (a == "level_regions") f->level_regions = atoi(v.c_str());
    else if (a == "level_components") f->level_components = atoi(v.c_str());
    else if (a == "components_n8") f->components_n8 = bv;
    else if (a == "level_boundaries") f->level_boundaries = atoi(v.c_str());
    else if (a == "boundaries_outer") f->boundaries_outer = bv;
    else if (a == "boundaries_components") f->boundaries_components = bv;
    else if (a == "level_adjacency") f->level_adjacency = atoi(v.c_str());
    else if (a == "adjacency_n8") f->adjacency_n8 = bv;
    else if (a == "adjacency_components") f->adjacency_components = bv;
    else if (a == "level_overlap") f->level_overlap = atoi(v.c_str());
    else if (a == "overlap_components") f->overlap_components = bv;
    else if (a == "persistence") f->persistence = bv;
    else if (a == "tree_cut") f->tree_cut = atoll(v.c_str());
    else if (a == "level_colors") f->level_colors = atoi(v.c_str());
    else if (a == "colors_components") f->colors_components = bv;
    else if (a == "level_pool") f->level_pool = atoi(v.c_str());
    else if (a == "pool_components") f->pool_components = bv;
    else if (a == "level_contours") f->level_contours = atoi(v.c_str());
    else if (a == "boundary_distance") f->boundary_distance = atoi(v.c_str());
    else if (a == "boundary_benchmark") f->boundary_benchmark = atoi(v.c_str());
    else if (a == "volume_level") f->volume_level = atoi(v.c_str());
    else if (a == "volume_out") f->volume_out = v;
    else if (a == "contours_components") f->contours_components = bv;
    else if (a == "level_mesh") f->level_mesh = atoi(v.c_str());
    else if (a == "mesh_components") f->mesh_components = bv;
    else if (a == "mesh_max_error") {
      f->mesh_simplified = true;
      f->mesh_max_error = (float)atof(v.c_str());
    } else if (a == "mesh_min_segment_points") {
      f->mesh_min_segment_points_given = true;
      f->mesh_min_segment_points = atoi(v.c_str());
    }
    else if (a == "chunk_set_size") f->chunk_set_size = atoi(v.c_str());
    else if (a == "chunk_set_overlap") f->chunk_set_overlap = atoi(v.c_str());
    else if (a == "min_region_num") f->min_region_num = atoi(v.c_str());
    else if (a == "input_file") f->input_file = v;
    else if (a == "dense_smoothing") f->dense_smoothing = v;
    else if (a == "dense_color_dist") f->dense_color_dist = v;
    else if (a == "dense_min_region_size") f->dense_min_region_size = atof(v.c_str());
    else if (a == "width") f->width = atoi(v.c_str());
    else if (a == "height") f->height = atoi(v.c_str());
    else if (a == "frames") f->frames = atoi(v.c_str());
    else if (a == "chunk_size") f->chunk_size = atoi(v.c_str());
    else if (a == "device") f->device = atoi(v.c_str());
    else if (a == "input") f->input = v;
    else if (a == "output_file") f->output_file = v;
    else if (a == "flow_file") f->flow_file = v;
    else if (a == "flow_output_file") f->flow_output_file = v;
    else if (a == "read_pb") f->read_pb = v;
    else if (a == "pipeline_max_rate") f->pipeline_max_rate = atof(v.c_str());
    else {
      std::fprintf(stderr, "unknown flag --%s\n", a.c_str());
      return false;
    }
  }
  if (f->mesh_simplified && f->level_mesh < 0) {
    std::fprintf(stderr, "--mesh_max_error needs --level_mesh\n");
    return false;
  }
  if (f->mesh_min_segment_points_given && !f->mesh_simplified) {
    std::fprintf(stderr, "--mesh_min_segment_points needs --mesh_max_error\n");
    return false;
  }
  if (f->mesh_simplified && (!std::isfinite(f->mesh_max_error) || f->mesh_max_error < 0)) {
    std::fprintf(stderr, "--mesh_max_error has to be a finite number >= 0\n");
    return false;
  }
  if (!f->volume_out.empty() && f->volume_level < 0) {
    std::fprintf(stderr, "--volume_out needs --volume_level\n");
    return false;
  }
  if (f->volume_level >= 0 && f->render_level < 0) f->render_level = 0;   // the session lives in the render unit
  if (f->mesh_min_segment_points < 0) {
    std::fprintf(stderr, "--mesh_min_segment_points has to be >= 0\n");
    return false;
  }
  return true;
}

int main(int argc, char** argv) {
  Flags FLAGS;
  if (!ParseFlags(argc, argv, &FLAGS)) return 2;
  if (FLAGS.run_on_server) {   // seg_tree.cpp:90-98
    FLAGS.use_pipeline = true;
    FLAGS.render_level = -1;
    FLAGS.write_to_file = true;
    FLAGS.downscale_min_size = 360;
  }
  if (!FLAGS.read_pb.empty()) return ReadBack(FLAGS.read_pb);
  if (!FLAGS.rewrite_pb.empty()) {
    return Rewrite(FLAGS.rewrite_pb, FLAGS.output_file, FLAGS.remove_rasterization, FLAGS.original_width,
                   FLAGS.original_height);
  }
  bool use_flow = FLAGS.flow;
  int frames = FLAGS.frames;
  std::string flow_file = FLAGS.flow_file;
  const std::string input_base = FLAGS.input_file.substr(0, FLAGS.input_file.find_last_of("."));

  // Root: a raw BGR24 file (--input_file) or the synthetic source; with --input_file the flow
  // comes from "<input base>.flow" when that file exists (seg_tree.cpp:120-126).
  std::unique_ptr<RawVideoReaderUnit> raw_reader;
  if (!FLAGS.input_file.empty()) {
    RawVideoReaderOptions ro;
    ro.trim_frames = 0;
    raw_reader.reset(new RawVideoReaderUnit(ro, FLAGS.input_file));
    if (use_flow && flow_file.empty()) {
      const std::string candidate = input_base + ".flow";
      if (std::ifstream(candidate.c_str()).good()) flow_file = candidate;
      else if (!FLAGS.compute_flow) use_flow = false;   // segment without temporal displacement
    }
  }
  const bool flow_from_file = use_flow && !flow_file.empty();
  const std::string save_flow =
      !FLAGS.flow_output_file.empty() ? FLAGS.flow_output_file
      : FLAGS.save_flow ? (FLAGS.input_file.empty() ? std::string("synth.flow") : input_base + ".flow")
                        : std::string();
  // --compute_flow: the flow comes from the flow units below, which also write --save_flow's file
  const bool compute_flow = FLAGS.compute_flow && use_flow && !flow_from_file;
  // the synthetic flow is one of the frames the segmentation sees, so of the downscaled size
  int flow_width = 0, flow_height = 0;
  if (FLAGS.downscale_min_size > 0 &&
      vsg_resize_output_size(VSG_RESIZE_TO_MIN_SIZE, 1.0f, FLAGS.downscale_min_size, FLAGS.width, FLAGS.height,
                             &flow_width, &flow_height, nullptr) != VSG_OK) {
    std::fprintf(stderr, "ERROR: --downscale_min_size: %s\n", vsg_resize_last_error());
    return 2;
  }
  SyntheticVideoUnit source(FLAGS.width, FLAGS.height, frames, use_flow && !flow_from_file && !compute_flow,
                            FLAGS.input == "bench" ? 1 : (FLAGS.input == "soft" ? 2 : 0),
                            compute_flow ? std::string() : save_flow, FLAGS.original_width, FLAGS.original_height,
                            flow_width, flow_height);
  VideoUnit* root = raw_reader ? static_cast<VideoUnit*>(raw_reader.get()) : &source;
  VideoUnit* input = root;

  // The reference's reader scales its own frames (video_reader_unit.cpp:155-206); here the unit that
  // does it follows the root directly, in the root's pipeline segment.
  std::unique_ptr<DownscaleUnit> downscale_unit;
  if (FLAGS.downscale_min_size > 0) {   // seg_tree.cpp:136-139
    DownscaleUnitOptions downscale_options;
    downscale_options.downscale = DownscaleUnitOptions::DOWNSCALE_TO_MIN_SIZE;
    downscale_options.downscale_size = FLAGS.downscale_min_size;
    downscale_options.device = FLAGS.device;
    downscale_unit.reset(new DownscaleUnit(downscale_options));
    downscale_unit->AttachTo(input);
    input = downscale_unit.get();
  }

  // Pipeline segments as in seg_tree.cpp:155-163, 211-217: reader | [flow reader] dense
  // segmentation | sink + writer, each on its own thread.
  std::vector<std::unique_ptr<VideoPipelineSource>> sources;
  std::vector<std::unique_ptr<VideoPipelineSink>> sinks;
  auto cut = [&]() {
    sinks.emplace_back(new VideoPipelineSink());
    sinks.back()->AttachTo(input);
    sources.emplace_back(new VideoPipelineSource(sinks.back().get()));
    input = sources.back().get();
  };
  if (FLAGS.use_pipeline) cut();

  std::unique_ptr<DenseFlowReaderUnit> flow_reader;
  if (flow_from_file) {   // seg_tree.cpp:164-169
    flow_reader.reset(new DenseFlowReaderUnit(DenseFlowReaderOptions(), flow_file));
    flow_reader->AttachTo(input);
    input = flow_reader.get();
  }

  std::unique_ptr<LuminanceUnit> luminance;
  std::unique_ptr<DenseFlowUnit> flow_unit;
  if (compute_flow) {   // seg_tree.cpp:170-187
    luminance.reset(new LuminanceUnit());
    luminance->AttachTo(input);
    DenseFlowOptions flow_options;
    flow_options.flow_output_file = save_flow;
    flow_options.device = FLAGS.device;
    flow_unit.reset(new DenseFlowUnit(flow_options));
    flow_unit->AttachTo(luminance.get());
    input = flow_unit.get();
  }

  DenseSegmentationUnitOptions unit_options;
  if (!use_flow) unit_options.flow_stream_name.clear();   // seg_tree.cpp:195-198
  unit_options.device = FLAGS.device;
  DenseSegmentationOptions seg_options;
  seg_options.chunk_size = FLAGS.chunk_size;
  seg_options.two_stage_oversegment = FLAGS.two_stage_oversegment;
  if (FLAGS.over_segment) seg_options.compute_vectorization = true;   // seg_tree.cpp:202-204
  // dense_segmentation.cpp:79-101: the flags override the options.
  seg_options.frac_min_region_size = (float)FLAGS.dense_min_region_size;
  if (FLAGS.dense_smoothing == "none") seg_options.presmoothing = DenseSegmentationOptions::PRESMOOTH_NONE;
  else if (FLAGS.dense_smoothing == "bilateral") seg_options.presmoothing = DenseSegmentationOptions::PRESMOOTH_BILATERAL;
  else if (FLAGS.dense_smoothing == "gaussian") seg_options.presmoothing = DenseSegmentationOptions::PRESMOOTH_GAUSSIAN;
  else {
    std::fprintf(stderr, "ERROR: --dense_smoothing %s is not supported (none | gaussian | bilateral)\n",
                 FLAGS.dense_smoothing.c_str());
    return 2;
  }
  if (FLAGS.dense_color_dist == "l1") seg_options.color_distance = DenseSegmentationOptions::COLOR_DISTANCE_L1;
  else if (FLAGS.dense_color_dist == "l2") seg_options.color_distance = DenseSegmentationOptions::COLOR_DISTANCE_L2;
  else {
    std::fprintf(stderr, "ERROR: unknown --dense_color_dist %s (l1 | l2)\n", FLAGS.dense_color_dist.c_str());
    return 2;
  }
  DenseSegmentationUnit dense_unit(unit_options, &seg_options);
  dense_unit.AttachTo(input);
  input = &dense_unit;
  if (FLAGS.use_pipeline) cut();

  std::unique_ptr<RegionSegmentationUnit> region_unit;   // seg_tree.cpp:219-241
  if (FLAGS.region_segmentation && !FLAGS.over_segment) {
    RegionSegmentationUnitOptions ro;
    if (!use_flow) ro.flow_stream_name.clear();
    RegionSegmentationOptions rso;
    rso.chunk_set_size = FLAGS.chunk_set_size;
    rso.chunk_set_overlap = FLAGS.chunk_set_overlap;
    rso.min_region_num = FLAGS.min_region_num;
    region_unit.reset(new RegionSegmentationUnit(ro, &rso));
    region_unit->AttachTo(input);
    input = region_unit.get();
    if (FLAGS.use_pipeline) cut();
  }

  // With --remove_rasterization the label sink and the writer come first (they read the rasters), then
  // the descs are made vector-only for the render unit.
  HashSinkUnit sink;
  std::unique_ptr<SegmentationWriterUnit> writer;
  auto attach_sink_and_writer = [&]() {
    sink.AttachTo(input);
    input = &sink;
    if (FLAGS.write_to_file || !FLAGS.output_file.empty()) {   // seg_tree.cpp:296-312
      SegmentationWriterUnitOptions wo;
      wo.filename = !FLAGS.output_file.empty() ? FLAGS.output_file
                    : (FLAGS.input_file.empty() ? std::string("synth.pb") : FLAGS.input_file + ".pb");
      wo.remove_rasterization = FLAGS.remove_rasterization;
      writer.reset(new SegmentationWriterUnit(wo));
      writer->AttachTo(input);
      input = writer.get();
    }
  };
  RemoveRasterizationUnit remove_unit;
  if (FLAGS.remove_rasterization) {
    attach_sink_and_writer();
    if (FLAGS.render_level >= 0) {
      remove_unit.AttachTo(input);
      input = &remove_unit;
    }
  }

  // the regions of a level, from the descs as the segmentation leaves them (rasters or vector-only)
  std::unique_ptr<LevelRegionsSinkUnit> level_sink;
  if (FLAGS.level_regions >= 0) {
    level_sink.reset(new LevelRegionsSinkUnit(FLAGS.level_regions, FLAGS.device));
    level_sink->AttachTo(input);
    input = level_sink.get();
  }
  std::unique_ptr<LevelComponentsSinkUnit> components_sink;
  if (FLAGS.level_components >= 0) {
    components_sink.reset(new LevelComponentsSinkUnit(FLAGS.level_components, FLAGS.components_n8, FLAGS.device));
    components_sink->AttachTo(input);
    input = components_sink.get();
  }
  std::unique_ptr<LevelBoundariesSinkUnit> boundaries_sink;
  if (FLAGS.level_boundaries >= 0) {
    const int connectedness = !FLAGS.boundaries_components ? 0
                              : FLAGS.components_n8        ? VSG_RENDER_CONNECT_N8
                                                           : VSG_RENDER_CONNECT_N4;
    boundaries_sink.reset(
        new LevelBoundariesSinkUnit(FLAGS.level_boundaries, connectedness, FLAGS.boundaries_outer, FLAGS.device));
    boundaries_sink->AttachTo(input);
    input = boundaries_sink.get();
  }
  std::unique_ptr<LevelAdjacencySinkUnit> adjacency_sink;
  if (FLAGS.level_adjacency >= 0) {
    const int connectedness = !FLAGS.adjacency_components ? 0
                              : FLAGS.components_n8       ? VSG_RENDER_CONNECT_N8
                                                          : VSG_RENDER_CONNECT_N4;
    adjacency_sink.reset(
        new LevelAdjacencySinkUnit(FLAGS.level_adjacency, connectedness, FLAGS.adjacency_n8, FLAGS.device));
    adjacency_sink->AttachTo(input);
    input = adjacency_sink.get();
  }
  std::unique_ptr<LevelOverlapSinkUnit> overlap_sink;
  if (FLAGS.level_overlap >= 0) {
    const int connectedness = !FLAGS.overlap_components ? 0
                              : FLAGS.components_n8     ? VSG_RENDER_CONNECT_N8
                                                        : VSG_RENDER_CONNECT_N4;
    overlap_sink.reset(new LevelOverlapSinkUnit(FLAGS.level_overlap, connectedness, FLAGS.device));
    overlap_sink->AttachTo(input);
    input = overlap_sink.get();
  }
  std::unique_ptr<TreeCutSinkUnit> tree_cut_sink;
  if (FLAGS.tree_cut >= 0) {
    tree_cut_sink.reset(new TreeCutSinkUnit(FLAGS.tree_cut, FLAGS.device));
    tree_cut_sink->AttachTo(input);
    input = tree_cut_sink.get();
  }
  std::unique_ptr<PersistenceSinkUnit> persistence_sink;
  if (FLAGS.persistence) {
    persistence_sink.reset(new PersistenceSinkUnit(FLAGS.adjacency_n8, FLAGS.device));
    persistence_sink->AttachTo(input);
    input = persistence_sink.get();
  }
  std::unique_ptr<LevelColorsSinkUnit> colors_sink;
  if (FLAGS.level_colors >= 0) {
    const int connectedness = !FLAGS.colors_components ? 0
                              : FLAGS.components_n8    ? VSG_RENDER_CONNECT_N8
                                                       : VSG_RENDER_CONNECT_N4;
    colors_sink.reset(new LevelColorsSinkUnit(FLAGS.level_colors, connectedness, FLAGS.device));
    colors_sink->AttachTo(input);
    input = colors_sink.get();
  }
  std::unique_ptr<LevelPoolSinkUnit> pool_sink;
  if (FLAGS.level_pool >= 0) {
    const int connectedness = !FLAGS.pool_components ? 0
                              : FLAGS.components_n8  ? VSG_RENDER_CONNECT_N8
                                                     : VSG_RENDER_CONNECT_N4;
    pool_sink.reset(new LevelPoolSinkUnit(FLAGS.level_pool, connectedness, FLAGS.device));
    pool_sink->AttachTo(input);
    input = pool_sink.get();
  }
  std::unique_ptr<LevelContoursSinkUnit> contours_sink;
  if (FLAGS.level_contours >= 0) {
    const int connectedness = !FLAGS.contours_components ? 0
                              : FLAGS.components_n8      ? VSG_RENDER_CONNECT_N8
                                                         : VSG_RENDER_CONNECT_N4;
    contours_sink.reset(new LevelContoursSinkUnit(FLAGS.level_contours, connectedness, FLAGS.device));
    contours_sink->AttachTo(input);
    input = contours_sink.get();
  }
  std::unique_ptr<LevelMeshSinkUnit> mesh_sink;
  if (FLAGS.level_mesh >= 0) {
    const int connectedness = !FLAGS.mesh_components ? 0
                              : FLAGS.components_n8  ? VSG_RENDER_CONNECT_N8
                                                     : VSG_RENDER_CONNECT_N4;
    mesh_sink.reset(new LevelMeshSinkUnit(FLAGS.level_mesh, connectedness, FLAGS.device,
                                          FLAGS.mesh_simplified ? FLAGS.mesh_max_error : -1.0f,
                                          FLAGS.mesh_min_segment_points));
    mesh_sink->AttachTo(input);
    input = mesh_sink.get();
  }
  std::unique_ptr<BoundaryDistanceSinkUnit> distance_sink;
  if (FLAGS.boundary_distance >= 0 || FLAGS.boundary_benchmark >= 0) {
    distance_sink.reset(new BoundaryDistanceSinkUnit(FLAGS.boundary_distance, FLAGS.boundary_benchmark, FLAGS.device));
    distance_sink->AttachTo(input);
    input = distance_sink.get();
  }

  std::unique_ptr<SegmentationRenderUnit> render_unit;   // seg_tree.cpp:254-294
  RenderHashSinkUnit render_sink;
  if (FLAGS.render_level >= 0) {
    SegmentationRenderUnitOptions render_options;
    render_options.hierarchy_level = (float)FLAGS.render_level;
    render_options.concat_with_source = FLAGS.render_concat;
    render_options.blend_alpha = (float)FLAGS.render_blend_alpha;
    render_options.device = FLAGS.device;
    render_options.volume_level = FLAGS.volume_level;
    render_unit.reset(new SegmentationRenderUnit(render_options));
    render_unit->AttachTo(input);
    render_sink.AttachTo(render_unit.get());
    input = &render_sink;
  }

  if (!FLAGS.remove_rasterization) attach_sink_and_writer();

  if (!root->PrepareProcessing()) {
    std::fprintf(stderr, "ERROR: Setup failed.\n");
    return 1;
  }
  const auto t0 = std::chrono::steady_clock::now();
  if (!FLAGS.use_pipeline) {
    root->Run();
  } else {   // seg_tree.cpp:339-364
    VideoPipelineInvoker invoker;
    RatePolicy pipeline_policy;
    pipeline_policy.max_rate = (float)FLAGS.pipeline_max_rate;
    invoker.RunRootRateLimited(pipeline_policy, root);
    for (size_t k = 0; k + 1 < sources.size(); ++k) invoker.RunPipelineSource(sources[k].get());
    sources.back()->Run();   // the last segment runs on the main thread
    invoker.WaitUntilPipelineFinished();
  }
  if (raw_reader) frames = raw_reader->num_frames();
  const double dt = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  std::printf("frames=%d first_frame_regions=%d total_regions=%ld label_fnv1a32=%08x bytes=%zu "
              "seconds=%.3f fps=%.2f pipeline=%d hierarchy_levels=%d\n",
              sink.frames(), sink.first_regions(), sink.total_regions(), sink.hash(), sink.bytes(),
              dt, sink.frames() / dt, FLAGS.use_pipeline ? 1 : 0, sink.first_levels());
  if (render_unit) {
    std::printf("render_frames=%d render_fnv1a32=%08x render_level=%d\n", render_sink.frames(), render_sink.hash(),
                render_unit->hierarchy_level());
  }
  if (render_unit && FLAGS.volume_level >= 0) {
    std::vector<vsg_render_volume_row> rows;
    std::vector<vsg_render_volume_col> cols;
    std::vector<vsg_render_volume_pair> pairs;
    if (!render_unit->VolumeTable(&rows, &cols, &pairs)) {
      std::fprintf(stderr, "ERROR: could not read the volume table: %s\n", vsg_render_last_error());
      return 1;
    }
    uint32_t hash = 2166136261u;
    const unsigned char* bytes = reinterpret_cast<const unsigned char*>(rows.data());
    for (size_t k = 0; k < rows.size() * sizeof(vsg_render_volume_row); ++k) hash = (hash ^ bytes[k]) * 16777619u;
    long long voxels = 0;
    for (const vsg_render_volume_row& r : rows) voxels += r.volume;
    std::printf("volume_level=%d volume_frames=%d volume_supervoxels=%zu volume_voxels=%lld volume_fnv1a32=%08x\n",
                FLAGS.volume_level, render_sink.frames(), rows.size(), voxels, hash);
    FILE* out = FLAGS.volume_out.empty() ? stdout : std::fopen(FLAGS.volume_out.c_str(), "w");
    if (!out) {
      std::fprintf(stderr, "ERROR: could not open %s\n", FLAGS.volume_out.c_str());
      return 1;
    }
    for (const vsg_render_volume_row& r : rows) {
      std::fprintf(out, "%s%d %d %d %d %lld %d %d %d %d %lld %lld %lld %lld %lld %lld\n",
                   FLAGS.volume_out.empty() ? "supervoxel " : "", r.id, r.first_frame, r.last_frame, r.frames,
                   (long long)r.volume, r.min_x, r.min_y, r.max_x, r.max_y, (long long)r.sum_x, (long long)r.sum_y,
                   (long long)r.sum_t, (long long)r.sum[0], (long long)r.sum[1], (long long)r.sum[2]);
    }
    if (out != stdout) std::fclose(out);
  }
  if (level_sink) {
    std::printf("level_regions=%ld level_intervals=%ld level_fnv1a32=%08x\n", level_sink->regions(),
                level_sink->intervals(), level_sink->hash());
  }
  if (components_sink) {
    std::printf("level_components=%ld component_intervals=%ld component_fnv1a32=%08x\n", components_sink->components(),
                components_sink->intervals(), components_sink->hash());
  }
  if (boundaries_sink) {
    std::printf("level_boundaries=%ld boundary_points=%ld boundary_fnv1a32=%08x\n", boundaries_sink->boundaries(),
                boundaries_sink->points(), boundaries_sink->hash());
  }
  if (adjacency_sink) {
    std::printf("level_adjacency_nodes=%ld adjacency_edges=%ld adjacency_fnv1a32=%08x\n", adjacency_sink->nodes(),
                adjacency_sink->edges(), adjacency_sink->hash());
  }
  if (overlap_sink) {
    std::printf("level_overlap_rows=%ld overlap_cols=%ld overlap_pairs=%ld overlap_fnv1a32=%08x\n",
                overlap_sink->rows(), overlap_sink->cols(), overlap_sink->pairs(), overlap_sink->hash());
  }
  if (tree_cut_sink) {
    std::printf("tree_cut_nodes=%ld tree_cut_total=%lld tree_cut_fnv1a32=%08x\n", tree_cut_sink->nodes(),
                tree_cut_sink->total(), tree_cut_sink->hash());
  }
  if (persistence_sink) {
    std::printf("persistence_levels=%d persistence_edge_pixels=%ld persistence_edges=%ld persistence_fnv1a32=%08x\n",
                persistence_sink->levels(), persistence_sink->edge_pixels(), persistence_sink->edges(),
                persistence_sink->hash());
  }
  if (colors_sink) {
    std::printf("level_colors_groups=%ld level_colors_fnv1a32=%08x\n", colors_sink->groups(), colors_sink->hash());
  }
  if (pool_sink) {
    const double* t = pool_sink->totals();
    std::printf("level_pool_groups=%ld level_pool_sums=%.17g,%.17g,%.17g,%.17g,%.17g level_pool_fnv1a32=%08x\n",
                pool_sink->groups(), t[0], t[1], t[2], t[3], t[4], pool_sink->hash());
  }
  if (contours_sink) {
    std::printf("level_contours_count=%ld level_contours_fnv1a32=%08x\n", contours_sink->contours(),
                contours_sink->hash());
  }
  if (mesh_sink) {
    std::printf(FLAGS.mesh_simplified ? "level_mesh_simplified_count=%ld level_mesh_simplified_fnv1a32=%08x\n"
                                          : "level_mesh_count=%ld level_mesh_fnv1a32=%08x\n",
                mesh_sink->segments(), mesh_sink->hash());
  }
  if (distance_sink && distance_sink->level() >= 0) {
    std::printf("boundary_distance_level=%d boundary_distance_edge_pixels=%ld boundary_distance_max=%ld "
                "boundary_distance_fnv1a32=%08x\n",
                distance_sink->level(), distance_sink->edge_pixels(), distance_sink->max_distance(),
                distance_sink->distance_hash());
  }
  if (distance_sink && distance_sink->tolerance_sq() >= 0) {
    const long* sums = distance_sink->sums();
    std::printf("boundary_benchmark_levels=%d boundary_seg_edges=%ld boundary_seg_matched=%ld boundary_gt_edges=%ld "
                "boundary_gt_matched=%ld boundary_benchmark_fnv1a32=%08x\n",
                distance_sink->levels(), sums[0], sums[1], sums[2], sums[3], distance_sink->benchmark_hash());
  }
  std::fprintf(stderr, "__SEGMENTATION_FINISHED__\n");
  return sink.frames() == frames ? 0 : 3;
}
