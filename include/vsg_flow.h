/*
 * vsg_flow.h -- C ABI of the dense optical flow unit (libvsg_flow.so).
 *
 * Mirrors the reference's LuminanceUnit -> DenseFlowUnit pair (video_framework/conversion_units.cpp:
 * 75-105, video_framework/flow_reader.{h,cpp}:141-371) on an MI355X: BGR24 (or 8-bit luminance)
 * frames go in, one dense Dual TV-L1 flow field per frame pair comes out as W*H (x, y) f32 pairs in
 * host or device memory -- the layout vsg_stream_process_frame reads its flow from.  The library is
 * independent of libvsg_hip.so and libvsg_render.so.
 *
 * The reference calls OpenCV's OpticalFlowDual_TVL1, which is not part of the reference tree; its
 * arithmetic is therefore not pinned by the reference.  The definition of what this library
 * computes is the numpy f32 model tests/flow_model.py (Zach/Pock/Bischof 2007 as laid out by
 * Sanchez/Meinhardt-Llopis/Facciolo, IPOL 2013, in the structure of OpenCV 2.4); the library equals
 * it bit for bit.  Fixed parameters: tau 0.25, lambda 0.15, theta 0.3, nscales 5, epsilon 0.01, no
 * initial flow.
 *
 * Conventions are those of vsg.h: every function returns VSG_OK (0) or a negative status,
 * vsg_flow_last_error() is a thread-local message of the last failure, a handle is
 * thread-compatible and owns one HIP stream, and there is NO CPU fallback: without a usable HIP
 * device vsg_flow_create fails with VSG_ERR_DEVICE.  Every call returns after its work on the
 * handle's stream has finished, so an output in device memory is complete on return; inputs in
 * device memory have to be complete when the call is made.
 *
 * Not offered (the reference has it): video_out_stream_name, the HSV picture of the flow.
 */
#ifndef VSG_FLOW_H_
#define VSG_FLOW_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#ifndef VSG_OK
#define VSG_OK 0
#define VSG_ERR_INVALID -1
#define VSG_ERR_DEVICE -2
#define VSG_ERR_STATE -3
#define VSG_ERR_INTERNAL -4
#define VSG_MEM_HOST 0
#define VSG_MEM_DEVICE 1
#endif

/* DenseFlowOptions::flow_type (flow_reader.h:134-140) */
#define VSG_FLOW_BACKWARD 0
#define VSG_FLOW_FORWARD 1
#define VSG_FLOW_BOTH 2

typedef struct vsg_flow vsg_flow;

typedef struct vsg_flow_options {
  int flow_type;    /* VSG_FLOW_BACKWARD                                                     */
  int iterations;   /* 10 (flow_reader.h:143): inner iterations per warp, at most             */
  int warps;        /* 2 (flow_reader.h:144): warps per scale                                 */
  int device;       /* -1 = the caller's current HIP device                                   */
} vsg_flow_options;

/* What the last process call of a handle did.  Times are HIP events on the handle's stream. */
typedef struct vsg_flow_stats {
  int scales;                  /* pyramid levels of the handle's frame size                         */
  int launches;                /* kernels + memsets + copies enqueued by the call                   */
  int iterations_run;          /* inner iterations that did work (the others returned at once)      */
  int host_syncs;              /* stream synchronisations of the call: 1                            */
  int64_t device_allocations;  /* hipMalloc / hipHostMalloc calls of the handle since creation      */
  float pyramid_us;            /* upload, luminance, pyrDown chain                                  */
  float warp_us;               /* gradient, warp kernels, upsampling (sum over scales)              */
  float iterate_us;            /* inner iteration kernels (sum over scales and warps)               */
  float export_us;             /* flow to the caller's memory                                       */
} vsg_flow_stats;

const char* vsg_flow_last_error(void);
void vsg_flow_default_options(vsg_flow_options* o);

int vsg_flow_create(const vsg_flow_options* o, int width, int height, vsg_flow** h);
void vsg_flow_destroy(vsg_flow* h);

/* One frame.  bgr: H rows of `stride` bytes (BGR24) in mem_in memory.  backward_out / forward_out:
 * W*H*2 f32 in mem_out memory; the one the handle's flow_type asks for is required, the other is
 * ignored.  backward = calc(current, previous) (flow_reader.cpp:291-294), forward =
 * calc(previous, current).  *has_flow is 0 for the first frame after creation or restart (nothing
 * is written), 1 afterwards.  The previous frame's luminance pyramid stays on the device. */
int vsg_flow_process_frame(vsg_flow* h, const uint8_t* bgr, size_t stride, int mem_in,
                           float* backward_out, float* forward_out, int mem_out, int* has_flow);

/* The same with an 8-bit single-channel frame (H rows of `stride` bytes). */
int vsg_flow_process_luminance(vsg_flow* h, const uint8_t* lum, size_t stride, int mem_in,
                               float* backward_out, float* forward_out, int mem_out, int* has_flow);

/* Forgets the previous frame: the next frame is a first frame again.  Device memory is kept. */
int vsg_flow_restart(vsg_flow* h);

int vsg_flow_last_stats(vsg_flow* h, vsg_flow_stats* s);

/* cvtColor(BGR2GRAY) on 8-bit data: (1868*B + 9617*G + 4899*R + 8192) >> 14, W*H bytes out.  Host
 * only; needs no device. */
int vsg_flow_luminance(const uint8_t* bgr, size_t stride, int width, int height, uint8_t* out);

#ifdef __cplusplus
}
#endif

#endif /* VSG_FLOW_H_ */
