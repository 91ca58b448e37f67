/*
 * vsg_resize.h -- C ABI of the downscale stage (libvsg_resize.so).
 *
 * Mirrors the scaling the reference's reader does before anything else sees a frame
 * (VideoReaderOptions::downscale, video_framework/video_reader_unit.cpp:155-206, :261-270, :374) on
 * an MI355X: BGR24 frames go in, in host or device memory, and the downscaled BGR24 frame comes out,
 * in host or device memory, ready for libvsg_flow.so and libvsg_hip.so.  The library is independent
 * of libvsg_hip.so, libvsg_render.so and libvsg_flow.so.
 *
 * The output size is the reference's rule, evaluated in f32 where the reference is in f32
 * (vsg_resize_output_size).  The resampling is NOT pinned by the reference: it calls swscale's
 * SWS_BICUBIC on a decoded YUV frame, and neither swscale nor a codec is part of the reference tree
 * (parity unpinned).  The definition of what this library computes is the numpy model
 * tests/resize_model.py: a separable Keys bicubic, a = -0.6, whose support widens with the ratio,
 * horizontal pass first into unrounded f32, every f32 operation rounded on its own, rint and
 * saturation at the end.  The library equals it byte for byte.
 *
 * Conventions are those of vsg.h: every function returns VSG_OK (0) or a negative status,
 * vsg_resize_last_error() is a thread-local message of the last failure, a handle is
 * thread-compatible and owns one HIP stream, and there is NO CPU fallback: without a usable HIP
 * device vsg_resize_create fails with VSG_ERR_DEVICE.  Every call returns after its work on the
 * handle's stream has finished (one synchronisation), so an output in device memory is complete on
 * return; inputs in device memory have to be complete when the call is made.
 *
 * Limits: frame sizes in [1, 65535]; at most VSG_RESIZE_MAX_TAPS_H source pixels per output pixel
 * horizontally (a ratio of 256), because a workgroup of the horizontal pass keeps its source span
 * in LDS.
 *
 * Not offered (the reference has it): pixel formats other than BGR24, YUV input, swscale bit
 * parity.
 */
#ifndef VSG_RESIZE_H_
#define VSG_RESIZE_H_

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

/* VideoReaderOptions::DownScale (video_reader_unit.h) */
#define VSG_RESIZE_NONE 0
#define VSG_RESIZE_BY_FACTOR 1
#define VSG_RESIZE_TO_MIN_SIZE 2
#define VSG_RESIZE_TO_MAX_SIZE 3

#define VSG_RESIZE_MAX_TAPS_H 1024

typedef struct vsg_resize vsg_resize;

typedef struct vsg_resize_options {
  int mode;      /* VSG_RESIZE_NONE                                                           */
  float factor;  /* 0.5 (video_reader_unit.h): used by VSG_RESIZE_BY_FACTOR, at most 1        */
  int size;      /* 0: used by the two size modes, the length the smaller / larger side gets  */
  int device;    /* -1 = the caller's current HIP device                                      */
} vsg_resize_options;

/* What the last process call of a handle did.  Times are HIP events on the handle's stream. */
typedef struct vsg_resize_stats {
  int launches;                /* kernels + copies enqueued by the call                             */
  int host_syncs;              /* stream synchronisations of the call: 1                            */
  int taps_h, taps_v;          /* widest filter row of each axis; 0 for a copied frame              */
  int64_t device_allocations;  /* hipMalloc calls of the handle since creation                      */
  float upload_us;             /* a host frame to the device                                        */
  float horizontal_us;         /* k_resize_h                                                        */
  float vertical_us;           /* k_resize_v                                                        */
  float download_us;           /* the result to host memory                                         */
  float copy_us;               /* the copy of a frame whose size does not change                    */
} vsg_resize_stats;

const char* vsg_resize_last_error(void);
void vsg_resize_default_options(vsg_resize_options* o);

/* OpenStreams' size rule.  factor = 1 (NONE), the given one (BY_FACTOR, above 1 is an error), or
 * min(1, max / min(size * (1.0f / in_w), size * (1.0f / in_h))) (TO_MIN_SIZE / TO_MAX_SIZE), all in
 * f32; out = ceil(in * factor) on the f32 product; the width is then made even (the height is not);
 * width_step = out_w * 3 padded to a multiple of 4.  A size <= 0 with a size mode, or an output below
 * 1 x 1, is VSG_ERR_INVALID.  Any out pointer may be null.  Host only; needs no device. */
int vsg_resize_output_size(int mode, float factor, int size, int in_w, int in_h, int* out_w, int* out_h,
                           int* width_step);

/* The filter of one axis as the kernels use it.  Output o reads the count[o] source indices
 * clamp(first[o] + j, 0, n_in - 1), j = 0 .. count[o] - 1 (first may be negative), with weights
 * weights[o * max_taps + j]; a row is zero beyond its count.  *max_taps is always set.  first and
 * count hold n_out ints, weights `capacity` floats.  A call with three null arrays and capacity 0
 * only asks for max_taps; otherwise a null array or capacity < n_out * max_taps is VSG_ERR_INVALID
 * and nothing is written.  Host only; needs no device. */
int vsg_resize_filter(int n_in, int n_out, int32_t* first, int32_t* count, float* weights, size_t capacity,
                      int* max_taps);

int vsg_resize_create(const vsg_resize_options* o, int in_w, int in_h, vsg_resize** h);
void vsg_resize_destroy(vsg_resize* h);

/* The handle's output size and the padded row size OpenStreams gives the stream. */
int vsg_resize_get_output_size(vsg_resize* h, int* out_w, int* out_h, int* width_step);

/* One frame.  bgr_in: in_h rows of stride_in bytes (BGR24) in mem_in memory; bgr_out: out_h rows of
 * stride_out bytes in mem_out memory.  Strides have to cover a row (in_w * 3, out_w * 3); any
 * alignment of pointers and strides is accepted.  Bytes of an output row beyond out_w * 3 are never
 * written. */
int vsg_resize_process(vsg_resize* h, const uint8_t* bgr_in, size_t stride_in, int mem_in, uint8_t* bgr_out,
                       size_t stride_out, int mem_out);

int vsg_resize_last_stats(vsg_resize* h, vsg_resize_stats* s);

#ifdef __cplusplus
}
#endif

#endif /* VSG_RESIZE_H_ */
