/* gfwarp.h — C ABI of libgfwarp, the MI355X (gfx950) warp backend.
 *
 * This is the drop-in boundary for gyroflow-core's per-pixel
 * undistort -> rotate (rolling shutter) -> redistort -> sample path.  Every
 * entry point states the reference interface it stands in for
 * (paths relative to the gyroflow tree, v1.6.3):
 *
 *   backend object          src/core/gpu/opencl.rs:178   OclWrapper::new
 *                           src/core/gpu/wgpu.rs:147     WgpuWrapper::new
 *   per-plane call          src/core/gpu/opencl.rs:330   OclWrapper::undistort_image
 *                           src/core/gpu/wgpu.rs:454     WgpuWrapper::undistort_image
 *   CPU twin (authoritative arithmetic)
 *                           src/core/stabilization/cpu_undistort.rs:233
 *   uniform block           src/core/stabilization/mod.rs:101-150  KernelParams
 *   buffers                 src/core/gpu/mod.rs:17-71    Buffers / BufferDescription / BufferSource
 *
 * Plain C: pointers and sizes only, no C++/torch types.  All functions are
 * thread-safe with respect to *different* contexts; one context is
 * single-thread-affine exactly like the reference's thread-local backend
 * caches (stabilization/mod.rs:59-66).
 */
#ifndef GFWARP_H
#define GFWARP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GFW_ABI_VERSION 2

/* ---- KernelParams: byte-exact mirror of stabilization/mod.rs:101-150 ------
 * #[repr(C, packed(4))], 92 four-byte words = 368 bytes. */
typedef struct gfw_kernel_params {
    int32_t width;               /*   0 */
    int32_t height;              /*   4 */
    int32_t stride;              /*   8  bytes */
    int32_t output_width;        /*  12 */
    int32_t output_height;       /*  16 */
    int32_t output_stride;       /*  20  bytes */
    int32_t matrix_count;        /*  24  1 = no rolling-shutter correction */
    int32_t interpolation;       /*  28  2,4,8 = LUT taps; 10..13 = EWA */
    int32_t background_mode;     /*  32  0 solid,1 repeat,2 mirror,3 margin+feather */
    int32_t flags;               /*  36  GFW_FLAG_* */
    int32_t bytes_per_pixel;     /*  40 */
    int32_t pix_element_count;   /*  44 */
    float   background[4];       /*  48 */
    float   f[2];                /*  64 */
    float   c[2];                /*  72 */
    float   k[12];               /*  80 */
    float   fov;                 /* 128 */
    float   r_limit;             /* 132 */
    float   lens_correction_amount;    /* 136 */
    float   input_vertical_stretch;    /* 140 */
    float   input_horizontal_stretch;  /* 144 */
    float   background_margin;         /* 148 */
    float   background_margin_feather; /* 152 */
    float   canvas_scale;              /* 156 */
    float   input_rotation;            /* 160  degrees */
    float   output_rotation;           /* 164  degrees */
    float   translation2d[2];          /* 168 */
    float   translation3d[4];          /* 176 */
    int32_t source_rect[4];            /* 192  x,y,w,h */
    int32_t output_rect[4];            /* 208  x,y,w,h */
    float   digital_lens_params[16];   /* 224 */
    float   safe_area_rect[4];         /* 288 */
    float   max_pixel_value;           /* 304 */
    int32_t distortion_model;          /* 308  GFW_MODEL_* (not trusted: see gfw_create) */
    int32_t digital_lens;              /* 312 */
    float   pixel_value_limit;         /* 316 */
    float   light_refraction_coefficient; /* 320 */
    int32_t plane_index;               /* 324 */
    float   reserved1;                 /* 328 */
    float   reserved2;                 /* 332 */
    float   ewa_coeffs_p[4];           /* 336 */
    float   ewa_coeffs_q[4];           /* 352 */
} gfw_kernel_params;                   /* 368 */

/* KernelParamsFlags, stabilization/mod.rs:83-99 */
enum {
    GFW_FLAG_FIX_COLOR_RANGE      = 1 << 0,
    GFW_FLAG_HAS_DIGITAL_LENS     = 1 << 1,
    GFW_FLAG_FILL_WITH_BACKGROUND = 1 << 2,
    GFW_FLAG_DRAWING_ENABLED      = 1 << 3,
    GFW_FLAG_HORIZONTAL_RS        = 1 << 4,
    GFW_FLAG_HAS_SOURCE_RECT      = 1 << 5,
    GFW_FLAG_HAS_OUTPUT_RECT      = 1 << 6,
    GFW_FLAG_FRAMEBUFFER_INVERTED = 1 << 7,
    GFW_FLAG_HAS_IBIS_DATA        = 1 << 8,
    GFW_FLAG_HAS_MESH_DATA        = 1 << 9,
    GFW_FLAG_HAS_FPD_DATA         = 1 << 10,
    GFW_FLAG_ANY_UNDERWATER       = 1 << 11
};

/* Interpolation, stabilization/mod.rs:25-34 */
enum {
    GFW_INTERP_BILINEAR       = 2,
    GFW_INTERP_BICUBIC        = 4,
    GFW_INTERP_LANCZOS4       = 8,
    GFW_INTERP_ROBIDOUX_SHARP = 10,
    GFW_INTERP_ROBIDOUX       = 11,
    GFW_INTERP_MITCHELL       = 12,
    GFW_INTERP_CATMULL_ROM    = 13
};

/* Distortion model ids: src/core/gpu/stabilize_spirv/src/distortion_models/mod.rs:62-81
 * (declaration order of impl_models!).  GoPro6Superview has no id there
 * (it exists only in stabilization/distortion_models/mod.rs:107); 14 is ours. */
enum {
    GFW_MODEL_NONE               = 0,
    GFW_MODEL_OPENCV_FISHEYE     = 1,
    GFW_MODEL_OPENCV_STANDARD    = 2,
    GFW_MODEL_POLY3              = 3,
    GFW_MODEL_POLY5              = 4,
    GFW_MODEL_PTLENS             = 5,
    GFW_MODEL_INSTA360           = 6,
    GFW_MODEL_SONY               = 7,
    GFW_MODEL_GENERIC_POLYNOMIAL = 8,
    GFW_MODEL_GOPRO              = 9,
    GFW_MODEL_GOPRO_SUPERVIEW    = 10,
    GFW_MODEL_GOPRO_HYPERVIEW    = 11,
    GFW_MODEL_GOPRO_WARP         = 12,
    GFW_MODEL_DIGITAL_STRETCH    = 13,
    GFW_MODEL_GOPRO6_SUPERVIEW   = 14
};

/* PixelType implementors, stabilization/pixel_formats.rs:48-60 (declaration order) */
enum {
    GFW_PIX_LUMA8   = 0,
    GFW_PIX_LUMA16  = 1,
    GFW_PIX_RGB8    = 2,
    GFW_PIX_RGBA8   = 3,
    GFW_PIX_BGRA8   = 4,
    GFW_PIX_RGB16   = 5,
    GFW_PIX_RGBA16  = 6,
    GFW_PIX_AYUV16  = 7,
    GFW_PIX_RGBAF   = 8,
    GFW_PIX_RGBAF16 = 9,
    GFW_PIX_R32F    = 10,
    GFW_PIX_UV8     = 11,
    GFW_PIX_UV16    = 12,
    GFW_PIX_COUNT   = 13
};

/* BufferSource, gpu/mod.rs:29-71.  HOST = BufferSource::Cpu{buffer};
 * HIP_DEVICE = the analogue of CUDABuffer{buffer} (a device pointer that
 * already lives in this GPU's HBM). */
enum {
    GFW_BUF_NONE       = 0,
    GFW_BUF_HOST       = 1,
    GFW_BUF_HIP_DEVICE = 2
};

/* BufferDescription, gpu/mod.rs:17-24 */
typedef struct gfw_buffer_desc {
    int32_t width, height, stride;   /* size: (w, h, stride in bytes) */
    int32_t has_rect;                /* Option<(x,y,w,h)> */
    int32_t rect[4];
    int32_t has_rotation;            /* Option<f32>, degrees */
    float   rotation;
    int32_t kind;                    /* GFW_BUF_* */
    int32_t texture_copy;            /* kept for layout parity; unused */
    void   *data;
    size_t  len;                     /* bytes available at data */
} gfw_buffer_desc;

/* Buffers, gpu/mod.rs:25-28 */
typedef struct gfw_buffers {
    gfw_buffer_desc input;
    gfw_buffer_desc output;
} gfw_buffers;

/* Error codes: GyroflowCoreError (src/core/lib.rs:2099-2141) + backend-level
 * conditions that the reference logs-and-skips (opencl.rs:336-358). */
enum {
    GFW_OK                        =  0,
    GFW_ERR_SIZE_TOO_SMALL        = -1,   /* SizeTooSmall          mod.rs:613 */
    GFW_ERR_SIZE_MISMATCH         = -2,   /* SizeMismatch          mod.rs:636-637 */
    GFW_ERR_INVALID_STRIDE        = -3,   /* InvalidStride         mod.rs:639-640 */
    GFW_ERR_NO_STABILIZATION_DATA = -4,   /* NoStabilizationData   mod.rs:721 */
    GFW_ERR_INPUT_BUFFER_EMPTY    = -5,   /* InputBufferEmpty      lib.rs:890 */
    GFW_ERR_OUTPUT_BUFFER_EMPTY   = -6,   /* OutputBufferEmpty     lib.rs:891 */
    GFW_ERR_UNSUPPORTED_BUFFER    = -7,   /* is_buffer_supported == false */
    GFW_ERR_BUFFER_SIZE_MISMATCH  = -8,   /* "Buffer size mismatch" opencl.rs:336-358 */
    GFW_ERR_INVALID_ARGUMENT      = -9,
    GFW_ERR_NO_DEVICE             = -10,  /* no gfx950 device / HIP runtime error */
    GFW_ERR_HIP                   = -11,
    GFW_ERR_UNKNOWN               = -100  /* Unknown */
};

typedef struct gfw_ctx gfw_ctx;

/* ---- device management --------------------------------------------------
 * OclWrapper::list_devices opencl.rs:60, ::set_device :93,
 * ::initialize_context :118, ::get_info (wgpu.rs:123). */
int  gfw_abi_version(void);
/* Writes '\n'-separated device names ("[HIP] <name>") into buf; returns the
 * device count, or a negative GFW_ERR_* */
int  gfw_list_devices(char *buf, size_t cap);
int  gfw_set_device(int index);
int  gfw_get_info(char *buf, size_t cap);
/* is_buffer_supported(): opencl.rs:451 / wgpu.rs:562 */
int  gfw_is_buffer_supported(const gfw_buffers *buffers);

/* ---- backend object -----------------------------------------------------
 * OclWrapper::new(params, ocl_names, distortion_model, digital_lens,
 *                 buffers, drawing_len)              opencl.rs:178
 * The model ids are explicit arguments because FrameTransform leaves
 * KernelParams.distortion_model/digital_lens at their defaults
 * (frame_transform.rs:322-340).  digital_lens = GFW_MODEL_NONE for "None".
 * Owns: the stream, device staging for HOST buffers (sized from `buffers`),
 * matrices (14 * (flags&16 ? width : height) floats), params, mesh
 * (MAX_BUFFER_SIZE = 839 floats, gyro_source/splines.rs:88-89).
 * Returns NULL on failure; see gfw_last_error(). */
gfw_ctx *gfw_create(const gfw_kernel_params *params, int pixel_type,
                    int distortion_model, int digital_lens,
                    const gfw_buffers *buffers, size_t drawing_len);
void     gfw_destroy(gfw_ctx *ctx);

/* OclWrapper::undistort_image(&self, buffers, itm: &FrameTransform, drawing)
 *                                                             opencl.rs:330
 * `matrices` = FrameTransform.matrices flattened ([f32;14] per row,
 * frame_transform.rs:13); host pointer unless GFW_MATRICES_ON_DEVICE is set
 * with gfw_set_option.  Synchronous for HOST buffers (output complete on
 * return, like opencl.rs:413); for HIP_DEVICE buffers the work is enqueued on
 * the context stream and the call returns after enqueue unless the context
 * is in synchronous mode (default: synchronous).
 * Returns GFW_OK or a negative code; never aborts. */
int gfw_undistort_image(gfw_ctx *ctx, const gfw_buffers *buffers,
                        const gfw_kernel_params *params,
                        const float *matrices, int matrix_count,
                        const uint8_t *drawing, size_t drawing_len,
                        const float *mesh, size_t mesh_len);

/* Additive: all planes of one frame in one launch, sharing the per-row
 * matrices and the coordinate evaluation between planes (the reference runs
 * one process_pixels per plane: src/rendering/mod.rs:655-658).  planes[i] /
 * params[i] / pixel_types[i] describe plane i exactly as the i-th
 * gfw_undistort_image call would.  Results are bit-identical to calling
 * gfw_undistort_image once per plane. */
int gfw_undistort_frame(gfw_ctx *ctx, int nplanes,
                        const gfw_buffers *planes,
                        const gfw_kernel_params *params,
                        const int *pixel_types,
                        const float *matrices, int matrix_count,
                        const float *mesh, size_t mesh_len);
/* The frame loop of a render on the library side (the reference drives process_pixels once per frame from
 * rendering/mod.rs:487-547): n_frames frames of one clip — `planes` holds n_frames * nplanes descriptions, frame-major;
 * `params` (nplanes entries) and `pixel_types` are shared by all frames; matrices[f] is frame f's table, with the meaning
 * GFW_OPT_MATRICES_ON_DEVICE gives it.  Frames are warped in order on the context's stream with the results of
 * gfw_undistort_frame; frames with HIP_DEVICE buffers and device-resident tables that share the context's run-time specialised
 * kernel (GFW_OPT_JIT) leave in launches of up to GFW_CLIP_FRAMES_MAX frames, so that the occupancy tail of one frame is
 * filled by the next and the cost differences between image regions average out over the GPU's partitions.  The frames of
 * one launch are in flight together; a frame whose buffers overlap a pending frame's (it writes or reads a destination
 * already in the launch, or writes one of its sources) starts a new launch, so the results are those of the ordered calls.
 * A launch also takes at most 1.1 GB of source + destination (sixteen 4K 16-bit 4:2:2 frames, four 8K ones; at least two
 * frames; environment GFW_CLIP_LAUNCH_MB overrides): past that the frames in flight together cost more than the tail they
 * fill (8K: 9 %), and the call's frames are dealt evenly over the launches it needs (16 under a cap of 4: 4 + 4 + 4 + 4). */
#define GFW_CLIP_FRAMES_MAX 16
int gfw_undistort_clip(gfw_ctx *ctx, int n_frames, int nplanes,
                       const gfw_buffers *planes,
                       const gfw_kernel_params *params,
                       const int *pixel_types,
                       const float *const *matrices, int matrix_count);
/* The same frame loop for a clip whose KernelParams change from frame to frame — FrameTransform::at_timestamp fills them per frame
 * (frame_transform.rs: the adaptive-zoom fov and translation2d, keyframed lens_correction_amount, background_margin and
 * background_margin_feather; the render loop sets GFW_FLAG_FILL_WITH_BACKGROUND per frame, rendering/mod.rs:538-540).
 * `params` holds n_frames * nplanes entries, frame-major like `planes`: frame f's own block per plane; `pixel_types` (nplanes) is shared.
 * Results are bit-identical to n_frames ordered gfw_undistort_frame calls, each given its own frame's params.  Ordering, overlap,
 * synchronous-default, checksum-ring and error behaviour are those of gfw_undistort_clip.  Frames that differ only in fov,
 * lens_correction_amount, translation2d, background_margin / _feather, the fill flag and their matrices share launches; a frame that
 * changes anything else (lens, sizes, a lens-correction amount reaching 1.0, ...) starts a new launch. */
int gfw_undistort_clip_params(gfw_ctx *ctx, int n_frames, int nplanes,
                              const gfw_buffers *planes,
                              const gfw_kernel_params *params,
                              const int *pixel_types,
                              const float *const *matrices, int matrix_count);
/* The same frame loop for a clip whose LENS moves from frame to frame as well — FrameTransform::at_timestamp fills f, c, k[12] and r_limit from
 * get_lens_data_at_timestamp (frame_transform.rs:82-163: the interpolated profile of a zoom lens, the per-frame focal length, principal point and
 * distortion coefficients of Sony / RED / BRAW telemetry), light_refraction_coefficient from a keyframe and mesh_data from mesh_correction[frame].
 * `meshes` is NULL or holds n_frames pointers, frame f's mesh_correction[frame].1 as f32 (NULL: that frame has none); `mesh_lens` is NULL with `meshes`
 * NULL, else the meshes' lengths in floats (0: none; at most 839).  Every mesh is validated on the host before anything is staged or launched;
 * consecutive frames that name the same pointer and length share one validation and one upload.
 * Results are bit-identical to n_frames ordered gfw_undistort_frame calls, each given its own frame's params and mesh.  Ordering, overlap,
 * synchronous-default, checksum-ring, launch-size and error behaviour are those of gfw_undistort_clip_params.  Frames share launches when they differ
 * only in what that call lets move, in f, c, k[0..11], r_limit, light_refraction_coefficient and in the CONTENTS of their meshes; a frame that differs
 * in anything the kernel is compiled for (sizes, strides, pixel types, lens model ids, interpolation, background mode, stretches, rotation, whether a
 * mesh is present, whether refraction is on, whether k[0..3] are all zero, ...) starts a new launch.  These launches take the exact first pass.  A frame
 * the fused kernel does not serve (a mesh with input_rotation, EWA, host buffers) goes out on its own behind the pending ones, as gfw_undistort_frame
 * would send it.  A call in which none of the lens fields moves and no frame has a mesh IS gfw_undistort_clip_params.
 * Rejected before any output is touched or anything enqueued, gfw_last_error() naming the frame: negative counts, mesh_lens without meshes (or the
 * reverse), a length with a NULL pointer (GFW_ERR_INVALID_ARGUMENT); a length above 839, a malformed mesh header (GFW_ERR_BUFFER_SIZE_MISMATCH). */
int gfw_undistort_clip_lens(gfw_ctx *ctx, int n_frames, int nplanes,
                            const gfw_buffers *planes,
                            const gfw_kernel_params *params,
                            const int *pixel_types,
                            const float *const *matrices, int matrix_count,
                            const float *const *meshes,
                            const size_t *mesh_lens);

/* ---- options / stream ---------------------------------------------------*/
enum {
    GFW_OPT_SYNCHRONOUS        = 1,  /* 1 (default): return after stream sync */
    GFW_OPT_MATRICES_ON_DEVICE = 2,  /* 0: host rows of [f32;14] (default, uploaded per call like opencl.rs:406);
                                        1: device pointer, rows of [f32;14]; 2: device pointer, rows of 16 floats as
                                        written by gfw_pack_matrices (no per-call work at all).  With 1 and 2 the
                                        library cannot scan the rows, so the IBIS/OIS terms m[9..13] are honoured only if
                                        GFW_FLAG_HAS_IBIS_DATA is set in params->flags (get_kernel_flags, mod.rs:226-251,
                                        sets it for every clip that has such data); with 1 the roll's cos/sin are
                                        evaluated on the device with the host libm's own routines (gfw_math.h). */
    GFW_OPT_KERNEL_VARIANT     = 3,  /* (further values: gfwarp_testing.h)  0 auto; 1 generic per-plane kernel; 2 fused kernel with the exact first pass;
                                        3 fused kernel, certified first pass in audit mode (see gfw_get_audit); 4 the same with the first pass evaluated
                                        per pixel (the form of rounds 2-4; by default a frame takes the lattice form where its certificate allows).
                                        Every variant produces the same pixels; any other value is rejected (GFW_ERR_INVALID_ARGUMENT) */
    GFW_OPT_PROFILE            = 4,  /* 1: bracket every warp-kernel launch with hipEvents on the context stream */
    GFW_OPT_TUNE_ROWS          = 5,  /* reserved (ignored) */
    GFW_OPT_TUNE_GRID          = 6,  /* tuning: persistent workgroups of the fused kernel (0 = 6 per CU) */
    GFW_OPT_JIT                = 7,  /* per-clip specialised kernel, compiled at run time the way the reference compiles its OpenCL source per clip
                                        (opencl.rs:181-214): 0 never; 1 (default) built in the background once the context has warped three
                                        frames with the same clip constants, frames run ahead-of-time until it is ready; 2 built at the first
                                        frame, which waits for it (~1 s).  Same results bit for bit; the environment variable GFW_JIT sets
                                        the default of new contexts.  Without libhiprtc.so the option has no effect. */
    GFW_OPT_COALESCE_PLANES    = 8,  /* the planes of a frame that arrive one per gfw_undistort_image call — the reference's render loop issues
                                        process_pixels once per plane, each plane through its own Stabilization / backend object
                                        (src/rendering/mod.rs:494-545) — leave as ONE fused launch.  Applies to calls that are stream-ordered anyway:
                                        GFW_OPT_SYNCHRONOUS = 0 (or GFW_OPT_FRAME_SYNC), HIP_DEVICE buffers on both sides.  Such a call validates its
                                        arguments, keeps a copy and returns; the frame is enqueued on the stream of the context that took plane_index 0
                                        when its last plane arrives — a UV8 / UV16 plane, the third Luma plane, the fourth R32f plane — or when anything
                                        else is asked of a member context (gfw_synchronize, gfw_flush, gfw_get_stream, an option, a plane that does not
                                        continue the frame, gfw_destroy).
                                        1 (default): only calls on contexts that have been SEEN as planes of a multi-plane frame are held (a call with
                                        plane_index k + 1 following, on the same thread, a call with plane_index k on another context of the same device,
                                        lens and matrix count): a clip's first frame leaves plane by plane, a lone greyscale / float plane is never held.
                                        2: every eligible call is held from the first frame on.  0: every call launches its own plane.
                                        ORDERING CONTRACT: the fused launch waits for everything that was enqueued on EACH member context's stream before
                                        the frame was completed (a plane's upload or decode, a consumer still reading its destination), and every member's
                                        stream is ordered behind the launch.  Observe completion through gfw_synchronize / gfw_flush / gfw_get_stream of
                                        any member context (or events recorded after them).  Results are bit-identical to the per-plane launches. */
    GFW_OPT_COALESCE_FRAMES    = 9,  /* frames assembled by GFW_OPT_COALESCE_PLANES that are held for one launch of the run-time specialised kernel
                                        (1..GFW_CLIP_FRAMES_MAX; default 1: a frame leaves when it is complete).  Larger values trade latency for the
                                        throughput of gfw_undistort_clip (the occupancy tail of one frame filled by the next).  Ignored by a
                                        synchronous owner (GFW_OPT_FRAME_SYNC). */
    GFW_OPT_FRAME_SYNC         = 10  /* 0 (default).  1: on a SYNCHRONOUS context (GFW_OPT_SYNCHRONOUS = 1, the reference's contract: opencl.rs:413) with
                                        HIP_DEVICE buffers, "complete on return" is relaxed to "the FRAME is complete when its LAST plane's call returns":
                                        the calls of the frame's earlier planes validate, are held (GFW_OPT_COALESCE_PLANES) and return at once, the last
                                        plane's call launches the fused kernel and waits for it.  This is what the render loop needs — it consumes a
                                        frame's planes only after all of its process_pixels calls (rendering/mod.rs:494-545) — but it is NOT what a caller
                                        that reads plane 0 right after plane 0's call gets; hence opt-in, on every context of the frame. */
};
int   gfw_set_option(gfw_ctx *ctx, int option, int64_t value);
/* Enqueues whatever gfw_undistort_image calls GFW_OPT_COALESCE_PLANES / _FRAMES are holding for a frame or launch this context belongs to
 * (no-op otherwise).  Does not wait for the GPU: gfw_synchronize does both. */
int   gfw_flush(gfw_ctx *ctx);
/* hipStream_t the context enqueues on (as void*); caller may substitute its
 * own stream (e.g. the decoder's) — mirrors passing the cl_command_queue in
 * BufferSource::OpenCL{queue} (gpu/mod.rs:37-40). */
void *gfw_get_stream(gfw_ctx *ctx);
/* Drains the stream in use (hipStreamSynchronize), then adopts `hip_stream` (not owned; NULL = the legacy default stream). */
int   gfw_set_stream(gfw_ctx *ctx, void *hip_stream);
int   gfw_synchronize(gfw_ctx *ctx);
/* Name of the kernel path the last call took ("plane_generic", "yuv_fused", ...):
 * the analogue of ProcessedInfo.backend (stabilization/mod.rs:194-200). */
const char *gfw_last_backend(gfw_ctx *ctx);
/* State of the context's run-time specialised kernel: 0 none / not available, 1 compiling, 2 ready (in use), 3 failed (frames keep
 * running ahead-of-time).  compile_ms and the compiler log (truncated to cap) are optional outputs. */
int   gfw_jit_status(gfw_ctx *ctx, double *compile_ms, char *log, size_t cap);

/* With GFW_OPT_PROFILE on: accumulated warp-kernel time (ms, hipEventElapsedTime on the context stream)
 * and launch count since the last reset; synchronises the stream.  reset != 0 clears the accumulators. */
int   gfw_get_profile(gfw_ctx *ctx, double *kernel_ms, int64_t *launches, int reset);
/* the same, plus the number of frames the bracketed launches covered (a gfw_undistort_clip launch carries up to GFW_CLIP_FRAMES_MAX) */
int   gfw_get_profile_frames(gfw_ctx *ctx, double *kernel_ms, int64_t *launches, int64_t *frames, int reset);

/* Thread-local, human-readable description of the last failure. */
const char *gfw_last_error(void);

/* Host helper: FrameTransform.matrices rows ([f32;14]) -> libgfwarp's 64-byte device row layout
 * (m0..m13, cosf(-m11), sinf(-m11) evaluated with the host libm as cpu_undistort.rs:159-160 does).  A pipeline that
 * knows its FrameTransforms ahead of time packs them once, keeps them in HBM and passes the device pointer with
 * GFW_OPT_MATRICES_ON_DEVICE = 2. */
int   gfw_pack_matrices(const float *rows14, int count, float *rows16);

/* ---- decoder / interop surfaces without the host ("next" row f-4) ----
 * The reference's zero-copy path imports memory another API owns and maps it to a device pointer of the compute API
 * (src/core/gpu/wgpu_interop_cuda.rs:181-215: cuImportExternalMemory -> cuExternalMemoryGetMappedBuffer; plane descriptors
 * src/rendering/zero_copy.rs:67-112; BufferSource::CUDABuffer, src/core/gpu/mod.rs:67-70).  gfw_import_external_fd does the same for a POSIX
 * file descriptor that names a device allocation (a dma-buf exported by the decoder / VA-API / Vulkan, or another process's
 * hipMemExportToShareableHandle): `*dev_ptr_out` is a device pointer to `size` bytes, to be used in GFW_BUF_HIP_DEVICE buffer descriptions —
 * plane offsets and the row pitch are the caller's (`data + offset`, `stride`).  `drm_format_modifier` states the surface layout: only
 * DRM_FORMAT_MOD_LINEAR (0) can be warped in place, anything else returns GFW_ERR_UNSUPPORTED_BUFFER.  The caller keeps its fd.
 * gfw_release_external unmaps (after the device has drained). */
typedef struct gfw_external gfw_external;
int   gfw_import_external_fd(int fd, size_t size, unsigned long long drm_format_modifier, void **dev_ptr_out, gfw_external **handle_out);
int   gfw_release_external(gfw_external *handle);

/* Verification helper for frame-sharded clip runs (no reference counterpart; SURVEY.md 8e: one 8-byte checksum per frame,
 * all-gathered across ranks): adds the sum of the u64 words of a device buffer (mod 2^64) to *d_out, enqueued in order
 * on the context's stream.  `bytes` a multiple of 8, `d_buf` 16-byte aligned, `d_out` a zero-initialised device word. */
int   gfw_checksum64(gfw_ctx *ctx, const void *d_buf, size_t bytes, unsigned long long *d_out);
/* The same checksum taken WHERE THE PIXELS LEAVE: from this call on, frame k submitted on the context (k = 0, 1, ...: a gfw_undistort_frame call, a frame of
 * gfw_undistort_clip, a frame assembled from coalesced gfw_undistort_image calls, a lone gfw_undistort_image call) adds the checksum of every byte it WRITES —
 * the byte times 256^(its address mod 8), modulo 2^64: what gfw_checksum64 of a zero-initialised destination holds afterwards — to d_sums[k mod count], in
 * order on the context's stream.  `d_sums`: `count` device words the caller zeroed; NULL or count = 0 turns it off.  A specialised fused kernel takes the sum in
 * its store path (no second pass over the output: 33 MB per C2 frame, 11 us); every other kernel is followed by a pass over the written region — same value.
 * HIP_DEVICE outputs only (GFW_ERR_INVALID_ARGUMENT from the frame's call otherwise). */
int   gfw_set_frame_checksums(gfw_ctx *ctx, unsigned long long *d_sums, size_t count);

/* ---- per-row matrices on the device ("next" row: FrameTransform::at_timestamp, frame_transform.rs:221-308) ----
 * gfw_set_quaternion_tracks uploads the clip's original and smoothed orientation tracks once
 * (GyroSource.quaternions / smoothed_quaternions: BTreeMap<i64 timestamp_us, Quat64>, gyro_source/mod.rs:857-882);
 * gfw_build_matrices then produces the packed rows of one frame directly in HBM (device pointer `rows16_out`, or a
 * context-owned table when NULL; its address is returned through `*out_ptr`) to be passed to
 * gfw_undistort_image/frame with GFW_OPT_MATRICES_ON_DEVICE = 2.  Results equal the host f64 statement to ~1 ULP of f32
 * (SVD vs closed-form inverse).  gfw_set_sync_offsets adds the clip's gyro/video sync offsets, gfw_build_matrices_stab the
 * IBIS/OIS terms, gfw_frame_timing.suppress_rotation the `suppress_rotation` switch: with them FrameTransform::at_timestamp's
 * matrix loop (frame_transform.rs:249-308) is covered in full. */
typedef struct gfw_frame_timing {
    double timestamp_ms;               /* frame centre */
    double per_frame_time_offset_ms;   /* file_metadata.per_frame_time_offsets[frame] */
    double frame_readout_time_ms;      /* signed, as get_frame_readout_time returns it */
    double new_k[9];                   /* get_new_k(), row-major (frame_transform.rs:37-51) */
    double video_rotation_deg;
    int32_t rows;                      /* matrix_count: H, W (horizontal readout) or 1 */
    int32_t readout_dim;               /* divisor of the row readout time: height, or width for horizontal readout */
    int32_t framebuffer_inverted;
    int32_t suppress_rotation;         /* 0; 1 = params.suppress_rotation (R = identity, frame_transform.rs:291-296);
                                          2 = the same with params.frame_readout_time == 0.0 (the IBIS/OIS terms are zeroed too).
                                          MUST be set (zero-initialise the struct): until GFW_ABI_VERSION 1 this slot was padding;
                                          any other value is rejected with GFW_ERR_INVALID_ARGUMENT */
} gfw_frame_timing;
/* file_metadata.camera_stab_data[frame] (gyro_source/file_metadata.rs:41-48): in-body / optical stabiliser positions along the
 * sensor readout, as two Catmull-Rom splines of the sensor row.  frame_transform.rs:234-241 and :270-289 turn them into
 * the per-row terms m[9..13] = (sx, sy, roll angle, ox, oy); gfw_build_matrices_stab evaluates them per row on the device
 * (f64, the reference's operation order) and fills the roll's cos/sin slots with the host libm's routines (gfw_math.h). */
typedef struct gfw_frame_stab {
    double offset;                     /* CameraStabData.offset */
    double sensor_size[2];             /* (u32, u32) */
    double crop_area[4];               /* (f32 x, y, w, h) widened exactly */
    double pixel_pitch[2];             /* (u32, u32) */
    double width, height;              /* params.width, params.height */
    int32_t ibis_count, ois_count;     /* control points of the two splines (ascending positions) */
    const double *ibis;                /* host, ibis_count x 4: position, x, y, z */
    const double *ois;                 /* host, ois_count x 4: position, x, y, z (z unused) */
} gfw_frame_stab;
int   gfw_set_quaternion_tracks(gfw_ctx *ctx, const int64_t *org_ts_us, const double *org_wxyz, int org_count,
                                const int64_t *smoothed_ts_us, const double *smoothed_wxyz, int smoothed_count);
int   gfw_build_matrices(gfw_ctx *ctx, const gfw_frame_timing *timing, float *rows16_out, float **out_ptr);
/* The same with the frame's IBIS/OIS stabiliser data (`stab` may be NULL): rows carry m[9..13] and cos/sin(-m[11]). */
int   gfw_build_matrices_stab(gfw_ctx *ctx, const gfw_frame_timing *timing, const gfw_frame_stab *stab, float *rows16_out, float **out_ptr);
/* Gyro/video synchronisation of the clip (GyroSource.offsets_adjusted: BTreeMap<i64 timestamp_us, f64 offset_ms> and
 * duration_ms): quat_at_timestamp subtracts offset_at_video_timestamp(t) from every lookup time — per row, since the offset is
 * interpolated at the row's own time — and returns identity when duration_ms <= 0 (gyro_source/mod.rs:857-860, :884-908).
 * Not calling this leaves no offsets and a positive duration.  `count` may be 0. */
int   gfw_set_sync_offsets(gfw_ctx *ctx, double duration_ms, const int64_t *timestamps_us, const double *offsets_ms, int count);
/* The tables of `count` (<= 64) upcoming frames in one launch, in order on the context's stream, into context-owned
 * memory (two batches alternate: a batch stays valid until the second next call).  out_ptrs[i] = device table of frame i,
 * to be passed as `matrices` with GFW_OPT_MATRICES_ON_DEVICE = 2.  Amortises the builder's latency and needs no
 * cross-stream synchronisation: the per-frame cost in a render loop drops to ~1 us of GPU time. */
int   gfw_build_matrices_batch(gfw_ctx *ctx, const gfw_frame_timing *timings, int count, float **out_ptrs);
/* The same for a clip with IBIS/OIS splines: stabs[i] is frame i's camera_stab_data entry or NULL (stabs itself may be NULL: no
 * frame has one).  Frame i's table equals gfw_build_matrices_stab(ctx, &timings[i], stabs[i], ...)'s bit for bit.  The control
 * points of all frames travel in one pinned staging copy in front of the launch; limits, ordering, the two alternating batches
 * and the error codes are gfw_build_matrices_batch's, and a rejected frame is named in gfw_last_error(). */
int   gfw_build_matrices_batch_stab(gfw_ctx *ctx, const gfw_frame_timing *timings, const gfw_frame_stab *const *stabs,
                                    int count, float **out_ptrs);

/* ---- STMap coordinate export ("next" row: src/core/stmap.rs:87-109, :127-137) ----------------------------
 * The "undist" ST map: for every pixel (x, y) of a width x height map, the rolling-shutter row pick followed by
 * rotate_and_distort, written as two f32 (source x, y in pixels) instead of being sampled.  `params` is the
 * KernelParams stmap.rs builds (width/height/output_* = map size, flags = HAS_DIGITAL_LENS | HORIZONTAL_RS).
 * Pixels whose projection is None are left untouched (parallel_exr leaves them 0).  Bit-exact vs the CPU closure.
 * matrix_count may not exceed the rows of the plane the context was created for (its height; its width under a horizontal
 * rolling shutter) — GFW_ERR_BUFFER_SIZE_MISMATCH, "Buffer size mismatch matrices!", nothing written — so a per-row map larger
 * than the source (stmap.rs sizes the undist map new_width x new_height) needs a context created at the map's size. */
int   gfw_stmap_undistort(gfw_ctx *ctx, const gfw_kernel_params *params, const float *matrices, int matrix_count,
                          const float *mesh, size_t mesh_len, int width, int height, float *coords, int coords_on_device);

/* ---- inverse point map ("next" row 3: cpu_undistort.rs:652-858 `undistort_points`; stmap.rs:123-127 "dist") ----
 * Source-image points -> stabilised output coordinates.  The STMap "dist" pass and the optical-flow caller
 * (cpu_undistort.rs:643-650) run it with lens_correction_amount == 1; with params->lens_correction_amount < 1 the
 * Newton inverse of the render's lens-correction blend follows (:785-851, what the zoom search uses), with
 * params->fov as its `fov`.  The lens / digital-lens models are the ones given to gfw_create.
 *   params     the KernelParams undistort_points builds (:669-681: width/height/output_*, f, c, k,
 *              digital_lens_params, light_refraction_coefficient) with input_*_stretch = lens.input_*_stretch (:704-705)
 *   points     n x 2 f32 (host), or NULL = the pixel grid parallel_exr walks: point i = (i % grid_width, i / grid_width)
 *   rotations  [rotation_count][9] row-major f32 = nalgebra::convert::<f64,f32> of `new_k * R` per point
 *              (FrameTransform::at_timestamp_for_points, frame_transform.rs:391-410)
 *   shifts     NULL, or [rotation_count][5] = (sx, sy, angle_rad, ox, oy) (frame_transform.rs:412-440)
 *   index_mode which rotation/shift row a point uses: GFW_POINT_INDEX_SINGLE (row 0: no rolling shutter),
 *              _PER_POINT (row i), _PER_ROW (grid y; vertical rolling shutter), _PER_COLUMN (grid x; horizontal);
 *              an index past rotation_count falls back to row 0 as `rot_per_point.get(index).unwrap_or(&rr)` does
 *   mesh       NULL, or the f64 lens mesh `undistort_points` receives (:714-753)
 *   out        n x 2 f32, host or device memory (out_on_device); (-1e6, -1e6) where the lens inverse is None (:855)
 * Bit-exact vs the CPU statement.  Synchronous. */
enum { GFW_POINT_INDEX_SINGLE = 0, GFW_POINT_INDEX_PER_POINT = 1, GFW_POINT_INDEX_PER_ROW = 2, GFW_POINT_INDEX_PER_COLUMN = 3 };
int   gfw_undistort_points(gfw_ctx *ctx, const gfw_kernel_params *params, const float *points, size_t n, int grid_width,
                           const float *rotations, int rotation_count, const float *shifts, int index_mode,
                           const double *mesh, size_t mesh_len, float *out, int out_on_device);

/* ---- adaptive zoom: the per-frame FOV search of a whole clip in one device call (src/core/zooming/) ----
 * calculate_fovs (zooming/mod.rs:35-70) = FovIterative::find_fov per frame (fov_iterative.rs:91-134), then zoom_dynamic::compute.
 * gfw_zoom_fovs is the first half on the device, one workgroup per frame: the 120-point outline of the source frame
 * (points_around_rect(w, h, 31, 31) with fov_algorithm_margin, :154-175) goes through undistort_points_with_rolling_shutter —
 * per point the rotation of at_timestamp_for_points (frame_transform.rs:376-410: always the four sign flips of :402-403,
 * whatever framebuffer_inverted says) and the inverse point map of gfw_undistort_points — the zoom centre is subtracted
 * (:99-102), nearest_edge (:136-151) folds the points in index order, and up to four refinement rounds (:110-131) follow,
 * restated as written: `rect[idx]` is indexed with the index into the polygon folded last (the 63-point one from the second
 * round on), `idx.overflowing_sub(1).0 % len` makes rect[15] the left neighbour of rect[0], and a round whose second fold
 * accepts nothing is followed by one more fold of the same 63 points before the loop ends.
 *   params     the KernelParams undistort_points builds (:671-683) with input_*_stretch, as for gfw_undistort_points, for the
 *              ComputeParams calculate_fovs patches (mod.rs:40-49: output size = source size); lens_correction_amount and fov
 *              are NOT read from it but from each frame's descriptor
 *   frames     one gfw_zoom_frame per frame (host memory)
 *   rotations  NULL = rotations from the tracks of gfw_set_quaternion_tracks / gfw_set_sync_offsets; or [n_frames][9] f32 =
 *              one `new_k * R` per frame given by the caller (no track is read; every frame_readout_time_ms must be 0): the
 *              form whose result is bit-exact against the CPU statement.  From tracks the f64 acos / sin of the slerp are the
 *              device library's: a rotation entry can differ from the host's in its last f32 bits (as for gfw_build_matrices).
 *   fov_minimal   n_frames f64: (nearest.1.0 * 2.0 / output_dim.0) as f64, host or device memory (out_on_device)
 *   debug_points  NULL, or [n_frames][120][2] f64 in the same memory space: the first round's mapped outline after the centre
 *              offset, divided by the input size (zooming_debug_points, :103-105)
 * One launch, in order on the context's stream; with device outputs an asynchronous context returns without waiting.  n_frames = 0 succeeds and writes nothing.
 * NOT covered, rejected with GFW_ERR_INVALID_ARGUMENT: clips with per-frame IBIS/OIS shifts (frame_transform.rs:412-435) or a
 * lens mesh / focal-plane distortion data (params->flags has HAS_IBIS_DATA, HAS_MESH_DATA or HAS_FPD_DATA): such a clip keeps
 * mapping its outline with gfw_undistort_points — or calls gfw_zoom_fovs_stab below. */
typedef struct gfw_zoom_frame {
    double timestamp_ms;               /* frame centre */
    double per_frame_time_offset_ms;   /* file_metadata.per_frame_time_offsets[frame] */
    double frame_readout_time_ms;      /* signed, get_frame_readout_time(can_invert = false) */
    double new_k[9];                   /* get_new_k(patched params, camera_matrix, fov), row-major */
    double fov;                        /* get_fov(use_fovs = false) * focal-length compensation: the lens-correction blend's fov */
    double video_rotation_deg;
    double zoom_center[2];             /* adaptive_zoom_center_offset, or its keyframed value at the frame (fov_iterative.rs:41-57) */
    double lens_correction_amount;     /* lens_correction_amount, or its keyframed value */
    int32_t suppress_rotation;         /* 0 or 1; gfw_zoom_fovs_stab also takes 2 = 1 with params.frame_readout_time == 0.0: the frame's
                                          shifts are dropped (frame_transform.rs:433-435), as in gfw_frame_timing */
    int32_t reserved;                  /* 0 */
} gfw_zoom_frame;
typedef struct gfw_zoom_search {
    int32_t width, height;             /* compute_params.width / height (input_dim) */
    int32_t org_output_width, org_output_height;   /* the output size before calculate_fovs patches it; both >= 1 (0 is rejected: the reference divides by it) */
    float   fov_algorithm_margin;
    int32_t horizontal_readout;        /* 1: a point's x picks its time and the row readout time is frame time / width */
} gfw_zoom_search;
int   gfw_zoom_fovs(gfw_ctx *ctx, const gfw_kernel_params *params, const gfw_zoom_search *search,
                    const gfw_zoom_frame *frames, int n_frames, const float *rotations,
                    double *fov_minimal, double *debug_points, int out_on_device);
/* The search for clips with in-body / optical stabiliser data (file_metadata.camera_stab_data) and a per-frame lens mesh
 * (file_metadata.mesh_correction): at_timestamp_for_points' shifts (frame_transform.rs:412-435) and undistort_points' mesh and
 * focal-plane-distortion steps (cpu_undistort.rs:712-760) per outline point, in the same single launch.
 *   stabs      NULL, or [n_frames] pointers: camera_stab_data.get(frame), NULL = None.  A present entry whose splines cannot be
 *              evaluated gives a shift of zeros, which is NOT the same as no shift (the shift's arithmetic rounds).  The scale is
 *              width / crop_w / pitch_x, height / crop_h / pitch_y — no framebuffer sign, no sensor-height flip: those belong to
 *              the matrix path — the spline position map_coord(y, 0, height, crop_y, crop_y + crop_h) + offset with the
 *              point's own y (under horizontal readout too), the roll (z / 1000).to_radians() as f32, cos / sin of +angle.
 *              A frame with rolling shutter shifts every point of the outline and of each refinement; a frame without has ONE
 *              shift, evaluated at y = 0, and shift_per_point.get(index) hands it to point 0 of each mapped set only — as written.
 *   meshes / mesh_lens   NULL, or [n_frames]: mesh_correction[frame].0 (the DISTORTING mesh, f64) and its length (0 = none; at
 *              most 839).  Consecutive frames naming the same pointer and length share one validation and one upload.
 *   params->flags   HAS_IBIS_DATA / HAS_MESH_DATA / HAS_FPD_DATA are accepted and not consulted: the data decides, as on the
 *              reference's CPU path.
 * Everything else — rotations (caller-given ones still require every readout time to be 0), outputs, ordering — is
 * gfw_zoom_fovs's; with stabs and meshes NULL the call IS gfw_zoom_fovs (same kernels, same bits).  Rejected with
 * GFW_ERR_INVALID_ARGUMENT and the frame named in gfw_last_error(), outputs untouched: negative counts, a count without its
 * array, descending spline positions, zero crop or pitch, a mesh that is NULL, longer than 839 values or inconsistent with its
 * own header, suppress_rotation outside 0..2. */
int   gfw_zoom_fovs_stab(gfw_ctx *ctx, const gfw_kernel_params *params, const gfw_zoom_search *search,
                         const gfw_zoom_frame *frames, int n_frames, const float *rotations,
                         const gfw_frame_stab *const *stabs, const double *const *meshes, const size_t *mesh_lens,
                         double *fov_minimal, double *debug_points, int out_on_device);
/* The second half, on the host in f64 with the reference's operation order (zooming/mod.rs:55-68, zoom_dynamic.rs); needs no
 * context and no GPU.  adaptive_zoom_window < -0.9: static zoom (every fov = the minimum); > 0.0001: dynamic zoom over
 * frames = floor(window * scaled_fps) made odd — method 0 Gaussian filter (pad_edge, min_rolling, pad_edge, convolve with the
 * normalised Gaussian window of sigma frames / 6), method 1 envelope follower (two passes, the second with a 0.2 s constant;
 * any other method is the Gaussian filter, as ZoomMethod::from); otherwise 1.0 everywhere.  trim_ranges: n_ranges pairs
 * (start, end) as fractions of the clip (fov_iterative.rs:59-69), applied to fov_minimal first: frames outside every range get
 * the maximum.  fovs_out and fov_minimal_out (the series after the trim ranges; may be NULL) hold n values each.
 * The keyframed-window branch (zoom_dynamic.rs:22-55: ZoomingSpeed keyframes, video speed) is not covered. */
int   gfw_zoom_smooth(const double *fov_minimal, int n, double adaptive_zoom_window, double scaled_fps, int method,
                      const double *trim_ranges, int n_ranges, double *fovs_out, double *fov_minimal_out);

/* ---- synchronization: the visual-features offset / readout-time search of a range in one device call ----
 * find_offset/visual_features.rs:10-147.  A range has matched frame pairs ((ts, points), (next_ts, points)); calculate_distance
 * (:49-83) of a candidate (offset_ms, frame_readout_time_ms) maps both point sets of every pair through
 * undistort_points_with_rolling_shutter at `ts_us as f64 / 1000.0 - offset` (per point the rotation of at_timestamp_for_points,
 * frame_transform.rs:376-410, with per_frame_time_offset 0 and the readout time of the candidate — negative and zero included:
 * |readout| > 0 decides rolling, otherwise ONE rotation at ts - readout / 2 serves every point — and the inverse point map of
 * gfw_undistort_points with lens_correction_amount 1.0), keeps a point pair when both mapped points lie strictly inside
 * (0, w) x (0, h), takes `dist as u64` of the f32 squared distance, and adds the k = (n_valid as f64 * 0.9) as usize smallest of
 * each pair.  Costs are sums of integers, far below 2^53: the device adds them as u64 and converts once, which equals the
 * reference's sequential f64 adds; given the mapped points a cost is exact.
 *   params     the KernelParams undistort_points builds, as for gfw_undistort_points; lens_correction_amount and fov are not read
 *   search     what the candidates share (below); rotations come from the tracks of gfw_set_quaternion_tracks, and with
 *              use_sync_offsets = 1 from gfw_set_sync_offsets as well (for_rs keeps the offsets, the offset search clears them)
 *   pair_ts_us [n_pairs][2] the two timestamps of a pair; pair_first [n_pairs + 1] ascending: pair p owns the points
 *              pair_first[p] .. pair_first[p + 1] - 1 of points_a (first frame) and points_b (second frame), [total][2] f32,
 *              source-image pixels; at most 4096 points in a pair, at most 65535 pairs; a pair of 0 points contributes 0
 *   candidates [n_candidates][2] f64 (offset_ms, frame_readout_time_ms), host memory
 *   costs      [n_candidates] f64; mapped NULL or [n_candidates][total][2][2] f32: p1 and p2 of every point pair as mapped
 *              ((-1e6, -1e6) where the lens inverse is None); both host or both device memory (out_on_device)
 * n_pairs = 0: every cost is 0.  n_candidates = 0 succeeds and writes nothing.
 * gfw_sync_visual_search is the two-stage search of one range (:87-131) without a host round trip — lens stage, coarse costs,
 * reduce + pick, fine costs of the 200 candidates `lowest.0 - 1.0 + i * 0.01` generated on the device, reduce + pick:
 *   mode 0     offset: search_size_ms as usize candidates initial_offset + (-(search_size / 2.0) + i), the given readout time
 *   mode 1     readout time (for_rs): steps = (1000.0 / scaled_fps) as isize, candidates i in -steps..steps, offset 0
 * `reduce_with(find_min)` with `if a.1 < b.1 { a } else { b }`: of equal minimal costs the LAST candidate wins, in both stages.
 *   result     found = 0 when the coarse stage has no candidates (then nothing else is meaningful); n_coarse; the coarse pick
 *              and its cost; value / cost: the fine pick (an offset_ms or a readout time in ms)
 *   coarse_costs / fine_costs   NULL or [n_coarse] / [200] f64; with result host or device memory (out_on_device)
 * The 90 %-of-range acceptance rule (:137) and the range's middle timestamp are the caller's (gyroflow::find_offsets_visual,
 * gyroflow_amd.synchronization).  Both calls run in order on the context's stream; with device outputs an asynchronous context
 * returns without waiting.  Rejected with GFW_ERR_INVALID_ARGUMENT, the pair named in gfw_last_error(), outputs untouched:
 * negative counts, a descending pair_first, more than 4096 points in a pair, width^2 + height^2 >= 2^32, params->flags with
 * HAS_IBIS_DATA, HAS_MESH_DATA or HAS_FPD_DATA, a non-zero reserved slot, no tracks.
 * NOT covered: clips with per_frame_time_offsets, camera_stab_data or mesh_correction (in the reference the frame index, and so
 * the mesh, follows `timestamp - offs`); lens data or a video rotation keyframed inside a range; suppress_rotation; AKAZE
 * (pyramidal Lucas-Kanade optical flow: gfw_flow_pyrlk below; its corner detection: gfw_corners_shi_tomasi below).  (essential_matrix: gfw_sync_gyro_search below; rs_sync: gfw_sync_rs_search below; optimsync: gfw_sync_optim_points below; pose estimation by the
 * Almeida method: gfw_pose_almeida below; by an essential matrix, pose methods 0 and 2: gfw_pose_essential below.) */
typedef struct gfw_sync_search {
    int32_t width, height;            /* params.width / height: the bounds test (`w as f32`) and the readout divisor */
    int32_t horizontal_readout;
    int32_t use_sync_offsets;         /* 0 = clear_offsets() (visual_features.rs:13-15: the offset search); 1 = keep the context's (for_rs) */
    double  new_k[9];                 /* get_new_k(params, camera_matrix, get_fov(use_fovs = false)), row-major */
    double  video_rotation_deg;
    int32_t reserved[2];              /* 0 */
} gfw_sync_search;
typedef struct gfw_sync_result { int32_t found, n_coarse; double coarse_value, coarse_cost, value, cost; } gfw_sync_result;
int   gfw_sync_visual_costs(gfw_ctx *ctx, const gfw_kernel_params *params, const gfw_sync_search *search,
                            const int64_t *pair_ts_us, const int32_t *pair_first, const float *points_a, const float *points_b, int n_pairs,
                            const double *candidates, int n_candidates, double *costs, float *mapped, int out_on_device);
int   gfw_sync_visual_search(gfw_ctx *ctx, const gfw_kernel_params *params, const gfw_sync_search *search,
                             const int64_t *pair_ts_us, const int32_t *pair_first, const float *points_a, const float *points_b, int n_pairs,
                             int mode, double initial_offset_ms, double search_size_ms, double frame_readout_time_ms, double scaled_fps,
                             gfw_sync_result *result, double *coarse_costs, double *fine_costs, int out_on_device);

/* ---- synchronization: the gyro-match offset search of all ranges of a clip in one device call ----
 * find_offset/essential_matrix.rs:13-131: offset method 0, and the fast initial offset of rs-sync (rs_sync.rs:26-45).  Per range the
 * angular rates pose estimation produced (estimated samples) are matched against the gyro's rates at `timestamp - offset`:
 * calculate_cost (:109-131) looks every estimated sample up in a BTreeMap of the range's gyro samples keyed by
 * `(timestamp_ms * 1000.0) as usize` (truncating, saturating, NaN and negatives -> 0; a later sample replaces an earlier one with the
 * same key) — the first key at or above `((o.timestamp_ms - offs) * 1000.0) as usize`: a negative query lands on the first sample, a
 * query past the last key is a miss.  A hit whose gyro is None, or an estimated sample whose gyro is None, is no match (and nothing
 * else is looked at for that sample).  Per match three separate f64 additions, (g0-o0)^2 * 70, (g1-o1)^2 * 70, (g2-o2)^2 * 100; the
 * cost is sum / matches when the range has samples and matches > len / 2 (integer division), f64::MAX otherwise.  A lane of the
 * device is a candidate and folds the samples in index order: a cost equals the reference's sequential f64 fold to the bit.
 *   est_first  [n_ranges + 1] ascending: range r owns the estimated samples est_first[r] .. est_first[r + 1] - 1 of
 *              est [n_est][4] f64 (timestamp_ms, x, y, z) and est_has [n_est] (0 = `gyro: None`; a NULL est_has = all present)
 *   gyro_first / gyro / gyro_has / n_gyro   the same for the gyro samples of each range, already cut to the range's window and
 *              filtered (:31-38, :48: the caller's work — gyroflow::find_offsets_essential, gyroflow_amd.synchronization); a range's
 *              slice need not be ascending: the sorted, de-duplicated key array is built while staging
 *   limits     at most 65535 ranges, 65536 estimated samples and 2^22 gyro samples a range, 2 000 000 candidates a range
 *              (search_size_ms <= 10^6), 2 GiB staged in all
 * gfw_sync_gyro_costs: calculate_cost of caller-given candidate offsets (ms): range r owns candidates cand_first[r] ..
 * cand_first[r + 1] - 1 of candidates [n_candidates], and the same entries of costs (host or device memory: out_on_device).
 * gfw_sync_gyro_search: the two-stage search of :52-75 for every range without a host round trip — coarse costs of the
 * `search_size as usize * 2` candidates `initial_offset - search_size + i` (the cast comes first: 2.5 gives 4), pick, fine costs of
 * the 200 candidates `lowest.0 + (-2.0 + i * (2.0 / 200.0))` generated on the device (below the coarse pick only), pick: four launches
 * for any number of ranges.  `reduce_with(find_min)` with `if a.1 < b.1 { a } else { b }`: of equal costs the LAST candidate wins,
 * in both stages, also when every cost is f64::MAX.
 *   results      [n_ranges] gfw_sync_result: found = 0 when the coarse stage has no candidates (search_size < 1; the second stage
 *                then does nothing and fine costs are 0); n_coarse; the coarse pick and its cost; value / cost: the fine pick
 *   coarse_costs / fine_costs   NULL or [n_ranges][n_coarse] / [n_ranges][200] f64; with results host or device memory
 * The guards, the range cut, the gyro window, the max-angle skip, the two low-pass calls, the 90 % rule (:81) and the middle
 * timestamp are the caller's.  Everything travels in one pinned staging copy; both calls run in order on the context's stream; with
 * device outputs an asynchronous context returns without waiting.  n_ranges = 0 succeeds and writes nothing.  Rejected with
 * GFW_ERR_INVALID_ARGUMENT, the range named in gfw_last_error(), outputs untouched: null arguments for non-zero counts, negative
 * counts, a negative or descending first array, a slice outside its array, a non-finite initial_offset or search_size, a negative
 * search_size, counts over the limits above.  Non-finite sample values are not rejected; the pick among NaN costs is unspecified.
 * NOT covered: AKAZE (pyramidal Lucas-Kanade optical flow: gfw_flow_pyrlk below; its corner detection: gfw_corners_shi_tomasi below; the DIS dense flow: gfw_flow_dis below), the rs-sync crate's own solver (what runs for rs_sync: gfw_sync_rs_search below), pose estimation by a homography (method 3; the Almeida method: gfw_pose_almeida below; methods 0 and 2, an essential matrix: gfw_pose_essential below; the series of
 * estimated samples is made of their rotations by gyroflow::estimated_gyro / gyroflow_amd.synchronization.estimated_gyro).
 *
 * gfw_lowpass_gyro: Lowpass::filter_gyro_forward_backward (filtering.rs:46-74) of xyz [n][3] f64 in place, on the host (no context):
 * biquad's second-order Butterworth low-pass (Q = 1/sqrt 2), transposed direct form II, forward over the series and then backward;
 * entries with has[i] == 0 are skipped and do not advance the filter state (a NULL has = all present).  Returns GFW_OK, or
 * GFW_FILTER_NOT_APPLIED with the data untouched where the reference's Coefficients::from_params fails (2 * freq > sample_rate; also
 * a non-finite or non-positive freq or sample_rate) — the reference ignores that error and goes on unfiltered (:47-48). */
#define GFW_FILTER_NOT_APPLIED 1
int   gfw_lowpass_gyro(double freq, double sample_rate, double *xyz, const uint8_t *has, int n);
int   gfw_sync_gyro_costs(gfw_ctx *ctx, const int32_t *est_first, const double *est, const uint8_t *est_has, int n_est,
                          const int32_t *gyro_first, const double *gyro, const uint8_t *gyro_has, int n_gyro, int n_ranges,
                          const int32_t *cand_first, const double *candidates, int n_candidates, double *costs, int out_on_device);
int   gfw_sync_gyro_search(gfw_ctx *ctx, const int32_t *est_first, const double *est, const uint8_t *est_has, int n_est,
                           const int32_t *gyro_first, const double *gyro, const uint8_t *gyro_has, int n_gyro, int n_ranges,
                           double initial_offset_ms, double search_size_ms, gfw_sync_result *results, double *coarse_costs, double *fine_costs,
                           int out_on_device);

/* ---- synchronization: where in a clip to sync (OptimSync) in one device call ----
 * optimsync.rs:68-225, which StabilizationManager runs before any optical flow: a Blackman-windowed spectrum of
 * fft_size = round(sample_rate) gyro samples per axis every 16 samples, every bin folded with its mirror
 * (`zip(cm.iter(), cm.iter().rev())`: X[k] + X[fft_size-1-k]), norm * scale, the axes merged as (x + y) + z; the band sums lf / mf / hf over
 * bins [map_to_bin(0), map_to_bin(2)), [.. 2, 30), [.. 30, 2000) with map_to_bin(f) = round(fft_size / sample_rate * f) clamped to
 * 0 .. fft_size/2 - 1; the rank (the low-motion formula when max(mf) < 50); the masks (rank < 50, outside every trim range, the first
 * and last 2 s when the windows span more than 12 s); the non-maximum suppression over `(sample_rate / 16 / 2 * 8) as usize` windows;
 * per segment of ceil(len / target) windows the LAST maximal element unless it is < 0.1, as the time
 * (idx * 16 + fft_size / 2.0) / sample_rate * 1000.0 ms.
 * The reference's transform is rustfft in f32, whose summation order is no contract; the quantity is restated: bin k of
 * a window is the left fold over n of xw[n] * cos[(k n) mod fft_size] (and of -(xw[n] * sin[..])), every product and sum one f32 operation,
 * xw[n] = (x[n] as f32) * win[n], the tables those of gfw_optim_tables; X[fft_size-1-k] of a real input is conj(X[k+1]); the norm is
 * sqrtf(re * re + im * im).  Everything behind the bins is the reference's own f32 arithmetic in its own order.
 *   gyro       [3][n_samples] f64, axis after axis (OptimSync::new's series: gfw_optim_resample); cast to f32 while staging
 *   limits     fft_size 16 .. 8192, n_samples <= 2^24, target_sync_points 1 .. 65535, at most 1024 trim ranges
 * gfw_sync_optim_rank: lf, mf, hf, rank (before the masks) [n_windows] f32, each NULL or host / device memory (out_on_device);
 * n_windows (NULL, or ALWAYS host memory: the arguments decide it) = 0 when n_samples < fft_size, else (n_samples - fft_size) / 16 + 1.
 * gfw_sync_optim_points: points_ms [target_sync_points] f64 of which the first *n_points (int32) are written, in segment order; rank
 * (before the masks) and rank_nms [n_windows] f32, NULL or memory as points_ms; ratio (NULL, or ALWAYS host memory) = 16 / sample_rate.
 * trim_ranges_s [n_trim][2] f64 seconds; an empty list yields no points (`any` over nothing).  n_samples < fft_size succeeds with 0
 * windows and 0 points.  The series travels in one pinned staging copy; both calls run in order on the context's stream (three and six
 * launches for any clip length); with device outputs an asynchronous context returns without waiting.  Rejected with
 * GFW_ERR_INVALID_ARGUMENT, the reason in gfw_last_error(), outputs untouched: null arguments for non-zero counts, negative counts,
 * target_sync_points < 1 (the reference divides by it) or > 65535, a non-finite or non-positive sample_rate, fft_size outside
 * 16 .. 8192, n_samples > 2^24, more than 1024 trim ranges.  Non-finite gyro values are not rejected; the result among NaNs is
 * unspecified.
 *
 * Host only, no context:
 * gfw_optim_tables: blackman(fft_size) as optimsync.rs:15-27 writes it (f32 arithmetic, the C library's cosf, size = width - 1) and the
 * twiddles cos / sin(2 pi j / fft_size), evaluated in f64 and rounded once; each array [fft_size] f32 or NULL.
 * gfw_optim_resample: OptimSync::new (:30-66) of timestamps_ms [n], xyz [n][3], has [n] (0 = `gyro: None`; NULL = all present): the
 * average rate over the samples that have a value, then `(duration_ms * rate / 1000.0) as usize` samples at i * 1000 / rate, each the
 * two-sided linear interpolation around partition_point(timestamp < t) in f64 (a None side counts as zeros).  out: NULL (a query of
 * *n_out and *sample_rate) or [3][out_stride] f64 with out_stride >= *n_out.  Rejected: n < 1, more than 2^24 samples. */
int   gfw_optim_tables(int fft_size, float *win, float *cosv, float *sinv);
int   gfw_optim_resample(const double *timestamps_ms, const double *xyz, const uint8_t *has, int n, double *out, int64_t out_stride,
                         int64_t *n_out, double *sample_rate);
int   gfw_sync_optim_rank(gfw_ctx *ctx, const double *gyro, int64_t n_samples, double sample_rate, float *lf, float *mf, float *hf, float *rank,
                          int32_t *n_windows, int out_on_device);
int   gfw_sync_optim_points(gfw_ctx *ctx, const double *gyro, int64_t n_samples, double sample_rate, int target_sync_points,
                            const double *trim_ranges_s, int n_trim, double *points_ms, int32_t *n_points, float *rank, float *rank_nms,
                            double *ratio, int out_on_device);

/* ---- synchronization: Almeida pose estimation of a clip's frame pairs in one device call ----
 * estimate_pose/almeida.rs:23-238 (`PoseAlmeida`, also what `EstimatePoseMethod::from` falls back to): per pair of frames the matched
 * optical-flow points become one camera rotation — `solve_ypr_ransac` (:194-238) over `solve_ypr_given` (:124-192).  The reference
 * draws a round's three points and its sample list from an unseeded generator, so it has no reproducible output: here THE DRAWS ARE
 * INPUTS, and the result is a function of them that tests/_posestmt.py states in f32, operation by operation (nalgebra's quaternion,
 * Euler-angle and LU forms are restated there from the crate's documented forms).  `Camera::delta` (:58-68) always maps a point at
 * the same position with lens_correction_amount 1.0, fov 1.0, no shifts and no mesh, so the lens is inverted once per point; every
 * later delta is one f32 gemv through f32(K * f64(R)) and two divides.
 *   params     the KernelParams `undistort_points` builds, as for gfw_undistort_points; f / c = the f32 cast of camera_matrix
 *   pair_first [n_pairs + 1] ascending: pair p owns points pair_first[p] .. pair_first[p + 1] - 1 of points_a / points_b [total][2] f32
 *              (optical-flow pixels of the first / second frame)
 *   triples    [n_pairs][num_iters][3] the three distinct points of each round, indices into the pair (ignored for pairs under 3 points)
 *   samples    NULL: every round's list is 0 .. n-1 (one of the permutations the reference's draw can produce; rejected when a pair has
 *              more than num_samples points).  Otherwise pair p owns samples[sample_first[p] ..]: [num_iters][min(n, num_samples)]
 *              indices into the pair, sample_first [n_pairs + 1] ascending with exactly that many entries a pair
 *   quats      [n_pairs][4] f32 (w, i, j, k): the estimated rotation; rotations [n_pairs][9] f64 row-major: its matrix, computed in f32
 *              and cast — what estimate_pose returns.  The identity for a pair under 3 points or under 3 best inliers
 *   best       [n_pairs][2] int32: the inliers of the best round and that round (the FIRST of equal counts; -1 without rounds)
 *   round_inliers / round_fits   NULL or [n_pairs][num_iters] int32 / [n_pairs][num_iters][4] f32: every round's count and fit
 *   limits     at most 4096 points in a pair, 65535 pairs, 1024 rounds, 2 GiB staged in all
 * Four launches for any clip, in order on the context's stream; outputs are host or device memory (out_on_device); with device
 * outputs an asynchronous context returns without waiting.  n_pairs = 0 succeeds and writes nothing.  Rejected with
 * GFW_ERR_INVALID_ARGUMENT, the pair named in gfw_last_error(), outputs untouched: null arguments for non-zero counts, negative counts,
 * a descending pair_first, counts over the limits, an index outside its pair, a triple with a repeated index, a sample_first that does
 * not match, params->flags with HAS_IBIS_DATA, HAS_MESH_DATA or HAS_FPD_DATA, f / c that are not the f32 cast of camera_matrix,
 * sizes under 1, a negative or NaN inlier angle, a non-zero reserved slot.
 * NOT covered: lens data or a refraction coefficient that changes between the pairs of one call (one call per lens); pose method 3
 * (`PoseFindHomography`; methods 0 and 2 map to gfw_pose_essential below, which reproduces neither OpenCV's LMedS nor ARRSAC); AKAZE (the DIS dense flow: gfw_flow_dis below; the matched points of the
 * pyramidal Lucas-Kanade method: gfw_flow_pyrlk below, its features: gfw_corners_shi_tomasi below).
 *
 * gfw_pose_draws (host only, no context): one valid set of draws per seed — not rand's sequence.  A counter-based generator:
 * word(seed, pair, round, k) = mix(mix(seed ^ (pair << 32 | round)) + k) with SplitMix64's finaliser as mix, an index below r the high
 * word of (word >> 32) * r; a triple is three distinct indices, a list the first min(n, num_samples) entries of a Fisher-Yates shuffle
 * of 0 .. n-1.  samples NULL: triples only.  Pairs under 3 points get zero triples. */
typedef struct gfw_pose_almeida_cfg {
    int32_t video_width, video_height;     /* compute_params.width / height */
    int32_t flow_width, flow_height;       /* FrameResult::frame_size */
    int32_t num_iters, num_samples;        /* 200, 1000 */
    float   inlier_angle_deg;              /* 0.05 */
    int32_t reserved;                      /* 0 */
    double  camera_matrix[9];              /* get_lens_data_at_timestamp(..).0, row-major */
} gfw_pose_almeida_cfg;
int   gfw_pose_almeida(gfw_ctx *ctx, const gfw_kernel_params *params, const gfw_pose_almeida_cfg *cfg,
                       const int32_t *pair_first, const float *points_a, const float *points_b, int n_pairs,
                       const int32_t *triples, const int32_t *sample_first, const int32_t *samples,
                       float *quats, double *rotations, int32_t *best, int32_t *round_inliers, float *round_fits, int out_on_device);
int   gfw_pose_draws(uint64_t seed, const int32_t *pair_first, int n_pairs, int num_iters, int num_samples,
                     int32_t *triples, const int32_t *sample_first, int32_t *samples);

/* ---- synchronization: essential-matrix pose estimation of a clip's frame pairs in one device call ----
 * estimate_pose/mod.rs:27-36: pose methods 0 (`PoseFindEssentialMat`) and 2 (`PoseEightPoint`) fit an essential matrix to the
 * undistorted points of a pair and return its rotation part — what a pair needs whose camera also MOVED (parallax that no rotation
 * explains: gfw_pose_almeida's model is rotation only).  Both methods map to this call.  Their solvers are NOT part of the reference
 * tree — OpenCV's findEssentialMat (LMedS) / recoverPose, and the `arrsac` and `eight-point` crates — and NEITHER IS REPRODUCED: no
 * LMedS, no ARRSAC, no five-point solver.  What runs is the published scheme both stand on, stated operation by operation in
 * tests/_posessstmt.py with THE DRAWS AS INPUTS; the device equals that statement to the bit, and the statement is held to recovering
 * a planted camera motion.  Nothing reference-produced is compared.  All arithmetic behind the lens inverse is f64 (+ - * / sqrt).
 *   prepare    `undistort_points_for_optical_flow` (cpu_undistort.rs:642-650): the lens inverse of every point of both frames, identity
 *              rotation, no P, correction amount 1.0, fov 1.0; a point without an inverse becomes (-1e6, -1e6) (:855) and takes part
 *              like any other.  The f32 (x, y) give the f64 normalised point (x, y, 1) and its unit bearing (eight_point.rs:29-34).
 *              (The point is scaled to the video's size in front of the unscaled K, as gfw_pose_almeida does it; the reference scales K.)
 *   fit        per (pair, round): M = sum of kron(b2, b1) kron(b2, b1)^T over the round's 8 points; E = the eigenvector of M's smallest
 *              eigenvalue by a cyclic Jacobi iteration (10 sweeps, (p, q) in row order, a rotation skipped where the off-diagonal is 0)
 *   score      a point is an inlier where the squared Sampson distance of the normalised points under E is <= inlier_threshold
 *              (1e-6: the last of the reference's three ARRSAC thresholds, 1 px at a focal length of 1000 px)
 *   pick       the FIRST round of maximal count; its inliers in point order; M over them, folded in list order; one more solve; the SVD
 *              of E through the Jacobi eigenvectors of E^T E; the two rotations U W V^T and U W^T V^T, both of determinant +1; per
 *              rotation and sign of t = +-u3 the inliers whose two depths are positive; a rotation's score is the larger of its two
 *              counts; the higher score wins, equal scores go to the larger trace (the smaller angle: eight_point.rs:50-55)
 *   no rotation   a pair under 8 points, a best round under 8 inliers, or a winning score under min_front (10:
 *              find_essential_mat.rs:43): found = 0, the rotation is the identity, the quaternion (1, 0, 0, 0)
 *   octets     [n_pairs][num_iters][8] the eight distinct points of each round, indices into the pair (ignored for pairs under 8 points)
 *   quats      [n_pairs][4] f32 (w, i, j, k); rotations [n_pairs][9] f64 row-major; essential [n_pairs][9] f64: the refit E (zeros
 *              where the best round has under 8 inliers); best [n_pairs][4] int32: inliers, round (-1 without rounds), front count, found
 *   round_inliers / round_fits   NULL or [n_pairs][num_iters] int32 / [n_pairs][num_iters][9] f64: every round's count and E
 *   limits     at most 4096 points in a pair, 65535 pairs, 1024 rounds, 2 GiB staged in all
 * Four launches for any clip, in order on the context's stream; outputs are host or device memory (out_on_device); with device
 * outputs an asynchronous context returns without waiting.  n_pairs = 0 succeeds and writes nothing.  Rejected with
 * GFW_ERR_INVALID_ARGUMENT, the pair named in gfw_last_error(), outputs untouched: null arguments for non-zero counts, negative counts,
 * a descending pair_first, counts over the limits, an octet index outside its pair or repeated within its octet, params->flags with
 * HAS_IBIS_DATA, HAS_MESH_DATA or HAS_FPD_DATA, f / c that are not the f32 cast of camera_matrix, sizes under 1, a negative or NaN
 * threshold, a negative min_front, a non-zero reserved slot.
 * NOT covered: what gfw_pose_almeida does not cover; pose method 3 (`PoseFindHomography`); the translation (its direction is +-u3 of
 * `essential`, its length is not observable).
 *
 * gfw_pose_draws_k (host only, no context): gfw_pose_draws' counter-based generator for k distinct indices a round (1 <= k <= 16):
 * draw j is the r-th of the indices not drawn yet, r the uniform index below n - j of counter j.  At k = 3 these are gfw_pose_draws'
 * triples to the bit.  tuples [n_pairs][num_iters][k]; a pair under k points gets zeros. */
typedef struct gfw_pose_essential_cfg {
    int32_t video_width, video_height;     /* compute_params.width / height */
    int32_t flow_width, flow_height;       /* FrameResult::frame_size */
    int32_t num_iters;                     /* 200 */
    int32_t min_front;                     /* 10 */
    double  inlier_threshold;              /* 1e-6 */
    int32_t reserved[2];                   /* 0 */
    double  camera_matrix[9];              /* get_lens_data_at_timestamp(..).0, row-major */
} gfw_pose_essential_cfg;
int   gfw_pose_essential(gfw_ctx *ctx, const gfw_kernel_params *params, const gfw_pose_essential_cfg *cfg,
                         const int32_t *pair_first, const float *points_a, const float *points_b, int n_pairs,
                         const int32_t *octets, float *quats, double *rotations, double *essential, int32_t *best,
                         int32_t *round_inliers, double *round_fits, int out_on_device);
int   gfw_pose_draws_k(uint64_t seed, const int32_t *pair_first, int n_pairs, int num_iters, int k, int32_t *tuples);

/* ---- synchronization: the rs-sync offset search of all ranges of a clip in one device call ----
 * find_offset/rs_sync.rs: offset method 2, the reference's default (synchronization/mod.rs:383) — the one search that is rolling-shutter
 * aware per point and tolerates a camera that moved.  The adapter is mirrored: what goes in (:115-146, per-point unit bearings and
 * per-point timestamps), what comes out (a delay in seconds and a cost) and, in the mirrors, the acceptance rule (:178).  Its solver,
 * the `rs-sync` crate, is NOT part of the reference tree and is NOT REPRODUCED — neither its cost, nor its round schedule, nor its
 * final gradient refinement.  What runs is stated operation by operation in tests/_rssyncstmt.py; the device equals that statement
 * to the bit, and the statement is held to finding planted delays.  Nothing reference-produced is compared.  All arithmetic behind
 * the lens inverse is f64 (+ - * / sqrt); every sum has one fixed order.
 *   prepare    `undistort_points_for_optical_flow` of both frames' points as gfw_pose_essential's prepare stage ((-1e6, -1e6) where
 *              the lens has no inverse); the f32 (x, y) give the f64 unit bearing of (x, y, 1); the point's time is
 *              pair_ts / 1e6 + (frame_readout_time_ms / 1000) * (y_raw / flow_height), y_raw the flow pixel's own y (:132-133)
 *   track      track_ts_us [n_track] strictly ascending, track_wxyz [n_track][4] f64 (w, x, y, z): an INPUT of the call, as
 *              rs_sync.rs:159 passes `gyro.quaternions` and guess_orient passes other tracks — not the context's tracks.  At time t:
 *              t clamped to the track's ends, bisection, normalised linear interpolation with the shorter-arc flip, one sqrt (not
 *              slerp: no acos / sin).  World bearing: R(q(t)) diag(1, -1, -1) p, the rotation by pi about X of set_quats (:248-251)
 *   pair cost  at delay d: m_i = ra_i x rb_i with both bearings in the world at t_i + d (a static scene: every m_i perpendicular to
 *              the camera's translation).  Direction hypothesis 0: the eigenvector of the smallest eigenvalue of sum m_i m_i^T
 *              (cyclic Jacobi, jacobi_sweeps sweeps, the first of equal eigenvalues); hypotheses h = 1 .. hypotheses: m_i x m_j
 *              normalised, i = 7h mod n, j = (13h + 5) mod n, skipped where its squared length is not > 0.  Score
 *              sum rho(loss_scale * m_i.t), rho(x) = x^2 / (1 + x^2); the FIRST minimal hypothesis wins; `refits` refits with
 *              w_i = 1 / (1 + x_i^2)^2; the cost is the score at the last t.  A pair of 0 points costs 0; of 1 point: hypothesis 0 only.
 *              Sums over a pair's points: lane l of 64 folds points l, l + 64, .. from 0.0, then v = v + v[l ^ off], off = 32 .. 1
 *   range      range r owns pairs range_first[r] .. range_first[r + 1] - 1 (range_first[0] = 0, range_first[n_ranges] = n_pairs);
 *              pair p owns points pair_first[p] .. of points_a / points_b [..][2] f32 and pair_ts_us [n_pairs][2] (both frames' times).
 *              A range's cost is the sum of its pairs' costs in pair order
 * gfw_sync_rs_costs: the range costs of caller-given candidate delays (seconds): range r owns candidates cand_first[r] ..
 * cand_first[r + 1] - 1 (cand_first[0] = 0) and the same entries of costs — the building block of pre_sync and the orientation guess.
 * gfw_sync_rs_search: `full_sync(initial_delay, from, to, step, radius, rounds)` (:164-175) for every range without a host round
 * trip, 1 + 2 * rounds launches: round 0 has 2h + 1 candidates initial_delay_s + (i - h) * step_s, h = floor(radius_s / step_s); every
 * later round 17 candidates pick + (i - 8) * (step / 8), the step divided by 8 again; of equal costs the FIRST candidate wins; with
 * `refine`, behind the last round the vertex of the parabola through the pick and its two neighbours where both exist and the second
 * difference is positive.
 *   results    [n_ranges] gfw_sync_result: found = 0 for a range without pairs (everything else 0); n_coarse = 2h + 1; the round-0
 *              pick and its cost; value / cost: the final delay (seconds) and the last pick's cost
 *   round_candidates / round_costs   NULL or [n_ranges][2h + 1 + 17 (rounds - 1)] f64: every round's candidates and range costs
 *   limits     at most 4096 points in a pair, 65535 pairs, 65535 ranges, 2^24 track samples, 2^20 candidates a range and round,
 *              rounds 1 .. 8, hypotheses 0 .. 64, refits 0 .. 16, jacobi_sweeps 1 .. 32, 2 GiB staged in all
 * The sign and unit conventions (initial_delay = -initial_offset, offset = -delay * 1000 - readout / 2), the readout rules (:74-81),
 * the range cut and the 90 % rule are the caller's (gyroflow::find_offsets_rssync, gyroflow_amd.synchronization).  Everything travels
 * in one pinned staging copy; both calls run in order on the context's stream; outputs are host or device memory (out_on_device);
 * with device outputs an asynchronous context returns without waiting.  n_ranges = 0 succeeds and writes nothing.  Rejected with
 * GFW_ERR_INVALID_ARGUMENT, the range or pair named in gfw_last_error(), outputs untouched: null arguments for non-zero counts,
 * negative counts, a first array that does not start at 0, descends or does not end at its count, more than 4096 points a pair,
 * counts over the limits, a track under 2 samples or not strictly ascending, a non-finite or non-positive step, a negative or
 * non-finite radius, a non-finite initial delay, rounds outside 1 .. 8, params->flags with HAS_IBIS_DATA, HAS_MESH_DATA or
 * HAS_FPD_DATA, f / c that are not the f32 cast of camera_matrix, sizes under 1, a non-zero reserved slot.  Non-finite point or
 * quaternion values are not rejected; the pick among NaN costs is unspecified.
 * NOT covered: the crate's own numerics; AKAZE; `apply_transforms` for the 48 orientations of guess_orient (the caller transforms the
 * tracks); per_frame_time_offsets; lens data keyframed inside a call. */
typedef struct gfw_sync_rs_cfg {
    int32_t video_width, video_height;     /* compute_params.width / height */
    int32_t flow_width, flow_height;       /* FrameResult::frame_size */
    int32_t rounds, refine;                /* 4, 1 */
    int32_t hypotheses, refits;            /* 16, 3 */
    int32_t jacobi_sweeps;                 /* 5: every 3 x 3 matrix of the test plants is at its floor after 4 */
    int32_t reserved[3];                   /* 0 */
    double  frame_readout_time_ms;         /* after the rules of rs_sync.rs:74-80 */
    double  step_s;                        /* 3.0 / 1000.0 */
    double  loss_scale;                    /* 1000: about 1 px at f = 1000 px */
    double  camera_matrix[9];              /* get_lens_data_at_timestamp(..).0, row-major */
} gfw_sync_rs_cfg;
int   gfw_sync_rs_costs(gfw_ctx *ctx, const gfw_kernel_params *params, const gfw_sync_rs_cfg *cfg, const int32_t *range_first, int n_ranges,
                        const int64_t *pair_ts_us, const int32_t *pair_first, const float *points_a, const float *points_b, int n_pairs,
                        const int64_t *track_ts_us, const double *track_wxyz, int n_track,
                        const int32_t *cand_first, const double *candidates, int n_candidates, double *costs, int out_on_device);
int   gfw_sync_rs_search(gfw_ctx *ctx, const gfw_kernel_params *params, const gfw_sync_rs_cfg *cfg, const int32_t *range_first, int n_ranges,
                         const int64_t *pair_ts_us, const int32_t *pair_first, const float *points_a, const float *points_b, int n_pairs,
                         const int64_t *track_ts_us, const double *track_wxyz, int n_track, double initial_delay_s, double radius_s,
                         gfw_sync_result *results, double *round_candidates, double *round_costs, int out_on_device);

/* ---- synchronization: pyramidal Lucas-Kanade optical flow of a clip's frame pairs in one device call ----
 * optical_flow/opencv_pyrlk.rs:63-119 (`OFOpenCVPyrLK::optical_flow_to`, the reference's method 1): the given features of each pair's
 * first frame are tracked into its second frame — calcOpticalFlowPyrLK with window 21 x 21, maxLevel 3, 30 iterations or eps 0.01,
 * flags 0, minEigThreshold 1e-4 — and the tracked points are filtered (:88-100).  OpenCV's source is not part of the reference tree, so
 * nothing reference-produced pins the tracker: the contract is tests/_flowstmt.py, the published pyramidal Lucas-Kanade scheme stated
 * operation by operation with every window sum an INTEGER (fixed-point pixels, derivatives and bilinear samples, exact sums, one
 * conversion to f32 per sum), which the device equals to the bit.  The statement is first held to tracking a planted motion.
 *   cfg         width, height (both 24 .. 8192), stride >= width, point_mode, reserved = 0
 *   frames      n_frames u8 gray planes back to back, frame f at frames + f * stride * height; host memory, or device memory with
 *               frames_on_device (it must stay valid until the stream has run the call)
 *   pair_frames [n_pairs][2] (first frame, second frame) indices
 *   point_mode 0: feat_first [n_frames + 1] ascending, frame f owns features[feat_first[f] .. feat_first[f + 1] - 1] ([..][2] f32 pixels,
 *               host memory); pair p has the features of its first frame.  A feature that is not finite or lies outside
 *               [0, w) x [0, h) is not tracked: status 0, next = the feature
 *   point_mode 1: feat_first / features are ignored; the points are the grid of opencv_dis.rs:62-119 (step = w / 15, the texture
 *               variance of a max(10, round(0.02 w)) window > 3.0) computed on the device from each frame; every pair has
 *               nodes = ceil(w / step) * ceil(h / step) raw slots, of which the first grid_counts[first frame] are used (the rest:
 *               status 0, next 0).  grid_points NULL or [n_frames][nodes][2] f32 (kept nodes first, in the reference's loop order, then
 *               zeros), grid_counts NULL or [n_frames] int32
 *   raw outputs over every (pair, feature), pair after pair: next [raw][2] f32, status [raw] u8, iters NULL or [raw][4] int32 (the
 *               updates made at level 0 .. 3, -1 for a level not built or skipped)
 *   compacted   out_pair_first [n_pairs + 1] int32 and points_a / points_b [..][2] f32: the pairs' kept points in feature order (status
 *               1, both points in [0, w) x [0, h)) — exactly gfw_pose_almeida's and gfw_sync_visual_*'s pair_first / points_a /
 *               points_b.  Room for [raw][2] each; only the kept entries are written.  The "at least 10" rule (:107) is the caller's
 *   limits      at most 4096 features a frame (grid nodes in mode 1), 65535 pairs, 4096 frames, 2 GiB staged in all
 * At most seven launches for any clip (three pyramid levels, the grid, the tracker, a scan, the compaction), in order on the context's
 * stream; outputs are host or device memory (out_on_device); with device outputs an asynchronous context returns
 * without waiting.  n_pairs = 0 succeeds and writes nothing.  Rejected with GFW_ERR_INVALID_ARGUMENT, the pair or frame named in
 * gfw_last_error(), outputs untouched: null arguments for non-zero counts, negative counts, a descending feat_first, a frame index out
 * of range, a pair of a frame with itself, sides outside 24 .. 8192, stride < width, mode 0 without features, counts over the limits,
 * a non-zero reserved slot.
 * NOT covered: AKAZE.  (Corner detection, goodFeaturesToTrack: gfw_corners_shi_tomasi below; the DIS dense flow, the reference's
 * default method 2: gfw_flow_dis below, with its variational refinement gfw_flow_dis_refined.) */
typedef struct gfw_flow_pyrlk_cfg {
    int32_t width, height, stride;         /* of every frame of the call */
    int32_t point_mode;                    /* 0 the caller's features, 1 the grid points */
    int32_t reserved;                      /* 0 */
} gfw_flow_pyrlk_cfg;
int   gfw_flow_pyrlk(gfw_ctx *ctx, const gfw_flow_pyrlk_cfg *cfg, const void *frames, int frames_on_device, int n_frames,
                     const int32_t *pair_frames, int n_pairs, const int32_t *feat_first, const float *features,
                     float *next, uint8_t *status, int32_t *iters, float *grid_points, int32_t *grid_counts,
                     int32_t *out_pair_first, float *points_a, float *points_b, int out_on_device);

/* ---- synchronization: Shi-Tomasi corner detection of a clip's frames in one device call ----
 * optical_flow/opencv_pyrlk.rs:25-42 (`OFOpenCVPyrLK::detect_features`, the first link of the reference's method 1): the features of a
 * frame are good_features_to_track(img, 200, 0.01, 10.0, no mask, blockSize 3, useHarris false, 0.04).  OpenCV's source is not part of
 * the reference tree, so nothing reference-produced pins the detector: the contract is tests/_cornerstmt.py, the published Shi-Tomasi /
 * goodFeaturesToTrack scheme stated operation by operation, which the device equals to the bit:
 *   Dx, Dy     the 3 x 3 Sobel of the u8 image as int32 on reflect-101 indices (-1 -> 1, n -> n - 2)
 *   S          the 3 x 3 unnormalised box sums of Dx^2, Dx Dy, Dy^2, the PRODUCT maps reflected (reflect-101), as OpenCV filters `cov`;
 *              every sum is an exact integer below 2^24
 *   e          (a + c) - sqrtf((a - c)^2 + b^2) with a = Sxx * 0.5, c = Syy * 0.5, b = Sxy in f32, one rounding per operation; OpenCV's
 *              scale 1 / (12 * 255) is dropped (the selection depends only on e relative to the frame's maximum): scores are this e
 *   threshold  t = max(max over all pixels of e, 0) * quality; candidates are the interior pixels (1 .. n - 2) with e > t and e >= all
 *              eight neighbours (plateaus count in full)
 *   pick       in descending order of the key bits(e) << 32 | (y * width + x) (on a tie the larger pixel index first) a candidate is
 *              accepted unless an accepted one lies closer than min_distance: (float)(dx^2 + dy^2) < min_distance * min_distance;
 *              min_distance < 1 accepts everything; at most max_corners.  A corner is (float x, float y), in pick order
 *   cfg        width, height (both 3 .. 8192), stride >= width (the padding is not read), max_corners 1 .. 4096, quality in (0, 1],
 *              min_distance in [0, 1024], max_workspace_mb (below), reserved = 0
 *   frames     n_frames u8 gray planes back to back, frame f at frames + f * stride * height; host memory, or device memory with
 *              frames_on_device (it must stay valid until the stream has run the call) — gfw_flow_pyrlk's contract
 *   corners    [n_frames][max_corners][2] f32: the kept corners first, in pick order, then zeros
 *   scores     NULL or [n_frames][max_corners] f32; counts [n_frames] int32
 *   feat_first [n_frames + 1] int32 and features [..][2] f32 (room for [n_frames * max_corners][2], only the kept entries written): the
 *              packed form gfw_flow_pyrlk takes in point mode 0.  Both NULL or both given
 * A frame's candidate list has room for EVERY interior pixel (8 bytes each; a plateau image makes all of them candidates): no overflow
 * path exists.  The call's frames are therefore dealt into batches whose lists fit max_workspace_mb MiB of device work space (0: 512,
 * which holds one frame of 8192 x 8192); a value too small for ONE frame is rejected with the need named.  Launches: two per batch plus
 * two (the scan and the pack of feat_first / features, only where they are asked for), in order on the context's stream; the pick of a
 * frame takes at most max_corners rounds of ceil(candidates / 256) steps.  Outputs are host or device memory (out_on_device); with device
 * outputs an asynchronous context returns without waiting.  n_frames = 0 succeeds and writes nothing.  Rejected with
 * GFW_ERR_INVALID_ARGUMENT, the reason in gfw_last_error(), outputs untouched: null arguments for non-zero counts, negative counts, sides
 * or stride out of range, max_corners / quality / min_distance out of range or not finite, a negative max_workspace_mb, a non-zero
 * reserved slot, more than 4096 frames, host frames over 2 GiB in all.
 * NOT covered: a mask, the Harris response (the reference passes neither); AKAZE.  (The DIS dense flow: gfw_flow_dis below, with its variational
 * refinement gfw_flow_dis_refined.) */
typedef struct gfw_corners_cfg {
    int32_t width, height, stride;      /* of every frame; sides 3 .. 8192, stride >= width */
    int32_t max_corners;                /* 1 .. 4096 (gfw_flow_pyrlk's features-a-frame limit); the reference: 200 */
    float   quality, min_distance;      /* the reference: 0.01, 10.0; quality finite in (0, 1], min_distance finite in [0, 1024] */
    int32_t max_workspace_mb;           /* 0 = default (512); the candidate lists of a batch */
    int32_t reserved;                   /* 0 */
} gfw_corners_cfg;
int   gfw_corners_shi_tomasi(gfw_ctx *ctx, const gfw_corners_cfg *cfg, const void *frames, int frames_on_device, int n_frames,
                             float *corners, float *scores, int32_t *counts, int32_t *feat_first, float *features, int out_on_device);

/* ---- synchronization: DIS dense optical flow of a clip's frame pairs in one device call ----
 * optical_flow/opencv_dis.rs (`OFOpenCVDis`, the reference's DEFAULT method 2: stabilization_params.rs:174): the dense inverse search
 * flow (Kroeger et al., "Fast Optical Flow using Dense Inverse Search") of every pair with the parameters of
 * DISOpticalFlow_PRESET_FAST (:59) — patch 8, patch stride 4, 16 descent iterations, finest scale 2, mean-normalised patches, spatial
 * propagation — read at the grid points of :62-119 (gfw_flow_pyrlk's point mode 1, unchanged).  VARIATIONAL REFINEMENT IS NOT PART OF
 * IT: the preset runs 5 iterations of it; cfg.variational_iters must be 0.  The refinement is gfw_flow_dis_refined below, a call of its
 * own with a configuration of its own: this interface, its rejection of a non-zero variational_iters and its kernels are pinned by
 * their tests as they were built, and the refinement's parameters (six of them) have no room in the one slot left here.
 * OpenCV's source is not part of the reference tree, so nothing reference-produced pins the flow: the contract is tests/_disstmt.py, the
 * published scheme stated operation by operation with every sum over a patch's 64 pixels an INTEGER (integer gradients, fixed-point
 * bilinear samples, exact sums, one conversion to f32 per sum), which the device equals to the bit.  The statement is first held to a
 * planted motion: every interior node within the pose estimator's inlier angle of its analytic destination.  OpenCV's raster-order
 * propagation depends on its thread count and is not reproduced: three synchronous passes a level (descend; left and top neighbour,
 * descend; right and bottom neighbour, descend), so no result depends on an order of execution.
 *   cfg         width, height, stride >= width, finest_scale 1 | 2 (the reference: 2; 1 halves the flow's pixel), variational_iters = 0,
 *               reserved = 0.  Scales coarsest .. finest_scale are processed, coarsest = min(int(log2(max(w, h) / 32) + 0.5),
 *               int(log2(min(w, h) / 8))); a size with coarsest < finest_scale is rejected.  Sides up to 8192
 *   frames      n_frames u8 gray planes back to back, frame f at frames + f * stride * height; host memory, or device memory with
 *               frames_on_device (it must stay valid until the stream has run the call) — gfw_flow_pyrlk's contract
 *   pair_frames [n_pairs][2] (first frame, second frame) indices
 *   grid_points NULL or [n_frames][nodes][2] f32 (kept nodes first, in the reference's loop order, then zeros), grid_counts NULL or
 *               [n_frames] int32, nodes = ceil(w / step) * ceil(h / step), step = w / 15: as gfw_flow_pyrlk's
 *   flow        NULL or [n_pairs][h_f][w_f][2] f32, w_f = width >> finest_scale, h_f alike: the finest level's dense field, in that
 *               level's pixels
 *   result      out_pair_first [n_pairs + 1] int32 and points_a / points_b [..][2] f32: for EVERY node (i, j) the grid keeps in the
 *               pair's first frame, in grid order, a = (i, j) and b = a + 2^finest_scale * the field at ((i + 0.5) / 2^finest_scale
 *               - 0.5, ..) — the DIS arm filters nothing (:113-117), not even a b outside the frame — exactly gfw_pose_almeida's and
 *               gfw_sync_visual_*'s pair_first / points_a / points_b.  Room for [n_pairs * nodes][2] each; only the returned entries
 *               are written.  The "at least 10" rule (:126) is the caller's
 *   limits      at most 4096 grid nodes a frame, 65535 pairs, 4096 frames, 2 GiB staged in all, 16 GiB of device work space
 * Launches, whatever the number of pairs and frames: 3 + coarsest + 4 (coarsest - finest_scale + 1) — the pyramid levels, the grid, per
 * level three passes and the dense field, a scan, the node sampling; 24 for 1280 x 720 at finest_scale 2 — in order on the context's
 * stream; outputs are host or device memory (out_on_device); with device outputs an asynchronous context returns without waiting.
 * n_pairs = 0 succeeds and writes nothing.  Rejected with GFW_ERR_INVALID_ARGUMENT, the pair or frame named in gfw_last_error(),
 * outputs untouched: null arguments for non-zero counts, negative counts, a frame index out of range, a pair of a frame with itself,
 * stride < width, a size with coarsest < finest_scale (the size named), a finest_scale other than 1 or 2, a non-zero variational_iters
 * or reserved slot, counts over the limits.
 * NOT covered: variational refinement (gfw_flow_dis_refined below); AKAZE. */
typedef struct gfw_flow_dis_cfg {
    int32_t width, height, stride;         /* of every frame of the call */
    int32_t finest_scale;                  /* 1 | 2 */
    int32_t variational_iters;             /* 0 */
    int32_t reserved;                      /* 0 */
} gfw_flow_dis_cfg;
int   gfw_flow_dis(gfw_ctx *ctx, const gfw_flow_dis_cfg *cfg, const void *frames, int frames_on_device, int n_frames,
                   const int32_t *pair_frames, int n_pairs, float *grid_points, int32_t *grid_counts, float *flow,
                   int32_t *out_pair_first, float *points_a, float *points_b, int out_on_device);

/* ---- synchronization: DIS dense optical flow WITH its variational refinement, the reference's preset as a whole ----
 * gfw_flow_dis (above) with the refinement DISOpticalFlow_PRESET_FAST runs on every pyramid level: directly behind a level's dense
 * field, the field is refined in place — the Brox-style energy (brightness constancy, gradient constancy, smoothness) as Kroeger et
 * al. use it, linearised fixed_point_iters times, each linear system relaxed by sor_iters red-black SOR iterations — and the next
 * finer level's start values, the nodes and `flow` read the refined field.  The contract is tests/_varrefstmt.py, the scheme stated
 * operation by operation in f32 (every operator rounds once, sums in a fixed order, the second image warped once per level by
 * gfw_flow_dis's fixed-point sampler), which the device equals to the bit.  It is first held to what refinement is for: on the planted
 * motions every pair's mean interior node error falls and its worst does not rise (tests/test_varref_statement.py).
 * THE DEFAULTS — alpha 20, delta 5, gamma 10, 5 fixed-point and 5 SOR iterations, omega 1.6, and the fixed zeta 0.1, eps 0.001 — ARE
 * THE VALUES OpenCV's DIS IMPLEMENTATION SETS TO THE BUILDER'S BEST KNOWLEDGE: OpenCV's source is not part of the reference tree and
 * nothing in this tree confirms them.  OpenCV's own buffers, its floating-point warp and its thread striping are not reproduced.
 *   cfg         gfw_flow_dis's, variational_iters = 0 here too: the count lives in ref.  A non-zero one is rejected with both named
 *   ref         fixed_point_iters 0 .. 64 (the preset: 5; 0 issues no refinement launch and equals gfw_flow_dis to the bit), sor_iters
 *               1 .. 64, alpha (smoothness), delta (brightness constancy), gamma (gradient constancy) finite and > 0, omega finite
 *               in (0, 2), reserved = 0
 *   everything else: gfw_flow_dis's arguments, contracts, limits and rejections.  The refinement adds 17 floats per pixel and pair of
 *   the finest level to the device work space; both together stay under 16 GiB.
 * Launches: gfw_flow_dis's, plus per level 2 + fixed_point_iters (1 + 2 sor_iters) — 57 at 5 / 5; 252 instead of 24 for 1280 x 720
 * at finest_scale 2 — whatever the number of pairs. */
typedef struct gfw_flow_varref_cfg {
    int32_t fixed_point_iters, sor_iters;  /* the preset: 5, 5 */
    float   alpha, delta, gamma, omega;    /* 20, 5, 10, 1.6 */
    int32_t reserved[2];                   /* 0 */
} gfw_flow_varref_cfg;
int   gfw_flow_dis_refined(gfw_ctx *ctx, const gfw_flow_dis_cfg *cfg, const gfw_flow_varref_cfg *ref, const void *frames,
                           int frames_on_device, int n_frames, const int32_t *pair_frames, int n_pairs, float *grid_points,
                           int32_t *grid_counts, float *flow, int32_t *out_pair_first, float *points_a, float *points_b,
                           int out_on_device);

/* First-pass audit of the fused kernel (GFW_OPT_KERNEL_VARIANT = 3): counters8 = {certified pixels,
 * certified-but-different-from-exact (must stay 0), queued to the exact path, queue overflows,
 * max |approximate - exact| coordinate over certified pixels as f32 bits, addresses outside their buffer (audit mode range-checks),
 * the certificate half-width E of the last frame as f32 bits, 1 spare}.  Call with reset = 1 before
 * the frames to be audited. */
int   gfw_get_audit(gfw_ctx *ctx, unsigned long long *counters8, int reset);
/* (test hooks — device-side math probes, the host-side build check of the run-time specialisation path — are declared in
 * include/gfwarp_testing.h: they are not part of the operator surface) */

/* Static tables the reference exposes through PixelType (pixel_formats.rs):
 * bytes per pixel, element count, default_max_value (0 => None). */
int   gfw_pixel_type_info(int pixel_type, int *bytes_per_pixel,
                          int *element_count, float *default_max_value);

#ifdef __cplusplus
}
#endif
#endif /* GFWARP_H */
