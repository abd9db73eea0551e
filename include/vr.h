/*
 * vr.h -- C ABI of the MI355X-native volume ray-marcher (libvr_hip.so).
 *
 * This is the drop-in boundary for the ONE hot path of gutiKristian/VolumeRendering:
 * the per-pixel front-to-back compositing loop that the reference runs as WGSL
 * fragment shaders (App/shaders/{...}.wgsl `fs_main`) behind WebGPU/Dawn.  The reference
 * has no FFI of its own; what it has is a bind-group contract between
 * `Application::OnUpdate/OnRender` and the shaders.  Every entry point below cites the
 * reference interface it replaces (paths relative to the reference root).
 *
 * Conventions
 *   - plain C, no C++/torch types; every function returns VR_OK (0) or a negative
 *     vr_status; the message for the last failure is available via vr_last_error().
 *     No exception crosses this boundary.  (The reference only logs / asserts:
 *     WebgpuLib/src/Platform/Native/NativeGraphicsContext.cpp:102-116.)
 *   - a vr_ctx is bound to ONE HIP device (one process per GPU) and must be used by one
 *     thread at a time (the reference is single threaded, App/src/Application.cpp:332-379).
 *   - host pointers are copied at call time; the caller keeps ownership, exactly like
 *     wgpuQueueWriteTexture / wgpuQueueWriteBuffer (App/src/renderer/Texture.cpp:80,
 *     App/src/renderer/UniformBuffer.cpp:27).
 *   - all matrices are column-major float[16] (glm layout, App/src/Application.cpp:102-105).
 *   - there is NO CPU fallback behind this ABI: if no HIP device is usable vr_create
 *     fails with VR_ERR_HIP.
 */
#ifndef VR_H_
#define VR_H_

#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VR_ABI_VERSION 1

typedef enum vr_status {
    VR_OK = 0,
    VR_ERR_INVALID_ARG = -1,  /* null pointer, bad slot / variant / size                    */
    VR_ERR_HIP = -2,          /* a HIP runtime call failed (message has hipGetErrorString)   */
    VR_ERR_NOT_READY = -3,    /* render called before the volumes / TFs the variant needs    */
    VR_ERR_UNSUPPORTED = -4,  /* e.g. non-identity model matrix (see vr_set_uniforms)        */
    VR_ERR_OOM = -5,
    VR_ERR_INTERNAL = -6      /* a fault of the library itself: the message names it        */
} vr_status;

/* One value per fragment shader of the reference. */
typedef enum vr_variant {
    VR_VARIANT_BASIC = 0,       /* App/shaders/BasicVolumeApp.wgsl:113-188   unlit, cut-off dst.a <= 0.95 */
    VR_VARIANT_LIGHT = 1,       /* App/shaders/BasicVolLightApp.wgsl:151-237 lit,   cut-off dst.a <  1.0  */
    VR_VARIANT_VOLUME_MASK = 2, /* App/shaders/VolumeMaskApp.wgsl:128-217    mask + RT + CT               */
    VR_VARIANT_THREE_FILES = 3, /* App/shaders/ThreeFilesApp.wgsl:170-272    CT/RT colour mix             */
    VR_VARIANT_MULTI_CTRT = 4,  /* App/shaders/MultiCTRTApp.wgsl:163-259     CT/RT mix + shade + |g| opacity */
    VR_VARIANT_TF_CALIB = 5,    /* App/shaders/TFCalibrationApp.wgsl:114-197 CT + nearest-sampled mask     */
    /* App/shaders/MutliCTRTIllustrative.wgsl:227-313: MULTI_CTRT with the context-preserving opacity
     * opacityCT * pow(|g|, pow(5 s (1 - d) (1 - dst.a), 0.8)); slots as MULTI_CTRT, reads camera_pos.  The reference
     * compiles this module next to MultiCTRTApp.wgsl but never attaches it (MutliCTRTApp.cpp:112-119). */
    VR_VARIANT_ILLUSTRATIVE = 6,
    /* App/shaders/BasicVolLightApp.wgsl with the call the reference keeps commented out at :212 enabled:
     * gradient = ComputeGradient(currentPosition, stepSize, textMain) (:239-253) -- central differences of six extra
     * trilinear density samples at +-stepSize along the uvw axes, negated and normalised (zero length -> 0), instead of
     * the pre-computed .rgb of the voxels.  Slots and light as LIGHT; only the density plane of the volume is read.  */
    VR_VARIANT_LIGHT_INSHADER = 7,
    /* Intensity projections of volume slot 0 through TF slot 0 (no shader of the reference; csrc/vr_proj.h).  Sample
     * positions are exactly BASIC's march (BasicVolumeApp.wgsl fs_main): the same start, direction, stepsCount, step size,
     * variable-step toggle, jitter and repeated rounded additions p += step; fragmentMode 1-4 return what BASIC returns.
     * Only the n samples that pass IsInSampleCoords (the clip box) count, each d = textureSample(vol0, linear, p).a with
     * BASIC's arithmetic in either vr_set_arithmetic mode; no opacity cut-off.
     *   MIP:     m = -inf, then if (d > m) m = d          (NaN samples are ignored)
     *   MINIP:   m = +inf, then if (d < m) m = d          (NaN samples are ignored)
     *   AVERAGE: s = +0.0f, then s = s + d in step order (f32), v = s / (float)n   (NaN propagates)
     * n == 0: the pixel is (0,0,0,0).  Otherwise v goes through TF slot 0 with BASIC's lookup (linear, clamp-to-edge) and the
     * fragment is FrontToBackBlend((c.rgb, o), dst = 0) in the blend's own arithmetic: (c.r o, c.g o, c.b o, o), a -0 made +0.
     * Counters: composited = sum of n, covered = pixels with n > 0, fetched = samples whose corners were loaded.  The output
     * is bit-identical across kernel forms, layouts, launch shapes and skipping on / off.                              */
    VR_VARIANT_MIP = 8,
    VR_VARIANT_MINIP = 9,
    VR_VARIANT_AVERAGE = 10,
    /* Shaded isosurface of volume slot 0 at the level set by vr_set_iso_value (no shader of the reference; csrc/vr_iso.h).
     * Volume slot 0 holds the pre-computed gradient in .rgb (as LIGHT); TF slot 0; the light of vr_uniforms (as LIGHT).
     *   Positions: exactly BASIC's march (start, direction, stepsCount, step size, variable-step toggle, jitter, repeated rounded
     *     additions p_{k+1} = p_k + step); fragmentMode 1-4 return what BASIC returns.  The world position w is LIGHT's: w_0 = the
     *     ray's worldCoord, w_{k+1} = w_k + wstep (rounded additions), wstep = CalculateWorldStep (BasicVolLightApp.wgsl:78-84,
     *     before the variable-step override, z negated).
     *   Hit: only the steps that pass IsInSampleCoords count (they are contiguous: positions are monotone per component and the
     *     box is convex).  The hit is the first of them, k, whose d_k = textureSample(vol0, linear, p_k).a satisfies d_k >= iso
     *     (NaN samples never hit).
     *   Refinement: if k is the ray's first in-box step, q = p_k and w_q = w_k.  Otherwise d_prev = the density at p_{k-1},
     *     t = (iso - d_prev) / (d_k - d_prev) (correctly rounded f32 division); if !(t >= 0 && t <= 1) then q = p_k, w_q = w_k,
     *     else q = mad(step, t, p_{k-1}) and w_q = mad(wstep, t, w_{k-1}) per component, in the vr_set_arithmetic mode's mad
     *     (two roundings with VR_ARITH_SEPARATE, one with VR_ARITH_FUSED).
     *   Shading: s = textureSample(vol0, linear, q) (all four channels), N = normalize(s.rgb) (a zero gradient gives NaN and
     *     max(NaN, 0) leaves the ambient term only, as in LIGHT), c = the TF slot 0 colour at iso with BASIC's lookup (linear,
     *     clamp-to-edge), rgb = c * BlinnPhong(N, w_q, light, kD = 2.5, kA = 0.5) as in LIGHT, and the fragment is
     *     FrontToBackBlend((rgb, 1), dst = 0) in the blend's own arithmetic (a -0 made +0): opaque; the opacity table is not read.
     *   No hit: the pixel is (0,0,0,0).
     *   Counters: composited = the in-box steps up to and including the hit (all of them without a hit), covered = pixels whose ray
     *     hit, fetched = march-loop samples whose corners were loaded (the refinement's fetches are not counted).
     * The output, composited and covered are bit-identical across kernel forms, layouts, launch shapes and skipping on / off. */
    VR_VARIANT_ISO = 11,
    VR_VARIANT_COUNT = 12
} vr_variant;

#define VR_MAX_VOLUMES 3
#define VR_MAX_TFS 2

/*
 * Volume slots = the order of the texture_3d bindings in the scene's @group(1):
 *   BASIC / LIGHT : 0 = volume                      (BasicVolLightApp.wgsl:50)
 *   VOLUME_MASK   : 0 = mask, 1 = RT dose, 2 = CT   (VolumeMaskApp.wgsl:40-42)
 *   THREE_FILES   : 0 = CT, 1 = RT, 2 = mask (bound, never sampled) (ThreeFilesApp.wgsl:50-52)
 *   MULTI_CTRT    : 0 = CT, 1 = RT                  (MultiCTRTApp.wgsl:50-51)
 *   TF_CALIB      : 0 = CT, 1 = mask                (TFCalibrationApp.wgsl:40-41)
 *   MIP / MINIP / AVERAGE : 0 = volume (as BASIC)
 *   ISO           : 0 = volume with its gradient in .rgb (as LIGHT)
 * TF slots = the order of the (opacity, colour) texture_1d pairs:
 *   single-TF scenes (and the projections, the isosurface): 0;  two-TF scenes: 0 = CT pair, 1 = RT pair (VolumeMaskApp.wgsl:43-46).
 */

/*
 * The uniform block.  Fields 1:1 with @group(0) of every shader
 * (App/shaders/BasicVolumeApp.wgsl:26-37, filled by App/src/Application.cpp:544-556 and
 * rewritten every frame by Application::OnUpdate, App/src/Application.cpp:96-119), followed
 * by the per-scene `Light` (App/src/renderer/Light.h:9-14 <-> BasicVolLightApp.wgsl:25-33).
 */
typedef struct vr_uniforms {
    float model[16];      /* binding 0 @0   : must be identity (Application.cpp:489-492 never rewrites it) */
    float view[16];       /* binding 0 @64  : Camera::GetViewMatrix              */
    float proj[16];       /* binding 0 @128 : Camera::GetProjectionMatrix        */
    float view_inv[16];   /* binding 0 @192 : Camera::GetInverseViewMatrix       */
    float proj_inv[16];   /* binding 0 @256 : Camera::GetInverseProjectionMatrix */
    float camera_pos[3];  /* binding 1      : Camera::GetPosition                */
    int32_t fragment_mode;/* binding 4      : 0 volume, 1 |dir|, 2 start, 3 end, 4 screen uv (Application.h:191-198) */
    int32_t steps_count;  /* binding 5 */
    float step_size;      /* binding 6 */
    float clip_x[2];      /* binding 7 */
    float clip_y[2];      /* binding 8 */
    float clip_z[2];      /* binding 9 */
    int32_t toggles[4];   /* binding 10: [0] variable step, [1] jitter, [2],[3] unused */
    float light_pos[4];   /* Light.Position */
    float light_ambient[4];
    float light_diffuse[4];
} vr_uniforms;

typedef struct vr_ctx vr_ctx;

/* ---- lifetime ------------------------------------------------------------------------- */

/* Replaces: base::Window + GraphicsContext::Init + Application::Initialize{Uniforms,Textures,
 * BindGroups,RenderPipelines} (App/src/Application.cpp:58-94, 475-615).  width x height is the
 * viewport (reference default 1280x720, Application.h:100-101).  device_id = HIP ordinal.      */
int vr_create(vr_ctx** out, uint32_t width, uint32_t height, int device_id);

/* Replaces: Application::OnResize (Application.cpp:299-323) -- re-creates the per-pixel buffers. */
int vr_resize(vr_ctx* ctx, uint32_t width, uint32_t height);

void vr_destroy(vr_ctx* ctx);

/* Message of the last failing call on this ctx (ctx may be NULL: last vr_create failure). */
const char* vr_last_error(const vr_ctx* ctx);

int vr_abi_version(void);

/* ---- scene resources ------------------------------------------------------------------ */

/* Replaces: Texture::CreateFromData(..., WGPUTextureDimension_3D, size, RGBA32Float, ...)
 * (App/src/renderer/Texture.cpp:34-85) called from every MiniApp::OnStart, e.g.
 * App/src/miniapps/BasicVolLightApp.cpp:39-40.  `vec4_voxels` is VolumeFile::GetVoidPtr():
 * nx*ny*nz glm::vec4, x fastest, index z*ny*nx + y*nx + x (VolumeFile.cpp:306), .rgb = gradient
 * (or the raw value), .a = density.                                                             */
int vr_volume_upload(vr_ctx* ctx, int slot, const float* vec4_voxels, uint16_t nx, uint16_t ny, uint16_t nz);

/* Same, from a DEVICE pointer that already holds the vec4 voxels (no host round trip). */
int vr_volume_upload_device(vr_ctx* ctx, int slot, const void* d_vec4_voxels, uint16_t nx, uint16_t ny, uint16_t nz);

/* ---- data preparation on the device ------------------------------------------------------
 * The reference prepares volumes on one CPU thread at load time; these do the same arithmetic on the GPU,
 * in place on an uploaded slot, bit for bit (tests/test_prep_gpu.py).
 *
 * vr_volume_upload_raw16/32: the readers' broadcast of the raw integer to all four lanes
 *   (App/src/file/dicom/DicomReader.cpp:239,247; App/src/file/dat/DatReader.cpp:42).
 * vr_volume_normalize: VolumeFile::NormalizeData (App/src/file/VolumeFile.cpp:165-184): .a /= value;
 *   value == 0 -> the maximum of component [0] truncated to an integer (GetMaxNumber, :53-60); the value used is
 *   returned through *used_value (may be NULL).
 * vr_volume_precompute_gradient: VolumeFile::PreComputeGradient (VolumeFile.cpp:196-257): .rgb = (-(p - m)) * 0.5
 *   per axis from the +-1 neighbours' .a (0 outside the grid); norm_to_zero_one != 0 divides every component by
 *   the largest gradient magnitude.
 * vr_volume_download: reads a slot back (n voxels * 4 floats).                                               */
int vr_volume_upload_raw16(vr_ctx* ctx, int slot, const uint16_t* raw, uint16_t nx, uint16_t ny, uint16_t nz);
int vr_volume_upload_raw32(vr_ctx* ctx, int slot, const uint32_t* raw, uint16_t nx, uint16_t ny, uint16_t nz);
int vr_volume_normalize(vr_ctx* ctx, int slot, int normalization_value, int* used_value);
int vr_volume_precompute_gradient(vr_ctx* ctx, int slot, int norm_to_zero_one);
int vr_volume_download(vr_ctx* ctx, int slot, float* vec4_voxels);

/* Replaces: OpacityTF / ColorTF texture creation and TransferFunction::UpdateTexture
 * (App/src/tf/OpacityTf.cpp:25-26,134-142; App/src/tf/ColorTf.cpp:23-24).  opacity: R floats
 * (R32Float 1-D), color_rgba: 4R floats (RGBA32Float 1-D).                                       */
int vr_tf_upload(vr_ctx* ctx, int slot, const float* opacity, const float* color_rgba, uint32_t resolution);

/* The two textures of a pair are separate objects in the reference and may differ in resolution (OpacityTF::Load
 * re-resolves only its own, OpacityTf.cpp:298): upload one table of a slot without touching the other.       */
int vr_tf_upload_opacity(vr_ctx* ctx, int slot, const float* opacity, uint32_t resolution);
int vr_tf_upload_color(vr_ctx* ctx, int slot, const float* color_rgba, uint32_t resolution);

/* Stream-ordered table edits (the reference's wgpuQueueWriteTexture, App/src/renderer/Texture.cpp:87-95): what an editor
 * calls every frame.  Arguments and validation as vr_tf_upload_opacity / _color; `stream` is a hipStream_t, NULL = the
 * context's own stream.
 *  - Copied on call: the table has been copied when the call returns; the caller may reuse or free its array at once.
 *  - Ordered: every render entry point enqueued after the call returns uses the new table, on any stream, and so do its
 *    empty-space skipping state and its counters.  Everything enqueued before the call keeps the old table, whatever its
 *    stream.  A launch on another stream than the edit's waits for the edit once (a device-side wait, one per stream
 *    per edit).
 *  - Non-blocking: neither the call nor the next render that picks the edit up waits for the device, with one
 *    exception: a call blocks the host while EIGHT earlier asynchronous edits are still being copied (the context stages
 *    edits in eight pinned buffers, used in turn).  Each table keeps FOUR device generations; a generation is rewritten
 *    on the device behind the last launch that read it, never by a host wait.  An opacity edit of slot 0 that moves the
 *    table's zero prefix or changes its resolution rebuilds the empty-space distance field on `stream` as well; until its
 *    active-brick box has reached the host, launches prune with no box (same bits, vr_unbounded_box_launches).  A
 *    resolution change may allocate; what it replaces is freed by the next call that drains the device.
 *  - The synchronous uploads, the volume uploads, vr_resize and vr_destroy still drain the device first, and with it
 *    every asynchronous edit made before them.                                                                      */
int vr_tf_upload_opacity_async(vr_ctx* ctx, int slot, const float* opacity, uint32_t resolution, void* stream);
int vr_tf_upload_color_async(vr_ctx* ctx, int slot, const float* color_rgba, uint32_t resolution, void* stream);

/* Replaces: the 12 wgpuQueueWriteBuffer calls of Application::OnUpdate (Application.cpp:96-119)
 * plus the scene's Light uniform (BasicVolLightApp.cpp:42).  Returns VR_ERR_UNSUPPORTED when
 * `model` is not the identity (the reference never uploads anything else).                       */
int vr_set_uniforms(vr_ctx* ctx, const vr_uniforms* u);

/* ---- the hot path --------------------------------------------------------------------- */

/* Replaces: the "ray end" pass + the volume pass of Application::OnRender
 * (Application.cpp:150-220): analytic ray/box set-up (rayCoords.wgsl + rasteriser) and the
 * fs_main compositing loop of the chosen shader, for every pixel.  Synchronous on return.       */
int vr_render(vr_ctx* ctx, int variant);

/* Image-tile partition (multi-GPU, one process per GPU): renders only the 64x64 screen tiles t
 * with (t % world) == rank, t = ty * tiles_x + tx, and stores them packed, tile after tile in
 * increasing t, each tile as 64*64 RGBA32F row-major (pixels outside the viewport = 0).
 * The packed buffer is `vr_tile_count(ctx, rank, world) * 64*64*4` floats.                       */
int vr_render_tiles(vr_ctx* ctx, int variant, int rank, int world);
int vr_tile_count(const vr_ctx* ctx, int rank, int world);

/* Asynchronous forms: enqueue on `stream` (a hipStream_t, NULL = the ctx's own stream) and write
 * to DEVICE memory supplied by the caller; nothing is synchronised.  `d_frame` = W*H*4 floats;
 * `d_tiles` as described above.  These are what a multi-rank host (RCCL gather) drives.
 * Up to FOUR renders may be in flight at a time, each on its own stream and into its own buffer (use
 * them in turn): the next frame fills the machine while the previous one's longest rays drain (two in
 * flight give 1.45x the frame rate of one on C3, three 1.5x).  What is enforced is EIGHT launches: a
 * ninth enqueue blocks the calling thread until the oldest of the eight has finished (each launch owns
 * one of eight record buffers, guarded by an event), so a caller that keeps four frames in flight never
 * waits for its oldest launch inside an enqueue.  vr_volume_upload*, vr_volume_normalize / _gradient,
 * vr_tf_upload, vr_tf_upload_opacity / _color, vr_resize and vr_destroy drain the whole device first, so they are
 * safe to call while asynchronous renders are still in flight on the caller's streams; the asynchronous table edits
 * (vr_tf_upload_opacity_async / _color_async) are ordered on a stream instead and drain nothing.                */
int vr_render_async(vr_ctx* ctx, int variant, void* d_frame, void* stream);

/* Streams for frames in flight.  HIP maps streams onto a few hardware queues, and two streams that share a queue run
 * their kernels one after the other -- two frames "in flight" on such a pair gain nothing (measured: 0.60 instead of 0.48 ms
 * per C3 frame).  vr_stream(ctx, i), i = 0..3, returns context-owned streams (hipStream_t) that were probed, on first use,
 * to really run side by side (two 150 us single-wavefront kernels; ~3 ms once); fewer than four may exist, then the index
 * wraps.  Use them in turn for vr_render_async / vr_render_tiles_async; NULL on failure.                              */
void* vr_stream(vr_ctx* ctx, int index);

/* Hint: how many frames the caller keeps in flight on different streams (1 = one at a time, the default; up to 4).  It only
 * steers the default choice of lanes per ray (vr_set_kernel_flavour(0)): frames that overlap fill the machine together, so
 * the throughput-optimal one-lane kernel is preferred earlier than for a frame that has the machine to itself.  Results do
 * not depend on it.                                                                                                    */
int vr_hint_frames_in_flight(vr_ctx* ctx, int frames);
int vr_render_tiles_async(vr_ctx* ctx, int variant, int rank, int world, void* d_tiles, void* stream);

/* Root side of the gather: `d_gathered` holds, for r = 0..world-1, rank r's packed tiles, each
 * rank's segment padded to `tiles_per_rank_max * 64*64*4` floats; scatters them back into the
 * W*H*4 frame `d_frame` (device).                                                                */
int vr_unpack_tiles_async(vr_ctx* ctx, const void* d_gathered, int world, void* d_frame, void* stream);

/* Several frames in ONE launch.  Replaces: nothing in the reference (it renders one frame per OnRender,
 * App/src/Application.cpp:121-239); this is the throughput form for callers that know the next frames' cameras
 * (turntables, offline sequences, and above all a multi-GPU run, where one rank's share of a frame is a launch far too
 * short to fill a GPU: a rank's eighth of the 1080p frame keeps 9 % of the wavefront slots busy).  n_frames = 1 .. 4
 * frames of the SAME scene (the volumes and tables currently bound) are marched by one grid -- frame f with
 * uniforms[f] into d_frames[f] / d_tiles[f] (device, each W*H*4 floats / packed tiles as above).  The context's own
 * uniforms (vr_set_uniforms) are neither used nor changed.  Every frame is bit-identical to what vr_render_async
 * would have produced with the same uniforms; vr_last_counters reports the LAST frame of the launch.  One launch counts
 * as one render in flight.                                                                                        */
int vr_render_batch_async(vr_ctx* ctx, int variant, int n_frames, const vr_uniforms* uniforms, void* const* d_frames, void* stream);
int vr_render_tiles_batch_async(vr_ctx* ctx, int variant, int rank, int world, int n_frames, const vr_uniforms* uniforms,
                                void* const* d_tiles, void* stream);

/* vr_unpack_tiles_async for gathered segments that lie `rank_stride_tiles` tiles apart (>= a segment) instead of back to
 * back: after gathering n frames' segments at once rank r's tiles of frame f start at
 * d_gathered + ((r * n + f) * tiles_per_rank_max) * 64*64*4 floats, so frame f is unpacked from the base of ITS first
 * segment with rank_stride_tiles = n * tiles_per_rank_max.                                                        */
int vr_unpack_tiles_strided_async(vr_ctx* ctx, const void* d_gathered, int world, int rank_stride_tiles, void* d_frame, void* stream);

/* Replaces: reading back the colour attachment.  frag_rgba (W*H*4 floats, may be NULL) receives
 * the fragment shader output `dst` per pixel BEFORE output merge; pixels with no fragment = 0.
 * present_bgra8 (W*H*4 bytes, may be NULL) receives the presented pixel: blend
 * SrcAlpha/OneMinusSrcAlpha over the white background quad, BGRA8Unorm
 * (App/src/renderer/PipelineBuilder.cpp:142-147, App/shaders/fullscreen.wgsl:33-41,
 * NativeGraphicsContext.cpp:118).  composited_samples (may be NULL) = number of loop iterations
 * whose blend executed, summed over the pixels rendered by the last render call.                 */
int vr_download(vr_ctx* ctx, float* frag_rgba, uint8_t* present_bgra8, uint64_t* composited_samples);

/* Presentation without a host round trip.  Replaces: the output merge + swap-chain present of Application::OnRender
 * (App/src/Application.cpp:180-233: blend SrcAlpha/OneMinusSrcAlpha over the white background quad into the BGRA8Unorm
 * swap-chain image) for a caller that shows the frame itself: writes the presented BGRA8Unorm pixels of the device frame
 * `d_frame` (W*H*4 floats; NULL = the ctx-owned frame of vr_render) into DEVICE memory `d_bgra8` (W*H*4 bytes) on `stream`
 * (NULL = the ctx's own) -- e.g. a GL / Vulkan buffer or texture staging buffer imported into HIP
 * (hipGraphicsGLRegisterBuffer + hipGraphicsResourceGetMappedPointer, or hipImportExternalMemory).  Nothing is
 * synchronised; the same arithmetic as vr_download's present_bgra8.                                               */
int vr_present_async(vr_ctx* ctx, const void* d_frame, void* d_bgra8, void* stream);

/* vr_present_async for the root of a multi-GPU gather: presents straight from the gathered, tile-major segments
 * (layout as vr_unpack_tiles_strided_async; rank_stride_tiles <= 0 = segments back to back) into `d_bgra8` (W*H*4 bytes,
 * row-major), so a viewer that only wants the presented frame needs no un-permuted float frame in between.  Replaces the
 * same output merge (App/src/renderer/PipelineBuilder.cpp:142-154); bit-identical to vr_unpack_tiles_async + vr_present_async. */
int vr_present_tiles_async(vr_ctx* ctx, const void* d_gathered, int world, int rank_stride_tiles, void* d_bgra8, void* stream);

/* Presenting where the tiles are rendered (multi-GPU, the presented frame alone is wanted): vr_present_packed_async applies the same
 * output merge to a rank's PACKED tiles (n_tiles x 64 x 64 RGBA32F -> as many BGRA8Unorm words, same order) -- the gather then moves
 * 4 bytes per pixel instead of 16 -- and vr_unpack_tiles_bgra8_async is vr_unpack_tiles_strided_async for such gathered BGRA8 tiles
 * (gathered[r][n][64*64] words -> the W x H frame).  Pixel for pixel the bytes of vr_present_async on the assembled frame.     */
int vr_present_packed_async(vr_ctx* ctx, const void* d_tiles_rgba, int n_tiles, void* d_tiles_bgra8, void* stream);
int vr_unpack_tiles_bgra8_async(vr_ctx* ctx, const void* d_gathered_bgra8, int world, int rank_stride_tiles, void* d_bgra8, void* stream);

/* Packed tiles of the last vr_render_tiles (host copy). */
int vr_download_tiles(vr_ctx* ctx, float* tiles_rgba, uint64_t* composited_samples);

/* ---- instrumentation ------------------------------------------------------------------ */

/* HIP-event time of the last synchronous render's (vr_render / vr_render_tiles) march kernel and of
 * the whole render call, in milliseconds; VR_ERR_NOT_READY after an *_async render (those are timed by
 * vr_kernel_times alone).  Replaces the FPS / frame-time read-out (Application.cpp:339-370). */
int vr_last_timing(vr_ctx* ctx, float* kernel_ms, float* total_ms);

/* Durations (ms) of the march launches of the most recent render calls, oldest first: first workgroup start to last
 * workgroup end on the 100 MHz device clock, taken from the launch's own per-workgroup records by the small kernel that
 * sorts them (two timing events around every launch cost the frame's stream 11 us: 2 % of a 1080p frame, 8 % of a
 * 1024^2 unlit one); launches without a sort behind them (LDS-tile flavours, > 192 K workgroups) are timed with HIP events
 * on their stream.  At most `capacity` (<= 256) values are written, the number written is returned (negative = error).
 * Waits for the launches concerned.  vr_reset_kernel_times() empties the ring: the launches before it are reported no more
 * (the measured kernel choice keeps reading their records: a reset does not disturb a running trial).                  */
int vr_kernel_times(vr_ctx* ctx, float* out_ms, int capacity);

/* How vr_kernel_times measures: VR_TIMING_RECORDS (default, as described above) or VR_TIMING_EVENTS -- a pair of HIP events
 * around every march launch on the stream it is enqueued on, whatever the launch (what bench.py's roofline divides by).  */
#define VR_TIMING_RECORDS 0
#define VR_TIMING_EVENTS 1
int vr_set_kernel_timing(vr_ctx* ctx, int mode);
int vr_reset_kernel_times(vr_ctx* ctx);

/* Viewport size and HIP device ordinal of a context (any pointer may be NULL). */
int vr_viewport(const vr_ctx* ctx, uint32_t* width, uint32_t* height, int* device_id);

/* Device pointer of the ctx-owned frame buffer (W*H*4 floats) written by vr_render. */
void* vr_frame_device_ptr(vr_ctx* ctx);

/* Number of pixels that produced a fragment in the last render (front face hit & not clipped). */
int vr_last_covered_pixels(vr_ctx* ctx, uint64_t* covered);

/* Counters of the last render: out[0] = composited samples (blends the reference's loop executes),
 * out[1] = covered pixels, out[2] = samples whose voxels were actually fetched (= out[0] minus the
 * samples the exact empty-space test proved to be the identity).                                 */
int vr_last_counters(vr_ctx* ctx, uint64_t out[3]);

/* Per-workgroup trace of the last march launch, for load-balance analysis: 6 words per workgroup
 * {composited samples, covered pixels, fetched samples, start, end (100 MHz device clock), HW_ID | XCC_ID << 32},
 * in blockIdx order.  Writes min(capacity, n) records and returns n (the number of workgroups launched).      */
int vr_last_block_trace(vr_ctx* ctx, uint64_t* out, int capacity);

/* Kernel flavour for A/B measurements.  All flavours are bit-identical in output and in the composited / covered counts; the
 * FETCHED count (vr_last_counters out[2]) is the same for all but 1 and 16, which skip nothing and fetch every composited sample
 * -- the default may pick 16 for volumes with next to nothing to skip, so `fetched` can differ between frames of one scene.
 * 2, 3, 4, 5, 9 and 14 were forms that lost every A/B and have been removed (HISTORY.md): VR_ERR_UNSUPPORTED.
 *   0  default: a MEASURED choice.  Every form below gives the same bits, so the context tries the eligible ones on the
 *      caller's own frames and keeps the fastest by the launches' own records (no synchronisation: the sort behind a launch
 *      writes its duration and its end to pinned memory).  Per "what is launched of what": shader, rank share, viewport, frames
 *      per launch, vr_hint_frames_in_flight, volume / table uploads, arithmetic, layout.  The rules (csrc/vr_tuner.h, pinned by
 *      tests/test_tuner.py), with f = the frames-in-flight hint:
 *        - a shape with one eligible form runs it and is not measured; launches that cannot be measured (VR_TIMING_EVENTS) run
 *          the first candidate and count for nothing;
 *        - f + 3 launches of the first candidate (the prior's pick) come first, so that a launch order exists; then every
 *          candidate in turn gets 3 launches (f = 1) or 3 f + 2 (f > 1); then the first candidate runs until the last of those
 *          launches has reported, and the choice is made once;
 *        - a candidate's cost, f = 1: the shortest span (first workgroup start to last workgroup end) of its launches but the
 *          first; f > 1: the mean interval between the ends of its launch number f and its launch number 3 f + 2 - f (counted
 *          from 0), f + 2 intervals that are its alone -- ends that do not advance make the candidate unusable;
 *        - another kernel replaces the first candidate only below 0.98 times its cost (0.95 with f > 1); between the others
 *          the strictly smaller cost wins;
 *        - a trial one of whose launches has not reported 64 launches after its last, or whose launches spread over 256 launches
 *          or more (vr_kernel_times' ring), keeps the first candidate and reports no costs;
 *        - the trial re-opens when the longest ray chain + 1 of the scene (c now, r when the choice was made, both known) has left
 *          [r - r / 4, r + r / 4] in integers; the kernel kept runs first in the new trial, and while it settles;
 *        - a changed set of eligible forms under the same key starts a fresh trial from the prior's pick; a new key of a shape
 *          (the key without uploads, arithmetic, layout) starts from what the most recently used decided trial of that shape
 *          kept, if that is still eligible;
 *        - eight trials are remembered, the least recently used one makes room.
 *      A trial names its launches by the context's count of march launches, which nothing rewinds: vr_reset_kernel_times in the
 *      middle of a trial changes neither the choice nor the costs.  A rank's share without a tile launches nothing and is no part
 *      of any trial.  Candidates: the prior's pick (exact skipping; whole one-at-a-time frames of
 *      the lit / unlit shader and the composite: 17, or 16 with nothing to skip; else lanes per ray from the launch size, the
 *      frames in flight and the chain length of an earlier launch), 17 / 16, 6, 18, and 10 / 11 (launches that leave the machine
 *      part empty) or 12.  vr_kernel_choice reports what was measured.  VR_EXP_TUNE=0 in the environment: the prior alone.
 *   1  one lane per ray, no empty-space skipping (every composited sample is fetched)
 *   6  one lane per ray (forced), 7  four lanes per ray (forced), 8  two lanes per ray (forced)
 *   10 / 11  four / two lanes per ray with the next round's corner loads software-pipelined (lit shader; what
 *      the default uses for small launches)
 *   12 / 13  persistent wavefronts (csrc/vr_pw.h): one workgroup of 16 wavefronts per CU, the packets come from a queue
 *      (eight heads, longest chains first), TF slot 0 is read from LDS; 13 also issues the next step's corner loads before
 *      this step's shading (lit / unlit shader).  Launches of one frame; fewer bytes through the texture addressers
 *   16 / 17  persistent wavefronts with the corner loads TWO steps ahead (csrc/vr_p2.h): two corner buffers, the gather an indexed
 *      buffer load of the voxel's slot in the bricked copy, the slot arithmetic of a cell from per-axis tables in LDS beside TF
 *      slot 0.  16 skips nothing (volumes with nothing to skip; 2 wavefronts per SIMD); 17 decides the exact empty-space skipping
 *      ahead of the loads (one distance-field byte per ray rides along with each corner buffer; idle rays' lanes are switched off
 *      for the loads; runs of identity steps become jumps of the requests while the steps in flight are consumed; 3 per SIMD).
 *      Lit / unlit shader and (17; 16 runs as 17) the three-volume composite, whose mask and dose are fetched on demand behind the
 *      per-brick mask record; volumes of 4 GiB and more through a window of z-slabs of bricks that follows the packet; launches of
 *      several frames take (frame, packet) items from the one queue.  Needs one table resolution <= 8190 and the bricked copy
 *      (vr_set_volume_layout(0)), and a volume whose axis tables fit the workgroup's LDS beside TF slot 0:
 *          (opacity resolution + 2) * 16 + (nx + ny + nz + 3) * 8  <=  160 KiB
 *      (a 64-entry table: nx + ny + nz <= 20345), a z-slab of storage bricks below 2^24 voxels and a bricked copy below 2^32
 *      voxels; else 13 / 12, or 6 for launches of several frames
 *   18  the one-lane kernel (6) with the slot arithmetic of volume 0's cells from per-axis tables in its workgroup's LDS (the
 *      clamp-to-edge texel pair of a coordinate is one ds_read2_b32; filled per workgroup, by the workgroups that can hit the box);
 *      the shaders that sample one volume (lit, unlit, in-shader gradient) on the bricked copy, launches of any number of frames,
 *      a volume whose tables fit 32 KiB of LDS:
 *          (nx + ny + nz + 6) * 4  <=  32 KiB            (nx + ny + nz <= 8186)
 *      and a bricked copy below 2^32 voxels; else it runs as 6
 *   15  the voxels of a packet's next four steps in an LDS tile filled by LDS-DMA (csrc/vr_lt.h): lit shader, launches of
 *       one frame (other launches run 6); never picked by the default -- slower than 17 / 16 wherever measured
 * THE BRICK-INDEX LIMIT.  Every skipping form finds the record of a step's brick (4^3 cells) with 24-bit multiplies and a 32-bit
 * byte offset.  With bn = ceil(n / 4) bricks per axis that is exact for
 *          bny * bnz <= 2^23,   bnx < 2^23   and   bnx * bny * bnz <= 2^29
 * (vr_skip_indexable).  Every cube up to 3248 voxels an axis is inside -- more than a device holds --; thin, long volumes are
 * what leaves it: (1, 8192, 16384) is the last shape of its kind inside, (1, 8196, 16384) the first outside.  A volume beyond
 * the limit is rendered all the same: its launches do not skip -- the skipping flavour of a pair (17; 19, 21, 23, 25, 27; the
 * slices) runs as the pair's other form, every counted sample is fetched, the outputs are the same bits -- and vr_skip_field
 * returns VR_ERR_NOT_READY.  The histogram and the region growing index their records with 64 bits and keep settling units
 * from them.
 * The projections (MIP / MINIP / AVERAGE) have forms of their own, reported by vr_last_kernel_flavour and never measured against
 * each other (vr_kernel_choice reports 0 candidates after a projection launch):
 *   19  march_proj_kernel with exact skipping (csrc/vr_proj.h): a step whose brick cannot change the result loads nothing
 *       (MIP: brick max <= m, MINIP: brick min >= m, AVERAGE: every voxel of the brick +-0), and MIP / MINIP stop loading once
 *       m has reached the volume's maximum / minimum.  Flavour 0 runs as 19, and so does every other flavour but 1.
 *   20  march_proj_kernel without skipping: every counted sample is fetched.  Flavour 1 runs as 20.
 * The isosurface (ISO) likewise (0 candidates after an ISO launch):
 *   21  march_iso_kernel with exact skipping (csrc/vr_iso.h): a step whose brick's maximum density is below the level loads
 *       nothing.  Flavour 0 runs as 21, and so does every other flavour but 1.
 *   22  march_iso_kernel without skipping: every in-box step up to the hit is fetched.  Flavour 1 runs as 22.
 * LIGHT with shadows on (vr_set_shadows) likewise (0 candidates after such a launch; nothing is measured against LIGHT's forms):
 *   23  march_shadow_kernel and shadow_build_kernel with exact skipping by LIGHT's distance field (csrc/vr_shadow.h): a step in
 *       an inert brick loads nothing, in the march and in the light volume's build, and a blended sample of opacity exactly 0
 *       is not shaded.  Flavour 0 runs as 23, and so does every other flavour but 1.  (When LIGHT would not skip -- a
 *       non-finite colour table or light, no zero prefix of the opacity table -- 23 runs 24's kernels.)
 *   24  both without skipping: every in-box step up to the cut-off is fetched and shaded.  Flavour 1 runs as 24.
 * BASIC / LIGHT with surface output (vr_set_output) likewise (0 candidates after such a launch; ISO's surface launches keep 21 / 22):
 *   25  march_surf_kernel with exact skipping by BASIC's distance field (csrc/vr_surf.h): a step in an inert brick loads nothing
 *       and leaves the accumulated alpha as it is.  Flavour 0 runs as 25, and so does every other flavour but 1.  (Without a zero
 *       prefix of the opacity table 25 runs 26's kernels; the colour table and the light play no part.)
 *   26  march_surf_kernel without skipping: every in-box step up to the hit is fetched.  Flavour 1 runs as 26.
 * BASIC / LIGHT between ray bounds (vr_set_ray_bounds) likewise (0 candidates after such a launch):
 *   27  march_bound_kernel with exact skipping by the variant's distance field (csrc/vr_bound.h): a step in an inert brick loads
 *       nothing and a sample of opacity exactly 0 is not shaded, whether the step counts or not.  Flavour 0 runs as 27, and so does
 *       every other flavour but 1.  (When the variant would not skip -- a non-finite colour table or light, no zero prefix of the
 *       opacity table -- 27 runs 28's kernels.)
 *   28  march_bound_kernel without skipping: every counted step up to the cut-off is fetched and shaded.  Flavour 1 runs as 28.
 *       Both are one-lane kernels: on a whole unbounded frame they are slower than 17.                                       */
int vr_set_kernel_flavour(vr_ctx* ctx, int flavour);

/* What the default's measured choice (flavour 0) knows about the launch shape it was asked for last: the candidates' flavours, the
 * milliseconds per launch measured for each (0 = its trial has not been evaluated yet) and the index of the one kept (-1 = trial
 * running: the prior's pick, flavours[0], runs meanwhile).  Returns the number of candidates (0: nothing launched through the
 * default yet, or the shape has a single eligible form).                                                               */
int vr_kernel_choice(vr_ctx* ctx, int flavours[6], float ms_per_launch[6], int* chosen);

/* Arithmetic mode.  WGSL leaves it to the implementation whether `a * b + c` is evaluated with one rounding or two
 * (the reference's Tint -> HLSL -> D3D12 back end emits `mad`).
 *   VR_ARITH_SEPARATE (default)  product and sum are rounded separately everywhere: bit-exact with the oracle's default mode
 *   VR_ARITH_FUSED               the per-sample expressions of that shape -- texture coordinates p * N - 0.5, every
 *                                linear-filter lerp a + (b - a) * t, dot products, light.diffuse * m * kD + light.ambient * kA,
 *                                the CT / RT colour mix and FrontToBackBlend -- are single fused multiply-adds: bit-exact with
 *                                the oracle's fused mode, about a fifth fewer vector instructions per sample.  Ray placement
 *                                (matrices, slab test, step vectors, p += step) is identical in both modes.
 * In full: a table look-up's coordinate d * R - 0.5 is a texture coordinate; a dot product is mad(a.z, b.z, mad(a.y, b.y, a.x * b.x)),
 * and the sum of squares under a per-sample normalize (the gradient, lightPos - w) is that dot product; the shading sum is
 * mad(dif_c * m, kD, amb_c * kA) and the blend mad(1 - dst.a, c * a, dst.c), their inner products dif_c * m, amb_c * kA, c.rgb * a
 * rounded on their own in both modes, like rgb * shade, 1 - dst.a, the scale 1 / sqrt and the coordinate's fraction x - floor(x).
 * The feature marches follow the same rule -- a per-sample expression of the shape a * b + c is fused, placement is not -- and
 * their sections name the expressions: ISO's and the surface's refinement mads and the surface's alpha line are fused; w += wstep,
 * sigma and g(d) of the ray bounds, the light volume's walk (D, len, dir, step, lim, q += step), s * a, T * (1 - a'), m * S, the t
 * divisions and AVERAGE's s + d and s / n are not.                                                                       */
#define VR_ARITH_SEPARATE 0
#define VR_ARITH_FUSED 1
int vr_set_arithmetic(vr_ctx* ctx, int mode);

/* Threshold of VR_VARIANT_ISO for launches enqueued after this call (default 0.5f).  Finite values only:
 * NaN / +-inf -> VR_ERR_INVALID_ARG, the previous value stays. */
int vr_set_iso_value(vr_ctx* ctx, float iso);

/* Shadows of the lit shader (VR_VARIANT_LIGHT only; every other variant ignores the setting).  grid_divisor 0 = off (default):
 * LIGHT is exactly what it was.  1, 2, 4 or 8 = one light-volume texel per divisor^3 voxels.  opacity_scale: finite and >= 0.
 * Otherwise VR_ERR_INVALID_ARG, and the previous setting stays.  Applies to launches enqueued after the call (captured at enqueue,
 * as vr_set_iso_value is).
 *
 * Light volume.  Inputs: volume slot 0 (nx, ny, nz), divisor r and scale s = opacity_scale, the launch's light_pos L and its clip
 * bounds bmin / bmax (IsInSampleCoords), TF slot 0's opacity table as the launch captured it, the context's arithmetic mode.
 *   Grid G = (ceil(nx/r), ceil(ny/r), ceil(nz/r)), x fastest.  Light in texture space l = (L.x + 0.5f, L.y + 0.5f, 0.5f - 2.0f * L.z)
 *   (setup_ray's world-to-uvw map of the box).  Step length h = 1.0f / (float)max(Gx, Gy, Gz).  Texel centre
 *   c = (((float)i + 0.5f) / (float)Gx, ...).  D = l - c, len = length3s(D), dir = normalize3s(D), step = dir * h (ray-placement
 *   forms: separately rounded in both arithmetic modes).  lim = len / h, K = lim < 65536.0f ? (int)lim : 65536 (NaN: 65536).
 *   T = 1.0f, q = c; for k = 1..K: q = q + step (a rounded addition per component); stop if any component of q is < 0, > 1 or
 *   NaN; if q is inside the clip box: d = BASIC's trilinear .a fetch at q, a = BASIC's opacity look-up of d, a' = s * a,
 *   a' = a' > 1 ? 1 : a', a' = a' > 0 ? a' : 0 (NaN -> 0), T = T * (1.0f - a'); stop if T < 0x1p-10f (T is kept as it is).
 *   The texel stores T.  The texture-coordinate and lerp expressions follow the arithmetic mode, as every per-sample expression.
 * Shadowed march: exactly LIGHT -- positions, world positions, variable step, jitter, the cut-off dst.a < 1.0, fragment modes
 *   1-4, the blend and the counters -- except in each blended sample's shading: S = the light volume sampled at the sample's uvw
 *   position p with the density sampler's texel pairs and lerps (linear, clamp-to-edge; the arithmetic mode's form), and the
 *   diffuse term dif_c * m of the shading becomes dif_c * (m * S), m * S rounded first.  `fetched` counts volume samples only.
 *   Consequences: s = 0 gives T == 1 everywhere, lerps of a constant grid are exact, m * 1 = m: a shadowed frame at s = 0 is
 *   bit-identical to LIGHT's in both arithmetic modes.  A build step in an inert brick of LIGHT's distance field has opacity
 *   exactly 0 and leaves T as it is: the skipping build (flavour 23) loads nothing there and stores the same texels.
 * The context keeps the light volumes of the last 4 keys (volume, opacity table, light, clip box, divisor, scale, arithmetic
 * mode); a launch whose key has none builds it on its own stream first, behind the launches still reading the entry it reuses.
 * Every frame of a batched launch must have the same key (VR_ERR_UNSUPPORTED otherwise); a light volume of 4 GiB or more is
 * VR_ERR_UNSUPPORTED, a failed allocation VR_ERR_OOM: nothing is enqueued in either case.  vr_last_timing's total_ms includes a
 * build the render enqueued, its kernel_ms and vr_kernel_times do not (the march alone). */
int vr_set_shadows(vr_ctx* ctx, int grid_divisor, float opacity_scale);

/* The light volume that a LIGHT launch enqueued now would read (the context's uniforms).  It is built if needed, synchronously, and
 * the call drains the device, like vr_skip_field.  Copies min(capacity, n) floats in x-fastest order, writes the grid to dims[3]
 * and returns n.  VR_ERR_NOT_READY when shadows are off, volume 0 / TF 0 are missing or no uniforms were set. */
int vr_shadow_volume(vr_ctx* ctx, float* out, size_t capacity, int dims[3]);

/* ---- surface positions: first-hit position, depth, picking --------------------------------------------------------------
 * What a launch writes.  VR_OUTPUT_COLOR (default): every launch is exactly what it is without this setting.  VR_OUTPUT_SURFACE:
 * the launches of VR_VARIANT_BASIC, VR_VARIANT_LIGHT and VR_VARIANT_ISO write surface positions instead of colour, through every
 * launch shape (synchronous, asynchronous, tiles, several frames per launch); every other variant returns VR_ERR_UNSUPPORTED and
 * enqueues nothing.  Applies to launches enqueued after the call (captured at enqueue, as vr_set_iso_value is).  The frame is
 * W*H*4 floats as ever.
 *
 * Surface output of BASIC and LIGHT (volume slot 0, TF slot 0's opacity table alone; both variants give the same bits: they share
 * their sample positions).  tau = the threshold of vr_set_surface_threshold when the launch was enqueued.
 *   Positions: exactly BASIC's march (start, direction, stepsCount, step size, variable-step toggle, jitter, repeated rounded
 *     additions p_{k+1} = p_k + step); fragmentMode 1-4 return what BASIC returns.
 *   Accumulation: a = +0.  For each step that passes IsInSampleCoords, while a <= tau: d = BASIC's trilinear .a fetch at the step,
 *     o = BASIC's opacity look-up of d (linear, clamp-to-edge), a_prev = a, a = mad(1 - a, o, a) -- the alpha line of
 *     FrontToBackBlend, in the vr_set_arithmetic mode's mad.  The variant's own cut-off (0.95 / 1.0) plays no part.
 *   Hit: the first in-box step k after whose blend a > tau.  A NaN a ends the loop and is no hit.
 *   Refinement (the isosurface's rule, on alpha): if k is the ray's first in-box step, q = p_k.  Otherwise
 *     t = (tau - a_prev) / (a - a_prev) (correctly rounded f32 division); if !(t >= 0 && t <= 1) then q = p_k, else
 *     q = mad(step, t, p_{k-1}) per component in the arithmetic mode's mad.
 *   Pixel: hit -> (q.x, q.y, q.z, a); ray through the box without a hit -> (0, 0, 0, a) with the final a; no ray -> (0, 0, 0, 0).
 *     So a pixel is a hit exactly when .w > tau; at tau = 0.95f the .w plane is BASIC's alpha plane bit for bit, at
 *     tau = 0x1.fffffep-1f LIGHT's.
 *   Counters: composited = the in-box steps up to and including the hit (all of them without one; a NaN a ends the count at its
 *     step), covered = pixels with a hit, fetched = samples whose corners were loaded.  In fragmentMode 1-4 all three are 0.
 *   Shadows (vr_set_shadows) are ignored: no light volume is built or read.
 * Surface output of ISO: hit -> (q.x, q.y, q.z, 1.0f) with q the refined point of VR_VARIANT_ISO's definition above; no hit -> zeros.
 *   Counters as ISO's.
 * The output, composited and covered are bit-identical across layouts, launch shapes and skipping on / off (flavours 25 / 26). */
#define VR_OUTPUT_COLOR 0
#define VR_OUTPUT_SURFACE 1
int vr_set_output(vr_ctx* ctx, int mode);

/* The alpha threshold of BASIC / LIGHT surface launches enqueued after this call (default 0.5f).  Finite, 0 <= tau < 1; otherwise
 * VR_ERR_INVALID_ARG and the previous value stays. */
int vr_set_surface_threshold(vr_ctx* ctx, float tau);

/* The depth a rasteriser drawing at the surface points would write: d_surface = a surface frame (W*H*4 floats, device), d_depth =
 * W*H floats (device), on `stream` (NULL = the ctx's own); nothing is synchronised.  Uses the view and proj matrices of the context's
 * uniforms and the threshold of vr_set_surface_threshold AT THIS CALL (not those of the launch that wrote the frame).  Per pixel s:
 * !(s.w > tau) -> 1.0f (an ISO frame's .w is 1 or 0).  Otherwise w = (s.x - 0.5f, s.y - 0.5f, (0.5f - s.z) * 0.5f) -- the inverse
 * of the ray set-up's world-to-uvw map --, e = view * (w, 1), c = proj * e, both with the column-major, left-to-right-summed product
 * of the ray set-up (separately rounded in both arithmetic modes), depth = c.z / c.w.  VR_ERR_NOT_READY before vr_set_uniforms. */
int vr_surface_depth_async(vr_ctx* ctx, const void* d_surface, void* d_depth, void* stream);

/* What is under a pixel.  hit = 0: every other field but alpha is 0 and depth is 1.0f. */
typedef struct vr_pick_result {
    int32_t hit;       /* the pixel's .w > tau                                                              */
    float uvw[3];      /* the surface point q in texture space                                              */
    float world[3];    /* (q.x - 0.5f, q.y - 0.5f, (0.5f - q.z) * 0.5f)                                     */
    float depth;       /* as vr_surface_depth_async                                                         */
    float alpha;       /* the pixel's .w                                                                    */
    int32_t voxel[3];  /* clamp((int)floor(uvw * n), 0, n - 1) of volume slot 0                             */
    float value[VR_MAX_VOLUMES][4]; /* the vec4 voxel there of every uploaded slot whose size equals slot 0's; else zeros */
} vr_pick_result;

/* Renders the surface pixel (x, y) of `variant` (BASIC, LIGHT or ISO; others VR_ERR_UNSUPPORTED) with the context's uniforms and
 * threshold into a buffer of its own -- whatever vr_set_output says --, drains the device (as vr_skip_field does) and fills *out.
 * The context's frame (vr_download), vr_last_counters, vr_last_kernel_flavour, vr_last_timing, vr_kernel_times and the measured
 * kernel choice stay what the render before the pick left: a pick between a render and its download is the normal use.
 * A pixel outside the viewport is VR_ERR_INVALID_ARG. */
int vr_pick(vr_ctx* ctx, int variant, uint32_t x, uint32_t y, vr_pick_result* out);

/* ---- per-pixel ray bounds: the colour march between two caller depth buffers ----------------------------------------------
 * d_near and d_far are device pointers to W*H floats each, row-major, pixel (px, py) at py*W + px.  NULL = no bound on that side;
 * both NULL = off (default): every launch is exactly what it is without this setting.  The buffers stay the caller's, as the d_frame
 * of vr_render_async does.  The pointers are captured when a launch is enqueued (as vr_set_iso_value is); the kernel reads the
 * contents in stream order: the caller writes the buffers on the launch's stream, or orders them before it.  vr_resize turns the
 * bounds off (the buffers no longer fit); nothing else changes them.  A depth value means exactly what vr_surface_depth_async
 * writes: clip.z / clip.w of proj * view * (world, 1) with the context's matrices -- a rasteriser's depth attachment under the same
 * matrices, or the depth of a surface frame of this library.
 *
 * Applies to the colour launches of VR_VARIANT_BASIC and VR_VARIANT_LIGHT (shadows off) through the synchronous, asynchronous and
 * tile launch shapes.  Everything is the variant's own march -- positions, world positions, variable step, jitter, the clip box, the
 * cut-off 0.95 / 1.0, fragment modes 1-4 (which return what they return without bounds), the blend and every per-sample expression
 * in the vr_set_arithmetic mode -- except which in-box steps count:
 *   g(d) = unproject(ndcx, ndcy, d) of the ray set-up -- the function it calls for d = 0 and d = 1, with the same pixel-centre ndcx,
 *     ndcy -- mapped to texture space with the ray set-up's map (x + 0.5f, y + 0.5f, 0.5f - 2.0f * z).
 *   sigma(x) = (x.x*dir.x + x.y*dir.y) + x.z*dir.z, dir = the ray's normalised texture-space direction: separately rounded and summed
 *     left to right in both arithmetic modes (ray placement, like length3s).
 *   S_near = sigma(g(near[pixel])), S_far = sigma(g(far[pixel])), once per ray.
 *   Step k at p_k counts iff it passes IsInSampleCoords and, near bound present, sigma(p_k) >= S_near and, far bound present,
 *     sigma(p_k) < S_far.  A step that does not count is treated exactly like a step outside the clip box: not fetched, not blended,
 *     not counted; p and w still advance by their rounded additions.
 *   A NaN bound makes both comparisons false: no step of that pixel counts and the fragment is what a fully clipped ray gives.  No
 *     value of a bound is an error: near > far, infinities and negatives included.
 *   Counters as the variant's: composited = blends executed, covered as without bounds, fetched = counted samples whose corners were
 *     loaded.
 * With bounds on, every other variant, VR_OUTPUT_SURFACE, LIGHT with shadows on and the two *_batch_async entry points return
 * VR_ERR_UNSUPPORTED and enqueue nothing (a silently ignored occluder is a wrong picture).  vr_pick ignores the bounds as it ignores
 * the output setting.  Frames and counters are bit-identical across layouts, launch shapes and skipping on / off (flavours 27 / 28). */
int vr_set_ray_bounds(vr_ctx* ctx, const void* d_near, const void* d_far);

/* ---- slice views: oblique reformats and slab projections of one volume slot ------------------------------------------------
 * A plane through a volume instead of a camera's view of it (no shader of the reference; csrc/vr_slice.h): parallel sample lines
 * on a caller-defined plane in texture space, any output size, any uploaded volume slot through any TF slot.  The context's
 * uniforms, clip box, viewport, output setting, ray bounds and shadows play no part.
 *   Positions: for pixel (px, py) and each component c, b.c = (origin.c + (float)px * du.c) + (float)py * dv.c -- product and sums
 *     rounded separately in both vr_set_arithmetic modes (placement, like the ray set-up).  p_0 = b, p_{k+1} = p_k + dn (a rounded
 *     addition per component), k = 0 .. slab_steps - 1.  Step k counts iff every component of p_k is >= 0 and <= 1 (NaN fails).
 *   Sample: VR_SLICE_LINEAR -- d = BASIC's trilinear .a fetch of the slot at p_k in the arithmetic mode (texture coordinates
 *     p * N - 0.5 and the seven lerps follow the mode, clamp-to-edge texel pairs).  VR_SLICE_NEAREST -- d = .a of the voxel
 *     clamp((int)floor(p_k * N), 0, N - 1) per axis, the product rounded once (TFCalibrationApp.wgsl:172).
 *   Reduction over the n counted samples, in step order, as MIP / MINIP / AVERAGE above:
 *     VR_SLICE_MAX:     m = -inf, then if (d > m) m = d          (NaN samples are ignored)
 *     VR_SLICE_MIN:     m = +inf, then if (d < m) m = d          (NaN samples are ignored)
 *     VR_SLICE_AVERAGE: s = +0.0f, then s = s + d (f32), v = s / (float)n   (NaN propagates)
 *   Pixel: n == 0 -> (0,0,0,0).  Otherwise v goes through the TF slot with BASIC's lookup (linear, clamp-to-edge, each table at its
 *     own resolution) and the fragment is FrontToBackBlend((c.rgb, o), dst = 0) in the blend's own arithmetic:
 *     (c.r o, c.g o, c.b o, o), a -0 made +0.  VR_SLICE_RGBA32F stores that float4; VR_SLICE_BGRA8 stores the four bytes
 *     vr_present_async gives for it (one 32-bit word per pixel; the n == 0 pixel is the white background, 0xFFFFFFFF).
 *     The output is row-major, pixel (px, py) at py * width + px: width * height * 16 or * 4 bytes.
 *   Counters (vr_slice_counters): out[0] = counted samples (the sum of n), out[1] = pixels with n > 0, out[2] = samples whose
 *     voxels were loaded.
 * Kernel forms: every flavour of vr_set_kernel_flavour but 1 runs slice_kernel with exact skipping by the slot's per-brick range
 * records (MAX: brick max <= m, MIN: brick min >= m, AVERAGE: every voxel the brick can touch +-0; MAX / MIN stop loading once m
 * has reached the slot's extreme), flavour 1 the form that loads every counted sample (out[2] == out[0]).  The output, out[0] and
 * out[1] are bit-identical across the two forms and the volume layouts.  vr_last_kernel_flavour does not report slices. */
#define VR_SLICE_MAX 0
#define VR_SLICE_MIN 1
#define VR_SLICE_AVERAGE 2
#define VR_SLICE_LINEAR 0
#define VR_SLICE_NEAREST 1
#define VR_SLICE_RGBA32F 0
#define VR_SLICE_BGRA8 1
typedef struct vr_slice_desc {
    int32_t volume_slot;    /* an uploaded slot, 0 .. VR_MAX_VOLUMES-1                         */
    int32_t tf_slot;        /* a slot with both tables uploaded                                */
    uint32_t width, height; /* of the output, 1 .. 16384 each; independent of the viewport     */
    float origin[3];        /* texture-space position of pixel (0,0)'s centre at slab step 0   */
    float du[3], dv[3];     /* texture-space displacement per output pixel in x / in y         */
    float dn[3];            /* ... per slab step                                               */
    int32_t slab_steps;     /* 1 .. 65536; 1 = the thin slice                                  */
    int32_t reduce, filter, format;
} vr_slice_desc;

/* Enqueues the slice on `stream` (a hipStream_t, NULL = the ctx's own) into DEVICE memory `d_out`; nothing is synchronised.
 * VR_ERR_INVALID_ARG, before anything is enqueued: a NULL pointer, a slot out of range, a zero or oversized output, slab_steps out of
 * range, an unknown reduce / filter / format.  VR_ERR_NOT_READY: the volume slot or one of the TF slot's tables is missing.  No value
 * of origin, du, dv or dn is an error: NaN and infinities simply count nothing.
 * A slice is a launch like any other for the stream-ordered machinery: it comes after every vr_tf_upload_*_async made before it and
 * keeps the tables it read from being rewritten under it; it is one of the eight launches that may be in flight; the range records it
 * skips by are built on its stream when a volume changed since they were built (no host wait), and slices on other streams wait for
 * that build once.  It changes nothing else the caller can read: the frame of vr_download, vr_last_counters, vr_last_kernel_flavour,
 * vr_last_timing, vr_kernel_times and vr_kernel_choice stay what the render before it left -- a slice between a render and its
 * download is the normal use -- and vr_resize does not concern it.                                                          */
int vr_slice_async(vr_ctx* ctx, const vr_slice_desc* desc, void* d_out, void* stream);

/* The same into HOST memory `out_host` (width * height * 16 or * 4 bytes), on the ctx's own stream; synchronous on return. */
int vr_slice_render(vr_ctx* ctx, const vr_slice_desc* desc, void* out_host);

/* Fills *out for the axis-aligned plane `axis` (0 = x, 1 = y, 2 = z) at voxel `index` of volume slot `slot`: one output pixel per
 * voxel, pixel centres at voxel centres ((float)i + 0.5f) / (float)n.  The output's x / y run along (y, z) for axis 0, (x, z) for
 * axis 1 and (x, y) for axis 2.  A slab of `thickness` >= 1 voxels is centred on `index`: step 0 lies at voxel index - (thickness - 1) / 2
 * (integer division) and dn is one voxel, 1.0f / (float)n, along the axis; where the slab runs past a face its steps simply do not
 * count (it is not moved).  Sets volume_slot = slot, tf_slot = 0, reduce = VR_SLICE_MAX, filter = VR_SLICE_LINEAR, format =
 * VR_SLICE_RGBA32F; the caller edits them.  Pure host arithmetic; VR_ERR_INVALID_ARG for a NULL pointer, a bad slot, axis, index or
 * thickness (1 .. 65536), VR_ERR_NOT_READY for an empty slot.                                                               */
int vr_slice_orthogonal(const vr_ctx* ctx, int slot, int axis, int index, int thickness, vr_slice_desc* out);

/* Counters of the last slice launch (as described above); waits for that launch.  Zeros before the first slice. */
int vr_slice_counters(vr_ctx* ctx, uint64_t out[3]);

/* ---- histograms: how the values of a volume slot are distributed, overall and inside each contour of a mask -------------------
 * Integer counts of one channel of an uploaded slot over a voxel box, on the device (csrc/vr_hist.h; the host surface's
 * OpacityTF::ActivateHistogram / CalibrateOnMask restated for volumes that live in HBM).  Row 0 counts every voxel of the box; row
 * 1 + c the voxels of the box that lie inside contour c of the mask slot.  The uniforms, tables, viewport and vr_set_arithmetic play
 * no part.
 *   Binning of a value v: t = v * scale, one f32 multiply; i = (int32)t by the normative conversion -- truncation toward zero,
 *     saturating, NaN -> 0.  VR_HIST_CLAMP: bin = min(max(i, 0), bins - 1), and every voxel is counted.  VR_HIST_DROP: the voxel is
 *     counted iff 0 <= i < bins; otherwise it adds one to the row's `dropped`.  (static_cast<int>(a * resolution) then clamp is
 *     ActivateHistogram; static_cast<int>(a) then value < bin.size() is CalibrateOnMask.)
 *   Mask: component c of the mask voxel at the same index selects iff m.c != 0.0f -- NaN selects, -0 does not.  A voxel inside two
 *     contours is counted in both rows.
 *   Outputs: counts = uint64[VR_HIST_ROWS][bins], rows = vr_hist_row[VR_HIST_ROWS] with voxels = counted + dropped, so that for every
 *     computed row the sum of its counts + dropped == voxels.  Rows that are not requested are all zero in both; the call zeroes
 *     its own outputs on the stream.  An empty box (lo == hi on an axis) is valid and gives zeros.
 *   Counters (vr_hist_counters): out[0] = voxels of the box, out[1] = voxels whose value was loaded, out[2] = voxels accounted for
 *     from a brick range record without being loaded.
 * Kernel forms: every flavour of vr_set_kernel_flavour but 1 runs the default form -- lanes of a wavefront that hold the same
 * (row, bin) are combined before they add, and an unmasked channel-3 launch settles every 4 x 4 x 4 brick of the box whose range
 * record pins all its voxels to one bin without loading it (exact: csrc/vr_hist.h), out[1] + out[2] == out[0].  Flavour 1 runs the plain
 * form: out[1] == out[0], out[2] == 0.  With a mask the value is loaded only where a requested row needs it: out[1] < out[0] when
 * row 0 is off and voxels lie outside every requested contour.  Counts, rows and out[0] are identical across the forms and the
 * volume layouts. */
#define VR_HIST_ROWS 5          /* row 0: every voxel of the box; row 1+c: voxels whose mask component c != 0 */
#define VR_HIST_MAX_BINS 65536
#define VR_HIST_CLAMP 0
#define VR_HIST_DROP 1
typedef struct vr_hist_desc {
    int32_t  volume_slot;   /* the values: an uploaded slot                                   */
    int32_t  channel;       /* 0..3 = .r .g .b .a of its voxels                               */
    int32_t  mask_slot;     /* -1 = none; else an uploaded slot of the same nx, ny, nz        */
    uint32_t rows;          /* bit r set = compute row r; bits 1..4 need a mask_slot          */
    uint32_t bins;          /* 1 .. VR_HIST_MAX_BINS                                          */
    float    scale;
    int32_t  out_of_range;  /* VR_HIST_CLAMP / VR_HIST_DROP                                   */
    int32_t  lo[3], hi[3];  /* voxel box, half open, 0 <= lo <= hi <= n per axis; lo == hi: empty, valid */
} vr_hist_desc;
typedef struct vr_hist_row { uint64_t voxels, dropped; } vr_hist_row;   /* voxels = counted + dropped */

/* Fills *out for the whole volume of `slot`: the box (0,0,0) .. (nx,ny,nz), channel 3, no mask, rows = 1, VR_HIST_CLAMP, the given
 * bins and scale.  Pure host arithmetic; VR_ERR_INVALID_ARG for a NULL pointer, a bad slot or bin count, VR_ERR_NOT_READY for an
 * empty slot. */
int vr_hist_whole(const vr_ctx* ctx, int slot, uint32_t bins, float scale, vr_hist_desc* out);

/* Enqueues the histogram on `stream` (a hipStream_t, NULL = the ctx's own) into DEVICE memory: d_counts = uint64[VR_HIST_ROWS][bins],
 * d_rows = vr_hist_row[VR_HIST_ROWS]; nothing is synchronised on the host.
 * Checked before anything is enqueued (the outputs stay untouched).  VR_ERR_INVALID_ARG: a NULL pointer; a volume or mask slot out of
 * range; a channel outside 0 .. 3; bins outside 1 .. VR_HIST_MAX_BINS; an unknown out_of_range; a box that is not 0 <= lo <= hi <= n
 * on every axis; rows == 0, a bit of rows above bit 4, or bits 1 .. 4 without a mask_slot; a mask whose nx, ny, nz differ from the
 * value volume's.  VR_ERR_NOT_READY: the volume slot or the mask slot is empty.  No value of scale is an error.
 * A histogram is a stream-ordered launch like a slice: it is one of the eight launches that may be in flight, and the range records the
 * default form settles by are built on its stream when a volume changed since they were built (no host wait).  It changes nothing
 * else the caller can read: the frame of vr_download, vr_last_counters, vr_last_kernel_flavour, vr_last_timing, vr_kernel_times,
 * vr_kernel_choice and vr_slice_counters stay what they were. */
int vr_histogram_async(vr_ctx* ctx, const vr_hist_desc* desc, void* d_counts, void* d_rows, void* stream);

/* The same into HOST memory (counts = uint64[VR_HIST_ROWS * bins], rows = vr_hist_row[VR_HIST_ROWS]), on the ctx's own stream;
 * synchronous on return. */
int vr_histogram(vr_ctx* ctx, const vr_hist_desc* desc, uint64_t* counts, vr_hist_row* rows);

/* Counters of the last histogram launch (as described above); waits for that launch.  Zeros before the first histogram. */
int vr_hist_counters(vr_ctx* ctx, uint64_t out[3]);

/* ---- region growing: the structure under a voxel, as a contour of a mask volume ---------------------------------------------------
 * Every consumer of a mask (VOLUME_MASK, TF_CALIB, rows 1 .. 4 of vr_histogram, vr_pick's value[]) runs on the device; this call
 * produces one there too (csrc/vr_grow.h): the threshold-connected region around seed voxels -- a vr_pick_result's `voxel`, say --
 * written into one component of a mask slot.  The result is a uniquely defined set of voxels; nothing about it is approximate.
 *   Sets: Q = the voxels of the box whose value v (channel `channel` of volume_slot) qualifies: v >= lo && v <= hi in f32, so NaN never
 *     does.  Two voxels are neighbours if they differ by at most 1 on every axis and are not equal; with VR_GROW_FACES only if they
 *     differ on exactly one axis.  R = the union of the connected components of Q -- adjacency restricted to the box: a path never
 *     leaves it -- that contain at least one seed.
 *   Seeds: a seed outside the box or not in Q contributes nothing (no error); duplicates are fine.
 *   Effect on component `contour` of the mask slot's voxels: VR_GROW_REPLACE: 1.0f in R and +0.0f everywhere else, outside the box
 *     too.  VR_GROW_ADD: 1.0f in R, every other voxel keeps its bits.  The other three components keep their bits in both modes (NaN
 *     payloads and -0 included).
 *   Bounds: no value of lo / hi is an error.  lo > hi or a NaN bound gives an empty Q; -inf / +inf admit every value that is not NaN.
 *   Mask slot: an empty mask_slot is created with the value volume's nx, ny, nz and every component +0.0f; one that holds a volume of
 *     other dimensions is VR_ERR_INVALID_ARG.
 *   Result: voxels = |R|; lo / hi = the half-open bounding box of R, all zero when R is empty; rounds = the propagation rounds that had
 *     something to do (>= 1; it depends on the kernel form, nothing else does).
 *   Counters (vr_grow_counters): out[0] = voxels of the box, out[1] = voxels whose value was loaded, out[2] = voxels classified from a
 *     brick range record without a load.
 * Kernel forms: every flavour of vr_set_kernel_flavour but 1 classifies whole 4 x 4 x 4 bricks of channel 3 from their range records
 * where those decide (out[1] + out[2] == out[0]) and propagates along a frontier of bricks; flavour 1 loads every voxel of the box
 * (out[1] == out[0], out[2] == 0) and sweeps every brick in every round.  The mask, the result but `rounds` and out[0] are identical
 * across the forms and the volume layouts.  The host enqueues VR_GROW_BATCH rounds at a time and looks at the outcome in between. */
#define VR_GROW_FACES 6          /* neighbours share a face                    */
#define VR_GROW_ALL   26         /* ... a face, an edge or a corner            */
#define VR_GROW_REPLACE 0
#define VR_GROW_ADD     1
#define VR_GROW_MAX_SEEDS 64
#define VR_GROW_BATCH 8          /* propagation rounds enqueued between two looks at the outcome */
typedef struct vr_grow_desc {
    int32_t volume_slot, channel;   /* the values: an uploaded slot, 0..3 = .r .g .b .a          */
    int32_t mask_slot, contour;     /* the result: a slot != volume_slot, component 0..3          */
    float   lo, hi;                 /* a voxel qualifies iff v >= lo && v <= hi (NaN never does)  */
    int32_t connectivity, mode;
    int32_t box_lo[3], box_hi[3];   /* voxel box, half open, 0 <= lo <= hi <= n per axis          */
    uint32_t n_seeds;               /* 1 .. VR_GROW_MAX_SEEDS                                     */
    int32_t seeds[VR_GROW_MAX_SEEDS][3];   /* x, y, z; each inside the volume                     */
} vr_grow_desc;
typedef struct vr_grow_result {
    uint64_t voxels;                /* |R|                                                        */
    int32_t  lo[3], hi[3];          /* half-open bounding box of R; all zero when R is empty      */
    uint32_t rounds;                /* propagation rounds executed (form-dependent, >= 1)         */
} vr_grow_result;

/* Fills *out for the whole volume of volume_slot: channel 3, VR_GROW_FACES, VR_GROW_REPLACE, the box (0,0,0) .. (nx,ny,nz), the given
 * mask slot, contour and bounds, n_seeds = 0: the caller adds the seeds.  Pure host arithmetic; VR_ERR_INVALID_ARG for a NULL pointer,
 * a slot out of range, mask_slot == volume_slot or a contour outside 0 .. 3, VR_ERR_NOT_READY for an empty volume slot. */
int vr_grow_whole(const vr_ctx* ctx, int volume_slot, int mask_slot, int contour, float lo, float hi, vr_grow_desc* out);

/* Grows the region and writes the contour; `result` may be NULL.  A data-preparation call like vr_volume_normalize: it waits for
 * everything in flight, runs on the ctx's own stream, rebuilds what is derived from the mask slot's voxels exactly as an upload does
 * (brick records, the bricked copy, the mask's part in VOLUME_MASK's records, the distance field, range records, light volumes) and is
 * synchronous on return.  What the reporting calls say about the last march, slice or histogram stays as it was.
 * Checked before anything is enqueued or the mask slot is touched.  VR_ERR_INVALID_ARG: a NULL ctx or descriptor; a slot out of range;
 * mask_slot == volume_slot; a channel or contour outside 0 .. 3; an unknown connectivity or mode; a box that is not
 * 0 <= lo <= hi <= n on every axis; n_seeds outside 1 .. VR_GROW_MAX_SEEDS; a seed outside the volume; a mask slot of other
 * dimensions.  VR_ERR_NOT_READY: the volume slot is empty.  VR_ERR_HIP "did not converge": more than voxels-of-the-box + 1 rounds
 * (a defect, never the data: R grows in every round but the first and the last). */
int vr_segment_grow(vr_ctx* ctx, const vr_grow_desc* desc, vr_grow_result* result);

/* Counters of the last vr_segment_grow (as described above).  Zeros before the first. */
int vr_grow_counters(vr_ctx* ctx, uint64_t out[3]);

/* Device time of the last vr_segment_grow in milliseconds, from events on the ctx's stream: ms[0] classify and seed, ms[1] the
 * propagation rounds (the host's looks in between included), ms[2] the write and the result, ms[3] the rebuild of what is derived
 * from the mask slot.  Zeros before the first and after one that failed. */
int vr_grow_timing(vr_ctx* ctx, float ms[4]);

/* ---- mask morphology and contour algebra: margins, shells, unions and closings of contours ---------------------------------------
 * A contour of a mask slot, restricted to a box, is dilated, eroded, closed or opened by a structuring element, or taken as it is, and
 * the result is combined into a contour of a mask slot -- on the device (csrc/vr_morph.h), so that a grown region can be smoothed and
 * a structure given a margin in millimetres without a download.  The result is exact set arithmetic on voxels.
 *   Membership: voxel p of a slot is IN contour k iff component k of its vec4 is != 0.0f (the rule of vr_histogram's rows 1 .. 4): NaN is
 *     in, -0.0f is out.
 *   Element E: a set of integer offsets, symmetric under reflection of each axis, given by its radii (rx, ry, rz) and a table of
 *     half-chords along x: half[dz + rz][dy + ry] = h >= 0 says that the offsets (-h .. h, dy, dz) belong to E, -1 that none with this
 *     (dy, dz) does.  Valid: every radius in 0 .. VR_MORPH_MAX_RADIUS; every entry of the (2 rz + 1) x (2 ry + 1) window in -1 .. rx;
 *     half[rz][ry] >= 0 (the origin is in E); half[rz + dz][ry + dy] == half[rz - dz][ry + dy] == half[rz + dz][ry - dy].  Entries outside
 *     the window are ignored.  Convexity is not required.
 *   Operand: A' = the voxels of the box that are in contour src_contour of src_slot.  Nothing outside the box is read as set or written.
 *   Operators (op), with E ignored by the first:
 *     VR_MORPH_NONE    R = A' (the pure contour algebra)
 *     VR_MORPH_DILATE  R = { p in the box : p - e in A' for some e in E }
 *     VR_MORPH_ERODE   R = box \ dilate(box \ A'): p survives iff every p + e THAT LIES IN THE BOX is in A' (the outside does not erode)
 *     VR_MORPH_CLOSE   R = erode(dilate(A'))
 *     VR_MORPH_OPEN    R = dilate(erode(A'))
 *     With these border rules closing is extensive, opening anti-extensive, and both are idempotent.
 *   Writing (combine), into component dst_contour of dst_slot, voxels of the box only:
 *     VR_MORPH_REPLACE  1.0f in R, +0.0f elsewhere          VR_MORPH_OR      1.0f in R, the rest keep their bits
 *     VR_MORPH_AND      +0.0f outside R, the rest keep theirs  VR_MORPH_ANDNOT  +0.0f in R, the rest keep their bits
 *     The other three components keep their bits (NaN payloads and -0 included), and so does every voxel outside the box.  A' is packed
 *     before anything is written: src == dst, in slot and in contour, is legal and means "in place".
 *   Destination: an empty dst_slot is created with the source's nx, ny, nz and every component +0.0f; one that holds a volume of other
 *     dimensions is VR_ERR_INVALID_ARG.  dst_slot == src_slot is allowed.
 *   Result: voxels = |R|, src_voxels = |A'|, lo / hi = the half-open bounding box of R, all zero when R is empty.
 *   Counters (vr_morph_counters), out[1] + out[2] == out[0] always: out[0] = voxels of the box; out[1] = voxels of the box in the words
 *     the last dilation launch of the call computed; out[2] = voxels of the box that were settled without computing them.  VR_MORPH_NONE
 *     launches no dilation: out[1] = 0 in both kernel forms.
 * Kernel forms: every flavour of vr_set_kernel_flavour but 1 computes only where the result can be set -- for a dilation the bounding box
 * of its source bits grown by the radii, for an erosion that bounding box itself, both within the box -- and zero-fills the rest; flavour
 * 1 computes every word of the box (out[1] == out[0] for the four operators with an element).  The mask and the result are identical
 * across the forms and the volume layouts. */
#define VR_MORPH_MAX_RADIUS 31
#define VR_MORPH_NONE   0
#define VR_MORPH_DILATE 1
#define VR_MORPH_ERODE  2
#define VR_MORPH_CLOSE  3
#define VR_MORPH_OPEN   4
#define VR_MORPH_REPLACE 0
#define VR_MORPH_OR      1
#define VR_MORPH_AND     2
#define VR_MORPH_ANDNOT  3
typedef struct vr_morph_element {
    int32_t radius[3];                /* rx, ry, rz: 0 .. VR_MORPH_MAX_RADIUS                                  */
    int8_t  half[2 * VR_MORPH_MAX_RADIUS + 1][2 * VR_MORPH_MAX_RADIUS + 1];
                                      /* half[dz + rz][dy + ry] = h >= 0: offsets (-h .. h, dy, dz) are in E; -1: none is */
} vr_morph_element;
typedef struct vr_morph_desc {
    int32_t src_slot, src_contour;    /* operand A: an uploaded slot, component 0 .. 3                         */
    int32_t dst_slot, dst_contour;    /* where the result goes; may equal the source (in place)                */
    int32_t op, combine;
    int32_t box_lo[3], box_hi[3];     /* voxel box, half open, 0 <= lo <= hi <= n per axis                     */
    vr_morph_element element;         /* checked and used only when op != VR_MORPH_NONE                        */
} vr_morph_desc;
typedef struct vr_morph_result {
    uint64_t voxels, src_voxels;      /* |R|, |A'|                                                             */
    int32_t  lo[3], hi[3];            /* half-open bounding box of R; all zero when R is empty                 */
} vr_morph_result;

/* The ball of `radius` on a grid of the given voxel spacing, both in one unit of the caller's choice (micrometres, say):
 * (dx, dy, dz) is in E iff (dx sx)^2 + (dy sy)^2 + (dz sz)^2 <= radius^2, evaluated in uint64_t; the radii are radius / spacing by
 * integer division; entries outside the window are -1.  Pure host integer arithmetic, no context and no device.  VR_ERR_INVALID_ARG for a
 * NULL pointer, a spacing of zero or above 2^20, or a radius above VR_MORPH_MAX_RADIUS voxels on some axis. */
int vr_morph_ball(const uint32_t spacing[3], uint32_t radius, vr_morph_element* out);

/* The full box of radii rx, ry, rz (each 0 .. VR_MORPH_MAX_RADIUS, else VR_ERR_INVALID_ARG): every half-chord of the window is rx.
 * (1, 1, 0) is a per-slice 3 x 3 element. */
int vr_morph_box(int rx, int ry, int rz, vr_morph_element* out);

/* Fills *out for the whole volume of src_slot: the given slots, contours and operator, VR_MORPH_REPLACE, the box (0,0,0) .. (nx,ny,nz)
 * and the radius-1 ball of unit spacing (the 6-neighbour cross).  Pure host arithmetic; VR_ERR_INVALID_ARG for a NULL pointer, a slot
 * or contour out of range or an unknown operator, VR_ERR_NOT_READY for an empty source slot. */
int vr_morph_whole(const vr_ctx* ctx, int src_slot, int src_contour, int dst_slot, int dst_contour, int op, vr_morph_desc* out);

/* Does the work; `result` may be NULL.  A data-preparation call exactly like vr_segment_grow: it waits for everything in flight, runs
 * on the ctx's own stream, rebuilds what is derived from the destination slot's voxels as an upload does and is synchronous on return.
 * What the reporting calls say about the last march, slice, histogram or grow stays as it was.
 * Checked before anything is enqueued or a slot is touched.  VR_ERR_INVALID_ARG: a NULL ctx or descriptor; a slot out of range; a
 * contour outside 0 .. 3; an unknown op or combine; a box that is not 0 <= lo <= hi <= n on every axis; an invalid element when
 * op != VR_MORPH_NONE; a destination slot of other dimensions.  VR_ERR_NOT_READY: the source slot is empty. */
int vr_mask_morph(vr_ctx* ctx, const vr_morph_desc* desc, vr_morph_result* result);

/* Counters of the last vr_mask_morph (as described above).  Zeros before the first. */
int vr_morph_counters(vr_ctx* ctx, uint64_t out[3]);

/* Device time of the last vr_mask_morph in milliseconds, from events on the ctx's stream: ms[0] the pack of the operand (the host's
 * look at its bounding box included), ms[1] the dilation launches, ms[2] the write and the result, ms[3] the rebuild of what is derived
 * from the destination slot.  Zeros before the first and after one that failed. */
int vr_morph_timing(vr_ctx* ctx, float ms[4]);

/* ---- signed distance maps of a mask contour: how far every voxel is from a structure ------------------------------------------------
 * The exact Euclidean distance transform of a contour of a mask slot, restricted to a box, on an anisotropic grid, written as f32 into
 * one component of a volume slot -- on the device (csrc/vr_dist.h).  A distance channel composes with everything downstream: slices,
 * histograms (dose against distance), VR_VARIANT_ISO (the smooth surface of a structure, or of the structure plus 7 mm).
 *   Membership, operand, box: exactly those of the morphology above.  A' = the voxels of the half-open box that are in contour src_contour
 *     of src_slot (!= 0.0f: NaN is in, -0.0f is out); B' = box \ A'.  Nothing outside the box is read as set or written: the outside of
 *     the box is neither foreground nor background (the border rule of VR_MORPH_ERODE).
 *   Spacing: spacing[3] (x, y, z) in an integer unit of the caller's choice (micrometres, say), each 1 .. 2^20, and on every axis
 *     (uint64_t)(box_hi[a] - box_lo[a]) * spacing[a] <= 1 << 30, else VR_ERR_INVALID_ARG: every squared distance stays below 2^62 and
 *     the differences an exact lower-envelope computation forms fit int64_t.
 *   Fields: for a voxel p of the box D2out(p) = min over q in A' of sum_a ((p_a - q_a) * spacing[a])^2, and D2in(p) the same over B',
 *     both exact in uint64_t.  An empty set gives BEYOND.
 *   Limit: limit (same unit), at most 2^31; 0 = none.  With a limit L a value greater than L^2 becomes BEYOND.
 *   Stored value: the magnitude of a finite D2 is m = sqrt_rn((float)D2) * scale -- the uint64_t -> f32 conversion rounded to nearest,
 *     the correctly rounded f32 square root, one f32 multiply; BEYOND gives (float)L * scale with a limit and +inf without one.  scale
 *     must be finite and > 0, else VR_ERR_INVALID_ARG (0.001f turns micrometres into millimetres).  mode:
 *       VR_DIST_OUTSIDE  +m(D2out): +0 inside A'
 *       VR_DIST_INSIDE   +m(D2in): +0 outside A'
 *       VR_DIST_SIGNED   +m(D2out) for p not in A', -m(D2in) for p in A': no voxel is 0, the zero level lies between voxel centres
 *     into component dst_channel of dst_slot, voxels of the box only.  The other three components keep their bits, and so does every
 *     voxel outside the box.  A' (and the probe) are packed before anything is written: source and destination may coincide in slot and
 *     component.  An empty dst_slot is created with the source's nx, ny, nz and every component +0.0f; one of other dimensions is
 *     VR_ERR_INVALID_ARG.
 *   Probe (optional): probe_slot / probe_contour name a second contour of the same dimensions, probe_slot = -1 none; it may be the
 *     destination.  Over the probe's voxels in the box the result holds probe_voxels and probe_min_sq / probe_max_sq of D2out (the limit
 *     applied; BEYOND is UINT64_MAX), both 0 when probe_voxels == 0: the minimum distance between two structures and the directed
 *     Hausdorff distance as exact integers.  A probe with VR_DIST_INSIDE is VR_ERR_INVALID_ARG.
 *   Result: src_voxels = |A'|, lo / hi = its half-open bounding box (all zero when it is empty), beyond = the voxels of the box whose
 *     stored value is BEYOND's, then the three probe fields.
 *   Counters (vr_dist_counters), out[1] + out[2] == out[0] always: out[0] = voxels of the box; out[1] = voxels of the box inside the region
 *     for which the envelope passes computed the call's field (the OUTSIDE field; the INSIDE field in VR_DIST_INSIDE); out[2] = the rest.
 * Kernel forms: flavour 1 of vr_set_kernel_flavour computes every voxel of the box (out[1] == out[0]).  Every other flavour computes a
 * field only inside a region outside of which it is known, and fills the rest: with a limit the OUTSIDE field is BEYOND outside the
 * bounding box of A' grown by limit / spacing[a] voxels per axis (without one the region is the box, and empty for an empty A'); the INSIDE
 * field is 0 outside A' and exact when computed on the bounding box of A' grown by one voxel, within the box.  The slot, the result and
 * out[0] are identical across the forms and the volume layouts.
 * Two laws tie this to the morphology: with E = the ball of vr_morph_ball for (spacing, r), { p : D2out(p) <= r^2 } is VR_MORPH_DILATE by E
 * and { p in the box : D2in(p) > r^2 } is VR_MORPH_ERODE by E. */
#define VR_DIST_OUTSIDE 0
#define VR_DIST_INSIDE  1
#define VR_DIST_SIGNED  2
typedef struct vr_dist_desc {
    int32_t  src_slot, src_contour;     /* the contour: an uploaded slot, component 0 .. 3                       */
    int32_t  dst_slot, dst_channel;     /* where the distances go; may equal the source (in place)               */
    int32_t  mode;                      /* VR_DIST_OUTSIDE / VR_DIST_INSIDE / VR_DIST_SIGNED                     */
    int32_t  probe_slot, probe_contour; /* a second contour whose D2out range is reported; probe_slot = -1: none */
    uint32_t limit;                     /* 0 = none; at most 2^31                                                */
    uint32_t spacing[3];                /* x, y, z: 1 .. 2^20 each                                               */
    float    scale;                     /* stored value = distance * scale                                       */
    int32_t  box_lo[3], box_hi[3];      /* voxel box, half open, 0 <= lo <= hi <= n per axis                     */
} vr_dist_desc;
typedef struct vr_dist_result {
    uint64_t src_voxels;                /* |A'|                                                                  */
    int32_t  lo[3], hi[3];              /* half-open bounding box of A'; all zero when it is empty               */
    uint64_t beyond;                    /* voxels of the box that store BEYOND's value                           */
    uint64_t probe_voxels, probe_min_sq, probe_max_sq;
} vr_dist_result;

/* Fills *out for the whole volume of src_slot: the given slots, components and mode, unit spacing, no limit, scale 1.0f, no probe, the
 * box (0,0,0) .. (nx,ny,nz).  Pure host arithmetic; VR_ERR_INVALID_ARG for a NULL pointer, a slot or component out of range or an
 * unknown mode, VR_ERR_NOT_READY for an empty source slot. */
int vr_dist_whole(const vr_ctx* ctx, int src_slot, int src_contour, int dst_slot, int dst_channel, int mode, vr_dist_desc* out);

/* Does the work; `result` may be NULL.  A data-preparation call exactly like vr_mask_morph: it waits for everything in flight, runs on
 * the ctx's own stream, rebuilds what is derived from the destination slot's voxels as an upload does and is synchronous on return.
 * What the reporting calls say about the last march, slice, histogram, grow or morph stays as it was.
 * Checked before anything is enqueued or a slot is touched.  VR_ERR_INVALID_ARG: a NULL ctx or descriptor; a slot out of range (the
 * probe's: other than -1); a contour or channel outside 0 .. 3; an unknown mode; a probe with VR_DIST_INSIDE; a spacing of 0 or above
 * 2^20; a limit above 2^31; a scale that is not finite or not > 0; a box that is not 0 <= lo <= hi <= n on every axis or whose extent
 * times the spacing exceeds 2^30 on some axis; a destination or probe slot of other dimensions.  VR_ERR_NOT_READY: the source slot, or
 * the probe slot, is empty.  VR_ERR_OOM: the working buffers could not be allocated; nothing has been written. */
int vr_mask_distance(vr_ctx* ctx, const vr_dist_desc* desc, vr_dist_result* result);

/* Counters of the last vr_mask_distance (as described above).  Zeros before the first. */
int vr_dist_counters(vr_ctx* ctx, uint64_t out[3]);

/* Device time of the last vr_mask_distance in milliseconds, from events on the ctx's stream: ms[0] the pack of the contour and the probe
 * (the host's look at the bounding box included), ms[1] the distance passes, ms[2] the write and the result, ms[3] the rebuild of what
 * is derived from the destination slot.  Zeros before the first and after one that failed. */
int vr_dist_timing(vr_ctx* ctx, float ms[4]);

/* ---- polygon rasterisation: closed planar outlines scan-converted into contours of a mask slot ------------------------------------
 * The closed polygons of a structure set, or what a user draws on a slice view, become contours of a mask slot -- on the device
 * (csrc/vr_raster.h), so that an outline can be added to a contour, cut out of it or replace it without a volume passing through the
 * host.  Everything is integer arithmetic; the result is exact and does not depend on scheduling.
 *   Grid: the voxels of grid_slot (nx, ny, nz).  The centre of voxel (i, j) of a slice is (xc, yc) = (origin[0] + i * spacing[0],
 *     origin[1] + j * spacing[1]) in an integer unit of the caller's choice (micrometres, say).  spacing: 1 .. 2^20 each.
 *   Polygons: polygon p is the points[first .. first + count) (pairs x, y in the same unit) on slice `slice`, for contour `contour`.  Its
 *     edges join consecutive points, and the last point joins the first.  Each edge is oriented from a to b so that by > ay; horizontal
 *     edges never count.
 *   Coverage: an edge COUNTS for voxel (i, j) iff ay <= yc < by and (xc - ax) * (by - ay) < (yc - ay) * (bx - ax): the row is half open
 *     and the centre lies strictly left of the crossing.  A polygon COVERS the voxel iff an odd number of its edges count.  Hence
 *       - a centre on a left or lower boundary is in, one on a right or upper boundary is out;
 *       - two polygons that share an edge partition the voxels between them: none is covered twice, none is left out;
 *       - a polygon of 1 or 2 points, or of zero area, covers nothing;
 *       - a self-intersecting polygon follows the even-odd rule.
 *   Range: every point coordinate and both origin values lie within -2^29 .. 2^29, else VR_ERR_INVALID_ARG.  Then on the rows where an
 *     edge can count yc - ay < by - ay <= 2^30, each product is below 2^60, N = (yc - ay) * (bx - ax) + (ax - origin[0]) * (by - ay) is
 *     below 2^61 in magnitude and D = spacing[0] * (by - ay) is at most 2^50: an edge on row j toggles exactly the voxels [0, k) of the
 *     row, k = clamp(ceil(N / D), 0, nx), in int64_t.
 *   Sets: for each contour k, R_k is a part of the box, built from the polygons of the call with contour == k and box_lo[2] <= slice <
 *     box_hi[2], each on its own slice, rows and columns cut to the box.  rule:
 *       VR_POLY_EVEN_ODD  a voxel is in R_k iff an odd number of those polygons cover it (a polygon inside another one is a hole)
 *       VR_POLY_UNION     ... iff at least one of them, taken even-odd on its own, covers it
 *     A polygon whose slice lies outside the box covers nothing.  A polygon whose contour is not in `contours` is VR_ERR_INVALID_ARG.
 *   Writing: for each k in `contours` (bit k set), component k of the voxels of the box is written by `combine`, with R_k for R, exactly
 *     as the morphology above writes: VR_MORPH_REPLACE 1.0f in R and +0.0f elsewhere, VR_MORPH_OR 1.0f in R, VR_MORPH_AND +0.0f
 *     outside R, VR_MORPH_ANDNOT +0.0f in R; the rest of the box, the components not in `contours` and every voxel outside the box keep
 *     their bits (NaN payloads and -0 included).  A contour in `contours` without polygons has an empty R_k: REPLACE clears the box.
 *   Destination: an empty dst_slot is created with the grid's nx, ny, nz and every component +0.0f; one that holds a volume of other
 *     dimensions is VR_ERR_INVALID_ARG.  dst_slot == grid_slot is allowed.
 *   Result: per contour k in `contours`, voxels[k] = |R_k| and lo[k] / hi[k] = its half-open bounding box; zeros for an empty set and
 *     for a contour that is not in `contours`.
 *   Counters (vr_polygons_counters), out[1] + out[2] == out[0] always: out[0] = polygons given; out[1] = polygons rasterised; out[2] =
 *     polygons skipped: those whose slice is outside the box and, in the default kernel form, those whose bounding rows or columns miss
 *     the box.
 * Kernel forms: every flavour of vr_set_kernel_flavour but 1 visits, for each polygon, only the rows of the box that its y span reaches
 * and skips a polygon that misses the box; flavour 1 visits every row of the box for every polygon of a slice inside the box.  The
 * slot, the result and out[0] are identical across the forms and the volume layouts. */
#define VR_POLY_EVEN_ODD 0
#define VR_POLY_UNION    1
typedef struct vr_polygon {
    uint32_t first, count;             /* points[first .. first + count)                                         */
    int32_t  slice;                    /* z of the slice the polygon lies on                                     */
    int32_t  contour;                  /* 0 .. 3, and in the descriptor's `contours`                             */
} vr_polygon;
typedef struct vr_polygons_desc {
    int32_t  grid_slot;                /* an uploaded slot: its nx, ny, nz are the grid (and a fresh destination's dimensions) */
    int32_t  dst_slot;                 /* may equal grid_slot                                                    */
    int32_t  contours;                 /* bit k set: contour k of dst_slot is written by this call (1 .. 15)     */
    int32_t  rule, combine;            /* VR_POLY_EVEN_ODD / VR_POLY_UNION; VR_MORPH_REPLACE / OR / AND / ANDNOT */
    int32_t  box_lo[3], box_hi[3];     /* voxel box, half open; nothing outside it is written                    */
    int32_t  origin[2];                /* x, y of the CENTRE of voxel (0, 0), in the caller's unit               */
    uint32_t spacing[2];               /* voxel pitch along x, y in the same unit: 1 .. 2^20                     */
    uint32_t n_points, n_polygons;
    const int32_t*    points;          /* n_points pairs (x, y) in that unit, host memory                        */
    const vr_polygon* polygons;        /* host memory                                                            */
} vr_polygons_desc;
typedef struct vr_polygons_result {
    uint64_t voxels[4];                /* |R_k|                                                                  */
    int32_t  lo[4][3], hi[4][3];       /* half-open bounding box of R_k; all zero when it is empty               */
} vr_polygons_result;

/* Fills *out for the whole grid of grid_slot: the given slots, contour 0 alone (contours = 1), VR_POLY_EVEN_ODD, VR_MORPH_REPLACE, the box
 * (0,0,0) .. (nx,ny,nz), origin (0, 0), unit spacing and no polygons.  Pure host arithmetic; VR_ERR_INVALID_ARG for a NULL pointer or a
 * slot out of range, VR_ERR_NOT_READY for an empty grid slot. */
int vr_polygons_whole(const vr_ctx* ctx, int grid_slot, int dst_slot, vr_polygons_desc* out);

/* Does the work; `result` may be NULL.  A data-preparation call exactly like vr_mask_morph: it waits for everything in flight, runs on
 * the ctx's own stream, rebuilds what is derived from the destination slot's voxels as an upload does and is synchronous on return: the
 * points and polygons may be freed then.  What the reporting calls say about earlier launches and tools stays as it was.
 * Checked before anything is enqueued or a slot is touched.  VR_ERR_INVALID_ARG: a NULL ctx or descriptor; a slot out of range; a NULL
 * points or polygons pointer with a non-zero count; a polygon with first + count > n_points, a contour outside 0 .. 3 or one that is
 * not in `contours`; `contours` outside 1 .. 15; an unknown rule or combine; a box that is not 0 <= lo <= hi <= n on every axis; a
 * spacing of 0 or above 2^20; a coordinate or origin value outside the range; a destination slot of other dimensions.
 * VR_ERR_NOT_READY: the grid slot is empty.  n_polygons == 0 is legal. */
int vr_mask_polygons(vr_ctx* ctx, const vr_polygons_desc* desc, vr_polygons_result* result);

/* Counters of the last vr_mask_polygons (as described above).  Zeros before the first. */
int vr_polygons_counters(vr_ctx* ctx, uint64_t out[3]);

/* Device time of the last vr_mask_polygons in milliseconds, from events on the ctx's stream: ms[0] the upload of the points and the
 * work list, ms[1] the raster, ms[2] the write and the result, ms[3] the rebuild of what is derived from the destination slot.  Zeros
 * before the first and after one that failed. */
int vr_polygons_timing(vr_ctx* ctx, float ms[4]);

/* ---- contour tracing: the contours of a mask slot as closed planar polygons --------------------------------------------------------
 * The inverse of vr_mask_polygons: the contours of a mask slot, slice by slice, become closed rectilinear polygons in the points /
 * vr_polygon layout that vr_mask_polygons reads -- on the device (csrc/vr_outline.h), so that a structure that was grown, given a margin
 * or cut can be stored as outlines, or drawn over a slice view, without its volume passing through the host.  Everything is integer
 * arithmetic; the output is exact and does not depend on scheduling.  The call reads slots and writes none.
 *   Set: for contour k and slice z of the box, S holds the voxels (i, j) of the box whose component k is != 0.0f (the membership rule of
 *     the other mask tools: NaN is in, -0 is out).  Everything outside the box is out.
 *   Cracks: lattice vertex (i, j), 0 <= i <= nx, 0 <= j <= ny, is the lower-left corner of voxel (i, j).  For every voxel of S and each
 *     of its four sides whose neighbour is not in S there is one directed unit edge with the voxel on its LEFT: with x to the right and
 *     y up, outer boundaries run counter-clockwise and holes clockwise.  Directions: 0 = +x, 1 = +y, 2 = -x, 3 = -y.  An edge's key is
 *     (j * (nx + 1) + i) * 4 + direction, of its tail vertex (i, j).
 *   Successor: an edge's successor is an edge that leaves its head vertex.  At a vertex where two edges leave (two diagonal voxels in,
 *     the other two out) VR_OUTLINE_SPLIT takes the left turn, which separates the two voxels, and VR_OUTLINE_JOIN the right turn, which
 *     connects them.  Every edge has exactly one successor and one predecessor: the edges fall into disjoint loops.
 *   Polygons: one per loop.  Its points are the tails of the loop's edges whose predecessor has another direction (the corners), in
 *     loop order, the first point the tail of the loop's edge with the smallest key: always a corner, and the lowest-then-leftmost
 *     vertex of the loop.  A polygon has an even number of points, at least 4, and no three consecutive collinear ones.
 *   Order: polygons are sorted by contour, then slice, then the key of their first edge; their points follow in the same order, `first`
 *     running.  vr_polygon.slice = z, .contour = k.
 *   Coordinates: vertex (i, j) is written as (origin[0] + i * spacing[0] - offset[0], origin[1] + j * spacing[1] - offset[1]), with
 *     0 <= offset[a] < spacing[a]; origin is the CENTRE of voxel (0, 0) as in vr_polygons_desc.  With offset = spacing / 2 (an even
 *     spacing) the points lie on the geometric voxel faces.  For ANY offset in that range and either connect rule, vr_mask_polygons of
 *     the output with the same origin and spacing, VR_POLY_EVEN_ODD and VR_MORPH_REPLACE over the same box reproduces S exactly: a
 *     face at centre - d, 0 <= d < spacing, cuts between the same two centres under the raster's half-open tie rule.  The origin lies
 *     within +-2^29 and so does every vertex of the box (0 <= lo <= i <= hi), else VR_ERR_INVALID_ARG.
 *   Capacity: max_points == max_polygons == 0 is the counting call: VR_OK, the result filled.  If either buffer is too small both
 *     arrays are left untouched, the result is filled all the same, the call returns VR_ERR_INVALID_ARG and vr_last_error names both
 *     needed counts.  More than 2^31 - 1 corners in one call: VR_ERR_UNSUPPORTED.
 *   Result: n_points, n_polygons = what the mask needs; per contour k its polygons, its points and area2[k] = twice the signed area of
 *     its polygons in lattice units = 2 * the voxels of the contour in the box.  Zeros for a contour that is not traced.
 *   Counters (vr_outlines_counters): out[0] = corner nodes (= n_points), out[1] = polygons, out[2] = doubling rounds launched.
 * Kernel forms: every flavour of vr_set_kernel_flavour but 1 stops the rounds that rank the corners along their loops after the first
 * round that changes nothing; flavour 1 runs ceil(log2(corners)) rounds.  Everything but out[2] is identical across the forms and the
 * volume layouts. */
#define VR_OUTLINE_SPLIT 0   /* voxels that touch only at a corner are separated */
#define VR_OUTLINE_JOIN  1   /* ... are connected                                 */
typedef struct vr_outlines_desc {
    int32_t  src_slot;                 /* an uploaded slot                                                       */
    int32_t  contours;                 /* bit k set: contour k is traced (1 .. 15)                               */
    int32_t  connect;                  /* VR_OUTLINE_SPLIT / VR_OUTLINE_JOIN                                     */
    int32_t  box_lo[3], box_hi[3];     /* voxel box, half open; voxels outside it count as not in                */
    int32_t  origin[2];                /* x, y of the CENTRE of voxel (0, 0), as in vr_polygons_desc             */
    uint32_t spacing[2];               /* voxel pitch along x, y in the same unit: 1 .. 2^20                     */
    uint32_t offset[2];                /* 0 <= offset[a] < spacing[a]: see Coordinates                           */
    uint32_t max_points, max_polygons; /* what the two arrays hold                                               */
    int32_t*    points;                /* host memory, max_points pairs (x, y); NULL iff max_points == 0         */
    vr_polygon* polygons;              /* host memory; NULL iff max_polygons == 0                                */
} vr_outlines_desc;
typedef struct vr_outlines_result {
    uint32_t n_points, n_polygons;     /* what the mask needs, whether or not it was stored                      */
    uint32_t polygons_of[4], points_of[4];
    int64_t  area2[4];                 /* twice the signed area in lattice units: 2 * voxels of the contour in the box */
} vr_outlines_result;

/* Fills *out for the whole volume of src_slot: contour 0 alone (contours = 1), VR_OUTLINE_SPLIT, the box (0,0,0) .. (nx,ny,nz), origin
 * (0, 0), unit spacing, offset 0 and no buffers.  Pure host arithmetic; VR_ERR_INVALID_ARG for a NULL pointer or a slot out of range,
 * VR_ERR_NOT_READY for an empty slot. */
int vr_outlines_whole(const vr_ctx* ctx, int src_slot, vr_outlines_desc* out);

/* Does the work; `result` may be NULL.  A synchronous data call on the ctx's own stream: it waits for everything in flight, writes no
 * slot, rebuilds nothing that is derived from one, and leaves what the reporting calls say about earlier launches and tools as it was.
 * An empty box or an empty contour gives zero polygons and VR_OK.
 * Checked before anything is enqueued.  VR_ERR_INVALID_ARG: a NULL ctx or descriptor; a slot out of range; `contours` outside 1 .. 15;
 * an unknown connect; a box that is not 0 <= lo <= hi <= n on every axis; a spacing of 0 or above 2^20; an offset that is not below its
 * spacing; an origin value or a vertex of the box outside +-2^29; points or polygons NULL with a capacity, or given with none.
 * VR_ERR_NOT_READY: the slot is empty.  VR_ERR_OOM: the working buffers could not be allocated. */
int vr_mask_outlines(vr_ctx* ctx, const vr_outlines_desc* desc, vr_outlines_result* result);

/* Counters of the last vr_mask_outlines that got as far as counting (as described above).  Zeros before the first. */
int vr_outlines_counters(vr_ctx* ctx, uint64_t out[3]);

/* Device time of the last vr_mask_outlines in milliseconds, from events on the ctx's stream: ms[0] the pack of the contours, ms[1] the
 * corners, their scan and the links, ms[2] the doubling rounds (the host's looks at their outcome included), ms[3] the polygons' scans,
 * the emit and the copy back.  A phase the call did not begin is 0: all four for an empty box, ms[2] and ms[3] when no contour has a
 * corner.  A call that fails only because points or polygons is too small has done the counting call's work and reports its phases
 * like one.  Zeros before the first call and after one that failed otherwise; a call refused for its arguments changes nothing. */
int vr_outlines_timing(vr_ctx* ctx, float ms[4]);

/* ---- connected components: the pieces a contour of a mask slot consists of ----------------------------------------------------------
 * Labels the connected components of a contour -- or of its complement in a box -- on the device (csrc/vr_comp.h), so that specks can be
 * removed, the largest piece kept, holes filled, lesions enumerated and islands coloured without the volume passing through the host.
 * Everything is integer arithmetic; nothing is approximate, and every output is a function of the inputs alone, never of scheduling.
 *   Set: with background = 0, S holds the voxels of the box whose component src_contour is != 0.0f (the membership rule of the other
 *     mask tools: NaN is in, -0.0f is out); with background = 1, the voxels of the box for which that is NOT so.  Everything outside the
 *     box is outside S in both modes and is never a neighbour: a path never leaves the box.
 *   Components: the classes of S under the connectivity.  Two voxels are neighbours as in vr_segment_grow: VR_COMP_FACES if they share a
 *     face, VR_COMP_ALL a face, an edge or a corner; VR_COMP_PLANE_FACES and VR_COMP_PLANE_ALL are the same within a slice: they also
 *     require equal z.
 *   Numbering: a voxel's index is z * ny * nx + y * nx + x; a component's `first` is its voxel with the smallest index.  Component c
 *     (0-based in the table, label c + 1) is the one with the c-th smallest `first`: labels rise in raster order of the components'
 *     first voxels.
 *   Table: per component its voxels, the half-open bounding box, `first`, and `faces`: bit 0 .. 5 set if it has a voxel with
 *     x == box_lo[0], x == box_hi[0] - 1, y == box_lo[1], y == box_hi[1] - 1, z == box_lo[2], z == box_hi[2] - 1.
 *   Selection: a component PASSES if min_voxels <= voxels <= max_voxels and (faces & reject_faces) == 0.  With keep_largest = K != 0
 *     only the K passing components with the most voxels are selected, ties going to the smaller label; with K = 0 every passing one.
 *     min_voxels > max_voxels selects nothing and is not an error.  R is the union of the selected components.
 *   Contour write (dst_slot >= 0): R is combined into component dst_contour of dst_slot over the voxels of the box by the rule of
 *     vr_mask_morph (`combine`, VR_MORPH_REPLACE .. VR_MORPH_ANDNOT).  The other three components keep their bits, and so does every
 *     voxel outside the box.  dst == src (slot and contour) is legal: S is packed before anything is written.
 *   Label map (label_slot >= 0): for every voxel of the box, component label_channel of label_slot becomes (float)label inside S and
 *     +0.0f outside S -- the labels of ALL components, not only the selected ones.  Everything else keeps its bits.  If a label map is
 *     asked for and n_components > VR_COMP_MAX_LABEL (labels are stored as f32: exact up to there) the call returns VR_ERR_UNSUPPORTED
 *     and nothing is written: neither the label map nor the contour nor the table, and an empty destination slot stays empty.  The
 *     result is filled all the same, as for a table that is too small, and vr_last_error names n_components.
 *   One slot per call: if both a contour and a label map are asked for they must lie in the same slot and in different components,
 *     else VR_ERR_INVALID_ARG.  An empty destination slot is created zeroed with the source's dimensions; a slot of other dimensions is
 *     VR_ERR_INVALID_ARG.  With neither, the call writes no slot and rebuilds nothing, like vr_mask_outlines.
 *   Capacity: max_components == 0 with components == NULL: no table is wanted (with both destinations -1 as well: the counting call).
 *     If 0 < max_components < n_components the table and every slot stay untouched, the result is filled all the same, the call returns
 *     VR_ERR_INVALID_ARG and vr_last_error names the needed count.  A pointer without a capacity or a capacity without a pointer:
 *     VR_ERR_INVALID_ARG.
 *   Result: n_components, n_selected; voxels = |S|, selected_voxels = |R|; largest = the voxels of the biggest component (0 if none);
 *     lo, hi = the half-open bounding box of R, zeros when R is empty.
 *   Nodes: the work is done on maximal runs of set bits along x within one row of the box (csrc/vr_comp.h); more than 2^32 - 1 of them
 *     in one call: VR_ERR_UNSUPPORTED.
 *   Counters (vr_components_counters): out[0] = voxels of the box, out[1] = run nodes, out[2] = pairs (node, run that touches it in an
 *     earlier row its connectivity names) examined.  All three are functions of the inputs.
 * vr_set_kernel_flavour, vr_set_arithmetic and the volume layout play no part in the result: there is one kernel form. */
#define VR_COMP_FACES        6    /* neighbours share a face                                     */
#define VR_COMP_ALL         26    /* ... a face, an edge or a corner                             */
#define VR_COMP_PLANE_FACES  4    /* as 6, within a slice only (dz == 0)                         */
#define VR_COMP_PLANE_ALL    8    /* as 26, within a slice only                                  */
#define VR_COMP_MAX_KEEP    64
#define VR_COMP_MAX_LABEL   (1u << 24)   /* labels are stored as f32: exact up to here           */
typedef struct vr_component {
    uint64_t voxels;
    int32_t  lo[3], hi[3];     /* half-open bounding box                                         */
    int32_t  first[3];         /* its voxel with the smallest index z*ny*nx + y*nx + x           */
    uint32_t faces;            /* bit 0..5: has a voxel with x == box_lo[0], x == box_hi[0]-1,
                                  y == box_lo[1], y == box_hi[1]-1, z == box_lo[2], z == box_hi[2]-1 */
} vr_component;
typedef struct vr_components_desc {
    int32_t  src_slot, src_contour;   /* the set: an uploaded slot, component 0..3               */
    int32_t  background;              /* 0: S = voxels of the box IN the contour; 1: those NOT in */
    int32_t  connectivity;
    int32_t  box_lo[3], box_hi[3];    /* half open, 0 <= lo <= hi <= n                           */
    uint64_t min_voxels, max_voxels;  /* selected iff min <= voxels <= max ...                   */
    uint32_t reject_faces;            /* ... and (faces & reject_faces) == 0 ...                 */
    uint32_t keep_largest;            /* ... and, if != 0, among the keep_largest biggest of those (0..VR_COMP_MAX_KEEP) */
    int32_t  dst_slot, dst_contour, combine;   /* dst_slot -1: no contour is written; combine = VR_MORPH_REPLACE .. ANDNOT */
    int32_t  label_slot, label_channel;        /* label_slot -1: no label map                    */
    uint32_t max_components;          /* what `components` holds; 0 with NULL = no table wanted  */
    vr_component* components;         /* host memory                                             */
} vr_components_desc;
typedef struct vr_components_result {
    uint64_t n_components, n_selected;
    uint64_t voxels, selected_voxels;  /* |S|, |R|                                               */
    uint64_t largest;                  /* voxels of the biggest component, 0 if none             */
    int32_t  lo[3], hi[3];             /* half-open bounding box of R, zeros when R is empty     */
} vr_components_result;

/* Fills *out for contour src_contour of the whole volume of src_slot: background = 0, VR_COMP_FACES, the box (0,0,0) .. (nx,ny,nz),
 * min_voxels = 1, max_voxels = UINT64_MAX, reject_faces = 0, keep_largest = 0, both destinations -1 (their components 0, combine
 * VR_MORPH_REPLACE) and no table.  Pure host arithmetic; VR_ERR_INVALID_ARG for a NULL pointer, a slot or a contour out of range,
 * VR_ERR_NOT_READY for an empty slot. */
int vr_components_whole(const vr_ctx* ctx, int src_slot, int src_contour, vr_components_desc* out);

/* Does the work; `result` may be NULL.  Synchronous, on the ctx's own stream: it waits for everything in flight.  When it writes a slot
 * it is a data-preparation call like vr_mask_morph: everything derived from that slot is rebuilt before it returns.  When it writes none
 * it rebuilds nothing.  Either way it leaves what the reporting calls say about earlier launches and tools as it was.  An empty box
 * or an empty set gives zero components and VR_OK (a contour or a label map that was asked for is still written over the box).
 * Checked before anything is enqueued or touched.  VR_ERR_INVALID_ARG: a NULL ctx or descriptor; a slot or component out of range
 * (dst_slot and label_slot may be -1); background not 0 or 1; an unknown connectivity or combine; keep_largest > VR_COMP_MAX_KEEP; bits
 * of reject_faces above bit 5; a box that is not 0 <= lo <= hi <= n on every axis; a contour and a label map in different slots or in
 * the same component; a destination slot whose dimensions differ from the source's; components NULL with a capacity, or given with
 * none.  VR_ERR_NOT_READY: the source slot is empty.  VR_ERR_OOM: the working buffers could not be allocated. */
int vr_mask_components(vr_ctx* ctx, const vr_components_desc* desc, vr_components_result* result);

/* Counters of the last vr_mask_components that got as far as counting (as described above).  Zeros before the first. */
int vr_components_counters(vr_ctx* ctx, uint64_t out[3]);

/* Device time of the last vr_mask_components in milliseconds, from events on the ctx's stream: ms[0] the pack, ms[1] the runs, their
 * scan, the merge and the flatten, ms[2] the numbering, the statistics, the selection, the writes and the copy back (the host's looks at
 * the counts included), ms[3] the rebuild of what is derived from the written slot.  A call that writes no slot reports ms[0 .. 2] and
 * ms[3] = 0, also when it fails only because `components` is too small.  A call that writes a slot reports all four, and zeros
 * when it fails, a table that is too small included (the counters are that call's all the same).  Zeros before the first call and
 * after one that failed otherwise; a call refused for its arguments changes nothing. */
int vr_components_timing(vr_ctx* ctx, float ms[4]);

/* ---- resampling: the values of one volume slot on the grid of another --------------------------------------------------------
 * vr_volume_resample writes selected components of a destination slot, over a voxel box, with values sampled from a source slot at
 * positions an affine map gives -- a dose grid brought onto the CT's, a second series or a registered prior onto the current study's
 * grid, a structure onto the dose grid -- on the device (csrc/vr_resample.h).  Every tool that takes a second slot "of the same
 * dimensions" (the mask rows of vr_histogram, the probe of vr_mask_distance, ...) works on the result.
 *   Position.  Destination voxel (i, j, k) of the box lies at the SOURCE TEXTURE COORDINATE, per component,
 *       p = ((origin + (float)i * di) + (float)j * dj) + (float)k * dk
 *     VR_ARITH_SEPARATE: every product and every sum is rounded.  VR_ARITH_FUSED: the three multiply-adds are fused,
 *     p = fma((float)k, dk, fma((float)j, dj, fma((float)i, di, origin))).  vr_set_arithmetic selects the mode, as for the samples.
 *   Inside.  A voxel is INSIDE iff 0 <= p <= 1 on all three components (a NaN component is outside): the slice views' test.
 *   Stored value, per selected component c (bit c of `channels`):
 *     inside, VR_RESAMPLE_LINEAR   textureSample(src, linear, p).c: the clamp-to-edge texel pairs of p * n - 0.5 and seven lerps
 *                                  (x, then y, then z), a + (b - a) * t each, in the arithmetic mode -- what the shaders sample
 *     inside, VR_RESAMPLE_NEAREST  component c of voxel clamp((int)floor(p * n), 0, n - 1) per axis, its bits unchanged
 *     outside                      outside[c]
 *   What keeps its bits: the components that are not selected, and every voxel outside the box.  The destination is never read.
 *   The uniforms, tables and viewport play no part.
 * Destination slot: an empty dst_slot is created with the dimensions dst_n, every component +0.0f; a filled one must have exactly
 * dst_n.  The call gathers, so src_slot == dst_slot is VR_ERR_INVALID_ARG.
 * Result: inside / outside count the voxels of the box; lo / hi are the half-open bounding box of the inside voxels (destination
 * voxel coordinates), all zero when there are none.
 * Gradients: where .rgb of the source holds gradients, an affine map does not rotate them -- the components are interpolated as the
 * scalars they are stored as.  Resample component 3 alone (channels = 8), then vr_volume_precompute_gradient on the destination.
 * Kernel forms: vr_set_kernel_flavour(1) runs the plain form -- every voxel of the box is positioned and tested, every inside voxel
 * loads the corners of its vec4 voxels.  Every other flavour runs the default form: a wavefront (64 voxels along x) whose voxels are
 * all outside stores `outside` without an address; with channels == 8 the corners are read from the density plane, and, LINEAR,
 * a wavefront whose inside voxels all lie in bricks of ONE value -- by the source's per-brick range records of .a, built on the
 * call's stream when the source changed since they were built -- stores that value without a load (a brick of zeros of either
 * sign gives +0.0f, as the lerps do; csrc/vr_resample.h has the argument).  The destination, the result and out[0] are bit-identical
 * across the forms and the volume layouts.
 *   Counters (vr_resample_counters), out[1] + out[2] == out[0] always: out[0] = voxels of the box; out[1] = voxels for which source
 *   voxels were loaded; out[2] = voxels stored without a load (plain form: exactly the outside voxels). */
#define VR_RESAMPLE_LINEAR 0
#define VR_RESAMPLE_NEAREST 1
typedef struct vr_resample_desc {
    int32_t src_slot, dst_slot;    /* two different slots                                                                      */
    uint32_t channels;             /* 1 .. 15; bit c: component c of dst is written from component c of src                    */
    int32_t filter;                /* VR_RESAMPLE_LINEAR / VR_RESAMPLE_NEAREST                                                 */
    int32_t dst_n[3];              /* nx, ny, nz of the destination grid, 1 .. 65535                                           */
    float origin[3], di[3], dj[3], dk[3];
    float outside[4];              /* per component: stored where p is not inside the source                                   */
    int32_t box_lo[3], box_hi[3];  /* destination voxel box, half open                                                         */
} vr_resample_desc;
typedef struct vr_resample_result {
    uint64_t inside, outside;
    int32_t lo[3], hi[3];
} vr_resample_result;
/* A voxel grid in patient space: n voxels per axis, `origin` the centre of voxel (0,0,0), `spacing` the pitch per axis, one unit. */
typedef struct vr_grid {
    int32_t n[3];
    double origin[3];
    double spacing[3];
} vr_grid;

/* Fills *out for the identity: dst_n = the dimensions (nx, ny, nz) of src_slot, origin = (0.5f / (float)nx, 0.5f / (float)ny,
 * 0.5f / (float)nz), di = (1.0f / (float)nx, 0, 0), dj = (0, 1.0f / (float)ny, 0), dk = (0, 0, 1.0f / (float)nz) -- voxel centres,
 * vr_slice_orthogonal's expressions --, channels = 15, outside = 0, the whole box.  Where every dimension is a power of two the
 * positions are exact and the descriptor reproduces finite source values bit for bit with either filter; elsewhere LINEAR differs
 * from the source in the last bits.  Pure host arithmetic; VR_ERR_INVALID_ARG for a NULL pointer, a slot out of range, equal slots
 * or an unknown filter, VR_ERR_NOT_READY for an empty source slot. */
int vr_resample_identity(const vr_ctx* ctx, int src_slot, int dst_slot, int filter, vr_resample_desc* out);

/* Fills dst_n, origin, di, dj, dk and the whole box of *out -- and nothing else of it -- for destination grid `dst` sampled from
 * source grid `src`; dst_to_src is a row-major 3 x 4 affine map (M | t) from destination patient coordinates to source patient
 * coordinates, NULL = the identity.  Pure host arithmetic in double, IEEE operations in exactly this order, for a = 0, 1, 2 (row a of
 * the map is m = dst_to_src + 4 a; the identity has m[a] = 1.0 and zeros elsewhere):
 *     s_a       = 1.0 / (src->spacing[a] * (double)src->n[a])
 *     v_a       = ((((m[0] * dst->origin[0]) + (m[1] * dst->origin[1])) + (m[2] * dst->origin[2])) + m[3]) - src->origin[a]
 *     origin[a] = (float)((v_a * s_a) + (0.5 / (double)src->n[a]))
 *     di[a]     = (float)((m[0] * dst->spacing[0]) * s_a)
 *     dj[a]     = (float)((m[1] * dst->spacing[1]) * s_a)
 *     dk[a]     = (float)((m[2] * dst->spacing[2]) * s_a)
 * -- origin = A (M o_dst + t - o_src) + 0.5 / n_src, di = A M e_x spacing_dst[0], ... with A = diag(1 / (spacing_src[a] n_src[a])),
 * each of the twelve numbers rounded to float once.  Needs no context.  VR_ERR_INVALID_ARG: a NULL src, dst or out; an n outside
 * 1 .. 65535; a spacing that is not finite and > 0; a matrix entry that is not finite. */
int vr_resample_between(const vr_grid* src, const vr_grid* dst, const double dst_to_src[12], vr_resample_desc* out);

/* Does the work; `result` may be NULL.  A data-preparation call like vr_mask_morph: it waits for everything in flight, runs on the
 * ctx's own stream, rebuilds everything derived from the destination slot as an upload does, and is synchronous on return.  It leaves
 * what the reporting calls say about earlier launches and tools as it was.  An empty box is valid and writes nothing (an empty
 * destination slot is still created).  Everything is checked before anything is enqueued or a slot is touched.
 * VR_ERR_INVALID_ARG: a NULL ctx or descriptor; a slot out of range; src_slot == dst_slot; channels 0 or above 15; an unknown
 * filter; a dst_n outside 1 .. 65535 (or more than 2^32 voxels in all, as for an upload); a filled destination of other dimensions;
 * a box that is not 0 <= lo <= hi <= dst_n on every axis.  No value of origin, di, dj, dk or outside is an error.
 * VR_ERR_NOT_READY: the source slot is empty.  VR_ERR_OOM: the destination or the working buffers could not be allocated. */
int vr_volume_resample(vr_ctx* ctx, const vr_resample_desc* desc, vr_resample_result* result);

/* Counters of the last vr_volume_resample that got as far as counting (as described above).  Zeros before the first. */
int vr_resample_counters(vr_ctx* ctx, uint64_t out[3]);

/* Device time of the last vr_volume_resample in milliseconds, from events on the ctx's stream: ms[0] the preparation (the source's
 * range records, where they had to be built), ms[1] the resample kernel, ms[2] the result words, ms[3] the rebuild of what is derived
 * from the destination slot.  Zeros before the first call and after one that failed. */
int vr_resample_timing(vr_ctx* ctx, float ms[4]);

/* ---- surface extraction: the surface {value >= level} of a component as an indexed triangle mesh -----------------------------------
 * The 3-D counterpart of vr_mask_outlines: the surface of a structure, or the surface VR_VARIANT_ISO renders, as a triangle mesh a
 * caller can save, print, measure or hand to a rasteriser -- extracted on the device (csrc/vr_mesh.h) by MARCHING TETRAHEDRA on the Kuhn
 * (Freudenthal) split of every cell, without the volume passing through the host.  The 16-case rule has no ambiguous case, and the mesh
 * is watertight and combinatorially manifold by construction.  The combinatorics are integer work; a position is two f32 subtractions and
 * one IEEE division.  Every output is a function of the inputs alone, never of scheduling.  The call reads a slot and writes none.
 *   Lattice and cells: lattice point (i, j, k) is the centre of voxel (i, j, k).  With cap = 0 the points are those of the box,
 *     lo <= p < hi, and the cells are the unit cubes with origin o, lo <= o < hi - 1 on every axis: a box thinner than 2 on an axis has
 *     no cells.  With cap = 1 the lattice grows by one layer of VIRTUAL points on every side, lo - 1 <= p <= hi, and the cell origins are
 *     lo - 1 <= o < hi.
 *   Inside: a real point is inside if value >= level (VR_VARIANT_ISO's rule: equal is in; NaN compares false, so NaN is out).  A
 *     virtual point is outside.  `level` must be finite.
 *   Tetrahedra: cell o is split into six tetrahedra, one per permutation (a, b, c) of the axes, in lexicographic order xyz, xzy, yxz,
 *     yzx, zxy, zyx: q0 = o, q1 = q0 + e_a, q2 = q1 + e_b, q3 = q2 + e_c = o + (1,1,1).  Every tetrahedron edge is a lattice edge
 *     (p, p + d) with d in {0,1}^3 \ {0}; its direction code is m = d.x + 2 d.y + 4 d.z (1 .. 7).
 *   Vertices: one per lattice edge whose two ends differ in "inside" and which belongs to some cell.  Its key is (the raster index of p in
 *     the (extended) lattice, x fastest, then y, then z; then m); vertices are numbered 0 .. V - 1 in ascending key order.  With a = p and
 *     b = p + d: t = (level - v_a) / (v_b - v_a) in f32 (two subtractions, one division); !(t >= 0) -> t = 0 (NaN too), t > 1 -> t = 1;
 *     a virtual -> t = 1, b virtual -> t = 0 (the vertex sits on the real end).  The coordinate on an axis is (float)p + t where d is 1 on
 *     that axis, (float)p otherwise: voxel-index units, three f32 per vertex.
 *   Triangles: cells in the raster order of their origins (cap = 0: lo <= o < hi - 1; cap = 1: lo - 1 <= o < hi; x fastest -- the CELL
 *     lattice, one layer shorter per axis than the point lattice), within a cell tetrahedra 0 .. 5.  With v_ij the vertex on edge q_i q_j:
 *     one point alone (q_i inside or outside alone, the others j < k < l): (v_ij, v_ik, v_il); two and two (inside i < j, outside k < l):
 *     (v_ik, v_il, v_jl) then (v_ik, v_jl, v_jk).  The last two indices of a case's triangles are swapped where needed so that
 *     (p1 - p0) x (p2 - p0) points from the inside points toward the outside points for vertices strictly inside their edges: seen from
 *     outside, triangles are counter-clockwise.  The swap is a function of (tetrahedron, case) alone.  Indices are uint32.
 *   A cell whose 8 corners agree yields nothing.  With cap = 1 the mesh is closed for every input; with cap = 0 it is open exactly where
 *     the surface meets the box.  Values equal to the level, or non-finite ones, can give zero-area triangles; they stay in the mesh.
 *   Capacity: max_vertices == max_triangles == 0 is the counting call: VR_OK, the result filled.  If either buffer is too small both
 *     arrays are left untouched, the result is filled all the same, the call returns VR_ERR_INVALID_ARG and vr_last_error names both
 *     needed counts.  More than 2^31 - 1 vertices or triangles in one call: VR_ERR_UNSUPPORTED.
 *   Result: n_vertices, n_triangles = what the surface needs; inside = the real points of the box that are inside; cells = the cells
 *     that emit at least one triangle and lo / hi the half-open box of their origins (zeros if none).
 *   Counters (vr_mesh_counters): out[0] = points of the box, out[1] = voxels loaded by the classification, out[2] = voxels settled from
 *     a range record, out[3] = cells that emit.
 * Kernel forms: for channel 3 the classification settles a voxel from its 4 x 4 x 4 brick's (min, max) record where that decides the
 * test exactly (csrc/vr_mesh.h has the proof); channels 0 .. 2 have no records and every voxel is loaded, and vr_set_kernel_flavour(1)
 * forces that plain form for channel 3 too.  Everything but the counters is identical across the forms and the volume layouts. */
typedef struct vr_mesh_desc {
    int32_t  src_slot, channel;        /* component 0 .. 3 of an uploaded slot                                   */
    float    level;                    /* finite                                                                 */
    int32_t  cap;                      /* 0 / 1: one layer of virtual outside points around the box              */
    int32_t  box_lo[3], box_hi[3];     /* voxel box, half open                                                   */
    uint32_t max_vertices, max_triangles; /* what the two arrays hold                                            */
    float*    vertices;                /* host memory, 3 per vertex; NULL iff max_vertices == 0                  */
    uint32_t* triangles;               /* host memory, 3 per triangle; NULL iff max_triangles == 0               */
} vr_mesh_desc;
typedef struct vr_mesh_result {
    uint32_t n_vertices, n_triangles;  /* what the surface needs, whether or not it was stored                   */
    uint64_t inside;                   /* real points of the box that are inside                                 */
    uint64_t cells;                    /* cells that emit at least one triangle                                  */
    int32_t  lo[3], hi[3];             /* half-open box of those cells' origins, zeros if none                   */
} vr_mesh_result;

/* Fills *out for the whole volume of src_slot: channel 3, level 0.5, cap 0, the box (0,0,0) .. (nx,ny,nz) and no buffers.  Pure host
 * arithmetic; VR_ERR_INVALID_ARG for a NULL pointer or a slot out of range, VR_ERR_NOT_READY for an empty slot. */
int vr_mesh_whole(const vr_ctx* ctx, int src_slot, vr_mesh_desc* out);

/* Does the work; `result` may be NULL.  A synchronous data call on the ctx's own stream: it waits for everything in flight, writes no
 * slot and leaves what the reporting calls say about earlier launches and tools as it was.  An empty box or a surface that does not
 * meet it gives an empty mesh and VR_OK.
 * Checked before anything is enqueued.  VR_ERR_INVALID_ARG: a NULL ctx or descriptor; a slot or channel out of range; a level that is
 * not finite; a cap other than 0 / 1; a box that is not 0 <= lo <= hi <= n on every axis; vertices or triangles NULL with a capacity, or
 * given with none.  VR_ERR_NOT_READY: the slot is empty.  VR_ERR_OOM: the working buffers could not be allocated. */
int vr_volume_mesh(vr_ctx* ctx, const vr_mesh_desc* desc, vr_mesh_result* result);

/* Counters of the last vr_volume_mesh that got as far as counting (as described above).  Zeros before the first. */
int vr_mesh_counters(vr_ctx* ctx, uint64_t out[4]);

/* Device time of the last vr_volume_mesh in milliseconds, from events on the ctx's stream: ms[0] the classification into bit-rows,
 * ms[1] the counts and their scans (the host's look at the totals included), ms[2] the vertex emit, ms[3] the triangle emit and the copy
 * back.  A phase the call did not begin is 0: all four for an empty box, ms[2] and ms[3] for the counting call and for a surface without
 * a vertex.  A call that fails only because vertices or triangles is too small reports ms[0] and ms[1] like the counting call.  Zeros
 * before the first call and after one that failed otherwise; a call refused for its arguments changes nothing. */
int vr_mesh_timing(vr_ctx* ctx, float ms[4]);

/* ---- separable filters: the values of a channel smoothed or differentiated, without leaving the device ---------------------------------
 * Every tool above reads a channel as it was uploaded; this one changes its values: up to three 1-D correlations with caller-given
 * weights, along x, then y, then z, of one component of a volume slot, restricted to a box, written as f32 into one component of a volume
 * slot -- on the device (csrc/vr_filter.h).  Smoothing before vr_volume_mesh, VR_VARIANT_ISO, vr_segment_grow or a threshold, and Gaussian
 * derivatives for the lit shader's gradients, are filters of this kind (vr_filter_gaussian makes their weights).
 *   Passes: the pass along axis a exists iff taps[a] != NULL, with radius r = radius[a] and weights w[0 .. 2r] = taps[a][0 .. 2r] (a NULL
 *     taps[a] goes with radius[a] == 0; a given taps[a] with radius 0 is the one-tap pass out = w[0] * in).  It maps a field `in` to a
 *     field `out`, every value f32:
 *         acc = w[0] * in[i - r]                                     (one rounded product)
 *         for t = 1 .. 2r:  acc = fmaf(w[t], in[i - r + t], acc)     (one fused multiply-add each, in this order)
 *         out[i] = acc
 *     Every tap after the first is an explicit fmaf: vr_set_arithmetic plays no part, and the result is the same in both modes.
 *   Borders: an index i - r + t outside 0 .. n_a - 1 reads the clamped index under VR_FILTER_CLAMP (scipy.ndimage's mode="nearest") and
 *     border_value under VR_FILTER_CONSTANT (mode="constant", cval) -- in every pass, for the source and for an intermediate field alike:
 *     the meaning of correlate1d applied three times.  The faces are the VOLUME's, not the box's: the box only limits which voxels are
 *     stored, and a pass reads real values outside it.
 *   Source and destination: the first pass reads component src_channel of src_slot; the value after the last pass is stored in component
 *     dst_channel of every voxel of the half-open box of dst_slot.  With no pass at all the stored value is the source value, its bits
 *     unchanged.  The other three components of the destination keep their bits, and so does every voxel outside the box.  The result is
 *     that of reading the whole source before anything is written: src_slot == dst_slot with src_channel == dst_channel is valid.  An
 *     empty dst_slot is created with the source's nx, ny, nz and every component +0.0f; one of other dimensions is VR_ERR_INVALID_ARG.
 *   Values: denormals are kept; NaN and +-inf travel as IEEE 754 says (an fmaf with a NaN gives a NaN, whose payload is not specified).
 *     No value of a tap, of border_value or of a voxel is an error.
 *   Result: stored = the voxels of the box; nonfinite = those whose stored value is NaN or +-inf; lo_value / hi_value = the least and the
 *     greatest finite stored value under the order of the value bits that puts -0.0f below +0.0f (exact, independent of scheduling),
 *     +0.0f both when there is none.
 *   Counters (vr_filter_counters): out[0] = voxels of the box; out[1] = the values the passes computed, summed over the passes -- the pass
 *     along axis a computes the box grown on every LATER axis that has a pass by that axis' radius and clipped to the volume; out[2] = the
 *     number of passes.  An empty box gives zeros.
 * Kernel forms: by default a pass loads every input value once per workgroup tile, plus the halo, into LDS and applies the taps from there;
 * flavour 1 of vr_set_kernel_flavour reads the 2r + 1 inputs of every output straight from memory.  The destination, the result and all
 * three counters are identical across the forms and the volume layouts. */
#define VR_FILTER_MAX_RADIUS 32
#define VR_FILTER_CLAMP    0   /* an index beyond a face reads the face's voxel (scipy mode="nearest") */
#define VR_FILTER_CONSTANT 1   /* ... reads border_value (scipy mode="constant")                       */
typedef struct vr_filter_desc {
    int32_t src_slot, src_channel;     /* component 0 .. 3 of a filled slot                                        */
    int32_t dst_slot, dst_channel;     /* may be the same slot, and the same channel                               */
    int32_t radius[3];                 /* per axis x, y, z: 0 .. VR_FILTER_MAX_RADIUS; 0 where taps[a] is NULL     */
    const float* taps[3];              /* host memory, 2 * radius[a] + 1 weights; NULL = no pass along that axis   */
    int32_t border;  float border_value;
    int32_t box_lo[3], box_hi[3];      /* voxel box of the OUTPUT, half open                                       */
} vr_filter_desc;
typedef struct vr_filter_result {
    uint64_t stored, nonfinite;        /* voxels of the box; those whose stored value is NaN or +-inf              */
    float    lo_value, hi_value;       /* least / greatest finite stored value; +0.0f both if there is none        */
} vr_filter_result;

/* Fills *out for the whole volume of src_slot: the given slots and channels, VR_FILTER_CLAMP, border_value 0, no taps (a copy until the
 * caller sets some) and the box (0,0,0) .. (nx,ny,nz).  Pure host arithmetic; VR_ERR_INVALID_ARG for a NULL pointer or a slot or channel
 * out of range, VR_ERR_NOT_READY for an empty source slot. */
int vr_filter_whole(const vr_ctx* ctx, int src_slot, int src_channel, int dst_slot, int dst_channel, vr_filter_desc* out);

/* The weights of a Gaussian (order 0) or of its first derivative (order 1) with standard deviation sigma in voxels, cut off at
 * r = (int)(truncate * sigma + 0.5) -- scipy.ndimage.gaussian_filter1d's kernel.  Pure host arithmetic in double; needs no context.
 *   phi[x] = exp(-0.5 * x * x / (sigma * sigma)) for x = 0 .. r;  S = phi[0] + 2 * (phi[1] + .. + phi[r]), summed in ascending x.
 *   order 0: taps[r + x] = taps[r - x] = (float)(phi[x] / S).
 *   order 1: taps[r + x] = (float)((x / (sigma * sigma)) * phi[x] / S), taps[r - x] = -taps[r + x], taps[r] = +0.0f: correlated with
 *     increasing data they give a positive derivative (gaussian_filter1d(order=1)), in 1 / voxel.
 * *radius = r whenever the arguments are valid.  VR_ERR_INVALID_ARG: radius is NULL; a sigma or truncate that is not finite and > 0; an
 * order other than 0 or 1; r > VR_FILTER_MAX_RADIUS; and, with *radius set all the same, taps NULL or capacity < 2r + 1 -- the counting call. */
int vr_filter_gaussian(double sigma, int order, double truncate, float* taps, int capacity, int* radius);

/* Does the work; `result` may be NULL.  A data-preparation call exactly like vr_mask_distance: it waits for everything in flight, runs on
 * the ctx's own stream, rebuilds what is derived from the destination slot's voxels as an upload does and is synchronous on return.  The
 * weights are copied before it returns.  What the reporting calls say about the last march, slice, histogram or other tool stays as it
 * was.  An empty box writes nothing and is VR_OK.
 * Checked before anything is enqueued or a slot is touched.  VR_ERR_INVALID_ARG: a NULL ctx or descriptor; a slot or channel out of range;
 * a radius outside 0 .. VR_FILTER_MAX_RADIUS, or a nonzero radius with NULL taps; an unknown border; a destination slot of other
 * dimensions; a box that is not 0 <= lo <= hi <= n on every axis.  VR_ERR_NOT_READY: the source slot is empty.  VR_ERR_OOM: the working
 * buffers -- two f32 fields, of the first and of the second pass' region -- could not be allocated.  A failed call changes no slot. */
int vr_volume_filter(vr_ctx* ctx, const vr_filter_desc* desc, vr_filter_result* result);

/* Counters of the last vr_volume_filter (as described above).  Zeros before the first. */
int vr_filter_counters(vr_ctx* ctx, uint64_t out[3]);

/* Device time of the last vr_volume_filter in milliseconds, from events on the ctx's stream: ms[0] the first pass that runs, ms[1] the
 * remaining passes, ms[2] the write into the destination and the result words, ms[3] the rebuild of what is derived from the destination
 * slot.  Zeros before the first and after one that failed. */
int vr_filter_timing(vr_ctx* ctx, float ms[4]);

/* ---- rank filters: the median, the minimum or the maximum over a box window of a channel, without leaving the device --------------------
 * The non-linear neighbourhood filters, which no separable filter expresses: the median (the edge-preserving denoise before
 * vr_segment_grow, vr_volume_mesh, VR_VARIANT_ISO or a threshold) and grey erosion and dilation (the minimum and the maximum of a value
 * field such as a dose, a distance map or a CT, as opposed to the mask morphology of vr_mask_morph) -- on the device (csrc/vr_rank.h).
 *   Window: the window of output voxel (x, y, z) holds N = (2 rx + 1)(2 ry + 1)(2 rz + 1) values: component src_channel of src_slot at
 *     (x + dx, y + dy, z + dz) for |dx| <= rx, |dy| <= ry, |dz| <= rz.  An index beyond a face of the volume reads the clamped index under
 *     VR_FILTER_CLAMP (scipy.ndimage's mode="nearest") and the bits of border_value under VR_FILTER_CONSTANT (mode="constant", cval).  The
 *     faces are the VOLUME's, not the box's: the box only limits which voxels are stored.
 *   Order: the N bit patterns are ordered as unsigned keys -- a pattern with the sign bit set maps to its complement, any other gets the
 *     sign bit set -- which gives  negative NaNs < -inf < .. < -0.0f < +0.0f < .. < +inf < positive NaNs,  NaNs among themselves by
 *     payload: a total order on all 2^32 patterns.  The stored value is the pattern at position k of the ascending order, its bits
 *     unchanged: a NaN keeps its payload, a denormal stays a denormal, and with N = 1 the call is a copy.  k = rank, or N / 2 for
 *     VR_RANK_MEDIAN, or N - 1 for VR_RANK_MAX.  For windows without NaN this is scipy.ndimage.rank_filter's value (where a window holds
 *     both -0.0f and +0.0f, one of scipy's two equal values).  Nothing is computed: vr_set_arithmetic plays no part.
 *   Source and destination: as for vr_volume_filter.  The other three components of the destination keep their bits, and so does every
 *     voxel outside the box.  The result is that of reading the whole source before anything is written: src_slot == dst_slot with
 *     src_channel == dst_channel is valid.  An empty dst_slot is created with the source's nx, ny, nz and every component +0.0f; one of
 *     other dimensions is VR_ERR_INVALID_ARG.
 *   Result: stored, nonfinite, lo_value and hi_value as in vr_filter_result; changed = the voxels of the box whose stored bits differ from
 *     the bits of src_channel of src_slot at the same voxel before the call: how much a median altered.  All five are exact and
 *     independent of scheduling.
 *   Counters (vr_rank_counters): out[0] = voxels of the box; out[1] = voxels of the box grown by the radii and clipped to the volume, the
 *     inputs a call must read; out[2] = the resolved rank k.  An empty box gives zeros.
 * Kernel forms: by default every input is loaded once per workgroup tile, plus the halo, into LDS as keys and selected from there -- by
 * three 1-D running minima or maxima for k = 0 and k = N - 1, by a network in registers for the 3 x 3 x 3 median, by a radix descent
 * otherwise; flavour 1 of vr_set_kernel_flavour reads the N inputs of every output straight from memory into one radix descent.  The
 * destination, the result and all three counters are identical across the forms and the volume layouts. */
#define VR_RANK_MAX_RADIUS 3          /* windows up to 7 x 7 x 7 = 343 values */
#define VR_RANK_MIN      0            /* rank 0: grey erosion by the box        */
#define VR_RANK_MEDIAN (-1)           /* resolves to N / 2                      */
#define VR_RANK_MAX    (-2)           /* resolves to N - 1: grey dilation       */
typedef struct vr_rank_desc {
    int32_t src_slot, src_channel;     /* component 0 .. 3 of a filled slot                                        */
    int32_t dst_slot, dst_channel;     /* may be the same slot, and the same channel                               */
    int32_t radius[3];                 /* per axis x, y, z: 0 .. VR_RANK_MAX_RADIUS; N = the product of 2 r + 1    */
    int32_t rank;                      /* 0 .. N - 1, or VR_RANK_MEDIAN / VR_RANK_MAX                              */
    int32_t border;  float border_value;   /* VR_FILTER_CLAMP / VR_FILTER_CONSTANT, as vr_volume_filter            */
    int32_t box_lo[3], box_hi[3];      /* voxel box of the OUTPUT, half open                                       */
} vr_rank_desc;
typedef struct vr_rank_result {
    uint64_t stored, nonfinite;        /* voxels of the box; those whose stored value is NaN or +-inf              */
    uint64_t changed;                  /* those whose stored bits differ from the source's at the same voxel       */
    float    lo_value, hi_value;       /* least / greatest finite stored value; +0.0f both if there is none        */
} vr_rank_result;

/* Fills *out for the whole volume of src_slot: the given slots and channels, radii 0, VR_RANK_MEDIAN, VR_FILTER_CLAMP, border_value 0 (a
 * copy until the caller sets a radius) and the box (0,0,0) .. (nx,ny,nz).  Pure host arithmetic; VR_ERR_INVALID_ARG for a NULL pointer or a
 * slot or channel out of range, VR_ERR_NOT_READY for an empty source slot. */
int vr_rank_whole(const vr_ctx* ctx, int src_slot, int src_channel, int dst_slot, int dst_channel, vr_rank_desc* out);

/* Does the work; `result` may be NULL.  A data-preparation call exactly like vr_volume_filter: it waits for everything in flight, runs on
 * the ctx's own stream, rebuilds what is derived from the destination slot's voxels as an upload does and is synchronous on return.  What
 * the reporting calls say about the last march, slice, histogram or other tool stays as it was.  An empty box writes nothing and is VR_OK.
 * Checked before anything is enqueued or a slot is touched.  VR_ERR_INVALID_ARG: a NULL ctx or descriptor; a slot or channel out of range;
 * a radius outside 0 .. VR_RANK_MAX_RADIUS; a rank outside 0 .. N - 1 that is neither VR_RANK_MEDIAN nor VR_RANK_MAX; an unknown border; a
 * destination slot of other dimensions; a box that is not 0 <= lo <= hi <= n on every axis.  VR_ERR_NOT_READY: the source slot is empty.
 * VR_ERR_OOM: the working field -- one word per voxel of the box -- could not be allocated.  A failed call changes no slot and no counter. */
int vr_volume_rank(vr_ctx* ctx, const vr_rank_desc* desc, vr_rank_result* result);

/* Counters of the last vr_volume_rank (as described above).  Zeros before the first. */
int vr_rank_counters(vr_ctx* ctx, uint64_t out[3]);

/* Device time of the last vr_volume_rank in milliseconds, from events on the ctx's stream: ms[0] the selection kernel, ms[1] any further
 * ones (0: every form selects in one kernel), ms[2] the write into the destination and the result words, ms[3] the rebuild of what is
 * derived from the destination slot.  Zeros before the first and after one that failed. */
int vr_rank_timing(vr_ctx* ctx, float ms[4]);

/* ---- the gamma index: comparing two dose channels, without leaving the device -------------------------------------------------------------
 * The gamma index of Low et al. (Med. Phys. 25, 1998): for every voxel of the reference dose the minimum, over nearby points of the
 * evaluated dose, of dose difference and distance combined -- a plan against a recalculation, a measurement or yesterday's plan -- on the
 * device (csrc/vr_gamma.h).  vr_volume_resample puts two doses on one grid before; vr_histogram and the slice views consume the result.
 * Every f32 operation is named; vr_set_arithmetic plays no part (every fused step is an explicit fmaf, every other step stays unfused).
 *   Operands: R = component ref_channel of ref_slot, E = component eval_channel of eval_slot; both slots filled and of equal dimensions
 *     (nx, ny, nz).  Output voxels are those of the half-open box.
 *   Spacing and distances: spacing[3] (x, y, z) in an integer unit of the caller's choice (micrometres, say), each 1 .. 2^20 as in
 *     vr_dist_desc; dta (distance to agreement) and reach (how far the search goes) in the same unit, each 1 .. 2^24; sub = candidate
 *     positions per voxel step and axis, 1 .. VR_GAMMA_MAX_SUB.  reach / spacing[a] (integer division) must be <= VR_GAMMA_MAX_RADIUS
 *     on every axis, else VR_ERR_INVALID_ARG.
 *   Candidates of an output voxel p: integer sub-step offsets o = (i, j, k) with
 *     D2n(o) = (i spacing[0])^2 + (j spacing[1])^2 + (k spacing[2])^2 <= (reach sub)^2, both exact in uint64_t.  Per axis
 *     o_a = sub m_a + f_a with floor division, 0 <= f_a < sub; the base voxel is b = p + m.  The candidate EXISTS iff 0 <= b_a and
 *     b_a + (f_a > 0 ? 1 : 0) <= n_a - 1 on every axis.  The faces are the VOLUME's, not the box's, and there is no border mode: a
 *     position outside the volume is not a candidate.
 *   Value at a candidate: t_a = (float)f_a / (float)sub (one rounded division); lerp(u, v, t) = fmaf(t, v - u, u) with v - u one rounded
 *     subtraction; E is interpolated along x between the corner pairs of b, then along y, then along z.  An axis with f_a == 0 takes its
 *     lower value as it is -- no arithmetic, the upper neighbour is not read.  The result is e; with sub = 1 it is E at b.
 *   Tolerance: r = R(p).  VR_GAMMA_GLOBAL: T = dose_tolerance (3 % of the prescription, say: the caller's number).  VR_GAMMA_LOCAL:
 *     T = dose_tolerance * r, one rounded product (dose_tolerance a fraction such as 0.03f).  invT = 1.0f / T, the IEEE division.
 *   Skipped voxels: p is skipped if !(r >= cutoff) (a NaN r is skipped), if T is not finite or not > 0, or if roi_slot != -1 and
 *     component roi_contour of roi_slot at p is not in the contour (vr_mask_distance's rule: != 0.0f, NaN is in, -0.0f is out).  A
 *     skipped voxel stores the bits of skip_value, whatever they are.
 *   Gamma: kc = (float)(1.0 / ((double)dta * dta * sub * sub)), computed on the host.  Per candidate c = (float)D2n * kc (the uint64_t ->
 *     f32 conversion rounded to nearest, then one product), d = (e - r) * invT (one rounded subtraction, one product),
 *     g2 = fmaf(d, d, c).  G2 = the least g2 over the existing admitted candidates, a NaN g2 ignored; if every g2 is NaN, G2 is the NaN
 *     0x7FC00000.  The stored value is the correctly rounded f32 square root of G2.  The voxel PASSES iff G2 <= 1.0f.
 *   Why the order of candidates cannot matter: g2 is +0 or positive, never -0 (d * d >= +0 and c >= +0, and a sum of those is never
 *     -0), so the minimum is one bit pattern whatever the order.
 *   Why the search may be cut short exactly: rounding is monotone and d * d >= 0, so g2 = round(d * d + c) >= round(c) = c always.  A
 *     candidate whose c is not below the running minimum therefore cannot lower it and may be left out; with the candidates in
 *     ascending c, everything after the first such candidate may.
 *   Source and destination: the stored values go into component dst_channel of the box's voxels of dst_slot; the other three components
 *     and every voxel outside the box keep their bits.  The result is that of reading both doses and the ROI before anything is
 *     written: the destination may be either dose's slot and channel.  An empty dst_slot is created with the reference's dimensions and
 *     every component +0.0f; one of other dimensions is VR_ERR_INVALID_ARG.
 *   Result: stored = voxels of the box; evaluated = those not skipped; passed = evaluated voxels with G2 <= 1; nonfinite = evaluated
 *     voxels whose stored value is NaN or +inf; hi_value = the greatest finite stored value among evaluated voxels, +0.0f if there is
 *     none.  All exact and independent of scheduling.
 *   Counters (vr_gamma_counters): out[0] = voxels of the box; out[1] = evaluated voxels; out[2] = K, the number of admitted offsets.  An
 *     empty box gives zeros.
 * Kernel forms: the host builds the table of admitted offsets, ascending D2n with ties by (k, j, i), each with its c.  By default a
 * workgroup stages E for a tile of outputs plus the halo in LDS and walks the table until no lane of a wavefront has a c below its
 * running minimum; flavour 1 of vr_set_kernel_flavour visits every admitted candidate of every voxel from memory, with no cut.  The
 * destination, the result and all three counters are identical across the forms and the volume layouts. */
#define VR_GAMMA_MAX_SUB    4
#define VR_GAMMA_MAX_RADIUS 8
#define VR_GAMMA_GLOBAL 0
#define VR_GAMMA_LOCAL  1
typedef struct vr_gamma_desc {
    int32_t  ref_slot, ref_channel;     /* R: component 0 .. 3 of a filled slot                                     */
    int32_t  eval_slot, eval_channel;   /* E: the same, of a slot of equal dimensions                               */
    int32_t  dst_slot, dst_channel;     /* where gamma goes; may be either dose's slot and channel                  */
    int32_t  roi_slot, roi_contour;     /* voxels outside this contour are skipped; roi_slot = -1: none             */
    uint32_t spacing[3];                /* x, y, z: 1 .. 2^20 each                                                  */
    uint32_t dta, reach;                /* same unit: 1 .. 2^24 each; reach / spacing[a] <= VR_GAMMA_MAX_RADIUS     */
    int32_t  sub;                       /* candidate positions per voxel step and axis: 1 .. VR_GAMMA_MAX_SUB       */
    int32_t  mode;                      /* VR_GAMMA_GLOBAL / VR_GAMMA_LOCAL                                         */
    float    dose_tolerance;            /* T (global), or the fraction of r (local)                                 */
    float    cutoff;                    /* voxels with !(r >= cutoff) are skipped; -inf: none                       */
    float    skip_value;                /* what a skipped voxel stores, bit for bit                                 */
    int32_t  box_lo[3], box_hi[3];      /* voxel box of the OUTPUT, half open                                       */
} vr_gamma_desc;
typedef struct vr_gamma_result {
    uint64_t stored, evaluated;         /* voxels of the box; those not skipped                                     */
    uint64_t passed, nonfinite;         /* evaluated voxels with G2 <= 1; those whose stored value is NaN or +inf   */
    float    hi_value;                  /* greatest finite stored value among evaluated voxels; +0.0f if none       */
    uint32_t reserved;                  /* 0                                                                        */
} vr_gamma_result;

/* Fills *out for the whole volume of ref_slot: the given slots and channels, unit spacing, dta = reach = 1, sub 1, VR_GAMMA_GLOBAL,
 * dose_tolerance 1.0f, cutoff -inf, no ROI (roi_slot -1), skip_value the NaN 0x7FC00000 and the box (0,0,0) .. (nx,ny,nz).  Pure host
 * arithmetic; VR_ERR_INVALID_ARG for a NULL pointer or a slot or channel out of range, VR_ERR_NOT_READY for an empty reference slot. */
int vr_gamma_whole(const vr_ctx* ctx, int ref_slot, int ref_channel, int eval_slot, int eval_channel, int dst_slot, int dst_channel,
                   vr_gamma_desc* out);

/* Does the work; `result` may be NULL.  A data-preparation call exactly like vr_volume_filter: it waits for everything in flight, runs on
 * the ctx's own stream, rebuilds what is derived from the destination slot's voxels as an upload does and is synchronous on return.  What
 * the reporting calls say about the last march, slice, histogram or other tool stays as it was.  An empty box writes nothing and is VR_OK.
 * Checked before anything is enqueued or a slot is touched.  VR_ERR_INVALID_ARG: a NULL ctx or descriptor; a slot (the ROI's: other than
 * -1), channel or contour out of range; a spacing outside 1 .. 2^20; dta or reach outside 1 .. 2^24; sub outside 1 .. VR_GAMMA_MAX_SUB;
 * reach / spacing[a] above VR_GAMMA_MAX_RADIUS; an unknown mode; an evaluated, ROI or destination slot of other dimensions than the
 * reference's; a box that is not 0 <= lo <= hi <= n on every axis.  VR_ERR_NOT_READY: the reference, evaluated or ROI slot is empty.
 * VR_ERR_OOM: the working field -- two words per voxel of the box -- or the offset table could not be allocated.  A failed call changes no
 * slot and no counter. */
int vr_volume_gamma(vr_ctx* ctx, const vr_gamma_desc* desc, vr_gamma_result* result);

/* Counters of the last vr_volume_gamma (as described above).  Zeros before the first. */
int vr_gamma_counters(vr_ctx* ctx, uint64_t out[3]);

/* Device time of the last vr_volume_gamma in milliseconds, from events on the ctx's stream: ms[0] the gamma kernel, ms[1] any further
 * ones (0: every form searches in one kernel), ms[2] the write into the destination and the result words, ms[3] the rebuild of what is
 * derived from the destination slot.  Zeros before the first and after one that failed. */
int vr_gamma_timing(vr_ctx* ctx, float ms[4]);

/* Volume layout in HBM (A/B measurements; frames and counts are bit-identical in every mode).
 *   0  default: the march kernels gather from a BRICKED copy of every slot -- the vec4 voxels and a scalar f32 density plane
 *      (what fetches that consume .a alone read: BasicVolumeApp.wgsl:171, the density / dose fetches of the other shaders)
 *      in bricks of 4 x 4 x 4 voxels, brick after brick: 1 KiB per brick, a 128-byte line = 4 x 2 x 1 voxels, so that the
 *      lines a packet of rays needs next are near the ones it has whatever direction it travels in.  The reference's
 *      x-fastest array (App/src/file/VolumeFile.cpp:287-307: what vr_volume_upload takes, the data-preparation calls work on
 *      and vr_volume_download returns) stays resident beside it; the copy is rebuilt after every upload / in-place change
 *   3  round 2's default: the reference's x-fastest vec4 voxels + an x-fastest density plane
 *   1  the reference's RGBA32F voxels only (16 B / voxel; what round 1 measured)
 *   2  (removed: the lit shader's gradients derived from the plane on the fly -- measured slower)
 *      VR_ERR_UNSUPPORTED
 * vr_volume_layout: *flags bit 0 = density plane present, bit 1 = .rgb verified, at upload, as the central difference of .a
 * (VolumeFile::PreComputeGradient(false), VolumeFile.cpp:196-257, bit for bit), bit 2 = no longer set (it said the last
 * render derived its gradients on the fly: layout 2), bit 3 = the bricked copy is what the gathers read.  */
int vr_set_volume_layout(vr_ctx* ctx, int mode);
int vr_volume_layout(vr_ctx* ctx, int slot, int* flags);

/* The flavour the last render actually ran (what 0 resolved to for that launch), or a negative vr_status. */
int vr_last_kernel_flavour(vr_ctx* ctx);

/* The brick distance field a launch of `variant` would use now: built / refreshed synchronously, copied to `dist`
 * (min(capacity, n) bytes, x fastest), the brick grid in dims[3], the active-brick box (brick coordinates, inclusive;
 * hi < 0 if none) in box[6], the number of active bricks in *active.  Each byte is min(Chebyshev distance in bricks to
 * the nearest active brick, 128): 0 for an active brick, 128 everywhere when none is active.  Drains the device.
 * Returns n, or a negative vr_status (VR_ERR_NOT_READY when such a launch would not skip empty space).             */
int vr_skip_field(vr_ctx* ctx, int variant, uint8_t* dist, size_t capacity, int dims[3], int box[6], uint64_t* active);

/* The hull of the active bricks of that field, which the skipping launches prune their rays with: lo[i] / hi[i] = the
 * smallest / largest n_i . b over the active bricks b (brick coordinates), for the 13 directions n_i, in this order:
 *   (1,0,0) (0,1,0) (0,0,1)  (1,1,0) (1,-1,0) (1,0,1) (1,0,-1) (0,1,1) (0,1,-1)  (1,1,1) (1,1,-1) (1,-1,1) (1,-1,-1)
 * The first three pairs are vr_skip_field's box.  No active brick: lo[i] = INT_MAX, hi[i] = INT_MIN for every i.  Built
 * synchronously like vr_skip_field, with its conditions and errors; drains the device.  Returns VR_OK or a negative vr_status. */
int vr_skip_hull(vr_ctx* ctx, int variant, int lo[13], int hi[13]);

/* 1 when the skipping kernels can index the bricks of an nx x ny x nz volume (THE BRICK-INDEX LIMIT at vr_set_kernel_flavour),
 * 0 when launches on such a volume run without skipping.  Needs no context and no device.                              */
int vr_skip_indexable(uint16_t nx, uint16_t ny, uint16_t nz);

/* How many skipping launches ran with no active-brick box because an asynchronous rebuild's box had not reached the
 * host yet (vr_tf_upload_opacity_async), since the context was created. */
int64_t vr_unbounded_box_launches(vr_ctx* ctx);

#ifdef __cplusplus
}
#endif
#endif /* VR_H_ */
