// vr_device.h -- device-side data structures shared by the kernels and the C-ABI implementation.
// gfx950 (MI355X) only.  All arithmetic IEEE f32, compiled with -ffp-contract=off.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "vr_choice.h"  // kTile, the brick shifts, kOrderMaxBlocks; KernelForm::Family
#include "vr_units.h"
// (the hull of the active bricks: plain C++ that the kernels and the host share; the device's reciprocal is v_rcp_f32)
#define VR_HULL_FN __host__ __device__ __forceinline__
#ifdef __HIP_DEVICE_COMPILE__
#define VR_HULL_RCP(x) __builtin_amdgcn_rcpf(x)
#endif
#include "vr_hull.h"

namespace vr {

constexpr int kBlockEdge = 16;   // one 256-thread workgroup = 16x16 pixels = four 8x8 wave packets
constexpr int kBlockRecord = 6;  // u64 words per block in MarchParams::block_counts
constexpr int kBlocksPerTile = (kTile / kBlockEdge) * (kTile / kBlockEdge);
// Empty-space bricks of 4 x 4 x 4 base cells (a brick's cells touch 5 x 5 x 5 voxels).  Round 1 used 8-cell bricks; 4-cell
// ones leave 6.5 % fewer samples of C3 (39 % of C2) inside active bricks for a distance field 8 times the size (2 MB for
// 512^3, 16 MB for 1024^3: one byte per brick) and are faster on every configuration (C3 0.573 -> 0.562 ms one frame at a
// time, 0.435 -> 0.423 batched; C2 0.119 -> 0.103 / 0.072 -> 0.065; C5 3.31 -> 3.28); 2-cell bricks fetch less still and
// are slower again (the look-ups), and their index outgrows a launch at 1024^3.  -DVR_BRICK_SHIFT=3 rebuilds round 1's.
// (kBrickShift, kBrickCells: vr_choice.h)
constexpr float kBrickInv = 1.0f / (float)kBrickCells;    // exact
constexpr float kBrickHalf = 0.5f / (float)kBrickCells;   // half a cell in brick units (the -0.5 of the cell coordinate)
#ifndef VR_DIST_MAX
#define VR_DIST_MAX 128
#endif
constexpr int kDistMax = VR_DIST_MAX;  // cap of the brick distance field
// (the builder's x pass sees 128 bricks to either side of a wavefront's 64, and its y / z tiles take 2 x (kDistMax - 1) rows of halo)
static_assert(kDistMax >= 2 && kDistMax <= 128, "the distance-field builder (vr_skipfield.h) is exact for caps up to 128");

// What a distance-field build reports to the host (pinned memory, written by its last workgroup): the active bricks and their box
// (brick coordinates, inclusive; hi < 0 if none).  `gen` is written last: the values belong to build `gen` once it reads so.
// hull_lo / hull_hi: min / max of n . b over the active bricks b for the ten diagonal directions of vr_hull.h (kHullDir[3 ..]); not
// written when there is none.
struct SkipSummary {
    unsigned long long gen;
    unsigned long long count;
    int box[6];
    int hull_lo[kHullDirs - kHullAxes], hull_hi[kHullDirs - kHullAxes];
};
// (the storage bricks of the bricked volume copy, kVbS / kVbM / kVbN: vr_choice.h)

struct DevVolume {
    const float4* data;  // reference layout: x fastest, (k*ny + j)*nx + i   (VolumeFile.cpp:306)
    // Scalar density plane: the .a of every voxel, same order, 4 B per voxel (built at upload, rebuilt after every in-place
    // change).  Every fetch that consumes .a alone reads it instead of the 16-byte voxels -- a quarter of the footprint in
    // L2 / Infinity Cache / HBM and four times the voxels per cache line.  a_base / a_shift address either form without a
    // branch: byte offset of voxel idx's density = idx << a_shift from a_base (the plane, or data + 12 bytes when the plane
    // is switched off for A/B measurements).
    const float* dens;
    const char* a_base;
    int a_shift;
    int nx, ny, nz;
    // Bricked layout (default, vr_set_volume_layout(0)): `data` and the density plane behind `a_base` hold the voxels
    // in bricks of 4 x 4 x 4, brick after brick (x fastest), the 64 voxels of a brick in x-fastest order: voxel (x, y, z) lives at
    //     (x >> 2) * 64 + (x & 3)  +  (y >> 2) * brick_row + (y & 3) * 4  +  (z >> 2) * brick_slab + (z & 3) * 16
    // (written with kVbS / kVbM / kVbN in the code: the brick edge is a build-time constant)
    // -- a sum of one term per axis, so the eight corners of a cell are sums of two terms per axis.  A 1 KiB brick is eight
    // 128-byte lines of 4 x 2 x 1 voxels: the 7 x 7 x 2 voxel patch a packet's corner load touches spans ~20 lines instead of
    // the ~30 of the reference's x-fastest rows, and the lines a ray needs next lie in the same or the neighbouring brick
    // whatever direction it travels in (with x-fastest rows a ray along z changes its 4 MiB slice every step).  bricked == 0:
    // the reference's order (VolumeFile.cpp:306), idx = (z * ny + y) * nx + x.
    int bricked;
    unsigned brick_row, brick_slab;  // voxels per row of bricks (ceil(nx / 4) * 64) and per slab of bricks (* ceil(ny / 4))
    unsigned data_bytes;             // size of `data` (the range of the kernels' buffer loads; volumes below 4 GiB)
    // 1: the workgroup's dynamic LDS holds this (bricked) volume's per-axis SLOT TABLES -- entry e (0 .. n + 1) of an axis = the slot
    // term of texel clamp(e - 1, 0, n - 1), the three axes one after the other -- and make_cell() reads the clamp-to-edge texel
    // pair of a coordinate t (-1 .. n - 1) as the entries t + 1, t + 2 with one ds_read2_b32 instead of computing clamps, shifts,
    // masks and multiplies (flavour 18: march_kernel fills the tables per workgroup; 0 elsewhere)
    int lut;
};

// Both tables are stored with their first and their last texel repeated once at either end: table[k] is at [k+1].
// The clamp-to-edge texel pair (i0, i1) of a linear fetch is then ALWAYS the adjacent pair [j], [j+1] with
// j = clamp(floor(x) + 1, 0, R): one index, no second clamp, and the second texel sits at a fixed offset.
struct DevTF {
    const float* opacity;  // R32Float[res_o + 2]     (OpacityTf.cpp:25-26)
    const float4* color;   // RGBA32Float[res_c + 2]  (ColorTf.cpp:23-24)
    int res_o, res_c;
};

// Kernel argument block (passed by value, lives in SGPRs / kernarg segment).
struct MarchParams {
    float proj_inv[16];
    float view_inv[16];
    int W, H;
    int fragment_mode;
    int steps_count;
    float step_size;
    float bmin[3], bmax[3];  // IsInSampleCoords bounds: 0.0f + clip?.x, 1.0f - clip?.y
    int toggle_varstep, toggle_jitter;
    float light_pos[3], light_amb[3], light_dif[3];
    float camera_pos[3];     // cameraPosition uniform (illustrative shader only)
    DevVolume vol[3];
    DevTF tf[2];
    // work decomposition: the launch walks the 64x64 tiles t = rank + n*world, n = 0..n_tiles-1
    int rank, world, tiles_x, tiles_y, n_tiles;
    int packed;              // 0: write frame[y*W+x]; 1: write packed tiles
    int rect[4];             // x0, y0, x1, y1 (inclusive): no ray outside this pixel rectangle can hit the box
    int n_blocks;            // logical blocks = n_tiles * kBlocksPerTile (grid is padded to a multiple of 8)
    // exact empty-space skipping (BASIC / LIGHT / THREE_FILES): per-brick maximum density of vol[0] over the
    // (c+1)^3 voxels a brick of c^3 base cells can touch (c = kBrickCells), and the length of the opacity table's zero prefix
    const float2* bricks;    // nullptr = disabled; per brick: x = max of vol[skip_vol].a, y = max(r,g,b) of the mask
                             // (y is filled from vol[0]'s bricks for VOLUME_MASK and is 0 otherwise)
    int use_rgb;             // VOLUME_MASK: a brick is inert only if its mask record y <= 0
    const unsigned char* brick_dist;  // per brick: 0 = active; k >= 1 = inert and every brick within Chebyshev
                                      // distance k-1 is inert too (capped); rebuilt when the volume / opacity table change
    int skip_vol;            // which volume carries the density that drives the opacity (0, or 2 for VOLUME_MASK)
    float abox[6];           // uvw box (lo xyz, hi xyz) around the ACTIVE bricks of brick_dist, one brick of margin: outside it nothing is sampled
                             // (the three axes of their hull, vr_hull.h; the ten diagonals: hull_lo / hull_hi at the end)
    int bnx, bny, bnz;       // bricks per axis
    float bsx, bsy, bsz;     // n / kBrickCells per axis of vol[skip_vol] (exact in f32)
    int tf_zero_prefix;      // largest Z with opacity[0..Z] == 0 exactly (-1: none); also the per-step vote of sample_and_blend
    // Launch order of the logical blocks: workgroup blockIdx.x works on logical block order[blockIdx.x] (nullptr =
    // identity).  The host sorts the blocks of the previous frame by their longest ray chain, longest first, so that the
    // long blocks start at once and the short ones fill the machine at the end (speed only: a permutation of the blocks).
    const unsigned* order;
    float4* out;
    unsigned long long* block_counts;  // [blocks of this frame][kBlockRecord]: composited, covered, fetched, t0, t1, hw id
    unsigned batch_n;        // frames the launch carries (1 .. kBatchMax): see MarchBatch
    float iso;               // VR_VARIANT_ISO: the level (vr_set_iso_value) when the launch was enqueued (in the tail padding after
                             // batch_n: the size and every other offset of the struct are what they were without it).  Surface
                             // launches of the unlit / lit shader (vr_surf.h), which read no level: the alpha threshold
    // The ten diagonal plane pairs of the active bricks' hull (vr_hull.h: lo <= g . p <= hi in brick units, margin included), which the
    // skipping marches prune their rays with beside abox.  At the end: every other offset of a frame is what it was without them.
    float hull_lo[kHullDiag], hull_hi[kHullDiag];
};

// One launch may carry up to kBatchMax frames of the same scene and shape (different uniforms, output and record buffers).
// A rank's share of a frame on N GPUs, or a small frame, is a launch too short to fill the machine; several of them in one
// launch do, without depending on how many streams the runtime really runs side by side.  The frames are
// interleaved in groups of 8 workgroups: group g = blockIdx.x / 8 belongs to frame g % n_frames and is that frame's group
// g / n_frames -- so a workgroup keeps the XCD residue of its index within the frame, and the longest-first launch order
// (MarchParams::order) holds across the whole launch: the long workgroups of EVERY frame start first.  (Frame after frame,
// the last frame's long ray chains would start when the others' blocks have all been dispatched.)  Passed by value:
// 4 x ~0.7 KB of the 4 KB kernarg segment.
constexpr int kBatchMax = 4;
struct MarchBatch {
    MarchParams frame[kBatchMax];
    unsigned n_frames;
};
static_assert(sizeof(MarchBatch) + 256 <= 4096, "a launch's frames, its queue and the hidden arguments share the 4 KB kernarg segment");

// Kernel argument block of a slice view (slice_kernel, vr_slice.h; vr_slice_desc of include/vr.h): passed by value.  A slice has
// a geometry of its own -- a plane in texture space, any output size, any volume and TF slot -- and reads nothing of MarchParams.
struct SliceParams {
    DevVolume vol;           // the sliced slot, in the layout in use
    DevTF tf;                // the TF slot
    float origin[3], du[3], dv[3], dn[3];
    int width, height;       // of the output
    int tiles_x;             // 8x8 pixel tiles per row: workgroup t works on tile (t % tiles_x, t / tiles_x)
    int slab_steps;
    int format;              // VR_SLICE_RGBA32F: float4 per pixel, VR_SLICE_BGRA8: the presented 32-bit word
    const float2* bricks;    // SKIP: (min, max) of the slot's .a per empty-space brick ...
    const float2* vrange;    // ... and over the whole volume (vr_proj.h)
    int bnx, bny, bnz;       // bricks per axis
    float bsx, bsy, bsz;     // n / kBrickCells per axis (exact in f32)
    void* out;               // width * height pixels, row-major
    unsigned long long* counts;  // [workgroups][3]: counted samples, pixels with a sample, samples loaded
};

// The device words of one resample (vr_resample.h): what the host sets before the kernel and reads behind it.
struct ResampleWords {
    CountBox inside;            // the inside voxels of the box and their bounding box (starts as CountBox::empty())
    unsigned long long loaded;  // voxels for which source voxels were loaded
};

// Kernel argument block of a resample (resample_kernel, vr_resample.h; vr_resample_desc of include/vr.h): passed by value.  Like a
// slice it has a geometry of its own and reads nothing of MarchParams.
struct ResampleParams {
    DevVolume src;           // the source slot, in the layout in use
    float4* dst;             // the destination's x-fastest vec4 voxels
    int n[3];                // nx, ny, nz of the destination grid
    int lo[3], hi[3];        // the destination voxel box, half open
    unsigned ux;             // 64-voxel units per row of the box: ceil((hi[0] - lo[0]) / 64)
    unsigned long long units;  // ux * rows * slices of the box: unit u is 64 voxels along x of row u / ux
    float origin[3], di[3], dj[3], dk[3];
    float outside[4];
    unsigned channels;       // bit c: component c is written
    const float2* bricks;    // exact settling: the source's range records (vr_proj.h), bnx x bny x ... bricks; nullptr = off
    int bnx, bny;
    ResampleWords* w;
};

// Kernel argument block of a histogram (hist_kernel, vr_hist.h; vr_hist_desc of include/vr.h): passed by value.
struct HistParams {
    const float* val;        // the value of voxel idx is val[idx * val_stride]: the channel of the x-fastest vec4 voxels (stride 4),
    int val_stride;          // or the density plane (stride 1: channel 3 of an unmasked launch, when the layout has one)
    const float4* mask;      // the mask slot's x-fastest vec4 voxels; nullptr = no mask
    int nx, ny, nz;          // of the value volume (and of the mask)
    BoxUnits box;            // the voxel box and the 4 x 4 x 4 brick units that meet it (vr_units.h)
    unsigned rows;           // bit r: row r is computed
    unsigned bins;
    float scale;
    int drop;                // VR_HIST_DROP
    int lds;                 // the counts go through a private u32 copy in LDS (dynamic, rows computed * bins words)
    const float2* bricks;    // exact settling: the slot's range records (vr_proj.h), bnx x bny x ... bricks; nullptr = off
    int bnx, bny;
    unsigned long long* counts;    // [VR_HIST_ROWS][bins]
    unsigned long long* row_sums;  // [VR_HIST_ROWS][2]: voxels, dropped (vr_hist_row)
    unsigned long long* stats;     // [3]: voxels of the box, voxels loaded, voxels settled from a record
};

// The device words of one region grow (vr_grow.h): what the host sets before the first kernel and reads behind a batch of rounds.
struct GrowWords {
    unsigned long long stats[3];  // voxels of the box, voxels loaded, voxels classified from a range record
    CountBox reached;             // |R| and its bounding box (starts as CountBox::empty())
    unsigned cnt[3];              // round k reads cnt[k % 3] (frontier: the length of its list; sweep: the round before it changed
                                  // something), adds to cnt[(k + 1) % 3] and zeroes cnt[(k + 2) % 3]
    unsigned rounds;              // the last round that had something to do
};

// Kernel argument block of a region grow (vr_grow.h; vr_grow_desc of include/vr.h): passed by value.
struct GrowParams {
    const float* val;        // the value of voxel idx is val[idx * val_stride]: as HistParams
    int val_stride;
    int nx, ny, nz;          // of the value volume (and of the mask)
    BoxUnits box;            // the voxel box and the brick units that meet it
    float vlo, vhi;          // a voxel qualifies iff v >= vlo && v <= vhi
    const float2* bricks;    // exact settling: the slot's range records (vr_proj.h); nullptr = off
    int bnx, bny, bnz;       // the volume's brick grid: brick (bx, by, bz) has index (bz * bny + by) * bnx + bx
    unsigned n_bricks;
    int all;                 // VR_GROW_ALL: 26 neighbours instead of 6
    unsigned long long* q;   // per brick: bit x + 4 y + 16 z = the voxel qualifies (and lies in the box)
    unsigned long long* r;   // ... = the voxel is reached
    unsigned* stamp;         // frontier: per brick, the last round it was queued for
    unsigned* list[2];       // frontier: round k reads list[k & 1] and fills list[(k + 1) & 1] (n_bricks words each)
    GrowWords* w;
    unsigned round;          // 1, 2, ...
    float4* mask;            // the mask slot's x-fastest vec4 voxels
    int contour;             // the component written
    int write_zeros;         // VR_GROW_REPLACE into a slot that held a mask: voxels outside R are stored +0.0f
};
struct GrowSeeds {
    unsigned n;
    int xyz[64][3];
};

// (The argument blocks of the bit-row mask tools live with their kernels: vr_bitrows.h, vr_morph.h, vr_dist.h, vr_raster.h.)
// Work queue of the persistent-wavefront kernel (vr_pw.h): eight heads, one per class of the workgroup index modulo 8,
// zero at launch; heads[c * 64] counts the items of class c handed out beyond every wavefront's first.
struct PwQueue {
    unsigned* heads;
    unsigned n_items;  // logical blocks of the launch (a multiple of 8)
    unsigned p2_window;  // march_p2_kernel<.., WIN>: records per gather window when not 0 (tests: a small window on a small volume)
};

// What enqueue_render decided about one march launch; handed to launch_march of the arithmetic mode's translation unit
// (vr_launch.h: namespace vr = separately rounded multiply-adds, namespace vrf = fused).  Host only.
struct LaunchDesc {
    int variant;      // vr_variant
    KernelForm::Family family;  // which kernel (vr_choice.h: KernelForm::Family; kShader says which shaders have it).  What a family reads
                      // beyond the batch: kPw / kP2 the packets from `queue` (grid = workgroups); kShadow MarchParams::vol[1] = the light
                      // volume; kSurf MarchParams::iso = the threshold; kBound MarchParams::vol[1].data / vol[2].data = the near / far
                      // depth buffers, W*H floats each or nullptr
    bool off32;       // every bound volume < 4 GiB: 32-bit byte offsets
    int lanes;        // KernelForm::lanes
    bool pipe;        // KernelForm::pipe (dropped at the launch where the shader has no pipelined form: ShaderTraits::kDpPipe / kPwPipe)
    bool ltf;         // kPw: TF slot 0 in LDS (lds_bytes of dynamic LDS)
    bool p2_win;      // kP2: a bound volume of 4 GiB or more: the gather window moves (march_p2_kernel<.., WIN>)
    unsigned lds_bytes;
    PwQueue queue;
    dim3 grid, block;
    bool skip;        // the skipping form of a flavour pair, asked for only with its records in place (KernelForm::skip, vr_api.hip).
                      // kP2: skipping by whole wavefronts on the distance field (march_p2_kernel<V, true>); kProj / kIso: by volume
                      // 0's range records in MarchParams::bricks (march_proj_kernel / march_iso_kernel / iso_point_kernel<.., SKIP = true,
                      // ..>); kShadow / kSurf / kBound: by the distance field (march_shadow_kernel / march_surf_kernel / march_bound_kernel<.., true, ..>).  The other
                      // families read MarchParams::brick_dist alone.
    const float2* vrange;  // kProj: (min, max) of volume 0 (vr_proj.h)
    bool surface;          // kIso: the refined point instead of the shaded fragment (iso_point_kernel, vr_iso.h)
};

// The forms of resample_kernel (vr_resample.h): the plain one (vr_set_kernel_flavour(1)); the default one; the default one of a launch
// that writes component 3 alone, which reads the density plane and settles wavefronts by the range records where it has them.
enum ResampleForm : int { kResamplePlain = 0, kResampleDefault = 1, kResampleDensity = 2 };

}  // namespace vr

// The entry points of a march unit (vr_launch.h defines them): all the C ABI's unit sees of the march kernels.  One text for both
// arithmetic modes -- vr:: in vr_march.hip, vrf:: in vr_fused.hip; the host picks by the context's mode (vr_set_arithmetic).
//   launch_march         enqueues the kernel of L; false: there is none for this family of this shader, nothing was launched
//   launch_shadow_build  the light volume of a shadowed launch (P: its parameters, vol[1] = the grid, whose storage is `out`)
//   launch_slice         a slice view: reduction x filter x addressing x skipping, `tiles` workgroups of one wavefront
//   launch_resample      a resample: filter x addressing x form (vr_resample.h: kResamplePlain ..), `blocks` persistent workgroups
#define VR_MARCH_ENTRY_POINTS                                                                                                          \
    bool launch_march(const vr::LaunchDesc& L, hipStream_t s, const vr::MarchBatch& B);                                                \
    void launch_shadow_build(const vr::MarchParams& P, float* out, float sigma, bool skip, bool off32, hipStream_t s);                 \
    void launch_slice(const vr::SliceParams& S, int reduce, bool nearest, bool off32, bool skip, unsigned tiles, hipStream_t s);         \
    void launch_resample(const vr::ResampleParams& R, bool nearest, bool off32, int form, unsigned blocks, hipStream_t s);
namespace vr {
VR_MARCH_ENTRY_POINTS
}
namespace vrf {
VR_MARCH_ENTRY_POINTS
}
#undef VR_MARCH_ENTRY_POINTS
