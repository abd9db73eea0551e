// vr_choice.h -- which kernel form a march launch runs and in what shape, as functions of a few facts: what may run
// (eligibility), the prior and the candidates of the measured choice (choose_flavour), what a flavour's number means (kernel_form) and
// the launch shape (launch_shape).  Plain C++ with no HIP header and nothing of the context, like vr_tuner.h: vr_device.h includes it
// for the constants and the kernel families, vr_api_render.h fills a ChoiceFacts from the context (choice_facts), and
// tests/choice_driver compiles it for the CPU to pin every rule.
#pragma once
#include <cstddef>

#include "../../include/vr.h"
#include "vr_tuner.h"

namespace vr {

constexpr int kTile = 64;  // multi-GPU ownership granule (pixels)
// Empty-space bricks of 4 x 4 x 4 base cells (vr_device.h says why 4); -DVR_BRICK_SHIFT=3 rebuilds round 1's.
#ifndef VR_BRICK_SHIFT
#define VR_BRICK_SHIFT 2
#endif
constexpr int kBrickShift = VR_BRICK_SHIFT;
constexpr int kBrickCells = 1 << kBrickShift;
// Storage bricks of the bricked volume copy (DevVolume::bricked): 2^S voxels per axis, S = 2 (4 x 4 x 4 = 1 KiB of vec4 voxels)
// by default; -DVR_VOX_BRICK_SHIFT=1 / 3 rebuilds with 2^3- / 8^3-voxel bricks for A/B (tools/run_r3l.sh).
#ifndef VR_VOX_BRICK_SHIFT
#define VR_VOX_BRICK_SHIFT 2
#endif
constexpr unsigned kVbS = VR_VOX_BRICK_SHIFT;  // log2 of the brick edge
constexpr unsigned kVbM = (1u << kVbS) - 1u;   // mask of the in-brick coordinate
constexpr unsigned kVbN = 1u << (3u * kVbS);   // voxels per brick
constexpr int kOrderMaxBlocks = 192 * 1024;    // launches with more blocks keep the index order (C5, one wavefront per block: 130 560)

// the bricked copy of a volume (DevVolume::bricked): storage bricks per axis, and their slots (voxels)
struct BrickedGrid {
    unsigned nbx, nby, nbz;
    size_t slots;
};
inline BrickedGrid bricked_grid(int nx, int ny, int nz)
{
    const unsigned nbx = ((unsigned)nx + kVbM) >> kVbS, nby = ((unsigned)ny + kVbM) >> kVbS, nbz = ((unsigned)nz + kVbM) >> kVbS;
    return {nbx, nby, nbz, (size_t)nbx * nby * nbz * kVbN};
}

// empty-space bricks along an axis of n base cells
inline int skip_bricks(int n) { return (n + kBrickCells - 1) >> kBrickShift; }

// Can the skipping kernels index a grid of bnx x bny x bnz bricks?  brick_of (vr_kernels.h) and slice_record (vr_slice.h) compute
// mul24(mul24(bz, bny) + by, bnx) + bx with SIGNED 24-bit multiplies, whose operands are sign-extended from bit 23: bz and bny are
// bricks of a 16-bit axis, bz * bny + by < bny * bnz and bnx must stay below 2^23; brick_record addresses with the 32-bit byte
// offset bid << 3.  A launch on a grid that fails this runs its form without skipping.
inline bool bricks_indexable(int bnx, int bny, int bnz)
{
    return (long long)bny * bnz <= (1 << 23) && bnx < (1 << 23) && (long long)bnx * bny * bnz <= (1ll << 29);
}
inline bool volume_bricks_indexable(int nx, int ny, int nz) { return bricks_indexable(skip_bricks(nx), skip_bricks(ny), skip_bricks(nz)); }

// finite and of moderate size: products of a colour, a light term and a shading factor stay finite, so "x * 0 == 0"
// holds for everything a provably-zero opacity is multiplied with
inline bool all_finite(const float* v, int n)
{
    for (int i = 0; i < n; ++i)
        if (!(v[i] - v[i] == 0.0f) || !(v[i] <= 1.0e15f && v[i] >= -1.0e15f)) return false;
    return true;
}
// ... the light (position, ambient, diffuse) of every one of a launch's n frames
inline bool lights_finite(const vr_uniforms* frames, int n)
{
    for (int f = 0; f < n; ++f)
        if (!all_finite(frames[f].light_pos, 12)) return false;
    return true;
}

// ---- the facts ------------------------------------------------------------------------------------------------------------------------

// What the choice reads of a launch and of the context (choice_facts, vr_api_render.h, fills it).
struct ChoiceFacts {
    // the request
    int variant, rank, world, n_frames;
    bool packed;
    bool surface, bounded;  // RenderRequest::surface, ::bounded
    // per bound volume: its size; the bricked copy, its density plane and the brick records exist
    struct Volume {
        int nx, ny, nz;
        bool bricked, bdens, bricks;
    } vols[VR_MAX_VOLUMES];
    // per TF slot: the tables' resolutions and what skipping derives from them (TfSlot)
    struct Table {
        int res_o, res_c, zero_prefix;
        bool color_finite, opacity_finite;
    } tf[VR_MAX_TFS];
    int layout_mode;      // vr_set_volume_layout
    unsigned p2_window;   // VR_EXP_P2_WINDOW
    int n_cus;
    unsigned W, H;
    int frames_in_flight;     // vr_hint_frames_in_flight
    bool shadows;             // vr_set_shadows: on
    bool lights_finite;       // the light of every frame of the launch
    double active_fraction;   // SkipField::active_fraction: share of bricks that are not inert (read behind prepare_skip)
    int tuner_mode;           // Tuner::mode
    unsigned last_chain;      // longest ray chain + 1 of the most recent plain colour launch of this scene shape whose sort has reported (0: none)
    // what only the trial's key reads
    unsigned long long brick_epoch, tf_epoch;
    int arith;
};

inline int tiles_across(unsigned pixels) { return (int)((pixels + kTile - 1) / kTile); }

// the tiles of a W x H frame that rank `rank` of `world` owns
inline int tile_count(unsigned W, unsigned H, int rank, int world)
{
    int total = tiles_across(W) * tiles_across(H);
    if (rank >= total) return 0;
    return (total - rank + world - 1) / world;
}

// ---- the shaders ----------------------------------------------------------------------------------------------------------------------

// What the host knows about a shader, one row per vr_variant: THE table.  check_render_args and eligibility / choose_flavour below read
// it, and so do the launch helpers of vr_launch.h, whose `if constexpr` guards instantiate a kernel exactly where a row says its form
// exists -- a flavour that the choice may ask for and a kernel that is compiled are one statement.
struct ShaderTraits {
    enum Form : unsigned {
        kMarch = 1u << 0,    // march_kernel (1, 6): the shaders that are not one of the one-lane families' alone
        kSkip = 1u << 1,     // exact empty-space skipping by brick records (the SKIP instantiations of every form it has)
        kDp = 1u << 2,       // depth-parallel, march_dp_kernel (7, 8; 10, 11)
        kDpPipe = 1u << 3,   // ... with the next round's corner loads pipelined (10, 11).  A DECISION: 10 / 11 of a shader with kDp alone
                             // run march_dp_kernel<.., PIPE = false> and still report 10 / 11 (they are what the default picks for small
                             // launches of every such shader)
        kPw = 1u << 4,       // persistent wavefronts, march_pw_kernel (12, 13)
        kPwPipe = 1u << 5,   // ... with the next step's corner loads pipelined (13).  A DECISION likewise: 13 of a shader with kPw alone
                             // runs without the pipeline and still reports 13
        kP2 = 1u << 6,       // two steps ahead, march_p2_kernel, skipping (17)
        kP2Plain = 1u << 7,  // ... and without skipping (16); a shader with kP2 alone runs 16 as 17
        kLut = 1u << 8,      // march_kernel with volume 0's slot tables in LDS (18): the shaders that sample one volume
        kLt = 1u << 9,       // LDS tiles, march_lt_kernel (15)
    };
    int nvol, ntf;    // volumes / TF pairs the shader samples (vr.h slot tables)
    bool projection;  // an intensity projection: march_proj_kernel alone (19, 20)
    bool surface;     // takes surface output (vr_set_output, vr_pick)
    bool bounds;      // takes ray bounds (vr_set_ray_bounds): march_bound_kernel<V> exists (27, 28)
    int skip_vol;     // the volume whose density drives tf[0]'s opacity: its records drive skipping
    unsigned forms;
    constexpr bool has(unsigned f) const { return (forms & f) == f; }
};
constexpr ShaderTraits kShader[VR_VARIANT_COUNT] = {
    // nvol ntf  proj  surface bounds skip_vol  forms
    {1, 1, false, true, true, 0,  // BASIC
     ShaderTraits::kMarch | ShaderTraits::kSkip | ShaderTraits::kDp | ShaderTraits::kPw | ShaderTraits::kPwPipe | ShaderTraits::kP2 |
         ShaderTraits::kP2Plain | ShaderTraits::kLut},
    {1, 1, false, true, true, 0,  // LIGHT
     ShaderTraits::kMarch | ShaderTraits::kSkip | ShaderTraits::kDp | ShaderTraits::kDpPipe | ShaderTraits::kPw | ShaderTraits::kPwPipe |
         ShaderTraits::kP2 | ShaderTraits::kP2Plain | ShaderTraits::kLut | ShaderTraits::kLt},
    {3, 2, false, false, false, 2,  // VOLUME_MASK (the composite)
     ShaderTraits::kMarch | ShaderTraits::kSkip | ShaderTraits::kDp | ShaderTraits::kPw | ShaderTraits::kP2},
    {2, 2, false, false, false, 0, ShaderTraits::kMarch | ShaderTraits::kSkip | ShaderTraits::kDp | ShaderTraits::kPw},  // THREE_FILES (the mask, slot 2, is bound but never sampled)
    {2, 2, false, false, false, 0, ShaderTraits::kMarch | ShaderTraits::kDp | ShaderTraits::kPw},                         // MULTI_CTRT
    {2, 1, false, false, false, 0, ShaderTraits::kMarch | ShaderTraits::kDp | ShaderTraits::kPw},                         // TF_CALIB
    // (the illustrative shader's opacity reads the accumulated alpha: its steps cannot be sampled side by side)
    {2, 2, false, false, false, 0, ShaderTraits::kMarch | ShaderTraits::kPw},  // ILLUSTRATIVE
    // (seven density fetches per sample: the one-lane kernels only)
    {1, 1, false, false, false, 0, ShaderTraits::kMarch | ShaderTraits::kSkip | ShaderTraits::kPw | ShaderTraits::kLut},  // LIGHT_INSHADER
    {1, 1, true, false, false, 0, 0u},  // MIP
    {1, 1, true, false, false, 0, 0u},  // MINIP
    {1, 1, true, false, false, 0, 0u},  // AVERAGE
    {1, 1, false, true, false, 0, 0u},  // ISO: march_iso_kernel / iso_point_kernel alone (21, 22)
};
static_assert(VR_VARIANT_BASIC == 0 && VR_VARIANT_LIGHT == 1 && VR_VARIANT_VOLUME_MASK == 2 && VR_VARIANT_THREE_FILES == 3 &&
                  VR_VARIANT_MULTI_CTRT == 4 && VR_VARIANT_TF_CALIB == 5 && VR_VARIANT_ILLUSTRATIVE == 6 && VR_VARIANT_LIGHT_INSHADER == 7 &&
                  VR_VARIANT_MIP == 8 && VR_VARIANT_MINIP == 9 && VR_VARIANT_AVERAGE == 10 && VR_VARIANT_ISO == 11 && VR_VARIANT_COUNT == 12,
              "kShader's rows are in the order of vr_variant");

// What each flavour launches -- the one place a flavour's number is decoded.
struct KernelForm {
    // march_kernel, march_dp_kernel, march_pw_kernel (persistent wavefronts), march_p2_kernel (the same, corner loads two steps ahead),
    // march_lt_kernel (LDS tiles), and the one-lane marches on vr_ray.h's prologue and shell: march_proj_kernel (vr_proj.h: the intensity
    // projections), march_iso_kernel / iso_point_kernel (vr_iso.h: the isosurface), march_shadow_kernel (vr_shadow.h: the lit shader with
    // shadows), march_surf_kernel (vr_surf.h: the surface-position output of the unlit / lit shader), march_bound_kernel (vr_bound.h: the
    // unlit / lit shader between per-pixel ray bounds)
    enum Family { kPlain, kDp, kPw, kP2, kLt, kProj, kIso, kShadow, kSurf, kBound };
    Family family;
    int lanes;            // kDp: lanes per ray (vr_dp.h): 64 / 32 workgroups per tile
    bool pipe;            // kDp / kPw: the next round's / step's corner loads software-pipelined
    bool skip;            // the skipping flavour of a pair (17 of 16 / 17; 19, 21, 23, 25, 27 of the one-lane families): LaunchDesc::skip once
                          // its records are in place
    bool lut;             // kPlain: the slot tables of volume 0 in LDS
    unsigned pw_threads;  // kPw / kP2: threads per workgroup
    // what follows from the family
    bool range_records() const { return family == kProj || family == kIso; }  // skips by prepare_proj's records
    bool measured() const  // a candidate of the measured choice (the one-lane families never are)
    {
        return !(range_records() || family == kShadow || family == kSurf || family == kBound);
    }
};

// The flavours a caller can ask for (vr_set_kernel_flavour, VR_EXP_FLAVOUR): 0 .. 18 but the kernel forms that lost every A/B and were
// removed (HISTORY.md) -- vr_set_kernel_flavour rejects those, VR_EXP_FLAVOUR ignores them.  19 .. 28 are what the one-lane families
// report; nobody can ask for them.
inline bool flavour_in_range(int f) { return f >= 0 && f <= 18; }
inline bool removed_flavour(int f) { return f == 2 || f == 3 || f == 4 || f == 5 || f == 9 || f == 14; }

inline KernelForm kernel_form(int fl, int variant)
{
    // (march_p2_kernel: two corner buffers, 3 wavefronts per SIMD at most; with every ray sampling all the time two per SIMD are faster
    // -- the corner data in flight is many times the L1 either way: noisy air 2.13 -> 2.04 ms.  The unlit shader's two buffers are 4-byte
    // densities, 101 VGPRs: 4 wavefronts per SIMD -- C2 one frame at a time 0.121 -> 0.113 ms, thin table 0.255 -> 0.239, four frames per
    // launch 0.070 -> 0.061: tools/experiments/s2h.sh.  Launches in flight: the same shape.  Two workgroups of 6 wavefronts do not share
    // a CU -- the second one's wavefronts would have to go 1-1-2-2 over the SIMDs where the dispatcher deals 2-2-1-1: measured 0.75 ms
    // per C3 frame, what one such workgroup per CU takes -- and two of 4 run at 8 wavefronts per CU: 0.63 against 0.54; three of 4, the
    // same 12 wavefronts per CU, take 0.79 ms one frame at a time and 0.62 in flight against 0.55 / 0.51: profiles/r04_p2_launch_shapes.txt)
    using D = KernelForm;
    switch (fl) {
    case 7: return {D::kDp, 4, false, false, false, 0u};
    case 8: return {D::kDp, 2, false, false, false, 0u};
    case 10: return {D::kDp, 4, true, false, false, 0u};
    case 11: return {D::kDp, 2, true, false, false, 0u};
    case 12: return {D::kPw, 0, false, false, false, 1024u};
    case 13: return {D::kPw, 0, true, false, false, 1024u};
    case 15: return {D::kLt, 0, false, false, false, 0u};
    case 16: return {D::kP2, 0, false, false, false, 512u};
    case 17: return {D::kP2, 0, false, true, false, variant == VR_VARIANT_BASIC ? 1024u : 768u};
    case 18: return {D::kPlain, 0, false, false, true, 0u};
    case 19:
    case 20: return {D::kProj, 0, false, fl == 19, false, 0u};
    case 21:
    case 22: return {D::kIso, 0, false, fl == 21, false, 0u};
    case 23:
    case 24: return {D::kShadow, 0, false, fl == 23, false, 0u};
    case 25:
    case 26: return {D::kSurf, 0, false, fl == 25, false, 0u};
    case 27:
    case 28: return {D::kBound, 0, false, fl == 27, false, 0u};
    default: return {D::kPlain, 0, false, false, false, 0u};  // 1, 6
    }
}

// Is there a kernel for `form` of shader `variant` (surface: a surface launch)?  After the two decisions above: the pipelining of a
// depth-parallel or persistent form is dropped where the shader has none.  launch_march (vr_launch.h) launches nothing and says so for
// a form that fails this; tests/test_choice.py shows that the choice never asks for one.
inline bool form_exists(const KernelForm& form, int variant, bool surface)
{
    const ShaderTraits& T = kShader[variant];
    using S = ShaderTraits;
    switch (form.family) {
    case KernelForm::kPlain: return T.has(S::kMarch) && (!form.lut || T.has(S::kLut));
    case KernelForm::kDp: return T.has(S::kDp);
    case KernelForm::kPw: return T.has(S::kPw);
    case KernelForm::kP2: return T.has(form.skip ? S::kP2 : S::kP2Plain);
    case KernelForm::kLt: return T.has(S::kLt);
    case KernelForm::kProj: return T.projection;
    case KernelForm::kIso: return variant == VR_VARIANT_ISO;
    case KernelForm::kShadow: return variant == VR_VARIANT_LIGHT;
    case KernelForm::kSurf: return surface && T.surface && variant != VR_VARIANT_ISO;
    case KernelForm::kBound: return T.bounds;
    }
    return false;
}

// rays per hardware lane (n_cus x 4 x 5 x 64) of `frames` launches of this rank's share of the frame: how full they keep the machine
inline double rays_per_lane(const ChoiceFacts& F, int rank, int world, int frames)
{
    const long long px = (long long)tile_count(F.W, F.H, rank, world) * kTile * kTile;
    return (double)px * frames / ((double)F.n_cus * 4.0 * 5.0 * 64.0);
}

// TF slot 0 fits a workgroup's LDS beside nothing else: one resolution for both tables, R <= 8190 (128 KiB)
inline bool tf0_fits_lds(const ChoiceFacts& F) { return F.tf[0].res_o == F.tf[0].res_c && F.tf[0].res_o + 2 <= 8192; }

// What a launch could run, worked out once before the kernel choice (choose_flavour).
struct Eligibility {
    bool p2_ok;             // two steps ahead (16, 17) can run
    unsigned p2_lds;        // ... with this much dynamic LDS (TF slot 0 and the three axis tables)
    bool lut_ok;            // 18 can run
    unsigned lut_lds;       // ... with this much (the slot tables of volume 0)
    bool indexable;         // the skipping kernels can index volume 0's bricks (bricks_indexable): every skipping form needs it
    bool can_skip;          // exact empty-space skipping (prepare_skip)
    bool whole_frame;       // enough rays to fill the machine in one frame
    bool empty;             // the share holds no tile: nothing is launched
    unsigned chain_known;   // longest ray chain + 1 of the most recent launch of this scene shape whose sort has reported (0: none)
};

inline Eligibility eligibility(const ChoiceFacts& F, int requested)
{
    Eligibility E = {};
    // two steps ahead (16, 17; march_p2_kernel, vr_p2.h): lit / unlit shader and the three-volume composite (with its brick records:
    // choose_flavour); TF slot 0 (one resolution for both tables) and the three axis tables in LDS; the bricked copy with 32-bit slots,
    // rows and slabs of bricks below 2^24 slots; a volume of 4 GiB or more through a moving window of at least four z-slabs of bricks.
    // Launches of several frames and launches in flight included.
    const ShaderTraits& T = kShader[F.variant];
    const int sv = T.skip_vol;  // the volume whose density drives tf[0]'s opacity
    E.p2_ok = T.has(ShaderTraits::kP2) && tf0_fits_lds(F) && F.layout_mode == 0 && F.vols[sv].bricked && F.vols[sv].bdens;
    if (E.p2_ok) {
        const ChoiceFacts::Volume& v = F.vols[sv];
        const BrickedGrid g = bricked_grid(v.nx, v.ny, v.nz);
        const size_t slab = (size_t)g.nbx * g.nby * kVbN, window = F.variant == VR_VARIANT_BASIC ? 0x3fffffffull : 0x0fffffffull;
        const size_t lds = (size_t)(F.tf[0].res_o + 2) * 16 + ((size_t)v.nx + v.ny + v.nz + 3) * 8;
        E.p2_ok = g.slots <= 0xFFFFFFFFull && slab < (1u << 24) && (F.p2_window ? F.p2_window / slab >= 3 : window / slab >= 4) && lds <= 160u * 1024u;
        E.p2_lds = (unsigned)lds;
    }
    // 18: march_kernel with the slot tables of volume 0 in its workgroup's LDS (make_cell_lut): the shaders that sample ONE volume, the
    // bricked copy with 32-bit slots
    E.lut_ok = T.has(ShaderTraits::kLut) && F.layout_mode == 0 && F.vols[0].bricked && F.vols[0].bdens;
    if (E.lut_ok) {
        E.lut_lds = (unsigned)(((size_t)F.vols[0].nx + F.vols[0].ny + F.vols[0].nz + 6) * 4);
        E.lut_ok = bricked_grid(F.vols[0].nx, F.vols[0].ny, F.vols[0].nz).slots <= 0xFFFFFFFFull && E.lut_lds <= 32u * 1024u;
    }
    // exact empty-space skipping: only for the shaders whose opacity is the CT table value alone, only when a zero-opacity sample is
    // provably the identity (finite colour table and light), and unless flavour 1 asks for the plain kernel (no rule of choose_flavour
    // turns another flavour into 1 or 1 into another)
    E.indexable = volume_bricks_indexable(F.vols[0].nx, F.vols[0].ny, F.vols[0].nz);
    E.can_skip = T.has(ShaderTraits::kSkip) && requested != 1 && F.vols[sv].bricks && F.tf[0].zero_prefix >= 0 && F.tf[0].color_finite &&
                 F.lights_finite;
    // the kernels index bricks with 24-bit multiplies and 32-bit byte offsets
    E.can_skip = E.can_skip && volume_bricks_indexable(F.vols[sv].nx, F.vols[sv].ny, F.vols[sv].nz);
    if (F.variant == VR_VARIANT_THREE_FILES) E.can_skip = E.can_skip && F.tf[1].color_finite && F.tf[1].opacity_finite;
    if (sv != 0)  // (the composite) mask and CT must share one grid so that one brick index serves both
        E.can_skip = E.can_skip && F.vols[0].bricks && F.vols[0].nx == F.vols[2].nx && F.vols[0].ny == F.vols[2].ny &&
                     F.vols[0].nz == F.vols[2].nz;
    E.whole_frame = rays_per_lane(F, F.rank, F.world, 1) >= 4.5;
    E.empty = tile_count(F.W, F.H, F.rank, F.world) == 0;
    E.chain_known = requested == 0 ? F.last_chain : 0;  // (the plain colour launch's key, always)
    if (F.surface && F.variant != VR_VARIANT_ISO) {
        // The surface march skips by the distance field of BASIC / LIGHT under the weakest condition that is still exact: an inert
        // brick's samples have opacity exactly 0, which leaves the accumulated alpha as it is whatever the colour table and the
        // light hold -- neither is read.  So: the brick records, a zero prefix of the opacity table, the kernels' index range.
        E.can_skip = requested != 1 && F.vols[0].bricks && F.tf[0].zero_prefix >= 0 && E.indexable;
        E.chain_known = 0;  // (a scene of its own: the colour launch's chains say nothing about it)
    }
    return E;
}

// What choose_flavour decides: the flavour the prior picks and, where the launch goes to the measured choice (tune), tune_pick's
// candidates and keys.
struct Choice {
    int prior;
    bool tune;
    int cand[6], n;
    unsigned long long shape, key;
};

// The kernel form ("flavour") a launch runs: `fl` is the one asked for (vr_set_kernel_flavour, else VR_EXP_FLAVOUR), 0 = the default.
inline Choice choose_flavour(const ChoiceFacts& F, int fl, const Eligibility& E)
{
    const ShaderTraits& T = kShader[F.variant];
    using S = ShaderTraits;
    Choice C = {};
    // The one-lane families come in pairs: 1 asks for the form without skipping (the odd flavour + 1), everything else runs as the
    // skipping one; nothing is measured.  The first row that applies decides (the isosurface's surface output keeps 21 / 22).
    const struct {
        bool applies;
        int skipping;
    } pairs[] = {
        {F.bounded, 27},                                   // the unlit / lit shader between ray bounds
        {F.surface && F.variant != VR_VARIANT_ISO, 25},    // the surface-position output of the unlit / lit shader
        {T.projection, 19},                                // the projections
        {F.variant == VR_VARIANT_ISO, 21},                 // the isosurface
        {F.variant == VR_VARIANT_LIGHT && F.shadows, 23},  // the shadowed lit shader
    };
    for (const auto& pr : pairs)
        if (pr.applies) return C.prior = fl == 1 ? pr.skipping + 1 : pr.skipping, C;
    const bool auto_choice = fl == 0;
    const double rays = rays_per_lane(F, F.rank, F.world, F.frames_in_flight * F.n_frames);
    const bool short_chains = E.chain_known != 0 && E.chain_known - 1 < 128;
    if (auto_choice) {
        // Default: pick the lanes per ray from what will be on the machine.  With many rays per hardware lane the machine is
        // throughput-bound and one lane per ray does the least work; with few (a small frame, or one GPU's share of the
        // tiles) the frame waits for its longest rays, whose chains of dependent samples the depth-parallel kernel cuts to a
        // half or a quarter (vr_dp.h).  Two things refine the round-1 rule (thresholds measured on C3 at 1 / 2 / 4 / 8 ranks):
        //  * frames in flight: when the caller keeps several frames in flight on different streams (it says so with
        //    vr_hint_frames_in_flight; asking the events instead flushes the runtime's command batches and costs more than it
        //    tells) the other launches fill the machine as well, so the rays per lane count once per frame in flight (a
        //    rank's half of C3, two frames pipelined: 0.34 ms with one lane, 0.42 with two);
        //  * how long the chains really are (E.chain_known).  Chains too short to matter -- under 128 samples, 0.2 ms (C2: 102) --
        //    leave nothing for the depth-parallel kernels to cut (C2: 0.133 / 0.091 ms per frame with one lane, 0.153 / 0.123 with
        //    two), unless the launch is too small to fill the machine at all.
        // (two lanes per ray from 2 rays per lane on, four below: re-measured on the bricked layout -- a rank's quarter of C3
        // (1.6 rays per lane), one frame at a time: 0.274 ms with two lanes, 0.203 with four; a rank's half (3.2): 0.362 / 0.377;
        // a quarter with two launches in flight counts 3.2 and keeps two lanes: 0.190 / 0.217 per frame)
        fl = (rays >= 4.5 || (short_chains && rays >= 1.2)) ? 6 : (rays >= 2.0 ? 11 : 10);
    }
    // what a form runs as where it cannot run: persistent wavefronts (12, 13; vr_pw.h) exist for launches of one frame
    if ((fl == 12 || fl == 13) && F.n_frames != 1) fl = 6;
    if ((fl == 16 || fl == 17) && !E.p2_ok) fl = F.n_frames != 1 ? 6 : (fl == 16 ? 13 : 12);
    if (fl == 18 && !E.lut_ok) fl = 6;
    // (p2_ok from here on: the shader has the form.)  The composite's form is the skipping one (its mask records): 16 runs as 17
    if (fl == 16 && !T.has(S::kP2Plain)) fl = 17;
    // LDS tiles (15; vr_lt.h): launches of one frame
    if (fl == 15 && (F.n_frames != 1 || !T.has(S::kLt))) fl = 6;
    // the depth-parallel flavours (7, 8, 10, 11) of a shader without the form
    if (kernel_form(fl, F.variant).family == KernelForm::kDp && !T.has(S::kDp)) fl = 6;
    // (the in-shader gradient variant reports 6 for every number that names none of its forms as well: kept as it was)
    if (F.variant == VR_VARIANT_LIGHT_INSHADER && fl != 1 && fl != 12 && fl != 13 && fl != 18) fl = 6;
    // a shader with the skipping two-steps-ahead form alone (the composite) has none without its brick records: no on-demand mask fetch
    if ((fl == 16 || fl == 17) && !T.has(S::kP2Plain) && !E.can_skip) fl = F.n_frames != 1 ? 6 : 12;
    if (!auto_choice) return C.prior = fl, C;

    // Default choice, second part -- THE PRIOR: what runs before anything has been measured.  Whole frames of the lit / unlit shader
    // and of the composite, one launch at a time: the kernel with the corner loads two steps ahead (vr_p2.h) -- 17, or 16 where next to
    // nothing can be skipped (noisy air under the default ramp 2.95 -> 1.97 ms; C3 0.65 -> 0.51; C4 0.72 -> 0.57) -- unless an earlier
    // launch of this shape says its chains are short (C2, longest chain 102: a packet is too short for the pipeline's fill and a
    // dequeue, 0.111 -> 0.161).  The same with launches in flight and several frames per launch since the approach loop (C3 0.417 / 0.382
    // ms per frame against march_kernel's 0.464 / 0.445; C5 level); shares of a frame: the first part's choice.
    const bool p2_variant = T.has(S::kP2) && (T.has(S::kP2Plain) || E.can_skip);
    const bool nothing_to_skip = !E.can_skip || F.active_fraction >= 0.9;  // (prepare_skip has measured the share of active bricks)
    if (fl == 6 && E.whole_frame && E.p2_ok && p2_variant) {
        if (nothing_to_skip && T.has(S::kP2Plain)) fl = 16;
        else if (!short_chains) fl = 17;
    }
    C.prior = fl;
    // (a share without a tile launches nothing and takes no launch number: a trial that counted it would name the next launch twice)
    if (!F.tuner_mode || E.empty) return C;
    // ... and THE MEASURED CHOICE (tune_pick): the eligible forms take turns on the caller's own frames, the fastest by the launches'
    // own records stays.  Candidates: the prior; the two-steps-ahead kernel; the one-lane kernel; the depth-parallel kernel (launches
    // that leave the machine part empty) or the persistent kernel without the pipeline (the longest chains).
    int* cand = C.cand;
    int& n = C.n;
    auto add = [&](int f) {
        for (int i = 0; i < n; ++i)
            if (cand[i] == f) return;
        if (n < 6) cand[n++] = f;
    };
    add(fl);
    if (E.p2_ok && p2_variant) add((nothing_to_skip && T.has(S::kP2Plain)) || !E.can_skip ? 16 : 17);
    add(6);
    if (E.lut_ok && E.lut_lds <= 8u * 1024u) add(18);  // (the one-lane kernel with its slot arithmetic from LDS tables; larger tables cost it wavefronts per CU: C5 4.2 vs 3.4 ms)
    if (!E.whole_frame && T.has(S::kDp)) add(rays >= 2.0 ? 11 : 10);
    else if (F.n_frames == 1 && T.has(S::kPwPipe)) add(12);  // (a candidate of the shaders that have the pipelined form too: lit / unlit)
    const unsigned long long shape = 0x9E3779B97F4A7C15ull * (((unsigned long long)F.variant << 56) ^ ((unsigned long long)F.world << 48) ^ ((unsigned long long)F.rank << 40) ^
                                                             ((unsigned long long)F.W << 24) ^ ((unsigned long long)F.H << 8) ^ (F.packed ? 0x80ull : 0ull) ^
                                                             ((unsigned long long)F.n_frames << 4) ^ (unsigned long long)F.frames_in_flight) | 1ull;
    const unsigned long long key = (shape ^ (F.brick_epoch * 0xD6E8FEB86659FD93ull) ^ (F.tf_epoch << 20) ^ ((unsigned long long)F.arith << 1) ^
                                    ((unsigned long long)F.layout_mode << 2)) | 1ull;
    C.tune = true;
    C.shape = shape;
    C.key = key;
    return C;
}

// The shape of a launch of `form`.
struct LaunchShape {
    int wpb;              // wavefronts per workgroup of the one-packet-per-wavefront and depth-parallel kernels
    unsigned blocks;      // the LOGICAL blocks of one frame (records, launch order)
    unsigned block;       // threads per workgroup
    unsigned grid;        // workgroups launched
    bool ordered;         // the launch takes a launch order and has a sort behind it
    bool pw;              // a persistent family (kPw / kP2): `grid` workgroups take the logical blocks from a queue
    bool ltf, p2_win;     // LaunchDesc::ltf, ::p2_win
    unsigned lds_bytes;   // dynamic LDS
};

// off32: every bound volume below 4 GiB; lut: volume 0's slot tables are in use (KernelForm::lut on the bricked copy)
inline LaunchShape launch_shape(const KernelForm& form, const ChoiceFacts& F, const Eligibility& E, bool off32, bool lut)
{
    LaunchShape S = {};
    const int n_tiles = tile_count(F.W, F.H, F.rank, F.world);
    // the LOGICAL blocks (records, launch order): one wavefront per workgroup (launch order at wavefront granularity) -- except
    // for the depth-parallel kernels on large launches, where 4x the workgroups cost more at dispatch than the finer order gains
    // (C2: 32 768 workgroups of a 0.12 ms frame).  See map_pixel / map_pixel_dp.
    const int dp = form.family == KernelForm::kDp ? form.lanes : 0, wpb = dp && n_tiles * dp * 64 > 16384 ? 4 : 1;
    const unsigned block = (unsigned)(64 * wpb);
    const unsigned grid = (unsigned)(dp ? n_tiles * dp * 64 / wpb : (n_tiles + 7) / 8 * 8 * (64 / wpb));
    S.wpb = wpb;
    S.blocks = grid;
    S.block = block;
    S.grid = grid * (unsigned)F.n_frames;
    S.ordered = grid <= (unsigned)kOrderMaxBlocks && grid % 8u == 0;
    S.pw = form.family == KernelForm::kPw || form.family == KernelForm::kP2;
    S.lds_bytes = lut ? E.lut_lds : 0u;
    if (S.pw) {
        // persistent wavefronts: `blocks` stays the number of LOGICAL blocks (records, launch order); the launch itself is one
        // workgroup of form.pw_threads per CU (fewer when there are fewer packets), TF slot 0 in LDS when it fits
        const bool p2 = form.family == KernelForm::kP2;
        const unsigned per_wg = form.pw_threads / 64u, wgs = (grid * (unsigned)F.n_frames + per_wg - 1u) / per_wg;
        S.ltf = tf0_fits_lds(F);
        S.p2_win = p2 && (!off32 || F.p2_window != 0);
        S.lds_bytes = p2 ? E.p2_lds : (S.ltf ? (unsigned)(F.tf[0].res_o + 2) * 16u : 0u);
        S.grid = wgs < (unsigned)F.n_cus ? wgs : (unsigned)F.n_cus;
        S.block = form.pw_threads;
    }
    return S;
}

}  // namespace vr
