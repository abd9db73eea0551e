// vr_launch.h -- picks the instantiation of the march kernels for one launch (variant x addressing x skipping x loop
// form x lanes per ray).  Included once per arithmetic mode: by vr_api.hip (namespace vr, separately rounded
// multiply-adds) and by vr_fused.hip (namespace vrf, fused multiply-adds); enqueue_render calls the one the context's
// arithmetic mode selects (vr_set_arithmetic).
#pragma once
// march_p2_kernel: the several-frames form also for a launch of ONE frame.  It reads a frame's parameters where it uses them, through
// a wave-uniform index, and keeps fewer of them in registers: no scratch reload in the pipelined loop, which the one-frame form of the
// >= 4 GiB kernel has at the register limit (C5 3.37 -> 2.94 ms, a rank's half of it 1.78 -> 1.57), and 1 % on C3 / C4 below 4 GiB.
// The template argument BATCH still names the launch -- one frame or several: two kernel names in a profile -- the code behind both
// is the same (vr_p2.h).

#include "../../include/vr.h"
#include "vr_kernels.h"
#include "vr_dp.h"
#include "vr_pw.h"
#include "vr_p2.h"
// Flavour 15 (vr_lt.h: the voxels of a packet's next steps in an LDS tile filled by LDS-DMA -- the north star's "volume in LDS tiles")
// is part of the shipped library: slower than the two-steps-ahead kernel everywhere measured, selectable with
// vr_set_kernel_flavour(15) and tested on every box, not a candidate of the measured choice.
#include "vr_lt.h"
// The ray prologue, the in-box tests and the kernel shell of the five one-lane families below
#include "vr_ray.h"
// Intensity projections (MIP / MinIP / AIP of volume slot 0; flavours 19 and 20)
#include "vr_proj.h"
// The shaded isosurface of volume slot 0 (flavours 21 and 22; it reads the projections' brick records) and its refined points
#include "vr_iso.h"
// Shadows of the lit shader through a light volume (flavours 23 and 24; the build and the shadowed march)
#include "vr_shadow.h"
// The surface-position output of the unlit / lit shader (flavours 25 and 26); the depth of a surface frame
#include "vr_surf.h"
// Per-pixel ray bounds of the unlit / lit shader (flavours 27 and 28; MarchParams::vol[1].data / vol[2].data = the depth buffers)
#include "vr_bound.h"
// Slice views of any volume slot (vr_slice_async): a kernel with a parameter struct of its own, outside launch_march
#include "vr_slice.h"

#include <type_traits>

namespace VR_KNS {

// the shaders with exact empty-space skipping (brick records), with a pipelined loop, with a two-steps-ahead kernel
template <int V> constexpr bool kCanSkip = V == V_BASIC || V == V_LIGHT || V == V_THREE_FILES || V == V_VOLUME_MASK || V == V_LIGHT_INSHADER;
template <int V> constexpr bool kCanPipe = V == V_BASIC || V == V_LIGHT;
template <int V> constexpr bool kCanP2 = kCanPipe<V> || V == V_VOLUME_MASK;

// f(std::bool_constant<b>{}...): run-time flags as template arguments.  f is instantiated for every combination; it skips the ones
// that have no kernel with `if constexpr`.
template <class F>
void with_flags(F&& f) { f(); }
template <class F, class... R>
void with_flags(F&& f, bool b, R... rest)
{
    if (b) with_flags([&](auto... c) { f(std::true_type{}, c...); }, rest...);
    else with_flags([&](auto... c) { f(std::false_type{}, c...); }, rest...);
}

// march_pw_kernel / march_p2_kernel: more than 48 KiB of dynamic LDS must be allowed per kernel first.  Keyed on the kernel itself: every
// instantiation of one kernel template has the same function type, and `raised` must be one per kernel (the attribute sticks to it).
template <auto K>
void launch_queued(const LaunchDesc& L, hipStream_t s, const MarchBatch& B)
{
    if (L.lds_bytes > 48u * 1024u) {
        static unsigned raised = 0;
        if (L.lds_bytes > raised) {
            (void)hipFuncSetAttribute(reinterpret_cast<const void*>(K), hipFuncAttributeMaxDynamicSharedMemorySize, (int)L.lds_bytes);
            raised = L.lds_bytes;
        }
    }
    hipLaunchKernelGGL(K, L.grid, L.block, L.lds_bytes, s, B, L.queue);
}

// march_kernel; launches that carry several frames (MarchBatch) exist for both loop forms: plain (0) and, skipping, runs (3)
template <int V>
void launch_plain(const LaunchDesc& L, hipStream_t s, const MarchBatch& B)
{
    with_flags([&](auto O, auto S, auto BT) {
        if constexpr (!S || kCanSkip<V>)
            hipLaunchKernelGGL((march_kernel<V, O, S, (S ? 3 : 0), BT>), L.grid, L.block, L.lds_bytes, s, B);
    }, L.off32, kCanSkip<V> && B.frame[0].brick_dist, B.n_frames > 1);
}

// march_dp_kernel, 4 or 2 lanes per ray (the pipelined form exists for the lit shader)
template <int V>
void launch_dp(const LaunchDesc& L, hipStream_t s, const MarchBatch& B)
{
    with_flags([&](auto O, auto S, auto K4, auto PIPE, auto BT) {
        if constexpr ((!S || kCanSkip<V>) && (!PIPE || V == V_LIGHT))
            hipLaunchKernelGGL((march_dp_kernel<V, O, S, (K4 ? 4 : 2), PIPE, BT>), L.grid, L.block, 0, s, B);
    }, L.off32, kCanSkip<V> && B.frame[0].brick_dist, L.lanes == 4, V == V_LIGHT && L.pipe, B.n_frames > 1);
}

// persistent wavefronts (vr_pw.h); the loop form is march_kernel's default (runs through inert bricks when skipping)
template <int V>
void launch_pw(const LaunchDesc& L, hipStream_t s, const MarchBatch& B)
{
    with_flags([&](auto O, auto S, auto T, auto PP) {
        if constexpr ((!S || kCanSkip<V>) && (!PP || kCanPipe<V>)) launch_queued<march_pw_kernel<V, O, S, T, PP>>(L, s, B);
    }, L.off32, kCanSkip<V> && B.frame[0].brick_dist, L.ltf, kCanPipe<V> && L.pipe);
}

// two steps ahead (vr_p2.h; the host: TF slot 0 and the axis tables fit LDS, the bricked copy is in use).  The composite's form is the
// skipping one (the host asks for it only with the brick records in place).
template <int V>
void launch_p2(const LaunchDesc& L, hipStream_t s, const MarchBatch& B)
{
    with_flags([&](auto S, auto WN, auto BT) {
        if constexpr (S || V != V_VOLUME_MASK) launch_queued<march_p2_kernel<V, S, WN, BT>>(L, s, B);
    }, V == V_VOLUME_MASK || (B.frame[0].brick_dist && L.skip), L.p2_win, B.n_frames > 1);
}

// The one-lane kernels of vr_proj.h, vr_iso.h, vr_shadow.h, vr_surf.h and vr_bound.h: skipping x addressing x frames per launch.
// kernel(S, O, BT) returns the instantiation; args follow the batch.
template <class K, class... A>
void launch_one_lane(const LaunchDesc& L, hipStream_t s, const MarchBatch& B, K kernel, A... args)
{
    with_flags([&](auto S, auto O, auto BT) { hipLaunchKernelGGL(kernel(S, O, BT), L.grid, L.block, 0, s, B, args...); }, L.skip, L.off32,
               B.n_frames > 1);
}

// the projections: one mode each
template <int M>
void launch_proj(const LaunchDesc& L, hipStream_t s, const MarchBatch& B)
{
    launch_one_lane(L, s, B, [](auto S, auto O, auto BT) { return march_proj_kernel<M, O, S, BT>; }, L.vrange);
}

// the light volume of a shadowed launch (P: its parameters, vol[1] = the grid, whose storage is `out`); skip: by LIGHT's distance field
void launch_shadow_build(const MarchParams& P, float* out, float sigma, bool skip, bool off32, hipStream_t s)
{
    const unsigned blocks = (((unsigned)P.vol[1].nx + 3u) >> 2) * (((unsigned)P.vol[1].ny + 3u) >> 2) * (((unsigned)P.vol[1].nz + 3u) >> 2);
    with_flags([&](auto S, auto O) { hipLaunchKernelGGL((shadow_build_kernel<O, S>), dim3(blocks), dim3(64), 0, s, P, out, sigma); }, skip,
               off32);
}

// a slice view (vr_slice.h): reduction x filter x addressing x skipping; one workgroup of one wavefront per 8x8 pixel tile
void launch_slice(const SliceParams& S, int reduce, bool nearest, bool off32, bool skip, unsigned tiles, hipStream_t s)
{
    auto launch = [&](auto r) {
        constexpr int R = decltype(r)::value;
        with_flags([&](auto N, auto O, auto K) { hipLaunchKernelGGL((slice_kernel<R, N, O, K>), dim3(tiles), dim3(64), 0, s, S); }, nearest, off32,
                   skip);
    };
    if (reduce == VR_SLICE_MAX) launch(std::integral_constant<int, kProjMax>{});
    else if (reduce == VR_SLICE_MIN) launch(std::integral_constant<int, kProjMin>{});
    else launch(std::integral_constant<int, kProjAvg>{});
}

void launch_march(const LaunchDesc& L, hipStream_t s, const MarchBatch& B)
{
    switch (L.family) {
    case LaunchDesc::kShadow: launch_one_lane(L, s, B, [](auto S, auto O, auto BT) { return march_shadow_kernel<O, S, BT>; }); return;
    case LaunchDesc::kSurf: launch_one_lane(L, s, B, [](auto S, auto O, auto BT) { return march_surf_kernel<O, S, BT>; }); return;
    case LaunchDesc::kBound:  // (launches of one frame: BT is not an argument)
        if (L.variant == VR_VARIANT_LIGHT) launch_one_lane(L, s, B, [](auto S, auto O, auto) { return march_bound_kernel<V_LIGHT, O, S>; });
        else launch_one_lane(L, s, B, [](auto S, auto O, auto) { return march_bound_kernel<V_BASIC, O, S>; });
        return;
    case LaunchDesc::kIso:  // (surface output: the refined points)
        if (L.surface) launch_one_lane(L, s, B, [](auto S, auto O, auto BT) { return iso_point_kernel<O, S, BT>; });
        else launch_one_lane(L, s, B, [](auto S, auto O, auto BT) { return march_iso_kernel<O, S, BT>; });
        return;
    case LaunchDesc::kProj:
        if (L.variant == VR_VARIANT_MIP) launch_proj<kProjMax>(L, s, B);
        else if (L.variant == VR_VARIANT_MINIP) launch_proj<kProjMin>(L, s, B);
        else launch_proj<kProjAvg>(L, s, B);
        return;
    case LaunchDesc::kLt:  // LDS tiles (vr_lt.h): lit shader
        with_flags([&](auto O, auto S) { hipLaunchKernelGGL((march_lt_kernel<O, S>), L.grid, L.block, 0, s, B); },
                   L.off32, B.frame[0].brick_dist != nullptr);
        return;
    default: break;  // the families that exist per shader variant
    }
    auto launch = [&](auto v) {
        constexpr int V = decltype(v)::value;
        switch (L.family) {
        case LaunchDesc::kDp:  // (no depth-parallel form of the illustrative and in-shader gradient shaders: enqueue_render never asks for one)
            if constexpr (V != V_ILLUSTRATIVE && V != V_LIGHT_INSHADER) launch_dp<V>(L, s, B);
            break;
        case LaunchDesc::kPw: launch_pw<V>(L, s, B); break;
        case LaunchDesc::kP2:
            if constexpr (kCanP2<V>) launch_p2<V>(L, s, B);
            break;
        default: launch_plain<V>(L, s, B); break;
        }
    };
    switch (L.variant) {
    case VR_VARIANT_BASIC: launch(std::integral_constant<int, V_BASIC>{}); break;
    case VR_VARIANT_LIGHT: launch(std::integral_constant<int, V_LIGHT>{}); break;
    case VR_VARIANT_VOLUME_MASK: launch(std::integral_constant<int, V_VOLUME_MASK>{}); break;
    case VR_VARIANT_THREE_FILES: launch(std::integral_constant<int, V_THREE_FILES>{}); break;
    case VR_VARIANT_MULTI_CTRT: launch(std::integral_constant<int, V_MULTI_CTRT>{}); break;
    case VR_VARIANT_ILLUSTRATIVE: launch(std::integral_constant<int, V_ILLUSTRATIVE>{}); break;
    case VR_VARIANT_LIGHT_INSHADER: launch(std::integral_constant<int, V_LIGHT_INSHADER>{}); break;
    default: launch(std::integral_constant<int, V_TF_CALIB>{}); break;
    }
}

}  // namespace VR_KNS
