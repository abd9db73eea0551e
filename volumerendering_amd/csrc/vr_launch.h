// vr_launch.h -- picks the instantiation of the march kernels for one launch (variant x addressing x skipping x loop
// form x lanes per ray).  Included once per arithmetic mode: by vr_march.hip (namespace vr, separately rounded
// multiply-adds) and by vr_fused.hip (namespace vrf, fused multiply-adds), each a translation unit that holds nothing else.  The C
// ABI's unit (vr_api.hip) sees the four entry points that vr_device.h declares -- launch_march, launch_shadow_build, launch_slice,
// launch_resample -- and calls the ones of the context's arithmetic mode (vr_set_arithmetic).
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
// A volume slot resampled onto another grid (vr_volume_resample): a kernel with a parameter struct of its own as well
#include "vr_resample.h"

#include <type_traits>
#include <utility>

namespace VR_KNS {

// which forms shader V has: kShader (vr_choice.h), the table the host's kernel choice reads -- there is no second list here
template <int V> constexpr bool has(unsigned forms) { return kShader[V].has(forms); }
template <int V> constexpr bool kCanSkip = has<V>(ShaderTraits::kSkip);

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

// The launch helpers return whether a kernel was enqueued: false for a combination that kShader says does not exist.

// march_kernel; launches that carry several frames (MarchBatch) exist for both loop forms: plain (0) and, skipping, runs (3)
template <int V>
bool launch_plain(const LaunchDesc& L, hipStream_t s, const MarchBatch& B)
{
    bool launched = false;
    with_flags([&](auto O, auto S, auto BT) {
        if constexpr (has<V>(ShaderTraits::kMarch) && (!S || kCanSkip<V>)) {
            hipLaunchKernelGGL((march_kernel<V, O, S, (S ? 3 : 0), BT>), L.grid, L.block, L.lds_bytes, s, B);
            launched = true;
        }
    }, L.off32, kCanSkip<V> && B.frame[0].brick_dist, B.n_frames > 1);
    return launched;
}

// march_dp_kernel, 4 or 2 lanes per ray; without the pipelined form (ShaderTraits::kDpPipe) L.pipe is dropped
template <int V>
bool launch_dp(const LaunchDesc& L, hipStream_t s, const MarchBatch& B)
{
    bool launched = false;
    with_flags([&](auto O, auto S, auto K4, auto PIPE, auto BT) {
        if constexpr (has<V>(ShaderTraits::kDp) && (!S || kCanSkip<V>) && (!PIPE || has<V>(ShaderTraits::kDpPipe))) {
            hipLaunchKernelGGL((march_dp_kernel<V, O, S, (K4 ? 4 : 2), PIPE, BT>), L.grid, L.block, 0, s, B);
            launched = true;
        }
    }, L.off32, kCanSkip<V> && B.frame[0].brick_dist, L.lanes == 4, has<V>(ShaderTraits::kDpPipe) && L.pipe, B.n_frames > 1);
    return launched;
}

// persistent wavefronts (vr_pw.h); the loop form is march_kernel's default (runs through inert bricks when skipping); without the
// pipelined form (ShaderTraits::kPwPipe) L.pipe is dropped
template <int V>
bool launch_pw(const LaunchDesc& L, hipStream_t s, const MarchBatch& B)
{
    bool launched = false;
    with_flags([&](auto O, auto S, auto T, auto PP) {
        if constexpr (has<V>(ShaderTraits::kPw) && (!S || kCanSkip<V>) && (!PP || has<V>(ShaderTraits::kPwPipe))) {
            launch_queued<march_pw_kernel<V, O, S, T, PP>>(L, s, B);
            launched = true;
        }
    }, L.off32, kCanSkip<V> && B.frame[0].brick_dist, L.ltf, has<V>(ShaderTraits::kPwPipe) && L.pipe);
    return launched;
}

// two steps ahead (vr_p2.h; the host: TF slot 0 and the axis tables fit LDS, the bricked copy is in use).  A shader without the form
// that does not skip (ShaderTraits::kP2Plain: the composite) runs the skipping one: the host asks for it only with the brick records
// in place.
template <int V>
bool launch_p2(const LaunchDesc& L, hipStream_t s, const MarchBatch& B)
{
    bool launched = false;
    with_flags([&](auto S, auto WN, auto BT) {
        if constexpr (has<V>(S ? ShaderTraits::kP2 : ShaderTraits::kP2Plain)) {
            launch_queued<march_p2_kernel<V, S, WN, BT>>(L, s, B);
            launched = true;
        }
    }, !has<V>(ShaderTraits::kP2Plain) || (B.frame[0].brick_dist && L.skip), L.p2_win, B.n_frames > 1);
    return launched;
}

// LDS tiles (vr_lt.h): the lit shader's kernel
template <int V>
bool launch_lt(const LaunchDesc& L, hipStream_t s, const MarchBatch& B)
{
    if constexpr (has<V>(ShaderTraits::kLt)) {
        static_assert(V == V_LIGHT, "march_lt_kernel is the lit shader");
        with_flags([&](auto O, auto S) { hipLaunchKernelGGL((march_lt_kernel<O, S>), L.grid, L.block, 0, s, B); }, L.off32,
                   B.frame[0].brick_dist != nullptr);
        return true;
    }
    return false;
}

// The one-lane kernels of vr_proj.h, vr_iso.h, vr_shadow.h, vr_surf.h and vr_bound.h: skipping x addressing x frames per launch.
// kernel(S, O, BT) returns the instantiation; args follow the batch.
template <class K, class... A>
bool launch_one_lane(const LaunchDesc& L, hipStream_t s, const MarchBatch& B, K kernel, A... args)
{
    with_flags([&](auto S, auto O, auto BT) { hipLaunchKernelGGL(kernel(S, O, BT), L.grid, L.block, 0, s, B, args...); }, L.skip, L.off32,
               B.n_frames > 1);
    return true;
}

// the projections: one mode each
template <int M>
bool launch_proj(const LaunchDesc& L, hipStream_t s, const MarchBatch& B)
{
    return launch_one_lane(L, s, B, [](auto S, auto O, auto BT) { return march_proj_kernel<M, O, S, BT>; }, L.vrange);
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

// a resample (vr_resample.h): filter x addressing x form; `blocks` persistent workgroups of four wavefronts
void launch_resample(const ResampleParams& R, bool nearest, bool off32, int form, unsigned blocks, hipStream_t s)
{
    auto launch = [&](auto f) {
        constexpr int F = decltype(f)::value;
        with_flags([&](auto N, auto O) { hipLaunchKernelGGL((resample_kernel<N, O, F>), dim3(blocks), dim3(256), 0, s, R); }, nearest, off32);
    };
    if (form == kResamplePlain) launch(std::integral_constant<int, kResamplePlain>{});
    else if (form == kResampleDensity) launch(std::integral_constant<int, kResampleDensity>{});
    else launch(std::integral_constant<int, kResampleDefault>{});
}

// the families that exist per shader, for shader V
template <int V>
bool launch_variant(const LaunchDesc& L, hipStream_t s, const MarchBatch& B)
{
    switch (L.family) {
    case KernelForm::kDp: return launch_dp<V>(L, s, B);
    case KernelForm::kPw: return launch_pw<V>(L, s, B);
    case KernelForm::kP2: return launch_p2<V>(L, s, B);
    case KernelForm::kLt: return launch_lt<V>(L, s, B);
    case KernelForm::kBound:  // (launches of one frame: BT is not an argument)
        if constexpr (kShader[V].bounds)
            return launch_one_lane(L, s, B, [](auto S, auto O, auto) { return march_bound_kernel<V, O, S>; });
        return false;
    default: return launch_plain<V>(L, s, B);
    }
}
template <int... V>
bool launch_variant_of(std::integer_sequence<int, V...>, const LaunchDesc& L, hipStream_t s, const MarchBatch& B)
{
    bool launched = false;
    (void)((L.variant == V && ((launched = launch_variant<V>(L, s, B)), true)) || ...);
    return launched;
}

// Enqueues the kernel of L; false: there is none for this family of this shader, nothing was launched (enqueue_render fails the call).
bool launch_march(const LaunchDesc& L, hipStream_t s, const MarchBatch& B)
{
    switch (L.family) {
    case KernelForm::kShadow: return launch_one_lane(L, s, B, [](auto S, auto O, auto BT) { return march_shadow_kernel<O, S, BT>; });
    case KernelForm::kSurf: return launch_one_lane(L, s, B, [](auto S, auto O, auto BT) { return march_surf_kernel<O, S, BT>; });
    case KernelForm::kIso:  // (surface output: the refined points)
        if (L.surface) return launch_one_lane(L, s, B, [](auto S, auto O, auto BT) { return iso_point_kernel<O, S, BT>; });
        return launch_one_lane(L, s, B, [](auto S, auto O, auto BT) { return march_iso_kernel<O, S, BT>; });
    case KernelForm::kProj:
        if (L.variant == VR_VARIANT_MIP) return launch_proj<kProjMax>(L, s, B);
        if (L.variant == VR_VARIANT_MINIP) return launch_proj<kProjMin>(L, s, B);
        return launch_proj<kProjAvg>(L, s, B);
    default:  // the families that exist per shader variant: by the variant's value
        return launch_variant_of(std::make_integer_sequence<int, VR_VARIANT_COUNT>{}, L, s, B);
    }
}

// The four definitions above are the ones vr_device.h declares: with another signature a definition would be a second overload,
// and the name's address ambiguous.
static_assert(sizeof(&launch_march) + sizeof(&launch_shadow_build) + sizeof(&launch_slice) + sizeof(&launch_resample) > 0);

}  // namespace VR_KNS
