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

namespace VR_KNS {

template <int V>
void launch_variant(bool off32, dim3 grid, dim3 block, hipStream_t s, const MarchBatch& B, unsigned lds_bytes = 0)
{
    constexpr bool kCanSkip = (V == V_BASIC || V == V_LIGHT || V == V_THREE_FILES || V == V_VOLUME_MASK || V == V_LIGHT_INSHADER);
    // launches that carry several frames (MarchBatch) exist for both loop forms: plain (0) and, skipping, runs (3)
#define VR_LAUNCH(O, S, L)                                                                                             \
    do {                                                                                                               \
        if (B.n_frames > 1) hipLaunchKernelGGL((march_kernel<V, O, S, L, true>), grid, block, lds_bytes, s, B);        \
        else hipLaunchKernelGGL((march_kernel<V, O, S, L, false>), grid, block, lds_bytes, s, B);                      \
    } while (0)
    if constexpr (kCanSkip) {
        if (B.frame[0].brick_dist) {
            if (off32) VR_LAUNCH(true, true, 3);
            else VR_LAUNCH(false, true, 3);
            return;
        }
    }
    if (off32) VR_LAUNCH(true, false, 0);
    else VR_LAUNCH(false, false, 0);
#undef VR_LAUNCH
}

template <int V, int K, bool PIPE>
void launch_dp(bool off32, dim3 grid, dim3 block, hipStream_t s, const MarchBatch& B)
{
    constexpr bool kCanSkip = (V == V_BASIC || V == V_LIGHT || V == V_THREE_FILES || V == V_VOLUME_MASK);
#define VR_LAUNCH_DP(O, S)                                                                                             \
    do {                                                                                                               \
        if (B.n_frames > 1) hipLaunchKernelGGL((march_dp_kernel<V, O, S, K, PIPE, true>), grid, block, 0, s, B);       \
        else hipLaunchKernelGGL((march_dp_kernel<V, O, S, K, PIPE, false>), grid, block, 0, s, B);                     \
    } while (0)
    if constexpr (kCanSkip) {
        if (B.frame[0].brick_dist) {
            if (off32) VR_LAUNCH_DP(true, true);
            else VR_LAUNCH_DP(false, true);
            return;
        }
    }
    if (off32) VR_LAUNCH_DP(true, false);
    else VR_LAUNCH_DP(false, false);
#undef VR_LAUNCH_DP
}

// persistent wavefronts (vr_pw.h); the loop form is march_kernel's default (runs through inert bricks when skipping)
template <int V>
void launch_pw(const LaunchDesc& L, hipStream_t s, const MarchBatch& B)
{
    constexpr bool kCanSkip = (V == V_BASIC || V == V_LIGHT || V == V_THREE_FILES || V == V_VOLUME_MASK || V == V_LIGHT_INSHADER);
    const bool skip = kCanSkip && B.frame[0].brick_dist != nullptr;
#define VR_LAUNCH_PW(O, S, T, PP)                                                                                      \
    do {                                                                                                               \
        auto k = march_pw_kernel<V, O, S, T, PP>;                                                                      \
        if (L.lds_bytes > 48u * 1024u) {                                                                               \
            static unsigned raised = 0;  /* per instantiation: the attribute sticks to the function */                 \
            if (L.lds_bytes > raised) {                                                                                \
                (void)hipFuncSetAttribute(reinterpret_cast<const void*>(k), hipFuncAttributeMaxDynamicSharedMemorySize,\
                                          (int)L.lds_bytes);                                                           \
                raised = L.lds_bytes;                                                                                  \
            }                                                                                                          \
        }                                                                                                              \
        hipLaunchKernelGGL(k, L.grid, L.block, L.lds_bytes, s, B, L.queue);                                            \
    } while (0)
#define VR_LAUNCH_PW_T(O, S)                                                                                           \
    do {                                                                                                               \
        if constexpr (kCanPipe) {                                                                                      \
            if (L.pw_pipe) {                                                                                           \
                if (L.pw_ltf) VR_LAUNCH_PW(O, S, true, true);                                                          \
                else VR_LAUNCH_PW(O, S, false, true);                                                                  \
                break;                                                                                                 \
            }                                                                                                          \
        }                                                                                                              \
        if (L.pw_ltf) VR_LAUNCH_PW(O, S, true, false);                                                                 \
        else VR_LAUNCH_PW(O, S, false, false);                                                                         \
    } while (0)
    constexpr bool kCanPipe = (V == V_BASIC || V == V_LIGHT);
    constexpr bool kCanP2 = kCanPipe || V == V_VOLUME_MASK;
    if constexpr (kCanP2) {
        if (L.pw_p2) {  // two steps ahead (vr_p2.h; the host: TF slot 0 and the axis tables fit LDS, the bricked copy is in use)
#define VR_LAUNCH_P2(S, WN, BT)                                                                                        \
    do {                                                                                                               \
        auto k = march_p2_kernel<V, S, WN, BT>;                                                                        \
        if (L.lds_bytes > 48u * 1024u) {                                                                               \
            static unsigned raised = 0;                                                                                \
            if (L.lds_bytes > raised) {                                                                                \
                (void)hipFuncSetAttribute(reinterpret_cast<const void*>(k), hipFuncAttributeMaxDynamicSharedMemorySize,\
                                          (int)L.lds_bytes);                                                           \
                raised = L.lds_bytes;                                                                                  \
            }                                                                                                          \
        }                                                                                                              \
        hipLaunchKernelGGL(k, L.grid, L.block, L.lds_bytes, s, B, L.queue);                                            \
    } while (0)
#define VR_LAUNCH_P2_W(S)                                                                                              \
    do {                                                                                                               \
        if (L.pw_p2_win) {                                                                                             \
            if (B.n_frames > 1) VR_LAUNCH_P2(S, true, true);                                                           \
            else VR_LAUNCH_P2(S, true, false);                                                                         \
        } else {                                                                                                       \
            if (B.n_frames > 1) VR_LAUNCH_P2(S, false, true);                                                          \
            else VR_LAUNCH_P2(S, false, false);                                                                        \
        }                                                                                                              \
    } while (0)
            if constexpr (V == V_VOLUME_MASK) {
                VR_LAUNCH_P2_W(true);  // (the host asks for it only with the brick records in place)
            } else {
                if (skip && L.pw_p2_skip) VR_LAUNCH_P2_W(true);
                else VR_LAUNCH_P2_W(false);
            }
#undef VR_LAUNCH_P2_W
#undef VR_LAUNCH_P2
            return;
        }
    }
    if constexpr (kCanSkip) {
        if (skip) {
            if (L.off32) VR_LAUNCH_PW_T(true, true);
            else VR_LAUNCH_PW_T(false, true);
            return;
        }
    }
    if (L.off32) VR_LAUNCH_PW_T(true, false);
    else VR_LAUNCH_PW_T(false, false);
#undef VR_LAUNCH_PW_T
#undef VR_LAUNCH_PW
}

void launch_march(const LaunchDesc& L, hipStream_t s, const MarchBatch& B)
{
    const int variant = L.variant;
    if (L.lt) {  // LDS tiles (vr_lt.h): lit shader
        const bool skip = B.frame[0].brick_dist != nullptr;
        if (L.off32) {
            if (skip) hipLaunchKernelGGL((march_lt_kernel<true, true>), L.grid, L.block, 0, s, B);
            else hipLaunchKernelGGL((march_lt_kernel<true, false>), L.grid, L.block, 0, s, B);
        } else {
            if (skip) hipLaunchKernelGGL((march_lt_kernel<false, true>), L.grid, L.block, 0, s, B);
            else hipLaunchKernelGGL((march_lt_kernel<false, false>), L.grid, L.block, 0, s, B);
        }
        return;
    }
    if (L.pw) {
        switch (variant) {
        case VR_VARIANT_BASIC: launch_pw<V_BASIC>(L, s, B); break;
        case VR_VARIANT_LIGHT: launch_pw<V_LIGHT>(L, s, B); break;
        case VR_VARIANT_VOLUME_MASK: launch_pw<V_VOLUME_MASK>(L, s, B); break;
        case VR_VARIANT_THREE_FILES: launch_pw<V_THREE_FILES>(L, s, B); break;
        case VR_VARIANT_MULTI_CTRT: launch_pw<V_MULTI_CTRT>(L, s, B); break;
        case VR_VARIANT_ILLUSTRATIVE: launch_pw<V_ILLUSTRATIVE>(L, s, B); break;
        case VR_VARIANT_LIGHT_INSHADER: launch_pw<V_LIGHT_INSHADER>(L, s, B); break;
        default: launch_pw<V_TF_CALIB>(L, s, B); break;
        }
        return;
    }
    const bool off32 = L.off32, dp_pipe = L.dp_pipe;
    const int dp = L.dp;
    const dim3 grid = L.grid, block = L.block;
    if (dp == 4) {
        switch (variant) {
        case VR_VARIANT_BASIC: launch_dp<V_BASIC, 4, false>(off32, grid, block, s, B); break;
        case VR_VARIANT_LIGHT:
            if (dp_pipe) launch_dp<V_LIGHT, 4, true>(off32, grid, block, s, B);
            else launch_dp<V_LIGHT, 4, false>(off32, grid, block, s, B);
            break;
        case VR_VARIANT_VOLUME_MASK: launch_dp<V_VOLUME_MASK, 4, false>(off32, grid, block, s, B); break;
        case VR_VARIANT_THREE_FILES: launch_dp<V_THREE_FILES, 4, false>(off32, grid, block, s, B); break;
        case VR_VARIANT_MULTI_CTRT: launch_dp<V_MULTI_CTRT, 4, false>(off32, grid, block, s, B); break;
        case VR_VARIANT_TF_CALIB: launch_dp<V_TF_CALIB, 4, false>(off32, grid, block, s, B); break;
        default: break;  // (no depth-parallel form of this shader: enqueue_render never asks for one)
        }
    } else if (dp == 2) {
        switch (variant) {
        case VR_VARIANT_BASIC: launch_dp<V_BASIC, 2, false>(off32, grid, block, s, B); break;
        case VR_VARIANT_LIGHT:
            if (dp_pipe) launch_dp<V_LIGHT, 2, true>(off32, grid, block, s, B);
            else launch_dp<V_LIGHT, 2, false>(off32, grid, block, s, B);
            break;
        case VR_VARIANT_VOLUME_MASK: launch_dp<V_VOLUME_MASK, 2, false>(off32, grid, block, s, B); break;
        case VR_VARIANT_THREE_FILES: launch_dp<V_THREE_FILES, 2, false>(off32, grid, block, s, B); break;
        case VR_VARIANT_MULTI_CTRT: launch_dp<V_MULTI_CTRT, 2, false>(off32, grid, block, s, B); break;
        case VR_VARIANT_TF_CALIB: launch_dp<V_TF_CALIB, 2, false>(off32, grid, block, s, B); break;
        default: break;  // (no depth-parallel form of this shader: enqueue_render never asks for one)
        }
    } else {
        switch (variant) {
        case VR_VARIANT_BASIC: launch_variant<V_BASIC>(off32, grid, block, s, B, L.lds_bytes); break;
        case VR_VARIANT_LIGHT: launch_variant<V_LIGHT>(off32, grid, block, s, B, L.lds_bytes); break;
        case VR_VARIANT_VOLUME_MASK: launch_variant<V_VOLUME_MASK>(off32, grid, block, s, B); break;
        case VR_VARIANT_THREE_FILES: launch_variant<V_THREE_FILES>(off32, grid, block, s, B); break;
        case VR_VARIANT_MULTI_CTRT: launch_variant<V_MULTI_CTRT>(off32, grid, block, s, B); break;
        case VR_VARIANT_ILLUSTRATIVE: launch_variant<V_ILLUSTRATIVE>(off32, grid, block, s, B); break;
        case VR_VARIANT_LIGHT_INSHADER: launch_variant<V_LIGHT_INSHADER>(off32, grid, block, s, B, L.lds_bytes); break;
        default: launch_variant<V_TF_CALIB>(off32, grid, block, s, B); break;
        }
    }
}

}  // namespace VR_KNS
