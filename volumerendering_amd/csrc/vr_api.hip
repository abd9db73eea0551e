// vr_api.hip -- implementation of the C ABI declared in include/vr.h on top of the gfx950 kernels: one translation unit, the host code
// by concern in vr_ctx.h and vr_api_*.h; here the context's life (create, resize, destroy), its settings and its streams.
// The march kernels are not in this unit: vr_march.hip and vr_fused.hip compile them, one per arithmetic mode, and the host code
// reaches them through launch_march, launch_shadow_build, launch_slice and launch_resample (vr_device.h).  What is compiled here, once, are the
// kernels that no arithmetic mode touches: the auxiliary kernels and the voxel tools.
// No CPU fallback exists behind this ABI (and nothing under oracle/ is referenced): without a usable HIP
// device vr_create fails with VR_ERR_HIP.
#include "../../include/vr.h"
#include "vr_device.h"
// Auxiliary kernels: a volume's preparation and brick records, the skip-field build, a frame around its launch
#include "vr_prep.h"
#include "vr_skipfield.h"
#include "vr_frame.h"
#include "vr_units.h"  // what the voxel tools below share
// Histograms (vr_histogram_async): nothing to fuse, so this kernel exists once, here
#include "vr_hist.h"
// Region growing (vr_segment_grow): integer work on bit-bricks, compiled once as well
#include "vr_grow.h"
// Mask morphology (vr_mask_morph): integer work on bit-rows (vr_bitrows.h: their box walk, pack and combine rule), compiled once as well
#include "vr_morph.h"
// Distance maps (vr_mask_distance): exact integer work on the same bit-rows, compiled once as well
#include "vr_dist.h"
// Polygon rasterisation (vr_mask_polygons): exact integer work on the same bit-rows, compiled once as well
#include "vr_raster.h"
// The prefix scan of the three tools below (tool_scan, vr_api_tools.h): integer work, compiled once as well
#include "vr_scan.h"
// Contour tracing (vr_mask_outlines): the inverse of the raster, exact integer work on the same bit-rows, compiled once as well
#include "vr_outline.h"
// Connected components (vr_mask_components): a union-find over the runs of the same bit-rows, compiled once as well
#include "vr_comp.h"
// Surface extraction (vr_volume_mesh): marching tetrahedra over bit-rows of the lattice; nothing to fuse, compiled once as well
#include "vr_mesh.h"
// Separable filters (vr_volume_filter): every tap an explicit fmaf whatever the arithmetic mode, compiled once as well
#include "vr_filter.h"
// Rank filters (vr_volume_rank): keys compared as unsigned integers, nothing computed and nothing to fuse, compiled once as well
#include "vr_rank.h"
// The gamma index (vr_volume_gamma): every fused step an explicit fmaf whatever the arithmetic mode, compiled once as well
#include "vr_gamma.h"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <string>
#include <type_traits>
#include <utility>
#include <vector>

using namespace vr;

#include "vr_ctx.h"
#include "vr_api_volume.h"
#include "vr_api_tools.h"
#include "vr_api_tf.h"
#include "vr_api_render.h"
#include "vr_api_views.h"
#include "vr_api_segment.h"
#include "vr_api_morph.h"
#include "vr_api_dist.h"
#include "vr_api_raster.h"
#include "vr_api_outline.h"
#include "vr_api_components.h"
#include "vr_api_resample.h"
#include "vr_api_mesh.h"
#include "vr_api_filter.h"
#include "vr_api_rank.h"
#include "vr_api_gamma.h"

namespace {

int alloc_frame(vr_ctx* c)
{
    VR_HIP(c, hipSetDevice(c->device));
    c->d_frame.release();
    c->d_present.release();
    c->d_pick.release();
    size_t n = (size_t)c->W * c->H;
    VR_HIP(c, c->d_frame.reserve(n));
    VR_HIP(c, c->d_present.reserve(n));
    VR_HIP(c, hipMemsetAsync(c->d_frame, 0, n * sizeof(float4), c->stream));
    return VR_OK;
}

}  // namespace

extern "C" {

int vr_abi_version(void) { return VR_ABI_VERSION; }

const char* vr_last_error(const vr_ctx* ctx) { return ctx ? ctx->err.c_str() : g_create_error.c_str(); }

int vr_create(vr_ctx** out, uint32_t width, uint32_t height, int device_id)
{
    if (!out) return fail(nullptr, VR_ERR_INVALID_ARG, "vr_create: out is NULL");
    *out = nullptr;
    if (width == 0 || height == 0 || width > 32768 || height > 32768)
        return fail(nullptr, VR_ERR_INVALID_ARG, "vr_create: bad viewport size");
    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev <= 0)
        return fail(nullptr, VR_ERR_HIP, std::string("vr_create: no HIP device available (") +
                                             (e != hipSuccess ? hipGetErrorString(e) : "device count 0") +
                                             "); this library has no CPU fallback");
    if (device_id < 0 || device_id >= ndev) return fail(nullptr, VR_ERR_INVALID_ARG, "vr_create: bad device_id");
    vr_ctx* c = new (std::nothrow) vr_ctx();
    if (!c) return fail(nullptr, VR_ERR_OOM, "vr_create: out of host memory");
    c->device = device_id;
    c->W = width;
    c->H = height;
    auto bail = [&](int code) {
        g_create_error = c->err;
        vr_destroy(c);
        return code;
    };
    auto hip_ok = [&](hipError_t he, const char* what) {
        if (he == hipSuccess) return true;
        c->err = std::string(what) + ": " + hipGetErrorString(he);
        return false;
    };
    if (!hip_ok(hipSetDevice(device_id), "hipSetDevice")) return bail(VR_ERR_HIP);
    if (!hip_ok(c->stream.create(), "hipStreamCreate")) return bail(VR_ERR_HIP);
    {
        int cus = 0;
        if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device_id) == hipSuccess && cus > 0) c->n_cus = cus;
    }
    // experiment knobs (A/B measurements; none changes any result)
    if (const char* e = getenv("VR_EXP_FLAVOUR")) {
        const int f = atoi(e);
        if (flavour_in_range(f) && !removed_flavour(f)) c->default_flavour = f;
    }
    if (const char* e = getenv("VR_EXP_P2_WINDOW")) {  // records per gather window of march_p2_kernel (tests: the moving window on small volumes)
        const long long w = atoll(e);
        if (w > 0 && w <= 0x3fffffffll) c->p2_window = (unsigned)w;
    }
    if (const char* e = getenv("VR_EXP_TUNE")) c->tuner.mode = atoi(e);
    if (!hip_ok(c->d_pw_heads.reserve((size_t)kInFlight * 8 * 64), "hipMalloc(queue heads)")) return bail(VR_ERR_HIP);
    if (!hip_ok(hipMemset(c->d_pw_heads, 0, (size_t)kInFlight * 8 * 64 * sizeof(unsigned)), "hipMemset(queue heads)")) return bail(VR_ERR_HIP);
    for (Event* e : {&c->tm.ev_begin, &c->tm.ev_k0, &c->tm.ev_k1, &c->tm.ev_end})
        if (!hip_ok(e->create(), "hipEventCreate")) return bail(VR_ERR_HIP);
    for (int i = 0; i < kRing; ++i)
        if (!hip_ok(c->ring.k0[i].create(), "hipEventCreate") || !hip_ok(c->ring.k1[i].create(), "hipEventCreate"))
            return bail(VR_ERR_HIP);
    for (auto& r : c->slot)
        if (!hip_ok(r.done.create(hipEventDisableTiming), "hipEventCreate")) return bail(VR_ERR_HIP);
    for (auto& o : c->order.ring)
        if (!hip_ok(o.sorted.create(hipEventDisableTiming), "hipEventCreate")) return bail(VR_ERR_HIP);
    // The sorts run on a stream of their own, default priority.  The runtime deals streams onto a handful of hardware queues
    // per priority level, and a sort waits (a barrier in its queue) for a launch that is still running, so WHICH streams end up
    // sharing a queue with this one matters: measured on this box, a high- or low-priority sort stream lets a third frame in
    // flight overlap (a rank's eighth of C3: 0.142 -> 0.110 ms per frame, kernels alone) but costs the multi-GPU loop 50 us per
    // frame (0.24 -> 0.29 ms one frame at a time; with a high-priority sort stream its gather stream, high priority too, meets
    // the sorts' barriers), and the full C3 frame gains nothing from a third frame in flight either way (tools/exp_tiles.py,
    // tools/exp_queues).
    if (!hip_ok(c->order.stream.create(), "hipStreamCreate")) return bail(VR_ERR_HIP);
    if (!hip_ok(c->edits.order.ev.create(hipEventDisableTiming), "hipEventCreate")) return bail(VR_ERR_HIP);
    for (auto& st : c->edits.stage)
        if (!hip_ok(st.done.create(hipEventDisableTiming), "hipEventCreate")) return bail(VR_ERR_HIP);
    if (!hip_ok(c->skip.h_sum.reserve(kGen, true), "hipHostMalloc")) return bail(VR_ERR_HIP);
    if (!hip_ok(c->skip.d_sum.reserve(kGen), "hipMalloc(skip summary)")) return bail(VR_ERR_HIP);
    if (!hip_ok(hipMemset(c->skip.d_sum, 0, kGen * sizeof(SkipSumDev)), "hipMemset(skip summary)")) return bail(VR_ERR_HIP);
    // (these three may fail: the buffer stays empty)
    (void)c->ring.h_span.reserve(kRing, true);         // (else every launch is timed with events)
    (void)c->ring.h_end.reserve(kRing, true);          // (else no measured kernel choice with launches in flight: the prior's pick stays)
    (void)c->order.h_chain.reserve(kOrderRing, true);  // (else the choice of lanes per ray goes by the launch size alone)
    if (!hip_ok(c->d_counters.reserve(3), "hipMalloc(counters)")) return bail(VR_ERR_HIP);
    if (!hip_ok(c->h_counters.reserve(3, true), "hipHostMalloc")) return bail(VR_ERR_HIP);
    if (const int rc = alloc_frame(c)) return bail(rc);
    *out = c;
    return VR_OK;
}

int vr_resize(vr_ctx* c, uint32_t width, uint32_t height)
{
    if (!c) return VR_ERR_INVALID_ARG;
    if (width == 0 || height == 0 || width > 32768 || height > 32768)
        return fail(c, VR_ERR_INVALID_ARG, "vr_resize: bad viewport size");
    (void)hipSetDevice(c->device);
    (void)hipDeviceSynchronize();  // frames may be in flight on the caller's streams
    drained(c);
    c->W = width;
    c->H = height;
    c->d_near = c->d_far = nullptr;  // (the caller's depth buffers no longer fit)
    return alloc_frame(c);
}

void vr_destroy(vr_ctx* c)
{
    if (!c) return;
    (void)hipSetDevice(c->device);
    (void)hipDeviceSynchronize();  // renders may be in flight on streams of the caller's
    drained(c);
    delete c;  // (every member that holds a HIP resource releases it)
}

int vr_set_uniforms(vr_ctx* c, const vr_uniforms* u)
{
    if (!c) return VR_ERR_INVALID_ARG;
    if (!u) return fail(c, VR_ERR_INVALID_ARG, "vr_set_uniforms: uniforms is NULL");
    if (!is_identity(u->model))
        return fail(c, VR_ERR_UNSUPPORTED,
                    "vr_set_uniforms: model matrix must be the identity (the reference never uploads another one, "
                    "App/src/Application.cpp:489-492)");
    c->u = *u;
    c->have_uniforms = true;
    return VR_OK;
}

void* vr_frame_device_ptr(vr_ctx* c) { return c ? (void*)c->d_frame : nullptr; }

int vr_viewport(const vr_ctx* c, uint32_t* width, uint32_t* height, int* device_id)
{
    if (!c) return VR_ERR_INVALID_ARG;
    if (width) *width = c->W;
    if (height) *height = c->H;
    if (device_id) *device_id = c->device;
    return VR_OK;
}

// Event-timed span of one 150 us single-wavefront spin on a and, if b is given, a second one on b right behind it.
static float spin_span_ms(hipStream_t a, hipStream_t b, hipEvent_t e0, hipEvent_t e1)
{
    const unsigned long long ticks = 15000;  // 150 us of the 100 MHz clock
    (void)hipStreamSynchronize(a);
    if (b) (void)hipStreamSynchronize(b);
    (void)hipEventRecord(e0, a);
    hipLaunchKernelGGL(spin_kernel, dim3(1), dim3(64), 0, a, ticks, (unsigned*)nullptr);
    if (b) hipLaunchKernelGGL(spin_kernel, dim3(1), dim3(64), 0, b, ticks, (unsigned*)nullptr);
    (void)hipEventRecord(e1, b ? b : a);
    (void)hipStreamSynchronize(a);
    if (b) (void)hipStreamSynchronize(b);
    float ms = 0.0f;
    if (hipEventElapsedTime(&ms, e0, e1) != hipSuccess) return -1.0f;
    return ms;
}

// true if kernels enqueued on a and b run concurrently: two spins take about as long as one (`one_ms`, measured on this
// box a moment ago -- launch overheads differ between boxes and runs, a fixed limit misjudged them now and then), not twice
static bool streams_overlap(hipStream_t a, hipStream_t b, hipEvent_t e0, hipEvent_t e1, float one_ms)
{
    for (int attempt = 0; attempt < 2; ++attempt) {  // a hiccup (page fault, clock ramp) must not cost a stream
        const float ms = spin_span_ms(a, b, e0, e1);
        if (getenv("VR_DEBUG_STREAMS")) fprintf(stderr, "[vr_stream] pair %p %p: %.3f ms (one spin %.3f ms)\n", (void*)a, (void*)b, ms, one_ms);
        if (ms < 0.0f || one_ms <= 0.0f) return true;  // cannot tell: assume the best
        if (ms < one_ms + 0.075f) return true;
    }
    return false;
}

void* vr_stream(vr_ctx* c, int index)
{
    if (!c || index < 0 || index >= kStreams) return nullptr;
    if (c->n_flight == 0) {
        if (hipSetDevice(c->device) != hipSuccess) return nullptr;
        (void)hipGetLastError();
        Event e0, e1;
        if (e0.create() != hipSuccess || e1.create() != hipSuccess) return nullptr;
        // candidates are created one by one; one is kept if it overlaps with every stream kept so far (at most 12 tries).
        // Rejected candidates stay alive until the search is over: the runtime hands a stream that is destroyed and created
        // again the very same hardware queue, and the search would try one queue twelve times.
        float one_ms = -1.0f;
        Stream rejected[12];  // (destroyed when the search is over)
        int n_rejected = 0;
        for (int tries = 0; tries < 12 && c->n_flight < kStreams; ++tries) {
            Stream cand;
            if (cand.create() != hipSuccess) break;
            const hipStream_t s = cand;
            if (c->n_flight == 0) {  // the yardstick: one spin alone (the second measurement: the first one warms up)
                (void)spin_span_ms(s, nullptr, e0, e1);
                one_ms = spin_span_ms(s, nullptr, e0, e1);
            }
            bool ok = true;
            for (int k = 0; k < c->n_flight && ok; ++k) ok = streams_overlap(c->flight[k], s, e0, e1, one_ms);
            // ... and with the stream of the launch-order sorts, whose barriers (a sort waits for its launch) would hold back
            // the launches of a render stream that shares its queue
            if (ok && c->order.stream) ok = streams_overlap(c->order.stream, s, e0, e1, one_ms);
            (ok ? c->flight[c->n_flight++] : rejected[n_rejected++]) = std::move(cand);  // (rejected: shares a hardware queue with a kept one)
        }
        (void)hipGetLastError();
        if (c->n_flight == 0) return nullptr;
    }
    return (void*)c->flight[index % c->n_flight];
}

int vr_hint_frames_in_flight(vr_ctx* c, int frames)
{
    if (!c) return VR_ERR_INVALID_ARG;
    if (frames < 1 || frames > kStreams) return fail(c, VR_ERR_INVALID_ARG, "vr_hint_frames_in_flight: 1 .. 4");
    c->frames_in_flight = frames;
    return VR_OK;
}

int vr_set_arithmetic(vr_ctx* c, int mode)
{
    if (!c) return VR_ERR_INVALID_ARG;
    if (mode != VR_ARITH_SEPARATE && mode != VR_ARITH_FUSED) return fail(c, VR_ERR_INVALID_ARG, "vr_set_arithmetic: unknown mode");
    c->arith = mode;
    return VR_OK;
}

int vr_set_iso_value(vr_ctx* c, float iso)
{
    if (!c) return VR_ERR_INVALID_ARG;
    if (!std::isfinite(iso)) return fail(c, VR_ERR_INVALID_ARG, "vr_set_iso_value: the level must be finite");
    c->iso = iso;
    return VR_OK;
}

int vr_set_shadows(vr_ctx* c, int grid_divisor, float opacity_scale)
{
    if (!c) return VR_ERR_INVALID_ARG;
    if (grid_divisor != 0 && grid_divisor != 1 && grid_divisor != 2 && grid_divisor != 4 && grid_divisor != 8)
        return fail(c, VR_ERR_INVALID_ARG, "vr_set_shadows: the divisor must be 0 (off), 1, 2, 4 or 8");
    if (!std::isfinite(opacity_scale) || !(opacity_scale >= 0.0f))
        return fail(c, VR_ERR_INVALID_ARG, "vr_set_shadows: the opacity scale must be finite and >= 0");
    c->shadows.div = grid_divisor;
    c->shadows.sigma = opacity_scale;
    return VR_OK;
}

int vr_set_output(vr_ctx* c, int mode)
{
    if (!c) return VR_ERR_INVALID_ARG;
    if (mode != VR_OUTPUT_COLOR && mode != VR_OUTPUT_SURFACE) return fail(c, VR_ERR_INVALID_ARG, "vr_set_output: unknown mode");
    c->output = mode;
    return VR_OK;
}

int vr_set_ray_bounds(vr_ctx* c, const void* d_near, const void* d_far)
{
    if (!c) return VR_ERR_INVALID_ARG;
    c->d_near = static_cast<const float*>(d_near);
    c->d_far = static_cast<const float*>(d_far);
    return VR_OK;
}

int vr_set_surface_threshold(vr_ctx* c, float tau)
{
    if (!c) return VR_ERR_INVALID_ARG;
    if (!std::isfinite(tau) || !(tau >= 0.0f) || !(tau < 1.0f))
        return fail(c, VR_ERR_INVALID_ARG, "vr_set_surface_threshold: the threshold must be finite, >= 0 and < 1");
    c->surf_tau = tau;
    return VR_OK;
}

int vr_set_kernel_flavour(vr_ctx* c, int flavour)
{
    if (!c) return VR_ERR_INVALID_ARG;
    if (!flavour_in_range(flavour)) return fail(c, VR_ERR_INVALID_ARG, "vr_set_kernel_flavour: unknown flavour");
    if (removed_flavour(flavour))
        return fail(c, VR_ERR_UNSUPPORTED, "vr_set_kernel_flavour: flavour " + std::to_string(flavour) + " was removed (it lost every A/B)");
    c->flavour = flavour;
    return VR_OK;
}

}  // extern "C"
