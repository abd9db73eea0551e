// vr_api.hip -- implementation of the C ABI declared in include/vr.h on top of the gfx950 kernels.
// No CPU fallback exists behind this ABI (and nothing under oracle/ is referenced): without a usable HIP
// device vr_create fails with VR_ERR_HIP.
#include "../../include/vr.h"
#include "vr_launch.h"
// Histograms (vr_histogram_async): nothing to fuse, so this kernel exists once, here
#include "vr_hist.h"

// the same dispatch over the kernels compiled with fused multiply-adds (vr_fused.hip)
namespace vrf {
void launch_march(const vr::LaunchDesc& L, hipStream_t s, const vr::MarchBatch& B);
void launch_shadow_build(const vr::MarchParams& P, float* out, float sigma, bool skip, bool off32, hipStream_t s);
void launch_slice(const vr::SliceParams& S, int reduce, bool nearest, bool off32, bool skip, unsigned tiles, hipStream_t s);
}

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <string>
#include <vector>

using namespace vr;

namespace {

thread_local std::string g_create_error;

struct Timing {
    hipEvent_t ev_begin = nullptr, ev_k0 = nullptr, ev_k1 = nullptr, ev_end = nullptr;
    bool valid = false;
};

constexpr int kRing = 256;
struct KernelRing {  // one (start, stop) event pair per render call, reused round-robin
    hipEvent_t k0[kRing] = {}, k1[kRing] = {};
    long long head = 0;  // total launches recorded since the last reset
};

}  // namespace

constexpr int kInFlight = 8;  // launches that may be in flight at a time (record buffers used in turn; twice the streams, so that
                               // a caller with four frames in flight never blocks on its oldest launch)
constexpr int kStreams = 4;   // vr_stream(): streams for frames in flight
constexpr int kOrderRing = 16;  // launch-order buffers: written behind launch k, read by launches k+3 .. k+6 only (see enqueue_render)
constexpr int kGen = 4;         // generations of each table and of the distance field (vr_tf_upload_*_async)
constexpr int kStage = 8;       // pinned staging buffers of the asynchronous table edits
constexpr int kEditSeen = 8;    // streams remembered to have waited for the latest asynchronous edit
constexpr int kShadowRing = 4;  // light volumes kept (vr_set_shadows): one per key, the least recently used one rebuilt

// A device buffer of one generation: written by an edit, read by the launches that captured it while it was current, on any
// streams.  Rewritten only behind every one of them (reuse_wait): reader[k] is the order_seq of the latest launch in record slot k
// (seq % kInFlight) that read it, -1 if none since it was last written.
struct GenBuf {
    void* d = nullptr;
    size_t cap = 0;  // bytes
    long long reader[kInFlight];
    GenBuf() { written(); }
    void written()
    {
        for (auto& r : reader) r = -1;
    }
};

// Something built on `stream` with `ev` recorded behind the build: a launch on another stream waits for the event once (seen), none
// after a draining call (pending = false).
struct BuiltOn {
    hipEvent_t ev = nullptr;
    hipStream_t stream = nullptr;
    bool pending = false;
    hipStream_t seen[kEditSeen] = {};
    int seen_next = 0;
    void built(hipStream_t s)  // (ev has been recorded on s)
    {
        stream = s;
        pending = true;
        for (auto& x : seen) x = nullptr;
    }
    hipError_t order_behind(hipStream_t s)  // a launch on s comes after the build
    {
        if (!pending || s == stream) return hipSuccess;
        for (auto x : seen)
            if (x == s) return hipSuccess;
        const hipError_t e = hipStreamWaitEvent(s, ev, 0);
        if (e == hipSuccess) seen[seen_next++ % kEditSeen] = s;
        return e;
    }
};

struct vr_ctx {
    int device = 0;
    uint32_t W = 0, H = 0;
    hipStream_t stream = nullptr;
    DevVolume vol[VR_MAX_VOLUMES] = {};
    size_t vol_bytes[VR_MAX_VOLUMES] = {};
    float2* vol_bricks[VR_MAX_VOLUMES] = {};  // per brick: (max density, max(r,g,b)) -- empty-space skipping
    float* vol_dens[VR_MAX_VOLUMES] = {};     // scalar density plane of each slot (DevVolume::dens)
    size_t vol_dens_cap[VR_MAX_VOLUMES] = {};  // in voxels
    float4* vol_bricked[VR_MAX_VOLUMES] = {};  // the voxels again in 4 x 4 x 4 bricks (DevVolume::bricked), what the march kernels gather from
    float* vol_bdens[VR_MAX_VOLUMES] = {};     // ... and their density plane in the same order
    size_t vol_bricked_cap[VR_MAX_VOLUMES] = {};  // in slots (bricks x 64)
    bool vol_grad_derived[VR_MAX_VOLUMES] = {};  // .rgb verified to be PreComputeGradient(false) of .a, bit for bit
    int arith = VR_ARITH_SEPARATE;             // vr_set_arithmetic
    int layout_mode = 0;                       // vr_set_volume_layout: 0 bricked copy + its density plane, 1 vec4 voxels only,
                                               // 3 x-fastest voxels + density plane (2, gradients on the fly, was removed)
    float2* merged_bricks = nullptr;           // VOLUME_MASK: (CT density max, mask rgb max), rebuilt when stale
    bool merged_stale = true;
    unsigned char* brick_dist = nullptr;       // distance field over the records in use (field[field_cur]); key below says for what
    GenBuf field[kGen];                        // its generations (an asynchronous opacity edit builds the next one)
    int field_cur = 0;
    unsigned char* dist_tmp = nullptr;         // the y pass's output, the z pass's input
    size_t tmp_cap = 0;
    int dist_bn[3] = {0, 0, 0};                // bricks per axis of the field
    const void* dist_records = nullptr;
    unsigned long long dist_epoch = ~0ull;     // volume-change counter the field was built at
    int dist_z = -2, dist_res = 0, dist_rgb = -1;
    unsigned long long brick_epoch = 0;        // bumped whenever any brick table changes
    int tf_zero_prefix[VR_MAX_TFS] = {-1, -1};  // zero prefix of each opacity table, -1 if none / not finite
    bool tf_color_finite[VR_MAX_TFS] = {false, false};
    bool tf_opacity_finite[VR_MAX_TFS] = {false, false};
    DevTF tf[VR_MAX_TFS] = {};
    GenBuf tf_buf[VR_MAX_TFS][2][kGen];        // [slot][opacity, colour]: the table's generations, tf_cur the one in use (DevTF layout)
    int tf_cur[VR_MAX_TFS][2] = {};
    // Asynchronous edits (vr_tf_upload_*_async): each records edit_ev on its stream, behind the one before it; a launch on
    // another stream waits for it once (edit_seen), nothing once a draining call has seen it (drained_gen).
    hipEvent_t edit_ev = nullptr;
    hipStream_t edit_stream = nullptr;
    unsigned long long edit_gen = 0, drained_gen = 0;
    struct EditSeen {
        hipStream_t s = nullptr;
        unsigned long long gen = 0;
    } edit_seen[kEditSeen];
    int seen_next = 0;
    struct Stage {  // pinned copy of an edited table, in the DevTF layout; reused behind its copy's event
        void* h = nullptr;
        size_t cap = 0;
        hipEvent_t done = nullptr;
        bool used = false;
    } stage[kStage];
    unsigned stage_next = 0;
    std::vector<void*> retired_dev, retired_host;  // replaced on a non-blocking path: freed by the next draining call
    // What each field build reports (SkipSummary, pinned, one per field generation) and the device words it accumulates in.
    // skip_pending: a build's count and box have not reached the host yet -- launches use the unbounded box meanwhile.
    SkipSummary* h_skip = nullptr;
    SkipSumDev* d_skip_sum = nullptr;
    unsigned long long skip_gen = 0;
    bool skip_pending = false;
    int skip_box[6] = {0x7fffffff, 0x7fffffff, 0x7fffffff, -1, -1, -1};  // of the field in use, once known (vr_skip_field)
    unsigned long long skip_active = 0;
    long long unbounded_launches = 0;
    vr_uniforms u = {};
    bool have_uniforms = false;
    float4* d_frame = nullptr;
    float4* d_tiles = nullptr;
    size_t tiles_cap = 0;       // in float4
    int last_tiles = 0;         // tiles rendered by the last vr_render_tiles
    uint32_t* d_present = nullptr;
    unsigned long long* d_counters = nullptr;  // [3] composited, covered, fetched
    // per-workgroup records (store_block_counts), kInFlight buffers used in turn so that several frames can be in
    // flight on different streams (the next ones fill the machine while the first one's long rays drain)
    unsigned long long* d_block_counts[kInFlight] = {};
    size_t block_counts_cap[kInFlight] = {};   // in blocks
    hipEvent_t slot_done[kInFlight] = {};      // recorded behind the launch that last used the slot (any stream)
    bool slot_used[kInFlight] = {};
    unsigned* d_pw_heads = nullptr;            // queue heads of the persistent-wavefront kernel: kInFlight x 8 heads, 256 B apart
    bool pw_heads_dirty[kInFlight] = {};       // the slot's last persistent launch had no sort behind it to clear its heads
    // Longest-first launch order (MarchParams::order): behind every march launch one small kernel sorts that launch's
    // blocks by their longest ray chain; a later launch of the same shape takes its blocks in that order.
    struct OrderSlot {
        unsigned* buf = nullptr;
        size_t cap = 0;
        hipStream_t stream = nullptr;
        hipEvent_t sorted = nullptr;
        unsigned long long key = 0, seq = 0;
        unsigned long long scene_key = 0;  // what the launch rendered, whatever kernel form it took (the chain length's key)
        bool valid = false;
    } order_ring[kOrderRing];
    unsigned long long* h_span = nullptr;  // pinned, kRing words: duration of launch q in 100 MHz ticks + 1, from its records (0 = not known)
    bool ring_events[kRing] = {};          // launch q was timed with the events k0 / k1 instead (no sort behind it)
    unsigned long long* h_end = nullptr;   // pinned, kRing words: end of launch q's last workgroup on the 100 MHz device clock, | 1 (0 = not known)
    unsigned* h_chain = nullptr;  // pinned, one word per ring slot: longest ray chain + 1 of that launch (0 = not known yet)
    // Measured kernel choice (flavour 0): every kernel form is bit-identical, so the context tries the eligible ones on
    // the caller's own frames and keeps the fastest by the launches' own records -- per "what is launched of what".
    struct Tune {
        unsigned long long key = 0;   // shader, share, viewport, frames per launch, frames in flight, scene epoch, arithmetic, layout (0 = free)
        unsigned long long shape = 0; // ... the same without the scene's epochs: a new scene starts from what the last one of this shape kept
        int n = 0, cand[6] = {};      // the eligible flavours; cand[0] = the prior's pick (what runs while nothing is known)
        int cur = 0, issued = 0;      // candidate on trial, launches it has had
        int per = 3, settle = 4;      // launches per candidate; launches before the trial starts (no launch order exists yet)
        long long launch[6][16] = {}; // ring.head of every trial launch of every candidate (other shapes' launches may lie in between)
        int choice = -1;              // index into cand of the kernel kept (-1 = trial running)
        unsigned chain_ref = 0;       // longest ray chain + 1 when it was chosen: the trial re-opens when that has moved by a quarter
        float cost[6] = {};           // ms per launch measured (0 = no data)
        unsigned long long used = 0;  // (least recently used slot is recycled)
    } tune[8];
    unsigned long long tune_clock = 0;
    unsigned long long tf_epoch = 0;  // bumped by every table upload
    int tune_mode = 1;                // VR_EXP_TUNE=0: the prior alone (round 3's thresholds)
    int frames_in_flight = 1;                 // vr_hint_frames_in_flight: frames the caller keeps in flight on different streams
    unsigned long long order_seq = 0;
    hipStream_t flight[kStreams] = {};  // vr_stream(): streams probed to run side by side (created on first use)
    int n_flight = 0;
    hipStream_t order_stream = nullptr;  // the sorts run here, behind their launch's event: never on a frame's critical path
    int cnt_buf = 0;                           // the buffer the last launch wrote
    bool cnt_pending = false;                  // block counts of the last launch not summed / copied yet
    int cnt_blocks = 0;
    bool event_timing = false;                 // vr_set_kernel_timing(VR_TIMING_EVENTS): time every launch with HIP events
    size_t cnt_offset = 0;                     // ... and where in that buffer the records of its last frame start (u64 words)
    unsigned long long* h_counters = nullptr;  // pinned [3]
    Timing tm;
    KernelRing ring;
    int flavour = 0;
    int n_cus = 256;          // compute units of the device
    int default_flavour = 0;  // what flavour 0 resolves to (experiment knob VR_EXP_FLAVOUR)
    int last_flavour = 0;     // the flavour the last launch resolved to
    unsigned p2_window = 0;   // flavours 16 / 17: records per gather window (VR_EXP_P2_WINDOW: the moving window of volumes >= 4 GiB, forced
                              // onto small volumes by the tests; 0 = what the hardware reaches, just below 4 GiB)
    double active_fraction = 1.0;  // share of bricks that are not inert, of the distance field in use
    float abox[6] = {-3.0e38f, -3.0e38f, -3.0e38f, 3.0e38f, 3.0e38f, 3.0e38f};  // uvw box around the active bricks of that field (MarchParams::abox)
    // Intensity projections (vr_proj.h), the isosurface (vr_iso.h) and slice views (vr_slice.h): (min, max) of a volume slot per
    // empty-space brick and over the whole volume, kept per slot ([0]: what the projections and the isosurface read), rebuilt on the
    // launch's stream by the first skipping launch that reads them after a volume change (proj_epoch = the brick_epoch they were built
    // at).  Launches on other streams wait once for the event behind the build (proj_built).
    float2* proj_rec[VR_MAX_VOLUMES] = {};
    size_t proj_rec_cap[VR_MAX_VOLUMES] = {};  // bytes
    float2* proj_range[VR_MAX_VOLUMES] = {};
    unsigned long long proj_epoch[VR_MAX_VOLUMES] = {~0ull, ~0ull, ~0ull};
    BuiltOn proj_built[VR_MAX_VOLUMES];
    // Slice views (vr_slice_async): the wavefront records of the slice launches, one buffer per record slot (a slice takes a record
    // slot like every launch, and leaves the march launches' records, counters and timings alone), and which of them the last
    // slice wrote (vr_slice_counters)
    unsigned long long* d_slice_counts[kInFlight] = {};
    size_t slice_counts_cap[kInFlight] = {};  // in workgroups
    int slice_buf = -1;
    unsigned slice_tiles = 0;
    void* d_slice_out = nullptr;  // vr_slice_render's device output (grown on demand)
    size_t slice_out_cap = 0;     // bytes
    // Histograms (vr_histogram_async): the three counters of the histogram launches, one buffer per record slot (a histogram takes
    // a record slot like a slice, and leaves every other launch's bookkeeping alone), which of them the last histogram wrote
    // (vr_hist_counters), and vr_histogram's device outputs (grown on demand)
    unsigned long long* d_hist_stats[kInFlight] = {};
    int hist_buf = -1;
    void* d_hist_out = nullptr;
    size_t hist_out_cap = 0;  // bytes
    bool last_unmeasured = false;  // the last launch's family is never measured (KernelForm::measured): vr_kernel_choice reports no candidates
    float iso = 0.5f;        // VR_VARIANT_ISO's level (vr_set_iso_value), copied into MarchParams::iso at enqueue
    // Shadows of the lit shader (vr_set_shadows, vr_shadow.h): the setting, and a ring of light volumes, one per key.  A launch whose key
    // matches an entry reads it (waiting once per stream for its build); otherwise it builds the least recently used entry on its own
    // stream, behind every launch still reading it (buf.reader, as the table generations).  A volume change drains the device and
    // empties the ring.
    int shadow_div = 0;                     // 0 = off; 1, 2, 4, 8 = voxels per light-volume texel and axis
    float shadow_sigma = 1.0f;              // opacity scale
    unsigned long long opacity_edits = 0;   // bumped by every upload of TF slot 0's opacity table, synchronous or not (the key's content)
    struct ShadowKey {
        unsigned long long epoch = 0, opacity = 0;  // brick_epoch, opacity_edits
        uint32_t light[3] = {}, box[6] = {}, sigma = 0;
        int div = 0, arith = 0;
        bool operator==(const ShadowKey& o) const
        {
            return epoch == o.epoch && opacity == o.opacity && std::memcmp(light, o.light, sizeof light) == 0 &&
                   std::memcmp(box, o.box, sizeof box) == 0 && sigma == o.sigma && div == o.div && arith == o.arith;
        }
    };
    struct ShadowVol {
        GenBuf buf;
        ShadowKey key;
        bool valid = false;
        BuiltOn built;                // the build may still run: other streams wait for it once
        unsigned long long used = 0;  // (least recently used entry is rebuilt)
    } shadow[kShadowRing];
    unsigned long long shadow_clock = 0;
    int shadow_cur = -1;  // the entry the launch being enqueued reads (mark_reads)
    // Surface-position output (vr_set_output, vr_surf.h): the setting and the threshold, both captured at enqueue; vr_pick's frame
    // (allocated on first use, freed with the viewport's buffers), and the pixel a pick launch is confined to (pick_px[0] < 0: none).
    int output = VR_OUTPUT_COLOR;
    float surf_tau = 0.5f;
    float4* d_pick = nullptr;
    float* d_pick_depth = nullptr;
    int pick_px[2] = {-1, -1};
    // Per-pixel ray bounds (vr_set_ray_bounds, vr_bound.h): the caller's depth buffers, W*H floats each (nullptr: no bound on that side);
    // captured at enqueue, dropped by vr_resize
    const float* d_near = nullptr;
    const float* d_far = nullptr;
    std::string err;
};

namespace {

// kernel forms that lost every A/B and were removed (HISTORY.md): vr_set_kernel_flavour rejects them, VR_EXP_FLAVOUR ignores them
bool removed_flavour(int f) { return f == 2 || f == 3 || f == 4 || f == 5 || f == 9 || f == 14; }

int fail(vr_ctx* c, int code, const std::string& msg)
{
    if (c) c->err = msg;
    else g_create_error = msg;
    return code;
}

#define VR_HIP(c, call)                                                                               \
    do {                                                                                              \
        hipError_t e__ = (call);                                                                      \
        if (e__ != hipSuccess)                                                                        \
            return fail((c), e__ == hipErrorOutOfMemory ? VR_ERR_OOM : VR_ERR_HIP,                    \
                        std::string(#call) + " (vr_api.hip:" + std::to_string(__LINE__) + "): " + hipGetErrorString(e__));                          \
    } while (0)

int refresh_bricks(vr_ctx* c, int slot);

int tiles_x_of(const vr_ctx* c) { return (int)((c->W + kTile - 1) / kTile); }
int tiles_y_of(const vr_ctx* c) { return (int)((c->H + kTile - 1) / kTile); }

int tile_count(const vr_ctx* c, int rank, int world)
{
    int total = tiles_x_of(c) * tiles_y_of(c);
    if (rank >= total) return 0;
    return (total - rank + world - 1) / world;
}

bool is_identity(const float* m)
{
    for (int i = 0; i < 16; ++i)
        if (m[i] != ((i % 5 == 0) ? 1.0f : 0.0f)) return false;
    return true;
}

bool is_projection(int variant) { return variant == VR_VARIANT_MIP || variant == VR_VARIANT_MINIP || variant == VR_VARIANT_AVERAGE; }

// volumes / TF pairs each variant samples (vr.h slot tables)
void variant_needs(int variant, int* nvol, int* ntf)
{
    switch (variant) {
    case VR_VARIANT_BASIC:
    case VR_VARIANT_LIGHT:
    case VR_VARIANT_LIGHT_INSHADER:
    case VR_VARIANT_MIP:
    case VR_VARIANT_MINIP:
    case VR_VARIANT_AVERAGE:
    case VR_VARIANT_ISO: *nvol = 1; *ntf = 1; break;
    case VR_VARIANT_VOLUME_MASK: *nvol = 3; *ntf = 2; break;
    case VR_VARIANT_THREE_FILES: *nvol = 2; *ntf = 2; break;  // the mask (slot 2) is bound but never sampled
    case VR_VARIANT_MULTI_CTRT: *nvol = 2; *ntf = 2; break;
    case VR_VARIANT_ILLUSTRATIVE: *nvol = 2; *ntf = 2; break;
    default: *nvol = 2; *ntf = 1; break;  // TF_CALIB
    }
}

int alloc_frame(vr_ctx* c)
{
    VR_HIP(c, hipSetDevice(c->device));
    if (c->d_frame) (void)hipFree(c->d_frame);
    if (c->d_present) (void)hipFree(c->d_present);
    if (c->d_pick) (void)hipFree(c->d_pick);
    c->d_frame = nullptr;
    c->d_present = nullptr;
    c->d_pick = nullptr;
    size_t n = (size_t)c->W * c->H;
    VR_HIP(c, hipMalloc(&c->d_frame, n * sizeof(float4)));
    VR_HIP(c, hipMalloc(&c->d_present, n * sizeof(uint32_t)));
    VR_HIP(c, hipMemsetAsync(c->d_frame, 0, n * sizeof(float4), c->stream));
    return VR_OK;
}

// Inverse of a column-major 4x4 in double precision (cofactors); false if singular / not finite.
bool invert4(const float* m, double* o)
{
    double a[16], inv[16];
    for (int i = 0; i < 16; ++i) a[i] = m[i];
    inv[0] = a[5] * a[10] * a[15] - a[5] * a[11] * a[14] - a[9] * a[6] * a[15] + a[9] * a[7] * a[14] + a[13] * a[6] * a[11] - a[13] * a[7] * a[10];
    inv[4] = -a[4] * a[10] * a[15] + a[4] * a[11] * a[14] + a[8] * a[6] * a[15] - a[8] * a[7] * a[14] - a[12] * a[6] * a[11] + a[12] * a[7] * a[10];
    inv[8] = a[4] * a[9] * a[15] - a[4] * a[11] * a[13] - a[8] * a[5] * a[15] + a[8] * a[7] * a[13] + a[12] * a[5] * a[11] - a[12] * a[7] * a[9];
    inv[12] = -a[4] * a[9] * a[14] + a[4] * a[10] * a[13] + a[8] * a[5] * a[14] - a[8] * a[6] * a[13] - a[12] * a[5] * a[10] + a[12] * a[6] * a[9];
    inv[1] = -a[1] * a[10] * a[15] + a[1] * a[11] * a[14] + a[9] * a[2] * a[15] - a[9] * a[3] * a[14] - a[13] * a[2] * a[11] + a[13] * a[3] * a[10];
    inv[5] = a[0] * a[10] * a[15] - a[0] * a[11] * a[14] - a[8] * a[2] * a[15] + a[8] * a[3] * a[14] + a[12] * a[2] * a[11] - a[12] * a[3] * a[10];
    inv[9] = -a[0] * a[9] * a[15] + a[0] * a[11] * a[13] + a[8] * a[1] * a[15] - a[8] * a[3] * a[13] - a[12] * a[1] * a[11] + a[12] * a[3] * a[9];
    inv[13] = a[0] * a[9] * a[14] - a[0] * a[10] * a[13] - a[8] * a[1] * a[14] + a[8] * a[2] * a[13] + a[12] * a[1] * a[10] - a[12] * a[2] * a[9];
    inv[2] = a[1] * a[6] * a[15] - a[1] * a[7] * a[14] - a[5] * a[2] * a[15] + a[5] * a[3] * a[14] + a[13] * a[2] * a[7] - a[13] * a[3] * a[6];
    inv[6] = -a[0] * a[6] * a[15] + a[0] * a[7] * a[14] + a[4] * a[2] * a[15] - a[4] * a[3] * a[14] - a[12] * a[2] * a[7] + a[12] * a[3] * a[6];
    inv[10] = a[0] * a[5] * a[15] - a[0] * a[7] * a[13] - a[4] * a[1] * a[15] + a[4] * a[3] * a[13] + a[12] * a[1] * a[7] - a[12] * a[3] * a[5];
    inv[14] = -a[0] * a[5] * a[14] + a[0] * a[6] * a[13] + a[4] * a[1] * a[14] - a[4] * a[2] * a[13] - a[12] * a[1] * a[6] + a[12] * a[2] * a[5];
    inv[3] = -a[1] * a[6] * a[11] + a[1] * a[7] * a[10] + a[5] * a[2] * a[11] - a[5] * a[3] * a[10] - a[9] * a[2] * a[7] + a[9] * a[3] * a[6];
    inv[7] = a[0] * a[6] * a[11] - a[0] * a[7] * a[10] - a[4] * a[2] * a[11] + a[4] * a[3] * a[10] + a[8] * a[2] * a[7] - a[8] * a[3] * a[6];
    inv[11] = -a[0] * a[5] * a[11] + a[0] * a[7] * a[9] + a[4] * a[1] * a[11] - a[4] * a[3] * a[9] - a[8] * a[1] * a[7] + a[8] * a[3] * a[5];
    inv[15] = a[0] * a[5] * a[10] - a[0] * a[6] * a[9] - a[4] * a[1] * a[10] + a[4] * a[2] * a[9] + a[8] * a[1] * a[6] - a[8] * a[2] * a[5];
    const double det = a[0] * inv[0] + a[1] * inv[4] + a[2] * inv[8] + a[3] * inv[12];
    if (!(det - det == 0.0) || det == 0.0) return false;
    for (int i = 0; i < 16; ++i) {
        o[i] = inv[i] / det;
        if (!(o[i] - o[i] == 0.0)) return false;
    }
    return true;
}

// Pixel rectangle outside which no ray can hit the box [-.5,.5]^2 x [-.25,.25]: the rays are defined by proj_inv and
// view_inv (setup_ray), so the box corners are projected with the inverses of exactly those.  With every corner in
// front of the eye the box projects inside the hull of its corners; 3 pixels of margin dwarf the rounding.  Anything
// doubtful (singular matrices, a corner at or behind the eye plane, non-finite numbers) -> the whole frame.
void hit_rectangle(const vr_uniforms& u, int W, int H, int rect[4])
{
    rect[0] = 0;
    rect[1] = 0;
    rect[2] = W - 1;
    rect[3] = H - 1;
    double proj[16], view[16];
    if (!invert4(u.proj_inv, proj) || !invert4(u.view_inv, view)) return;
    double x0 = 1e300, y0 = 1e300, x1 = -1e300, y1 = -1e300;
    for (int k = 0; k < 8; ++k) {
        const double wp[4] = {(k & 1) ? 0.5 : -0.5, (k & 2) ? 0.5 : -0.5, (k & 4) ? 0.25 : -0.25, 1.0};
        double e[4], cl[4];
        for (int r = 0; r < 4; ++r) e[r] = view[r] * wp[0] + view[4 + r] * wp[1] + view[8 + r] * wp[2] + view[12 + r] * wp[3];
        for (int r = 0; r < 4; ++r) cl[r] = proj[r] * e[0] + proj[4 + r] * e[1] + proj[8 + r] * e[2] + proj[12 + r] * e[3];
        if (!(cl[3] > 1e-9)) return;
        const double px = (cl[0] / cl[3] + 1.0) * 0.5 * W, py = (1.0 - cl[1] / cl[3]) * 0.5 * H;
        if (!(px - px == 0.0) || !(py - py == 0.0)) return;
        x0 = px < x0 ? px : x0;
        x1 = px > x1 ? px : x1;
        y0 = py < y0 ? py : y0;
        y1 = py > y1 ? py : y1;
    }
    auto clampd = [](double v, double lo, double hi) { return v < lo ? lo : (v > hi ? hi : v); };
    rect[0] = (int)clampd(x0 - 3.0, 0.0, (double)W);
    rect[1] = (int)clampd(y0 - 3.0, 0.0, (double)H);
    rect[2] = (int)clampd(x1 + 3.0, -1.0, (double)(W - 1));
    rect[3] = (int)clampd(y1 + 3.0, -1.0, (double)(H - 1));
}

// finite and of moderate size: products of a colour, a light term and a shading factor stay finite, so "x * 0 == 0"
// holds for everything a provably-zero opacity is multiplied with
bool all_finite(const float* v, int n)
{
    for (int i = 0; i < n; ++i)
        if (!(v[i] - v[i] == 0.0f) || !(v[i] <= 1.0e15f && v[i] >= -1.0e15f)) return false;
    return true;
}

// the fields of a launch's parameters that come from the uniforms of ONE frame
void fill_frame_params(MarchParams& P, const vr_uniforms& u)
{
    std::memcpy(P.proj_inv, u.proj_inv, sizeof P.proj_inv);
    std::memcpy(P.view_inv, u.view_inv, sizeof P.view_inv);
    hit_rectangle(u, P.W, P.H, P.rect);
    P.fragment_mode = u.fragment_mode;
    P.steps_count = u.steps_count;
    P.step_size = u.step_size;
    // IsInSampleCoords bounds, BasicVolumeApp.wgsl:73-74 (same f32 expressions as the shader)
    P.bmin[0] = 0.0f + u.clip_x[0]; P.bmin[1] = 0.0f + u.clip_y[0]; P.bmin[2] = 0.0f + u.clip_z[0];
    P.bmax[0] = 1.0f - u.clip_x[1]; P.bmax[1] = 1.0f - u.clip_y[1]; P.bmax[2] = 1.0f - u.clip_z[1];
    P.toggle_varstep = u.toggles[0];
    P.toggle_jitter = u.toggles[1];
    for (int i = 0; i < 3; ++i) {
        P.light_pos[i] = u.light_pos[i];
        P.light_amb[i] = u.light_ambient[i];
        P.light_dif[i] = u.light_diffuse[i];
        P.camera_pos[i] = u.camera_pos[i];
    }
}

// The measured kernel choice (flavour 0).  `cand[0 .. n)` are the flavours that may run this launch (cand[0] = the prior's pick); returns
// the one to launch now.  A trial gives every candidate `per` launches in turn -- after `settle` launches of the prior, so that a
// launch order exists (the trial then measures what the steady state runs) -- and reads the launches' durations from
// the pinned words their sorts fill (no synchronisation: a trial is evaluated when its last word has arrived; until then the
// prior runs).  One launch at a time: the shortest first-start-to-last-end span of a candidate's launches but its first.  Launches
// in flight: the mean interval between the ends of its consecutive launches that ran beside launches of the same candidate only
// (3 x in_flight + 2 launches per turn, the first and the last in_flight of them not used).  The trial re-opens when the scene, the tables,
// the launch shape or the frames-in-flight hint change (the key) and when the longest ray chain has moved by a quarter.
int tune_pick(vr_ctx* c, unsigned long long key, unsigned long long shape, const int* cand, int n, unsigned chain_now, bool measurable)
{
    if (n <= 1) return cand[0];
    vr_ctx::Tune* t = nullptr;
    for (auto& e : c->tune)
        if (e.key == key) t = &e;
    const int in_flight = c->frames_in_flight;
    auto reset = [&](vr_ctx::Tune& e, int first) {
        e.key = key;
        e.shape = shape;
        e.n = 0;
        e.cand[e.n++] = first;
        for (int i = 0; i < n; ++i)
            if (cand[i] != first && e.n < 6) e.cand[e.n++] = cand[i];
        e.cur = 0;
        e.issued = 0;
        e.per = in_flight > 1 ? 3 * in_flight + 2 : 3;  // (<= 14: kStreams is 4)
        e.settle = in_flight + 3;
        e.choice = -1;
        e.chain_ref = 0;
        for (int i = 0; i < 6; ++i) {
            e.cost[i] = 0.0f;
            for (int q = 0; q < 16; ++q) e.launch[i][q] = -1;
        }
    };
    if (!t) {
        // a new scene (or table, or arithmetic) of a shape that has been measured before: what that trial kept runs first, if it is
        // still eligible -- a host that edits a table frame after frame keeps its kernel while every new trial settles
        int first = cand[0];
        unsigned long long newest = 0;
        for (const auto& e : c->tune)
            if (e.key != 0 && e.shape == shape && e.choice >= 0 && e.used > newest)
                for (int i = 0; i < n; ++i)
                    if (cand[i] == e.cand[e.choice]) {
                        first = cand[i];
                        newest = e.used;
                    }
        t = &c->tune[0];
        for (auto& e : c->tune)
            if (e.used < t->used) t = &e;
        reset(*t, first);
    } else {
        // the eligible set may have changed under the same key (a flavour knob, a table that fits LDS no more)
        bool same = t->n == n;
        for (int i = 0; i < n && same; ++i) {
            bool found = false;
            for (int j = 0; j < t->n; ++j) found = found || t->cand[j] == cand[i];
            same = found;
        }
        if (!same) reset(*t, cand[0]);
    }
    t->used = ++c->tune_clock;
    if (t->choice >= 0) {
        if (chain_now != 0 && t->chain_ref != 0) {
            const unsigned lo = t->chain_ref - t->chain_ref / 4, hi = t->chain_ref + t->chain_ref / 4;
            if (chain_now < lo || chain_now > hi) reset(*t, t->cand[t->choice]);  // (the kernel kept so far runs while the new trial settles)
        }
        if (t->choice >= 0) return t->cand[t->choice];
    }
    if (!measurable) return t->cand[0];
    if (t->settle > 0) {
        --t->settle;
        return t->cand[0];
    }
    if (t->cur < t->n) {
        const int f = t->cand[t->cur];
        t->launch[t->cur][t->issued] = c->ring.head;  // (the ring slot this launch will record itself in)
        if (++t->issued == t->per) {
            ++t->cur;
            t->issued = 0;
        }
        return f;
    }
    // every candidate has had its turn: are the records in?
    const long long last = t->launch[t->n - 1][t->per - 1];
    // (a launch of the trial was never measured -- timed with events, or not ordered -- or so many launches of other shapes ran in
    // between that the trial's first ring slots are about to be written again: keep the prior)
    if (c->ring.head > last + 64 || c->ring.head - t->launch[0][0] >= kRing) {
        t->choice = 0;
        t->chain_ref = chain_now;
        return t->cand[0];
    }
    for (int i = 0; i < t->n; ++i)
        for (int q = 0; q < t->per; ++q)
            if (*(volatile unsigned long long*)&c->h_span[t->launch[i][q] % kRing] == 0) return t->cand[0];
    int best = 0;
    for (int i = 0; i < t->n; ++i) {
        double ticks;
        if (in_flight > 1) {
            // (its first `in_flight` launches ran beside the candidate before it, its last ones beside the next: the ends of the
            // launches in between are `in_flight + 2` intervals apart that are this candidate's alone)
            const unsigned long long e0 = *(volatile unsigned long long*)&c->h_end[t->launch[i][in_flight] % kRing];
            const unsigned long long e1 = *(volatile unsigned long long*)&c->h_end[t->launch[i][t->per - in_flight] % kRing];
            ticks = e1 > e0 ? (double)(e1 - e0) / (double)(t->per - 2 * in_flight) : 1.0e18;
        } else {
            ticks = 1.0e18;
            for (int q = 1; q < t->per; ++q) {
                const double v = (double)*(volatile unsigned long long*)&c->h_span[t->launch[i][q] % kRing];
                ticks = v < ticks ? v : ticks;
            }
        }
        t->cost[i] = (float)(ticks * 1.0e-5);  // 100 MHz ticks -> ms
        // (another kernel must be 2 % faster than the prior's to replace it: the spans of equal kernels differ by about that much)
        // (... with launches in flight by 5 %: a candidate's interior launches still run beside its neighbours' tails -- a trial that
        // measured march_kernel at 0.407 ms per C3 frame pipelined against 0.418 kept it, and it then ran at 0.467: gpurun_out/s2p)
        if (i > 0 && t->cost[i] < t->cost[best] * (best == 0 ? (in_flight > 1 ? 0.95f : 0.98f) : 1.0f)) best = i;
    }
    t->choice = best;
    t->chain_ref = chain_now;
    return t->cand[best];
}

// the bricked copy of a volume (DevVolume::bricked): storage bricks per axis, and their slots (voxels)
struct BrickedGrid {
    unsigned nbx, nby, nbz;
    size_t slots;
};
BrickedGrid bricked_grid(const DevVolume& v)
{
    const unsigned nbx = ((unsigned)v.nx + kVbM) >> kVbS, nby = ((unsigned)v.ny + kVbM) >> kVbS, nbz = ((unsigned)v.nz + kVbM) >> kVbS;
    return {nbx, nby, nbz, (size_t)nbx * nby * nbz * kVbN};
}

// empty-space bricks along an axis of n base cells
int skip_bricks(int n) { return (n + kBrickCells - 1) >> kBrickShift; }

// rays per hardware lane (n_cus x 4 x 5 x 64) of `frames` launches of this rank's share of the frame: how full they keep the machine
double rays_per_lane(const vr_ctx* c, int rank, int world, int frames)
{
    const long long px = (long long)tile_count(c, rank, world) * kTile * kTile;
    return (double)px * frames / ((double)c->n_cus * 4.0 * 5.0 * 64.0);
}

// what a launch rendered, whatever kernel form it took (OrderSlot::scene_key: the key of the longest ray chain its sort reports)
// (a surface launch -- vr_set_output -- is a scene of its own: its chains say nothing about the colour launch's)
// (so is a launch between ray bounds -- vr_set_ray_bounds)
unsigned long long scene_key(const vr_ctx* c, int variant, int rank, int world, bool packed, bool surface = false, bool bounded = false)
{
    return ((unsigned long long)(variant | (surface ? 0x80 : 0) | (bounded ? 0x40 : 0)) << 16) ^ ((unsigned long long)world << 8) ^ (unsigned long long)rank ^ (packed ? 1ull << 63 : 0ull) ^
           ((unsigned long long)c->W << 40) ^ ((unsigned long long)c->H << 24);
}

// TF slot 0 fits a workgroup's LDS beside nothing else: one resolution for both tables, R <= 8190 (128 KiB)
bool tf0_fits_lds(const vr_ctx* c) { return c->tf[0].res_o == c->tf[0].res_c && c->tf[0].res_o + 2 <= 8192; }

// The arguments of a launch and the slots its shader samples (*nvol volumes); *off32: every one of them below 4 GiB.
int check_render_args(vr_ctx* c, int variant, int rank, int world, int n_frames, const vr_uniforms* batch_u, void* const* batch_out,
                      int* nvol, bool* off32)
{
    if (variant < 0 || variant >= VR_VARIANT_COUNT) return fail(c, VR_ERR_INVALID_ARG, "vr_render: bad variant");
    if (world < 1 || rank < 0 || rank >= world) return fail(c, VR_ERR_INVALID_ARG, "vr_render: bad rank/world");
    if (n_frames < 1 || n_frames > kBatchMax) return fail(c, VR_ERR_INVALID_ARG, "vr_render: 1 .. 4 frames per launch");
    if (batch_u) {
        if (!batch_out) return fail(c, VR_ERR_INVALID_ARG, "vr_render: a batch needs its output buffers");
        for (int f = 0; f < n_frames; ++f) {
            if (!batch_out[f]) return fail(c, VR_ERR_INVALID_ARG, "vr_render: output buffer " + std::to_string(f) + " of the batch is NULL");
            if (batch_u[f].steps_count < 0) return fail(c, VR_ERR_INVALID_ARG, "vr_render: negative steps_count");
            if (!is_identity(batch_u[f].model))  // (as vr_set_uniforms)
                return fail(c, VR_ERR_UNSUPPORTED, "vr_render: model matrix must be the identity (App/src/Application.cpp:489-492)");
        }
    } else {
        if (n_frames != 1) return fail(c, VR_ERR_INVALID_ARG, "vr_render: several frames per launch need their uniforms");
        if (!c->have_uniforms) return fail(c, VR_ERR_NOT_READY, "vr_render: vr_set_uniforms has not been called");
    }
    int ntf;
    variant_needs(variant, nvol, &ntf);
    *off32 = true;
    for (int i = 0; i < *nvol; ++i) {
        if (!c->vol[i].data) return fail(c, VR_ERR_NOT_READY, "vr_render: volume slot " + std::to_string(i) + " is empty");
        if (c->vol_bytes[i] > 0xFFFFFFFFull) *off32 = false;
    }
    for (int i = 0; i < ntf; ++i)
        if (!c->tf[i].opacity || !c->tf[i].color)
            return fail(c, VR_ERR_NOT_READY, "vr_render: TF slot " + std::to_string(i) + " is empty");
    if ((batch_u ? batch_u[0] : c->u).steps_count < 0) return fail(c, VR_ERR_INVALID_ARG, "vr_render: negative steps_count");
    return VR_OK;
}

// The parameters of a launch that no kernel form changes; the volumes as the vec4 voxels and their density plane (the bricked copies
// replace them in use_bricked_copies).
// volume slot i as the vec4 voxels and their density plane
DevVolume linear_volume(const vr_ctx* c, int i)
{
    DevVolume v = c->vol[i];
    const bool plane = c->layout_mode != 1 && c->vol_dens[i] && c->vol[i].data;
    v.dens = plane ? c->vol_dens[i] : nullptr;
    v.a_base = plane ? reinterpret_cast<const char*>(c->vol_dens[i]) : reinterpret_cast<const char*>(c->vol[i].data) + 12;
    v.a_shift = plane ? 2 : 4;
    v.bricked = 0;
    v.brick_row = v.brick_slab = 0;
    const size_t lin_bytes = c->vol_bytes[i];
    v.data_bytes = lin_bytes > 0xFFFFFFFFull ? 0xFFFFFFFFu : (unsigned)lin_bytes;
    return v;
}

void fill_launch_params(const vr_ctx* c, MarchParams& P, const vr_uniforms& u0, int rank, int world, bool packed)
{
    std::memset(&P, 0, sizeof P);
    P.W = (int)c->W;
    P.H = (int)c->H;
    fill_frame_params(P, u0);
    for (int i = 0; i < VR_MAX_VOLUMES; ++i) P.vol[i] = linear_volume(c, i);
    for (int i = 0; i < VR_MAX_TFS; ++i) P.tf[i] = c->tf[i];
    P.rank = rank;
    P.world = world;
    P.tiles_x = tiles_x_of(c);
    P.tiles_y = tiles_y_of(c);
    P.n_tiles = tile_count(c, rank, world);
    P.packed = packed ? 1 : 0;
    P.n_blocks = P.n_tiles * kBlocksPerTile;
    P.iso = c->iso;  // (every frame of a batch: fill_batch copies P)
}

// the bricked copies (layout 0) are what the gathers read
void use_bricked_copy(const vr_ctx* c, int i, DevVolume& v)
{
    if (!c->vol[i].data || !c->vol_bricked[i] || !c->vol_bdens[i]) return;
    const BrickedGrid g = bricked_grid(c->vol[i]);
    if (g.slots > 0xFFFFFFFFull) return;  // (indices are 32 bits)
    v.data = c->vol_bricked[i];
    v.a_base = reinterpret_cast<const char*>(c->vol_bdens[i]);
    v.a_shift = 2;
    v.bricked = 1;
    v.brick_row = g.nbx * kVbN;
    v.brick_slab = g.nbx * g.nby * kVbN;
    v.data_bytes = g.slots * 16 > 0xFFFFFFFFull ? 0xFFFFFFFFu : (unsigned)(g.slots * 16);
}
void use_bricked_copies(const vr_ctx* c, MarchParams& P)
{
    for (int i = 0; i < VR_MAX_VOLUMES; ++i) use_bricked_copy(c, i, P.vol[i]);
}

// What a launch could run, worked out once before the kernel choice (choose_flavour).
struct Eligibility {
    bool p2_ok;             // two steps ahead (16, 17) can run
    unsigned p2_lds;        // ... with this much dynamic LDS (TF slot 0 and the three axis tables)
    bool lut_ok;            // 18 can run
    unsigned lut_lds;       // ... with this much (the slot tables of volume 0)
    bool can_skip;          // exact empty-space skipping (prepare_skip)
    bool whole_frame;       // enough rays to fill the machine in one frame
    unsigned chain_known;   // longest ray chain + 1 of the most recent launch of this scene shape whose sort has reported (0: none)
};

// the longest ray chain + 1 of the most recent launch of this scene shape whose sort has reported (written to pinned memory by the
// launch-order sort; read without synchronising, 0 = not known)
unsigned last_chain(const vr_ctx* c, unsigned long long skey)
{
    unsigned chain = 0;
    if (!c->h_chain) return chain;
    unsigned long long best_seq = 0;
    for (int i = 0; i < kOrderRing; ++i) {
        const unsigned v = *(volatile unsigned*)&c->h_chain[i];
        if (v != 0 && c->order_ring[i].scene_key == skey && c->order_ring[i].seq + 1 > best_seq) {
            best_seq = c->order_ring[i].seq + 1;
            chain = v;
        }
    }
    return chain;
}

Eligibility eligibility(const vr_ctx* c, int requested, int variant, int n_frames, int rank, int world, bool packed, const vr_uniforms* batch_u)
{
    Eligibility E = {};
    // two steps ahead (16, 17; march_p2_kernel, vr_p2.h): lit / unlit shader and the three-volume composite (with its brick records:
    // choose_flavour); TF slot 0 (one resolution for both tables) and the three axis tables in LDS; the bricked copy with 32-bit slots,
    // rows and slabs of bricks below 2^24 slots; a volume of 4 GiB or more through a moving window of at least four z-slabs of bricks.
    // Launches of several frames and launches in flight included.
    const int sv = variant == VR_VARIANT_VOLUME_MASK ? 2 : 0;  // the volume whose density drives tf[0]'s opacity
    E.p2_ok = (variant == VR_VARIANT_LIGHT || variant == VR_VARIANT_BASIC || variant == VR_VARIANT_VOLUME_MASK) && tf0_fits_lds(c) &&
              c->layout_mode == 0 && c->vol_bricked[sv] && c->vol_bdens[sv];
    if (E.p2_ok) {
        const DevVolume& v = c->vol[sv];
        const BrickedGrid g = bricked_grid(v);
        const size_t slab = (size_t)g.nbx * g.nby * kVbN, window = variant == VR_VARIANT_BASIC ? 0x3fffffffull : 0x0fffffffull;
        const size_t lds = (size_t)(c->tf[0].res_o + 2) * 16 + ((size_t)v.nx + v.ny + v.nz + 3) * 8;
        E.p2_ok = g.slots <= 0xFFFFFFFFull && slab < (1u << 24) && (c->p2_window ? c->p2_window / slab >= 3 : window / slab >= 4) && lds <= 160u * 1024u;
        E.p2_lds = (unsigned)lds;
    }
    // 18: march_kernel with the slot tables of volume 0 in its workgroup's LDS (make_cell_lut): the shaders that sample ONE volume, the
    // bricked copy with 32-bit slots
    E.lut_ok = (variant == VR_VARIANT_LIGHT || variant == VR_VARIANT_BASIC || variant == VR_VARIANT_LIGHT_INSHADER) && c->layout_mode == 0 &&
               c->vol_bricked[0] && c->vol_bdens[0];
    if (E.lut_ok) {
        E.lut_lds = (unsigned)(((size_t)c->vol[0].nx + c->vol[0].ny + c->vol[0].nz + 6) * 4);
        E.lut_ok = bricked_grid(c->vol[0]).slots <= 0xFFFFFFFFull && E.lut_lds <= 32u * 1024u;
    }
    // exact empty-space skipping: only for the shaders whose opacity is the CT table value alone, only when a zero-opacity sample is
    // provably the identity (finite colour table and light), and unless flavour 1 asks for the plain kernel (no rule of choose_flavour
    // turns another flavour into 1 or 1 into another)
    E.can_skip = (variant == VR_VARIANT_BASIC || variant == VR_VARIANT_LIGHT || variant == VR_VARIANT_THREE_FILES ||
                  variant == VR_VARIANT_VOLUME_MASK || variant == VR_VARIANT_LIGHT_INSHADER) &&
                 requested != 1 && c->vol_bricks[sv] && c->tf_zero_prefix[0] >= 0 && c->tf_color_finite[0];
    for (int f = 0; f < n_frames; ++f) E.can_skip = E.can_skip && all_finite(batch_u ? batch_u[f].light_pos : c->u.light_pos, 12);
    // the kernels index bricks with 24-bit multiplies and 32-bit byte offsets
    E.can_skip = E.can_skip && skip_bricks(c->vol[sv].nx) * (long long)skip_bricks(c->vol[sv].ny) < (1 << 23);
    if (variant == VR_VARIANT_THREE_FILES) E.can_skip = E.can_skip && c->tf_color_finite[1] && c->tf_opacity_finite[1];
    if (variant == VR_VARIANT_VOLUME_MASK)  // mask and CT must share one grid so that one brick index serves both
        E.can_skip = E.can_skip && c->vol_bricks[0] && c->vol[0].nx == c->vol[2].nx && c->vol[0].ny == c->vol[2].ny &&
                     c->vol[0].nz == c->vol[2].nz;
    E.whole_frame = rays_per_lane(c, rank, world, 1) >= 4.5;
    E.chain_known = requested == 0 ? last_chain(c, scene_key(c, variant, rank, world, packed)) : 0;
    return E;
}

// After a hipDeviceSynchronize: every asynchronous edit has completed, and what they replaced can be freed.
void drained(vr_ctx* c)
{
    for (void* p : c->retired_dev) (void)hipFree(p);
    for (void* p : c->retired_host) (void)hipHostFree(p);
    c->retired_dev.clear();
    c->retired_host.clear();
    c->drained_gen = c->edit_gen;
    for (auto& b : c->proj_built) b.pending = false;
    for (auto& e : c->shadow) e.built.pending = false;
}

// Before `s` rewrites generation b: every launch that read it must have finished, whatever its stream (launches on different
// streams finish in any order).  A reader fewer than kInFlight launches old still owns its record slot's event: s waits for it on
// the device, one wait per such slot.  An older one was waited for on the host by the take_record_slot that reused its slot.
int reuse_wait(vr_ctx* c, hipStream_t s, const GenBuf& b)
{
    for (int k = 0; k < kInFlight; ++k)
        if (b.reader[k] >= 0 && (unsigned long long)b.reader[k] + kInFlight >= c->order_seq)
            VR_HIP(c, hipStreamWaitEvent(s, c->slot_done[k], 0));
    return VR_OK;
}

// A launch on `s` comes after every asynchronous edit made so far: once per stream per edit, a wait for the latest edit's event
// (each edit is ordered behind the one before it).
int wait_for_edits(vr_ctx* c, hipStream_t s)
{
    if (c->edit_gen <= c->drained_gen) return VR_OK;
    vr_ctx::EditSeen* e = nullptr;
    for (auto& x : c->edit_seen)
        if (x.s == s) e = &x;
    if (e && e->gen >= c->edit_gen) return VR_OK;
    if (s != c->edit_stream) VR_HIP(c, hipStreamWaitEvent(s, c->edit_ev, 0));
    if (!e) e = &c->edit_seen[c->seen_next++ % kEditSeen];
    e->s = s;
    e->gen = c->edit_gen;
    return VR_OK;
}

// The launches' reads of the current generations (enqueued as launch order_seq, whose slot event is recorded behind it).
void mark_table_reads(vr_ctx* c, int slot)
{
    for (int k = 0; k < 2; ++k) {
        GenBuf& b = c->tf_buf[slot][k][c->tf_cur[slot][k]];
        if (b.d) b.reader[c->order_seq % kInFlight] = (long long)c->order_seq;
    }
}

void mark_reads(vr_ctx* c, const MarchParams& P)
{
    for (int i = 0; i < VR_MAX_TFS; ++i) mark_table_reads(c, i);
    if (P.brick_dist) c->field[c->field_cur].reader[c->order_seq % kInFlight] = (long long)c->order_seq;
    if (c->shadow_cur >= 0) c->shadow[c->shadow_cur].buf.reader[c->order_seq % kInFlight] = (long long)c->order_seq;
}

// The distance field of records `rec` (bricks bn) into `field` on `s`: the active bricks, the x, y and z passes (vr_kernels.h), the
// count and box of build `gen` into h_skip[slot].  dist_tmp holds at least bn[0] * bn[1] * bn[2] bytes.
int build_field(vr_ctx* c, hipStream_t s, const float2* rec, const int bn[3], int use_rgb, int zero_prefix, int res_o, unsigned char* field,
                int slot, unsigned long long gen)
{
    const int nb = bn[0] * bn[1] * bn[2];
    hipLaunchKernelGGL(brick_active_kernel, dim3((unsigned)((nb + 255) / 256)), dim3(256), 0, s, rec, field, nb, use_rgb, zero_prefix, res_o);
    const long long waves = (long long)((bn[0] + 63) >> 6) * bn[1] * bn[2];
    hipLaunchKernelGGL(brick_dist_x_kernel, dim3((unsigned)((waves + 3) / 4)), dim3(256), 0, s, field, bn[0], bn[1] * bn[2]);
    const unsigned tx = (unsigned)((bn[0] + kDistCols - 1) / kDistCols);
    hipLaunchKernelGGL((brick_dist_axis_kernel<false>), dim3(tx, (unsigned)((bn[1] + kDistRows - 1) / kDistRows), (unsigned)bn[2]), dim3(256),
                       0, s, field, c->dist_tmp, bn[0], bn[1], (size_t)bn[0], (size_t)bn[0] * bn[1], (SkipSumDev*)nullptr,
                       (SkipSummary*)nullptr, 0ull);
    hipLaunchKernelGGL((brick_dist_axis_kernel<true>), dim3(tx, (unsigned)((bn[2] + kDistRows - 1) / kDistRows), (unsigned)bn[1]), dim3(256),
                       0, s, c->dist_tmp, field, bn[0], bn[2], (size_t)bn[0] * bn[1], (size_t)bn[0], c->d_skip_sum + slot, c->h_skip + slot, gen);
    VR_HIP(c, hipGetLastError());
    return VR_OK;
}

// The count and box of the field in use, once its build has reported them (pinned h_skip, generation first): the share of active bricks
// (which the kernel choice reads) and the box of the active bricks in uvw with one brick of margin (MarchParams::abox): brick b of axis
// a holds the positions with p * bs - kBrickHalf in [b, b + 1), the first and the last brick those beyond them as well.
void adopt_skip(vr_ctx* c, const float bs[3])
{
    if (!c->skip_pending) return;
    const volatile SkipSummary& h = c->h_skip[c->field_cur];
    if (h.gen != c->skip_gen) return;
    __atomic_thread_fence(__ATOMIC_ACQUIRE);
    const long long nb = (long long)c->dist_bn[0] * c->dist_bn[1] * c->dist_bn[2];
    c->skip_active = h.count;
    c->active_fraction = nb > 0 ? (double)h.count / (double)nb : 1.0;
    for (int a = 0; a < 6; ++a) c->skip_box[a] = h.box[a];
    for (int a = 0; a < 3; ++a) {
        if (c->skip_box[3 + a] < 0) {  // (no active brick: every ray misses)
            c->abox[a] = 3.0e38f;
            c->abox[3 + a] = -3.0e38f;
        } else {
            c->abox[a] = (float)(((double)c->skip_box[a] - 1.0 + (double)kBrickHalf) / (double)bs[a]);
            c->abox[3 + a] = (float)(((double)c->skip_box[3 + a] + 2.0 + (double)kBrickHalf) / (double)bs[a]);
        }
    }
    c->skip_pending = false;
}

// Grows a generation to `bytes`.  `drain`: nothing is in flight, the old buffer is freed; otherwise it waits for the next draining call.
int grow(vr_ctx* c, void** d, size_t* cap, size_t bytes, bool drain)
{
    if (bytes <= *cap) return VR_OK;
    if (*d) {
        if (drain) (void)hipFree(*d);
        else c->retired_dev.push_back(*d);
    }
    *d = nullptr;
    *cap = 0;
    VR_HIP(c, hipMalloc(d, bytes));
    *cap = bytes;
    return VR_OK;
}

// The empty-space brick grid of volume slot sv in P: bricks per axis and voxels per brick edge (exact in f32).
void fill_brick_grid(MarchParams& P, int sv, const DevVolume& v)
{
    P.skip_vol = sv;
    P.bnx = skip_bricks(v.nx);
    P.bny = skip_bricks(v.ny);
    P.bnz = skip_bricks(v.nz);
    P.bsx = (float)v.nx * kBrickInv;
    P.bsy = (float)v.ny * kBrickInv;
    P.bsz = (float)v.nz * kBrickInv;
}

// Exact empty-space skipping (E.can_skip): fills P's brick fields from c, and rebuilds what is stale of the merged mask records, the
// distance field, the share of active bricks (active_fraction, which the kernel choice reads) and the box of the active bricks.
int prepare_skip(vr_ctx* c, int variant, hipStream_t s, MarchParams& P)
{
    const int sv = variant == VR_VARIANT_VOLUME_MASK ? 2 : 0;
    fill_brick_grid(P, sv, c->vol[sv]);
    P.tf_zero_prefix = c->tf_zero_prefix[0];
    P.bricks = c->vol_bricks[sv];
    P.use_rgb = 0;
    const int nb = P.bnx * P.bny * P.bnz;
    if (variant == VR_VARIANT_VOLUME_MASK) {
        if (c->merged_stale || !c->merged_bricks) {
            if (c->merged_bricks) (void)hipFree(c->merged_bricks);
            c->merged_bricks = nullptr;
            VR_HIP(c, hipMalloc(&c->merged_bricks, (size_t)nb * sizeof(float2)));
            hipLaunchKernelGGL(merge_bricks_kernel, dim3((unsigned)((nb + 255) / 256)), dim3(256), 0, s, c->vol_bricks[2],
                               c->vol_bricks[0], c->merged_bricks, nb);
            VR_HIP(c, hipGetLastError());
            c->merged_stale = false;
        }
        P.bricks = c->merged_bricks;
        P.use_rgb = 1;
    }
    // distance field over the inert bricks (Chebyshev distance to the nearest active brick), rebuilt when the
    // records, the zero prefix or the table resolution changed since it was last built (an asynchronous opacity edit rebuilds it
    // on its own stream for the records it was built from: vr_tf_upload_opacity_async)
    const float bs[3] = {P.bsx, P.bsy, P.bsz};
    if (c->dist_records != (const void*)P.bricks || c->dist_epoch != c->brick_epoch || c->dist_z != P.tf_zero_prefix ||
        c->dist_res != c->tf[0].res_o || c->dist_rgb != P.use_rgb || !c->brick_dist) {
        // (rare: an input changed.  Frames may be in flight on other streams and read the field: drain them first,
        // and finish the rebuild before any other stream's launch can follow)
        VR_HIP(c, hipDeviceSynchronize());
        drained(c);
        GenBuf& g = c->field[c->field_cur];
        c->brick_dist = nullptr;
        if (const int rc = grow(c, &g.d, &g.cap, (size_t)nb, true)) return rc;
        if (const int rc = grow(c, (void**)&c->dist_tmp, &c->tmp_cap, (size_t)nb, true)) return rc;
        const int bn[3] = {P.bnx, P.bny, P.bnz};
        if (const int rc = build_field(c, s, P.bricks, bn, P.use_rgb, P.tf_zero_prefix, c->tf[0].res_o, (unsigned char*)g.d, c->field_cur,
                                       ++c->skip_gen))
            return rc;
        VR_HIP(c, hipStreamSynchronize(s));
        g.written();
        c->brick_dist = (unsigned char*)g.d;
        c->skip_pending = true;
        for (int a = 0; a < 3; ++a) c->dist_bn[a] = bn[a];
        c->dist_records = (const void*)P.bricks;
        c->dist_epoch = c->brick_epoch;
        c->dist_z = P.tf_zero_prefix;
        c->dist_res = c->tf[0].res_o;
        c->dist_rgb = P.use_rgb;
    }
    adopt_skip(c, bs);
    P.brick_dist = c->brick_dist;
    if (c->skip_pending) {
        // (the count and box of an asynchronous rebuild are on their way: the unbounded box -- the kernels only prune with it -- and
        // the last share of active bricks)
        const float unbounded[6] = {-3.0e38f, -3.0e38f, -3.0e38f, 3.0e38f, 3.0e38f, 3.0e38f};
        for (int a = 0; a < 6; ++a) P.abox[a] = unbounded[a];
    } else {
        for (int a = 0; a < 6; ++a) P.abox[a] = c->abox[a];
    }
    return VR_OK;
}

// The range records of volume slot `slot` (bn bricks per axis): (re)builds them and the whole volume's range on `s` when a volume
// changed since they were built (no host wait), and orders a launch on another stream behind that build once.  *rec = the records,
// the return value the whole volume's range (both device), or nullptr after a failure (c->err says why).
const float2* prepare_range(vr_ctx* c, hipStream_t s, int slot, int bnx, int bny, int bnz, const float2** rec)
{
    const DevVolume& v = c->vol[slot];
    const size_t nb = (size_t)bnx * bny * bnz;
    BuiltOn& built = c->proj_built[slot];
    if (c->proj_epoch[slot] != c->brick_epoch || !c->proj_rec[slot] || !c->proj_range[slot]) {
        // (a volume change drained the device: nothing in flight reads the records; a smaller buffer is retired all the same)
        if (grow(c, (void**)&c->proj_rec[slot], &c->proj_rec_cap[slot], nb * sizeof(float2), false)) return nullptr;
        if (!c->proj_range[slot] && hipMalloc(&c->proj_range[slot], sizeof(float2)) != hipSuccess) {
            c->proj_range[slot] = nullptr;
            fail(c, VR_ERR_OOM, "vr_render: no memory for the projection's volume range");
            return nullptr;
        }
        if (!built.ev && hipEventCreateWithFlags(&built.ev, hipEventDisableTiming) != hipSuccess) {
            built.ev = nullptr;
            fail(c, VR_ERR_HIP, "vr_render: hipEventCreateWithFlags failed");
            return nullptr;
        }
        hipLaunchKernelGGL(brick_range_kernel, dim3((unsigned)nb), dim3(64), 0, s, v.data, v.nx, v.ny, v.nz, bnx, bny, c->proj_rec[slot]);
        hipLaunchKernelGGL(range_reduce_kernel, dim3(1), dim3(1024), 0, s, (const float2*)c->proj_rec[slot], (int)nb, c->proj_range[slot]);
        if (hipGetLastError() != hipSuccess || hipEventRecord(built.ev, s) != hipSuccess) {
            fail(c, VR_ERR_HIP, "vr_render: the projection's brick ranges could not be enqueued");
            return nullptr;
        }
        c->proj_epoch[slot] = c->brick_epoch;
        built.built(s);
    } else if (built.order_behind(s) != hipSuccess) {
        fail(c, VR_ERR_HIP, "vr_render: hipStreamWaitEvent failed");
        return nullptr;
    }
    *rec = c->proj_rec[slot];
    return c->proj_range[slot];
}

// The skipping projection (flavour 19) and isosurface (21): fills P's brick fields with volume 0's range records (prepare_range).
const float2* prepare_proj(vr_ctx* c, hipStream_t s, MarchParams& P)
{
    fill_brick_grid(P, 0, c->vol[0]);
    return prepare_range(c, s, 0, P.bnx, P.bny, P.bnz, &P.bricks);
}

// Shadows (vr_set_shadows): the key of the light volume a LIGHT frame with uniforms u reads, and the light volume's grid (texels per axis).
vr_ctx::ShadowKey shadow_key(const vr_ctx* c, const vr_uniforms& u)
{
    vr_ctx::ShadowKey k;
    k.epoch = c->brick_epoch;
    k.opacity = c->opacity_edits;
    // (the clip bounds as fill_frame_params computes them)
    const float box[6] = {0.0f + u.clip_x[0], 0.0f + u.clip_y[0], 0.0f + u.clip_z[0], 1.0f - u.clip_x[1], 1.0f - u.clip_y[1], 1.0f - u.clip_z[1]};
    std::memcpy(k.light, u.light_pos, sizeof k.light);
    std::memcpy(k.box, box, sizeof k.box);
    std::memcpy(&k.sigma, &c->shadow_sigma, sizeof k.sigma);
    k.div = c->shadow_div;
    k.arith = c->arith;
    return k;
}

size_t shadow_grid(const vr_ctx* c, int g[3])
{
    const int n[3] = {c->vol[0].nx, c->vol[0].ny, c->vol[0].nz};
    for (int a = 0; a < 3; ++a) g[a] = (n[a] + c->shadow_div - 1) / c->shadow_div;
    return (size_t)g[0] * g[1] * g[2];
}

// The light volume of a shadowed LIGHT launch on `s` whose parameters are P (volume 0, TF slot 0, the clip box and the light of its first
// frame; with `skip` LIGHT's distance field in P.brick_dist): the ring's entry of that key, built on `s` into the least recently used
// entry if there is none -- behind every launch that still reads that entry and behind its own last build -- or waited for once on a
// stream other than its build's.  Binds it as P.vol[1] and makes it the entry the launch reads (shadow_cur).  An allocation failure
// returns before anything is enqueued.
int prepare_shadow(vr_ctx* c, hipStream_t s, MarchParams& P, const vr_ctx::ShadowKey& key, bool skip, bool off32)
{
    int g[3];
    const size_t texels = shadow_grid(c, g);
    int e = -1;
    for (int i = 0; i < kShadowRing; ++i)
        if (c->shadow[i].valid && c->shadow[i].key == key) e = i;
    bool build = e < 0;
    if (build) {
        e = 0;
        for (int i = 1; i < kShadowRing; ++i)
            if (c->shadow[i].used < c->shadow[e].used) e = i;
    }
    vr_ctx::ShadowVol& v = c->shadow[e];
    if (build) {
        v.valid = false;
        const bool fresh = texels * sizeof(float) > v.buf.cap;
        // (a smaller buffer may still be read by launches in flight: it is retired, freed by the next draining call)
        if (const int rc = grow(c, &v.buf.d, &v.buf.cap, texels * sizeof(float), false)) return rc;
        if (!v.built.ev) VR_HIP(c, hipEventCreateWithFlags(&v.built.ev, hipEventDisableTiming));
        if (!fresh) {
            if (const int rc = reuse_wait(c, s, v.buf)) return rc;
            if (v.built.pending && v.built.stream != s) VR_HIP(c, hipStreamWaitEvent(s, v.built.ev, 0));
        }
    }
    DevVolume& lv = P.vol[1];
    lv = DevVolume{};
    lv.data = nullptr;
    lv.dens = (const float*)v.buf.d;
    lv.a_base = (const char*)v.buf.d;
    lv.a_shift = 2;
    lv.nx = g[0];
    lv.ny = g[1];
    lv.nz = g[2];
    lv.bricked = 0;
    lv.lut = 0;
    lv.data_bytes = (unsigned)(texels * sizeof(float));
    if (build) {
        if (c->arith == VR_ARITH_FUSED) vrf::launch_shadow_build(P, (float*)v.buf.d, c->shadow_sigma, skip, off32, s);
        else vr::launch_shadow_build(P, (float*)v.buf.d, c->shadow_sigma, skip, off32, s);
        VR_HIP(c, hipGetLastError());
        VR_HIP(c, hipEventRecord(v.built.ev, s));
        v.buf.written();
        v.key = key;
        v.valid = true;
        v.built.built(s);
    } else {
        VR_HIP(c, v.built.order_behind(s));
    }
    v.used = ++c->shadow_clock;
    c->shadow_cur = e;
    return VR_OK;
}

// The kernel form ("flavour") a launch runs: `fl` is the one asked for (vr_set_kernel_flavour, else VR_EXP_FLAVOUR), 0 = the default.
int choose_flavour(vr_ctx* c, int fl, int variant, int n_frames, int rank, int world, bool packed, const Eligibility& E, bool surface,
                   bool bounded)
{
    // The one-lane families come in pairs: 1 asks for the form without skipping (the odd flavour + 1), everything else runs as the
    // skipping one; nothing is measured.  The first row that applies decides (the isosurface's surface output keeps 21 / 22).
    const struct {
        bool applies;
        int skipping;
    } pairs[] = {
        {bounded, 27},                                            // the unlit / lit shader between ray bounds
        {surface && variant != VR_VARIANT_ISO, 25},               // the surface-position output of the unlit / lit shader
        {is_projection(variant), 19},                             // the projections
        {variant == VR_VARIANT_ISO, 21},                          // the isosurface
        {variant == VR_VARIANT_LIGHT && c->shadow_div != 0, 23},  // the shadowed lit shader
    };
    for (const auto& pr : pairs)
        if (pr.applies) return fl == 1 ? pr.skipping + 1 : pr.skipping;
    const bool auto_choice = fl == 0;
    const double rays = rays_per_lane(c, rank, world, c->frames_in_flight * n_frames);
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
    if ((fl == 12 || fl == 13) && n_frames != 1) fl = 6;
    if ((fl == 16 || fl == 17) && !E.p2_ok) fl = n_frames != 1 ? 6 : (fl == 16 ? 13 : 12);
    if (fl == 18 && !E.lut_ok) fl = 6;
    if (fl == 16 && variant == VR_VARIANT_VOLUME_MASK) fl = 17;  // (the composite's form is the skipping one: its mask records)
    // LDS tiles (15; vr_lt.h): the lit shader, launches of one frame
    if (fl == 15 && (n_frames != 1 || variant != VR_VARIANT_LIGHT)) fl = 6;
    // the illustrative shader's opacity reads the accumulated alpha: its steps cannot be sampled side by side
    if (variant == VR_VARIANT_ILLUSTRATIVE && (fl == 7 || fl == 8 || fl == 10 || fl == 11)) fl = 6;
    // the in-shader gradient variant (seven density fetches per sample) exists as the one-lane kernel only
    if (variant == VR_VARIANT_LIGHT_INSHADER && fl != 1 && fl != 12 && fl != 13 && fl != 18) fl = 6;
    if ((fl == 16 || fl == 17) && variant == VR_VARIANT_VOLUME_MASK && !E.can_skip)  // (no brick records: no on-demand mask fetch)
        fl = n_frames != 1 ? 6 : 12;
    if (!auto_choice) return fl;

    // Default choice, second part -- THE PRIOR: what runs before anything has been measured.  Whole frames of the lit / unlit shader
    // and of the composite, one launch at a time: the kernel with the corner loads two steps ahead (vr_p2.h) -- 17, or 16 where next to
    // nothing can be skipped (noisy air under the default ramp 2.95 -> 1.97 ms; C3 0.65 -> 0.51; C4 0.72 -> 0.57) -- unless an earlier
    // launch of this shape says its chains are short (C2, longest chain 102: a packet is too short for the pipeline's fill and a
    // dequeue, 0.111 -> 0.161).  The same with launches in flight and several frames per launch since the approach loop (C3 0.417 / 0.382
    // ms per frame against march_kernel's 0.464 / 0.445; C5 level); shares of a frame: the first part's choice.
    const bool p2_variant = variant == VR_VARIANT_LIGHT || variant == VR_VARIANT_BASIC || (variant == VR_VARIANT_VOLUME_MASK && E.can_skip);
    const bool nothing_to_skip = !E.can_skip || c->active_fraction >= 0.9;  // (prepare_skip has measured the share of active bricks)
    if (fl == 6 && E.whole_frame && E.p2_ok && p2_variant) {
        if (nothing_to_skip && variant != VR_VARIANT_VOLUME_MASK) fl = 16;
        else if (!short_chains) fl = 17;
    }
    if (!c->tune_mode) return fl;
    // ... and THE MEASURED CHOICE (tune_pick): the eligible forms take turns on the caller's own frames, the fastest by the launches'
    // own records stays.  Candidates: the prior; the two-steps-ahead kernel; the one-lane kernel; the depth-parallel kernel (launches
    // that leave the machine part empty) or the persistent kernel without the pipeline (the longest chains).
    int cand[6], n = 0;
    auto add = [&](int f) {
        for (int i = 0; i < n; ++i)
            if (cand[i] == f) return;
        if (n < 6) cand[n++] = f;
    };
    add(fl);
    if (E.p2_ok && p2_variant) add((nothing_to_skip && variant != VR_VARIANT_VOLUME_MASK) || !E.can_skip ? 16 : 17);
    add(6);
    if (E.lut_ok && E.lut_lds <= 8u * 1024u) add(18);  // (the one-lane kernel with its slot arithmetic from LDS tables; larger tables cost it wavefronts per CU: C5 4.2 vs 3.4 ms)
    const bool dp_variant = variant != VR_VARIANT_ILLUSTRATIVE && variant != VR_VARIANT_LIGHT_INSHADER;
    if (!E.whole_frame && dp_variant) add(rays >= 2.0 ? 11 : 10);
    else if (n_frames == 1 && (variant == VR_VARIANT_LIGHT || variant == VR_VARIANT_BASIC)) add(12);
    const unsigned long long shape = 0x9E3779B97F4A7C15ull * (((unsigned long long)variant << 56) ^ ((unsigned long long)world << 48) ^ ((unsigned long long)rank << 40) ^
                                                             ((unsigned long long)c->W << 24) ^ ((unsigned long long)c->H << 8) ^ (packed ? 0x80ull : 0ull) ^
                                                             ((unsigned long long)n_frames << 4) ^ (unsigned long long)c->frames_in_flight) | 1ull;
    const unsigned long long key = (shape ^ (c->brick_epoch * 0xD6E8FEB86659FD93ull) ^ (c->tf_epoch << 20) ^ ((unsigned long long)c->arith << 1) ^
                                    ((unsigned long long)c->layout_mode << 2)) | 1ull;
    const bool measurable = c->h_span && c->h_end && !c->event_timing;
    return tune_pick(c, key, shape, cand, n, E.chain_known, measurable);
}

// What each flavour launches -- the one place a flavour's number is decoded.
struct KernelForm {
    LaunchDesc::Family family;
    int lanes;            // kDp: lanes per ray (vr_dp.h): 64 / 32 workgroups per tile
    bool pipe;            // kDp / kPw: the next round's / step's corner loads software-pipelined
    bool skip;            // the skipping flavour of a pair (17 of 16 / 17; 19, 21, 23, 25, 27 of the one-lane families): LaunchDesc::skip once
                          // its records are in place
    bool lut;             // kPlain: the slot tables of volume 0 in LDS
    unsigned pw_threads;  // kPw / kP2: threads per workgroup
    // what follows from the family
    bool range_records() const { return family == LaunchDesc::kProj || family == LaunchDesc::kIso; }  // skips by prepare_proj's records
    bool measured() const  // a candidate of the measured choice (the one-lane families never are)
    {
        return !(range_records() || family == LaunchDesc::kShadow || family == LaunchDesc::kSurf || family == LaunchDesc::kBound);
    }
};

KernelForm kernel_form(int fl, int variant)
{
    // (march_p2_kernel: two corner buffers, 3 wavefronts per SIMD at most; with every ray sampling all the time two per SIMD are faster
    // -- the corner data in flight is many times the L1 either way: noisy air 2.13 -> 2.04 ms.  The unlit shader's two buffers are 4-byte
    // densities, 101 VGPRs: 4 wavefronts per SIMD -- C2 one frame at a time 0.121 -> 0.113 ms, thin table 0.255 -> 0.239, four frames per
    // launch 0.070 -> 0.061: tools/experiments/s2h.sh.  Launches in flight: the same shape.  Two workgroups of 6 wavefronts do not share
    // a CU -- the second one's wavefronts would have to go 1-1-2-2 over the SIMDs where the dispatcher deals 2-2-1-1: measured 0.75 ms
    // per C3 frame, what one such workgroup per CU takes -- and two of 4 run at 8 wavefronts per CU: 0.63 against 0.54; three of 4, the
    // same 12 wavefronts per CU, take 0.79 ms one frame at a time and 0.62 in flight against 0.55 / 0.51: profiles/r04_p2_launch_shapes.txt)
    using D = LaunchDesc;
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

// The record slot of the next launch, *cb = order_seq % kInFlight.  (Record slot and order slot both derive from order_seq, which
// advances only once a launch has really been enqueued: a failed enqueue cannot shift one against the other.)  The slot's previous
// launch (kInFlight launches ago, possibly on another stream) must have finished before its record buffer is written again or
// re-allocated: this is what bounds the launches in flight to kInFlight.  *slot_sort: the sort that read those records, which the
// launch's stream has yet to wait for (wait_for_order); waited for at once only when the buffer is re-allocated (the memset behind
// the allocation writes it).
int take_record_slot(vr_ctx* c, hipStream_t s, size_t n_records, int* cb, const vr_ctx::OrderSlot** slot_sort)
{
    const int k = (int)(c->order_seq % (unsigned long long)kInFlight);
    *cb = k;
    if (c->slot_used[k]) VR_HIP(c, hipEventSynchronize(c->slot_done[k]));
    *slot_sort = nullptr;
    if (c->order_seq >= (unsigned long long)kInFlight) {
        const vr_ctx::OrderSlot& po = c->order_ring[(c->order_seq - kInFlight) % kOrderRing];
        if (po.valid && po.seq + kInFlight == c->order_seq) *slot_sort = &po;
    }
    if (n_records > c->block_counts_cap[k]) {
        if (*slot_sort) VR_HIP(c, hipStreamWaitEvent(s, (*slot_sort)->sorted, 0));
        *slot_sort = nullptr;
        if (c->d_block_counts[k]) (void)hipFree(c->d_block_counts[k]);
        c->d_block_counts[k] = nullptr;
        c->block_counts_cap[k] = 0;
        VR_HIP(c, hipMalloc(&c->d_block_counts[k], n_records * kBlockRecord * sizeof(unsigned long long)));
        VR_HIP(c, hipMemsetAsync(c->d_block_counts[k], 0, n_records * kBlockRecord * sizeof(unsigned long long), s));
        c->block_counts_cap[k] = n_records;
    }
    return VR_OK;
}

// The launch order an ordered launch takes (*order; nullptr = index order) and the one wait for a sort it implies.  The order: the most
// recent sort of a launch of the same shape (okey) that is three or four launches old (two or three more than the frames the caller
// says it keeps in flight, if that is more: with short frames -- C2, 0.08 ms -- the sort of the launch that finished one frame time ago
// is itself only just finishing) -- a younger one may still be waiting for its launch to finish (the sorts run on a side stream behind
// their launches; waiting for one would put a bubble into this stream, and with four frames in flight it would chain this launch behind
// the one three before it), an older one's buffer may be recycled under this launch; ordered behind it by its event (long complete by
// then).  A stream's wait for another stream's event costs the stream 5 us per launch even when the event completed long ago
// (tools/ubench/stream_gap.hip), so the wait for `slot_sort` is left out when the order's wait covers it: every sort runs on the one
// order stream, in the order of the launches.
int wait_for_order(vr_ctx* c, hipStream_t s, bool ordered, unsigned long long okey, const vr_ctx::OrderSlot* slot_sort, const unsigned** order)
{
    *order = nullptr;
    if (ordered) {
        const vr_ctx::OrderSlot* best = nullptr;
        const unsigned long long age = (unsigned long long)(c->frames_in_flight + 2 > 3 ? c->frames_in_flight + 2 : 3);
        for (const auto& o : c->order_ring)
            if (o.valid && o.key == okey && o.seq + age + 1 >= c->order_seq && o.seq + age <= c->order_seq && (!best || o.seq > best->seq))
                best = &o;
        if (best) {
            VR_HIP(c, hipStreamWaitEvent(s, best->sorted, 0));
            if (slot_sort && best->seq >= slot_sort->seq) slot_sort = nullptr;  // (covered: the order stream runs its sorts in order)
            *order = best->buf;
        }
    }
    if (slot_sort) VR_HIP(c, hipStreamWaitEvent(s, slot_sort->sorted, 0));
    return VR_OK;
}

// Behind the launch in record slot cb: the slot's event and, for an ordered launch, the sort of its n_blocks records on the order stream
// into order slot order_seq % kOrderRing -- the launch order of later launches; the longest chain (h_chain), and unless the launch is
// timed with events its span and end (h_span / h_end, ring slot `ring`); the persistent kernels' queue heads cleared.  Then the next
// launch takes the next slots.
int enqueue_sort(vr_ctx* c, hipStream_t s, int cb, bool ordered, unsigned long long okey, unsigned long long skey, unsigned n_blocks, int ring,
                 bool time_with_events, bool pw)
{
    vr_ctx::OrderSlot& o = c->order_ring[c->order_seq % kOrderRing];
    if (ordered) {
        o.valid = false;
        if (n_blocks > o.cap) {
            if (o.buf) (void)hipFree(o.buf);
            o.buf = nullptr;
            o.cap = 0;
            VR_HIP(c, hipMalloc(&o.buf, (size_t)n_blocks * sizeof(unsigned)));
            o.cap = n_blocks;
        }
        o.stream = s;
        o.key = okey;
        o.scene_key = skey;
        o.seq = c->order_seq;
        if (c->h_chain) c->h_chain[c->order_seq % kOrderRing] = 0;  // not known until this launch's sort has run
    }
    VR_HIP(c, hipEventRecord(c->slot_done[cb], s));
    c->slot_used[cb] = true;
    if (ordered) {
        VR_HIP(c, hipStreamWaitEvent(c->order_stream, c->slot_done[cb], 0));
        hipLaunchKernelGGL(order_blocks_kernel, dim3(1), dim3(1024), 0, c->order_stream, c->d_block_counts[cb], (int)n_blocks, o.buf,
                           c->h_chain ? c->h_chain + (c->order_seq % kOrderRing) : (unsigned*)nullptr,
                           (c->h_span && !time_with_events) ? c->h_span + ring : (unsigned long long*)nullptr,
                           pw ? c->d_pw_heads + (size_t)cb * 8 * 64 : (unsigned*)nullptr,
                           (c->h_span && c->h_end && !time_with_events) ? c->h_end + ring : (unsigned long long*)nullptr);
        VR_HIP(c, hipGetLastError());
        if (pw) c->pw_heads_dirty[cb] = false;  // (the sort zeroes the heads behind the launch: the slot's next user finds them clean)
        VR_HIP(c, hipEventRecord(o.sorted, c->order_stream));
        o.valid = true;
    }
    ++c->order_seq;
    return VR_OK;
}

// The launch's frames (frame f: every n_frames-th group of 8 workgroups, MarchBatch), each with its own uniforms, output and records;
// the launch order (a heuristic of the shape) is shared.
const MarchBatch& fill_batch(MarchParams& P, int n_frames, const vr_uniforms* batch_u, void* const* batch_out, unsigned blocks_per_frame)
{
    static thread_local MarchBatch B;
    P.batch_n = (unsigned)n_frames;
    B.frame[0] = P;
    for (int f = 1; f < n_frames; ++f) {
        MarchParams& Pf = B.frame[f];
        Pf = P;
        fill_frame_params(Pf, batch_u[f]);
        Pf.out = (float4*)batch_out[f];
        Pf.block_counts = P.block_counts + (size_t)f * blocks_per_frame * kBlockRecord;
    }
    B.n_frames = (unsigned)n_frames;
    return B;
}

// Enqueue one launch on `s`: ONE frame with the context's uniforms into `out` (nullptr -> ctx-owned buffer), or, with
// batch_u / batch_out, n_frames (2 .. kBatchMax) frames of the same scene, each with its own uniforms and output buffer.
int enqueue_render(vr_ctx* c, int variant, int rank, int world, bool packed, float4* out, hipStream_t s, bool frame_events,
                   int n_frames = 1, const vr_uniforms* batch_u = nullptr, void* const* batch_out = nullptr)
{
    int nvol;
    bool off32;
    // surface-position output (vr_set_output; a pick launch whatever the setting): the unlit / lit shader and the isosurface -- any
    // other variant is refused whatever the scene holds
    const bool surface = c->output == VR_OUTPUT_SURFACE || c->pick_px[0] >= 0;
    if (surface && variant >= 0 && variant < VR_VARIANT_COUNT && variant != VR_VARIANT_BASIC && variant != VR_VARIANT_LIGHT &&
        variant != VR_VARIANT_ISO)
        return fail(c, VR_ERR_UNSUPPORTED, "vr_render: surface output exists for BASIC, LIGHT and ISO only");
    // ray bounds (vr_set_ray_bounds; a pick launch ignores them): colour launches of one frame of the unlit shader and of the lit one
    // without shadows -- anything else is refused, never rendered with the occluder ignored
    const bool bounded = (c->d_near || c->d_far) && c->pick_px[0] < 0;
    if (bounded && variant >= 0 && variant < VR_VARIANT_COUNT) {
        if (variant != VR_VARIANT_BASIC && variant != VR_VARIANT_LIGHT)
            return fail(c, VR_ERR_UNSUPPORTED, "vr_render: ray bounds exist for BASIC and LIGHT only");
        if (surface) return fail(c, VR_ERR_UNSUPPORTED, "vr_render: ray bounds do not apply to surface output");
        if (variant == VR_VARIANT_LIGHT && c->shadow_div != 0)
            return fail(c, VR_ERR_UNSUPPORTED, "vr_render: ray bounds do not apply to LIGHT with shadows on");
        if (batch_u) return fail(c, VR_ERR_UNSUPPORTED, "vr_render: ray bounds do not apply to launches of several frames");
    }
    if (const int rc = check_render_args(c, variant, rank, world, n_frames, batch_u, batch_out, &nvol, &off32)) return rc;
    // shadows: every frame of the launch reads one light volume, of less than 4 GiB (a surface launch reads none)
    const bool shadowed = variant == VR_VARIANT_LIGHT && c->shadow_div != 0 && !surface;
    vr_ctx::ShadowKey shadow_k;
    if (shadowed) {
        shadow_k = shadow_key(c, batch_u ? batch_u[0] : c->u);
        for (int f = 1; f < n_frames; ++f)
            if (!(shadow_key(c, batch_u[f]) == shadow_k))
                return fail(c, VR_ERR_UNSUPPORTED, "vr_render: the frames of a shadowed batch must share the light and the clip box");
        int g[3];
        if (shadow_grid(c, g) * sizeof(float) >= (1ull << 32))
            return fail(c, VR_ERR_UNSUPPORTED, "vr_render: the light volume would take 4 GiB or more (a larger divisor)");
    }
    c->shadow_cur = -1;
    if (batch_u) out = (float4*)batch_out[0];
    VR_HIP(c, hipSetDevice(c->device));
    (void)hipGetLastError();  // a stale error of somebody else's call must not be reported as a failed launch below
    if (const int rc = wait_for_edits(c, s)) return rc;

    MarchParams P;
    fill_launch_params(c, P, batch_u ? batch_u[0] : c->u, rank, world, packed);
    if (surface && variant != VR_VARIANT_ISO) P.iso = c->surf_tau;  // (these launches read no level)
    if (c->pick_px[0] >= 0)  // vr_pick: the one pixel's ray (a rectangle no larger than the one the box can be hit in)
        for (int a = 0; a < 2; ++a) {
            P.rect[a] = P.rect[a] > c->pick_px[a] ? P.rect[a] : c->pick_px[a];
            P.rect[2 + a] = P.rect[2 + a] < c->pick_px[a] ? P.rect[2 + a] : c->pick_px[a];
        }
    // the kernel choice: what can run, the skipping state (the prior reads its share of active bricks), the flavour
    const int requested = c->flavour == 0 ? c->default_flavour : c->flavour;
    Eligibility E = eligibility(c, requested, variant, n_frames, rank, world, packed, batch_u);
    if (surface && variant != VR_VARIANT_ISO) {
        // The surface march skips by the distance field of BASIC / LIGHT under the weakest condition that is still exact: an inert
        // brick's samples have opacity exactly 0, which leaves the accumulated alpha as it is whatever the colour table and the
        // light hold -- neither is read.  So: the brick records, a zero prefix of the opacity table, the kernels' index range.
        E.can_skip = requested != 1 && c->vol_bricks[0] && c->tf_zero_prefix[0] >= 0 &&
                     skip_bricks(c->vol[0].nx) * (long long)skip_bricks(c->vol[0].ny) < (1 << 23);
        E.chain_known = 0;
    }
    if (E.can_skip) {
        if (const int rc = prepare_skip(c, variant, s, P)) return rc;
        if (c->skip_pending) ++c->unbounded_launches;
    }
    const int fl = choose_flavour(c, requested, variant, n_frames, rank, world, packed, E, surface, bounded);
    c->last_flavour = fl;
    const KernelForm form = kernel_form(fl, variant);
    c->last_unmeasured = !form.measured();
    const float2* vrange = nullptr;
    if (form.skip && form.range_records()) {
        vrange = prepare_proj(c, s, P);
        if (!vrange) return VR_ERR_HIP;
    }

    if (c->layout_mode == 0) use_bricked_copies(c, P);
    if (form.lut && P.vol[0].bricked) P.vol[0].lut = 1;  // (march_kernel fills the tables; every fetch of volume 0 goes through them)
    if (form.family == LaunchDesc::kBound) {  // the depth buffers, in the slots these shaders do not sample (vr_bound.h)
        P.vol[1].data = reinterpret_cast<const float4*>(c->d_near);
        P.vol[2].data = reinterpret_cast<const float4*>(c->d_far);
    }
    for (int i = 0; i < nvol; ++i)  // (a bricked copy is padded to whole bricks: a volume just below 4 GiB may cross the line)
        if (P.vol[i].bricked && bricked_grid(P.vol[i]).slots * 16 > 0xFFFFFFFFull) off32 = false;

    if (packed && !out) {
        size_t need = (size_t)P.n_tiles * kTile * kTile;
        if (need > c->tiles_cap) {
            if (c->d_tiles) (void)hipFree(c->d_tiles);
            c->d_tiles = nullptr;
            c->tiles_cap = 0;
            VR_HIP(c, hipMalloc(&c->d_tiles, (need ? need : 1) * sizeof(float4)));
            c->tiles_cap = need;
        }
        out = c->d_tiles;
    } else if (!out) {
        out = c->d_frame;
    }
    P.out = out;
    c->last_tiles = packed ? P.n_tiles : 0;

    if (frame_events) VR_HIP(c, hipEventRecord(c->tm.ev_begin, s));
    // the skipping form of a pair runs with its records in place -- the projections' range records, else the distance field -- and
    // as the pair's other kernels without them
    const bool skip = form.skip && (form.range_records() ? vrange != nullptr : P.brick_dist != nullptr);
    if (P.n_blocks > 0) {
        // the light volume it reads: built here when its key has none (inside vr_last_timing's total, outside its kernel time)
        if (shadowed)
            if (const int rc = prepare_shadow(c, s, P, shadow_k, skip, off32)) return rc;
        // the LOGICAL blocks (records, launch order): one wavefront per workgroup (launch order at wavefront granularity) -- except
        // for the depth-parallel kernels on large launches, where 4x the workgroups cost more at dispatch than the finer order gains
        // (C2: 32 768 workgroups of a 0.12 ms frame).  See map_pixel / map_pixel_dp.
        const int dp = form.family == LaunchDesc::kDp ? form.lanes : 0, wpb = dp && P.n_tiles * dp * 64 > 16384 ? 4 : 1;
        const dim3 block((unsigned)(64 * wpb));
        const dim3 grid((unsigned)(dp ? P.n_tiles * dp * 64 / wpb : (P.n_tiles + 7) / 8 * 8 * (64 / wpb)));
        if (n_frames > 1 && grid.x % 8u != 0) return fail(c, VR_ERR_INVALID_ARG, "vr_render: launch shape cannot carry several frames");
        const bool pw = form.family == LaunchDesc::kPw || form.family == LaunchDesc::kP2;
        // the ring slots: record buffer, then the launch order and the sort waits (a launch order is kept per launch shape -- not per
        // flavour: the kernels that march one packet per wavefront -- 6, 12, 13, 16, 17 -- share the logical blocks, so an order sorted
        // behind one of them serves the others, and the measured choice tries them in turn on a live scene)
        int cb;
        const vr_ctx::OrderSlot* slot_sort;
        if (const int rc = take_record_slot(c, s, (size_t)grid.x * (size_t)n_frames, &cb, &slot_sort)) return rc;
        P.block_counts = c->d_block_counts[cb];
        c->cnt_buf = cb;
        const unsigned long long okey = ((unsigned long long)grid.x << 32) ^ ((unsigned long long)block.x << 20) ^
                                        ((unsigned long long)(variant | (surface ? 0x10 : 0) | (bounded ? 0x20 : 0)) << 16) ^ ((unsigned long long)world << 8) ^
                                        (unsigned long long)rank ^ (packed ? 1ull << 63 : 0ull);
        const bool ordered = grid.x <= (unsigned)kOrderMaxBlocks && grid.x % 8u == 0;
        if (const int rc = wait_for_order(c, s, ordered, okey, slot_sort, &P.order)) return rc;

        const int ring = (int)(c->ring.head % kRing);
        if (frame_events) VR_HIP(c, hipEventRecord(c->tm.ev_k0, s));
        // launches with a sort behind them are timed from their own records (order_blocks_kernel); events only otherwise
        const bool time_with_events = !(ordered && c->h_span) || c->event_timing;
        c->ring_events[ring] = time_with_events;
        if (c->h_span) c->h_span[ring] = 0;
        if (c->h_end) c->h_end[ring] = 0;
        if (time_with_events) VR_HIP(c, hipEventRecord(c->ring.k0[ring], s));
        const MarchBatch& B = fill_batch(P, n_frames, batch_u, batch_out, grid.x);
        LaunchDesc L = {};
        L.variant = variant;
        L.family = form.family;
        L.off32 = off32;
        L.lanes = form.lanes;
        L.pipe = form.pipe;
        L.lds_bytes = P.vol[0].lut ? E.lut_lds : 0u;
        L.grid = dim3(grid.x * (unsigned)n_frames);
        L.block = block;
        L.vrange = vrange;
        L.skip = skip;
        L.surface = surface;
        if (pw) {
            // persistent wavefronts: `grid` stays the number of LOGICAL blocks (records, launch order); the launch itself is one
            // workgroup of form.pw_threads per CU (fewer when there are fewer packets), TF slot 0 in LDS when it fits
            const bool p2 = form.family == LaunchDesc::kP2;
            const unsigned per_wg = form.pw_threads / 64u, wgs = (grid.x * (unsigned)n_frames + per_wg - 1u) / per_wg;
            L.ltf = tf0_fits_lds(c);
            L.p2_win = p2 && (!off32 || c->p2_window != 0);
            L.lds_bytes = p2 ? E.p2_lds : (L.ltf ? (unsigned)(c->tf[0].res_o + 2) * 16u : 0u);
            L.queue = PwQueue{c->d_pw_heads + (size_t)cb * 8 * 64, grid.x, c->p2_window};
            L.grid = dim3(wgs < (unsigned)c->n_cus ? wgs : (unsigned)c->n_cus);
            L.block = dim3(form.pw_threads);
            if (c->pw_heads_dirty[cb]) VR_HIP(c, hipMemsetAsync(L.queue.heads, 0, 8 * 64 * sizeof(unsigned), s));
            c->pw_heads_dirty[cb] = true;  // (until the sort that clears them behind this launch has really been enqueued)
        }
        if (c->arith == VR_ARITH_FUSED) vrf::launch_march(L, s, B);
        else vr::launch_march(L, s, B);
        VR_HIP(c, hipGetLastError());
        mark_reads(c, P);
        if (time_with_events) VR_HIP(c, hipEventRecord(c->ring.k1[ring], s));

        if (const int rc = enqueue_sort(c, s, cb, ordered, okey, scene_key(c, variant, rank, world, packed, surface, bounded), grid.x, ring, time_with_events, pw))
            return rc;
        if (frame_events) VR_HIP(c, hipEventRecord(c->tm.ev_k1, s));
        ++c->ring.head;
        c->cnt_blocks = (int)grid.x;
        c->cnt_offset = (size_t)(n_frames - 1) * grid.x * kBlockRecord;  // vr_last_counters: the LAST frame of the launch
    } else {
        c->cnt_blocks = 0;
        c->cnt_offset = 0;
        if (frame_events) {
            VR_HIP(c, hipEventRecord(c->tm.ev_k0, s));
            VR_HIP(c, hipEventRecord(c->tm.ev_k1, s));
        }
    }
    // the per-block counts are summed and copied to the host when somebody asks for them (fetch_counters)
    c->cnt_pending = true;
    if (frame_events) VR_HIP(c, hipEventRecord(c->tm.ev_end, s));
    c->tm.valid = frame_events;
    return VR_OK;
}

// Sums the per-block counts of the last launch into h_counters (blocks until that launch has finished).
int fetch_counters(vr_ctx* c)
{
    if (!c->cnt_pending) return VR_OK;
    VR_HIP(c, hipSetDevice(c->device));
    (void)hipGetLastError();
    if (c->cnt_blocks > 0) {
        // the launch may have been enqueued on a stream of the caller's that no longer exists: wait for the event recorded
        // behind it (owned by the context; other launches in flight are not waited for), then use the context's own stream
        VR_HIP(c, hipEventSynchronize(c->slot_done[c->cnt_buf]));
        hipLaunchKernelGGL(sum_block_counts_kernel, dim3(1), dim3(256), 0, c->stream, c->d_block_counts[c->cnt_buf] + c->cnt_offset,
                           c->cnt_blocks, c->d_counters);
        VR_HIP(c, hipGetLastError());
        VR_HIP(c, hipMemcpyAsync(c->h_counters, c->d_counters, 3 * sizeof(unsigned long long), hipMemcpyDeviceToHost,
                                 c->stream));
        VR_HIP(c, hipStreamSynchronize(c->stream));
    } else {
        c->h_counters[0] = c->h_counters[1] = c->h_counters[2] = 0;
    }
    c->cnt_pending = false;
    return VR_OK;
}

// per-brick density / rgb maxima for the exact empty-space test (one pass over the volume; after every change)
int refresh_bricks(vr_ctx* c, int slot)
{
    (void)hipGetLastError();  // (see enqueue_render)
    const DevVolume& v = c->vol[slot];
    if (c->vol_bricks[slot]) (void)hipFree(c->vol_bricks[slot]);
    c->vol_bricks[slot] = nullptr;
    c->merged_stale = true;
    ++c->brick_epoch;
    for (auto& e : c->shadow) e.valid = false;  // (the caller drained the device)
    const int bnx = skip_bricks(v.nx), bny = skip_bricks(v.ny), bnz = skip_bricks(v.nz);
    const size_t nbricks = (size_t)bnx * bny * bnz;
    VR_HIP(c, hipMalloc(&c->vol_bricks[slot], nbricks * sizeof(float2)));
    hipLaunchKernelGGL(brick_max_kernel, dim3((unsigned)nbricks), dim3(64), 0, c->stream, v.data, v.nx, v.ny, v.nz, bnx, bny,
                       c->vol_bricks[slot]);
    VR_HIP(c, hipGetLastError());
    // scalar density plane + "is .rgb the central difference of .a?" (vr_volume_layout bit 2)
    const size_t n = (size_t)v.nx * v.ny * v.nz;
    c->vol_grad_derived[slot] = false;
    if (n > c->vol_dens_cap[slot]) {
        if (c->vol_dens[slot]) (void)hipFree(c->vol_dens[slot]);
        c->vol_dens[slot] = nullptr;
        c->vol_dens_cap[slot] = 0;
        VR_HIP(c, hipMalloc(&c->vol_dens[slot], n * sizeof(float)));
        c->vol_dens_cap[slot] = n;
    }
    hipLaunchKernelGGL(extract_density_kernel, dim3(4096), dim3(256), 0, c->stream, v.data, c->vol_dens[slot], n);
    VR_HIP(c, hipGetLastError());
    unsigned* d_flag = reinterpret_cast<unsigned*>(c->d_counters);
    VR_HIP(c, hipMemsetAsync(d_flag, 0, sizeof(unsigned), c->stream));
    hipLaunchKernelGGL(verify_gradient_kernel, dim3((unsigned)((v.nx + 255) / 256), (unsigned)v.ny, (unsigned)v.nz), dim3(256), 0,
                       c->stream, v.data, c->vol_dens[slot], v.nx, v.ny, v.nz, d_flag);
    VR_HIP(c, hipGetLastError());
    unsigned flag = 1;
    VR_HIP(c, hipMemcpyAsync(&flag, d_flag, sizeof flag, hipMemcpyDeviceToHost, c->stream));
    VR_HIP(c, hipStreamSynchronize(c->stream));
    c->vol_grad_derived[slot] = flag == 0;
    c->vol[slot].dens = c->vol_dens[slot];
    {   // the bricked copy the march kernels gather from (DevVolume::bricked)
        const BrickedGrid g = bricked_grid(v);
        const size_t slots = g.slots;
        if (slots > c->vol_bricked_cap[slot]) {
            if (c->vol_bricked[slot]) (void)hipFree(c->vol_bricked[slot]);
            if (c->vol_bdens[slot]) (void)hipFree(c->vol_bdens[slot]);
            c->vol_bricked[slot] = nullptr;
            c->vol_bdens[slot] = nullptr;
            c->vol_bricked_cap[slot] = 0;
            // (the bricked copies cost 20 B per voxel on top of the reference layout's 16 + 4: when they do not fit, the kernels gather
            // from the x-fastest arrays as with vr_set_volume_layout(3) -- slower, not an error)
            if (hipMalloc(&c->vol_bricked[slot], slots * sizeof(float4)) != hipSuccess) c->vol_bricked[slot] = nullptr;
            if (c->vol_bricked[slot] && hipMalloc(&c->vol_bdens[slot], slots * sizeof(float)) != hipSuccess) {
                (void)hipFree(c->vol_bricked[slot]);
                c->vol_bricked[slot] = nullptr;
                c->vol_bdens[slot] = nullptr;
            }
            (void)hipGetLastError();
            c->vol_bricked_cap[slot] = c->vol_bricked[slot] ? slots : 0;
        }
        if (!c->vol_bricked[slot]) {
            VR_HIP(c, hipStreamSynchronize(c->stream));
            return VR_OK;
        }
        hipLaunchKernelGGL(rebrick_kernel, dim3(8192), dim3(256), 0, c->stream, v.data, c->vol_bricked[slot], c->vol_bdens[slot], v.nx,
                           v.ny, v.nz, g.nbx, g.nby, slots);
        VR_HIP(c, hipGetLastError());
        VR_HIP(c, hipStreamSynchronize(c->stream));
    }
    return VR_OK;
}

int check_slot(vr_ctx* c, int slot, const char* who)
{
    if (!c) return VR_ERR_INVALID_ARG;
    if (slot < 0 || slot >= VR_MAX_VOLUMES) return fail(c, VR_ERR_INVALID_ARG, std::string(who) + ": bad slot");
    if (!c->vol[slot].data) return fail(c, VR_ERR_NOT_READY, std::string(who) + ": volume slot is empty");
    VR_HIP(c, hipSetDevice(c->device));
    VR_HIP(c, hipDeviceSynchronize());  // asynchronous renders on the caller's streams may still read the slot
    drained(c);
    (void)hipGetLastError();
    return VR_OK;
}

template <typename T>
int upload_raw(vr_ctx* c, int slot, const T* raw, uint16_t nx, uint16_t ny, uint16_t nz)
{
    if (!c) return VR_ERR_INVALID_ARG;
    if (slot < 0 || slot >= VR_MAX_VOLUMES) return fail(c, VR_ERR_INVALID_ARG, "vr_volume_upload_raw: bad slot");
    if (!raw) return fail(c, VR_ERR_INVALID_ARG, "vr_volume_upload_raw: data is NULL");
    if (nx == 0 || ny == 0 || nz == 0) return fail(c, VR_ERR_INVALID_ARG, "vr_volume_upload_raw: empty volume");
    const size_t n = (size_t)nx * ny * nz;
    if (n > 0xFFFFFFFFull) return fail(c, VR_ERR_INVALID_ARG, "vr_volume_upload_raw: more than 2^32 voxels");
    VR_HIP(c, hipSetDevice(c->device));
    VR_HIP(c, hipDeviceSynchronize());  // asynchronous renders on the caller's streams may still read the slot
    drained(c);
    (void)hipGetLastError();
    const size_t bytes = n * sizeof(float4);
    if (c->vol[slot].data && c->vol_bytes[slot] != bytes) {
        (void)hipFree(const_cast<float4*>(c->vol[slot].data));
        c->vol[slot] = DevVolume{};
        c->vol_bytes[slot] = 0;
    }
    float4* d = const_cast<float4*>(c->vol[slot].data);
    if (!d) VR_HIP(c, hipMalloc(&d, bytes));
    T* d_raw = nullptr;
    hipError_t e = hipMalloc(&d_raw, n * sizeof(T));
    if (e == hipSuccess) e = hipMemcpyAsync(d_raw, raw, n * sizeof(T), hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) {
        hipLaunchKernelGGL((broadcast_raw_kernel<T>), dim3(2048), dim3(256), 0, c->stream, d_raw, d, n);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (d_raw) (void)hipFree(d_raw);
    if (e != hipSuccess) {
        if (!c->vol[slot].data) (void)hipFree(d);
        return fail(c, e == hipErrorOutOfMemory ? VR_ERR_OOM : VR_ERR_HIP,
                    std::string("vr_volume_upload_raw: ") + hipGetErrorString(e));
    }
    c->vol[slot].data = d;
    c->vol[slot].nx = nx;
    c->vol[slot].ny = ny;
    c->vol[slot].nz = nz;
    c->vol_bytes[slot] = bytes;
    return refresh_bricks(c, slot);
}

}  // namespace

extern "C" {

int vr_volume_upload_raw16(vr_ctx* c, int slot, const uint16_t* raw, uint16_t nx, uint16_t ny, uint16_t nz)
{
    return upload_raw(c, slot, raw, nx, ny, nz);
}
int vr_volume_upload_raw32(vr_ctx* c, int slot, const uint32_t* raw, uint16_t nx, uint16_t ny, uint16_t nz)
{
    return upload_raw(c, slot, raw, nx, ny, nz);
}

int vr_volume_normalize(vr_ctx* c, int slot, int normalization_value, int* used_value)
{
    int rc = check_slot(c, slot, "vr_volume_normalize");
    if (rc != VR_OK) return rc;
    float4* d = const_cast<float4*>(c->vol[slot].data);
    const size_t n = (size_t)c->vol[slot].nx * c->vol[slot].ny * c->vol[slot].nz;
    if (normalization_value == 0) {  // GetMaxNumber(): max of component [0], truncated
        unsigned* d_max = reinterpret_cast<unsigned*>(c->d_counters);
        VR_HIP(c, hipMemsetAsync(d_max, 0, sizeof(unsigned), c->stream));
        hipLaunchKernelGGL(max_component_kernel, dim3(2048), dim3(256), 0, c->stream, d, n, 0, d_max);
        VR_HIP(c, hipGetLastError());
        unsigned bits = 0;
        VR_HIP(c, hipMemcpyAsync(&bits, d_max, sizeof bits, hipMemcpyDeviceToHost, c->stream));
        VR_HIP(c, hipStreamSynchronize(c->stream));
        float mx;
        std::memcpy(&mx, &bits, sizeof mx);
        normalization_value = (int)(size_t)mx;
    }
    if (used_value) *used_value = normalization_value;
    hipLaunchKernelGGL(normalize_kernel, dim3(2048), dim3(256), 0, c->stream, d, n, normalization_value);
    VR_HIP(c, hipGetLastError());
    return refresh_bricks(c, slot);
}

int vr_volume_precompute_gradient(vr_ctx* c, int slot, int norm_to_zero_one)
{
    int rc = check_slot(c, slot, "vr_volume_precompute_gradient");
    if (rc != VR_OK) return rc;
    float4* d = const_cast<float4*>(c->vol[slot].data);
    const DevVolume& v = c->vol[slot];
    const size_t n = (size_t)v.nx * v.ny * v.nz;
    unsigned* d_max = reinterpret_cast<unsigned*>(c->d_counters);
    VR_HIP(c, hipMemsetAsync(d_max, 0, sizeof(unsigned), c->stream));
    dim3 block(256), grid((unsigned)((v.nx + 255) / 256), (unsigned)v.ny, (unsigned)v.nz);
    hipLaunchKernelGGL(gradient_kernel, grid, block, 0, c->stream, d, v.nx, v.ny, v.nz, norm_to_zero_one ? 1 : 0, d_max);
    VR_HIP(c, hipGetLastError());
    if (norm_to_zero_one) {
        hipLaunchKernelGGL(scale_gradient_kernel, dim3(2048), dim3(256), 0, c->stream, d, n, d_max);
        VR_HIP(c, hipGetLastError());
    }
    return refresh_bricks(c, slot);
}

int vr_volume_download(vr_ctx* c, int slot, float* vec4_voxels)
{
    int rc = check_slot(c, slot, "vr_volume_download");
    if (rc != VR_OK) return rc;
    if (!vec4_voxels) return fail(c, VR_ERR_INVALID_ARG, "vr_volume_download: destination is NULL");
    VR_HIP(c, hipMemcpy(vec4_voxels, c->vol[slot].data, c->vol_bytes[slot], hipMemcpyDeviceToHost));
    return VR_OK;
}

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
    int rc;
    auto hip_ok = [&](hipError_t he, const char* what) {
        if (he == hipSuccess) return true;
        c->err = std::string(what) + ": " + hipGetErrorString(he);
        return false;
    };
    if (!hip_ok(hipSetDevice(device_id), "hipSetDevice")) return bail(VR_ERR_HIP);
    if (!hip_ok(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking), "hipStreamCreate")) return bail(VR_ERR_HIP);
    {
        int cus = 0;
        if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device_id) == hipSuccess && cus > 0) c->n_cus = cus;
    }
    // experiment knobs (A/B measurements; none changes any result)
    if (const char* e = getenv("VR_EXP_FLAVOUR")) {
        const int f = atoi(e);
        if (f >= 0 && f <= 18 && !removed_flavour(f)) c->default_flavour = f;
    }
    if (const char* e = getenv("VR_EXP_P2_WINDOW")) {  // records per gather window of march_p2_kernel (tests: the moving window on small volumes)
        const long long w = atoll(e);
        if (w > 0 && w <= 0x3fffffffll) c->p2_window = (unsigned)w;
    }
    if (const char* e = getenv("VR_EXP_TUNE")) c->tune_mode = atoi(e);
    if (!hip_ok(hipMalloc(&c->d_pw_heads, (size_t)kInFlight * 8 * 64 * sizeof(unsigned)), "hipMalloc(queue heads)")) return bail(VR_ERR_HIP);
    if (!hip_ok(hipMemset(c->d_pw_heads, 0, (size_t)kInFlight * 8 * 64 * sizeof(unsigned)), "hipMemset(queue heads)")) return bail(VR_ERR_HIP);
    if (!hip_ok(hipEventCreate(&c->tm.ev_begin), "hipEventCreate")) return bail(VR_ERR_HIP);
    if (!hip_ok(hipEventCreate(&c->tm.ev_k0), "hipEventCreate")) return bail(VR_ERR_HIP);
    if (!hip_ok(hipEventCreate(&c->tm.ev_k1), "hipEventCreate")) return bail(VR_ERR_HIP);
    if (!hip_ok(hipEventCreate(&c->tm.ev_end), "hipEventCreate")) return bail(VR_ERR_HIP);
    for (int i = 0; i < kRing; ++i)
        if (!hip_ok(hipEventCreate(&c->ring.k0[i]), "hipEventCreate") || !hip_ok(hipEventCreate(&c->ring.k1[i]), "hipEventCreate"))
            return bail(VR_ERR_HIP);
    for (int i = 0; i < kInFlight; ++i)
        if (!hip_ok(hipEventCreateWithFlags(&c->slot_done[i], hipEventDisableTiming), "hipEventCreate")) return bail(VR_ERR_HIP);
    for (auto& o : c->order_ring)
        if (!hip_ok(hipEventCreateWithFlags(&o.sorted, hipEventDisableTiming), "hipEventCreate")) return bail(VR_ERR_HIP);
    // The sorts run on a stream of their own, default priority.  The runtime deals streams onto a handful of hardware queues
    // per priority level, and a sort waits (a barrier in its queue) for a launch that is still running, so WHICH streams end up
    // sharing a queue with this one matters: measured on this box, a high- or low-priority sort stream lets a third frame in
    // flight overlap (a rank's eighth of C3: 0.142 -> 0.110 ms per frame, kernels alone) but costs the multi-GPU loop 50 us per
    // frame (0.24 -> 0.29 ms one frame at a time; with a high-priority sort stream its gather stream, high priority too, meets
    // the sorts' barriers), and the full C3 frame gains nothing from a third frame in flight either way (tools/exp_tiles.py,
    // tools/exp_queues).
    if (!hip_ok(hipStreamCreateWithFlags(&c->order_stream, hipStreamNonBlocking), "hipStreamCreate")) return bail(VR_ERR_HIP);
    if (!hip_ok(hipEventCreateWithFlags(&c->edit_ev, hipEventDisableTiming), "hipEventCreate")) return bail(VR_ERR_HIP);
    for (auto& st : c->stage)
        if (!hip_ok(hipEventCreateWithFlags(&st.done, hipEventDisableTiming), "hipEventCreate")) return bail(VR_ERR_HIP);
    if (!hip_ok(hipHostMalloc((void**)&c->h_skip, kGen * sizeof(SkipSummary), hipHostMallocDefault), "hipHostMalloc")) return bail(VR_ERR_HIP);
    std::memset(c->h_skip, 0, kGen * sizeof(SkipSummary));
    if (!hip_ok(hipMalloc(&c->d_skip_sum, kGen * sizeof(SkipSumDev)), "hipMalloc(skip summary)")) return bail(VR_ERR_HIP);
    if (!hip_ok(hipMemset(c->d_skip_sum, 0, kGen * sizeof(SkipSumDev)), "hipMemset(skip summary)")) return bail(VR_ERR_HIP);
    if (hipHostMalloc((void**)&c->h_span, kRing * sizeof(unsigned long long), hipHostMallocDefault) == hipSuccess)
        std::memset(c->h_span, 0, kRing * sizeof(unsigned long long));
    else
        c->h_span = nullptr;  // (every launch is then timed with events)
    if (hipHostMalloc((void**)&c->h_end, kRing * sizeof(unsigned long long), hipHostMallocDefault) == hipSuccess)
        std::memset(c->h_end, 0, kRing * sizeof(unsigned long long));
    else
        c->h_end = nullptr;  // (no measured kernel choice with launches in flight: the prior's pick stays)
    if (hipHostMalloc((void**)&c->h_chain, kOrderRing * sizeof(unsigned), hipHostMallocDefault) == hipSuccess)
        std::memset(c->h_chain, 0, kOrderRing * sizeof(unsigned));
    else
        c->h_chain = nullptr;  // (the choice of lanes per ray then goes by the launch size alone)
    if (!hip_ok(hipMalloc(&c->d_counters, 3 * sizeof(unsigned long long)), "hipMalloc(counters)")) return bail(VR_ERR_HIP);
    if (!hip_ok(hipHostMalloc((void**)&c->h_counters, 3 * sizeof(unsigned long long), hipHostMallocDefault),
                "hipHostMalloc"))
        return bail(VR_ERR_HIP);
    c->h_counters[0] = c->h_counters[1] = c->h_counters[2] = 0;
    rc = alloc_frame(c);
    if (rc != VR_OK) return bail(rc);
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
    for (int i = 0; i < VR_MAX_VOLUMES; ++i)
        if (c->vol[i].data) (void)hipFree(const_cast<float4*>(c->vol[i].data));
    for (int i = 0; i < VR_MAX_VOLUMES; ++i)
        if (c->vol_bricks[i]) (void)hipFree(c->vol_bricks[i]);
    for (int i = 0; i < VR_MAX_VOLUMES; ++i) {
        if (c->vol_dens[i]) (void)hipFree(c->vol_dens[i]);
        if (c->vol_bricked[i]) (void)hipFree(c->vol_bricked[i]);
        if (c->vol_bdens[i]) (void)hipFree(c->vol_bdens[i]);
    }
    if (c->merged_bricks) (void)hipFree(c->merged_bricks);
    for (int i = 0; i < VR_MAX_VOLUMES; ++i) {
        if (c->proj_rec[i]) (void)hipFree(c->proj_rec[i]);
        if (c->proj_range[i]) (void)hipFree(c->proj_range[i]);
        if (c->proj_built[i].ev) (void)hipEventDestroy(c->proj_built[i].ev);
    }
    for (auto* b : c->d_slice_counts)
        if (b) (void)hipFree(b);
    if (c->d_slice_out) (void)hipFree(c->d_slice_out);
    for (auto* b : c->d_hist_stats)
        if (b) (void)hipFree(b);
    if (c->d_hist_out) (void)hipFree(c->d_hist_out);
    for (auto& e : c->shadow) {
        if (e.buf.d) (void)hipFree(e.buf.d);
        if (e.built.ev) (void)hipEventDestroy(e.built.ev);
    }
    for (auto& g : c->field)
        if (g.d) (void)hipFree(g.d);
    if (c->dist_tmp) (void)hipFree(c->dist_tmp);
    for (auto& slot : c->tf_buf)
        for (auto& kind : slot)
            for (auto& g : kind)
                if (g.d) (void)hipFree(g.d);
    for (auto& st : c->stage) {
        if (st.h) (void)hipHostFree(st.h);
        if (st.done) (void)hipEventDestroy(st.done);
    }
    if (c->edit_ev) (void)hipEventDestroy(c->edit_ev);
    if (c->h_skip) (void)hipHostFree(c->h_skip);
    if (c->d_skip_sum) (void)hipFree(c->d_skip_sum);
    if (c->d_frame) (void)hipFree(c->d_frame);
    if (c->d_tiles) (void)hipFree(c->d_tiles);
    if (c->d_present) (void)hipFree(c->d_present);
    if (c->d_pick) (void)hipFree(c->d_pick);
    if (c->d_pick_depth) (void)hipFree(c->d_pick_depth);
    if (c->d_counters) (void)hipFree(c->d_counters);
    if (c->d_pw_heads) (void)hipFree(c->d_pw_heads);
    for (auto* b : c->d_block_counts)
        if (b) (void)hipFree(b);
    if (c->h_counters) (void)hipHostFree(c->h_counters);
    for (int i = 0; i < kRing; ++i) {
        if (c->ring.k0[i]) (void)hipEventDestroy(c->ring.k0[i]);
        if (c->ring.k1[i]) (void)hipEventDestroy(c->ring.k1[i]);
    }
    for (auto e : c->slot_done)
        if (e) (void)hipEventDestroy(e);
    for (auto& o : c->order_ring) {
        if (o.sorted) (void)hipEventDestroy(o.sorted);
        if (o.buf) (void)hipFree(o.buf);
    }
    if (c->order_stream) (void)hipStreamDestroy(c->order_stream);
    if (c->h_chain) (void)hipHostFree(c->h_chain);
    if (c->h_span) (void)hipHostFree(c->h_span);
    if (c->h_end) (void)hipHostFree(c->h_end);
    for (int k = 0; k < c->n_flight; ++k) (void)hipStreamDestroy(c->flight[k]);
    if (c->tm.ev_begin) (void)hipEventDestroy(c->tm.ev_begin);
    if (c->tm.ev_k0) (void)hipEventDestroy(c->tm.ev_k0);
    if (c->tm.ev_k1) (void)hipEventDestroy(c->tm.ev_k1);
    if (c->tm.ev_end) (void)hipEventDestroy(c->tm.ev_end);
    if (c->stream) (void)hipStreamDestroy(c->stream);
    delete c;
}

static int volume_upload_common(vr_ctx* c, int slot, const void* src, bool src_is_device, uint16_t nx, uint16_t ny,
                                uint16_t nz)
{
    if (!c) return VR_ERR_INVALID_ARG;
    if (slot < 0 || slot >= VR_MAX_VOLUMES) return fail(c, VR_ERR_INVALID_ARG, "vr_volume_upload: bad slot");
    if (!src) return fail(c, VR_ERR_INVALID_ARG, "vr_volume_upload: data is NULL");
    if (nx == 0 || ny == 0 || nz == 0) return fail(c, VR_ERR_INVALID_ARG, "vr_volume_upload: empty volume");
    unsigned long long voxels = (unsigned long long)nx * ny * nz;
    if (voxels > 0xFFFFFFFFull) return fail(c, VR_ERR_INVALID_ARG, "vr_volume_upload: more than 2^32 voxels");
    size_t bytes = (size_t)voxels * sizeof(float4);
    VR_HIP(c, hipSetDevice(c->device));
    VR_HIP(c, hipDeviceSynchronize());  // asynchronous renders on the caller's streams may still read the slot
    drained(c);
    if (c->vol[slot].data && c->vol_bytes[slot] != bytes) {
        (void)hipFree(const_cast<float4*>(c->vol[slot].data));
        c->vol[slot] = DevVolume{};
        c->vol_bytes[slot] = 0;
    }
    float4* d = const_cast<float4*>(c->vol[slot].data);
    if (!d) VR_HIP(c, hipMalloc(&d, bytes));
    hipError_t e = hipMemcpyAsync(d, src, bytes, src_is_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) {
        if (!c->vol[slot].data) (void)hipFree(d);
        return fail(c, VR_ERR_HIP, std::string("vr_volume_upload: copy failed: ") + hipGetErrorString(e));
    }
    c->vol[slot].data = d;
    c->vol[slot].nx = nx;
    c->vol[slot].ny = ny;
    c->vol[slot].nz = nz;
    c->vol_bytes[slot] = bytes;
    return refresh_bricks(c, slot);
}

int vr_volume_upload(vr_ctx* c, int slot, const float* vec4_voxels, uint16_t nx, uint16_t ny, uint16_t nz)
{
    return volume_upload_common(c, slot, vec4_voxels, false, nx, ny, nz);
}

int vr_volume_upload_device(vr_ctx* c, int slot, const void* d_vec4_voxels, uint16_t nx, uint16_t ny, uint16_t nz)
{
    return volume_upload_common(c, slot, d_vec4_voxels, true, nx, ny, nz);
}

static int tf_check(vr_ctx* c, int slot, const float* table, uint32_t R, const char* who)
{
    if (slot < 0 || slot >= VR_MAX_TFS) return fail(c, VR_ERR_INVALID_ARG, std::string(who) + ": bad slot");
    if (!table) return fail(c, VR_ERR_INVALID_ARG, std::string(who) + ": table is NULL");
    if (R == 0 || R > (1u << 24)) return fail(c, VR_ERR_INVALID_ARG, std::string(who) + ": bad resolution");
    return VR_OK;
}

// the host state of a table as the launches after an upload see it: the current generation, its resolution, its flags
static void tf_set_current(vr_ctx* c, int slot, const float* table, uint32_t R, bool is_color)
{
    ++c->tf_epoch;
    const GenBuf& g = c->tf_buf[slot][is_color ? 1 : 0][c->tf_cur[slot][is_color ? 1 : 0]];
    if (is_color) {
        c->tf[slot].color = (const float4*)g.d;
        c->tf[slot].res_c = (int)R;
        c->tf_color_finite[slot] = all_finite(table, (int)(4 * R));
    } else {
        if (slot == 0) ++c->opacity_edits;  // (the light volumes' key)
        c->tf[slot].opacity = (const float*)g.d;
        c->tf[slot].res_o = (int)R;
        int z = -1;
        c->tf_opacity_finite[slot] = all_finite(table, (int)R);
        if (c->tf_opacity_finite[slot])
            while (z + 1 < (int)R && table[z + 1] == 0.0f) ++z;
        c->tf_zero_prefix[slot] = z;
    }
}

static int tf_upload_one(vr_ctx* c, int slot, const float* table, uint32_t R, bool is_color)
{
    if (!c) return VR_ERR_INVALID_ARG;
    if (const int rc = tf_check(c, slot, table, R, "vr_tf_upload")) return rc;
    VR_HIP(c, hipSetDevice(c->device));
    VR_HIP(c, hipDeviceSynchronize());  // asynchronous renders on the caller's streams may still read the table
    drained(c);
    const int comps = is_color ? 4 : 1;
    GenBuf& g = c->tf_buf[slot][is_color ? 1 : 0][c->tf_cur[slot][is_color ? 1 : 0]];
    if (is_color) {
        c->tf[slot].color = nullptr;
        c->tf[slot].res_c = 0;
    } else {
        c->tf[slot].opacity = nullptr;
        c->tf[slot].res_o = 0;
    }
    if (const int rc = grow(c, &g.d, &g.cap, ((size_t)R + 2) * comps * sizeof(float), true)) return rc;
    // device layout (DevTF): the first and the last texel once more at either end
    float* d = (float*)g.d;
    const size_t texel = comps * sizeof(float);
    VR_HIP(c, hipMemcpyAsync(d + comps, table, R * texel, hipMemcpyHostToDevice, c->stream));
    VR_HIP(c, hipMemcpyAsync(d, table, texel, hipMemcpyHostToDevice, c->stream));
    VR_HIP(c, hipMemcpyAsync(d + ((size_t)R + 1) * comps, table + comps * ((size_t)R - 1), texel, hipMemcpyHostToDevice, c->stream));
    VR_HIP(c, hipStreamSynchronize(c->stream));
    g.written();
    tf_set_current(c, slot, table, R, is_color);
    return VR_OK;
}

// An asynchronous opacity edit of slot 0 that moves the zero prefix or changes the resolution: the field in use is rebuilt on the edit's
// stream into its next generation, for the records it was built from -- unless it is stale anyway (a volume changed, no field yet): then
// the next skipping launch rebuilds it as before.  A failure here leaves it to that launch as well.
static void rebuild_field_async(vr_ctx* c, hipStream_t s)
{
    const int z = c->tf_zero_prefix[0], res = c->tf[0].res_o;
    if (!c->brick_dist || (c->dist_z == z && c->dist_res == res) || c->dist_epoch != c->brick_epoch) return;
    if (c->dist_rgb ? (c->merged_stale || c->dist_records != (const void*)c->merged_bricks) : c->dist_records != (const void*)c->vol_bricks[0])
        return;
    const int b = (c->field_cur + 1) % kGen;
    GenBuf& g = c->field[b];
    const size_t nb = (size_t)c->dist_bn[0] * c->dist_bn[1] * c->dist_bn[2];
    const bool fresh = nb > g.cap;
    if (grow(c, &g.d, &g.cap, nb, false) != VR_OK || grow(c, (void**)&c->dist_tmp, &c->tmp_cap, nb, false) != VR_OK ||
        (!fresh && reuse_wait(c, s, g) != VR_OK) ||
        build_field(c, s, (const float2*)c->dist_records, c->dist_bn, c->dist_rgb, z, res, (unsigned char*)g.d, b, c->skip_gen + 1) != VR_OK) {
        (void)hipGetLastError();
        return;
    }
    ++c->skip_gen;
    g.written();
    c->field_cur = b;
    c->brick_dist = (unsigned char*)g.d;
    c->skip_pending = true;
    c->dist_z = z;
    c->dist_res = res;
}

// vr_tf_upload_opacity_async / _color_async: the table into pinned staging (DevTF layout), one copy on `s` into the next generation
// behind the last launch that read it, the host state as the synchronous upload sets it; then edit_ev behind it all.
static int tf_upload_async(vr_ctx* c, int slot, const float* table, uint32_t R, bool is_color, void* stream)
{
    if (!c) return VR_ERR_INVALID_ARG;
    if (const int rc = tf_check(c, slot, table, R, is_color ? "vr_tf_upload_color_async" : "vr_tf_upload_opacity_async")) return rc;
    VR_HIP(c, hipSetDevice(c->device));
    (void)hipGetLastError();
    hipStream_t s = stream ? (hipStream_t)stream : c->stream;
    const int comps = is_color ? 4 : 1, kind = is_color ? 1 : 0;
    const size_t texel = comps * sizeof(float), bytes = ((size_t)R + 2) * texel;
    vr_ctx::Stage& st = c->stage[c->stage_next % kStage];
    if (st.used) VR_HIP(c, hipEventSynchronize(st.done));  // (the one host wait: kStage edits are still being copied)
    st.used = false;
    if (bytes > st.cap) {
        if (st.h) c->retired_host.push_back(st.h);
        st.h = nullptr;
        st.cap = 0;
        VR_HIP(c, hipHostMalloc(&st.h, bytes, hipHostMallocDefault));
        st.cap = bytes;
    }
    float* h = (float*)st.h;
    std::memcpy(h + comps, table, R * texel);
    std::memcpy(h, table, texel);
    std::memcpy(h + ((size_t)R + 1) * comps, table + comps * ((size_t)R - 1), texel);
    // behind the edit before it, whatever its stream
    if (c->edit_gen > c->drained_gen && s != c->edit_stream) VR_HIP(c, hipStreamWaitEvent(s, c->edit_ev, 0));
    const int b = (c->tf_cur[slot][kind] + 1) % kGen;
    GenBuf& g = c->tf_buf[slot][kind][b];
    if (bytes > g.cap) {
        if (const int rc = grow(c, &g.d, &g.cap, bytes, false)) return rc;
    } else if (const int rc = reuse_wait(c, s, g)) {
        return rc;
    }
    VR_HIP(c, hipMemcpyAsync(g.d, h, bytes, hipMemcpyHostToDevice, s));
    VR_HIP(c, hipEventRecord(st.done, s));
    st.used = true;
    ++c->stage_next;
    g.written();
    c->tf_cur[slot][kind] = b;
    tf_set_current(c, slot, table, R, is_color);
    if (!is_color && slot == 0) rebuild_field_async(c, s);
    VR_HIP(c, hipEventRecord(c->edit_ev, s));
    c->edit_stream = s;
    ++c->edit_gen;
    return VR_OK;
}

int vr_tf_upload_opacity(vr_ctx* c, int slot, const float* opacity, uint32_t R) { return tf_upload_one(c, slot, opacity, R, false); }
int vr_tf_upload_color(vr_ctx* c, int slot, const float* color_rgba, uint32_t R) { return tf_upload_one(c, slot, color_rgba, R, true); }
int vr_tf_upload_opacity_async(vr_ctx* c, int slot, const float* opacity, uint32_t R, void* stream)
{
    return tf_upload_async(c, slot, opacity, R, false, stream);
}
int vr_tf_upload_color_async(vr_ctx* c, int slot, const float* color_rgba, uint32_t R, void* stream)
{
    return tf_upload_async(c, slot, color_rgba, R, true, stream);
}

int vr_tf_upload(vr_ctx* c, int slot, const float* opacity, const float* color_rgba, uint32_t R)
{
    if (!c) return VR_ERR_INVALID_ARG;
    if (!opacity || !color_rgba) return fail(c, VR_ERR_INVALID_ARG, "vr_tf_upload: table is NULL");
    int rc = tf_upload_one(c, slot, opacity, R, false);
    return rc != VR_OK ? rc : tf_upload_one(c, slot, color_rgba, R, true);
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

int vr_render(vr_ctx* c, int variant)
{
    if (!c) return VR_ERR_INVALID_ARG;
    int rc = enqueue_render(c, variant, 0, 1, false, nullptr, c->stream, true);
    if (rc != VR_OK) return rc;
    VR_HIP(c, hipStreamSynchronize(c->stream));
    return fetch_counters(c);
}

int vr_tile_count(const vr_ctx* c, int rank, int world)
{
    if (!c || world < 1 || rank < 0 || rank >= world) return VR_ERR_INVALID_ARG;
    return tile_count(c, rank, world);
}

int vr_render_tiles(vr_ctx* c, int variant, int rank, int world)
{
    if (!c) return VR_ERR_INVALID_ARG;
    int rc = enqueue_render(c, variant, rank, world, true, nullptr, c->stream, true);
    if (rc != VR_OK) return rc;
    VR_HIP(c, hipStreamSynchronize(c->stream));
    return fetch_counters(c);
}

int vr_render_async(vr_ctx* c, int variant, void* d_frame, void* stream)
{
    if (!c) return VR_ERR_INVALID_ARG;
    hipStream_t s = stream ? (hipStream_t)stream : c->stream;
    return enqueue_render(c, variant, 0, 1, false, (float4*)d_frame, s, false);
}

int vr_render_tiles_async(vr_ctx* c, int variant, int rank, int world, void* d_tiles, void* stream)
{
    if (!c) return VR_ERR_INVALID_ARG;
    hipStream_t s = stream ? (hipStream_t)stream : c->stream;
    return enqueue_render(c, variant, rank, world, true, (float4*)d_tiles, s, false);
}

int vr_render_batch_async(vr_ctx* c, int variant, int n_frames, const vr_uniforms* uniforms, void* const* d_frames, void* stream)
{
    if (!c) return VR_ERR_INVALID_ARG;
    if (!uniforms || !d_frames) return fail(c, VR_ERR_INVALID_ARG, "vr_render_batch_async: uniforms / buffers are NULL");
    hipStream_t s = stream ? (hipStream_t)stream : c->stream;
    return enqueue_render(c, variant, 0, 1, false, nullptr, s, false, n_frames, uniforms, d_frames);
}

int vr_render_tiles_batch_async(vr_ctx* c, int variant, int rank, int world, int n_frames, const vr_uniforms* uniforms,
                                void* const* d_tiles, void* stream)
{
    if (!c) return VR_ERR_INVALID_ARG;
    if (!uniforms || !d_tiles) return fail(c, VR_ERR_INVALID_ARG, "vr_render_tiles_batch_async: uniforms / buffers are NULL");
    hipStream_t s = stream ? (hipStream_t)stream : c->stream;
    return enqueue_render(c, variant, rank, world, true, nullptr, s, false, n_frames, uniforms, d_tiles);
}

int vr_unpack_tiles_strided_async(vr_ctx* c, const void* d_gathered, int world, int rank_stride_tiles, void* d_frame, void* stream)
{
    if (!c) return VR_ERR_INVALID_ARG;
    if (!d_gathered || world < 1) return fail(c, VR_ERR_INVALID_ARG, "vr_unpack_tiles_async: bad arguments");
    const int tpr = tile_count(c, 0, world);
    if (rank_stride_tiles < tpr) return fail(c, VR_ERR_INVALID_ARG, "vr_unpack_tiles_strided_async: stride smaller than a segment");
    VR_HIP(c, hipSetDevice(c->device));
    (void)hipGetLastError();
    hipStream_t s = stream ? (hipStream_t)stream : c->stream;
    float4* frame = d_frame ? (float4*)d_frame : c->d_frame;
    dim3 block(64, 4), grid((c->W + 63) / 64, (c->H + 3) / 4);
    hipLaunchKernelGGL(unpack_tiles_kernel, grid, block, 0, s, (const float4*)d_gathered, frame, (int)c->W, (int)c->H,
                       tiles_x_of(c), world, rank_stride_tiles);
    VR_HIP(c, hipGetLastError());
    return VR_OK;
}

int vr_unpack_tiles_async(vr_ctx* c, const void* d_gathered, int world, void* d_frame, void* stream)
{
    if (!c) return VR_ERR_INVALID_ARG;
    if (world < 1) return fail(c, VR_ERR_INVALID_ARG, "vr_unpack_tiles_async: bad arguments");
    return vr_unpack_tiles_strided_async(c, d_gathered, world, tile_count(c, 0, world), d_frame, stream);
}

int vr_present_async(vr_ctx* c, const void* d_frame, void* d_bgra8, void* stream)
{
    if (!c) return VR_ERR_INVALID_ARG;
    if (!d_bgra8) return fail(c, VR_ERR_INVALID_ARG, "vr_present_async: destination is NULL");
    VR_HIP(c, hipSetDevice(c->device));
    (void)hipGetLastError();
    hipStream_t s = stream ? (hipStream_t)stream : c->stream;
    const size_t n = (size_t)c->W * c->H;
    hipLaunchKernelGGL(present_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s,
                       d_frame ? (const float4*)d_frame : c->d_frame, (uint32_t*)d_bgra8, (int)n);
    VR_HIP(c, hipGetLastError());
    return VR_OK;
}

int vr_present_tiles_async(vr_ctx* c, const void* d_gathered, int world, int rank_stride_tiles, void* d_bgra8, void* stream)
{
    if (!c) return VR_ERR_INVALID_ARG;
    if (!d_gathered || !d_bgra8 || world < 1) return fail(c, VR_ERR_INVALID_ARG, "vr_present_tiles_async: bad arguments");
    const int tpr = tile_count(c, 0, world);
    if (rank_stride_tiles <= 0) rank_stride_tiles = tpr;
    if (rank_stride_tiles < tpr) return fail(c, VR_ERR_INVALID_ARG, "vr_present_tiles_async: stride smaller than a segment");
    VR_HIP(c, hipSetDevice(c->device));
    (void)hipGetLastError();
    hipStream_t s = stream ? (hipStream_t)stream : c->stream;
    dim3 block(64, 4), grid((c->W + 63) / 64, (c->H + 3) / 4);
    hipLaunchKernelGGL(present_tiles_kernel, grid, block, 0, s, (const float4*)d_gathered, (uint32_t*)d_bgra8, (int)c->W, (int)c->H,
                       tiles_x_of(c), world, rank_stride_tiles);
    VR_HIP(c, hipGetLastError());
    return VR_OK;
}

int vr_present_packed_async(vr_ctx* c, const void* d_tiles_rgba, int n_tiles, void* d_tiles_bgra8, void* stream)
{
    if (!c) return VR_ERR_INVALID_ARG;
    if (!d_tiles_rgba || !d_tiles_bgra8 || n_tiles < 0) return fail(c, VR_ERR_INVALID_ARG, "vr_present_packed_async: bad arguments");
    if (n_tiles == 0) return VR_OK;
    VR_HIP(c, hipSetDevice(c->device));
    (void)hipGetLastError();
    hipStream_t s = stream ? (hipStream_t)stream : c->stream;
    const size_t n = (size_t)n_tiles * kTile * kTile;
    if (n > 0x7fffffffull) return fail(c, VR_ERR_INVALID_ARG, "vr_present_packed_async: too many tiles");
    hipLaunchKernelGGL(present_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, (const float4*)d_tiles_rgba, (uint32_t*)d_tiles_bgra8, (int)n);
    VR_HIP(c, hipGetLastError());
    return VR_OK;
}

int vr_unpack_tiles_bgra8_async(vr_ctx* c, const void* d_gathered_bgra8, int world, int rank_stride_tiles, void* d_bgra8, void* stream)
{
    if (!c) return VR_ERR_INVALID_ARG;
    if (!d_gathered_bgra8 || !d_bgra8 || world < 1) return fail(c, VR_ERR_INVALID_ARG, "vr_unpack_tiles_bgra8_async: bad arguments");
    const int tpr = tile_count(c, 0, world);
    if (rank_stride_tiles <= 0) rank_stride_tiles = tpr;
    if (rank_stride_tiles < tpr) return fail(c, VR_ERR_INVALID_ARG, "vr_unpack_tiles_bgra8_async: stride smaller than a segment");
    VR_HIP(c, hipSetDevice(c->device));
    (void)hipGetLastError();
    hipStream_t s = stream ? (hipStream_t)stream : c->stream;
    dim3 block(64, 4), grid((c->W + 63) / 64, (c->H + 3) / 4);
    hipLaunchKernelGGL(unpack_tiles_u32_kernel, grid, block, 0, s, (const uint32_t*)d_gathered_bgra8, (uint32_t*)d_bgra8, (int)c->W, (int)c->H,
                       tiles_x_of(c), world, rank_stride_tiles);
    VR_HIP(c, hipGetLastError());
    return VR_OK;
}

int vr_download(vr_ctx* c, float* frag_rgba, uint8_t* present_bgra8, uint64_t* composited_samples)
{
    if (!c) return VR_ERR_INVALID_ARG;
    VR_HIP(c, hipSetDevice(c->device));
    VR_HIP(c, hipStreamSynchronize(c->stream));
    size_t n = (size_t)c->W * c->H;
    if (frag_rgba) VR_HIP(c, hipMemcpy(frag_rgba, c->d_frame, n * sizeof(float4), hipMemcpyDeviceToHost));
    if (present_bgra8) {
        (void)hipGetLastError();
        hipLaunchKernelGGL(present_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c->stream, c->d_frame,
                           c->d_present, (int)n);
        VR_HIP(c, hipGetLastError());
        VR_HIP(c, hipStreamSynchronize(c->stream));
        VR_HIP(c, hipMemcpy(present_bgra8, c->d_present, n * sizeof(uint32_t), hipMemcpyDeviceToHost));
    }
    if (composited_samples) {
        int rc = fetch_counters(c);
        if (rc != VR_OK) return rc;
        *composited_samples = c->h_counters[0];
    }
    return VR_OK;
}

int vr_download_tiles(vr_ctx* c, float* tiles_rgba, uint64_t* composited_samples)
{
    if (!c) return VR_ERR_INVALID_ARG;
    VR_HIP(c, hipSetDevice(c->device));
    VR_HIP(c, hipStreamSynchronize(c->stream));
    if (tiles_rgba && c->last_tiles > 0)
        VR_HIP(c, hipMemcpy(tiles_rgba, c->d_tiles, (size_t)c->last_tiles * kTile * kTile * sizeof(float4),
                            hipMemcpyDeviceToHost));
    if (composited_samples) {
        int rc = fetch_counters(c);
        if (rc != VR_OK) return rc;
        *composited_samples = c->h_counters[0];
    }
    return VR_OK;
}

int vr_last_timing(vr_ctx* c, float* kernel_ms, float* total_ms)
{
    if (!c) return VR_ERR_INVALID_ARG;
    if (!c->tm.valid) return fail(c, VR_ERR_NOT_READY, "vr_last_timing: no vr_render / vr_render_tiles since the context was created or an *_async call");
    VR_HIP(c, hipSetDevice(c->device));
    VR_HIP(c, hipEventSynchronize(c->tm.ev_end));
    float k = 0.0f, t = 0.0f;
    VR_HIP(c, hipEventElapsedTime(&k, c->tm.ev_k0, c->tm.ev_k1));
    VR_HIP(c, hipEventElapsedTime(&t, c->tm.ev_begin, c->tm.ev_end));
    if (kernel_ms) *kernel_ms = k;
    if (total_ms) *total_ms = t;
    return VR_OK;
}

int vr_kernel_times(vr_ctx* c, float* out_ms, int capacity)
{
    if (!c) return VR_ERR_INVALID_ARG;
    if (!out_ms || capacity < 0) return fail(c, VR_ERR_INVALID_ARG, "vr_kernel_times: bad arguments");
    VR_HIP(c, hipSetDevice(c->device));
    long long have = c->ring.head < kRing ? c->ring.head : kRing;
    int n = (int)(have < capacity ? have : capacity);
    bool synced = false;
    for (int i = 0; i < n; ++i) {
        int slot = (int)((c->ring.head - n + i) % kRing);
        if (!c->ring_events[slot]) {  // from the launch's records, written by the sort that runs behind it
            if (!synced) VR_HIP(c, hipStreamSynchronize(c->order_stream));
            synced = true;
            const unsigned long long ticks = *(volatile unsigned long long*)&c->h_span[slot];
            out_ms[i] = ticks ? (float)((double)(ticks - 1) * 1.0e-5) : 0.0f;
            continue;
        }
        VR_HIP(c, hipEventSynchronize(c->ring.k1[slot]));
        VR_HIP(c, hipEventElapsedTime(&out_ms[i], c->ring.k0[slot], c->ring.k1[slot]));
    }
    return n;
}

int vr_set_kernel_timing(vr_ctx* c, int mode)
{
    if (!c) return VR_ERR_INVALID_ARG;
    if (mode != VR_TIMING_RECORDS && mode != VR_TIMING_EVENTS) return fail(c, VR_ERR_INVALID_ARG, "vr_set_kernel_timing: bad mode");
    c->event_timing = mode == VR_TIMING_EVENTS;
    return VR_OK;
}

int vr_reset_kernel_times(vr_ctx* c)
{
    if (!c) return VR_ERR_INVALID_ARG;
    // (sorts of earlier launches still report their launch's duration into the ring: let them finish first)
    VR_HIP(c, hipSetDevice(c->device));
    VR_HIP(c, hipStreamSynchronize(c->order_stream));
    c->ring.head = 0;
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

int vr_last_covered_pixels(vr_ctx* c, uint64_t* covered)
{
    if (!c || !covered) return VR_ERR_INVALID_ARG;
    VR_HIP(c, hipSetDevice(c->device));
    VR_HIP(c, hipStreamSynchronize(c->stream));
    int rc = fetch_counters(c);
    if (rc != VR_OK) return rc;
    *covered = c->h_counters[1];
    return VR_OK;
}

int vr_last_counters(vr_ctx* c, uint64_t out[3])
{
    if (!c || !out) return VR_ERR_INVALID_ARG;
    VR_HIP(c, hipSetDevice(c->device));
    VR_HIP(c, hipStreamSynchronize(c->stream));
    int rc = fetch_counters(c);
    if (rc != VR_OK) return rc;
    out[0] = c->h_counters[0];
    out[1] = c->h_counters[1];
    out[2] = c->h_counters[2];
    return VR_OK;
}

int vr_last_block_trace(vr_ctx* c, uint64_t* out, int capacity)
{
    if (!c || capacity < 0 || (capacity > 0 && !out)) return VR_ERR_INVALID_ARG;
    VR_HIP(c, hipSetDevice(c->device));
    VR_HIP(c, hipDeviceSynchronize());
    const int n = c->cnt_blocks < capacity ? c->cnt_blocks : capacity;
    if (n > 0) {
        const unsigned long long* src = c->d_block_counts[c->cnt_buf] + c->cnt_offset;
        VR_HIP(c, hipMemcpy(out, src, (size_t)n * kBlockRecord * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    }
    return c->cnt_blocks;
}

int vr_last_kernel_flavour(vr_ctx* c)
{
    if (!c) return VR_ERR_INVALID_ARG;
    return c->last_flavour;
}

int vr_skip_field(vr_ctx* c, int variant, uint8_t* dist, size_t capacity, int dims[3], int box[6], uint64_t* active)
{
    if (!c) return VR_ERR_INVALID_ARG;
    if (variant < 0 || variant >= VR_VARIANT_COUNT) return fail(c, VR_ERR_INVALID_ARG, "vr_skip_field: bad variant");
    if (capacity > 0 && !dist) return fail(c, VR_ERR_INVALID_ARG, "vr_skip_field: dist is NULL");
    int nvol, ntf;
    variant_needs(variant, &nvol, &ntf);
    for (int i = 0; i < nvol; ++i)
        if (!c->vol[i].data) return fail(c, VR_ERR_NOT_READY, "vr_skip_field: volume slot " + std::to_string(i) + " is empty");
    for (int i = 0; i < ntf; ++i)
        if (!c->tf[i].opacity || !c->tf[i].color) return fail(c, VR_ERR_NOT_READY, "vr_skip_field: TF slot " + std::to_string(i) + " is empty");
    VR_HIP(c, hipSetDevice(c->device));
    VR_HIP(c, hipDeviceSynchronize());
    drained(c);
    (void)hipGetLastError();
    const Eligibility E = eligibility(c, 0, variant, 1, 0, 1, false, nullptr);
    if (!E.can_skip) return fail(c, VR_ERR_NOT_READY, "vr_skip_field: launches of this variant do not skip empty space now");
    MarchParams P;
    std::memset(&P, 0, sizeof P);
    if (const int rc = prepare_skip(c, variant, c->stream, P)) return rc;
    VR_HIP(c, hipStreamSynchronize(c->stream));
    const float bs[3] = {P.bsx, P.bsy, P.bsz};
    adopt_skip(c, bs);
    if (c->skip_pending) return fail(c, VR_ERR_HIP, "vr_skip_field: the field's count and box did not arrive");
    const size_t n = (size_t)c->dist_bn[0] * c->dist_bn[1] * c->dist_bn[2];
    if (capacity > 0) VR_HIP(c, hipMemcpy(dist, c->brick_dist, capacity < n ? capacity : n, hipMemcpyDeviceToHost));
    if (dims)
        for (int a = 0; a < 3; ++a) dims[a] = c->dist_bn[a];
    if (box)
        for (int a = 0; a < 6; ++a) box[a] = c->skip_box[a];
    if (active) *active = c->skip_active;
    return (int)n;
}

int64_t vr_unbounded_box_launches(vr_ctx* c)
{
    if (!c) return VR_ERR_INVALID_ARG;
    return c->unbounded_launches;
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
        hipEvent_t e0 = nullptr, e1 = nullptr;
        if (hipEventCreate(&e0) != hipSuccess || hipEventCreate(&e1) != hipSuccess) return nullptr;
        // candidates are created one by one; one is kept if it overlaps with every stream kept so far (at most 12 tries).
        // Rejected candidates stay alive until the search is over: the runtime hands a stream that is destroyed and created
        // again the very same hardware queue, and the search would try one queue twelve times.
        float one_ms = -1.0f;
        hipStream_t rejected[12];
        int n_rejected = 0;
        for (int tries = 0; tries < 12 && c->n_flight < kStreams; ++tries) {
            hipStream_t s = nullptr;
            if (hipStreamCreateWithFlags(&s, hipStreamNonBlocking) != hipSuccess) break;
            if (c->n_flight == 0) {  // the yardstick: one spin alone (the second measurement: the first one warms up)
                (void)spin_span_ms(s, nullptr, e0, e1);
                one_ms = spin_span_ms(s, nullptr, e0, e1);
            }
            bool ok = true;
            for (int k = 0; k < c->n_flight && ok; ++k) ok = streams_overlap(c->flight[k], s, e0, e1, one_ms);
            // ... and with the stream of the launch-order sorts, whose barriers (a sort waits for its launch) would hold back
            // the launches of a render stream that shares its queue
            if (ok && c->order_stream) ok = streams_overlap(c->order_stream, s, e0, e1, one_ms);
            if (ok) c->flight[c->n_flight++] = s;
            else rejected[n_rejected++] = s;  // shares a hardware queue with a kept one
        }
        for (int k = 0; k < n_rejected; ++k) (void)hipStreamDestroy(rejected[k]);
        (void)hipEventDestroy(e0);
        (void)hipEventDestroy(e1);
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
    c->shadow_div = grid_divisor;
    c->shadow_sigma = opacity_scale;
    return VR_OK;
}

int vr_shadow_volume(vr_ctx* c, float* out, size_t capacity, int dims[3])
{
    if (!c) return VR_ERR_INVALID_ARG;
    if (capacity > 0 && !out) return fail(c, VR_ERR_INVALID_ARG, "vr_shadow_volume: out is NULL");
    if (c->shadow_div == 0) return fail(c, VR_ERR_NOT_READY, "vr_shadow_volume: shadows are off");
    if (!c->vol[0].data) return fail(c, VR_ERR_NOT_READY, "vr_shadow_volume: volume slot 0 is empty");
    if (!c->tf[0].opacity || !c->tf[0].color) return fail(c, VR_ERR_NOT_READY, "vr_shadow_volume: TF slot 0 is empty");
    if (!c->have_uniforms) return fail(c, VR_ERR_NOT_READY, "vr_shadow_volume: vr_set_uniforms has not been called");
    int g[3];
    const size_t n = shadow_grid(c, g);
    if (n * sizeof(float) >= (1ull << 32)) return fail(c, VR_ERR_UNSUPPORTED, "vr_shadow_volume: the light volume would take 4 GiB or more");
    VR_HIP(c, hipSetDevice(c->device));
    VR_HIP(c, hipDeviceSynchronize());
    drained(c);
    (void)hipGetLastError();
    // the parameters a LIGHT launch of the context's uniforms would have (the flavour asked for decides the build's form; both give the
    // same texels)
    MarchParams P;
    fill_launch_params(c, P, c->u, 0, 1, false);
    const int requested = c->flavour == 0 ? c->default_flavour : c->flavour;
    const Eligibility E = eligibility(c, requested, VR_VARIANT_LIGHT, 1, 0, 1, false, nullptr);
    if (E.can_skip)
        if (const int rc = prepare_skip(c, VR_VARIANT_LIGHT, c->stream, P)) return rc;
    if (c->layout_mode == 0) use_bricked_copies(c, P);
    const bool off32 = c->vol_bytes[0] <= 0xFFFFFFFFull && !(P.vol[0].bricked && bricked_grid(P.vol[0]).slots * 16 > 0xFFFFFFFFull);
    const int rc = prepare_shadow(c, c->stream, P, shadow_key(c, c->u), P.brick_dist != nullptr && requested != 1, off32);
    c->shadow_cur = -1;  // (no launch reads it)
    if (rc) return rc;
    VR_HIP(c, hipStreamSynchronize(c->stream));
    if (capacity > 0) VR_HIP(c, hipMemcpy(out, P.vol[1].dens, (capacity < n ? capacity : n) * sizeof(float), hipMemcpyDeviceToHost));
    if (dims)
        for (int a = 0; a < 3; ++a) dims[a] = g[a];
    return (int)n;
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

namespace {

// the uniforms a depth pass needs, and the threshold of the context now
DepthParams depth_params(const vr_ctx* c)
{
    DepthParams D;
    std::memcpy(D.view, c->u.view, sizeof D.view);
    std::memcpy(D.proj, c->u.proj, sizeof D.proj);
    D.tau = c->surf_tau;
    return D;
}

}  // namespace

int vr_surface_depth_async(vr_ctx* c, const void* d_surface, void* d_depth, void* stream)
{
    if (!c) return VR_ERR_INVALID_ARG;
    if (!d_surface || !d_depth) return fail(c, VR_ERR_INVALID_ARG, "vr_surface_depth_async: a buffer is NULL");
    if (!c->have_uniforms) return fail(c, VR_ERR_NOT_READY, "vr_surface_depth_async: vr_set_uniforms has not been called");
    VR_HIP(c, hipSetDevice(c->device));
    (void)hipGetLastError();
    hipStream_t s = stream ? (hipStream_t)stream : c->stream;
    const size_t n = (size_t)c->W * c->H;
    hipLaunchKernelGGL(surface_depth_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, (const float4*)d_surface, (float*)d_depth,
                       (int)n, depth_params(c));
    VR_HIP(c, hipGetLastError());
    return VR_OK;
}

int vr_pick(vr_ctx* c, int variant, uint32_t x, uint32_t y, vr_pick_result* out)
{
    if (!c) return VR_ERR_INVALID_ARG;
    if (!out) return fail(c, VR_ERR_INVALID_ARG, "vr_pick: out is NULL");
    if (x >= c->W || y >= c->H) return fail(c, VR_ERR_INVALID_ARG, "vr_pick: the pixel lies outside the viewport");
    VR_HIP(c, hipSetDevice(c->device));
    // what the render before the pick left behind stays what the context reports: its counters are summed now ...
    if (const int rc = fetch_counters(c)) return rc;
    if (!c->d_pick) VR_HIP(c, hipMalloc(&c->d_pick, (size_t)c->W * c->H * sizeof(float4)));
    if (!c->d_pick_depth) VR_HIP(c, hipMalloc(&c->d_pick_depth, sizeof(float)));
    // ... and the launch's bookkeeping is put back behind the pick's own launch (which takes the next record slot, not the last one's)
    const int last_flavour = c->last_flavour, last_tiles = c->last_tiles, cnt_buf = c->cnt_buf, cnt_blocks = c->cnt_blocks;
    const bool last_unmeasured = c->last_unmeasured, tm_valid = c->tm.valid;
    const size_t cnt_offset = c->cnt_offset;
    const long long ring_head = c->ring.head;
    const unsigned long long counters[3] = {c->h_counters[0], c->h_counters[1], c->h_counters[2]};
    c->pick_px[0] = (int)x;
    c->pick_px[1] = (int)y;
    const int rc = enqueue_render(c, variant, 0, 1, false, c->d_pick, c->stream, false);
    c->pick_px[0] = c->pick_px[1] = -1;
    const hipError_t sync = hipDeviceSynchronize();
    if (sync == hipSuccess) drained(c);
    c->last_flavour = last_flavour;
    c->last_tiles = last_tiles;
    c->cnt_buf = cnt_buf;
    c->cnt_blocks = cnt_blocks;
    c->cnt_offset = cnt_offset;
    c->cnt_pending = false;
    c->last_unmeasured = last_unmeasured;
    c->tm.valid = tm_valid;
    c->ring.head = ring_head;
    for (int i = 0; i < 3; ++i) c->h_counters[i] = counters[i];
    if (rc != VR_OK) return rc;
    VR_HIP(c, sync);

    const size_t idx = (size_t)y * c->W + x;
    float4 px;
    VR_HIP(c, hipMemcpy(&px, c->d_pick + idx, sizeof px, hipMemcpyDeviceToHost));
    std::memset(out, 0, sizeof *out);
    out->alpha = px.w;
    out->depth = 1.0f;
    out->hit = px.w > c->surf_tau ? 1 : 0;  // (an ISO frame's .w is 1 or 0)
    if (!out->hit) return VR_OK;
    (void)hipGetLastError();
    hipLaunchKernelGGL(surface_depth_kernel, dim3(1), dim3(256), 0, c->stream, (const float4*)(c->d_pick + idx), c->d_pick_depth, 1,
                       depth_params(c));
    VR_HIP(c, hipGetLastError());
    VR_HIP(c, hipStreamSynchronize(c->stream));
    VR_HIP(c, hipMemcpy(&out->depth, c->d_pick_depth, sizeof(float), hipMemcpyDeviceToHost));
    const float q[3] = {px.x, px.y, px.z};
    out->world[0] = q[0] - 0.5f;
    out->world[1] = q[1] - 0.5f;
    out->world[2] = (0.5f - q[2]) * 0.5f;
    const int n0[3] = {c->vol[0].nx, c->vol[0].ny, c->vol[0].nz};
    for (int a = 0; a < 3; ++a) {
        out->uvw[a] = q[a];
        const float f = std::floor(q[a] * (float)n0[a]);
        out->voxel[a] = f >= (float)(n0[a] - 1) ? n0[a] - 1 : (f > 0.0f ? (int)f : 0);  // (NaN -> 0)
    }
    const size_t v = ((size_t)out->voxel[2] * (size_t)n0[1] + (size_t)out->voxel[1]) * (size_t)n0[0] + (size_t)out->voxel[0];
    for (int i = 0; i < VR_MAX_VOLUMES; ++i)
        if (c->vol[i].data && c->vol[i].nx == n0[0] && c->vol[i].ny == n0[1] && c->vol[i].nz == n0[2])
            VR_HIP(c, hipMemcpy(out->value[i], c->vol[i].data + v, sizeof(float4), hipMemcpyDeviceToHost));
    return VR_OK;
}

namespace {

// the descriptor's own fields (VR_ERR_INVALID_ARG), then what the context must hold (VR_ERR_NOT_READY)
int check_slice(vr_ctx* c, const vr_slice_desc* d, const void* out, const char* who)
{
    const std::string w(who);
    if (!d || !out) return fail(c, VR_ERR_INVALID_ARG, w + ": the descriptor or the output is NULL");
    if (d->volume_slot < 0 || d->volume_slot >= VR_MAX_VOLUMES) return fail(c, VR_ERR_INVALID_ARG, w + ": bad volume slot");
    if (d->tf_slot < 0 || d->tf_slot >= VR_MAX_TFS) return fail(c, VR_ERR_INVALID_ARG, w + ": bad TF slot");
    if (d->width < 1 || d->width > 16384 || d->height < 1 || d->height > 16384)
        return fail(c, VR_ERR_INVALID_ARG, w + ": the output must be 1 .. 16384 pixels each way");
    if (d->slab_steps < 1 || d->slab_steps > 65536) return fail(c, VR_ERR_INVALID_ARG, w + ": slab_steps must be 1 .. 65536");
    if (d->reduce != VR_SLICE_MAX && d->reduce != VR_SLICE_MIN && d->reduce != VR_SLICE_AVERAGE)
        return fail(c, VR_ERR_INVALID_ARG, w + ": unknown reduction");
    if (d->filter != VR_SLICE_LINEAR && d->filter != VR_SLICE_NEAREST) return fail(c, VR_ERR_INVALID_ARG, w + ": unknown filter");
    if (d->format != VR_SLICE_RGBA32F && d->format != VR_SLICE_BGRA8) return fail(c, VR_ERR_INVALID_ARG, w + ": unknown format");
    if (!c->vol[d->volume_slot].data) return fail(c, VR_ERR_NOT_READY, w + ": volume slot " + std::to_string(d->volume_slot) + " is empty");
    if (!c->tf[d->tf_slot].opacity || !c->tf[d->tf_slot].color)
        return fail(c, VR_ERR_NOT_READY, w + ": TF slot " + std::to_string(d->tf_slot) + " is empty");
    return VR_OK;
}

// One slice launch on `s` (the descriptor has been checked).  It takes the next record slot -- so it is one of the kInFlight launches
// in flight, and its slot's event is what reuse_wait orders a later table edit behind -- but writes records of its own
// (d_slice_counts) and touches none of the march launches' bookkeeping: counters, last flavour, timings, kernel choice, launch order.
int enqueue_slice(vr_ctx* c, const vr_slice_desc& d, void* d_out, hipStream_t s)
{
    VR_HIP(c, hipSetDevice(c->device));
    (void)hipGetLastError();
    if (const int rc = wait_for_edits(c, s)) return rc;
    const int vs = d.volume_slot;
    SliceParams S;
    std::memset(&S, 0, sizeof S);
    S.vol = linear_volume(c, vs);
    if (c->layout_mode == 0) use_bricked_copy(c, vs, S.vol);
    bool off32 = c->vol_bytes[vs] <= 0xFFFFFFFFull;
    if (S.vol.bricked && bricked_grid(S.vol).slots * 16 > 0xFFFFFFFFull) off32 = false;
    S.tf = c->tf[d.tf_slot];
    for (int a = 0; a < 3; ++a) {
        S.origin[a] = d.origin[a];
        S.du[a] = d.du[a];
        S.dv[a] = d.dv[a];
        S.dn[a] = d.dn[a];
    }
    S.width = (int)d.width;
    S.height = (int)d.height;
    S.tiles_x = (int)((d.width + 7u) / 8u);
    S.slab_steps = d.slab_steps;
    S.format = d.format;
    S.out = d_out;
    const unsigned tiles = (unsigned)S.tiles_x * ((d.height + 7u) / 8u);
    // exact skipping by the slot's range records, unless flavour 1 asks for the plain form (the kernels index bricks with 24-bit
    // multiplies and 32-bit byte offsets, as every skipping kernel)
    const DevVolume& v = c->vol[vs];
    S.bnx = skip_bricks(v.nx);
    S.bny = skip_bricks(v.ny);
    S.bnz = skip_bricks(v.nz);
    S.bsx = (float)v.nx * kBrickInv;
    S.bsy = (float)v.ny * kBrickInv;
    S.bsz = (float)v.nz * kBrickInv;
    const int requested = c->flavour == 0 ? c->default_flavour : c->flavour;
    const bool skip = requested != 1 && (long long)S.bnx * S.bny < (1 << 23);
    if (skip) {
        S.vrange = prepare_range(c, s, vs, S.bnx, S.bny, S.bnz, &S.bricks);
        if (!S.vrange) return VR_ERR_HIP;
    }
    // the record slot: the launch that used it last has finished (host wait: the bound on launches in flight); the sort that read that
    // launch's records is waited for on the stream, so that whoever takes the slot next may write them behind this launch's event
    int cb;
    const vr_ctx::OrderSlot* slot_sort;
    if (const int rc = take_record_slot(c, s, 0, &cb, &slot_sort)) return rc;
    if (slot_sort) VR_HIP(c, hipStreamWaitEvent(s, slot_sort->sorted, 0));
    if (tiles > c->slice_counts_cap[cb]) {
        if (c->d_slice_counts[cb]) (void)hipFree(c->d_slice_counts[cb]);  // (its last slice has finished: the slot's event, above)
        c->d_slice_counts[cb] = nullptr;
        c->slice_counts_cap[cb] = 0;
        VR_HIP(c, hipMalloc(&c->d_slice_counts[cb], (size_t)tiles * 3 * sizeof(unsigned long long)));
        c->slice_counts_cap[cb] = tiles;
    }
    S.counts = c->d_slice_counts[cb];
    if (c->arith == VR_ARITH_FUSED) vrf::launch_slice(S, d.reduce, d.filter == VR_SLICE_NEAREST, off32, skip, tiles, s);
    else vr::launch_slice(S, d.reduce, d.filter == VR_SLICE_NEAREST, off32, skip, tiles, s);
    VR_HIP(c, hipGetLastError());
    mark_table_reads(c, d.tf_slot);
    VR_HIP(c, hipEventRecord(c->slot_done[cb], s));
    c->slot_used[cb] = true;
    ++c->order_seq;
    c->slice_buf = cb;
    c->slice_tiles = tiles;
    return VR_OK;
}

}  // namespace

int vr_slice_async(vr_ctx* c, const vr_slice_desc* desc, void* d_out, void* stream)
{
    if (!c) return VR_ERR_INVALID_ARG;
    if (const int rc = check_slice(c, desc, d_out, "vr_slice_async")) return rc;
    return enqueue_slice(c, *desc, d_out, stream ? (hipStream_t)stream : c->stream);
}

int vr_slice_render(vr_ctx* c, const vr_slice_desc* desc, void* out_host)
{
    if (!c) return VR_ERR_INVALID_ARG;
    if (const int rc = check_slice(c, desc, out_host, "vr_slice_render")) return rc;
    VR_HIP(c, hipSetDevice(c->device));
    const size_t bytes = (size_t)desc->width * desc->height * (desc->format == VR_SLICE_BGRA8 ? 4u : 16u);
    // (the buffer's earlier uses were synchronous on this stream; a smaller one is freed by the next draining call)
    if (const int rc = grow(c, &c->d_slice_out, &c->slice_out_cap, bytes, false)) return rc;
    if (const int rc = enqueue_slice(c, *desc, c->d_slice_out, c->stream)) return rc;
    VR_HIP(c, hipMemcpyAsync(out_host, c->d_slice_out, bytes, hipMemcpyDeviceToHost, c->stream));
    VR_HIP(c, hipStreamSynchronize(c->stream));
    return VR_OK;
}

int vr_slice_orthogonal(const vr_ctx* c, int slot, int axis, int index, int thickness, vr_slice_desc* out)
{
    if (!c || !out) return VR_ERR_INVALID_ARG;
    if (slot < 0 || slot >= VR_MAX_VOLUMES || axis < 0 || axis > 2 || thickness < 1 || thickness > 65536) return VR_ERR_INVALID_ARG;
    if (!c->vol[slot].data) return VR_ERR_NOT_READY;
    const int n[3] = {c->vol[slot].nx, c->vol[slot].ny, c->vol[slot].nz};
    if (index < 0 || index >= n[axis]) return VR_ERR_INVALID_ARG;
    const int ua = axis == 0 ? 1 : 0, va = axis == 2 ? 1 : 2;  // the output's x / y axes: (y, z), (x, z), (x, y)
    std::memset(out, 0, sizeof *out);
    out->volume_slot = slot;
    out->tf_slot = 0;
    out->width = (uint32_t)n[ua];
    out->height = (uint32_t)n[va];
    out->origin[ua] = 0.5f / (float)n[ua];
    out->origin[va] = 0.5f / (float)n[va];
    out->origin[axis] = ((float)(index - (thickness - 1) / 2) + 0.5f) / (float)n[axis];
    out->du[ua] = 1.0f / (float)n[ua];
    out->dv[va] = 1.0f / (float)n[va];
    out->dn[axis] = 1.0f / (float)n[axis];
    out->slab_steps = thickness;
    out->reduce = VR_SLICE_MAX;
    out->filter = VR_SLICE_LINEAR;
    out->format = VR_SLICE_RGBA32F;
    return VR_OK;
}

int vr_slice_counters(vr_ctx* c, uint64_t out[3])
{
    if (!c) return VR_ERR_INVALID_ARG;
    if (!out) return fail(c, VR_ERR_INVALID_ARG, "vr_slice_counters: out is NULL");
    out[0] = out[1] = out[2] = 0;
    if (c->slice_buf < 0) return VR_OK;
    VR_HIP(c, hipSetDevice(c->device));
    (void)hipGetLastError();
    // the event behind the slice (or behind a later launch in its record slot), then the context's own stream: the caller's may be gone
    VR_HIP(c, hipEventSynchronize(c->slot_done[c->slice_buf]));
    // (d_counters: every use of it is synchronous on the context's stream, as this one)
    hipLaunchKernelGGL(slice_sum_kernel, dim3(1), dim3(1024), 0, c->stream, (const unsigned long long*)c->d_slice_counts[c->slice_buf],
                       c->slice_tiles, c->d_counters);
    VR_HIP(c, hipGetLastError());
    unsigned long long h[3] = {0, 0, 0};
    VR_HIP(c, hipMemcpyAsync(h, c->d_counters, sizeof h, hipMemcpyDeviceToHost, c->stream));
    VR_HIP(c, hipStreamSynchronize(c->stream));
    for (int i = 0; i < 3; ++i) out[i] = h[i];
    return VR_OK;
}

namespace {

// the descriptor's own fields (VR_ERR_INVALID_ARG), then what the context must hold (VR_ERR_NOT_READY, mismatched mask)
int check_hist(vr_ctx* c, const vr_hist_desc* d, const void* counts, const void* rows, const char* who)
{
    const std::string w(who);
    if (!d || !counts || !rows) return fail(c, VR_ERR_INVALID_ARG, w + ": the descriptor or an output is NULL");
    if (d->volume_slot < 0 || d->volume_slot >= VR_MAX_VOLUMES) return fail(c, VR_ERR_INVALID_ARG, w + ": bad volume slot");
    if (d->mask_slot < -1 || d->mask_slot >= VR_MAX_VOLUMES) return fail(c, VR_ERR_INVALID_ARG, w + ": bad mask slot");
    if (d->channel < 0 || d->channel > 3) return fail(c, VR_ERR_INVALID_ARG, w + ": the channel must be 0 .. 3");
    if (d->bins < 1 || d->bins > VR_HIST_MAX_BINS) return fail(c, VR_ERR_INVALID_ARG, w + ": bins must be 1 .. 65536");
    if (d->out_of_range != VR_HIST_CLAMP && d->out_of_range != VR_HIST_DROP) return fail(c, VR_ERR_INVALID_ARG, w + ": unknown out_of_range policy");
    if (d->rows == 0 || (d->rows >> VR_HIST_ROWS) != 0) return fail(c, VR_ERR_INVALID_ARG, w + ": rows must have a bit of 0 .. 4 set and none above");
    if ((d->rows & ~1u) != 0 && d->mask_slot < 0) return fail(c, VR_ERR_INVALID_ARG, w + ": contour rows need a mask slot");
    const DevVolume& v = c->vol[d->volume_slot];
    if (!v.data) return fail(c, VR_ERR_NOT_READY, w + ": volume slot " + std::to_string(d->volume_slot) + " is empty");
    const int n[3] = {v.nx, v.ny, v.nz};
    for (int a = 0; a < 3; ++a)
        if (d->lo[a] < 0 || d->lo[a] > d->hi[a] || d->hi[a] > n[a]) return fail(c, VR_ERR_INVALID_ARG, w + ": the box must be 0 <= lo <= hi <= n on every axis");
    if (d->mask_slot >= 0) {
        const DevVolume& m = c->vol[d->mask_slot];
        if (!m.data) return fail(c, VR_ERR_NOT_READY, w + ": mask slot " + std::to_string(d->mask_slot) + " is empty");
        if (m.nx != v.nx || m.ny != v.ny || m.nz != v.nz) return fail(c, VR_ERR_INVALID_ARG, w + ": the mask's dimensions differ from the volume's");
    }
    return VR_OK;
}

// One histogram launch on `s` (the descriptor has been checked).  Like a slice it takes the next record slot -- it is one of the
// kInFlight launches in flight -- and touches none of the other launches' bookkeeping.
int enqueue_hist(vr_ctx* c, const vr_hist_desc& d, void* d_counts, void* d_rows, hipStream_t s)
{
    VR_HIP(c, hipSetDevice(c->device));
    (void)hipGetLastError();
    const int vs = d.volume_slot;
    const DevVolume v = linear_volume(c, vs);
    HistParams H;
    std::memset(&H, 0, sizeof H);
    const bool plane = d.channel == 3 && d.mask_slot < 0 && v.dens;
    H.val = plane ? v.dens : reinterpret_cast<const float*>(v.data) + d.channel;
    H.val_stride = plane ? 1 : 4;
    H.mask = d.mask_slot >= 0 ? c->vol[d.mask_slot].data : nullptr;
    H.nx = v.nx;
    H.ny = v.ny;
    H.nz = v.nz;
    unsigned long long units = 1, box = 1;
    for (int a = 0; a < 3; ++a) {
        H.lo[a] = d.lo[a];
        H.hi[a] = d.hi[a];
        H.u0[a] = d.lo[a] >> 2;
        H.un[a] = d.hi[a] > d.lo[a] ? ((d.hi[a] + 3) >> 2) - H.u0[a] : 0;
        units *= (unsigned long long)H.un[a];
        box *= (unsigned long long)(d.hi[a] - d.lo[a]);
    }
    if (box == 0) units = 0;
    if (units > 0xFFFFFFFFull) return fail(c, VR_ERR_UNSUPPORTED, "vr_histogram: the box has 2^32 brick units or more");
    H.units = (unsigned)units;
    H.rows = d.rows;
    H.bins = d.bins;
    H.scale = d.scale;
    H.drop = d.out_of_range == VR_HIST_DROP;
    unsigned n_rows = 0;
    for (int r = 0; r < VR_HIST_ROWS; ++r) n_rows += (d.rows >> r) & 1u;
    const unsigned blocks = units < 4 ? 1u : (units / 4 < kHistBlocks ? (unsigned)(units / 4) : kHistBlocks);
    // the private LDS copy: within the budget, and a workgroup's share of the voxels (its four wavefronts' units) below 2^32 so that
    // no u32 count can wrap; otherwise the kernel adds into the u64 outputs directly
    const unsigned long long per_block = (units + blocks * 4ull - 1) / (blocks * 4ull) * 4ull * 64ull;
    H.lds = (size_t)n_rows * d.bins * sizeof(unsigned) <= kHistLdsBytes && per_block < (1ull << 32);
    const int requested = c->flavour == 0 ? c->default_flavour : c->flavour;
    const bool plain = requested == 1;
    // exact settling by the slot's range records (of .a: channel 3), for the unmasked launch
    if (!plain && d.channel == 3 && d.mask_slot < 0 && units != 0) {
        H.bnx = skip_bricks(v.nx);
        H.bny = skip_bricks(v.ny);
        if (!prepare_range(c, s, vs, H.bnx, H.bny, skip_bricks(v.nz), &H.bricks)) return VR_ERR_HIP;
    }
    int cb;
    const vr_ctx::OrderSlot* slot_sort;
    if (const int rc = take_record_slot(c, s, 0, &cb, &slot_sort)) return rc;
    if (slot_sort) VR_HIP(c, hipStreamWaitEvent(s, slot_sort->sorted, 0));
    if (!c->d_hist_stats[cb]) {
        VR_HIP(c, hipMalloc(&c->d_hist_stats[cb], 3 * sizeof(unsigned long long)));
    }
    VR_HIP(c, hipMemsetAsync(c->d_hist_stats[cb], 0, 3 * sizeof(unsigned long long), s));
    VR_HIP(c, hipMemsetAsync(d_counts, 0, (size_t)VR_HIST_ROWS * d.bins * sizeof(unsigned long long), s));
    VR_HIP(c, hipMemsetAsync(d_rows, 0, VR_HIST_ROWS * sizeof(vr_hist_row), s));
    H.counts = static_cast<unsigned long long*>(d_counts);
    H.row_sums = static_cast<unsigned long long*>(d_rows);
    H.stats = c->d_hist_stats[cb];
    const size_t lds_bytes = H.lds ? (size_t)n_rows * d.bins * sizeof(unsigned) : 0;
    if (plain) hipLaunchKernelGGL(hist_kernel<true>, dim3(blocks), dim3(256), lds_bytes, s, H);
    else hipLaunchKernelGGL(hist_kernel<false>, dim3(blocks), dim3(256), lds_bytes, s, H);
    VR_HIP(c, hipGetLastError());
    VR_HIP(c, hipEventRecord(c->slot_done[cb], s));
    c->slot_used[cb] = true;
    ++c->order_seq;
    c->hist_buf = cb;
    return VR_OK;
}

}  // namespace

int vr_hist_whole(const vr_ctx* c, int slot, uint32_t bins, float scale, vr_hist_desc* out)
{
    if (!c || !out) return VR_ERR_INVALID_ARG;
    if (slot < 0 || slot >= VR_MAX_VOLUMES || bins < 1 || bins > VR_HIST_MAX_BINS) return VR_ERR_INVALID_ARG;
    if (!c->vol[slot].data) return VR_ERR_NOT_READY;
    std::memset(out, 0, sizeof *out);
    out->volume_slot = slot;
    out->channel = 3;
    out->mask_slot = -1;
    out->rows = 1;
    out->bins = bins;
    out->scale = scale;
    out->out_of_range = VR_HIST_CLAMP;
    out->hi[0] = c->vol[slot].nx;
    out->hi[1] = c->vol[slot].ny;
    out->hi[2] = c->vol[slot].nz;
    return VR_OK;
}

int vr_histogram_async(vr_ctx* c, const vr_hist_desc* desc, void* d_counts, void* d_rows, void* stream)
{
    if (!c) return VR_ERR_INVALID_ARG;
    if (const int rc = check_hist(c, desc, d_counts, d_rows, "vr_histogram_async")) return rc;
    return enqueue_hist(c, *desc, d_counts, d_rows, stream ? (hipStream_t)stream : c->stream);
}

int vr_histogram(vr_ctx* c, const vr_hist_desc* desc, uint64_t* counts, vr_hist_row* rows)
{
    if (!c) return VR_ERR_INVALID_ARG;
    if (const int rc = check_hist(c, desc, counts, rows, "vr_histogram")) return rc;
    VR_HIP(c, hipSetDevice(c->device));
    const size_t cbytes = (size_t)VR_HIST_ROWS * desc->bins * sizeof(uint64_t), rbytes = VR_HIST_ROWS * sizeof(vr_hist_row);
    // (the buffer's earlier uses were synchronous on this stream; a smaller one is freed by the next draining call)
    if (const int rc = grow(c, &c->d_hist_out, &c->hist_out_cap, cbytes + rbytes, false)) return rc;
    char* d = static_cast<char*>(c->d_hist_out);
    if (const int rc = enqueue_hist(c, *desc, d, d + cbytes, c->stream)) return rc;
    VR_HIP(c, hipMemcpyAsync(counts, d, cbytes, hipMemcpyDeviceToHost, c->stream));
    VR_HIP(c, hipMemcpyAsync(rows, d + cbytes, rbytes, hipMemcpyDeviceToHost, c->stream));
    VR_HIP(c, hipStreamSynchronize(c->stream));
    return VR_OK;
}

int vr_hist_counters(vr_ctx* c, uint64_t out[3])
{
    if (!c) return VR_ERR_INVALID_ARG;
    if (!out) return fail(c, VR_ERR_INVALID_ARG, "vr_hist_counters: out is NULL");
    out[0] = out[1] = out[2] = 0;
    if (c->hist_buf < 0) return VR_OK;
    VR_HIP(c, hipSetDevice(c->device));
    (void)hipGetLastError();
    // the event behind the histogram (or behind a later launch in its record slot), then the context's own stream
    VR_HIP(c, hipEventSynchronize(c->slot_done[c->hist_buf]));
    unsigned long long h[3] = {0, 0, 0};
    VR_HIP(c, hipMemcpyAsync(h, c->d_hist_stats[c->hist_buf], sizeof h, hipMemcpyDeviceToHost, c->stream));
    VR_HIP(c, hipStreamSynchronize(c->stream));
    for (int i = 0; i < 3; ++i) out[i] = h[i];
    return VR_OK;
}

int vr_set_volume_layout(vr_ctx* c, int mode)
{
    if (!c) return VR_ERR_INVALID_ARG;
    if (mode < 0 || mode > 3) return fail(c, VR_ERR_INVALID_ARG, "vr_set_volume_layout: unknown mode");
    if (mode == 2) return fail(c, VR_ERR_UNSUPPORTED, "vr_set_volume_layout: layout 2 (gradients derived on the fly) was removed");
    c->layout_mode = mode;
    return VR_OK;
}

int vr_volume_layout(vr_ctx* c, int slot, int* flags)
{
    if (!c || !flags) return VR_ERR_INVALID_ARG;
    if (slot < 0 || slot >= VR_MAX_VOLUMES) return fail(c, VR_ERR_INVALID_ARG, "vr_volume_layout: bad slot");
    if (!c->vol[slot].data) return fail(c, VR_ERR_NOT_READY, "vr_volume_layout: volume slot is empty");
    *flags = (c->vol_dens[slot] ? 1 : 0) | (c->vol_grad_derived[slot] ? 2 : 0) | ((c->vol_bricked[slot] && c->layout_mode == 0) ? 8 : 0);
    return VR_OK;
}

int vr_kernel_choice(vr_ctx* c, int flavours[6], float ms_per_launch[6], int* chosen)
{
    if (!c) return VR_ERR_INVALID_ARG;
    if (c->last_unmeasured) {  // (the projections', the isosurface's, the shadowed, the surface and the bounded forms)
        if (chosen) *chosen = -1;
        return 0;
    }
    const vr_ctx::Tune* t = nullptr;
    for (const auto& e : c->tune)
        if (e.key != 0 && e.used != 0 && (!t || e.used > t->used)) t = &e;
    if (chosen) *chosen = t ? t->choice : -1;
    if (!t) return 0;
    for (int i = 0; i < 6; ++i) {
        if (flavours) flavours[i] = i < t->n ? t->cand[i] : 0;
        if (ms_per_launch) ms_per_launch[i] = i < t->n ? t->cost[i] : 0.0f;
    }
    return t->n;
}

int vr_set_kernel_flavour(vr_ctx* c, int flavour)
{
    if (!c) return VR_ERR_INVALID_ARG;
    if (flavour < 0 || flavour > 18) return fail(c, VR_ERR_INVALID_ARG, "vr_set_kernel_flavour: unknown flavour");
    if (removed_flavour(flavour))
        return fail(c, VR_ERR_UNSUPPORTED, "vr_set_kernel_flavour: flavour " + std::to_string(flavour) + " was removed (it lost every A/B)");
    c->flavour = flavour;
    return VR_OK;
}

}  // extern "C"
