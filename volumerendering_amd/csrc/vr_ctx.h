// vr_ctx.h -- the context behind the C ABI (struct vr_ctx), the owners of its HIP resources, its error reporting.
// Part of vr_api.hip's translation unit: included there once, behind the kernel headers and `using namespace vr`.
#pragma once

// ---- owners: move-only, released by their destructors (vr_destroy drains the device, then deletes the context) ---------------------

// Memory that knows its capacity, in elements of T (bytes for void): device memory (DevBuf) or pinned host memory (PinnedBuf).
template <typename T, bool kPinned>
struct Buf {
    T* p = nullptr;
    size_t cap = 0;
    Buf() = default;
    Buf(Buf&& o) noexcept : p(o.p), cap(o.cap) { o.p = nullptr, o.cap = 0; }
    Buf& operator=(Buf&& o) noexcept { return std::swap(p, o.p), std::swap(cap, o.cap), *this; }
    ~Buf() { release(); }
    operator T*() const { return p; }
    void release()
    {
        if (p) (void)(kPinned ? hipHostFree(p) : hipFree(p));
        p = nullptr;
        cap = 0;
    }
    // n elements, the old contents gone; empty (capacity 0) if the allocation fails.  zeroed: pinned memory that the device reports into
    // and the host reads before the first report
    hipError_t reserve(size_t n, bool zeroed = false)
    {
        release();
        const size_t bytes = n * sizeof(std::conditional_t<std::is_void<T>::value, char, T>);
        const hipError_t e = kPinned ? hipHostMalloc((void**)&p, bytes, hipHostMallocDefault) : hipMalloc((void**)&p, bytes);
        if (e != hipSuccess) p = nullptr;
        else if (kPinned && zeroed) std::memset(p, 0, bytes);
        cap = p ? n : 0;
        return e;
    }
    T* detach() { return cap = 0, std::exchange(p, nullptr); }  // hands the memory over (the retire lists)
};
template <typename T> using DevBuf = Buf<T, false>;
template <typename T> using PinnedBuf = Buf<T, true>;

// The device words of a tool and the pinned copy where the host sets them before a call's first kernel and reads them behind its last.
template <typename T>
struct WordsPair {
    DevBuf<T> d;
    PinnedBuf<T> h;
    hipError_t first_use()
    {
        if (!d)
            if (const hipError_t e = d.reserve(1)) return e;
        return h ? hipSuccess : h.reserve(1, true);
    }
    hipError_t push(hipStream_t s) const { return hipMemcpyAsync(d.p, h.p, sizeof(T), hipMemcpyHostToDevice, s); }
    hipError_t pull(hipStream_t s) const { return hipMemcpyAsync(h.p, d.p, sizeof(T), hipMemcpyDeviceToHost, s); }
};

struct Event {
    hipEvent_t e = nullptr;
    Event() = default;
    Event(Event&& o) noexcept : e(o.e) { o.e = nullptr; }
    Event& operator=(Event&& o) noexcept { return std::swap(e, o.e), *this; }
    ~Event() { if (e) (void)hipEventDestroy(e); }
    operator hipEvent_t() const { return e; }
    hipError_t create(unsigned flags = hipEventDefault)
    {
        const hipError_t rc = hipEventCreateWithFlags(&e, flags);
        if (rc != hipSuccess) e = nullptr;
        return rc;
    }
};

struct Stream {
    hipStream_t s = nullptr;
    Stream() = default;
    Stream(Stream&& o) noexcept : s(o.s) { o.s = nullptr; }
    Stream& operator=(Stream&& o) noexcept { return std::swap(s, o.s), *this; }
    ~Stream() { if (s) (void)hipStreamDestroy(s); }
    operator hipStream_t() const { return s; }
    hipError_t create()
    {
        const hipError_t rc = hipStreamCreateWithFlags(&s, hipStreamNonBlocking);
        if (rc != hipSuccess) s = nullptr;
        return rc;
    }
};

// ---- the context's parts -------------------------------------------------------------------------------------------------------------

#include "vr_tuner.h"  // kRing; the measured kernel choice (Trial, Tuner, tune_pick)

constexpr int kInFlight = 8;  // launches that may be in flight at a time (record buffers used in turn; twice the streams, so that
                               // a caller with four frames in flight never blocks on its oldest launch)
constexpr int kStreams = 4;   // vr_stream(): streams for frames in flight
constexpr int kOrderRing = 16;  // launch-order buffers: written behind launch k, read by launches k+3 .. k+6 only (see enqueue_render)
constexpr int kGen = 4;         // generations of each table and of the distance field (vr_tf_upload_*_async)
constexpr int kStage = 8;       // pinned staging buffers of the asynchronous table edits
constexpr int kEditSeen = 8;    // streams remembered to have waited for something built on another stream (BuiltOn)
constexpr int kShadowRing = 4;  // light volumes kept (vr_set_shadows): one per key, the least recently used one rebuilt

// A device buffer of one generation (capacity in bytes): written by an edit, read by the launches that captured it while it was
// current, on any streams.  Rewritten only behind every one of them (reuse_wait): reader[k] is the order_seq of the latest launch in
// record slot k (seq % kInFlight) that read it, -1 if none since it was last written.
struct GenBuf : DevBuf<void> {
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
    Event ev;
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
    // the next build, on s, comes after this one: a wait of its own, whether or not a launch on s has waited already
    hipError_t rebuild_behind(hipStream_t s) { return pending && s != stream ? hipStreamWaitEvent(s, ev, 0) : hipSuccess; }
};

// The transfer-function tables of one slot, [kind]: 0 opacity, 1 colour.  dev is what the launches after an upload see (DevTF layout:
// the first and the last texel once more at either end); the flags are what skipping derives from the tables.
struct TfSlot {
    DevTF dev = {};
    GenBuf buf[2][kGen];  // the table's generations, cur[kind] the one in use
    int cur[2] = {};
    int zero_prefix = -1;  // of the opacity table, -1 if none / not finite
    bool opacity_finite = false, color_finite = false;
    GenBuf& current(int kind) { return buf[kind][cur[kind]]; }
    GenBuf& next(int kind) { return buf[kind][(cur[kind] + 1) % kGen]; }
    void advance(int kind) { cur[kind] = (cur[kind] + 1) % kGen; }
    // the host state as the launches after an upload of `table` into current(kind) see it: its resolution, its flags (vr_api_tf.h)
    void set_current(const float* table, uint32_t R, bool is_color);
    // launch `seq` (whose slot event is recorded behind it) reads the current generations
    void mark_reads(unsigned long long seq)
    {
        for (int k = 0; k < 2; ++k)
            if (current(k).p) current(k).reader[seq % kInFlight] = (long long)seq;
    }
};

// Asynchronous table edits (vr_tf_upload_*_async): each records order.ev on its stream, behind the one before it; a launch on another
// stream waits for it once, nothing once a draining call has seen it.  stage: pinned copies of the edited tables, used in turn.
struct TfEdits {
    BuiltOn order;
    struct Stage {  // in the DevTF layout (capacity in bytes); reused behind its copy's event
        PinnedBuf<void> h;
        Event done;
        bool used = false;
    } stage[kStage];
    unsigned stage_next = 0;
};

// What a distance field was built for.
struct FieldKey {
    const void* records = nullptr;
    unsigned long long epoch = ~0ull;  // vr_ctx::brick_epoch
    int zero_prefix = -2, res = 0, use_rgb = -1;
    bool operator==(const FieldKey& o) const
    {
        return records == o.records && epoch == o.epoch && zero_prefix == o.zero_prefix && res == o.res && use_rgb == o.use_rgb;
    }
};

// Exact empty-space skipping (prepare_skip, vr_api_tf.h): VOLUME_MASK's merged records, the distance field over the records in use with
// its generations, and what each build reports about it.
struct SkipField {
    DevBuf<float2> merged_bricks;         // VOLUME_MASK: (CT density max, mask rgb max), rebuilt when stale
    bool merged_stale = true;
    unsigned char* brick_dist = nullptr;  // the field in use (field[cur]), built for `key`
    GenBuf field[kGen];                   // its generations (an asynchronous opacity edit builds the next one)
    int cur = 0;
    DevBuf<unsigned char> tmp;            // the y pass's output, the z pass's input
    int bn[3] = {0, 0, 0};                // bricks per axis of the field
    FieldKey key;
    // What each build reports (SkipSummary, pinned, one per generation) and the device words it accumulates in.  pending: the count and
    // box of build `gen` have not reached the host yet -- launches use the unbounded box meanwhile.
    PinnedBuf<SkipSummary> h_sum;
    DevBuf<SkipSumDev> d_sum;
    unsigned long long gen = 0;
    bool pending = false;
    int box[6] = {0x7fffffff, 0x7fffffff, 0x7fffffff, -1, -1, -1};  // of the field in use, once known (vr_skip_field)
    unsigned long long active = 0;
    long long unbounded_launches = 0;
    double active_fraction = 1.0;  // share of bricks that are not inert
    // min / max of n . b over the active bricks along the hull's 13 directions (vr_skip_hull; the first three are the box; INT_MAX /
    // INT_MIN when there is none), and the plane pairs the launches get for them (MarchParams::hull)
    int hull_lo[kHullDirs], hull_hi[kHullDirs];
    HullPlanes hull = hull_unbounded();
    // generation b holds a field of bn_ bricks freshly built for k: it is the one in use, its count and box on their way
    void publish(int b, const FieldKey& k, const int bn_[3])
    {
        field[b].written();
        cur = b;
        brick_dist = (unsigned char*)field[b].p;
        pending = true;
        key = k;
        for (int a = 0; a < 3; ++a) bn[a] = bn_[a];
    }
    // The count and box of the field in use, once its build has reported them (pinned, generation first): the share of active bricks
    // (which the kernel choice reads) and the box of the active bricks in uvw with one brick of margin: brick b of axis a holds the
    // positions with p * bs - kBrickHalf in [b, b + 1), the first and the last brick those beyond them as well.
    void adopt(const float bs[3])
    {
        if (!pending) return;
        const volatile SkipSummary& h = h_sum[cur];
        if (h.gen != gen) return;
        __atomic_thread_fence(__ATOMIC_ACQUIRE);
        const long long nb = (long long)bn[0] * bn[1] * bn[2];
        active = h.count;
        active_fraction = nb > 0 ? (double)h.count / (double)nb : 1.0;
        for (int a = 0; a < 6; ++a) box[a] = h.box[a];
        if (h.count == 0) {  // (no active brick: every pair inverted, hull_inverted)
            for (int d = 0; d < kHullDirs; ++d) {
                hull_lo[d] = 0x7fffffff;
                hull_hi[d] = -0x7fffffff - 1;
            }
            hull = hull_inverted();
        } else {
            for (int d = 0; d < kHullDirs; ++d) {
                hull_lo[d] = d < kHullAxes ? box[d] : h.hull_lo[d - kHullAxes];
                hull_hi[d] = d < kHullAxes ? box[3 + d] : h.hull_hi[d - kHullAxes];
            }
            hull = hull_bounds(hull_lo, hull_hi, bs, kBrickHalf);
        }
        pending = false;
    }
    // the hull a launch gets: unbounded (the kernels only prune with it) while the count and planes of a rebuild are on their way
    HullPlanes launch_box() const { return pending ? hull_unbounded() : hull; }
};

// The kernel-time ring (vr_kernel_times): launch number `head` (LastLaunch::ring_head) records itself in slot(head) -- with the events
// k0 / k1 around it, or, a launch with a sort behind it, from its own records in the pinned words that sort fills.  Launch numbers only
// grow: vr_reset_kernel_times moves `reported_from` up to the head, so that vr_kernel_times reports nothing older, and leaves the slots
// and the numbers of the trials' launches (Trial::launch) alone.
struct KernelRing {
    long long reported_from = 0;           // vr_kernel_times reports launches reported_from .. head - 1 (the last kRing of them)
    Event k0[kRing], k1[kRing];
    bool by_events[kRing] = {};            // launch q was timed with the events (no sort behind it)
    PinnedBuf<unsigned long long> h_span;  // duration of launch q in 100 MHz ticks + 1, from its records (0 = not known)
    PinnedBuf<unsigned long long> h_end;   // end of launch q's last workgroup on the 100 MHz device clock, | 1 (0 = not known)
    static int slot(long long head) { return (int)(head % kRing); }
    void begin(int q, bool events)  // a launch takes slot q: nothing is known about it yet
    {
        by_events[q] = events;
        if (h_span) h_span[q] = 0;
        if (h_end) h_end[q] = 0;
    }
    unsigned long long span_ticks(int q) const { return *(volatile unsigned long long*)&h_span[q]; }
    unsigned long long end_ticks(int q) const { return *(volatile unsigned long long*)&h_end[q]; }
};

// Longest-first launch order (MarchParams::order): behind every march launch one small kernel sorts that launch's blocks by their
// longest ray chain; a later launch of the same shape takes its blocks in that order.
struct OrderSlot {
    DevBuf<unsigned> buf;
    hipStream_t stream = nullptr;
    Event sorted;
    unsigned long long key = 0, seq = 0;
    unsigned long long scene_key = 0;  // what the launch rendered, whatever kernel form it took (the chain length's key)
    bool valid = false;
};
struct LaunchOrder {
    OrderSlot ring[kOrderRing];    // launch seq sorts into ring[seq % kOrderRing]
    Stream stream;                 // the sorts run here, behind their launch's event: never on a frame's critical path
    PinnedBuf<unsigned> h_chain;   // one word per ring slot: longest ray chain + 1 of that launch (0 = not known yet)
    // the longest ray chain + 1 of the most recent launch of scene shape skey whose sort has reported (written to pinned memory by the
    // launch-order sort; read without synchronising, 0 = not known)
    unsigned last_chain(unsigned long long skey) const
    {
        unsigned chain = 0;
        if (!h_chain) return chain;
        unsigned long long best_seq = 0;
        for (int i = 0; i < kOrderRing; ++i) {
            const unsigned v = *(volatile unsigned*)&h_chain[i];
            if (v != 0 && ring[i].scene_key == skey && ring[i].seq + 1 > best_seq) {
                best_seq = ring[i].seq + 1;
                chain = v;
            }
        }
        return chain;
    }
    // the most recent sort of shape okey that is `age` or `age` + 1 launches old when launch `seq` is enqueued (wait_for_order)
    const OrderSlot* best(unsigned long long okey, unsigned long long seq, unsigned long long age) const
    {
        const OrderSlot* b = nullptr;
        for (const auto& o : ring)
            if (o.valid && o.key == okey && o.seq + age + 1 >= seq && o.seq + age <= seq && (!b || o.seq > b->seq)) b = &o;
        return b;
    }
};

// Shadows of the lit shader (vr_set_shadows, vr_shadow.h): the setting, and a ring of light volumes, one per key.  A launch whose key
// matches an entry reads it (waiting once per stream for its build); otherwise it builds the least recently used entry on its own
// stream, behind every launch still reading it (buf.reader, as the table generations).  A volume change drains the device and
// empties the ring.
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
};
struct Shadows {
    int div = 0;         // 0 = off; 1, 2, 4, 8 = voxels per light-volume texel and axis
    float sigma = 1.0f;  // opacity scale
    ShadowVol ring[kShadowRing];
    unsigned long long clock = 0;
    int cur = -1;  // the entry the launch being enqueued reads (mark_reads)
    // the entry of `key` (*build = false), else the least recently used one, to be built (*build = true)
    int entry(const ShadowKey& key, bool* build) const
    {
        int e = -1, lru = 0;
        for (int i = 0; i < kShadowRing; ++i) {
            if (ring[i].valid && ring[i].key == key) e = i;
            if (ring[i].used < ring[lru].used) lru = i;
        }
        *build = e < 0;
        return *build ? lru : e;
    }
};

// A record slot: what launch order_seq takes for itself, k = order_seq % kInFlight (claim_slot), and gives back behind its kernel
// (finish_slot).  Several frames can be in flight on different streams (the next ones fill the machine while the first one's long rays
// drain); a march, a slice and a histogram each keep records of their own in the slot and leave the others' alone.
struct RecordSlot {
    Event done;                               // recorded behind the launch that last used the slot (any stream)
    bool used = false;
    DevBuf<unsigned long long> block_counts;  // march: per-workgroup records (store_block_counts), kBlockRecord words per block
    bool pw_heads_dirty = false;              // the slot's last persistent launch had no sort behind it to clear its heads (d_pw_heads)
    DevBuf<unsigned long long> slice_counts;  // slice views: the wavefront records, three words per workgroup
    DevBuf<unsigned long long> hist_stats;    // histograms: the three counters
};

// A volume slot: the vec4 voxels as uploaded and what refresh_bricks derives from them.
struct VolumeSlot {
    DevVolume vol = {};        // the kernels' view (vol.data = voxels, once an upload has succeeded)
    DevBuf<float4> voxels;
    size_t bytes() const { return voxels.cap * sizeof(float4); }
    DevBuf<float2> bricks;     // per brick: (max density, max(r,g,b)) -- empty-space skipping
    DevBuf<float> dens;        // scalar density plane (DevVolume::dens)
    DevBuf<float4> bricked;    // the voxels again in 4 x 4 x 4 bricks (DevVolume::bricked), what the march kernels gather from (in slots:
                               // bricks x 64)
    DevBuf<float> bdens;       // ... and their density plane in the same order
    bool grad_derived = false;  // .rgb verified to be PreComputeGradient(false) of .a, bit for bit
    // Intensity projections (vr_proj.h), the isosurface (vr_iso.h) and slice views (vr_slice.h): (min, max) of the slot per
    // empty-space brick and over the whole volume ([0]: what the projections and the isosurface read), rebuilt on the launch's stream
    // by the first skipping launch that reads them after a volume change (proj_epoch = the brick_epoch they were built at).  Launches
    // on other streams wait once for the event behind the build (proj_built).
    DevBuf<float2> proj_rec;
    DevBuf<float2> proj_range;
    unsigned long long proj_epoch = ~0ull;
    BuiltOn proj_built;
};

// A voxel tool's report on its last call: three counters, and up to four phases (a mask tool's three and refresh_bricks) timed between
// five events.  open_report and close_report (vr_api_tools.h) begin and end it; a data call that writes no slot marks its events through
// Phases.
struct ToolReport {
    Event ev[5];
    unsigned long long counters[3] = {0, 0, 0};
    float ms[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    // the counters of a tool that computes a part of its box and settles the rest
    void computed_of_box(unsigned long long box, unsigned long long computed)
    {
        counters[0] = box, counters[1] = computed, counters[2] = box - computed;
    }
};

// Region growing (vr_segment_grow, vr_grow.h): the working buffers of the last grow, grown on demand; what vr_grow_counters and
// vr_grow_timing report.
struct GrowState {
    DevBuf<unsigned long long> words;  // the bit-bricks: Q of every brick, then R of every brick
    DevBuf<unsigned> lists;            // per brick: the round stamp, then the frontier's two lists
    WordsPair<GrowWords> io;           // counters, result and the rounds' words
    ToolReport report;                 // phases: classify + seed, propagate, write, refresh_bricks
};

// Mask morphology (vr_mask_morph, vr_morph.h): what vr_morph_counters and vr_morph_timing report.  Of vr_ctx::bit_row_scratch it takes three
// buffers: the packed operand and the two a dilation pass writes in turn.
struct MorphState {
    DevBuf<unsigned> rows;             // the element's rows ...
    PinnedBuf<unsigned> h_rows;        // ... and where the host sorts them
    WordsPair<MorphWords> io;          // the counts and bounding boxes
    ToolReport report;                 // phases: pack, morphology, write, refresh_bricks
};

// Distance maps (vr_mask_distance, vr_dist.h): the working buffers of the last call, grown on demand; what vr_dist_counters and
// vr_dist_timing report.  Of vr_ctx::bit_row_scratch it takes two buffers: the packed contour and the packed probe.
struct DistState {
    DevBuf<unsigned long long> d2[2];    // the OUTSIDE and the INSIDE field: one word per voxel of the field's region
    DevBuf<unsigned long long> stack_g;  // the envelope stacks of a line pass, one entry per voxel of the larger region ...
    DevBuf<unsigned> stack_st;           // ... (vr_dist.h: DistLine)
    WordsPair<DistWords> io;             // the counts, the bounding box and the probe's range
    ToolReport report;                   // phases: pack, distance passes, write, refresh_bricks
};

// Polygon rasterisation (vr_mask_polygons, vr_raster.h): the working buffers of the last call, grown on demand; what
// vr_polygons_counters and vr_polygons_timing report.  Of vr_ctx::bit_row_scratch it takes four buffers: R_k of every contour.
struct RasterState {
    DevBuf<unsigned char> d_stage;       // the points, the polygons that are rasterised and the work items, one behind the other ...
    PinnedBuf<unsigned char> h_stage;    // ... and where the host puts them together
    WordsPair<RasterWords> io;           // the counts and bounding boxes
    ToolReport report;                   // phases: upload, raster, write, refresh_bricks
};

// Contour tracing (vr_mask_outlines, vr_outline.h): the working buffers of the last call, grown on demand; what vr_outlines_counters
// and vr_outlines_timing report.  Of vr_ctx::bit_row_scratch it takes one buffer per contour traced.
struct OutlineState {
    DevBuf<ulonglong2> masks;            // per vertex word: the vertices with one corner, with two
    DevBuf<unsigned> base;               // per vertex word: its corners, then the corners before it
    DevBuf<unsigned> pred, meta;         // per corner node: the node before it on its loop; its slice and contour
    DevBuf<int2> pt;                     // ... its point
    DevBuf<uint4> st[2];                 // ... (leader, rank, jump) of the doubling rounds, written in turn; the idle one takes the output
    DevBuf<unsigned> pidx, pcount;       // per node: the polygons led by smaller nodes; per polygon: its points, then its first point
    WordsPair<OutlineWords> io;          // the totals, the areas, the rounds' outcomes
    ToolReport report;                   // phases: pack, corners + scan + link, doubling rounds, emit + copy back
};

// Connected components (vr_mask_components, vr_comp.h): the working buffers of the last call, grown on demand; what
// vr_components_counters and vr_components_timing report.  Of vr_ctx::bit_row_scratch it takes two buffers: S and R.
struct CompState {
    DevBuf<unsigned> base;               // per word of the box: the runs that start in it, then the nodes before it
    DevBuf<unsigned> parent, root;       // per node: the union-find forest, then the roots before it; its root
    DevBuf<unsigned> row, ab;            // ... its row of the box, its first and last x
    DevBuf<vr_component> table;          // per component
    DevBuf<unsigned> sel;                // ... it is selected
    DevBuf<unsigned long long> pass;     // ... its voxels if it passes the filters (keep_largest: the host picks the winners from a copy)
    WordsPair<CompWords> io;             // the totals, the pairs, the counts and bounding boxes
    ToolReport report;                   // phases: pack, runs + scan + merge + flatten, numbering .. copy back, refresh_bricks
};

// Resampling (vr_volume_resample, vr_resample.h): what vr_resample_counters and vr_resample_timing report.
struct ResampleState {
    WordsPair<ResampleWords> io;         // the inside count, its bounding box, the loaded voxels
    ToolReport report;                   // phases: the source's range records, the kernel, the result words, refresh_bricks
};

// Surface extraction (vr_volume_mesh, vr_mesh.h): the working buffers of the last call, grown on demand; what vr_mesh_counters and
// vr_mesh_timing report.  Of vr_ctx::bit_row_scratch it takes one buffer: the lattice rows of the "inside" bits.
struct MeshState {
    DevBuf<unsigned long long> masks;    // per lattice word: the cells that emit, the seven crossing masks
    DevBuf<unsigned> vbase, tbase;       // per lattice word: its vertices / triangles, then those before it
    DevBuf<float> vertices;              // the output, three per vertex ...
    DevBuf<unsigned> triangles;          // ... and three per triangle
    WordsPair<MeshWords> io;             // the counters, the totals, the emitting cells' box
    ToolReport report;                   // phases: pack, counts + scans, vertex emit, triangle emit + copy back (counters: the first three)
    unsigned long long active_cells = 0; // vr_mesh_counters' fourth
};

// Separable filters (vr_volume_filter, vr_filter.h): the working buffers of the last call, grown on demand; what vr_filter_counters and
// vr_filter_timing report.
struct FilterState {
    DevBuf<float> field[2];              // the fields the passes write in turn: the first pass' region, the second pass' region
    WordsPair<FilterWords> io;           // the non-finite count, the least and greatest finite value
    ToolReport report;                   // phases: the first pass, the remaining passes, write + result words, refresh_bricks
};

// Rank filters (vr_volume_rank, vr_rank.h): the working field of the last call, grown on demand; what vr_rank_counters and
// vr_rank_timing report.
struct RankState {
    DevBuf<unsigned> field;              // the selected bit pattern of every voxel of the box
    WordsPair<RankWords> io;             // the non-finite and changed counts, the least and greatest finite value
    ToolReport report;                   // phases: the selection kernel, further ones (none), write + result words, refresh_bricks
};

// The gamma index (vr_volume_gamma, vr_gamma.h): the offset table and the working field of the last call, grown on demand; what
// vr_gamma_counters and vr_gamma_timing report.
struct GammaState {
    std::vector<GammaEntry> entries;     // the admitted offsets as the host built them (alive until the upload has completed) ...
    DevBuf<GammaEntry> table;            // ... and on the device
    DevBuf<uint2> field;                 // the bits to store and the flags of every voxel of the box
    WordsPair<GammaWords> io;            // the evaluated, passed and non-finite counts, the greatest finite value
    ToolReport report;                   // phases: the search kernel, further ones (none), write + result words, refresh_bricks
    bool lds_raised = false;             // the default form's kernels may take their largest tile of dynamic LDS
};

// What the reporting calls (vr_last_counters, vr_last_kernel_flavour, vr_last_timing, vr_kernel_times, vr_kernel_choice,
// vr_download_tiles, vr_last_block_trace) read about the most recent march launch.  vr_pick copies it out and back as one value.
struct LastLaunch {
    int flavour = 0;           // the flavour the launch resolved to
    bool unmeasured = false;   // its family is never measured (KernelForm::measured): vr_kernel_choice reports no candidates
    int tiles = 0;             // tiles rendered by the last vr_render_tiles
    int cnt_buf = 0;           // the record slot the launch wrote
    int cnt_blocks = 0;
    size_t cnt_offset = 0;     // ... and where in that buffer the records of its last frame start (u64 words)
    bool cnt_pending = false;  // its block counts are not summed / copied to h_counters yet
    bool timed = false;        // it recorded Timing's events (vr_last_timing)
    long long ring_head = 0;   // march launches recorded in the KernelRing since the context was created: the number the next one takes
                               // (never rewound by vr_reset_kernel_times -- KernelRing::reported_from; the tuner's trials name launches by it)
};

// One march launch as its caller asks for it: ONE frame with the context's uniforms into `out` (nullptr -> ctx-owned buffer), or, with
// batch_u / batch_out, n_frames (2 .. kBatchMax) frames of the same scene, each with its own uniforms and output buffer.
struct RenderRequest {
    int variant = 0, rank = 0, world = 1;
    bool packed = false, frame_events = false;
    float4* out = nullptr;
    hipStream_t stream = nullptr;
    int n_frames = 1;
    const vr_uniforms* batch_u = nullptr;
    void* const* batch_out = nullptr;
    int pick_px[2] = {-1, -1};  // vr_pick: the pixel the launch is confined to (pick_px[0] < 0: none)
    // derived once from the request and the context's settings (check_render_args)
    bool surface = false;  // surface-position output (vr_set_output; a pick launch whatever the setting)
    bool bounded = false;  // between ray bounds (vr_set_ray_bounds; a pick launch ignores them)
};

struct vr_ctx {
    int device = 0;
    uint32_t W = 0, H = 0;
    Stream stream;
    VolumeSlot vols[VR_MAX_VOLUMES];
    int arith = VR_ARITH_SEPARATE;             // vr_set_arithmetic
    int layout_mode = 0;                       // vr_set_volume_layout: 0 bricked copy + its density plane, 1 vec4 voxels only,
                                               // 3 x-fastest voxels + density plane (2, gradients on the fly, was removed)
    unsigned long long brick_epoch = 0;        // bumped whenever any brick table changes
    SkipField skip;                            // exact empty-space skipping: the distance field, its count and box
    TfSlot tf[VR_MAX_TFS];
    unsigned long long tf_epoch = 0;           // bumped by every table upload
    unsigned long long opacity_edits = 0;      // bumped by every upload of TF slot 0's opacity table, synchronous or not (ShadowKey's content)
    TfEdits edits;                             // the asynchronous ones: their order and staging
    std::vector<void*> retired_dev, retired_host;  // replaced on a non-blocking path: freed by the next draining call (drained)
    vr_uniforms u = {};
    bool have_uniforms = false;
    DevBuf<float4> d_frame;
    DevBuf<float4> d_tiles;
    DevBuf<uint32_t> d_present;
    DevBuf<unsigned long long> d_counters;  // [3] composited, covered, fetched
    RecordSlot slot[kInFlight];
    DevBuf<unsigned> d_pw_heads;  // queue heads of the persistent-wavefront kernel: kInFlight x 8 heads, 256 B apart
    unsigned long long order_seq = 0;  // launches enqueued: record slot order_seq % kInFlight, order slot order_seq % kOrderRing
    LaunchOrder order;
    KernelRing ring;
    Tuner tuner;
    int frames_in_flight = 1;                 // vr_hint_frames_in_flight: frames the caller keeps in flight on different streams
    Stream flight[kStreams];  // vr_stream(): streams probed to run side by side (created on first use)
    int n_flight = 0;
    LastLaunch last;
    bool event_timing = false;                 // vr_set_kernel_timing(VR_TIMING_EVENTS): time every launch with HIP events
    PinnedBuf<unsigned long long> h_counters;  // [3]: the last launch's block counts summed (fetch_counters)
    struct {  // vr_last_timing's events (last.timed: whether the last launch recorded them)
        Event ev_begin, ev_k0, ev_k1, ev_end;
    } tm;
    int flavour = 0;
    int n_cus = 256;          // compute units of the device
    int default_flavour = 0;  // what flavour 0 resolves to (experiment knob VR_EXP_FLAVOUR)
    unsigned p2_window = 0;   // flavours 16 / 17: records per gather window (VR_EXP_P2_WINDOW: the moving window of volumes >= 4 GiB, forced
                              // onto small volumes by the tests; 0 = what the hardware reaches, just below 4 GiB)
    // Slice views (vr_slice_async): a slice takes a record slot like every launch and leaves the march launches' records, counters
    // and timings alone; which slot the last slice wrote (vr_slice_counters)
    int slice_buf = -1;
    unsigned slice_tiles = 0;
    DevBuf<void> d_slice_out;  // vr_slice_render's device output (grown on demand, bytes)
    // Histograms (vr_histogram_async): a histogram takes a record slot like a slice, and leaves every other launch's bookkeeping
    // alone; which slot the last histogram wrote (vr_hist_counters), and vr_histogram's device outputs (grown on demand, bytes)
    int hist_buf = -1;
    DevBuf<void> d_hist_out;
    float iso = 0.5f;        // VR_VARIANT_ISO's level (vr_set_iso_value), copied into MarchParams::iso at enqueue
    Shadows shadows;         // vr_set_shadows: the setting and the light volumes
    // Surface-position output (vr_set_output, vr_surf.h): the setting and the threshold, both captured at enqueue; vr_pick's frame
    // (allocated on first use, freed with the viewport's buffers)
    int output = VR_OUTPUT_COLOR;
    float surf_tau = 0.5f;
    DevBuf<float4> d_pick;
    DevBuf<float> d_pick_depth;
    // Per-pixel ray bounds (vr_set_ray_bounds, vr_bound.h): the caller's depth buffers, W*H floats each (nullptr: no bound on that side);
    // captured at enqueue, dropped by vr_resize
    const float* d_near = nullptr;
    const float* d_far = nullptr;
    GrowState grow;  // region growing (vr_segment_grow)
    // The bit-row scratch of the five mask tools below (vr_bitrows.h), grown to the most words a call has asked for.  Each call drains
    // the device, zeroes the buffers it takes before it reads them and is synchronous on return: no two uses are ever live.
    DevBuf<unsigned long long> bit_row_scratch;
    // The tile sums of a prefix scan (tool_scan, vr_api_tools.h), grown to the most tiles a scan has had: contour tracing, connected
    // components and surface extraction take it, one scan after the other.  Every one of them has drained the device before its first
    // scan, and all scans run on the context's stream; a regrow frees the old buffer with hipFree, which waits for the scans already
    // on the stream.  So no scan ever reads another's sums.
    DevBuf<unsigned long long> scan_sums;
    MorphState morph;  // mask morphology (vr_mask_morph)
    DistState dist;    // distance maps (vr_mask_distance)
    RasterState raster;  // polygon rasterisation (vr_mask_polygons)
    OutlineState outline;  // contour tracing (vr_mask_outlines)
    CompState comp;  // connected components (vr_mask_components)
    ResampleState resample;  // resampling onto another grid (vr_volume_resample)
    MeshState mesh;  // surface extraction (vr_volume_mesh)
    FilterState filter;  // separable filters of a channel (vr_volume_filter)
    RankState rank;  // rank filters of a channel (vr_volume_rank)
    GammaState gamma;  // the gamma index of two dose channels (vr_volume_gamma)
    std::string err;
};

namespace {

thread_local std::string g_create_error;

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
                        std::string(#call) + " (" __FILE_NAME__ ":" + std::to_string(__LINE__) + "): " + hipGetErrorString(e__));            \
    } while (0)

// After a hipDeviceSynchronize: every asynchronous edit has completed, and what they replaced can be freed.
void drained(vr_ctx* c)
{
    for (void* p : c->retired_dev) (void)hipFree(p);
    for (void* p : c->retired_host) (void)hipHostFree(p);
    c->retired_dev.clear();
    c->retired_host.clear();
    c->edits.order.pending = false;
    for (auto& v : c->vols) v.proj_built.pending = false;
    for (auto& e : c->shadows.ring) e.built.pending = false;
}

// Waits for everything on the device, the launches on the caller's streams included; nothing is in flight after it.
int drain(vr_ctx* c)
{
    VR_HIP(c, hipSetDevice(c->device));
    VR_HIP(c, hipDeviceSynchronize());
    drained(c);
    return VR_OK;
}

// Grows a buffer to n elements.  `drain`: nothing is in flight, the old memory is freed; otherwise it waits for the next draining call.
template <typename T>
int grow(vr_ctx* c, DevBuf<T>& b, size_t n, bool drain)
{
    if (n <= b.cap) return VR_OK;
    if (b.p && !drain) c->retired_dev.push_back(b.detach());
    VR_HIP(c, b.reserve(n));
    return VR_OK;
}

}  // namespace
