// vr_api_tf.h -- the transfer-function tables (TfSlot, TfEdits): uploads, generations and asynchronous edits, and what skipping derives
// from the opacity table (SkipField: distance field, active box: prepare_skip).  Part of vr_api.hip's translation unit.
#pragma once

namespace {

// Before `s` rewrites generation b: every launch that read it must have finished, whatever its stream (launches on different
// streams finish in any order).  A reader fewer than kInFlight launches old still owns its record slot's event: s waits for it on
// the device, one wait per such slot.  An older one was waited for on the host by the claim_slot that reused its slot.
int reuse_wait(vr_ctx* c, hipStream_t s, const GenBuf& b)
{
    for (int k = 0; k < kInFlight; ++k)
        if (b.reader[k] >= 0 && (unsigned long long)b.reader[k] + kInFlight >= c->order_seq)
            VR_HIP(c, hipStreamWaitEvent(s, c->slot[k].done, 0));
    return VR_OK;
}

// The reads of a march launch (enqueued as launch order_seq, whose slot event is recorded behind it): the current generations.
void mark_reads(vr_ctx* c, const MarchParams& P)
{
    for (auto& t : c->tf) t.mark_reads(c->order_seq);
    if (P.brick_dist) c->skip.field[c->skip.cur].reader[c->order_seq % kInFlight] = (long long)c->order_seq;
    if (c->shadows.cur >= 0) c->shadows.ring[c->shadows.cur].buf.reader[c->order_seq % kInFlight] = (long long)c->order_seq;
}

// The distance field for `k` (records of bn bricks) into generation `slot` on `s`: the active bricks, the x, y and z passes
// (vr_skipfield.h), the count and box of build `gen` into h_sum[slot].  F.tmp holds at least bn[0] * bn[1] * bn[2] bytes.
int build_field(vr_ctx* c, hipStream_t s, const FieldKey& k, const int bn[3], int slot, unsigned long long gen)
{
    SkipField& F = c->skip;
    unsigned char* field = (unsigned char*)F.field[slot].p;
    const int nb = bn[0] * bn[1] * bn[2];
    hipLaunchKernelGGL(brick_active_kernel, dim3((unsigned)((nb + 255) / 256)), dim3(256), 0, s, (const float2*)k.records, field, nb, k.use_rgb,
                       k.zero_prefix, k.res);
    const long long waves = (long long)((bn[0] + 63) >> 6) * bn[1] * bn[2];
    hipLaunchKernelGGL(brick_dist_x_kernel, dim3((unsigned)((waves + 3) / 4)), dim3(256), 0, s, field, bn[0], bn[1] * bn[2]);
    const unsigned tx = (unsigned)((bn[0] + kDistCols - 1) / kDistCols);
    hipLaunchKernelGGL((brick_dist_axis_kernel<false>), dim3(tx, (unsigned)((bn[1] + kDistRows - 1) / kDistRows), (unsigned)bn[2]), dim3(256),
                       0, s, field, F.tmp, bn[0], bn[1], (size_t)bn[0], (size_t)bn[0] * bn[1], (SkipSumDev*)nullptr,
                       (SkipSummary*)nullptr, 0ull);
    hipLaunchKernelGGL((brick_dist_axis_kernel<true>), dim3(tx, (unsigned)((bn[2] + kDistRows - 1) / kDistRows), (unsigned)bn[1]), dim3(256),
                       0, s, F.tmp, field, bn[0], bn[2], (size_t)bn[0] * bn[1], (size_t)bn[0], F.d_sum + slot, F.h_sum + slot, gen);
    VR_HIP(c, hipGetLastError());
    return VR_OK;
}

// Exact empty-space skipping (E.can_skip): fills P's brick fields from c, and rebuilds what is stale of the merged mask records, the
// distance field, the share of active bricks (active_fraction, which the kernel choice reads) and the box of the active bricks.
int prepare_skip(vr_ctx* c, int variant, hipStream_t s, MarchParams& P)
{
    SkipField& F = c->skip;
    const int sv = variant == VR_VARIANT_VOLUME_MASK ? 2 : 0;
    fill_brick_grid(P, sv, c->vols[sv].vol);
    P.tf_zero_prefix = c->tf[0].zero_prefix;
    P.bricks = c->vols[sv].bricks;
    P.use_rgb = 0;
    const int nb = P.bnx * P.bny * P.bnz;
    if (variant == VR_VARIANT_VOLUME_MASK) {
        if (F.merged_stale || !F.merged_bricks) {
            VR_HIP(c, F.merged_bricks.reserve((size_t)nb));
            hipLaunchKernelGGL(merge_bricks_kernel, dim3((unsigned)((nb + 255) / 256)), dim3(256), 0, s, c->vols[2].bricks,
                               c->vols[0].bricks, F.merged_bricks, nb);
            VR_HIP(c, hipGetLastError());
            F.merged_stale = false;
        }
        P.bricks = F.merged_bricks;
        P.use_rgb = 1;
    }
    // distance field over the inert bricks (Chebyshev distance to the nearest active brick), rebuilt when the
    // records, the zero prefix or the table resolution changed since it was last built (an asynchronous opacity edit rebuilds it
    // on its own stream for the records it was built from: vr_tf_upload_opacity_async)
    const float bs[3] = {P.bsx, P.bsy, P.bsz};
    const FieldKey want = {(const void*)P.bricks, c->brick_epoch, P.tf_zero_prefix, c->tf[0].dev.res_o, P.use_rgb};
    if (!(F.key == want) || !F.brick_dist) {
        // (rare: an input changed.  Frames may be in flight on other streams and read the field: drain them first,
        // and finish the rebuild before any other stream's launch can follow)
        VR_HIP(c, hipDeviceSynchronize());
        drained(c);
        F.brick_dist = nullptr;
        if (const int rc = grow(c, F.field[F.cur], (size_t)nb, true)) return rc;
        if (const int rc = grow(c, F.tmp, (size_t)nb, true)) return rc;
        const int bn[3] = {P.bnx, P.bny, P.bnz};
        if (const int rc = build_field(c, s, want, bn, F.cur, ++F.gen)) return rc;
        VR_HIP(c, hipStreamSynchronize(s));
        F.publish(F.cur, want, bn);
    }
    F.adopt(bs);
    P.brick_dist = F.brick_dist;
    const HullPlanes hull = F.launch_box();
    for (int a = 0; a < kHullAxes; ++a) {
        P.abox[a] = hull.lo[a];
        P.abox[3 + a] = hull.hi[a];
    }
    for (int d = 0; d < kHullDiag; ++d) {
        P.hull_lo[d] = hull.lo[kHullAxes + d];
        P.hull_hi[d] = hull.hi[kHullAxes + d];
    }
    return VR_OK;
}

}  // namespace

extern "C" {

static int tf_check(vr_ctx* c, int slot, const float* table, uint32_t R, const char* who)
{
    if (slot < 0 || slot >= VR_MAX_TFS) return fail(c, VR_ERR_INVALID_ARG, std::string(who) + ": bad slot");
    if (!table) return fail(c, VR_ERR_INVALID_ARG, std::string(who) + ": table is NULL");
    if (R == 0 || R > (1u << 24)) return fail(c, VR_ERR_INVALID_ARG, std::string(who) + ": bad resolution");
    return VR_OK;
}

void TfSlot::set_current(const float* table, uint32_t R, bool is_color)
{
    if (is_color) {
        dev.color = (const float4*)current(1).p;
        dev.res_c = (int)R;
        color_finite = all_finite(table, (int)(4 * R));
    } else {
        dev.opacity = (const float*)current(0).p;
        dev.res_o = (int)R;
        int z = -1;
        opacity_finite = all_finite(table, (int)R);
        if (opacity_finite)
            while (z + 1 < (int)R && table[z + 1] == 0.0f) ++z;
        zero_prefix = z;
    }
}

// an upload into the current generation of a table has completed or been enqueued: the slot's host state and the context's counters
static void tf_uploaded(vr_ctx* c, int slot, const float* table, uint32_t R, bool is_color)
{
    ++c->tf_epoch;
    if (!is_color && slot == 0) ++c->opacity_edits;  // (the light volumes' key)
    c->tf[slot].current(is_color ? 1 : 0).written();
    c->tf[slot].set_current(table, R, is_color);
}

static int tf_upload_one(vr_ctx* c, int slot, const float* table, uint32_t R, bool is_color)
{
    if (!c) return VR_ERR_INVALID_ARG;
    if (const int rc = tf_check(c, slot, table, R, "vr_tf_upload")) return rc;
    if (const int rc = drain(c)) return rc;  // asynchronous renders on the caller's streams may still read the table
    const int comps = is_color ? 4 : 1;
    TfSlot& T = c->tf[slot];
    GenBuf& g = T.current(is_color ? 1 : 0);
    if (is_color) {
        T.dev.color = nullptr;
        T.dev.res_c = 0;
    } else {
        T.dev.opacity = nullptr;
        T.dev.res_o = 0;
    }
    if (const int rc = grow(c, g, ((size_t)R + 2) * comps * sizeof(float), true)) return rc;
    // device layout (DevTF): the first and the last texel once more at either end
    float* d = (float*)g.p;
    const size_t texel = comps * sizeof(float);
    VR_HIP(c, hipMemcpyAsync(d + comps, table, R * texel, hipMemcpyHostToDevice, c->stream));
    VR_HIP(c, hipMemcpyAsync(d, table, texel, hipMemcpyHostToDevice, c->stream));
    VR_HIP(c, hipMemcpyAsync(d + ((size_t)R + 1) * comps, table + comps * ((size_t)R - 1), texel, hipMemcpyHostToDevice, c->stream));
    VR_HIP(c, hipStreamSynchronize(c->stream));
    tf_uploaded(c, slot, table, R, is_color);
    return VR_OK;
}

// An asynchronous opacity edit of slot 0 that moves the zero prefix or changes the resolution: the field in use is rebuilt on the edit's
// stream into its next generation, for the records it was built from -- unless it is stale anyway (a volume changed, no field yet): then
// the next skipping launch rebuilds it as before.  A failure here leaves it to that launch as well.
static void rebuild_field_async(vr_ctx* c, hipStream_t s)
{
    SkipField& F = c->skip;
    FieldKey want = F.key;
    want.zero_prefix = c->tf[0].zero_prefix;
    want.res = c->tf[0].dev.res_o;
    if (!F.brick_dist || want == F.key || F.key.epoch != c->brick_epoch) return;
    if (F.key.use_rgb ? (F.merged_stale || F.key.records != (const void*)F.merged_bricks) : F.key.records != (const void*)c->vols[0].bricks)
        return;
    const int b = (F.cur + 1) % kGen;
    GenBuf& g = F.field[b];
    const size_t nb = (size_t)F.bn[0] * F.bn[1] * F.bn[2];
    const bool fresh = nb > g.cap;
    if (grow(c, g, nb, false) != VR_OK || grow(c, F.tmp, nb, false) != VR_OK || (!fresh && reuse_wait(c, s, g) != VR_OK) ||
        build_field(c, s, want, F.bn, b, F.gen + 1) != VR_OK) {
        (void)hipGetLastError();
        return;
    }
    ++F.gen;
    F.publish(b, want, F.bn);
}

// vr_tf_upload_opacity_async / _color_async: the table into pinned staging (DevTF layout), one copy on `s` into the next generation
// behind the last launch that read it, the host state as the synchronous upload sets it; then the edits' event behind it all.
static int tf_upload_async(vr_ctx* c, int slot, const float* table, uint32_t R, bool is_color, void* stream)
{
    if (!c) return VR_ERR_INVALID_ARG;
    if (const int rc = tf_check(c, slot, table, R, is_color ? "vr_tf_upload_color_async" : "vr_tf_upload_opacity_async")) return rc;
    VR_HIP(c, hipSetDevice(c->device));
    (void)hipGetLastError();
    hipStream_t s = stream ? (hipStream_t)stream : c->stream;
    const int comps = is_color ? 4 : 1, kind = is_color ? 1 : 0;
    const size_t texel = comps * sizeof(float), bytes = ((size_t)R + 2) * texel;
    TfEdits& E = c->edits;
    TfEdits::Stage& st = E.stage[E.stage_next % kStage];
    if (st.used) VR_HIP(c, hipEventSynchronize(st.done));  // (the one host wait: kStage edits are still being copied)
    st.used = false;
    if (bytes > st.h.cap) {
        if (st.h) c->retired_host.push_back(st.h.detach());
        VR_HIP(c, st.h.reserve(bytes));
    }
    float* h = (float*)st.h.p;
    std::memcpy(h + comps, table, R * texel);
    std::memcpy(h, table, texel);
    std::memcpy(h + ((size_t)R + 1) * comps, table + comps * ((size_t)R - 1), texel);
    VR_HIP(c, E.order.rebuild_behind(s));  // behind the edit before it, whatever its stream
    GenBuf& g = c->tf[slot].next(kind);
    if (bytes > g.cap) {
        if (const int rc = grow(c, g, bytes, false)) return rc;
    } else if (const int rc = reuse_wait(c, s, g)) {
        return rc;
    }
    VR_HIP(c, hipMemcpyAsync(g.p, h, bytes, hipMemcpyHostToDevice, s));
    VR_HIP(c, hipEventRecord(st.done, s));
    st.used = true;
    ++E.stage_next;
    c->tf[slot].advance(kind);
    tf_uploaded(c, slot, table, R, is_color);
    if (!is_color && slot == 0) rebuild_field_async(c, s);
    VR_HIP(c, hipEventRecord(E.order.ev, s));
    E.order.built(s);
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

}  // extern "C"
