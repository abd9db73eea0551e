// vr_api_tf.h -- the transfer-function tables: uploads, generations and asynchronous edits, and what skipping derives from the opacity
// table (distance field, active box: prepare_skip).  Part of vr_api.hip's translation unit.
#pragma once

namespace {

// finite and of moderate size: products of a colour, a light term and a shading factor stay finite, so "x * 0 == 0"
// holds for everything a provably-zero opacity is multiplied with
bool all_finite(const float* v, int n)
{
    for (int i = 0; i < n; ++i)
        if (!(v[i] - v[i] == 0.0f) || !(v[i] <= 1.0e15f && v[i] >= -1.0e15f)) return false;
    return true;
}

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
        if (b.p) b.reader[c->order_seq % kInFlight] = (long long)c->order_seq;
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

// Exact empty-space skipping (E.can_skip): fills P's brick fields from c, and rebuilds what is stale of the merged mask records, the
// distance field, the share of active bricks (active_fraction, which the kernel choice reads) and the box of the active bricks.
int prepare_skip(vr_ctx* c, int variant, hipStream_t s, MarchParams& P)
{
    const int sv = variant == VR_VARIANT_VOLUME_MASK ? 2 : 0;
    fill_brick_grid(P, sv, c->vols[sv].vol);
    P.tf_zero_prefix = c->tf_zero_prefix[0];
    P.bricks = c->vols[sv].bricks;
    P.use_rgb = 0;
    const int nb = P.bnx * P.bny * P.bnz;
    if (variant == VR_VARIANT_VOLUME_MASK) {
        if (c->merged_stale || !c->merged_bricks) {
            VR_HIP(c, c->merged_bricks.reserve((size_t)nb));
            hipLaunchKernelGGL(merge_bricks_kernel, dim3((unsigned)((nb + 255) / 256)), dim3(256), 0, s, c->vols[2].bricks,
                               c->vols[0].bricks, c->merged_bricks, nb);
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
        if (const int rc = grow(c, g, (size_t)nb, true)) return rc;
        if (const int rc = grow(c, c->dist_tmp, (size_t)nb, true)) return rc;
        const int bn[3] = {P.bnx, P.bny, P.bnz};
        if (const int rc = build_field(c, s, P.bricks, bn, P.use_rgb, P.tf_zero_prefix, c->tf[0].res_o, (unsigned char*)g.p, c->field_cur,
                                       ++c->skip_gen))
            return rc;
        VR_HIP(c, hipStreamSynchronize(s));
        g.written();
        c->brick_dist = (unsigned char*)g.p;
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

}  // namespace

extern "C" {

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
        c->tf[slot].color = (const float4*)g.p;
        c->tf[slot].res_c = (int)R;
        c->tf_color_finite[slot] = all_finite(table, (int)(4 * R));
    } else {
        if (slot == 0) ++c->opacity_edits;  // (the light volumes' key)
        c->tf[slot].opacity = (const float*)g.p;
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
    if (const int rc = drain(c)) return rc;  // asynchronous renders on the caller's streams may still read the table
    const int comps = is_color ? 4 : 1;
    GenBuf& g = c->tf_buf[slot][is_color ? 1 : 0][c->tf_cur[slot][is_color ? 1 : 0]];
    if (is_color) {
        c->tf[slot].color = nullptr;
        c->tf[slot].res_c = 0;
    } else {
        c->tf[slot].opacity = nullptr;
        c->tf[slot].res_o = 0;
    }
    if (const int rc = grow(c, g, ((size_t)R + 2) * comps * sizeof(float), true)) return rc;
    // device layout (DevTF): the first and the last texel once more at either end
    float* d = (float*)g.p;
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
    if (c->dist_rgb ? (c->merged_stale || c->dist_records != (const void*)c->merged_bricks) : c->dist_records != (const void*)c->vols[0].bricks)
        return;
    const int b = (c->field_cur + 1) % kGen;
    GenBuf& g = c->field[b];
    const size_t nb = (size_t)c->dist_bn[0] * c->dist_bn[1] * c->dist_bn[2];
    const bool fresh = nb > g.cap;
    if (grow(c, g, nb, false) != VR_OK || grow(c, c->dist_tmp, nb, false) != VR_OK ||
        (!fresh && reuse_wait(c, s, g) != VR_OK) ||
        build_field(c, s, (const float2*)c->dist_records, c->dist_bn, c->dist_rgb, z, res, (unsigned char*)g.p, b, c->skip_gen + 1) != VR_OK) {
        (void)hipGetLastError();
        return;
    }
    ++c->skip_gen;
    g.written();
    c->field_cur = b;
    c->brick_dist = (unsigned char*)g.p;
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
    if (bytes > st.h.cap) {
        if (st.h) c->retired_host.push_back(st.h.detach());
        VR_HIP(c, st.h.reserve(bytes));
    }
    float* h = (float*)st.h.p;
    std::memcpy(h + comps, table, R * texel);
    std::memcpy(h, table, texel);
    std::memcpy(h + ((size_t)R + 1) * comps, table + comps * ((size_t)R - 1), texel);
    // behind the edit before it, whatever its stream
    if (c->edit_gen > c->drained_gen && s != c->edit_stream) VR_HIP(c, hipStreamWaitEvent(s, c->edit_ev, 0));
    const int b = (c->tf_cur[slot][kind] + 1) % kGen;
    GenBuf& g = c->tf_buf[slot][kind][b];
    if (bytes > g.cap) {
        if (const int rc = grow(c, g, bytes, false)) return rc;
    } else if (const int rc = reuse_wait(c, s, g)) {
        return rc;
    }
    VR_HIP(c, hipMemcpyAsync(g.p, h, bytes, hipMemcpyHostToDevice, s));
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

}  // extern "C"
