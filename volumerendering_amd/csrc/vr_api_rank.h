// vr_api_rank.h -- rank filters of a volume channel on the device (vr_volume_rank; the kernels are vr_rank.h's) and the host filler of
// its descriptor.  vr_volume_rank is a data-preparation call like vr_volume_filter: it drains the device, runs on the context's stream,
// ends with bind_voxels for a slot it created and with refresh_bricks otherwise, and is synchronous on return.  Part of vr_api.hip's
// translation unit.
#pragma once

namespace {

// the values of a window, and the position a descriptor's rank resolves to (-1: none)
int rank_window(const vr_rank_desc& d) { return (2 * d.radius[0] + 1) * (2 * d.radius[1] + 1) * (2 * d.radius[2] + 1); }
int rank_resolved(const vr_rank_desc& d)
{
    const int n = rank_window(d);
    if (d.rank == VR_RANK_MEDIAN) return n / 2;
    if (d.rank == VR_RANK_MAX) return n - 1;
    return d.rank >= 0 && d.rank < n ? d.rank : -1;
}

// the descriptor's own fields (VR_ERR_INVALID_ARG), then what the context must hold (VR_ERR_NOT_READY, the box, the destination)
int check_rank(vr_ctx* c, const vr_rank_desc* d)
{
    const std::string w("vr_volume_rank");
    if (!d) return fail(c, VR_ERR_INVALID_ARG, w + ": the descriptor is NULL");
    if (const int rc = check_slot(c, w, "source", d->src_slot)) return rc;
    if (const int rc = check_slot(c, w, "destination", d->dst_slot)) return rc;
    if (const int rc = check_component(c, w, "source channel", d->src_channel)) return rc;
    if (const int rc = check_component(c, w, "destination channel", d->dst_channel)) return rc;
    for (int a = 0; a < 3; ++a)
        if (d->radius[a] < 0 || d->radius[a] > VR_RANK_MAX_RADIUS) return fail(c, VR_ERR_INVALID_ARG, w + ": a radius is outside 0 .. " + std::to_string(VR_RANK_MAX_RADIUS));
    if (rank_resolved(*d) < 0) return fail(c, VR_ERR_INVALID_ARG, w + ": the rank is neither 0 .. N - 1 nor VR_RANK_MEDIAN / VR_RANK_MAX");
    if (d->border != VR_FILTER_CLAMP && d->border != VR_FILTER_CONSTANT) return fail(c, VR_ERR_INVALID_ARG, w + ": unknown border");
    if (const int rc = check_filled(c, w, "source", d->src_slot)) return rc;
    const DevVolume& v = c->vols[d->src_slot].vol;
    if (const int rc = check_box(c, w, d->box_lo, d->box_hi, v)) return rc;
    const DevVolume& m = c->vols[d->dst_slot].vol;
    return m.data ? check_same_dims(c, w, "destination", m, "source", v) : VR_OK;
}

// The call itself, every argument checked and the device drained.
int run_rank(vr_ctx* c, const vr_rank_desc& d, float4* dst, vr_rank_result* result)
{
    RankState& S = c->rank;
    hipStream_t s = c->stream;
    const DevVolume& v = c->vols[d.src_slot].vol;
    const int n[3] = {v.nx, v.ny, v.nz};
    const int window = rank_window(d), k = rank_resolved(d);
    unsigned long long box = 1, read = 1;
    for (int a = 0; a < 3; ++a) {
        box *= (unsigned long long)(d.box_hi[a] - d.box_lo[a]);
        read *= (unsigned long long)(std::min(n[a], d.box_hi[a] + d.radius[a]) - std::max(0, d.box_lo[a] - d.radius[a]));
    }
    if (box != 0)
        if (const int rc = grow(c, S.field, (size_t)box, true)) return rc;
    VR_HIP(c, S.io.first_use());

    VR_HIP(c, hipEventRecord(S.report.ev[0], s));
    if (box != 0) {
        RankArgs A;
        std::memset(&A, 0, sizeof A);
        A.src = reinterpret_cast<const unsigned*>(v.data);
        A.channel = d.src_channel;
        for (int a = 0; a < 3; ++a) A.n[a] = n[a], A.lo[a] = d.box_lo[a], A.bn[a] = d.box_hi[a] - d.box_lo[a], A.r[a] = d.radius[a];
        A.k = (unsigned)k;
        A.border = d.border;
        unsigned bits;
        std::memcpy(&bits, &d.border_value, sizeof bits);
        A.border_key = filter_key(bits);
        A.out = S.field.p;
        if (plain_form(c)) hipLaunchKernelGGL(rank_plain_kernel, dim3(lane_blocks(box)), dim3(256), 0, s, A);
        else {
            A.tx = (unsigned)((A.bn[0] + kRankTX - 1) / kRankTX);
            A.ty = (unsigned)((A.bn[1] + kRankTY - 1) / kRankTY);
            A.tiles = (unsigned long long)A.tx * (unsigned long long)A.ty * (unsigned long long)((A.bn[2] + kRankTZ - 1) / kRankTZ);
            const dim3 blocks(lane_blocks(A.tiles * 256ull));
            if (k == 0) hipLaunchKernelGGL((rank_tile_kernel<kRankMinMax, false>), blocks, dim3(256), 0, s, A);  // (a window of one value too)
            else if (k == window - 1) hipLaunchKernelGGL((rank_tile_kernel<kRankMinMax, true>), blocks, dim3(256), 0, s, A);
            else if (window == 27 && d.radius[0] == 1 && d.radius[1] == 1 && k == 13) hipLaunchKernelGGL((rank_tile_kernel<kRankMed27, false>), blocks, dim3(256), 0, s, A);
            else hipLaunchKernelGGL((rank_tile_kernel<kRankGeneric, false>), blocks, dim3(256), 0, s, A);
        }
        VR_HIP(c, hipGetLastError());
    }
    VR_HIP(c, hipEventRecord(S.report.ev[1], s));  // (one selection kernel in every form: the second phase is empty)
    VR_HIP(c, hipEventRecord(S.report.ev[2], s));
    *S.io.h.p = RankWords{0ull, 0ull, ~0u, 0u};
    VR_HIP(c, S.io.push(s));
    if (box != 0) {
        RankWrite W;
        std::memset(&W, 0, sizeof W);
        W.field = S.field.p;
        W.src = reinterpret_cast<const unsigned*>(v.data) + d.src_channel;
        W.dst = reinterpret_cast<unsigned*>(dst) + d.dst_channel;
        W.nx = n[0];
        W.ny = n[1];
        for (int a = 0; a < 3; ++a) W.lo[a] = d.box_lo[a], W.n[a] = d.box_hi[a] - d.box_lo[a];
        W.w = S.io.d;
        hipLaunchKernelGGL(rank_write_kernel, dim3(lane_blocks(box)), dim3(256), 0, s, W);
        VR_HIP(c, hipGetLastError());
    }
    VR_HIP(c, S.io.pull(s));
    VR_HIP(c, hipEventRecord(S.report.ev[3], s));
    VR_HIP(c, hipStreamSynchronize(s));
    const RankWords& w = *S.io.h.p;
    S.report.counters[0] = box, S.report.counters[1] = box != 0 ? read : 0ull, S.report.counters[2] = box != 0 ? (unsigned long long)k : 0ull;
    if (result) {
        std::memset(result, 0, sizeof *result);
        result->stored = box;
        result->nonfinite = w.nonfinite;
        result->changed = w.changed;
        if (w.lo_key <= w.hi_key) {  // (some finite value; otherwise both stay +0.0f)
            const unsigned lo = filter_unkey(w.lo_key), hi = filter_unkey(w.hi_key);
            std::memcpy(&result->lo_value, &lo, sizeof lo);
            std::memcpy(&result->hi_value, &hi, sizeof hi);
        }
    }
    return VR_OK;
}

}  // namespace

extern "C" {

int vr_rank_whole(const vr_ctx* c, int src_slot, int src_channel, int dst_slot, int dst_channel, vr_rank_desc* out)
{
    if (!c || !out) return VR_ERR_INVALID_ARG;
    if (!is_slot(src_slot) || !is_slot(dst_slot) || !is_component(src_channel) || !is_component(dst_channel)) return VR_ERR_INVALID_ARG;
    if (!c->vols[src_slot].vol.data) return VR_ERR_NOT_READY;
    std::memset(out, 0, sizeof *out);
    out->src_slot = src_slot;
    out->src_channel = src_channel;
    out->dst_slot = dst_slot;
    out->dst_channel = dst_channel;
    out->rank = VR_RANK_MEDIAN;
    out->border = VR_FILTER_CLAMP;
    whole_box(c->vols[src_slot].vol, out->box_hi);
    return VR_OK;
}

int vr_volume_rank(vr_ctx* c, const vr_rank_desc* desc, vr_rank_result* result)
{
    if (!c) return VR_ERR_INVALID_ARG;
    if (const int rc = check_rank(c, desc)) return rc;
    return mask_tool_call(c, "vr_volume_rank", desc->src_slot, desc->dst_slot, c->rank.report,
                          [&](float4* dst, bool) { return run_rank(c, *desc, dst, result); });
}

int vr_rank_counters(vr_ctx* c, uint64_t out[3]) { return tool_counters(c, &vr_ctx::rank, out, "vr_rank_counters"); }

int vr_rank_timing(vr_ctx* c, float ms[4])
{
    const int rc = tool_timing(c, &vr_ctx::rank, ms, "vr_rank_timing");
    if (rc == VR_OK) ms[1] = 0.0f;  // (every form selects in one kernel: no time between the two events is a further one's)
    return rc;
}

}  // extern "C"
