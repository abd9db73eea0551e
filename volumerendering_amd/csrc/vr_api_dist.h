// vr_api_dist.h -- exact signed distance maps of a mask contour on the device (vr_mask_distance; the kernels are vr_dist.h's, the pack is
// vr_bitrows.h's) and the host filler of its descriptor.  vr_mask_distance is a data-preparation call like vr_mask_morph: it drains the
// device, runs on the context's stream, ends with bind_voxels for a slot it created and with refresh_bricks otherwise, and is
// synchronous on return.  Part of vr_api.hip's translation unit.
#pragma once

namespace {

constexpr uint32_t kDistMaxSpacing = 1u << 20, kDistMaxLimit = 1u << 31;
constexpr uint64_t kDistMaxExtent = 1ull << 30;  // of (hi - lo) * spacing per axis: every squared distance stays below 2^62

// the descriptor's own fields (VR_ERR_INVALID_ARG), then what the context must hold (VR_ERR_NOT_READY, the box, the other slots)
int check_dist(vr_ctx* c, const vr_dist_desc* d)
{
    const std::string w("vr_mask_distance");
    if (!d) return fail(c, VR_ERR_INVALID_ARG, w + ": the descriptor is NULL");
    if (const int rc = check_slot(c, w, "source", d->src_slot)) return rc;
    if (const int rc = check_slot(c, w, "destination", d->dst_slot)) return rc;
    if (const int rc = check_component(c, w, "source contour", d->src_contour)) return rc;
    if (const int rc = check_component(c, w, "destination channel", d->dst_channel)) return rc;
    if (d->mode < VR_DIST_OUTSIDE || d->mode > VR_DIST_SIGNED) return fail(c, VR_ERR_INVALID_ARG, w + ": unknown mode");
    if (d->probe_slot != -1) {
        if (const int rc = check_slot(c, w, "probe", d->probe_slot)) return rc;
        if (const int rc = check_component(c, w, "probe contour", d->probe_contour)) return rc;
        if (d->mode == VR_DIST_INSIDE) return fail(c, VR_ERR_INVALID_ARG, w + ": a probe reports the OUTSIDE field, which VR_DIST_INSIDE does not compute");
    }
    for (int a = 0; a < 3; ++a)
        if (d->spacing[a] == 0 || d->spacing[a] > kDistMaxSpacing) return fail(c, VR_ERR_INVALID_ARG, w + ": a spacing is outside 1 .. 2^20");
    if (d->limit > kDistMaxLimit) return fail(c, VR_ERR_INVALID_ARG, w + ": the limit is above 2^31");
    if (!std::isfinite(d->scale) || !(d->scale > 0.0f)) return fail(c, VR_ERR_INVALID_ARG, w + ": the scale must be finite and > 0");
    if (const int rc = check_filled(c, w, "source", d->src_slot)) return rc;
    const DevVolume& v = c->vols[d->src_slot].vol;
    if (const int rc = check_box(c, w, d->box_lo, d->box_hi, v)) return rc;
    for (int a = 0; a < 3; ++a)
        if ((uint64_t)(d->box_hi[a] - d->box_lo[a]) * d->spacing[a] > kDistMaxExtent)
            return fail(c, VR_ERR_INVALID_ARG, w + ": the box's extent times the spacing exceeds 2^30 on some axis");
    if (d->probe_slot != -1) {
        if (const int rc = check_filled(c, w, "probe", d->probe_slot)) return rc;
        if (const int rc = check_same_dims(c, w, "probe", c->vols[d->probe_slot].vol, "source", v)) return rc;
    }
    const DevVolume& m = c->vols[d->dst_slot].vol;
    return m.data ? check_same_dims(c, w, "destination", m, "source", v) : VR_OK;
}

unsigned long long field_voxels(const DistField& F) { return (unsigned long long)F.n[0] * (unsigned long long)F.n[1] * (unsigned long long)F.n[2]; }

// One field over its region: the x pass from the bit-rows, then the envelope passes along y and z in place (a line of one voxel is
// what it was).  COMP: the INSIDE field.
int dist_field(vr_ctx* c, const DistParams& P, const vr_dist_desc& d, const DistField& F, bool comp)
{
    if (field_voxels(F) == 0) return VR_OK;
    DistState& S = c->dist;
    hipStream_t s = c->stream;
    DistXPass X;
    X.bits = P.a;
    X.F = F;
    X.ny = P.b.ny;
    X.wx = P.b.wx;
    X.rw0 = F.lo[0] >> 6;
    X.rw = ((F.lo[0] + F.n[0] + 63) >> 6) - X.rw0;
    X.words = (unsigned long long)X.rw * (unsigned long long)F.n[1] * (unsigned long long)F.n[2];
    X.spacing = d.spacing[0];
    const unsigned blocks = tool_blocks(X.words);
    if (comp) hipLaunchKernelGGL(dist_x_kernel<true>, dim3(blocks), dim3(256), 0, s, X);
    else hipLaunchKernelGGL(dist_x_kernel<false>, dim3(blocks), dim3(256), 0, s, X);
    VR_HIP(c, hipGetLastError());
    const unsigned long long row = (unsigned long long)F.n[0], slice = row * (unsigned long long)F.n[1];
    for (int axis = 1; axis < 3; ++axis) {
        if (F.n[axis] <= 1) continue;
        DistLine L;
        L.d2 = F.d2;
        L.n = F.n[axis];
        L.spacing = d.spacing[axis];
        L.stack_g = S.stack_g;
        L.stack_st = S.stack_st;
        if (axis == 1) {  // lane t = (x, z): the line along y
            L.lanes = row * (unsigned long long)F.n[2];
            L.inner = row;
            L.outer = slice;
            L.stride = row;
        } else {  // lane t = (x, y): the line along z
            L.lanes = slice;
            L.inner = slice;
            L.outer = 0;
            L.stride = slice;
        }
        const unsigned line_blocks = (unsigned)((L.lanes + 63ull) / 64ull);  // (a field that fits the device: far below 2^31 blocks)
        hipLaunchKernelGGL(dist_line_kernel, dim3(line_blocks), dim3(64), 0, s, L);
        VR_HIP(c, hipGetLastError());
    }
    return VR_OK;
}

// The call itself, every argument checked and the device drained.
int run_dist(vr_ctx* c, const vr_dist_desc& d, float4* dst, vr_dist_result* result)
{
    DistState& S = c->dist;
    hipStream_t s = c->stream;
    const DevVolume& v = c->vols[d.src_slot].vol;
    const bool probe = d.probe_slot != -1;
    DistParams P;
    std::memset(&P, 0, sizeof P);
    unsigned long long box;
    const BitRows W = P.b = bit_rows(v, d.box_lo, d.box_hi, &box);
    P.dst = dst;
    P.dst_channel = d.dst_channel;
    const size_t nw = W.words();
    if (const int rc = grow(c, c->bit_row_scratch, 2 * nw, true)) return rc;  // (drained: a smaller scratch is freed at once)
    unsigned long long* const words = c->bit_row_scratch.p;  // the packed operand A', and the packed probe
    VR_HIP(c, S.io.first_use());
    P.a = words;
    P.probe = probe ? words + nw : nullptr;
    P.w = S.io.d;
    const unsigned blocks = tool_blocks(W.box_words);

    VR_HIP(c, hipEventRecord(S.report.ev[0], s));
    *S.io.h.p = DistWords{CountBox::empty(), CountBox::empty(), 0ull, 0ull, kDistNone, 0ull};
    VR_HIP(c, S.io.push(s));
    VR_HIP(c, hipMemsetAsync(words, 0, (probe ? 2 : 1) * nw * sizeof(unsigned long long), s));
    if (const int rc = tool_pack(c, v.data, d.src_contour, W, words, &S.io.d.p->src)) return rc;
    if (probe)
        if (const int rc = tool_pack(c, c->vols[d.probe_slot].vol.data, d.probe_contour, W, words + nw, &S.io.d.p->probe)) return rc;
    VR_HIP(c, S.io.pull(s));
    VR_HIP(c, hipStreamSynchronize(s));
    const CountBox packed = S.io.h.p->src;
    VR_HIP(c, hipEventRecord(S.report.ev[1], s));

    // Where a field is computed; outside it is known.  OUTSIDE: with a limit BEYOND outside the bounding box of A' grown by
    // limit / spacing voxels, everywhere for an empty A'.  INSIDE: zero outside A', and a voxel of A' finds its nearest voxel of B' within
    // the bounding box of A' grown by one voxel (clamping a farther one into it gives one of B' that is no farther on any axis).  The
    // plain form takes the whole box.
    const bool plain = plain_form(c);
    const bool need[2] = {d.mode != VR_DIST_INSIDE, d.mode != VR_DIST_OUTSIDE};
    DistField F[2];
    std::memset(F, 0, sizeof F);
    for (int f = 0; f < 2; ++f) {
        if (!need[f] || box == 0 || (!plain && packed.voxels == 0)) continue;
        for (int a = 0; a < 3; ++a) {
            long long lo = W.lo[a], hi = W.hi[a];
            if (!plain && (f == 1 || d.limit != 0)) {
                const long long g = f == 1 ? 1 : (long long)(d.limit / d.spacing[a]);
                lo = std::max(lo, (long long)packed.lo[a] - g);
                hi = std::min(hi, (long long)packed.hi[a] + g);
            }
            F[f].lo[a] = (int)lo;
            F[f].n[a] = (int)(hi - lo);
        }
    }
    const unsigned long long fv[2] = {field_voxels(F[0]), field_voxels(F[1])};
    for (int f = 0; f < 2; ++f) {
        if (const int rc = grow(c, S.d2[f], (size_t)fv[f], true)) return rc;
        F[f].d2 = S.d2[f];
    }
    if (const int rc = grow(c, S.stack_g, (size_t)std::max(fv[0], fv[1]), true)) return rc;
    if (const int rc = grow(c, S.stack_st, (size_t)std::max(fv[0], fv[1]), true)) return rc;
    for (int f = 0; f < 2; ++f)
        if (const int rc = dist_field(c, P, d, F[f], f == 1)) return rc;
    VR_HIP(c, hipEventRecord(S.report.ev[2], s));

    P.out = F[0];
    P.in = F[1];
    P.mode = d.mode;
    P.limit_sq = (unsigned long long)d.limit * d.limit;
    P.scale = d.scale;
    P.beyond_value = d.limit != 0 ? (float)d.limit * d.scale : INFINITY;
    if (W.box_words != 0) {
        hipLaunchKernelGGL(dist_write_kernel, dim3(blocks), dim3(256), 0, s, P);
        VR_HIP(c, hipGetLastError());
    }
    VR_HIP(c, S.io.pull(s));
    VR_HIP(c, hipEventRecord(S.report.ev[3], s));
    VR_HIP(c, hipStreamSynchronize(s));
    const DistWords& w = *S.io.h.p;
    S.report.computed_of_box(box, fv[d.mode == VR_DIST_INSIDE ? 1 : 0]);
    if (result) {
        std::memset(result, 0, sizeof *result);
        copy_count_box(w.src, &result->src_voxels, result->lo, result->hi);
        result->beyond = w.beyond;
        result->probe_voxels = w.probe_voxels;
        result->probe_min_sq = w.probe_voxels ? w.probe_min : 0;
        result->probe_max_sq = w.probe_voxels ? w.probe_max : 0;
    }
    return VR_OK;
}

}  // namespace

extern "C" {

int vr_dist_whole(const vr_ctx* c, int src_slot, int src_contour, int dst_slot, int dst_channel, int mode, vr_dist_desc* out)
{
    if (!c || !out) return VR_ERR_INVALID_ARG;
    if (!is_slot(src_slot) || !is_slot(dst_slot) || !is_component(src_contour) || !is_component(dst_channel)) return VR_ERR_INVALID_ARG;
    if (mode < VR_DIST_OUTSIDE || mode > VR_DIST_SIGNED) return VR_ERR_INVALID_ARG;
    if (!c->vols[src_slot].vol.data) return VR_ERR_NOT_READY;
    std::memset(out, 0, sizeof *out);
    out->src_slot = src_slot;
    out->src_contour = src_contour;
    out->dst_slot = dst_slot;
    out->dst_channel = dst_channel;
    out->mode = mode;
    out->probe_slot = -1;
    out->spacing[0] = out->spacing[1] = out->spacing[2] = 1;
    out->scale = 1.0f;
    whole_box(c->vols[src_slot].vol, out->box_hi);
    return VR_OK;
}

int vr_mask_distance(vr_ctx* c, const vr_dist_desc* desc, vr_dist_result* result)
{
    if (!c) return VR_ERR_INVALID_ARG;
    if (const int rc = check_dist(c, desc)) return rc;
    return mask_tool_call(c, "vr_mask_distance", desc->src_slot, desc->dst_slot, c->dist.report,
                          [&](float4* dst, bool) { return run_dist(c, *desc, dst, result); });
}

int vr_dist_counters(vr_ctx* c, uint64_t out[3]) { return tool_counters(c, &vr_ctx::dist, out, "vr_dist_counters"); }

int vr_dist_timing(vr_ctx* c, float ms[4]) { return tool_timing(c, &vr_ctx::dist, ms, "vr_dist_timing"); }

}  // extern "C"
