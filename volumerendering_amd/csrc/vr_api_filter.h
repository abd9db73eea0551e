// vr_api_filter.h -- separable filters of a volume channel on the device (vr_volume_filter; the kernels are vr_filter.h's), the host
// filler of its descriptor and the Gaussian weights (vr_filter_gaussian, pure host arithmetic).  vr_volume_filter is a data-preparation
// call like vr_mask_distance: it drains the device, runs on the context's stream, ends with bind_voxels for a slot it created and with
// refresh_bricks otherwise, and is synchronous on return.  Part of vr_api.hip's translation unit.
#pragma once

namespace {

// the descriptor's own fields (VR_ERR_INVALID_ARG), then what the context must hold (VR_ERR_NOT_READY, the box, the destination)
int check_filter(vr_ctx* c, const vr_filter_desc* d)
{
    const std::string w("vr_volume_filter");
    if (!d) return fail(c, VR_ERR_INVALID_ARG, w + ": the descriptor is NULL");
    if (const int rc = check_slot(c, w, "source", d->src_slot)) return rc;
    if (const int rc = check_slot(c, w, "destination", d->dst_slot)) return rc;
    if (const int rc = check_component(c, w, "source channel", d->src_channel)) return rc;
    if (const int rc = check_component(c, w, "destination channel", d->dst_channel)) return rc;
    for (int a = 0; a < 3; ++a) {
        if (d->radius[a] < 0 || d->radius[a] > VR_FILTER_MAX_RADIUS) return fail(c, VR_ERR_INVALID_ARG, w + ": a radius is outside 0 .. " + std::to_string(VR_FILTER_MAX_RADIUS));
        if (d->radius[a] != 0 && !d->taps[a]) return fail(c, VR_ERR_INVALID_ARG, w + ": a radius without taps");
    }
    if (d->border != VR_FILTER_CLAMP && d->border != VR_FILTER_CONSTANT) return fail(c, VR_ERR_INVALID_ARG, w + ": unknown border");
    if (const int rc = check_filled(c, w, "source", d->src_slot)) return rc;
    const DevVolume& v = c->vols[d->src_slot].vol;
    if (const int rc = check_box(c, w, d->box_lo, d->box_hi, v)) return rc;
    const DevVolume& m = c->vols[d->dst_slot].vol;
    return m.data ? check_same_dims(c, w, "destination", m, "source", v) : VR_OK;
}

// One pass on the context's stream: the default form's tiles, or the plain form's lanes.
int filter_pass(vr_ctx* c, FilterPass& P, int axis, bool plain)
{
    hipStream_t s = c->stream;
    if (plain) {
        const unsigned blocks = lane_blocks(P.out.voxels());
        if (axis == 0) hipLaunchKernelGGL(filter_plain_kernel<0>, dim3(blocks), dim3(256), 0, s, P);
        else if (axis == 1) hipLaunchKernelGGL(filter_plain_kernel<1>, dim3(blocks), dim3(256), 0, s, P);
        else hipLaunchKernelGGL(filter_plain_kernel<2>, dim3(blocks), dim3(256), 0, s, P);
    } else if (axis == 0) {
        P.tx = (unsigned)((P.out.n[0] + kFilterRun - 1) / kFilterRun);
        P.ta = 1;
        const unsigned long long rows = (unsigned long long)P.out.n[1] * (unsigned long long)P.out.n[2];
        P.tiles = (unsigned long long)P.tx * ((rows + kFilterRows - 1) / kFilterRows);
        hipLaunchKernelGGL(filter_x_kernel, dim3(lane_blocks(P.tiles * 256ull)), dim3(256), 0, s, P);
    } else {
        P.tx = (unsigned)((P.out.n[0] + 63) / 64);
        P.ta = (unsigned)((P.out.n[axis] + kFilterT - 1) / kFilterT);
        P.tiles = (unsigned long long)P.tx * (unsigned long long)P.ta * (unsigned long long)P.out.n[axis == 1 ? 2 : 1];
        const unsigned blocks = lane_blocks(P.tiles * 256ull);
        const size_t lds = (size_t)(kFilterT + 2 * P.r) * 64 * sizeof(float);
        if (axis == 1) hipLaunchKernelGGL(filter_line_kernel<1>, dim3(blocks), dim3(256), lds, s, P);
        else hipLaunchKernelGGL(filter_line_kernel<2>, dim3(blocks), dim3(256), lds, s, P);
    }
    VR_HIP(c, hipGetLastError());
    return VR_OK;
}

// The call itself, every argument checked and the device drained.
int run_filter(vr_ctx* c, const vr_filter_desc& d, float4* dst, vr_filter_result* result)
{
    FilterState& S = c->filter;
    hipStream_t s = c->stream;
    const DevVolume& v = c->vols[d.src_slot].vol;
    const int n[3] = {v.nx, v.ny, v.nz};
    unsigned long long box = 1;
    for (int a = 0; a < 3; ++a) box *= (unsigned long long)(d.box_hi[a] - d.box_lo[a]);
    // the passes and their regions: the box, grown on every later axis that has a pass by that axis' radius, clipped to the volume
    int axes[3], passes = 0;
    for (int a = 0; a < 3 && box != 0; ++a)
        if (d.taps[a]) axes[passes++] = a;
    FilterView region[3];
    unsigned long long computed = 0;
    for (int k = 0; k < passes; ++k) {
        FilterView& R = region[k];
        R.stride = 1;
        for (int a = 0; a < 3; ++a) {
            int lo = d.box_lo[a], hi = d.box_hi[a];
            for (int j = k + 1; j < passes; ++j)
                if (axes[j] == a) lo = std::max(0, lo - d.radius[a]), hi = std::min(n[a], hi + d.radius[a]);
            R.lo[a] = lo;
            R.n[a] = hi - lo;
        }
        computed += R.voxels();
    }
    // the working buffers: the passes write the two fields in turn, the first one is the largest
    for (int k = 0; k < passes && k < 2; ++k)
        if (const int rc = grow(c, S.field[k], (size_t)region[k].voxels(), true)) return rc;
    VR_HIP(c, S.io.first_use());

    FilterView cur;  // what the next pass, or the write, reads: at first the source's component
    cur.p = reinterpret_cast<float*>(const_cast<float4*>(v.data)) + d.src_channel;
    cur.stride = 4;
    for (int a = 0; a < 3; ++a) cur.lo[a] = 0, cur.n[a] = n[a];
    const bool plain = plain_form(c);
    VR_HIP(c, hipEventRecord(S.report.ev[0], s));
    for (int k = 0; k < passes; ++k) {
        const int a = axes[k];
        FilterPass P;
        std::memset(&P, 0, sizeof P);
        P.in = cur;
        P.out = region[k];
        P.out.p = S.field[k & 1];
        P.r = d.radius[a];
        P.extent = n[a];
        P.border = d.border;
        P.border_value = d.border_value;
        std::memcpy(P.w, d.taps[a], (size_t)(2 * P.r + 1) * sizeof(float));
        if (const int rc = filter_pass(c, P, a, plain)) return rc;
        cur = P.out;
        if (k == 0) VR_HIP(c, hipEventRecord(S.report.ev[1], s));
    }
    if (passes == 0) VR_HIP(c, hipEventRecord(S.report.ev[1], s));
    VR_HIP(c, hipEventRecord(S.report.ev[2], s));
    *S.io.h.p = FilterWords{0ull, ~0u, 0u};
    VR_HIP(c, S.io.push(s));
    if (box != 0) {
        FilterWrite W;
        std::memset(&W, 0, sizeof W);
        W.in = cur;
        W.dst = reinterpret_cast<unsigned*>(dst);
        W.dst_channel = d.dst_channel;
        W.nx = n[0];
        W.ny = n[1];
        for (int a = 0; a < 3; ++a) W.lo[a] = d.box_lo[a], W.n[a] = d.box_hi[a] - d.box_lo[a];
        W.w = S.io.d;
        hipLaunchKernelGGL(filter_write_kernel, dim3(lane_blocks(box)), dim3(256), 0, s, W);
        VR_HIP(c, hipGetLastError());
    }
    VR_HIP(c, S.io.pull(s));
    VR_HIP(c, hipEventRecord(S.report.ev[3], s));
    VR_HIP(c, hipStreamSynchronize(s));
    const FilterWords& w = *S.io.h.p;
    S.report.counters[0] = box, S.report.counters[1] = computed, S.report.counters[2] = (unsigned long long)passes;
    if (result) {
        std::memset(result, 0, sizeof *result);
        result->stored = box;
        result->nonfinite = w.nonfinite;
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

int vr_filter_whole(const vr_ctx* c, int src_slot, int src_channel, int dst_slot, int dst_channel, vr_filter_desc* out)
{
    if (!c || !out) return VR_ERR_INVALID_ARG;
    if (!is_slot(src_slot) || !is_slot(dst_slot) || !is_component(src_channel) || !is_component(dst_channel)) return VR_ERR_INVALID_ARG;
    if (!c->vols[src_slot].vol.data) return VR_ERR_NOT_READY;
    std::memset(out, 0, sizeof *out);
    out->src_slot = src_slot;
    out->src_channel = src_channel;
    out->dst_slot = dst_slot;
    out->dst_channel = dst_channel;
    out->border = VR_FILTER_CLAMP;
    whole_box(c->vols[src_slot].vol, out->box_hi);
    return VR_OK;
}

int vr_filter_gaussian(double sigma, int order, double truncate, float* taps, int capacity, int* radius)
{
    if (!radius) return VR_ERR_INVALID_ARG;
    if (!std::isfinite(sigma) || !(sigma > 0.0) || !std::isfinite(truncate) || !(truncate > 0.0)) return VR_ERR_INVALID_ARG;
    if (order != 0 && order != 1) return VR_ERR_INVALID_ARG;
    const double reach = truncate * sigma + 0.5;
    if (!(reach < (double)(VR_FILTER_MAX_RADIUS + 1))) return VR_ERR_INVALID_ARG;
    const int r = (int)reach;
    *radius = r;
    if (!taps || capacity < 2 * r + 1) return VR_ERR_INVALID_ARG;  // (the counting call)
    double phi[VR_FILTER_MAX_RADIUS + 1], tail = 0.0;
    for (int x = 0; x <= r; ++x) phi[x] = std::exp(-0.5 * (double)x * (double)x / (sigma * sigma));
    for (int x = 1; x <= r; ++x) tail += phi[x];
    const double S = phi[0] + 2.0 * tail;
    for (int x = 0; x <= r; ++x) {
        if (order == 0) taps[r + x] = taps[r - x] = (float)(phi[x] / S);
        else {
            taps[r + x] = (float)(((double)x / (sigma * sigma)) * phi[x] / S);
            taps[r - x] = -taps[r + x];
        }
    }
    if (order == 1) taps[r] = 0.0f;
    return VR_OK;
}

int vr_volume_filter(vr_ctx* c, const vr_filter_desc* desc, vr_filter_result* result)
{
    if (!c) return VR_ERR_INVALID_ARG;
    if (const int rc = check_filter(c, desc)) return rc;
    return mask_tool_call(c, "vr_volume_filter", desc->src_slot, desc->dst_slot, c->filter.report,
                          [&](float4* dst, bool) { return run_filter(c, *desc, dst, result); });
}

int vr_filter_counters(vr_ctx* c, uint64_t out[3]) { return tool_counters(c, &vr_ctx::filter, out, "vr_filter_counters"); }

int vr_filter_timing(vr_ctx* c, float ms[4]) { return tool_timing(c, &vr_ctx::filter, ms, "vr_filter_timing"); }

}  // extern "C"
