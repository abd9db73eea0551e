// vr_api_gamma.h -- the gamma index of two dose channels on the device (vr_volume_gamma; the kernels are vr_gamma.h's), the table of
// admitted offsets and the host filler of the descriptor.  vr_volume_gamma is a data-preparation call like vr_volume_filter: it drains
// the device, runs on the context's stream, ends with bind_voxels for a slot it created and with refresh_bricks otherwise, and is
// synchronous on return.  Part of vr_api.hip's translation unit.
#pragma once

namespace {

// the descriptor's own fields (VR_ERR_INVALID_ARG), then what the context must hold (VR_ERR_NOT_READY, the dimensions, the box)
int check_gamma(vr_ctx* c, const vr_gamma_desc* d)
{
    const std::string w("vr_volume_gamma");
    if (!d) return fail(c, VR_ERR_INVALID_ARG, w + ": the descriptor is NULL");
    if (const int rc = check_slot(c, w, "reference", d->ref_slot)) return rc;
    if (const int rc = check_slot(c, w, "evaluated", d->eval_slot)) return rc;
    if (const int rc = check_slot(c, w, "destination", d->dst_slot)) return rc;
    if (const int rc = check_component(c, w, "reference channel", d->ref_channel)) return rc;
    if (const int rc = check_component(c, w, "evaluated channel", d->eval_channel)) return rc;
    if (const int rc = check_component(c, w, "destination channel", d->dst_channel)) return rc;
    if (d->roi_slot != -1) {
        if (const int rc = check_slot(c, w, "ROI", d->roi_slot)) return rc;
        if (const int rc = check_component(c, w, "ROI contour", d->roi_contour)) return rc;
    }
    for (int a = 0; a < 3; ++a)
        if (d->spacing[a] < 1u || d->spacing[a] > (1u << 20)) return fail(c, VR_ERR_INVALID_ARG, w + ": a spacing is outside 1 .. 2^20");
    if (d->dta < 1u || d->dta > (1u << 24) || d->reach < 1u || d->reach > (1u << 24)) return fail(c, VR_ERR_INVALID_ARG, w + ": dta or reach is outside 1 .. 2^24");
    if (d->sub < 1 || d->sub > VR_GAMMA_MAX_SUB) return fail(c, VR_ERR_INVALID_ARG, w + ": sub is outside 1 .. " + std::to_string(VR_GAMMA_MAX_SUB));
    for (int a = 0; a < 3; ++a)
        if (d->reach / d->spacing[a] > (unsigned)VR_GAMMA_MAX_RADIUS)
            return fail(c, VR_ERR_INVALID_ARG, w + ": reach / spacing is above " + std::to_string(VR_GAMMA_MAX_RADIUS) + " voxels on some axis");
    if (d->mode != VR_GAMMA_GLOBAL && d->mode != VR_GAMMA_LOCAL) return fail(c, VR_ERR_INVALID_ARG, w + ": unknown mode");
    if (const int rc = check_filled(c, w, "reference", d->ref_slot)) return rc;
    if (const int rc = check_filled(c, w, "evaluated", d->eval_slot)) return rc;
    const DevVolume& v = c->vols[d->ref_slot].vol;
    if (const int rc = check_same_dims(c, w, "evaluated slot", c->vols[d->eval_slot].vol, "reference", v)) return rc;
    if (d->roi_slot != -1) {
        if (const int rc = check_filled(c, w, "ROI", d->roi_slot)) return rc;
        if (const int rc = check_same_dims(c, w, "ROI", c->vols[d->roi_slot].vol, "reference", v)) return rc;
    }
    if (const int rc = check_box(c, w, d->box_lo, d->box_hi, v)) return rc;
    const DevVolume& m = c->vols[d->dst_slot].vol;
    return m.data ? check_same_dims(c, w, "destination", m, "reference", v) : VR_OK;
}

// The admitted offsets of a (checked) descriptor in the order of the header: ascending D2n, ties by (k, j, i); each with its c.  K + 1
// entries: the last one twice.
void gamma_table(const vr_gamma_desc& d, std::vector<GammaEntry>& out)
{
    struct Offset {
        uint64_t d2;
        int o[3];
    };
    const int64_t sub = d.sub;
    const uint64_t lim = (uint64_t)d.reach * (uint64_t)sub * ((uint64_t)d.reach * (uint64_t)sub);
    int64_t top[3];
    for (int a = 0; a < 3; ++a) top[a] = (int64_t)d.reach * sub / (int64_t)d.spacing[a];
    std::vector<Offset> all;
    for (int64_t k = -top[2]; k <= top[2]; ++k)
        for (int64_t j = -top[1]; j <= top[1]; ++j)
            for (int64_t i = -top[0]; i <= top[0]; ++i) {
                const uint64_t x = (uint64_t)std::llabs(i) * d.spacing[0], y = (uint64_t)std::llabs(j) * d.spacing[1], z = (uint64_t)std::llabs(k) * d.spacing[2];
                const uint64_t d2 = x * x + y * y + z * z;
                if (d2 <= lim) all.push_back({d2, {(int)i, (int)j, (int)k}});
            }
    std::sort(all.begin(), all.end(), [](const Offset& p, const Offset& q) {
        if (p.d2 != q.d2) return p.d2 < q.d2;
        if (p.o[2] != q.o[2]) return p.o[2] < q.o[2];
        if (p.o[1] != q.o[1]) return p.o[1] < q.o[1];
        return p.o[0] < q.o[0];
    });
    const float kc = (float)(1.0 / ((double)d.dta * (double)d.dta * (double)sub * (double)sub));
    out.resize(all.size());
    for (size_t e = 0; e < all.size(); ++e) {
        int m[3], f[3];
        for (int a = 0; a < 3; ++a) {
            const int o = all[e].o[a];
            m[a] = o >= 0 ? o / (int)sub : -((-o + (int)sub - 1) / (int)sub);  // floor division
            f[a] = o - (int)sub * m[a];
        }
        out[e].packed = gamma_pack(m, f);
        out[e].c = (float)all[e].d2 * kc;
    }
    out.push_back(out.back());  // (the default form loads one entry ahead; the offset (0, 0, 0) is always admitted: out is not empty)
}

// The call itself, every argument checked and the device drained.
int run_gamma(vr_ctx* c, const vr_gamma_desc& d, float4* dst, vr_gamma_result* result)
{
    GammaState& S = c->gamma;
    hipStream_t s = c->stream;
    const DevVolume& v = c->vols[d.ref_slot].vol;
    const int n[3] = {v.nx, v.ny, v.nz};
    unsigned long long box = 1;
    for (int a = 0; a < 3; ++a) box *= (unsigned long long)(d.box_hi[a] - d.box_lo[a]);
    if (box != 0) {
        gamma_table(d, S.entries);
        if (const int rc = grow(c, S.table, S.entries.size(), true)) return rc;
        if (const int rc = grow(c, S.field, (size_t)box, true)) return rc;
    }
    VR_HIP(c, S.io.first_use());
    const unsigned long long K = box != 0 ? (unsigned long long)S.entries.size() - 1ull : 0ull;

    if (box != 0) VR_HIP(c, hipMemcpyAsync(S.table.p, S.entries.data(), S.entries.size() * sizeof(GammaEntry), hipMemcpyHostToDevice, s));
    VR_HIP(c, hipEventRecord(S.report.ev[0], s));
    if (box != 0) {
        GammaArgs A;
        std::memset(&A, 0, sizeof A);
        A.ref = reinterpret_cast<const float*>(v.data) + d.ref_channel;
        A.eval = reinterpret_cast<const float*>(c->vols[d.eval_slot].vol.data) + d.eval_channel;
        A.roi = d.roi_slot != -1 ? reinterpret_cast<const float*>(c->vols[d.roi_slot].vol.data) + d.roi_contour : nullptr;
        for (int a = 0; a < 3; ++a) {
            A.n[a] = n[a], A.lo[a] = d.box_lo[a], A.bn[a] = d.box_hi[a] - d.box_lo[a];
            A.h[a] = (int)(d.reach / d.spacing[a]) + (d.sub > 1 ? 1 : 0);
        }
        A.sub = d.sub;
        for (int f = 0; f < d.sub; ++f) A.t[f] = (float)f / (float)d.sub;
        A.mode = d.mode;
        A.tol = d.dose_tolerance;
        A.cutoff = d.cutoff;
        std::memcpy(&A.skip_bits, &d.skip_value, sizeof A.skip_bits);
        A.table = S.table.p;
        A.K = (unsigned)K;
        A.out = S.field.p;
        if (plain_form(c)) hipLaunchKernelGGL(gamma_plain_kernel, dim3(lane_blocks(box)), dim3(256), 0, s, A);
        else {
            A.tx = (unsigned)((A.bn[0] + kGammaTX - 1) / kGammaTX);
            A.ty = (unsigned)((A.bn[1] + kGammaTY - 1) / kGammaTY);
            A.tiles = (unsigned long long)A.tx * (unsigned long long)A.ty * (unsigned long long)((A.bn[2] + kGammaTZ - 1) / kGammaTZ);
            const dim3 blocks(lane_blocks(A.tiles * 256ull));
            const size_t lds = (size_t)(kGammaTX + 2 * A.h[0]) * (size_t)(kGammaTY + 2 * A.h[1]) * (size_t)(kGammaTZ + 2 * A.h[2]) * sizeof(float);
            if (!S.lds_raised) {  // (more than 48 KiB of dynamic LDS must be allowed per kernel first; the attribute sticks)
                VR_HIP(c, hipFuncSetAttribute(reinterpret_cast<const void*>(gamma_tile_kernel<false>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)kGammaMaxLds));
                VR_HIP(c, hipFuncSetAttribute(reinterpret_cast<const void*>(gamma_tile_kernel<true>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)kGammaMaxLds));
                S.lds_raised = true;
            }
            if (d.sub > 1) hipLaunchKernelGGL(gamma_tile_kernel<true>, blocks, dim3(256), lds, s, A);
            else hipLaunchKernelGGL(gamma_tile_kernel<false>, blocks, dim3(256), lds, s, A);
        }
        VR_HIP(c, hipGetLastError());
    }
    VR_HIP(c, hipEventRecord(S.report.ev[1], s));  // (one search kernel in every form: the second phase is empty)
    VR_HIP(c, hipEventRecord(S.report.ev[2], s));
    *S.io.h.p = GammaWords{0ull, 0ull, 0ull, 0u, 0u};
    VR_HIP(c, S.io.push(s));
    if (box != 0) {
        GammaWrite W;
        std::memset(&W, 0, sizeof W);
        W.field = S.field.p;
        W.dst = reinterpret_cast<unsigned*>(dst) + d.dst_channel;
        W.nx = n[0];
        W.ny = n[1];
        for (int a = 0; a < 3; ++a) W.lo[a] = d.box_lo[a], W.n[a] = d.box_hi[a] - d.box_lo[a];
        W.w = S.io.d;
        hipLaunchKernelGGL(gamma_write_kernel, dim3(lane_blocks(box)), dim3(256), 0, s, W);
        VR_HIP(c, hipGetLastError());
    }
    VR_HIP(c, S.io.pull(s));
    VR_HIP(c, hipEventRecord(S.report.ev[3], s));
    VR_HIP(c, hipStreamSynchronize(s));
    const GammaWords& w = *S.io.h.p;
    S.report.counters[0] = box, S.report.counters[1] = w.evaluated, S.report.counters[2] = K;
    if (result) {
        std::memset(result, 0, sizeof *result);
        result->stored = box;
        result->evaluated = w.evaluated;
        result->passed = w.passed;
        result->nonfinite = w.nonfinite;
        std::memcpy(&result->hi_value, &w.hi_bits, sizeof w.hi_bits);
    }
    return VR_OK;
}

}  // namespace

extern "C" {

int vr_gamma_whole(const vr_ctx* c, int ref_slot, int ref_channel, int eval_slot, int eval_channel, int dst_slot, int dst_channel, vr_gamma_desc* out)
{
    if (!c || !out) return VR_ERR_INVALID_ARG;
    if (!is_slot(ref_slot) || !is_slot(eval_slot) || !is_slot(dst_slot)) return VR_ERR_INVALID_ARG;
    if (!is_component(ref_channel) || !is_component(eval_channel) || !is_component(dst_channel)) return VR_ERR_INVALID_ARG;
    if (!c->vols[ref_slot].vol.data) return VR_ERR_NOT_READY;
    std::memset(out, 0, sizeof *out);
    out->ref_slot = ref_slot;
    out->ref_channel = ref_channel;
    out->eval_slot = eval_slot;
    out->eval_channel = eval_channel;
    out->dst_slot = dst_slot;
    out->dst_channel = dst_channel;
    out->roi_slot = -1;
    out->spacing[0] = out->spacing[1] = out->spacing[2] = 1u;
    out->dta = out->reach = 1u;
    out->sub = 1;
    out->mode = VR_GAMMA_GLOBAL;
    out->dose_tolerance = 1.0f;
    out->cutoff = -INFINITY;
    const unsigned nan = kGammaNan;
    std::memcpy(&out->skip_value, &nan, sizeof nan);
    whole_box(c->vols[ref_slot].vol, out->box_hi);
    return VR_OK;
}

int vr_volume_gamma(vr_ctx* c, const vr_gamma_desc* desc, vr_gamma_result* result)
{
    if (!c) return VR_ERR_INVALID_ARG;
    if (const int rc = check_gamma(c, desc)) return rc;
    return mask_tool_call(c, "vr_volume_gamma", desc->ref_slot, desc->dst_slot, c->gamma.report,
                          [&](float4* dst, bool) { return run_gamma(c, *desc, dst, result); });
}

int vr_gamma_counters(vr_ctx* c, uint64_t out[3]) { return tool_counters(c, &vr_ctx::gamma, out, "vr_gamma_counters"); }

int vr_gamma_timing(vr_ctx* c, float ms[4])
{
    const int rc = tool_timing(c, &vr_ctx::gamma, ms, "vr_gamma_timing");
    if (rc == VR_OK) ms[1] = 0.0f;  // (every form searches in one kernel: no time between the two events is a further one's)
    return rc;
}

}  // extern "C"
