// vr_api_resample.h -- a volume slot resampled onto another grid (vr_volume_resample; the kernel is vr_resample.h's, in the march units
// behind launch_resample) and the host fillers of its descriptor.  vr_volume_resample is a data-preparation call like vr_mask_morph:
// it drains the device, runs on the context's stream, ends with bind_voxels for a slot it created and with refresh_bricks otherwise,
// and is synchronous on return.  Part of vr_api.hip's translation unit.
#pragma once

namespace {

bool is_grid_size(int n) { return n >= 1 && n <= 65535; }

// the descriptor's own fields (VR_ERR_INVALID_ARG), then what the context must hold (VR_ERR_NOT_READY, the destination's dimensions)
int check_resample(vr_ctx* c, const vr_resample_desc* d)
{
    const std::string w("vr_volume_resample");
    if (!d) return fail(c, VR_ERR_INVALID_ARG, w + ": the descriptor is NULL");
    if (const int rc = check_slot(c, w, "source", d->src_slot)) return rc;
    if (const int rc = check_slot(c, w, "destination", d->dst_slot)) return rc;
    if (d->src_slot == d->dst_slot) return fail(c, VR_ERR_INVALID_ARG, w + ": the source and the destination are one slot (the call gathers)");
    if (d->channels == 0 || d->channels > 15) return fail(c, VR_ERR_INVALID_ARG, w + ": channels must be 1 .. 15");
    if (d->filter != VR_RESAMPLE_LINEAR && d->filter != VR_RESAMPLE_NEAREST) return fail(c, VR_ERR_INVALID_ARG, w + ": unknown filter");
    for (int a = 0; a < 3; ++a)
        if (!is_grid_size(d->dst_n[a])) return fail(c, VR_ERR_INVALID_ARG, w + ": dst_n must be 1 .. 65535 on every axis");
    if ((unsigned long long)d->dst_n[0] * d->dst_n[1] * d->dst_n[2] > 0xFFFFFFFFull)
        return fail(c, VR_ERR_INVALID_ARG, w + ": more than 2^32 voxels");  // (as an upload: what a slot's derived data can index)
    for (int a = 0; a < 3; ++a)
        if (d->box_lo[a] < 0 || d->box_lo[a] > d->box_hi[a] || d->box_hi[a] > d->dst_n[a])
            return fail(c, VR_ERR_INVALID_ARG, w + ": the box must be 0 <= lo <= hi <= dst_n on every axis");
    if (const int rc = check_filled(c, w, "source", d->src_slot)) return rc;
    const DevVolume& m = c->vols[d->dst_slot].vol;
    if (m.data && (m.nx != d->dst_n[0] || m.ny != d->dst_n[1] || m.nz != d->dst_n[2]))
        return fail(c, VR_ERR_INVALID_ARG, w + ": the destination's dimensions differ from dst_n");
    return VR_OK;
}

// The call itself, every argument checked and the device drained.
int run_resample(vr_ctx* c, const vr_resample_desc& d, float4* dst, vr_resample_result* result)
{
    ResampleState& S = c->resample;
    hipStream_t s = c->stream;
    ResampleParams R;
    std::memset(&R, 0, sizeof R);
    R.src = linear_volume(c, d.src_slot);
    if (c->layout_mode == 0) use_bricked_copy(c, d.src_slot, R.src);
    bool off32 = c->vols[d.src_slot].bytes() <= 0xFFFFFFFFull;
    if (R.src.bricked && bricked_grid(R.src).slots * 16 > 0xFFFFFFFFull) off32 = false;
    R.dst = dst;
    unsigned long long box = 1;
    for (int a = 0; a < 3; ++a) {
        R.n[a] = d.dst_n[a];
        R.lo[a] = d.box_lo[a];
        R.hi[a] = d.box_hi[a];
        R.origin[a] = d.origin[a];
        R.di[a] = d.di[a];
        R.dj[a] = d.dj[a];
        R.dk[a] = d.dk[a];
        box *= (unsigned long long)(d.box_hi[a] - d.box_lo[a]);
    }
    for (int k = 0; k < 4; ++k) R.outside[k] = d.outside[k];
    R.channels = d.channels;
    R.ux = (unsigned)((d.box_hi[0] - d.box_lo[0] + 63) >> 6);
    R.units = box == 0 ? 0ull : (unsigned long long)R.ux * (unsigned long long)(d.box_hi[1] - d.box_lo[1]) * (unsigned long long)(d.box_hi[2] - d.box_lo[2]);
    const bool nearest = d.filter == VR_RESAMPLE_NEAREST;
    const int form = plain_form(c) ? kResamplePlain : (d.channels == 8u ? kResampleDensity : kResampleDefault);
    VR_HIP(c, S.io.first_use());
    R.w = S.io.d;

    VR_HIP(c, hipEventRecord(S.report.ev[0], s));
    // exact settling by the source's range records (of .a), rebuilt here when the source changed since they were built
    const DevVolume& v = c->vols[d.src_slot].vol;
    const int bnx = skip_bricks(v.nx), bny = skip_bricks(v.ny), bnz = skip_bricks(v.nz);
    if (form == kResampleDensity && !nearest && R.units != 0 && bricks_indexable(bnx, bny, bnz)) {
        R.bnx = bnx;
        R.bny = bny;
        if (!prepare_range(c, s, d.src_slot, bnx, bny, bnz, &R.bricks)) return VR_ERR_HIP;
    }
    VR_HIP(c, hipEventRecord(S.report.ev[1], s));
    *S.io.h.p = ResampleWords{CountBox::empty(), 0ull};
    VR_HIP(c, S.io.push(s));
    if (R.units != 0) {
        const unsigned blocks = tool_blocks(R.units);
        if (c->arith == VR_ARITH_FUSED) vrf::launch_resample(R, nearest, off32, form, blocks, s);
        else vr::launch_resample(R, nearest, off32, form, blocks, s);
        VR_HIP(c, hipGetLastError());
    }
    VR_HIP(c, hipEventRecord(S.report.ev[2], s));
    VR_HIP(c, S.io.pull(s));
    VR_HIP(c, hipEventRecord(S.report.ev[3], s));
    VR_HIP(c, hipStreamSynchronize(s));
    const ResampleWords& w = *S.io.h.p;
    S.report.computed_of_box(box, w.loaded);
    if (result) {
        std::memset(result, 0, sizeof *result);
        copy_count_box(w.inside, &result->inside, result->lo, result->hi);
        result->outside = box - w.inside.voxels;
    }
    return VR_OK;
}

}  // namespace

extern "C" {

int vr_resample_identity(const vr_ctx* c, int src_slot, int dst_slot, int filter, vr_resample_desc* out)
{
    if (!c || !out) return VR_ERR_INVALID_ARG;
    if (!is_slot(src_slot) || !is_slot(dst_slot) || src_slot == dst_slot) return VR_ERR_INVALID_ARG;
    if (filter != VR_RESAMPLE_LINEAR && filter != VR_RESAMPLE_NEAREST) return VR_ERR_INVALID_ARG;
    if (!c->vols[src_slot].vol.data) return VR_ERR_NOT_READY;
    const DevVolume& v = c->vols[src_slot].vol;
    const int n[3] = {v.nx, v.ny, v.nz};
    std::memset(out, 0, sizeof *out);
    out->src_slot = src_slot;
    out->dst_slot = dst_slot;
    out->channels = 15;
    out->filter = filter;
    for (int a = 0; a < 3; ++a) {
        out->dst_n[a] = n[a];
        out->origin[a] = 0.5f / (float)n[a];
        out->box_hi[a] = n[a];
    }
    out->di[0] = 1.0f / (float)n[0];
    out->dj[1] = 1.0f / (float)n[1];
    out->dk[2] = 1.0f / (float)n[2];
    return VR_OK;
}

int vr_resample_between(const vr_grid* src, const vr_grid* dst, const double dst_to_src[12], vr_resample_desc* out)
{
    if (!src || !dst || !out) return VR_ERR_INVALID_ARG;
    static const double identity[12] = {1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0};
    const double* M = dst_to_src ? dst_to_src : identity;
    for (int a = 0; a < 3; ++a) {
        if (!is_grid_size(src->n[a]) || !is_grid_size(dst->n[a])) return VR_ERR_INVALID_ARG;
        if (!std::isfinite(src->spacing[a]) || !(src->spacing[a] > 0.0) || !std::isfinite(dst->spacing[a]) || !(dst->spacing[a] > 0.0)) return VR_ERR_INVALID_ARG;
    }
    for (int i = 0; i < 12; ++i)
        if (!std::isfinite(M[i])) return VR_ERR_INVALID_ARG;
    for (int a = 0; a < 3; ++a) {  // (the order of operations is the header's: a float64 restatement gives the same twelve floats)
        const double* m = M + 4 * a;
        const double s = 1.0 / (src->spacing[a] * (double)src->n[a]);
        const double v = ((((m[0] * dst->origin[0]) + (m[1] * dst->origin[1])) + (m[2] * dst->origin[2])) + m[3]) - src->origin[a];
        out->origin[a] = (float)((v * s) + (0.5 / (double)src->n[a]));
        out->di[a] = (float)((m[0] * dst->spacing[0]) * s);
        out->dj[a] = (float)((m[1] * dst->spacing[1]) * s);
        out->dk[a] = (float)((m[2] * dst->spacing[2]) * s);
        out->dst_n[a] = dst->n[a];
        out->box_lo[a] = 0;
        out->box_hi[a] = dst->n[a];
    }
    return VR_OK;
}

int vr_volume_resample(vr_ctx* c, const vr_resample_desc* desc, vr_resample_result* result)
{
    if (!c) return VR_ERR_INVALID_ARG;
    if (const int rc = check_resample(c, desc)) return rc;
    unsigned long long ran_at = ~0ull;  // the brick epoch the kernel ran at
    const int rc = mask_tool_call(c, "vr_volume_resample", desc->dst_n, desc->dst_slot, c->resample.report, [&](float4* dst, bool) {
        const int r = run_resample(c, *desc, dst, result);
        ran_at = c->brick_epoch;
        return r;
    });
    // The rebuild behind the kernel moved the epoch for the destination alone: range records of the source that were current when the
    // kernel ran still are (the next resample of this source does not build them again).
    VolumeSlot& S = c->vols[desc->src_slot];
    if (rc == VR_OK && S.proj_epoch == ran_at) S.proj_epoch = c->brick_epoch;
    return rc;
}

int vr_resample_counters(vr_ctx* c, uint64_t out[3]) { return tool_counters(c, &vr_ctx::resample, out, "vr_resample_counters"); }

int vr_resample_timing(vr_ctx* c, float ms[4]) { return tool_timing(c, &vr_ctx::resample, ms, "vr_resample_timing"); }

}  // extern "C"
