// vr_api_segment.h -- segmentation on the device: region growing from seed voxels into a contour of a mask slot (vr_segment_grow; the
// kernels are vr_grow.h's).  A data-preparation call like vr_volume_normalize: it drains the device, runs on the context's stream, ends
// with refresh_bricks and is synchronous on return.  Part of vr_api.hip's translation unit.
#pragma once

namespace {

// the descriptor's own fields (VR_ERR_INVALID_ARG), then what the context must hold (VR_ERR_NOT_READY, the box, the seeds, the mask)
int check_grow(vr_ctx* c, const vr_grow_desc* d)
{
    const std::string w("vr_segment_grow");
    if (!d) return fail(c, VR_ERR_INVALID_ARG, w + ": the descriptor is NULL");
    if (const int rc = check_slot(c, w, "volume", d->volume_slot)) return rc;
    if (const int rc = check_slot(c, w, "mask", d->mask_slot)) return rc;
    if (d->mask_slot == d->volume_slot) return fail(c, VR_ERR_INVALID_ARG, w + ": the mask slot is the volume slot");
    if (const int rc = check_component(c, w, "channel", d->channel)) return rc;
    if (const int rc = check_component(c, w, "contour", d->contour)) return rc;
    if (d->connectivity != VR_GROW_FACES && d->connectivity != VR_GROW_ALL) return fail(c, VR_ERR_INVALID_ARG, w + ": unknown connectivity");
    if (d->mode != VR_GROW_REPLACE && d->mode != VR_GROW_ADD) return fail(c, VR_ERR_INVALID_ARG, w + ": unknown mode");
    if (d->n_seeds < 1 || d->n_seeds > VR_GROW_MAX_SEEDS) return fail(c, VR_ERR_INVALID_ARG, w + ": n_seeds must be 1 .. 64");
    if (const int rc = check_filled(c, w, "volume", d->volume_slot)) return rc;
    const DevVolume& v = c->vols[d->volume_slot].vol;
    if (const int rc = check_box(c, w, d->box_lo, d->box_hi, v)) return rc;
    const int n[3] = {v.nx, v.ny, v.nz};
    for (uint32_t i = 0; i < d->n_seeds; ++i)
        for (int a = 0; a < 3; ++a)
            if (d->seeds[i][a] < 0 || d->seeds[i][a] >= n[a]) return fail(c, VR_ERR_INVALID_ARG, w + ": seed " + std::to_string(i) + " lies outside the volume");
    const DevVolume& m = c->vols[d->mask_slot].vol;
    return m.data ? check_same_dims(c, w, "mask", m, "volume", v) : VR_OK;
}

// the working buffers of a grow over nb bricks (first use)
int prepare_grow_state(vr_ctx* c, size_t nb)
{
    GrowState& G = c->grow;
    // (the device is drained and every earlier use was synchronous: a smaller buffer is freed at once)
    if (const int rc = grow(c, G.words, 2 * nb, true)) return rc;
    if (const int rc = grow(c, G.lists, 3 * nb, true)) return rc;
    VR_HIP(c, G.io.first_use());
    return VR_OK;
}

// The grow itself, every argument checked and the device drained.  `fresh`: the mask slot's voxels were allocated and zeroed by this call.
int run_grow(vr_ctx* c, const vr_grow_desc& d, float4* mask, bool fresh, vr_grow_result* result)
{
    GrowState& G = c->grow;
    hipStream_t s = c->stream;
    const int vs = d.volume_slot;
    const DevVolume v = linear_volume(c, vs);
    GrowParams P;
    std::memset(&P, 0, sizeof P);
    const bool plane = d.channel == 3 && v.dens;
    P.val = plane ? v.dens : reinterpret_cast<const float*>(v.data) + d.channel;
    P.val_stride = plane ? 1 : 4;
    P.nx = v.nx;
    P.ny = v.ny;
    P.nz = v.nz;
    unsigned long long box;
    P.box = box_units(d.box_lo, d.box_hi, &box);  // (units: at most the volume's bricks, below 2^26)
    P.vlo = d.lo;
    P.vhi = d.hi;
    P.bnx = skip_bricks(v.nx);
    P.bny = skip_bricks(v.ny);
    P.bnz = skip_bricks(v.nz);
    const size_t nb = (size_t)P.bnx * P.bny * P.bnz;
    P.n_bricks = (unsigned)nb;
    P.all = d.connectivity == VR_GROW_ALL;
    const bool plain = plain_form(c);
    if (const int rc = prepare_grow_state(c, nb)) return rc;
    P.q = G.words;
    P.r = G.words.p + nb;
    P.stamp = G.lists;
    P.list[0] = G.lists.p + nb;
    P.list[1] = G.lists.p + 2 * nb;
    P.w = G.io.d;
    P.mask = mask;
    P.contour = d.contour;
    P.write_zeros = d.mode == VR_GROW_REPLACE && !fresh;
    GrowSeeds S;
    std::memset(&S, 0, sizeof S);
    S.n = d.n_seeds;
    std::memcpy(S.xyz, d.seeds, sizeof(int32_t) * 3 * d.n_seeds);

    VR_HIP(c, hipEventRecord(G.report.ev[0], s));
    // exact settling by the slot's range records (of .a: channel 3)
    if (!plain && d.channel == 3 && P.box.units != 0 && !prepare_range(c, s, vs, P.bnx, P.bny, P.bnz, &P.bricks)) return VR_ERR_HIP;
    *G.io.h.p = GrowWords{{0, 0, 0}, CountBox::empty(), {0, 0, 0}, 0};
    VR_HIP(c, G.io.push(s));
    VR_HIP(c, hipMemsetAsync(G.words, 0, 2 * nb * sizeof(unsigned long long), s));
    VR_HIP(c, hipMemsetAsync(G.lists, 0, nb * sizeof(unsigned), s));  // (the stamps; the lists are written before they are read)
    if (P.box.units != 0) {
        const unsigned blocks = tool_blocks(P.box.units);
        if (plain) hipLaunchKernelGGL(grow_classify_kernel<true>, dim3(blocks), dim3(256), 0, s, P);
        else hipLaunchKernelGGL(grow_classify_kernel<false>, dim3(blocks), dim3(256), 0, s, P);
        VR_HIP(c, hipGetLastError());
    }
    if (plain) hipLaunchKernelGGL(grow_seed_kernel<true>, dim3(1), dim3(64), 0, s, P, S);
    else hipLaunchKernelGGL(grow_seed_kernel<false>, dim3(1), dim3(64), 0, s, P, S);
    VR_HIP(c, hipGetLastError());
    VR_HIP(c, hipEventRecord(G.report.ev[1], s));

    // Rounds in batches of VR_GROW_BATCH, the words read behind each batch: done when the next round's input word is zero.  R grows
    // strictly in every round but the first and the last that have anything to do, so voxels + 1 rounds bound them all.
    const unsigned blocks = tool_blocks(nb);
    const unsigned long long limit = box + 1 < 0xFFFFFFF0ull ? box + 1 : 0xFFFFFFF0ull;
    unsigned long long k = 0;
    for (;;) {
        if (k >= limit) return fail(c, VR_ERR_HIP, "vr_segment_grow: did not converge in voxels + 1 rounds");
        for (int i = 0; i < VR_GROW_BATCH; ++i) {
            P.round = (unsigned)++k;
            if (plain) hipLaunchKernelGGL(grow_round_kernel<true>, dim3(blocks), dim3(256), 0, s, P);
            else hipLaunchKernelGGL(grow_round_kernel<false>, dim3(blocks), dim3(256), 0, s, P);
        }
        VR_HIP(c, hipGetLastError());
        VR_HIP(c, G.io.pull(s));
        VR_HIP(c, hipStreamSynchronize(s));
        if (G.io.h.p->cnt[(k + 1) % 3] == 0) break;
    }
    VR_HIP(c, hipEventRecord(G.report.ev[2], s));

    hipLaunchKernelGGL(grow_write_kernel, dim3(blocks), dim3(256), 0, s, P);
    VR_HIP(c, hipGetLastError());
    VR_HIP(c, G.io.pull(s));
    VR_HIP(c, hipEventRecord(G.report.ev[3], s));
    VR_HIP(c, hipStreamSynchronize(s));
    const GrowWords& w = *G.io.h.p;
    for (int i = 0; i < 3; ++i) G.report.counters[i] = w.stats[i];
    if (result) {
        std::memset(result, 0, sizeof *result);
        copy_count_box(w.reached, &result->voxels, result->lo, result->hi);
        result->rounds = w.rounds > 0 ? w.rounds : 1u;
    }
    return VR_OK;
}

}  // namespace

extern "C" {

int vr_grow_whole(const vr_ctx* c, int volume_slot, int mask_slot, int contour, float lo, float hi, vr_grow_desc* out)
{
    if (!c || !out) return VR_ERR_INVALID_ARG;
    if (!is_slot(volume_slot) || !is_slot(mask_slot) || mask_slot == volume_slot || !is_component(contour)) return VR_ERR_INVALID_ARG;
    if (!c->vols[volume_slot].vol.data) return VR_ERR_NOT_READY;
    std::memset(out, 0, sizeof *out);
    out->volume_slot = volume_slot;
    out->channel = 3;
    out->mask_slot = mask_slot;
    out->contour = contour;
    out->lo = lo;
    out->hi = hi;
    out->connectivity = VR_GROW_FACES;
    out->mode = VR_GROW_REPLACE;
    whole_box(c->vols[volume_slot].vol, out->box_hi);
    return VR_OK;
}

int vr_segment_grow(vr_ctx* c, const vr_grow_desc* desc, vr_grow_result* result)
{
    if (!c) return VR_ERR_INVALID_ARG;
    if (const int rc = check_grow(c, desc)) return rc;
    return mask_tool_call(c, "vr_segment_grow", desc->volume_slot, desc->mask_slot, c->grow.report,
                          [&](float4* mask, bool fresh) { return run_grow(c, *desc, mask, fresh, result); });
}

int vr_grow_counters(vr_ctx* c, uint64_t out[3]) { return tool_counters(c, &vr_ctx::grow, out, "vr_grow_counters"); }

int vr_grow_timing(vr_ctx* c, float ms[4]) { return tool_timing(c, &vr_ctx::grow, ms, "vr_grow_timing"); }

}  // extern "C"
