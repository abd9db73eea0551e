// vr_api_components.h -- connected components of a mask contour on the device (vr_mask_components; the kernels are vr_comp.h's, the
// scan vr_scan.h's): the checks of a descriptor, the choice of keep_largest's winners and the call itself.  When it writes a slot it is
// a data-preparation call like vr_mask_morph (mask_tool_call: drains, runs on the context's stream, ends with bind_voxels or
// refresh_bricks, synchronous on return); when it writes none it is a data call like vr_mask_outlines (data_tool_call) and rebuilds
// nothing.  It looks at device words between its phases (the node count, the component count, the passing sizes).  Part of
// vr_api.hip's translation unit.
#pragma once

namespace {

constexpr unsigned long long kCompNodesMax = 0xffffffffull;  // run nodes of one call

bool comp_connectivity(int k) { return k == VR_COMP_FACES || k == VR_COMP_ALL || k == VR_COMP_PLANE_FACES || k == VR_COMP_PLANE_ALL; }

// the slot a call writes, or -1
int comp_written_slot(const vr_components_desc& d) { return d.dst_slot >= 0 ? d.dst_slot : d.label_slot; }

// the descriptor's own fields (VR_ERR_INVALID_ARG), then what the context must hold (VR_ERR_NOT_READY, the box, the destination)
int check_components(vr_ctx* c, const vr_components_desc* d)
{
    const std::string w("vr_mask_components");
    if (!d) return fail(c, VR_ERR_INVALID_ARG, w + ": the descriptor is NULL");
    if (const int rc = check_slot(c, w, "source", d->src_slot)) return rc;
    if (const int rc = check_component(c, w, "source contour", d->src_contour)) return rc;
    if (d->background != 0 && d->background != 1) return fail(c, VR_ERR_INVALID_ARG, w + ": background must be 0 or 1");
    if (!comp_connectivity(d->connectivity)) return fail(c, VR_ERR_INVALID_ARG, w + ": unknown connectivity");
    if (d->keep_largest > VR_COMP_MAX_KEEP) return fail(c, VR_ERR_INVALID_ARG, w + ": keep_largest must be 0 .. 64");
    if (d->reject_faces & ~63u) return fail(c, VR_ERR_INVALID_ARG, w + ": reject_faces has bits above bit 5");
    if (d->dst_slot != -1) {
        if (const int rc = check_slot(c, w, "destination", d->dst_slot)) return rc;
        if (const int rc = check_component(c, w, "destination contour", d->dst_contour)) return rc;
        if (d->combine < VR_MORPH_REPLACE || d->combine > VR_MORPH_ANDNOT) return fail(c, VR_ERR_INVALID_ARG, w + ": unknown combine");
    }
    if (d->label_slot != -1) {
        if (const int rc = check_slot(c, w, "label", d->label_slot)) return rc;
        if (const int rc = check_component(c, w, "label channel", d->label_channel)) return rc;
    }
    if (d->dst_slot != -1 && d->label_slot != -1) {
        if (d->dst_slot != d->label_slot) return fail(c, VR_ERR_INVALID_ARG, w + ": the contour and the label map must lie in the same slot");
        if (d->dst_contour == d->label_channel) return fail(c, VR_ERR_INVALID_ARG, w + ": the contour and the label map must lie in different components");
    }
    if ((d->max_components != 0) != (d->components != nullptr))
        return fail(c, VR_ERR_INVALID_ARG, w + ": components must be NULL exactly when max_components is 0");
    if (const int rc = check_filled(c, w, "source", d->src_slot)) return rc;
    const DevVolume& v = c->vols[d->src_slot].vol;
    if (const int rc = check_box(c, w, d->box_lo, d->box_hi, v)) return rc;
    const int written = comp_written_slot(*d);
    if (written < 0) return VR_OK;
    const DevVolume& m = c->vols[written].vol;
    return m.data ? check_same_dims(c, w, "destination", m, "source", v) : VR_OK;
}

// keep_largest: the (at most) K passing components with the most voxels, ties to the smaller number; pass[i] = voxels, or 0
void comp_winners(const std::vector<unsigned long long>& pass, unsigned keep, CompFilter* F)
{
    std::vector<std::pair<unsigned long long, unsigned>> cand;
    for (size_t i = 0; i < pass.size(); ++i)
        if (pass[i] != 0) cand.emplace_back(pass[i], (unsigned)i);
    const size_t k = std::min<size_t>(keep, cand.size());
    std::partial_sort(cand.begin(), cand.begin() + (std::ptrdiff_t)k, cand.end(),
                      [](const auto& a, const auto& b) { return a.first != b.first ? a.first > b.first : a.second < b.second; });
    F->n_winners = (unsigned)k;
    for (size_t i = 0; i < k; ++i) F->winners[i] = cand[i].second;
}

// The call itself, every argument checked and the device drained.  dst: the written slot's voxels, nullptr when no slot is written;
// `fresh`: they were allocated and zeroed by this call.  P takes its three phases; when a slot is written a fourth begins behind them
// (the shell's: the slot's rebuild).  A table that is too small (VR_ERR_INVALID_ARG) and a label map of more than VR_COMP_MAX_LABEL
// components (VR_ERR_UNSUPPORTED) fill the result and the counters and write nothing.
int run_components(vr_ctx* c, const vr_components_desc& d, float4* dst, bool fresh, vr_components_result* result, Phases& P)
{
    CompState& K = c->comp;
    hipStream_t s = c->stream;
    const DevVolume& v = c->vols[d.src_slot].vol;
    if (result) std::memset(result, 0, sizeof *result);
    const bool want_contour = dst && d.dst_slot >= 0, want_labels = dst && d.label_slot >= 0;

    CompGrid G;
    std::memset(&G, 0, sizeof G);
    unsigned long long box;
    G.b = bit_rows(v, d.box_lo, d.box_hi, &box);
    G.rows = (unsigned)(d.box_hi[1] - d.box_lo[1]);
    G.conn = d.connectivity;
    const unsigned long long bwords = G.b.box_words;
    const size_t nw = G.b.words();
    if (const int rc = grow(c, c->bit_row_scratch, 2 * nw, true)) return rc;  // (drained: a smaller scratch is freed at once)
    unsigned long long* const S = c->bit_row_scratch.p;
    unsigned long long* const R = S + nw;
    G.s = S;
    if (bwords != 0)
        if (const int rc = grow(c, K.base, (size_t)bwords, true)) return rc;
    VR_HIP(c, K.io.first_use());
    CompWords* const dw = K.io.d;
    CompWords& hw = *K.io.h.p;
    std::memset(&hw, 0, sizeof hw);
    hw.packed = hw.result = CountBox::empty();

    // pack
    VR_HIP(c, P.begin());
    VR_HIP(c, K.io.push(s));
    VR_HIP(c, hipMemsetAsync(S, 0, (want_contour ? 2 : 1) * nw * sizeof(unsigned long long), s));
    if (const int rc = tool_pack(c, v.data, d.src_contour, G.b, S, &dw->packed)) return rc;
    if (bwords != 0 && d.background) {
        hipLaunchKernelGGL(comp_complement_kernel, dim3(lane_blocks(bwords)), dim3(256), 0, s, G.b, S);
        VR_HIP(c, hipGetLastError());
    }
    VR_HIP(c, P.begin());

    // the runs, their scan, the merge, the flatten
    unsigned long long nodes = 0;
    if (bwords != 0) {
        hipLaunchKernelGGL(comp_starts_kernel, dim3(lane_blocks(bwords)), dim3(256), 0, s, G, K.base.p);
        VR_HIP(c, hipGetLastError());
        if (const int rc = tool_scan(c, K.base.p, bwords, K.base.p, &dw->nodes)) return rc;
        VR_HIP(c, hipMemcpyAsync(&hw.nodes, &dw->nodes, sizeof hw.nodes, hipMemcpyDeviceToHost, s));
        VR_HIP(c, hipStreamSynchronize(s));
        nodes = hw.nodes;
    }
    if (nodes > kCompNodesMax) return fail(c, VR_ERR_UNSUPPORTED, "vr_mask_components: more than 2^32 - 1 run nodes in one call (" + std::to_string(nodes) + ")");
    const unsigned n = (unsigned)nodes;
    CompNodes N = {K.base.p, n, nullptr, nullptr, nullptr, nullptr};
    const unsigned nblocks = lane_blocks(n);
    if (n != 0) {
        for (DevBuf<unsigned>* b : {&K.parent, &K.root, &K.row, &K.ab})
            if (const int rc = grow(c, *b, n, true)) return rc;
        N.parent = K.parent.p, N.root = K.root.p, N.row = K.row.p, N.ab = K.ab.p;
        hipLaunchKernelGGL(comp_runs_kernel, dim3(lane_blocks(bwords)), dim3(256), 0, s, G, N);
        hipLaunchKernelGGL(comp_merge_kernel, dim3(nblocks), dim3(256), 0, s, G, N, dw);
        hipLaunchKernelGGL(comp_flatten_kernel, dim3(nblocks), dim3(256), 0, s, (const unsigned*)N.parent, n, N.root);
        VR_HIP(c, hipGetLastError());
    }
    VR_HIP(c, P.begin());

    // the numbering
    if (n != 0) {
        hipLaunchKernelGGL(comp_leaders_kernel, dim3(nblocks), dim3(256), 0, s, (const unsigned*)N.root, n, N.parent);
        VR_HIP(c, hipGetLastError());
        if (const int rc = tool_scan(c, N.parent, n, N.parent, &dw->components)) return rc;
    }
    VR_HIP(c, K.io.pull(s));
    VR_HIP(c, hipStreamSynchronize(s));
    const unsigned long long ncomp = hw.components;
    K.report.counters[0] = box, K.report.counters[1] = nodes, K.report.counters[2] = hw.pairs;

    // the statistics, the selection
    if (ncomp != 0) {
        if (const int rc = grow(c, K.table, (size_t)ncomp, true)) return rc;
        if (const int rc = grow(c, K.sel, (size_t)ncomp, true)) return rc;
        CompFilter F;
        std::memset(&F, 0, sizeof F);
        F.min_voxels = d.min_voxels, F.max_voxels = d.max_voxels, F.reject_faces = d.reject_faces;
        F.by_winners = d.keep_largest != 0;
        if (F.by_winners)
            if (const int rc = grow(c, K.pass, (size_t)ncomp, true)) return rc;
        const unsigned cblocks = lane_blocks(ncomp);
        hipLaunchKernelGGL(comp_init_kernel, dim3(nblocks), dim3(256), 0, s, G, N, K.table.p);
        hipLaunchKernelGGL(comp_stats_kernel, dim3(nblocks), dim3(256), 0, s, G, N, K.table.p);
        hipLaunchKernelGGL(comp_pass_kernel, dim3(cblocks), dim3(256), 0, s, (const vr_component*)K.table.p, ncomp, F, K.sel.p, K.pass.p, dw);
        VR_HIP(c, hipGetLastError());
        if (F.by_winners) {
            std::vector<unsigned long long> pass((size_t)ncomp);
            VR_HIP(c, hipMemcpyAsync(pass.data(), K.pass.p, (size_t)ncomp * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
            VR_HIP(c, hipStreamSynchronize(s));
            comp_winners(pass, d.keep_largest, &F);
            hipLaunchKernelGGL(comp_pick_kernel, dim3(1), dim3(64), 0, s, F, K.sel.p);
        }
        hipLaunchKernelGGL(comp_result_kernel, dim3(cblocks), dim3(256), 0, s, (const vr_component*)K.table.p, ncomp, (const unsigned*)K.sel.p, dw);
        VR_HIP(c, hipGetLastError());
        VR_HIP(c, K.io.pull(s));
        VR_HIP(c, hipStreamSynchronize(s));
    }
    if (result) {
        result->n_components = ncomp;
        result->n_selected = hw.selected;
        result->voxels = d.background ? box - hw.packed.voxels : hw.packed.voxels;
        result->largest = hw.largest;
        copy_count_box(hw.result, &result->selected_voxels, result->lo, result->hi);
    }
    if (d.max_components != 0 && d.max_components < ncomp)
        return short_of_room(c, P, "vr_mask_components: the mask has " + std::to_string(ncomp) + " components, the table holds " +
                                       std::to_string(d.max_components));
    if (want_labels && ncomp > VR_COMP_MAX_LABEL)
        return fail(c, VR_ERR_UNSUPPORTED, "vr_mask_components: a label map of " + std::to_string(ncomp) + " components (labels are f32: at most 2^24)");

    // the writes, the copy back
    if (dst && bwords != 0) {
        if (want_contour && n != 0) hipLaunchKernelGGL(comp_expand_kernel, dim3(nblocks), dim3(256), 0, s, G, N, (const unsigned*)K.sel.p, R);
        const CompWrite P = {dst, want_contour ? d.dst_contour : -1, want_labels ? d.label_channel : -1, R, {d.combine, fresh ? 1 : 0}};
        hipLaunchKernelGGL(comp_write_kernel, dim3(tool_blocks(bwords)), dim3(256), 0, s, G, N, P);
        VR_HIP(c, hipGetLastError());
    }
    if (d.max_components != 0 && ncomp != 0)
        VR_HIP(c, hipMemcpyAsync(d.components, K.table.p, (size_t)ncomp * sizeof(vr_component), hipMemcpyDeviceToHost, s));
    if (!dst) return VR_OK;  // (the shell ends the third phase and waits for it)
    VR_HIP(c, P.begin());
    VR_HIP(c, hipStreamSynchronize(s));
    return VR_OK;
}

}  // namespace

extern "C" {

int vr_components_whole(const vr_ctx* c, int src_slot, int src_contour, vr_components_desc* out)
{
    if (!c || !out) return VR_ERR_INVALID_ARG;
    if (!is_slot(src_slot) || !is_component(src_contour)) return VR_ERR_INVALID_ARG;
    if (!c->vols[src_slot].vol.data) return VR_ERR_NOT_READY;
    std::memset(out, 0, sizeof *out);
    out->src_slot = src_slot;
    out->src_contour = src_contour;
    out->connectivity = VR_COMP_FACES;
    whole_box(c->vols[src_slot].vol, out->box_hi);
    out->min_voxels = 1;
    out->max_voxels = UINT64_MAX;
    out->dst_slot = out->label_slot = -1;
    out->combine = VR_MORPH_REPLACE;
    return VR_OK;
}

int vr_mask_components(vr_ctx* c, const vr_components_desc* desc, vr_components_result* result)
{
    if (!c) return VR_ERR_INVALID_ARG;
    if (const int rc = check_components(c, desc)) return rc;
    ToolReport& report = c->comp.report;
    const int written = comp_written_slot(*desc);
    if (written < 0) return data_tool_call(c, report, [&](Phases& P) { return run_components(c, *desc, nullptr, false, result, P); });
    Phases P = {report, c->stream};
    return mask_tool_call(c, "vr_mask_components", desc->src_slot, written, report,
                          [&](float4* dst, bool fresh) { return run_components(c, *desc, dst, fresh, result, P); });
}

int vr_components_counters(vr_ctx* c, uint64_t out[3]) { return tool_counters(c, &vr_ctx::comp, out, "vr_components_counters"); }

int vr_components_timing(vr_ctx* c, float ms[4]) { return tool_timing(c, &vr_ctx::comp, ms, "vr_components_timing"); }

}  // extern "C"
