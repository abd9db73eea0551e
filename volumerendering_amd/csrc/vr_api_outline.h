// vr_api_outline.h -- contour tracing on the device (vr_mask_outlines; the kernels are vr_outline.h's, the scan vr_scan.h's): the checks
// of a descriptor and the call itself.  A data call that writes no slot (data_tool_call, vr_api_tools.h): it drains the device, runs on
// the context's stream, looks at a device word between its phases (the node count, the rounds' outcome, the polygon count) and is
// synchronous on return; nothing derived from a slot is rebuilt and no launch's bookkeeping is touched.  Part of vr_api.hip's
// translation unit.
#pragma once

namespace {

constexpr unsigned long long kOutlineNodesMax = 0x7fffffffull;  // corners of one call

// the descriptor's own fields (VR_ERR_INVALID_ARG), then what the context must hold (VR_ERR_NOT_READY, the box, the coordinates' range)
int check_outlines(vr_ctx* c, const vr_outlines_desc* d)
{
    const std::string w("vr_mask_outlines");
    if (!d) return fail(c, VR_ERR_INVALID_ARG, w + ": the descriptor is NULL");
    if (const int rc = check_slot(c, w, "source", d->src_slot)) return rc;
    if (d->contours < 1 || d->contours > 15) return fail(c, VR_ERR_INVALID_ARG, w + ": contours must be 1 .. 15");
    if (d->connect != VR_OUTLINE_SPLIT && d->connect != VR_OUTLINE_JOIN) return fail(c, VR_ERR_INVALID_ARG, w + ": unknown connect");
    for (int a = 0; a < 2; ++a) {
        if (d->spacing[a] == 0 || d->spacing[a] > kPolySpacingMax) return fail(c, VR_ERR_INVALID_ARG, w + ": a spacing must be 1 .. 2^20");
        if (d->origin[a] < -kPolyCoordMax || d->origin[a] > kPolyCoordMax) return fail(c, VR_ERR_INVALID_ARG, w + ": the origin must lie within +-2^29");
        if (d->offset[a] >= d->spacing[a]) return fail(c, VR_ERR_INVALID_ARG, w + ": an offset must be below its spacing");
    }
    if ((d->max_points != 0) != (d->points != nullptr)) return fail(c, VR_ERR_INVALID_ARG, w + ": points must be NULL exactly when max_points is 0");
    if ((d->max_polygons != 0) != (d->polygons != nullptr)) return fail(c, VR_ERR_INVALID_ARG, w + ": polygons must be NULL exactly when max_polygons is 0");
    if (const int rc = check_filled(c, w, "source", d->src_slot)) return rc;
    if (const int rc = check_box(c, w, d->box_lo, d->box_hi, c->vols[d->src_slot].vol)) return rc;
    for (int a = 0; a < 2; ++a)  // the extreme vertices of the box (vertex i of an axis: lo <= i <= hi)
        for (const int32_t i : {d->box_lo[a], d->box_hi[a]}) {
            const long long v = (long long)d->origin[a] + (long long)i * (long long)d->spacing[a] - (long long)d->offset[a];
            if (v < -kPolyCoordMax || v > kPolyCoordMax) return fail(c, VR_ERR_INVALID_ARG, w + ": a vertex of the box lies outside +-2^29");
        }
    return VR_OK;
}

// fills *result from the device words of a call (pulled and the stream synchronised)
void outline_result(const OutlineWords& w, vr_outlines_result* result)
{
    if (!result) return;
    result->n_points = (uint32_t)w.nodes;
    result->n_polygons = (uint32_t)w.polygons;
    for (int k = 0; k < 4; ++k) {
        result->polygons_of[k] = w.polygons_of[k];
        result->points_of[k] = w.points_of[k];
        result->area2[k] = w.area2[k];
    }
}

// The call itself, every argument checked and the device drained; P takes its (at most four) phases.
int run_outlines(vr_ctx* c, const vr_outlines_desc& d, vr_outlines_result* result, Phases& P)
{
    OutlineState& O = c->outline;
    hipStream_t s = c->stream;
    const DevVolume& v = c->vols[d.src_slot].vol;
    if (result) std::memset(result, 0, sizeof *result);

    OutlineGrid G;
    std::memset(&G, 0, sizeof G);
    unsigned long long box;
    G.b = bit_rows(v, d.box_lo, d.box_hi, &box);
    for (int k = 0; k < 4; ++k)
        if ((d.contours >> k) & 1) G.kmap[G.nc++] = k;
    G.vwx = (v.nx >> 6) + 1;
    G.rows = (unsigned)(d.box_hi[1] - d.box_lo[1]) + 1u;
    G.slices = (unsigned)(d.box_hi[2] - d.box_lo[2]);
    G.vwords = (unsigned long long)G.nc * G.slices * G.rows * (unsigned)G.vwx;
    G.ox = (long long)d.origin[0] - (long long)d.offset[0];
    G.oy = (long long)d.origin[1] - (long long)d.offset[1];
    G.sx = d.spacing[0];
    G.sy = d.spacing[1];
    G.join = d.connect == VR_OUTLINE_JOIN;
    auto done = [&](unsigned long long nodes, unsigned long long polygons, unsigned long long rounds) {
        O.report.counters[0] = nodes, O.report.counters[1] = polygons, O.report.counters[2] = rounds;
    };
    if (box == 0) return done(0, 0, 0), VR_OK;  // (no voxel: no polygon)

    // the working buffers that do not depend on the mask (the device is drained: a smaller buffer is freed at once)
    const size_t nw = G.b.words();
    if (const int rc = grow(c, c->bit_row_scratch, (size_t)G.nc * nw, true)) return rc;
    if (const int rc = grow(c, O.masks, (size_t)G.vwords, true)) return rc;
    if (const int rc = grow(c, O.base, (size_t)G.vwords, true)) return rc;
    VR_HIP(c, O.io.first_use());
    OutlineWords* const dw = O.io.d;
    OutlineWords& hw = *O.io.h.p;
    std::memset(&hw, 0, sizeof hw);
    for (CountBox& b : hw.packed) b = CountBox::empty();
    for (int k = 0; k < G.nc; ++k) G.bits[k] = c->bit_row_scratch.p + (size_t)k * nw;

    // pack
    VR_HIP(c, P.begin());
    VR_HIP(c, O.io.push(s));
    VR_HIP(c, hipMemsetAsync(c->bit_row_scratch.p, 0, (size_t)G.nc * nw * sizeof(unsigned long long), s));
    for (int k = 0; k < G.nc; ++k)
        if (const int rc = tool_pack(c, v.data, G.kmap[k], G.b, c->bit_row_scratch.p + (size_t)k * nw, &dw->packed[k])) return rc;
    VR_HIP(c, P.begin());

    // corners, their scan, the links
    hipLaunchKernelGGL(outline_corners_kernel, dim3(lane_blocks(G.vwords)), dim3(256), 0, s, G, O.masks.p, O.base.p);
    VR_HIP(c, hipGetLastError());
    if (const int rc = tool_scan(c, O.base.p, G.vwords, O.base.p, &dw->nodes)) return rc;
    VR_HIP(c, hipMemcpyAsync(&hw.nodes, &dw->nodes, sizeof hw.nodes, hipMemcpyDeviceToHost, s));
    VR_HIP(c, hipStreamSynchronize(s));
    const unsigned long long nodes = hw.nodes;
    if (nodes > kOutlineNodesMax) return fail(c, VR_ERR_UNSUPPORTED, "vr_mask_outlines: more than 2^31 - 1 corners in one call (" + std::to_string(nodes) + ")");
    if (nodes == 0) return done(0, 0, 0), VR_OK;  // (every contour is empty in the box)
    const unsigned n = (unsigned)nodes;
    if (const int rc = grow(c, O.pred, n, true)) return rc;
    if (const int rc = grow(c, O.pt, n, true)) return rc;
    if (const int rc = grow(c, O.meta, n, true)) return rc;
    if (const int rc = grow(c, O.pidx, n, true)) return rc;
    if (const int rc = grow(c, O.pcount, n, true)) return rc;
    for (auto& b : O.st)
        if (const int rc = grow(c, b, n, true)) return rc;
    const OutlineNodes N = {O.masks.p, O.base.p, n, O.pred.p, O.pt.p, O.meta.p};
    const unsigned blocks = lane_blocks(n);
    VR_HIP(c, hipMemsetAsync(O.pred.p, 0, (size_t)n * sizeof(unsigned), s));
    hipLaunchKernelGGL(outline_link_kernel, dim3(blocks), dim3(256), 0, s, G, N, dw);
    VR_HIP(c, hipGetLastError());
    VR_HIP(c, P.begin());

    // leader and rank: one launch per round; the plain form runs every round a loop of all the nodes would need
    unsigned fixed = 0;
    while ((1ull << fixed) < nodes) ++fixed;
    hipLaunchKernelGGL(outline_rank_init_kernel, dim3(blocks), dim3(256), 0, s, (const unsigned*)O.pred.p, n, O.st[0].p);
    unsigned rounds = 0;
    int cur = 0;
    for (unsigned r = 0; r < fixed; ++r) {
        hipLaunchKernelGGL(outline_rank_kernel, dim3(blocks), dim3(256), 0, s, (const uint4*)O.st[cur].p, O.st[cur ^ 1].p, n, 1u << r, &dw->changed[r]);
        VR_HIP(c, hipGetLastError());
        cur ^= 1;
        ++rounds;
        if (plain_form(c)) continue;
        VR_HIP(c, hipMemcpyAsync(&hw.changed[r], &dw->changed[r], sizeof(unsigned), hipMemcpyDeviceToHost, s));
        VR_HIP(c, hipStreamSynchronize(s));
        if (!hw.changed[r]) break;
    }
    VR_HIP(c, P.begin());

    // the polygons: leaders, their scan, the counts of each contour
    const uint4* const st = O.st[cur].p;
    hipLaunchKernelGGL(outline_leaders_kernel, dim3(blocks), dim3(256), 0, s, st, n, O.pidx.p);
    VR_HIP(c, hipGetLastError());
    if (const int rc = tool_scan(c, O.pidx.p, n, O.pidx.p, &dw->polygons)) return rc;
    hipLaunchKernelGGL(outline_totals_kernel, dim3(1), dim3(64), 0, s, G, (const unsigned*)O.base.p, (const unsigned*)O.pidx.p, dw);
    VR_HIP(c, hipGetLastError());
    VR_HIP(c, O.io.pull(s));
    VR_HIP(c, hipStreamSynchronize(s));
    const unsigned long long polygons = hw.polygons;
    if (polygons > nodes / 4) return fail(c, VR_ERR_HIP, "vr_mask_outlines: internal error: a polygon of fewer than 4 corners");  // (the emit's room)
    outline_result(hw, result);
    done(nodes, polygons, rounds);
    if (d.max_points == 0 && d.max_polygons == 0) return VR_OK;  // the counting call
    if (d.max_points < nodes || d.max_polygons < polygons)
        return short_of_room(c, P, "vr_mask_outlines: the mask needs " + std::to_string(nodes) + " points and " + std::to_string(polygons) +
                                        " polygons, the buffers hold " + std::to_string(d.max_points) + " and " + std::to_string(d.max_polygons));

    // emit into the idle half of the rounds' buffers (16 bytes a node: 8 for its point, at most 4 for its share of a polygon), copy back
    int2* const points = reinterpret_cast<int2*>(O.st[cur ^ 1].p);
    vr_polygon* const polys = reinterpret_cast<vr_polygon*>(points + n);
    hipLaunchKernelGGL(outline_counts_kernel, dim3(blocks), dim3(256), 0, s, st, (const unsigned*)O.pred.p, (const unsigned*)O.pidx.p, n, O.pcount.p);
    VR_HIP(c, hipGetLastError());
    if (const int rc = tool_scan(c, O.pcount.p, polygons, O.pcount.p, &dw->points)) return rc;
    hipLaunchKernelGGL(outline_emit_kernel, dim3(blocks), dim3(256), 0, s, st, N, (const unsigned*)O.pidx.p, (const unsigned*)O.pcount.p, points, polys);
    VR_HIP(c, hipGetLastError());
    VR_HIP(c, hipMemcpyAsync(d.points, points, (size_t)n * sizeof(int2), hipMemcpyDeviceToHost, s));
    VR_HIP(c, hipMemcpyAsync(d.polygons, polys, (size_t)polygons * sizeof(vr_polygon), hipMemcpyDeviceToHost, s));
    VR_HIP(c, hipStreamSynchronize(s));
    return VR_OK;
}

}  // namespace

extern "C" {

int vr_outlines_whole(const vr_ctx* c, int src_slot, vr_outlines_desc* out)
{
    if (!c || !out) return VR_ERR_INVALID_ARG;
    if (!is_slot(src_slot)) return VR_ERR_INVALID_ARG;
    if (!c->vols[src_slot].vol.data) return VR_ERR_NOT_READY;
    std::memset(out, 0, sizeof *out);
    out->src_slot = src_slot;
    out->contours = 1;
    out->connect = VR_OUTLINE_SPLIT;
    whole_box(c->vols[src_slot].vol, out->box_hi);
    out->spacing[0] = out->spacing[1] = 1;
    return VR_OK;
}

int vr_mask_outlines(vr_ctx* c, const vr_outlines_desc* desc, vr_outlines_result* result)
{
    if (!c) return VR_ERR_INVALID_ARG;
    if (const int rc = check_outlines(c, desc)) return rc;
    return data_tool_call(c, c->outline.report, [&](Phases& P) { return run_outlines(c, *desc, result, P); });
}

int vr_outlines_counters(vr_ctx* c, uint64_t out[3]) { return tool_counters(c, &vr_ctx::outline, out, "vr_outlines_counters"); }

int vr_outlines_timing(vr_ctx* c, float ms[4]) { return tool_timing(c, &vr_ctx::outline, ms, "vr_outlines_timing"); }

}  // extern "C"
