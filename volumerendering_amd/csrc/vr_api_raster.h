// vr_api_raster.h -- polygon rasterisation on the device (vr_mask_polygons; the kernels are vr_raster.h's): the checks of a descriptor, the
// work list (which rows of which polygon a wavefront takes) and the call itself.  A data-preparation call like vr_mask_morph: it drains
// the device, runs on the context's stream, ends with bind_voxels for a slot it created and with refresh_bricks otherwise, and is
// synchronous on return.  Part of vr_api.hip's translation unit.
#pragma once

namespace {

constexpr int32_t kPolyCoordMax = 1 << 29;   // of a point coordinate and an origin value, in magnitude
constexpr uint32_t kPolySpacingMax = 1u << 20;
constexpr int kRasterRowsPerItem = 8;         // rows of one polygon that a wavefront takes at a time

// ceil(a / b) for b > 0
long long ceil_div(long long a, long long b) { return a >= 0 ? (a + b - 1) / b : -((-a) / b); }

// the descriptor's own fields (VR_ERR_INVALID_ARG), then what the context must hold (VR_ERR_NOT_READY, the box, the destination)
int check_polygons(vr_ctx* c, const vr_polygons_desc* d)
{
    const std::string w("vr_mask_polygons");
    if (!d) return fail(c, VR_ERR_INVALID_ARG, w + ": the descriptor is NULL");
    if (const int rc = check_slot(c, w, "grid", d->grid_slot)) return rc;
    if (const int rc = check_slot(c, w, "destination", d->dst_slot)) return rc;
    if (d->contours < 1 || d->contours > 15) return fail(c, VR_ERR_INVALID_ARG, w + ": contours must be 1 .. 15");
    if (d->rule != VR_POLY_EVEN_ODD && d->rule != VR_POLY_UNION) return fail(c, VR_ERR_INVALID_ARG, w + ": unknown rule");
    if (d->combine < VR_MORPH_REPLACE || d->combine > VR_MORPH_ANDNOT) return fail(c, VR_ERR_INVALID_ARG, w + ": unknown combine");
    for (int a = 0; a < 2; ++a) {
        if (d->spacing[a] == 0 || d->spacing[a] > kPolySpacingMax) return fail(c, VR_ERR_INVALID_ARG, w + ": a spacing must be 1 .. 2^20");
        if (d->origin[a] < -kPolyCoordMax || d->origin[a] > kPolyCoordMax) return fail(c, VR_ERR_INVALID_ARG, w + ": the origin must lie within +-2^29");
    }
    if (d->n_points != 0 && !d->points) return fail(c, VR_ERR_INVALID_ARG, w + ": points is NULL");
    if (d->n_polygons != 0 && !d->polygons) return fail(c, VR_ERR_INVALID_ARG, w + ": polygons is NULL");
    for (uint32_t i = 0; i < d->n_polygons; ++i) {
        const vr_polygon& p = d->polygons[i];
        if ((uint64_t)p.first + p.count > d->n_points) return fail(c, VR_ERR_INVALID_ARG, w + ": polygon " + std::to_string(i) + " reads beyond the points");
        if (!is_component(p.contour))  // (asked here first: the message's name is put together only for a polygon that fails)
            return check_component(c, w, "contour of polygon " + std::to_string(i), p.contour);
        if (!((d->contours >> p.contour) & 1)) return fail(c, VR_ERR_INVALID_ARG, w + ": the contour of polygon " + std::to_string(i) + " is not in contours");
    }
    for (size_t i = 0; i < (size_t)d->n_points * 2; ++i)
        if (d->points[i] < -kPolyCoordMax || d->points[i] > kPolyCoordMax) return fail(c, VR_ERR_INVALID_ARG, w + ": a point coordinate lies outside +-2^29");
    if (const int rc = check_filled(c, w, "grid", d->grid_slot)) return rc;
    const DevVolume& v = c->vols[d->grid_slot].vol;
    if (const int rc = check_box(c, w, d->box_lo, d->box_hi, v)) return rc;
    const DevVolume& m = c->vols[d->dst_slot].vol;
    return m.data ? check_same_dims(c, w, "destination", m, "grid", v) : VR_OK;
}

// The work of a (checked) call: the polygons that are rasterised, with the voxel span of a row each can set, and their items.
// `plain`: every polygon of a slice inside the box, every row of the box.  *skipped = the polygons that are not rasterised.
void raster_work(const vr_polygons_desc& d, bool plain, std::vector<RasterPoly>& polys, std::vector<RasterItem>& items, unsigned long long* skipped)
{
    const bool empty = d.box_hi[0] <= d.box_lo[0] || d.box_hi[1] <= d.box_lo[1];  // (no voxel on any slice: no items)
    *skipped = 0;
    for (uint32_t i = 0; i < d.n_polygons; ++i) {
        const vr_polygon& p = d.polygons[i];
        if (p.slice < d.box_lo[2] || p.slice >= d.box_hi[2]) {
            ++*skipped;
            continue;
        }
        RasterPoly G = {p.first, p.count, p.slice, p.contour, d.box_lo[0], d.box_hi[0]};
        long long j0 = d.box_lo[1], j1 = d.box_hi[1];
        if (!plain) {  // the rows whose centres lie in [ymin, ymax) and the voxels whose centres lie in [xmin, xmax), within the box
            if (p.count == 0) {
                ++*skipped;
                continue;
            }
            const int32_t* q = d.points + (size_t)p.first * 2;
            int32_t xmin = q[0], xmax = q[0], ymin = q[1], ymax = q[1];
            for (uint32_t e = 1; e < p.count; ++e) {
                xmin = std::min(xmin, q[2 * e]);
                xmax = std::max(xmax, q[2 * e]);
                ymin = std::min(ymin, q[2 * e + 1]);
                ymax = std::max(ymax, q[2 * e + 1]);
            }
            const long long s0 = std::max<long long>(ceil_div((long long)xmin - d.origin[0], d.spacing[0]), d.box_lo[0]);
            const long long s1 = std::min<long long>(ceil_div((long long)xmax - d.origin[0], d.spacing[0]), d.box_hi[0]);
            j0 = std::max<long long>(ceil_div((long long)ymin - d.origin[1], d.spacing[1]), d.box_lo[1]);
            j1 = std::min<long long>(ceil_div((long long)ymax - d.origin[1], d.spacing[1]), d.box_hi[1]);
            if (s0 >= s1 || j0 >= j1) {
                ++*skipped;
                continue;
            }
            G.s0 = (int)s0;
            G.s1 = (int)s1;
        }
        if (empty) continue;  // (rasterised, and nothing to do)
        const unsigned index = (unsigned)polys.size();
        polys.push_back(G);
        for (long long j = j0; j < j1; j += kRasterRowsPerItem)
            items.push_back(RasterItem{index, (unsigned short)j, (unsigned short)std::min<long long>(kRasterRowsPerItem, j1 - j)});
    }
}

// The call itself, every argument checked and the device drained.  `fresh`: the destination slot's voxels were allocated and zeroed by
// this call.
int run_polygons(vr_ctx* c, const vr_polygons_desc& d, float4* dst, bool fresh, vr_polygons_result* result)
{
    RasterState& R = c->raster;
    hipStream_t s = c->stream;
    const DevVolume& v = c->vols[d.grid_slot].vol;
    RasterParams P;
    std::memset(&P, 0, sizeof P);
    unsigned long long box;
    const BitRows W = P.b = bit_rows(v, d.box_lo, d.box_hi, &box);
    P.dst = dst;
    P.c = {d.combine, fresh ? 1 : 0};
    P.contours = d.contours;
    P.ox = d.origin[0];
    P.oy = d.origin[1];
    P.sx = d.spacing[0];
    P.sy = d.spacing[1];

    std::vector<RasterPoly> polys;
    std::vector<RasterItem> items;
    unsigned long long skipped = 0;
    raster_work(d, plain_form(c), polys, items, &skipped);
    if (items.size() > 0x7fffffffull) return fail(c, VR_ERR_INVALID_ARG, "vr_mask_polygons: more than 2^31 work items");

    // the working buffers (first use; the device is drained and every earlier use was synchronous: a smaller buffer is freed at once)
    const size_t nw = W.words();
    if (const int rc = grow(c, c->bit_row_scratch, 4 * nw, true)) return rc;
    unsigned long long* const words = c->bit_row_scratch.p;  // R_k of every contour
    VR_HIP(c, R.io.first_use());
    const size_t b_points = (size_t)d.n_points * sizeof(int2), b_polys = polys.size() * sizeof(RasterPoly), b_items = items.size() * sizeof(RasterItem);
    const size_t bytes = b_points + b_polys + b_items;
    if (R.h_stage.cap < bytes) VR_HIP(c, R.h_stage.reserve(bytes));
    if (const int rc = grow(c, R.d_stage, bytes, true)) return rc;
    if (b_points) std::memcpy(R.h_stage.p, d.points, b_points);
    if (b_polys) std::memcpy(R.h_stage.p + b_points, polys.data(), b_polys);
    if (b_items) std::memcpy(R.h_stage.p + b_points + b_polys, items.data(), b_items);
    P.pts = reinterpret_cast<const int2*>(R.d_stage.p);
    P.polys = reinterpret_cast<const RasterPoly*>(R.d_stage.p + b_points);
    P.items = reinterpret_cast<const RasterItem*>(R.d_stage.p + b_points + b_polys);
    P.n_items = (unsigned)items.size();
    for (int k = 0; k < 4; ++k) P.bits[k] = words + (size_t)k * nw;
    P.w = R.io.d;

    VR_HIP(c, hipEventRecord(R.report.ev[0], s));
    if (bytes) VR_HIP(c, hipMemcpyAsync(R.d_stage, R.h_stage, bytes, hipMemcpyHostToDevice, s));
    for (CountBox& b : R.io.h.p->r) b = CountBox::empty();
    VR_HIP(c, R.io.push(s));
    VR_HIP(c, hipMemsetAsync(words, 0, 4 * nw * sizeof(unsigned long long), s));
    VR_HIP(c, hipEventRecord(R.report.ev[1], s));

    if (P.n_items != 0) {
        const unsigned blocks = tool_blocks(P.n_items);
        if (d.rule == VR_POLY_UNION) hipLaunchKernelGGL(raster_rows_kernel<true>, dim3(blocks), dim3(256), 0, s, P);
        else hipLaunchKernelGGL(raster_rows_kernel<false>, dim3(blocks), dim3(256), 0, s, P);
        VR_HIP(c, hipGetLastError());
    }
    VR_HIP(c, hipEventRecord(R.report.ev[2], s));

    if (W.box_words != 0) {
        hipLaunchKernelGGL(raster_write_kernel, dim3(tool_blocks(W.box_words)), dim3(256), 0, s, P);
        VR_HIP(c, hipGetLastError());
    }
    VR_HIP(c, R.io.pull(s));
    VR_HIP(c, hipEventRecord(R.report.ev[3], s));
    VR_HIP(c, hipStreamSynchronize(s));
    R.report.counters[0] = d.n_polygons;
    R.report.counters[1] = d.n_polygons - skipped;
    R.report.counters[2] = skipped;
    if (result) {
        std::memset(result, 0, sizeof *result);
        for (int k = 0; k < 4; ++k) copy_count_box(R.io.h.p->r[k], &result->voxels[k], result->lo[k], result->hi[k]);
    }
    return VR_OK;
}

}  // namespace

extern "C" {

int vr_polygons_whole(const vr_ctx* c, int grid_slot, int dst_slot, vr_polygons_desc* out)
{
    if (!c || !out) return VR_ERR_INVALID_ARG;
    if (!is_slot(grid_slot) || !is_slot(dst_slot)) return VR_ERR_INVALID_ARG;
    if (!c->vols[grid_slot].vol.data) return VR_ERR_NOT_READY;
    std::memset(out, 0, sizeof *out);
    out->grid_slot = grid_slot;
    out->dst_slot = dst_slot;
    out->contours = 1;
    out->rule = VR_POLY_EVEN_ODD;
    out->combine = VR_MORPH_REPLACE;
    whole_box(c->vols[grid_slot].vol, out->box_hi);
    out->spacing[0] = out->spacing[1] = 1;
    return VR_OK;
}

int vr_mask_polygons(vr_ctx* c, const vr_polygons_desc* desc, vr_polygons_result* result)
{
    if (!c) return VR_ERR_INVALID_ARG;
    if (const int rc = check_polygons(c, desc)) return rc;
    return mask_tool_call(c, "vr_mask_polygons", desc->grid_slot, desc->dst_slot, c->raster.report,
                          [&](float4* dst, bool fresh) { return run_polygons(c, *desc, dst, fresh, result); });
}

int vr_polygons_counters(vr_ctx* c, uint64_t out[3]) { return tool_counters(c, &vr_ctx::raster, out, "vr_polygons_counters"); }

int vr_polygons_timing(vr_ctx* c, float ms[4]) { return tool_timing(c, &vr_ctx::raster, ms, "vr_polygons_timing"); }

}  // extern "C"
