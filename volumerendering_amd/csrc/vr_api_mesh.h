// vr_api_mesh.h -- surface extraction on the device (vr_volume_mesh; the kernels are vr_mesh.h's, the scan vr_scan.h's): the checks of
// a descriptor and the call itself.  A data call that writes no slot, like vr_mask_outlines (data_tool_call, vr_api_tools.h): it drains
// the device, runs on the context's stream, looks at the device words between the counting and the emitting phases and is synchronous
// on return; no launch's bookkeeping and no other tool's report is touched.  Part of vr_api.hip's translation unit.
#pragma once

namespace {

constexpr unsigned long long kMeshMax = 0x7fffffffull;  // vertices, and triangles, of one call

// the descriptor's own fields (VR_ERR_INVALID_ARG), then what the context must hold (VR_ERR_NOT_READY, the box)
int check_mesh(vr_ctx* c, const vr_mesh_desc* d)
{
    const std::string w("vr_volume_mesh");
    if (!d) return fail(c, VR_ERR_INVALID_ARG, w + ": the descriptor is NULL");
    if (const int rc = check_slot(c, w, "source", d->src_slot)) return rc;
    if (const int rc = check_component(c, w, "channel", d->channel)) return rc;
    if (!std::isfinite(d->level)) return fail(c, VR_ERR_INVALID_ARG, w + ": the level must be finite");
    if (d->cap != 0 && d->cap != 1) return fail(c, VR_ERR_INVALID_ARG, w + ": cap must be 0 or 1");
    if ((d->max_vertices != 0) != (d->vertices != nullptr)) return fail(c, VR_ERR_INVALID_ARG, w + ": vertices must be NULL exactly when max_vertices is 0");
    if ((d->max_triangles != 0) != (d->triangles != nullptr)) return fail(c, VR_ERR_INVALID_ARG, w + ": triangles must be NULL exactly when max_triangles is 0");
    if (const int rc = check_filled(c, w, "source", d->src_slot)) return rc;
    return check_box(c, w, d->box_lo, d->box_hi, c->vols[d->src_slot].vol);
}

// The call itself, every argument checked and the device drained; P takes its (at most four) phases.
int run_mesh(vr_ctx* c, const vr_mesh_desc& d, vr_mesh_result* result, Phases& P)
{
    MeshState& M = c->mesh;
    hipStream_t s = c->stream;
    const DevVolume& v = c->vols[d.src_slot].vol;
    if (result) std::memset(result, 0, sizeof *result);

    MeshGrid G;
    std::memset(&G, 0, sizeof G);
    G.val = reinterpret_cast<const float*>(v.data) + d.channel;
    G.nx = v.nx, G.ny = v.ny, G.nz = v.nz;
    unsigned long long box = 1;
    bool cells = true;
    for (int a = 0; a < 3; ++a) {
        G.lo[a] = d.box_lo[a];
        G.hi[a] = d.box_hi[a];
        G.e[a] = d.box_lo[a] - d.cap;
        G.ln[a] = d.box_hi[a] - d.box_lo[a] + 2 * d.cap;
        box *= (unsigned long long)(d.box_hi[a] - d.box_lo[a]);
        cells = cells && G.ln[a] >= 2;
    }
    G.lw = (G.ln[0] + 63) >> 6;
    G.words = (unsigned long long)G.lw * (unsigned long long)G.ln[1] * (unsigned long long)G.ln[2];
    G.level = d.level;
    auto done = [&](const MeshWords& w) {
        M.report.counters[0] = w.stats[0], M.report.counters[1] = w.stats[1], M.report.counters[2] = w.stats[2];
        M.active_cells = w.cells.voxels;
    };
    if (box == 0) return done(MeshWords{}), VR_OK;  // (no real point: nothing is inside)

    if (const int rc = grow(c, c->bit_row_scratch, (size_t)G.words, true)) return rc;
    if (cells) {
        if (const int rc = grow(c, M.masks, (size_t)G.words * 8u, true)) return rc;
        if (const int rc = grow(c, M.vbase, (size_t)G.words, true)) return rc;
        if (const int rc = grow(c, M.tbase, (size_t)G.words, true)) return rc;
    }
    VR_HIP(c, M.io.first_use());
    MeshWords* const dw = M.io.d;
    MeshWords& hw = *M.io.h.p;
    std::memset(&hw, 0, sizeof hw);
    hw.cells = CountBox::empty();
    unsigned long long* const bits = c->bit_row_scratch.p;

    // pack
    VR_HIP(c, P.begin());
    const bool plain = plain_form(c) || d.channel != 3;
    if (!plain) {  // exact settling by the slot's range records (of .a: channel 3)
        G.bnx = skip_bricks(v.nx);
        G.bny = skip_bricks(v.ny);
        if (!prepare_range(c, s, d.src_slot, G.bnx, G.bny, skip_bricks(v.nz), &G.bricks)) return VR_ERR_HIP;
    }
    VR_HIP(c, M.io.push(s));
    if (plain) hipLaunchKernelGGL(mesh_pack_kernel<true>, dim3(tool_blocks(G.words)), dim3(256), 0, s, G, bits, dw);
    else hipLaunchKernelGGL(mesh_pack_kernel<false>, dim3(tool_blocks(G.words)), dim3(256), 0, s, G, bits, dw);
    VR_HIP(c, hipGetLastError());
    VR_HIP(c, P.begin());

    // the crossings and the cases of every word, their two scans (a lattice thinner than 2 points on an axis has no cells)
    if (cells) {
        hipLaunchKernelGGL(mesh_count_kernel, dim3(lane_blocks(G.words)), dim3(256), 0, s, G, (const unsigned long long*)bits, M.masks.p, M.vbase.p,
                           M.tbase.p, dw);
        VR_HIP(c, hipGetLastError());
        if (const int rc = tool_scan(c, M.vbase.p, G.words, M.vbase.p, &dw->vertices)) return rc;
        if (const int rc = tool_scan(c, M.tbase.p, G.words, M.tbase.p, &dw->triangles)) return rc;
    }
    VR_HIP(c, M.io.pull(s));
    VR_HIP(c, hipStreamSynchronize(s));
    const unsigned long long nv = hw.vertices, nt = hw.triangles;
    if (nv > kMeshMax || nt > kMeshMax)
        return fail(c, VR_ERR_UNSUPPORTED, "vr_volume_mesh: more than 2^31 - 1 vertices or triangles in one call (" + std::to_string(nv) + ", " +
                                               std::to_string(nt) + ")");
    if (result) {
        result->n_vertices = (uint32_t)nv;
        result->n_triangles = (uint32_t)nt;
        result->inside = hw.inside;
        copy_count_box(hw.cells, &result->cells, result->lo, result->hi);
    }
    done(hw);
    if (d.max_vertices == 0 && d.max_triangles == 0) return VR_OK;  // the counting call
    if (d.max_vertices < nv || d.max_triangles < nt)
        return short_of_room(c, P, "vr_volume_mesh: the surface needs " + std::to_string(nv) + " vertices and " + std::to_string(nt) +
                                        " triangles, the buffers hold " + std::to_string(d.max_vertices) + " and " + std::to_string(d.max_triangles));
    if (nv == 0) return VR_OK;  // (no crossing edge: no triangle either)

    // emit, copy back
    if (const int rc = grow(c, M.vertices, (size_t)nv * 3u, true)) return rc;
    if (const int rc = grow(c, M.triangles, (size_t)nt * 3u, true)) return rc;
    VR_HIP(c, P.begin());
    hipLaunchKernelGGL(mesh_vertex_kernel, dim3(tool_blocks(G.words)), dim3(256), 0, s, G, (const unsigned long long*)M.masks.p, (const unsigned*)M.vbase.p,
                       (unsigned)nv, M.vertices.p);
    VR_HIP(c, hipGetLastError());
    VR_HIP(c, P.begin());
    hipLaunchKernelGGL(mesh_triangle_kernel, dim3(tool_blocks(G.words)), dim3(256), 0, s, G, (const unsigned long long*)bits,
                       (const unsigned long long*)M.masks.p, (const unsigned*)M.vbase.p, (const unsigned*)M.tbase.p, (unsigned)nt, M.triangles.p);
    VR_HIP(c, hipGetLastError());
    VR_HIP(c, hipMemcpyAsync(d.vertices, M.vertices.p, (size_t)nv * 3u * sizeof(float), hipMemcpyDeviceToHost, s));
    VR_HIP(c, hipMemcpyAsync(d.triangles, M.triangles.p, (size_t)nt * 3u * sizeof(unsigned), hipMemcpyDeviceToHost, s));
    VR_HIP(c, hipStreamSynchronize(s));
    return VR_OK;
}

}  // namespace

extern "C" {

int vr_mesh_whole(const vr_ctx* c, int src_slot, vr_mesh_desc* out)
{
    if (!c || !out) return VR_ERR_INVALID_ARG;
    if (!is_slot(src_slot)) return VR_ERR_INVALID_ARG;
    if (!c->vols[src_slot].vol.data) return VR_ERR_NOT_READY;
    std::memset(out, 0, sizeof *out);
    out->src_slot = src_slot;
    out->channel = 3;
    out->level = 0.5f;
    whole_box(c->vols[src_slot].vol, out->box_hi);
    return VR_OK;
}

int vr_volume_mesh(vr_ctx* c, const vr_mesh_desc* desc, vr_mesh_result* result)
{
    if (!c) return VR_ERR_INVALID_ARG;
    if (const int rc = check_mesh(c, desc)) return rc;
    return data_tool_call(c, c->mesh.report, [&](Phases& P) { return run_mesh(c, *desc, result, P); });
}

int vr_mesh_counters(vr_ctx* c, uint64_t out[4])
{
    if (const int rc = tool_counters(c, &vr_ctx::mesh, out, "vr_mesh_counters")) return rc;
    out[3] = c->mesh.active_cells;
    return VR_OK;
}

int vr_mesh_timing(vr_ctx* c, float ms[4]) { return tool_timing(c, &vr_ctx::mesh, ms, "vr_mesh_timing"); }

}  // extern "C"
