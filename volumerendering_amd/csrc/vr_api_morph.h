// vr_api_morph.h -- mask morphology and contour algebra on the device (vr_mask_morph; the kernels are vr_morph.h's) and the two host
// fillers of a structuring element.  vr_mask_morph is a data-preparation call like vr_segment_grow: it drains the device, runs on the
// context's stream, ends with bind_voxels for a slot it created and with refresh_bricks otherwise, and is synchronous on return.
// Part of vr_api.hip's translation unit.
#pragma once

namespace {

constexpr int kMorphSide = 2 * VR_MORPH_MAX_RADIUS + 1;

// the rules of include/vr.h for an element; nullptr if it meets them, else what is wrong
const char* check_element(const vr_morph_element& e)
{
    for (int a = 0; a < 3; ++a)
        if (e.radius[a] < 0 || e.radius[a] > VR_MORPH_MAX_RADIUS) return "a radius of the element is outside 0 .. 31";
    const int rx = e.radius[0], ry = e.radius[1], rz = e.radius[2];
    if (e.half[rz][ry] < 0) return "the element does not hold the origin";
    for (int dz = 0; dz <= rz; ++dz)
        for (int dy = 0; dy <= ry; ++dy) {
            const int h = e.half[rz + dz][ry + dy];
            if (h < -1 || h > rx) return "a half-chord of the element is outside -1 .. rx";
            if (e.half[rz - dz][ry + dy] != h || e.half[rz + dz][ry - dy] != h || e.half[rz - dz][ry - dy] != h)
                return "the element is not symmetric under reflection of y or z";
        }
    return nullptr;
}

// the descriptor's own fields (VR_ERR_INVALID_ARG), then what the context must hold (VR_ERR_NOT_READY, the box, the destination)
int check_morph(vr_ctx* c, const vr_morph_desc* d)
{
    const std::string w("vr_mask_morph");
    if (!d) return fail(c, VR_ERR_INVALID_ARG, w + ": the descriptor is NULL");
    if (const int rc = check_slot(c, w, "source", d->src_slot)) return rc;
    if (const int rc = check_slot(c, w, "destination", d->dst_slot)) return rc;
    if (const int rc = check_component(c, w, "source contour", d->src_contour)) return rc;
    if (const int rc = check_component(c, w, "destination contour", d->dst_contour)) return rc;
    if (d->op < VR_MORPH_NONE || d->op > VR_MORPH_OPEN) return fail(c, VR_ERR_INVALID_ARG, w + ": unknown op");
    if (d->combine < VR_MORPH_REPLACE || d->combine > VR_MORPH_ANDNOT) return fail(c, VR_ERR_INVALID_ARG, w + ": unknown combine");
    if (d->op != VR_MORPH_NONE)
        if (const char* what = check_element(d->element)) return fail(c, VR_ERR_INVALID_ARG, w + ": " + what);
    if (const int rc = check_filled(c, w, "source", d->src_slot)) return rc;
    const DevVolume& v = c->vols[d->src_slot].vol;
    if (const int rc = check_box(c, w, d->box_lo, d->box_hi, v)) return rc;
    const DevVolume& m = c->vols[d->dst_slot].vol;
    return m.data ? check_same_dims(c, w, "destination", m, "source", v) : VR_OK;
}

// a half-open voxel region; empty when some hi <= lo
struct MorphRegion {
    int lo[3], hi[3];
    bool empty() const { return hi[0] <= lo[0] || hi[1] <= lo[1] || hi[2] <= lo[2]; }
};

// One dilation launch over the words that meet `reg` (a part of the box): dst is zeroed first and keeps zeros outside them.
// *computed = the voxels of the box in those words.
int morph_pass(vr_ctx* c, const MorphParams& P, const unsigned long long* src, unsigned long long* dst, size_t nw, bool comp,
               const MorphRegion& reg, unsigned long long* computed)
{
    hipStream_t s = c->stream;
    VR_HIP(c, hipMemsetAsync(dst, 0, nw * sizeof(unsigned long long), s));
    *computed = 0;
    if (reg.empty()) return VR_OK;
    MorphPass S;
    S.src = src;
    S.dst = dst;
    S.rw0 = reg.lo[0] >> 6;
    S.rw = ((reg.hi[0] + 63) >> 6) - S.rw0;
    S.ry0 = reg.lo[1];
    S.ry = reg.hi[1] - reg.lo[1];
    S.rz0 = reg.lo[2];
    S.rz = reg.hi[2] - reg.lo[2];
    S.words = (unsigned long long)S.rw * (unsigned long long)S.ry * (unsigned long long)S.rz;
    const int x0 = S.rw0 << 6 > P.b.lo[0] ? S.rw0 << 6 : P.b.lo[0], x1 = (S.rw0 + S.rw) << 6 < P.b.hi[0] ? (S.rw0 + S.rw) << 6 : P.b.hi[0];
    *computed = (unsigned long long)(x1 - x0) * (unsigned long long)S.ry * (unsigned long long)S.rz;
    const unsigned blocks = (unsigned)((S.words + 255ull) / 256ull);  // (at most 2^32 / 64 words: below 2^18 blocks)
    if (comp) hipLaunchKernelGGL(morph_dilate_kernel<true>, dim3(blocks), dim3(256), 0, s, P, S);
    else hipLaunchKernelGGL(morph_dilate_kernel<false>, dim3(blocks), dim3(256), 0, s, P, S);
    VR_HIP(c, hipGetLastError());
    return VR_OK;
}

// The call itself, every argument checked and the device drained.  `fresh`: the destination slot's voxels were allocated and zeroed by
// this call.
int run_morph(vr_ctx* c, const vr_morph_desc& d, float4* dst, bool fresh, vr_morph_result* result)
{
    MorphState& M = c->morph;
    hipStream_t s = c->stream;
    const DevVolume& v = c->vols[d.src_slot].vol;
    MorphParams P;
    std::memset(&P, 0, sizeof P);
    unsigned long long box;
    const BitRows W = P.b = bit_rows(v, d.box_lo, d.box_hi, &box);
    P.dst = dst;
    P.dst_contour = d.dst_contour;
    P.c = {d.combine, fresh ? 1 : 0};
    const size_t nw = W.words();
    if (const int rc = grow(c, c->bit_row_scratch, 3 * nw, true)) return rc;  // (drained: a smaller scratch is freed at once)
    unsigned long long* const A = c->bit_row_scratch.p;  // the packed operand A', and the two buffers a dilation pass writes in turn
    unsigned long long* const B = A + nw;
    unsigned long long* const C = A + 2 * nw;
    if (!M.rows) VR_HIP(c, M.rows.reserve((size_t)kMorphSide * kMorphSide));
    if (!M.h_rows) VR_HIP(c, M.h_rows.reserve((size_t)kMorphSide * kMorphSide, true));
    VR_HIP(c, M.io.first_use());
    P.w = M.io.d;
    const bool plain = plain_form(c);
    const bool morph = d.op != VR_MORPH_NONE;
    const int rad[3] = {morph ? d.element.radius[0] : 0, morph ? d.element.radius[1] : 0, morph ? d.element.radius[2] : 0};
    if (morph) {  // the element's rows, sorted by half-chord, largest first (a counting sort over h = rx .. 0)
        unsigned* rows = M.h_rows;
        int n = 0;
        for (int h = rad[0]; h >= 0; --h)
            for (int dz = -rad[2]; dz <= rad[2]; ++dz)
                for (int dy = -rad[1]; dy <= rad[1]; ++dy)
                    if (d.element.half[dz + rad[2]][dy + rad[1]] == h) rows[n++] = (unsigned)h | (unsigned)(dy + 32) << 8 | (unsigned)(dz + 32) << 16;
        P.n_rows = n;
        P.hmax = (int)(rows[0] & 0xFFu);  // (n >= 1: the origin's row)
        VR_HIP(c, hipMemcpyAsync(M.rows, M.h_rows, (size_t)n * sizeof(unsigned), hipMemcpyHostToDevice, s));
        P.rows = M.rows;
    }
    const unsigned blocks = tool_blocks(W.box_words);

    VR_HIP(c, hipEventRecord(M.report.ev[0], s));
    *M.io.h.p = MorphWords{CountBox::empty(), CountBox::empty()};
    VR_HIP(c, M.io.push(s));
    VR_HIP(c, hipMemsetAsync(A, 0, nw * sizeof(unsigned long long), s));
    if (const int rc = tool_pack(c, v.data, d.src_contour, W, A, &M.io.d.p->src)) return rc;
    VR_HIP(c, M.io.pull(s));
    VR_HIP(c, hipStreamSynchronize(s));
    const MorphWords packed = *M.io.h.p;
    VR_HIP(c, hipEventRecord(M.report.ev[1], s));

    // Where the result of a pass can be set: a dilation's within the bounding box of its source bits grown by the radii, an erosion's
    // within that bounding box itself (the origin is in E), both within the box.  The plain form takes the whole box.
    MorphRegion bb, grown, whole;
    for (int a = 0; a < 3; ++a) {
        whole.lo[a] = W.lo[a];
        whole.hi[a] = box == 0 ? W.lo[a] : W.hi[a];
        bb.lo[a] = packed.src.voxels ? packed.src.lo[a] : 0;
        bb.hi[a] = packed.src.voxels ? packed.src.hi[a] : 0;
        grown.lo[a] = bb.lo[a] - rad[a] > W.lo[a] ? bb.lo[a] - rad[a] : W.lo[a];
        grown.hi[a] = bb.hi[a] + rad[a] < W.hi[a] ? bb.hi[a] + rad[a] : W.hi[a];
        if (!packed.src.voxels) grown.hi[a] = grown.lo[a] = W.lo[a];
    }
    if (plain) bb = grown = whole;
    unsigned long long computed = 0;
    const unsigned long long* R = A;
    switch (d.op) {
    case VR_MORPH_DILATE:
        if (const int rc = morph_pass(c, P, A, B, nw, false, grown, &computed)) return rc;
        R = B;
        break;
    case VR_MORPH_ERODE:
        if (const int rc = morph_pass(c, P, A, B, nw, true, bb, &computed)) return rc;
        R = B;
        break;
    case VR_MORPH_CLOSE:  // (the dilation is empty outside `grown`, and the erosion of it is a part of it)
        if (const int rc = morph_pass(c, P, A, B, nw, false, grown, &computed)) return rc;
        if (const int rc = morph_pass(c, P, B, C, nw, true, grown, &computed)) return rc;
        R = C;
        break;
    case VR_MORPH_OPEN:  // (the erosion is a part of A': its bounding box lies within A''s)
        if (const int rc = morph_pass(c, P, A, B, nw, true, bb, &computed)) return rc;
        if (const int rc = morph_pass(c, P, B, C, nw, false, grown, &computed)) return rc;
        R = C;
        break;
    default: break;
    }
    P.r = R;
    VR_HIP(c, hipEventRecord(M.report.ev[2], s));

    if (W.box_words != 0) {
        hipLaunchKernelGGL(morph_write_kernel, dim3(blocks), dim3(256), 0, s, P);
        VR_HIP(c, hipGetLastError());
    }
    VR_HIP(c, M.io.pull(s));
    VR_HIP(c, hipEventRecord(M.report.ev[3], s));
    VR_HIP(c, hipStreamSynchronize(s));
    const MorphWords& w = *M.io.h.p;
    M.report.computed_of_box(box, computed);
    if (result) {
        std::memset(result, 0, sizeof *result);
        copy_count_box(w.result, &result->voxels, result->lo, result->hi);
        result->src_voxels = w.src.voxels;
    }
    return VR_OK;
}

void fill_element(vr_morph_element* e, int rx, int ry, int rz)
{
    std::memset(e->half, -1, sizeof e->half);
    e->radius[0] = rx;
    e->radius[1] = ry;
    e->radius[2] = rz;
}

}  // namespace

extern "C" {

int vr_morph_ball(const uint32_t spacing[3], uint32_t radius, vr_morph_element* out)
{
    if (!spacing || !out) return VR_ERR_INVALID_ARG;
    int r[3];
    for (int a = 0; a < 3; ++a) {
        if (spacing[a] == 0 || spacing[a] > (1u << 20)) return VR_ERR_INVALID_ARG;
        if (radius / spacing[a] > VR_MORPH_MAX_RADIUS) return VR_ERR_INVALID_ARG;
        r[a] = (int)(radius / spacing[a]);
    }
    fill_element(out, r[0], r[1], r[2]);
    // (|d| <= 31 and a spacing <= 2^20: a term is below 2^50, the sum of three below 2^52)
    const uint64_t rr = (uint64_t)radius * radius, sx = spacing[0], sy = spacing[1], sz = spacing[2];
    for (int dz = -r[2]; dz <= r[2]; ++dz)
        for (int dy = -r[1]; dy <= r[1]; ++dy) {
            const uint64_t ay = (uint64_t)(dy < 0 ? -dy : dy) * sy, az = (uint64_t)(dz < 0 ? -dz : dz) * sz;
            const uint64_t yz = ay * ay + az * az;
            int h = -1;
            for (int dx = 0; dx <= r[0]; ++dx) {
                const uint64_t ax = (uint64_t)dx * sx;
                if (ax * ax + yz <= rr) h = dx;
                else break;
            }
            out->half[dz + r[2]][dy + r[1]] = (int8_t)h;
        }
    return VR_OK;
}

int vr_morph_box(int rx, int ry, int rz, vr_morph_element* out)
{
    if (!out) return VR_ERR_INVALID_ARG;
    if (rx < 0 || rx > VR_MORPH_MAX_RADIUS || ry < 0 || ry > VR_MORPH_MAX_RADIUS || rz < 0 || rz > VR_MORPH_MAX_RADIUS) return VR_ERR_INVALID_ARG;
    fill_element(out, rx, ry, rz);
    for (int z = 0; z <= 2 * rz; ++z)
        for (int y = 0; y <= 2 * ry; ++y) out->half[z][y] = (int8_t)rx;
    return VR_OK;
}

int vr_morph_whole(const vr_ctx* c, int src_slot, int src_contour, int dst_slot, int dst_contour, int op, vr_morph_desc* out)
{
    if (!c || !out) return VR_ERR_INVALID_ARG;
    if (!is_slot(src_slot) || !is_slot(dst_slot) || !is_component(src_contour) || !is_component(dst_contour)) return VR_ERR_INVALID_ARG;
    if (op < VR_MORPH_NONE || op > VR_MORPH_OPEN) return VR_ERR_INVALID_ARG;
    if (!c->vols[src_slot].vol.data) return VR_ERR_NOT_READY;
    std::memset(out, 0, sizeof *out);
    out->src_slot = src_slot;
    out->src_contour = src_contour;
    out->dst_slot = dst_slot;
    out->dst_contour = dst_contour;
    out->op = op;
    out->combine = VR_MORPH_REPLACE;
    whole_box(c->vols[src_slot].vol, out->box_hi);
    const uint32_t unit[3] = {1, 1, 1};
    return vr_morph_ball(unit, 1, &out->element);
}

int vr_mask_morph(vr_ctx* c, const vr_morph_desc* desc, vr_morph_result* result)
{
    if (!c) return VR_ERR_INVALID_ARG;
    if (const int rc = check_morph(c, desc)) return rc;
    return mask_tool_call(c, "vr_mask_morph", desc->src_slot, desc->dst_slot, c->morph.report,
                          [&](float4* dst, bool fresh) { return run_morph(c, *desc, dst, fresh, result); });
}

int vr_morph_counters(vr_ctx* c, uint64_t out[3]) { return tool_counters(c, &vr_ctx::morph, out, "vr_morph_counters"); }

int vr_morph_timing(vr_ctx* c, float ms[4]) { return tool_timing(c, &vr_ctx::morph, ms, "vr_morph_timing"); }

}  // extern "C"
