// vr_api_tools.h -- what the voxel tools (the histograms of vr_api_views.h, vr_api_segment.h, vr_api_morph.h, vr_api_dist.h,
// vr_api_raster.h, vr_api_outline.h, vr_api_components.h, vr_api_resample.h, vr_api_mesh.h) share on the host: the rules for a slot, a
// component, a box and a second slot, a walk's units (vr_units.h) or word rows (vr_bitrows.h) and its grid, the two launch rules, the pack
// of a contour, the prefix scan (vr_scan.h), the opening and the closing of a report, and the two shells of a call: into a mask slot
// (mask_tool_call), and returning data without writing a slot (data_tool_call).
#pragma once

namespace {

constexpr unsigned kToolBlocks = 512;  // persistent workgroups of four wavefronts: two per CU of the 256

// vr_set_kernel_flavour(1) asks for the plain form of a tool: no settling, no skipping, everything loaded
bool plain_form(const vr_ctx* c) { return (c->flavour == 0 ? c->default_flavour : c->flavour) == 1; }

bool is_slot(int slot) { return slot >= 0 && slot < VR_MAX_VOLUMES; }
bool is_component(int k) { return k >= 0 && k <= 3; }  // a contour of a mask, a channel of a volume

// `what`: which slot or component of the descriptor, as the message names it ("source", "destination channel")
int check_slot(vr_ctx* c, const std::string& who, const char* what, int slot)
{
    return is_slot(slot) ? VR_OK : fail(c, VR_ERR_INVALID_ARG, who + ": bad " + what + " slot");
}
int check_component(vr_ctx* c, const std::string& who, const std::string& what, int k)
{
    return is_component(k) ? VR_OK : fail(c, VR_ERR_INVALID_ARG, who + ": the " + what + " must be 0 .. 3");
}
int check_filled(vr_ctx* c, const std::string& who, const char* what, int slot)
{
    return c->vols[slot].vol.data ? VR_OK : fail(c, VR_ERR_NOT_READY, who + ": " + what + " slot " + std::to_string(slot) + " is empty");
}

int check_box(vr_ctx* c, const std::string& who, const int32_t lo[3], const int32_t hi[3], const DevVolume& vol)
{
    const int n[3] = {vol.nx, vol.ny, vol.nz};
    for (int a = 0; a < 3; ++a)
        if (lo[a] < 0 || lo[a] > hi[a] || hi[a] > n[a]) return fail(c, VR_ERR_INVALID_ARG, who + ": the box must be 0 <= lo <= hi <= n on every axis");
    return VR_OK;
}

int check_same_dims(vr_ctx* c, const std::string& who, const char* other_is, const DevVolume& other, const char* vol_is, const DevVolume& vol)
{
    if (other.nx == vol.nx && other.ny == vol.ny && other.nz == vol.nz) return VR_OK;
    return fail(c, VR_ERR_INVALID_ARG, who + ": the " + other_is + "'s dimensions differ from the " + vol_is + "'s");
}

// The 4 x 4 x 4 brick units that meet a (checked) box; *voxels = the voxels of the box.  An empty box has no units: some un is 0.
BoxUnits box_units(const int32_t lo[3], const int32_t hi[3], unsigned long long* voxels)
{
    BoxUnits B;
    unsigned long long units = 1;
    *voxels = 1;
    for (int a = 0; a < 3; ++a) {
        B.lo[a] = lo[a];
        B.hi[a] = hi[a];
        B.u0[a] = lo[a] >> 2;
        B.un[a] = hi[a] > lo[a] ? ((hi[a] + 3) >> 2) - B.u0[a] : 0;
        units *= (unsigned long long)B.un[a];
        *voxels *= (unsigned long long)(hi[a] - lo[a]);
    }
    B.units = (unsigned)units;  // (vr_histogram alone takes volumes whose units could pass 2^32, and refuses such a box)
    return B;
}

// The word rows of a volume's bit-rows that meet a (checked) box; *voxels = the voxels of the box.  An empty box has no words.
BitRows bit_rows(const DevVolume& v, const int32_t lo[3], const int32_t hi[3], unsigned long long* voxels)
{
    BitRows B = {v.nx, v.ny, v.nz, (v.nx + 63) >> 6};  // (wx = ceil(nx / 64))
    *voxels = 1;
    for (int a = 0; a < 3; ++a) {
        B.lo[a] = lo[a];
        B.hi[a] = hi[a];
        *voxels *= (unsigned long long)(hi[a] - lo[a]);
    }
    B.bw0 = B.lo[0] >> 6;
    B.bw = ((B.hi[0] + 63) >> 6) - B.bw0;
    B.box_words = *voxels == 0 ? 0ull : (unsigned long long)B.bw * (unsigned long long)(B.hi[1] - B.lo[1]) * (unsigned long long)(B.hi[2] - B.lo[2]);
    return B;
}

void whole_box(const DevVolume& v, int32_t hi[3]) { hi[0] = v.nx, hi[1] = v.ny, hi[2] = v.nz; }  // (a descriptor's lo stays 0)

// The two launch rules, workgroups of 256: persistent, one wavefront per unit or word (tool_blocks); one lane per element, beyond
// 4 x kToolBlocks workgroups the kernels' loops go round (lane_blocks)
unsigned tool_blocks(unsigned long long n) { return n < 4 ? 1u : (n / 4 < kToolBlocks ? (unsigned)(n / 4) : kToolBlocks); }
unsigned lane_blocks(unsigned long long n) { return (unsigned)std::min<unsigned long long>((n + 255ull) / 256ull, 4ull * kToolBlocks); }

// Packs contour `contour` of `voxels` into the bit-rows `bits` (zeroed by the caller, whose extent it knows) on the context's stream;
// *d_count (device) takes their count and bounding box.  An empty box has no words: nothing is launched.
int tool_pack(vr_ctx* c, const float4* voxels, int contour, const BitRows& b, unsigned long long* bits, CountBox* d_count)
{
    if (b.box_words == 0) return VR_OK;
    const BitPack P = {voxels, contour, b, bits, d_count};
    hipLaunchKernelGGL(bit_pack_kernel, dim3(tool_blocks(b.box_words)), dim3(256), 0, c->stream, P);
    VR_HIP(c, hipGetLastError());
    return VR_OK;
}

// out[i] = in[0] + .. + in[i - 1] for i < n (in == out is allowed), *d_total = the sum of all, on the context's stream; n > 0.
// The tile sums are the context's (vr_ctx::scan_sums says why one buffer serves every caller).
int tool_scan(vr_ctx* c, const unsigned* in, unsigned long long n, unsigned* out, unsigned long long* d_total)
{
    const unsigned long long nb = (n + kScanTile - 1) / kScanTile;
    if (const int rc = grow(c, c->scan_sums, (size_t)nb, true)) return rc;
    unsigned long long* const sums = c->scan_sums.p;
    hipLaunchKernelGGL(scan_sums_kernel, dim3((unsigned)nb), dim3(256), 0, c->stream, in, n, sums);
    hipLaunchKernelGGL(scan_spine_kernel, dim3(1), dim3(256), 0, c->stream, sums, nb, d_total);
    hipLaunchKernelGGL(scan_apply_kernel, dim3((unsigned)nb), dim3(256), 0, c->stream, in, n, (const unsigned long long*)sums, out);
    VR_HIP(c, hipGetLastError());
    return VR_OK;
}

// a device count and box into a result's count / lo / hi (zeroed before): the box only if anything was counted
void copy_count_box(const CountBox& b, uint64_t* voxels, int32_t lo[3], int32_t hi[3])
{
    *voxels = b.voxels;
    for (int a = 0; a < 3 && b.voxels != 0; ++a) {
        lo[a] = b.lo[a];
        hi[a] = b.hi[a];
    }
}

template <typename State>
int tool_counters(vr_ctx* c, State vr_ctx::*tool, uint64_t out[3], const char* who)
{
    if (!c) return VR_ERR_INVALID_ARG;
    if (!out) return fail(c, VR_ERR_INVALID_ARG, std::string(who) + ": out is NULL");
    for (int i = 0; i < 3; ++i) out[i] = (c->*tool).report.counters[i];
    return VR_OK;
}
template <typename State>
int tool_timing(vr_ctx* c, State vr_ctx::*tool, float ms[4], const char* who)
{
    if (!c) return VR_ERR_INVALID_ARG;
    if (!ms) return fail(c, VR_ERR_INVALID_ARG, std::string(who) + ": ms is NULL");
    for (int i = 0; i < 4; ++i) ms[i] = (c->*tool).report.ms[i];
    return VR_OK;
}

// Opens a report for a call (the device drained): clears the sticky error, creates the events on first use, zeroes the times.
int open_report(vr_ctx* c, ToolReport& report)
{
    (void)hipGetLastError();
    for (Event& e : report.ev)  // (first use)
        if (!e) VR_HIP(c, e.create());
    for (float& t : report.ms) t = 0.0f;
    return VR_OK;
}

// Closes a report over its first `phases` phases, ev[0 .. phases - 1] recorded: records the event that ends the last one, waits for it
// and takes the times.  The later phases stay at zero; no phase, nothing to wait for.
int close_report(vr_ctx* c, ToolReport& report, int phases)
{
    if (phases == 0) return VR_OK;
    VR_HIP(c, hipEventRecord(report.ev[phases], c->stream));
    VR_HIP(c, hipEventSynchronize(report.ev[phases]));
    for (int i = 0; i < phases; ++i)
        if (hipEventElapsedTime(&report.ms[i], report.ev[i], report.ev[i + 1]) != hipSuccess) report.ms[i] = 0.0f;
    return VR_OK;
}

// The phases of a call as its run function marks them: begin() records the report's next event on the stream.  Returning
// short_of_room(..) is the run function's word that the counting was done (result and counters are this call's) and the error is only
// about the caller's capacity: the one failure that still counts, its phases timed like a success's.
struct Phases {
    ToolReport& report;
    hipStream_t stream;
    int begun = 0;
    bool short_of_room = false;
    hipError_t begin() { return hipEventRecord(report.ev[begun++], stream); }
};
int short_of_room(vr_ctx* c, Phases& P, const std::string& msg) { return P.short_of_room = true, fail(c, VR_ERR_INVALID_ARG, msg); }

// The shell of a data call that writes no slot, its descriptor checked: drains, opens the report, runs the tool -- run(Phases&), on the
// context's stream -- and closes the report over the phases it began (a call that ended early leaves the later ones at zero).  A failure
// that does not count leaves every time at zero.  Synchronous on return.
template <typename Run>
int data_tool_call(vr_ctx* c, ToolReport& report, Run run)
{
    if (const int rc = drain(c)) return rc;  // renders on the caller's streams may still be in flight; the bit-row scratch is taken
    if (const int rc = open_report(c, report)) return rc;
    Phases P = {report, c->stream};
    const int rc = run(P);
    if (rc != VR_OK && !P.short_of_room) {
        (void)hipStreamSynchronize(c->stream);
        return rc;
    }
    if (const int rc2 = close_report(c, report, P.begun)) return rc2;
    return rc;
}

// The shell of a data-preparation call into slot `dst_slot`, its descriptor checked.  An empty slot is created with the dimensions
// dims = (nx, ny, nz), zeroed; run(float4* dst, bool fresh) is the tool, on the context's stream, and records report.ev[0 .. 3].
template <typename Run>
int mask_tool_call(vr_ctx* c, const char* who, const int dims[3], int dst_slot, ToolReport& report, Run run)
{
    if (const int rc = drain(c)) return rc;  // asynchronous renders on the caller's streams may still read the destination slot
    VolumeSlot& D = c->vols[dst_slot];
    const uint16_t nx = (uint16_t)dims[0], ny = (uint16_t)dims[1], nz = (uint16_t)dims[2];
    const bool fresh = !D.vol.data;
    if (fresh) {  // every component +0.0f
        const size_t n = (size_t)nx * ny * nz;
        float4* dst;
        if (D.voxels && D.voxels.cap != n) D.voxels.release();
        if (const int rc = voxels_for_upload(c, dst_slot, n, &dst)) return rc;
        const hipError_t e = hipMemsetAsync(dst, 0, n * sizeof(float4), c->stream);
        if (e != hipSuccess) {
            D.voxels.release();
            return fail(c, VR_ERR_HIP, std::string(who) + ": hipMemsetAsync failed: " + hipGetErrorString(e));
        }
    }
    int rc = open_report(c, report);  // (a slot that could not be created has left the earlier call's report)
    if (rc == VR_OK) rc = run(D.voxels, fresh);
    if (rc != VR_OK) {
        (void)hipStreamSynchronize(c->stream);
        if (fresh) D.voxels.release();  // (the slot stays empty)
        return rc;
    }
    rc = fresh ? bind_voxels(c, dst_slot, nx, ny, nz) : refresh_bricks(c, dst_slot);
    return rc != VR_OK ? rc : close_report(c, report, 4);
}

// ... an empty slot taking the dimensions of slot `dims_of_slot`: a mask on its volume's grid
template <typename Run>
int mask_tool_call(vr_ctx* c, const char* who, int dims_of_slot, int dst_slot, ToolReport& report, Run run)
{
    const DevVolume& v = c->vols[dims_of_slot].vol;
    const int n[3] = {v.nx, v.ny, v.nz};
    return mask_tool_call(c, who, n, dst_slot, report, run);
}

}  // namespace
