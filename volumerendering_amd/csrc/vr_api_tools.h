// vr_api_tools.h -- what the voxel tools (the histograms of vr_api_views.h, vr_api_segment.h, vr_api_morph.h, vr_api_dist.h,
// vr_api_raster.h, vr_api_resample.h) share on the host: the rules for a slot, a component, a box and a second slot, a walk's units (vr_units.h) or word
// rows (vr_bitrows.h) and its grid, the shell and the report of a call into a mask slot.
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

unsigned tool_blocks(unsigned long long n) { return n < 4 ? 1u : (n / 4 < kToolBlocks ? (unsigned)(n / 4) : kToolBlocks); }

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

// The shell of a data-preparation call into slot `dst_slot`, its descriptor checked.  An empty slot is created with the dimensions
// dims = (nx, ny, nz), zeroed; run(float4* dst, bool fresh) is the tool, on the context's stream, and records report.ev[0 .. 3].
template <typename Run>
int mask_tool_call(vr_ctx* c, const char* who, const int dims[3], int dst_slot, ToolReport& report, Run run)
{
    if (const int rc = drain(c)) return rc;  // asynchronous renders on the caller's streams may still read the destination slot
    (void)hipGetLastError();
    for (Event& e : report.ev)  // (first use)
        if (!e) VR_HIP(c, e.create());
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
    for (float& t : report.ms) t = 0.0f;
    if (const int rc = run(D.voxels, fresh)) {
        (void)hipStreamSynchronize(c->stream);
        if (fresh) D.voxels.release();  // (the slot stays empty)
        return rc;
    }
    if (const int rc = fresh ? bind_voxels(c, dst_slot, nx, ny, nz) : refresh_bricks(c, dst_slot)) return rc;
    VR_HIP(c, hipEventRecord(report.ev[4], c->stream));
    VR_HIP(c, hipEventSynchronize(report.ev[4]));
    for (int i = 0; i < 4; ++i)
        if (hipEventElapsedTime(&report.ms[i], report.ev[i], report.ev[i + 1]) != hipSuccess) report.ms[i] = 0.0f;
    return VR_OK;
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
