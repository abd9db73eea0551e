// vr_api_tools.h -- what the voxel tools (the histograms of vr_api_views.h, vr_api_segment.h, vr_api_morph.h, vr_api_dist.h) share on the host: the
// rules for a box and a second slot, a walk's units and grid (vr_units.h), the shell and the report of a call into a mask slot.
#pragma once

namespace {

constexpr unsigned kToolBlocks = 512;  // persistent workgroups of four wavefronts: two per CU of the 256

// vr_set_kernel_flavour(1) asks for the plain form of a tool: no settling, no skipping, everything loaded
bool plain_form(const vr_ctx* c) { return (c->flavour == 0 ? c->default_flavour : c->flavour) == 1; }

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

void whole_box(const DevVolume& v, int32_t hi[3]) { hi[0] = v.nx, hi[1] = v.ny, hi[2] = v.nz; }  // (a descriptor's lo stays 0)

unsigned tool_blocks(unsigned long long n) { return n < 4 ? 1u : (n / 4 < kToolBlocks ? (unsigned)(n / 4) : kToolBlocks); }

// a device count and box into a result's voxels / lo / hi (zeroed before): the box only if anything was counted
template <typename Result>
void copy_count_box(const CountBox& b, Result* r)
{
    r->voxels = b.voxels;
    for (int a = 0; a < 3 && b.voxels != 0; ++a) {
        r->lo[a] = b.lo[a];
        r->hi[a] = b.hi[a];
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

// The shell of a data-preparation call into mask slot `dst_slot`, its descriptor checked.  An empty slot gets the dimensions of slot
// `dims_of_slot`, zeroed; run(float4* dst, bool fresh) is the tool, on the context's stream, and records report.ev[0 .. 3].
template <typename Run>
int mask_tool_call(vr_ctx* c, const char* who, int dims_of_slot, int dst_slot, ToolReport& report, Run run)
{
    if (const int rc = drain(c)) return rc;  // asynchronous renders on the caller's streams may still read the destination slot
    (void)hipGetLastError();
    for (Event& e : report.ev)  // (first use)
        if (!e) VR_HIP(c, e.create());
    VolumeSlot& D = c->vols[dst_slot];
    const DevVolume& v = c->vols[dims_of_slot].vol;
    const uint16_t nx = (uint16_t)v.nx, ny = (uint16_t)v.ny, nz = (uint16_t)v.nz;
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

}  // namespace
