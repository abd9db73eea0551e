// vr_api_volume.h -- the volume slots: uploads, normalisation, gradients, what is derived from the voxels (brick records, density
// plane, bricked copy, range records) and the volume layouts a launch binds.  Part of vr_api.hip's translation unit.
#pragma once

namespace {

// the grid helpers of vr_choice.h on a volume
BrickedGrid bricked_grid(const DevVolume& v) { return vr::bricked_grid(v.nx, v.ny, v.nz); }
bool volume_bricks_indexable(const DevVolume& v) { return vr::volume_bricks_indexable(v.nx, v.ny, v.nz); }

// The parameters of a launch that no kernel form changes; the volumes as the vec4 voxels and their density plane (the bricked copies
// replace them in use_bricked_copies).
// volume slot i as the vec4 voxels and their density plane
DevVolume linear_volume(const vr_ctx* c, int i)
{
    DevVolume v = c->vols[i].vol;
    const bool plane = c->layout_mode != 1 && c->vols[i].dens && c->vols[i].vol.data;
    v.dens = plane ? c->vols[i].dens.p : nullptr;
    v.a_base = plane ? reinterpret_cast<const char*>(c->vols[i].dens.p) : reinterpret_cast<const char*>(c->vols[i].vol.data) + 12;
    v.a_shift = plane ? 2 : 4;
    v.bricked = 0;
    v.brick_row = v.brick_slab = 0;
    const size_t lin_bytes = c->vols[i].bytes();
    v.data_bytes = lin_bytes > 0xFFFFFFFFull ? 0xFFFFFFFFu : (unsigned)lin_bytes;
    return v;
}

// the bricked copies (layout 0) are what the gathers read
void use_bricked_copy(const vr_ctx* c, int i, DevVolume& v)
{
    if (!c->vols[i].vol.data || !c->vols[i].bricked || !c->vols[i].bdens) return;
    const BrickedGrid g = bricked_grid(c->vols[i].vol);
    if (g.slots > 0xFFFFFFFFull) return;  // (indices are 32 bits)
    v.data = c->vols[i].bricked;
    v.a_base = reinterpret_cast<const char*>(c->vols[i].bdens.p);
    v.a_shift = 2;
    v.bricked = 1;
    v.brick_row = g.nbx * kVbN;
    v.brick_slab = g.nbx * g.nby * kVbN;
    v.data_bytes = g.slots * 16 > 0xFFFFFFFFull ? 0xFFFFFFFFu : (unsigned)(g.slots * 16);
}
void use_bricked_copies(const vr_ctx* c, MarchParams& P)
{
    for (int i = 0; i < VR_MAX_VOLUMES; ++i) use_bricked_copy(c, i, P.vol[i]);
}

// The empty-space brick grid of volume slot sv in P: bricks per axis and voxels per brick edge (exact in f32).
void fill_brick_grid(MarchParams& P, int sv, const DevVolume& v)
{
    P.skip_vol = sv;
    P.bnx = skip_bricks(v.nx);
    P.bny = skip_bricks(v.ny);
    P.bnz = skip_bricks(v.nz);
    P.bsx = (float)v.nx * kBrickInv;
    P.bsy = (float)v.ny * kBrickInv;
    P.bsz = (float)v.nz * kBrickInv;
}

// The range records of volume slot `slot` (bn bricks per axis): (re)builds them and the whole volume's range on `s` when a volume
// changed since they were built (no host wait), and orders a launch on another stream behind that build once.  *rec = the records,
// the return value the whole volume's range (both device), or nullptr after a failure (c->err says why).
const float2* prepare_range(vr_ctx* c, hipStream_t s, int slot, int bnx, int bny, int bnz, const float2** rec)
{
    const DevVolume& v = c->vols[slot].vol;
    const size_t nb = (size_t)bnx * bny * bnz;
    VolumeSlot& V = c->vols[slot];
    BuiltOn& built = V.proj_built;
    if (V.proj_epoch != c->brick_epoch || !V.proj_rec || !V.proj_range) {
        // (a volume change drained the device: nothing in flight reads the records; a smaller buffer is retired all the same)
        if (grow(c, V.proj_rec, nb, false)) return nullptr;
        if (!V.proj_range && V.proj_range.reserve(1) != hipSuccess) {
            fail(c, VR_ERR_OOM, "vr_render: no memory for the projection's volume range");
            return nullptr;
        }
        if (!built.ev && built.ev.create(hipEventDisableTiming) != hipSuccess) {
            fail(c, VR_ERR_HIP, "vr_render: hipEventCreateWithFlags failed");
            return nullptr;
        }
        hipLaunchKernelGGL(brick_range_kernel, dim3((unsigned)nb), dim3(64), 0, s, v.data, v.nx, v.ny, v.nz, bnx, bny, V.proj_rec);
        hipLaunchKernelGGL(range_reduce_kernel, dim3(1), dim3(1024), 0, s, (const float2*)V.proj_rec, (int)nb, V.proj_range);
        if (hipGetLastError() != hipSuccess || hipEventRecord(built.ev, s) != hipSuccess) {
            fail(c, VR_ERR_HIP, "vr_render: the projection's brick ranges could not be enqueued");
            return nullptr;
        }
        V.proj_epoch = c->brick_epoch;
        built.built(s);
    } else if (built.order_behind(s) != hipSuccess) {
        fail(c, VR_ERR_HIP, "vr_render: hipStreamWaitEvent failed");
        return nullptr;
    }
    *rec = V.proj_rec;
    return V.proj_range;
}

// The skipping projection (flavour 19) and isosurface (21): fills P's brick fields with volume 0's range records (prepare_range).
// The caller has checked bricks_indexable().
const float2* prepare_proj(vr_ctx* c, hipStream_t s, MarchParams& P)
{
    fill_brick_grid(P, 0, c->vols[0].vol);
    return prepare_range(c, s, 0, P.bnx, P.bny, P.bnz, &P.bricks);
}

// per-brick density / rgb maxima for the exact empty-space test (one pass over the volume; after every change)
int refresh_bricks(vr_ctx* c, int slot)
{
    (void)hipGetLastError();  // (see enqueue_render)
    VolumeSlot& V = c->vols[slot];
    const DevVolume& v = V.vol;
    c->skip.merged_stale = true;
    ++c->brick_epoch;
    for (auto& e : c->shadows.ring) e.valid = false;  // (the caller drained the device)
    const int bnx = skip_bricks(v.nx), bny = skip_bricks(v.ny), bnz = skip_bricks(v.nz);
    const size_t nbricks = (size_t)bnx * bny * bnz;
    VR_HIP(c, V.bricks.reserve(nbricks));
    hipLaunchKernelGGL(brick_max_kernel, dim3((unsigned)nbricks), dim3(64), 0, c->stream, v.data, v.nx, v.ny, v.nz, bnx, bny,
                       V.bricks);
    VR_HIP(c, hipGetLastError());
    // scalar density plane + "is .rgb the central difference of .a?" (vr_volume_layout bit 2)
    const size_t n = (size_t)v.nx * v.ny * v.nz;
    V.grad_derived = false;
    if (n > V.dens.cap) VR_HIP(c, V.dens.reserve(n));
    hipLaunchKernelGGL(extract_density_kernel, dim3(4096), dim3(256), 0, c->stream, v.data, V.dens, n);
    VR_HIP(c, hipGetLastError());
    unsigned* d_flag = reinterpret_cast<unsigned*>(c->d_counters.p);
    VR_HIP(c, hipMemsetAsync(d_flag, 0, sizeof(unsigned), c->stream));
    hipLaunchKernelGGL(verify_gradient_kernel, dim3((unsigned)((v.nx + 255) / 256), (unsigned)v.ny, (unsigned)v.nz), dim3(256), 0,
                       c->stream, v.data, V.dens, v.nx, v.ny, v.nz, d_flag);
    VR_HIP(c, hipGetLastError());
    unsigned flag = 1;
    VR_HIP(c, hipMemcpyAsync(&flag, d_flag, sizeof flag, hipMemcpyDeviceToHost, c->stream));
    VR_HIP(c, hipStreamSynchronize(c->stream));
    V.grad_derived = flag == 0;
    V.vol.dens = V.dens;
    {   // the bricked copy the march kernels gather from (DevVolume::bricked)
        const BrickedGrid g = bricked_grid(v);
        const size_t slots = g.slots;
        if (slots > V.bricked.cap) {
            V.bricked.release();
            V.bdens.release();
            // (the bricked copies cost 20 B per voxel on top of the reference layout's 16 + 4: when they do not fit, the kernels gather
            // from the x-fastest arrays as with vr_set_volume_layout(3) -- slower, not an error)
            if (V.bricked.reserve(slots) == hipSuccess && V.bdens.reserve(slots) != hipSuccess) V.bricked.release();
            (void)hipGetLastError();
        }
        if (!V.bricked) {
            VR_HIP(c, hipStreamSynchronize(c->stream));
            return VR_OK;
        }
        hipLaunchKernelGGL(rebrick_kernel, dim3(8192), dim3(256), 0, c->stream, v.data, V.bricked, V.bdens, v.nx,
                           v.ny, v.nz, g.nbx, g.nby, slots);
        VR_HIP(c, hipGetLastError());
        VR_HIP(c, hipStreamSynchronize(c->stream));
    }
    return VR_OK;
}

int check_slot(vr_ctx* c, int slot, const char* who)
{
    if (!c) return VR_ERR_INVALID_ARG;
    if (slot < 0 || slot >= VR_MAX_VOLUMES) return fail(c, VR_ERR_INVALID_ARG, std::string(who) + ": bad slot");
    if (!c->vols[slot].vol.data) return fail(c, VR_ERR_NOT_READY, std::string(who) + ": volume slot is empty");
    if (const int rc = drain(c)) return rc;  // asynchronous renders on the caller's streams may still read the slot
    (void)hipGetLastError();
    return VR_OK;
}

// The arguments of an upload into `slot`, then the device drained: asynchronous renders on the caller's streams may still read the slot.
int begin_upload(vr_ctx* c, int slot, const void* src, uint16_t nx, uint16_t ny, uint16_t nz, const std::string& who)
{
    if (!c) return VR_ERR_INVALID_ARG;
    if (slot < 0 || slot >= VR_MAX_VOLUMES) return fail(c, VR_ERR_INVALID_ARG, who + ": bad slot");
    if (!src) return fail(c, VR_ERR_INVALID_ARG, who + ": data is NULL");
    if (nx == 0 || ny == 0 || nz == 0) return fail(c, VR_ERR_INVALID_ARG, who + ": empty volume");
    if ((unsigned long long)nx * ny * nz > 0xFFFFFFFFull) return fail(c, VR_ERR_INVALID_ARG, who + ": more than 2^32 voxels");
    return drain(c);
}

// The voxel buffer an upload of n voxels into `slot` fills (the device has been drained): the slot's own when it has that size, else a
// new one, the slot emptied first.  The slot holds a volume only once bind_voxels has said so.
int voxels_for_upload(vr_ctx* c, int slot, size_t n, float4** d)
{
    VolumeSlot& V = c->vols[slot];
    if (V.vol.data && V.voxels.cap != n) {
        V.voxels.release();
        V.vol = DevVolume{};
    }
    if (!V.voxels) VR_HIP(c, V.voxels.reserve(n));
    *d = V.voxels;
    return VR_OK;
}

// ... and how a successful upload ends (a failed one into a new buffer releases it: the slot stays empty)
int bind_voxels(vr_ctx* c, int slot, uint16_t nx, uint16_t ny, uint16_t nz)
{
    VolumeSlot& V = c->vols[slot];
    V.vol.data = V.voxels;
    V.vol.nx = nx;
    V.vol.ny = ny;
    V.vol.nz = nz;
    return refresh_bricks(c, slot);
}

template <typename T>
int upload_raw(vr_ctx* c, int slot, const T* raw, uint16_t nx, uint16_t ny, uint16_t nz)
{
    if (const int rc = begin_upload(c, slot, raw, nx, ny, nz, "vr_volume_upload_raw")) return rc;
    const size_t n = (size_t)nx * ny * nz;
    (void)hipGetLastError();
    float4* d;
    if (const int rc = voxels_for_upload(c, slot, n, &d)) return rc;
    DevBuf<T> d_raw;
    hipError_t e = d_raw.reserve(n);
    if (e == hipSuccess) e = hipMemcpyAsync(d_raw, raw, n * sizeof(T), hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) {
        hipLaunchKernelGGL((broadcast_raw_kernel<T>), dim3(2048), dim3(256), 0, c->stream, d_raw, d, n);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    d_raw.release();
    if (e != hipSuccess) {
        if (!c->vols[slot].vol.data) c->vols[slot].voxels.release();
        return fail(c, e == hipErrorOutOfMemory ? VR_ERR_OOM : VR_ERR_HIP,
                    std::string("vr_volume_upload_raw: ") + hipGetErrorString(e));
    }
    return bind_voxels(c, slot, nx, ny, nz);
}

}  // namespace

extern "C" {

int vr_volume_upload_raw16(vr_ctx* c, int slot, const uint16_t* raw, uint16_t nx, uint16_t ny, uint16_t nz)
{
    return upload_raw(c, slot, raw, nx, ny, nz);
}
int vr_volume_upload_raw32(vr_ctx* c, int slot, const uint32_t* raw, uint16_t nx, uint16_t ny, uint16_t nz)
{
    return upload_raw(c, slot, raw, nx, ny, nz);
}

int vr_volume_normalize(vr_ctx* c, int slot, int normalization_value, int* used_value)
{
    int rc = check_slot(c, slot, "vr_volume_normalize");
    if (rc != VR_OK) return rc;
    float4* d = const_cast<float4*>(c->vols[slot].vol.data);
    const size_t n = (size_t)c->vols[slot].vol.nx * c->vols[slot].vol.ny * c->vols[slot].vol.nz;
    if (normalization_value == 0) {  // GetMaxNumber(): max of component [0], truncated
        unsigned* d_max = reinterpret_cast<unsigned*>(c->d_counters.p);
        VR_HIP(c, hipMemsetAsync(d_max, 0, sizeof(unsigned), c->stream));
        hipLaunchKernelGGL(max_component_kernel, dim3(2048), dim3(256), 0, c->stream, d, n, 0, d_max);
        VR_HIP(c, hipGetLastError());
        unsigned bits = 0;
        VR_HIP(c, hipMemcpyAsync(&bits, d_max, sizeof bits, hipMemcpyDeviceToHost, c->stream));
        VR_HIP(c, hipStreamSynchronize(c->stream));
        float mx;
        std::memcpy(&mx, &bits, sizeof mx);
        normalization_value = (int)(size_t)mx;
    }
    if (used_value) *used_value = normalization_value;
    hipLaunchKernelGGL(normalize_kernel, dim3(2048), dim3(256), 0, c->stream, d, n, normalization_value);
    VR_HIP(c, hipGetLastError());
    return refresh_bricks(c, slot);
}

int vr_volume_precompute_gradient(vr_ctx* c, int slot, int norm_to_zero_one)
{
    int rc = check_slot(c, slot, "vr_volume_precompute_gradient");
    if (rc != VR_OK) return rc;
    float4* d = const_cast<float4*>(c->vols[slot].vol.data);
    const DevVolume& v = c->vols[slot].vol;
    const size_t n = (size_t)v.nx * v.ny * v.nz;
    unsigned* d_max = reinterpret_cast<unsigned*>(c->d_counters.p);
    VR_HIP(c, hipMemsetAsync(d_max, 0, sizeof(unsigned), c->stream));
    dim3 block(256), grid((unsigned)((v.nx + 255) / 256), (unsigned)v.ny, (unsigned)v.nz);
    hipLaunchKernelGGL(gradient_kernel, grid, block, 0, c->stream, d, v.nx, v.ny, v.nz, norm_to_zero_one ? 1 : 0, d_max);
    VR_HIP(c, hipGetLastError());
    if (norm_to_zero_one) {
        hipLaunchKernelGGL(scale_gradient_kernel, dim3(2048), dim3(256), 0, c->stream, d, n, d_max);
        VR_HIP(c, hipGetLastError());
    }
    return refresh_bricks(c, slot);
}

int vr_volume_download(vr_ctx* c, int slot, float* vec4_voxels)
{
    int rc = check_slot(c, slot, "vr_volume_download");
    if (rc != VR_OK) return rc;
    if (!vec4_voxels) return fail(c, VR_ERR_INVALID_ARG, "vr_volume_download: destination is NULL");
    VR_HIP(c, hipMemcpy(vec4_voxels, c->vols[slot].vol.data, c->vols[slot].bytes(), hipMemcpyDeviceToHost));
    return VR_OK;
}

static int volume_upload_common(vr_ctx* c, int slot, const void* src, bool src_is_device, uint16_t nx, uint16_t ny,
                                uint16_t nz)
{
    if (const int rc = begin_upload(c, slot, src, nx, ny, nz, "vr_volume_upload")) return rc;
    const size_t voxels = (size_t)nx * ny * nz, bytes = voxels * sizeof(float4);
    float4* d;
    if (const int rc = voxels_for_upload(c, slot, voxels, &d)) return rc;
    hipError_t e = hipMemcpyAsync(d, src, bytes, src_is_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) {
        if (!c->vols[slot].vol.data) c->vols[slot].voxels.release();
        return fail(c, VR_ERR_HIP, std::string("vr_volume_upload: copy failed: ") + hipGetErrorString(e));
    }
    return bind_voxels(c, slot, nx, ny, nz);
}

int vr_volume_upload(vr_ctx* c, int slot, const float* vec4_voxels, uint16_t nx, uint16_t ny, uint16_t nz)
{
    return volume_upload_common(c, slot, vec4_voxels, false, nx, ny, nz);
}

int vr_volume_upload_device(vr_ctx* c, int slot, const void* d_vec4_voxels, uint16_t nx, uint16_t ny, uint16_t nz)
{
    return volume_upload_common(c, slot, d_vec4_voxels, true, nx, ny, nz);
}

int vr_set_volume_layout(vr_ctx* c, int mode)
{
    if (!c) return VR_ERR_INVALID_ARG;
    if (mode < 0 || mode > 3) return fail(c, VR_ERR_INVALID_ARG, "vr_set_volume_layout: unknown mode");
    if (mode == 2) return fail(c, VR_ERR_UNSUPPORTED, "vr_set_volume_layout: layout 2 (gradients derived on the fly) was removed");
    c->layout_mode = mode;
    return VR_OK;
}

int vr_volume_layout(vr_ctx* c, int slot, int* flags)
{
    if (!c || !flags) return VR_ERR_INVALID_ARG;
    if (slot < 0 || slot >= VR_MAX_VOLUMES) return fail(c, VR_ERR_INVALID_ARG, "vr_volume_layout: bad slot");
    if (!c->vols[slot].vol.data) return fail(c, VR_ERR_NOT_READY, "vr_volume_layout: volume slot is empty");
    *flags = (c->vols[slot].dens ? 1 : 0) | (c->vols[slot].grad_derived ? 2 : 0) | ((c->vols[slot].bricked && c->layout_mode == 0) ? 8 : 0);
    return VR_OK;
}

}  // extern "C"
