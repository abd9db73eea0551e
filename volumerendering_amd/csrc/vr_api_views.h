// vr_api_views.h -- what is made of or beside the march launches: present / unpack, downloads, the shadows' light volumes, surface
// depth and picking, slice views, histograms.  Part of vr_api.hip's translation unit.
#pragma once

namespace {

// Shadows (vr_set_shadows): the key of the light volume a LIGHT frame with uniforms u reads, and the light volume's grid (texels per axis).
ShadowKey shadow_key(const vr_ctx* c, const vr_uniforms& u)
{
    ShadowKey k;
    k.epoch = c->brick_epoch;
    k.opacity = c->opacity_edits;
    // (the clip bounds as fill_frame_params computes them)
    const float box[6] = {0.0f + u.clip_x[0], 0.0f + u.clip_y[0], 0.0f + u.clip_z[0], 1.0f - u.clip_x[1], 1.0f - u.clip_y[1], 1.0f - u.clip_z[1]};
    std::memcpy(k.light, u.light_pos, sizeof k.light);
    std::memcpy(k.box, box, sizeof k.box);
    std::memcpy(&k.sigma, &c->shadows.sigma, sizeof k.sigma);
    k.div = c->shadows.div;
    k.arith = c->arith;
    return k;
}

size_t shadow_grid(const vr_ctx* c, int g[3])
{
    const int n[3] = {c->vols[0].vol.nx, c->vols[0].vol.ny, c->vols[0].vol.nz};
    for (int a = 0; a < 3; ++a) g[a] = (n[a] + c->shadows.div - 1) / c->shadows.div;
    return (size_t)g[0] * g[1] * g[2];
}

// The light volume of a shadowed LIGHT launch on `s` whose parameters are P (volume 0, TF slot 0, the clip box and the light of its first
// frame; with `skip` LIGHT's distance field in P.brick_dist): the ring's entry of that key, built on `s` into the least recently used
// entry if there is none -- behind every launch that still reads that entry and behind its own last build -- or waited for once on a
// stream other than its build's.  Binds it as P.vol[1] and makes it the entry the launch reads (Shadows::cur).  An allocation failure
// returns before anything is enqueued.
int prepare_shadow(vr_ctx* c, hipStream_t s, MarchParams& P, const ShadowKey& key, bool skip, bool off32)
{
    Shadows& S = c->shadows;
    int g[3];
    const size_t texels = shadow_grid(c, g);
    bool build;
    const int e = S.entry(key, &build);
    ShadowVol& v = S.ring[e];
    if (build) {
        v.valid = false;
        const bool fresh = texels * sizeof(float) > v.buf.cap;
        // (a smaller buffer may still be read by launches in flight: it is retired, freed by the next draining call)
        if (const int rc = grow(c, v.buf, texels * sizeof(float), false)) return rc;
        if (!v.built.ev) VR_HIP(c, v.built.ev.create(hipEventDisableTiming));
        if (!fresh) {
            if (const int rc = reuse_wait(c, s, v.buf)) return rc;
            VR_HIP(c, v.built.rebuild_behind(s));
        }
    }
    DevVolume& lv = P.vol[1];
    lv = DevVolume{};
    lv.data = nullptr;
    lv.dens = (const float*)v.buf.p;
    lv.a_base = (const char*)v.buf.p;
    lv.a_shift = 2;
    lv.nx = g[0];
    lv.ny = g[1];
    lv.nz = g[2];
    lv.bricked = 0;
    lv.lut = 0;
    lv.data_bytes = (unsigned)(texels * sizeof(float));
    if (build) {
        if (c->arith == VR_ARITH_FUSED) vrf::launch_shadow_build(P, (float*)v.buf.p, S.sigma, skip, off32, s);
        else vr::launch_shadow_build(P, (float*)v.buf.p, S.sigma, skip, off32, s);
        VR_HIP(c, hipGetLastError());
        VR_HIP(c, hipEventRecord(v.built.ev, s));
        v.buf.written();
        v.key = key;
        v.valid = true;
        v.built.built(s);
    } else {
        VR_HIP(c, v.built.order_behind(s));
    }
    v.used = ++S.clock;
    S.cur = e;
    return VR_OK;
}

// the uniforms a depth pass needs, and the threshold of the context now
DepthParams depth_params(const vr_ctx* c)
{
    DepthParams D;
    std::memcpy(D.view, c->u.view, sizeof D.view);
    std::memcpy(D.proj, c->u.proj, sizeof D.proj);
    D.tau = c->surf_tau;
    return D;
}

// the descriptor's own fields (VR_ERR_INVALID_ARG), then what the context must hold (VR_ERR_NOT_READY)
int check_slice(vr_ctx* c, const vr_slice_desc* d, const void* out, const char* who)
{
    const std::string w(who);
    if (!d || !out) return fail(c, VR_ERR_INVALID_ARG, w + ": the descriptor or the output is NULL");
    if (d->volume_slot < 0 || d->volume_slot >= VR_MAX_VOLUMES) return fail(c, VR_ERR_INVALID_ARG, w + ": bad volume slot");
    if (d->tf_slot < 0 || d->tf_slot >= VR_MAX_TFS) return fail(c, VR_ERR_INVALID_ARG, w + ": bad TF slot");
    if (d->width < 1 || d->width > 16384 || d->height < 1 || d->height > 16384)
        return fail(c, VR_ERR_INVALID_ARG, w + ": the output must be 1 .. 16384 pixels each way");
    if (d->slab_steps < 1 || d->slab_steps > 65536) return fail(c, VR_ERR_INVALID_ARG, w + ": slab_steps must be 1 .. 65536");
    if (d->reduce != VR_SLICE_MAX && d->reduce != VR_SLICE_MIN && d->reduce != VR_SLICE_AVERAGE)
        return fail(c, VR_ERR_INVALID_ARG, w + ": unknown reduction");
    if (d->filter != VR_SLICE_LINEAR && d->filter != VR_SLICE_NEAREST) return fail(c, VR_ERR_INVALID_ARG, w + ": unknown filter");
    if (d->format != VR_SLICE_RGBA32F && d->format != VR_SLICE_BGRA8) return fail(c, VR_ERR_INVALID_ARG, w + ": unknown format");
    if (!c->vols[d->volume_slot].vol.data) return fail(c, VR_ERR_NOT_READY, w + ": volume slot " + std::to_string(d->volume_slot) + " is empty");
    if (!c->tf[d->tf_slot].dev.opacity || !c->tf[d->tf_slot].dev.color)
        return fail(c, VR_ERR_NOT_READY, w + ": TF slot " + std::to_string(d->tf_slot) + " is empty");
    return VR_OK;
}

// One slice launch on `s` (the descriptor has been checked).  It takes the next record slot -- so it is one of the kInFlight launches
// in flight, and its slot's event is what reuse_wait orders a later table edit behind -- but writes records of its own
// (RecordSlot::slice_counts) and touches none of the march launches' bookkeeping: counters, last flavour, timings, kernel choice, launch order.
int enqueue_slice(vr_ctx* c, const vr_slice_desc& d, void* d_out, hipStream_t s)
{
    VR_HIP(c, hipSetDevice(c->device));
    (void)hipGetLastError();
    VR_HIP(c, c->edits.order.order_behind(s));  // the launch comes after every asynchronous edit made so far
    const int vs = d.volume_slot;
    SliceParams S;
    std::memset(&S, 0, sizeof S);
    S.vol = linear_volume(c, vs);
    if (c->layout_mode == 0) use_bricked_copy(c, vs, S.vol);
    bool off32 = c->vols[vs].bytes() <= 0xFFFFFFFFull;
    if (S.vol.bricked && bricked_grid(S.vol).slots * 16 > 0xFFFFFFFFull) off32 = false;
    S.tf = c->tf[d.tf_slot].dev;
    for (int a = 0; a < 3; ++a) {
        S.origin[a] = d.origin[a];
        S.du[a] = d.du[a];
        S.dv[a] = d.dv[a];
        S.dn[a] = d.dn[a];
    }
    S.width = (int)d.width;
    S.height = (int)d.height;
    S.tiles_x = (int)((d.width + 7u) / 8u);
    S.slab_steps = d.slab_steps;
    S.format = d.format;
    S.out = d_out;
    const unsigned tiles = (unsigned)S.tiles_x * ((d.height + 7u) / 8u);
    // exact skipping by the slot's range records, unless flavour 1 asks for the plain form (the kernels index bricks with 24-bit
    // multiplies and 32-bit byte offsets, as every skipping kernel)
    const DevVolume& v = c->vols[vs].vol;
    S.bnx = skip_bricks(v.nx);
    S.bny = skip_bricks(v.ny);
    S.bnz = skip_bricks(v.nz);
    S.bsx = (float)v.nx * kBrickInv;
    S.bsy = (float)v.ny * kBrickInv;
    S.bsz = (float)v.nz * kBrickInv;
    const bool skip = !plain_form(c) && bricks_indexable(S.bnx, S.bny, S.bnz);
    if (skip) {
        S.vrange = prepare_range(c, s, vs, S.bnx, S.bny, S.bnz, &S.bricks);
        if (!S.vrange) return VR_ERR_HIP;
    }
    // the record slot: the launch that used it last has finished (host wait: the bound on launches in flight); the sort that read that
    // launch's records is waited for on the stream, so that whoever takes the slot next may write them behind this launch's event
    int cb;
    if (const int rc = claim_slot(c, s, &cb)) return rc;
    // (the slot's last slice has finished: the slot's event, in claim_slot)
    if ((size_t)tiles * 3 > c->slot[cb].slice_counts.cap) VR_HIP(c, c->slot[cb].slice_counts.reserve((size_t)tiles * 3));
    S.counts = c->slot[cb].slice_counts;
    if (c->arith == VR_ARITH_FUSED) vrf::launch_slice(S, d.reduce, d.filter == VR_SLICE_NEAREST, off32, skip, tiles, s);
    else vr::launch_slice(S, d.reduce, d.filter == VR_SLICE_NEAREST, off32, skip, tiles, s);
    VR_HIP(c, hipGetLastError());
    c->tf[d.tf_slot].mark_reads(c->order_seq);
    if (const int rc = finish_slot(c, s, cb)) return rc;
    c->slice_buf = cb;
    c->slice_tiles = tiles;
    return VR_OK;
}

// the descriptor's own fields (VR_ERR_INVALID_ARG), then what the context must hold (VR_ERR_NOT_READY, mismatched mask)
int check_hist(vr_ctx* c, const vr_hist_desc* d, const void* counts, const void* rows, const char* who)
{
    const std::string w(who);
    if (!d || !counts || !rows) return fail(c, VR_ERR_INVALID_ARG, w + ": the descriptor or an output is NULL");
    if (const int rc = check_slot(c, w, "volume", d->volume_slot)) return rc;
    if (d->mask_slot != -1)
        if (const int rc = check_slot(c, w, "mask", d->mask_slot)) return rc;
    if (const int rc = check_component(c, w, "channel", d->channel)) return rc;
    if (d->bins < 1 || d->bins > VR_HIST_MAX_BINS) return fail(c, VR_ERR_INVALID_ARG, w + ": bins must be 1 .. 65536");
    if (d->out_of_range != VR_HIST_CLAMP && d->out_of_range != VR_HIST_DROP) return fail(c, VR_ERR_INVALID_ARG, w + ": unknown out_of_range policy");
    if (d->rows == 0 || (d->rows >> VR_HIST_ROWS) != 0) return fail(c, VR_ERR_INVALID_ARG, w + ": rows must have a bit of 0 .. 4 set and none above");
    if ((d->rows & ~1u) != 0 && d->mask_slot < 0) return fail(c, VR_ERR_INVALID_ARG, w + ": contour rows need a mask slot");
    if (const int rc = check_filled(c, w, "volume", d->volume_slot)) return rc;
    const DevVolume& v = c->vols[d->volume_slot].vol;
    if (const int rc = check_box(c, w, d->lo, d->hi, v)) return rc;
    if (d->mask_slot >= 0) {
        if (const int rc = check_filled(c, w, "mask", d->mask_slot)) return rc;
        return check_same_dims(c, w, "mask", c->vols[d->mask_slot].vol, "volume", v);
    }
    return VR_OK;
}

// One histogram launch on `s` (the descriptor has been checked).  Like a slice it takes the next record slot -- it is one of the
// kInFlight launches in flight -- and touches none of the other launches' bookkeeping.
int enqueue_hist(vr_ctx* c, const vr_hist_desc& d, void* d_counts, void* d_rows, hipStream_t s)
{
    VR_HIP(c, hipSetDevice(c->device));
    (void)hipGetLastError();
    const int vs = d.volume_slot;
    const DevVolume v = linear_volume(c, vs);
    HistParams H;
    std::memset(&H, 0, sizeof H);
    const bool plane = d.channel == 3 && d.mask_slot < 0 && v.dens;
    H.val = plane ? v.dens : reinterpret_cast<const float*>(v.data) + d.channel;
    H.val_stride = plane ? 1 : 4;
    H.mask = d.mask_slot >= 0 ? c->vols[d.mask_slot].vol.data : nullptr;
    H.nx = v.nx;
    H.ny = v.ny;
    H.nz = v.nz;
    unsigned long long box;
    H.box = box_units(d.lo, d.hi, &box);
    if ((unsigned long long)H.box.un[0] * H.box.un[1] * H.box.un[2] > 0xFFFFFFFFull) return fail(c, VR_ERR_UNSUPPORTED, "vr_histogram: the box has 2^32 brick units or more");
    H.rows = d.rows;
    H.bins = d.bins;
    H.scale = d.scale;
    H.drop = d.out_of_range == VR_HIST_DROP;
    unsigned n_rows = 0;
    for (int r = 0; r < VR_HIST_ROWS; ++r) n_rows += (d.rows >> r) & 1u;
    const unsigned blocks = tool_blocks(H.box.units);
    // the private LDS copy: within the budget, and a workgroup's share of the voxels (its four wavefronts' units) below 2^32 so that
    // no u32 count can wrap; otherwise the kernel adds into the u64 outputs directly
    const unsigned long long per_block = (H.box.units + blocks * 4ull - 1) / (blocks * 4ull) * 4ull * 64ull;
    H.lds = (size_t)n_rows * d.bins * sizeof(unsigned) <= kHistLdsBytes && per_block < (1ull << 32);
    const bool plain = plain_form(c);
    // exact settling by the slot's range records (of .a: channel 3), for the unmasked launch
    if (!plain && d.channel == 3 && d.mask_slot < 0 && H.box.units != 0) {
        H.bnx = skip_bricks(v.nx);
        H.bny = skip_bricks(v.ny);
        if (!prepare_range(c, s, vs, H.bnx, H.bny, skip_bricks(v.nz), &H.bricks)) return VR_ERR_HIP;
    }
    int cb;
    if (const int rc = claim_slot(c, s, &cb)) return rc;
    if (!c->slot[cb].hist_stats) VR_HIP(c, c->slot[cb].hist_stats.reserve(3));
    VR_HIP(c, hipMemsetAsync(c->slot[cb].hist_stats, 0, 3 * sizeof(unsigned long long), s));
    VR_HIP(c, hipMemsetAsync(d_counts, 0, (size_t)VR_HIST_ROWS * d.bins * sizeof(unsigned long long), s));
    VR_HIP(c, hipMemsetAsync(d_rows, 0, VR_HIST_ROWS * sizeof(vr_hist_row), s));
    H.counts = static_cast<unsigned long long*>(d_counts);
    H.row_sums = static_cast<unsigned long long*>(d_rows);
    H.stats = c->slot[cb].hist_stats;
    const size_t lds_bytes = H.lds ? (size_t)n_rows * d.bins * sizeof(unsigned) : 0;
    if (plain) hipLaunchKernelGGL(hist_kernel<true>, dim3(blocks), dim3(256), lds_bytes, s, H);
    else hipLaunchKernelGGL(hist_kernel<false>, dim3(blocks), dim3(256), lds_bytes, s, H);
    VR_HIP(c, hipGetLastError());
    if (const int rc = finish_slot(c, s, cb)) return rc;
    c->hist_buf = cb;
    return VR_OK;
}

}  // namespace

extern "C" {

int vr_unpack_tiles_strided_async(vr_ctx* c, const void* d_gathered, int world, int rank_stride_tiles, void* d_frame, void* stream)
{
    if (!c) return VR_ERR_INVALID_ARG;
    if (!d_gathered || world < 1) return fail(c, VR_ERR_INVALID_ARG, "vr_unpack_tiles_async: bad arguments");
    const int tpr = tile_count(c, 0, world);
    if (rank_stride_tiles < tpr) return fail(c, VR_ERR_INVALID_ARG, "vr_unpack_tiles_strided_async: stride smaller than a segment");
    VR_HIP(c, hipSetDevice(c->device));
    (void)hipGetLastError();
    hipStream_t s = stream ? (hipStream_t)stream : c->stream;
    float4* frame = d_frame ? (float4*)d_frame : c->d_frame;
    dim3 block(64, 4), grid((c->W + 63) / 64, (c->H + 3) / 4);
    hipLaunchKernelGGL(unpack_tiles_kernel, grid, block, 0, s, (const float4*)d_gathered, frame, (int)c->W, (int)c->H,
                       tiles_x_of(c), world, rank_stride_tiles);
    VR_HIP(c, hipGetLastError());
    return VR_OK;
}

int vr_unpack_tiles_async(vr_ctx* c, const void* d_gathered, int world, void* d_frame, void* stream)
{
    if (!c) return VR_ERR_INVALID_ARG;
    if (world < 1) return fail(c, VR_ERR_INVALID_ARG, "vr_unpack_tiles_async: bad arguments");
    return vr_unpack_tiles_strided_async(c, d_gathered, world, tile_count(c, 0, world), d_frame, stream);
}

int vr_present_async(vr_ctx* c, const void* d_frame, void* d_bgra8, void* stream)
{
    if (!c) return VR_ERR_INVALID_ARG;
    if (!d_bgra8) return fail(c, VR_ERR_INVALID_ARG, "vr_present_async: destination is NULL");
    VR_HIP(c, hipSetDevice(c->device));
    (void)hipGetLastError();
    hipStream_t s = stream ? (hipStream_t)stream : c->stream;
    const size_t n = (size_t)c->W * c->H;
    hipLaunchKernelGGL(present_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s,
                       d_frame ? (const float4*)d_frame : c->d_frame, (uint32_t*)d_bgra8, (int)n);
    VR_HIP(c, hipGetLastError());
    return VR_OK;
}

int vr_present_tiles_async(vr_ctx* c, const void* d_gathered, int world, int rank_stride_tiles, void* d_bgra8, void* stream)
{
    if (!c) return VR_ERR_INVALID_ARG;
    if (!d_gathered || !d_bgra8 || world < 1) return fail(c, VR_ERR_INVALID_ARG, "vr_present_tiles_async: bad arguments");
    const int tpr = tile_count(c, 0, world);
    if (rank_stride_tiles <= 0) rank_stride_tiles = tpr;
    if (rank_stride_tiles < tpr) return fail(c, VR_ERR_INVALID_ARG, "vr_present_tiles_async: stride smaller than a segment");
    VR_HIP(c, hipSetDevice(c->device));
    (void)hipGetLastError();
    hipStream_t s = stream ? (hipStream_t)stream : c->stream;
    dim3 block(64, 4), grid((c->W + 63) / 64, (c->H + 3) / 4);
    hipLaunchKernelGGL(present_tiles_kernel, grid, block, 0, s, (const float4*)d_gathered, (uint32_t*)d_bgra8, (int)c->W, (int)c->H,
                       tiles_x_of(c), world, rank_stride_tiles);
    VR_HIP(c, hipGetLastError());
    return VR_OK;
}

int vr_present_packed_async(vr_ctx* c, const void* d_tiles_rgba, int n_tiles, void* d_tiles_bgra8, void* stream)
{
    if (!c) return VR_ERR_INVALID_ARG;
    if (!d_tiles_rgba || !d_tiles_bgra8 || n_tiles < 0) return fail(c, VR_ERR_INVALID_ARG, "vr_present_packed_async: bad arguments");
    if (n_tiles == 0) return VR_OK;
    VR_HIP(c, hipSetDevice(c->device));
    (void)hipGetLastError();
    hipStream_t s = stream ? (hipStream_t)stream : c->stream;
    const size_t n = (size_t)n_tiles * kTile * kTile;
    if (n > 0x7fffffffull) return fail(c, VR_ERR_INVALID_ARG, "vr_present_packed_async: too many tiles");
    hipLaunchKernelGGL(present_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, (const float4*)d_tiles_rgba, (uint32_t*)d_tiles_bgra8, (int)n);
    VR_HIP(c, hipGetLastError());
    return VR_OK;
}

int vr_unpack_tiles_bgra8_async(vr_ctx* c, const void* d_gathered_bgra8, int world, int rank_stride_tiles, void* d_bgra8, void* stream)
{
    if (!c) return VR_ERR_INVALID_ARG;
    if (!d_gathered_bgra8 || !d_bgra8 || world < 1) return fail(c, VR_ERR_INVALID_ARG, "vr_unpack_tiles_bgra8_async: bad arguments");
    const int tpr = tile_count(c, 0, world);
    if (rank_stride_tiles <= 0) rank_stride_tiles = tpr;
    if (rank_stride_tiles < tpr) return fail(c, VR_ERR_INVALID_ARG, "vr_unpack_tiles_bgra8_async: stride smaller than a segment");
    VR_HIP(c, hipSetDevice(c->device));
    (void)hipGetLastError();
    hipStream_t s = stream ? (hipStream_t)stream : c->stream;
    dim3 block(64, 4), grid((c->W + 63) / 64, (c->H + 3) / 4);
    hipLaunchKernelGGL(unpack_tiles_u32_kernel, grid, block, 0, s, (const uint32_t*)d_gathered_bgra8, (uint32_t*)d_bgra8, (int)c->W, (int)c->H,
                       tiles_x_of(c), world, rank_stride_tiles);
    VR_HIP(c, hipGetLastError());
    return VR_OK;
}

int vr_download(vr_ctx* c, float* frag_rgba, uint8_t* present_bgra8, uint64_t* composited_samples)
{
    if (!c) return VR_ERR_INVALID_ARG;
    VR_HIP(c, hipSetDevice(c->device));
    VR_HIP(c, hipStreamSynchronize(c->stream));
    size_t n = (size_t)c->W * c->H;
    if (frag_rgba) VR_HIP(c, hipMemcpy(frag_rgba, c->d_frame, n * sizeof(float4), hipMemcpyDeviceToHost));
    if (present_bgra8) {
        (void)hipGetLastError();
        hipLaunchKernelGGL(present_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c->stream, c->d_frame,
                           c->d_present, (int)n);
        VR_HIP(c, hipGetLastError());
        VR_HIP(c, hipStreamSynchronize(c->stream));
        VR_HIP(c, hipMemcpy(present_bgra8, c->d_present, n * sizeof(uint32_t), hipMemcpyDeviceToHost));
    }
    if (composited_samples) {
        int rc = fetch_counters(c);
        if (rc != VR_OK) return rc;
        *composited_samples = c->h_counters[0];
    }
    return VR_OK;
}

int vr_download_tiles(vr_ctx* c, float* tiles_rgba, uint64_t* composited_samples)
{
    if (!c) return VR_ERR_INVALID_ARG;
    VR_HIP(c, hipSetDevice(c->device));
    VR_HIP(c, hipStreamSynchronize(c->stream));
    if (tiles_rgba && c->last.tiles > 0)
        VR_HIP(c, hipMemcpy(tiles_rgba, c->d_tiles, (size_t)c->last.tiles * kTile * kTile * sizeof(float4),
                            hipMemcpyDeviceToHost));
    if (composited_samples) {
        int rc = fetch_counters(c);
        if (rc != VR_OK) return rc;
        *composited_samples = c->h_counters[0];
    }
    return VR_OK;
}

int vr_shadow_volume(vr_ctx* c, float* out, size_t capacity, int dims[3])
{
    if (!c) return VR_ERR_INVALID_ARG;
    if (capacity > 0 && !out) return fail(c, VR_ERR_INVALID_ARG, "vr_shadow_volume: out is NULL");
    if (c->shadows.div == 0) return fail(c, VR_ERR_NOT_READY, "vr_shadow_volume: shadows are off");
    if (!c->vols[0].vol.data) return fail(c, VR_ERR_NOT_READY, "vr_shadow_volume: volume slot 0 is empty");
    if (!c->tf[0].dev.opacity || !c->tf[0].dev.color) return fail(c, VR_ERR_NOT_READY, "vr_shadow_volume: TF slot 0 is empty");
    if (!c->have_uniforms) return fail(c, VR_ERR_NOT_READY, "vr_shadow_volume: vr_set_uniforms has not been called");
    int g[3];
    const size_t n = shadow_grid(c, g);
    if (n * sizeof(float) >= (1ull << 32)) return fail(c, VR_ERR_UNSUPPORTED, "vr_shadow_volume: the light volume would take 4 GiB or more");
    if (const int rc = drain(c)) return rc;
    (void)hipGetLastError();
    // the parameters a LIGHT launch of the context's uniforms would have (the flavour asked for decides the build's form; both give the
    // same texels)
    MarchParams P;
    fill_launch_params(c, P, c->u, 0, 1, false);
    const int requested = c->flavour == 0 ? c->default_flavour : c->flavour;
    const Eligibility E = eligibility(choice_facts(c, render_request(c, VR_VARIANT_LIGHT, 0, 1, false, nullptr, nullptr), requested), requested);
    if (E.can_skip)
        if (const int rc = prepare_skip(c, VR_VARIANT_LIGHT, c->stream, P)) return rc;
    if (c->layout_mode == 0) use_bricked_copies(c, P);
    const bool off32 = c->vols[0].bytes() <= 0xFFFFFFFFull && !(P.vol[0].bricked && bricked_grid(P.vol[0]).slots * 16 > 0xFFFFFFFFull);
    const int rc = prepare_shadow(c, c->stream, P, shadow_key(c, c->u), P.brick_dist != nullptr && requested != 1, off32);
    c->shadows.cur = -1;  // (no launch reads it)
    if (rc) return rc;
    VR_HIP(c, hipStreamSynchronize(c->stream));
    if (capacity > 0) VR_HIP(c, hipMemcpy(out, P.vol[1].dens, (capacity < n ? capacity : n) * sizeof(float), hipMemcpyDeviceToHost));
    if (dims)
        for (int a = 0; a < 3; ++a) dims[a] = g[a];
    return (int)n;
}

int vr_surface_depth_async(vr_ctx* c, const void* d_surface, void* d_depth, void* stream)
{
    if (!c) return VR_ERR_INVALID_ARG;
    if (!d_surface || !d_depth) return fail(c, VR_ERR_INVALID_ARG, "vr_surface_depth_async: a buffer is NULL");
    if (!c->have_uniforms) return fail(c, VR_ERR_NOT_READY, "vr_surface_depth_async: vr_set_uniforms has not been called");
    VR_HIP(c, hipSetDevice(c->device));
    (void)hipGetLastError();
    hipStream_t s = stream ? (hipStream_t)stream : c->stream;
    const size_t n = (size_t)c->W * c->H;
    hipLaunchKernelGGL(surface_depth_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, (const float4*)d_surface, (float*)d_depth,
                       (int)n, depth_params(c));
    VR_HIP(c, hipGetLastError());
    return VR_OK;
}

int vr_pick(vr_ctx* c, int variant, uint32_t x, uint32_t y, vr_pick_result* out)
{
    if (!c) return VR_ERR_INVALID_ARG;
    if (!out) return fail(c, VR_ERR_INVALID_ARG, "vr_pick: out is NULL");
    if (x >= c->W || y >= c->H) return fail(c, VR_ERR_INVALID_ARG, "vr_pick: the pixel lies outside the viewport");
    VR_HIP(c, hipSetDevice(c->device));
    // what the render before the pick left behind stays what the context reports: its counters are summed now ...
    if (const int rc = fetch_counters(c)) return rc;
    if (!c->d_pick) VR_HIP(c, c->d_pick.reserve((size_t)c->W * c->H));
    if (!c->d_pick_depth) VR_HIP(c, c->d_pick_depth.reserve(1));
    // ... and the launch's bookkeeping is put back behind the pick's own launch (which takes the next record slot, not the last one's)
    // (the sums of its counters, in pinned memory, beside it; cnt_pending is false: they have just been fetched)
    const struct {
        LastLaunch last;
        unsigned long long counters[3];
    } before = {c->last, {c->h_counters[0], c->h_counters[1], c->h_counters[2]}};
    RenderRequest R = render_request(c, variant, 0, 1, false, c->d_pick, nullptr);
    R.pick_px[0] = (int)x;
    R.pick_px[1] = (int)y;
    const int rc = enqueue_render(c, R);
    const hipError_t sync = hipDeviceSynchronize();
    if (sync == hipSuccess) drained(c);
    c->last = before.last;
    std::memcpy(c->h_counters, before.counters, sizeof before.counters);
    if (rc != VR_OK) return rc;
    VR_HIP(c, sync);

    const size_t idx = (size_t)y * c->W + x;
    float4 px;
    VR_HIP(c, hipMemcpy(&px, c->d_pick + idx, sizeof px, hipMemcpyDeviceToHost));
    std::memset(out, 0, sizeof *out);
    out->alpha = px.w;
    out->depth = 1.0f;
    out->hit = px.w > c->surf_tau ? 1 : 0;  // (an ISO frame's .w is 1 or 0)
    if (!out->hit) return VR_OK;
    (void)hipGetLastError();
    hipLaunchKernelGGL(surface_depth_kernel, dim3(1), dim3(256), 0, c->stream, (const float4*)(c->d_pick + idx), c->d_pick_depth, 1,
                       depth_params(c));
    VR_HIP(c, hipGetLastError());
    VR_HIP(c, hipStreamSynchronize(c->stream));
    VR_HIP(c, hipMemcpy(&out->depth, c->d_pick_depth, sizeof(float), hipMemcpyDeviceToHost));
    const float q[3] = {px.x, px.y, px.z};
    out->world[0] = q[0] - 0.5f;
    out->world[1] = q[1] - 0.5f;
    out->world[2] = (0.5f - q[2]) * 0.5f;
    const int n0[3] = {c->vols[0].vol.nx, c->vols[0].vol.ny, c->vols[0].vol.nz};
    for (int a = 0; a < 3; ++a) {
        out->uvw[a] = q[a];
        const float f = std::floor(q[a] * (float)n0[a]);
        out->voxel[a] = f >= (float)(n0[a] - 1) ? n0[a] - 1 : (f > 0.0f ? (int)f : 0);  // (NaN -> 0)
    }
    const size_t v = ((size_t)out->voxel[2] * (size_t)n0[1] + (size_t)out->voxel[1]) * (size_t)n0[0] + (size_t)out->voxel[0];
    for (int i = 0; i < VR_MAX_VOLUMES; ++i)
        if (c->vols[i].vol.data && c->vols[i].vol.nx == n0[0] && c->vols[i].vol.ny == n0[1] && c->vols[i].vol.nz == n0[2])
            VR_HIP(c, hipMemcpy(out->value[i], c->vols[i].vol.data + v, sizeof(float4), hipMemcpyDeviceToHost));
    return VR_OK;
}

int vr_slice_async(vr_ctx* c, const vr_slice_desc* desc, void* d_out, void* stream)
{
    if (!c) return VR_ERR_INVALID_ARG;
    if (const int rc = check_slice(c, desc, d_out, "vr_slice_async")) return rc;
    return enqueue_slice(c, *desc, d_out, stream ? (hipStream_t)stream : c->stream);
}

int vr_slice_render(vr_ctx* c, const vr_slice_desc* desc, void* out_host)
{
    if (!c) return VR_ERR_INVALID_ARG;
    if (const int rc = check_slice(c, desc, out_host, "vr_slice_render")) return rc;
    VR_HIP(c, hipSetDevice(c->device));
    const size_t bytes = (size_t)desc->width * desc->height * (desc->format == VR_SLICE_BGRA8 ? 4u : 16u);
    // (the buffer's earlier uses were synchronous on this stream; a smaller one is freed by the next draining call)
    if (const int rc = grow(c, c->d_slice_out, bytes, false)) return rc;
    if (const int rc = enqueue_slice(c, *desc, c->d_slice_out, c->stream)) return rc;
    VR_HIP(c, hipMemcpyAsync(out_host, c->d_slice_out, bytes, hipMemcpyDeviceToHost, c->stream));
    VR_HIP(c, hipStreamSynchronize(c->stream));
    return VR_OK;
}

int vr_slice_orthogonal(const vr_ctx* c, int slot, int axis, int index, int thickness, vr_slice_desc* out)
{
    if (!c || !out) return VR_ERR_INVALID_ARG;
    if (slot < 0 || slot >= VR_MAX_VOLUMES || axis < 0 || axis > 2 || thickness < 1 || thickness > 65536) return VR_ERR_INVALID_ARG;
    if (!c->vols[slot].vol.data) return VR_ERR_NOT_READY;
    const int n[3] = {c->vols[slot].vol.nx, c->vols[slot].vol.ny, c->vols[slot].vol.nz};
    if (index < 0 || index >= n[axis]) return VR_ERR_INVALID_ARG;
    const int ua = axis == 0 ? 1 : 0, va = axis == 2 ? 1 : 2;  // the output's x / y axes: (y, z), (x, z), (x, y)
    std::memset(out, 0, sizeof *out);
    out->volume_slot = slot;
    out->tf_slot = 0;
    out->width = (uint32_t)n[ua];
    out->height = (uint32_t)n[va];
    out->origin[ua] = 0.5f / (float)n[ua];
    out->origin[va] = 0.5f / (float)n[va];
    out->origin[axis] = ((float)(index - (thickness - 1) / 2) + 0.5f) / (float)n[axis];
    out->du[ua] = 1.0f / (float)n[ua];
    out->dv[va] = 1.0f / (float)n[va];
    out->dn[axis] = 1.0f / (float)n[axis];
    out->slab_steps = thickness;
    out->reduce = VR_SLICE_MAX;
    out->filter = VR_SLICE_LINEAR;
    out->format = VR_SLICE_RGBA32F;
    return VR_OK;
}

int vr_slice_counters(vr_ctx* c, uint64_t out[3])
{
    if (!c) return VR_ERR_INVALID_ARG;
    if (!out) return fail(c, VR_ERR_INVALID_ARG, "vr_slice_counters: out is NULL");
    out[0] = out[1] = out[2] = 0;
    if (c->slice_buf < 0) return VR_OK;
    VR_HIP(c, hipSetDevice(c->device));
    (void)hipGetLastError();
    // the event behind the slice (or behind a later launch in its record slot), then the context's own stream: the caller's may be gone
    VR_HIP(c, hipEventSynchronize(c->slot[c->slice_buf].done));
    // (d_counters: every use of it is synchronous on the context's stream, as this one)
    hipLaunchKernelGGL(slice_sum_kernel, dim3(1), dim3(1024), 0, c->stream, (const unsigned long long*)c->slot[c->slice_buf].slice_counts,
                       c->slice_tiles, c->d_counters);
    VR_HIP(c, hipGetLastError());
    unsigned long long h[3] = {0, 0, 0};
    VR_HIP(c, hipMemcpyAsync(h, c->d_counters, sizeof h, hipMemcpyDeviceToHost, c->stream));
    VR_HIP(c, hipStreamSynchronize(c->stream));
    for (int i = 0; i < 3; ++i) out[i] = h[i];
    return VR_OK;
}

int vr_hist_whole(const vr_ctx* c, int slot, uint32_t bins, float scale, vr_hist_desc* out)
{
    if (!c || !out) return VR_ERR_INVALID_ARG;
    if (!is_slot(slot) || bins < 1 || bins > VR_HIST_MAX_BINS) return VR_ERR_INVALID_ARG;
    if (!c->vols[slot].vol.data) return VR_ERR_NOT_READY;
    std::memset(out, 0, sizeof *out);
    out->volume_slot = slot;
    out->channel = 3;
    out->mask_slot = -1;
    out->rows = 1;
    out->bins = bins;
    out->scale = scale;
    out->out_of_range = VR_HIST_CLAMP;
    whole_box(c->vols[slot].vol, out->hi);
    return VR_OK;
}

int vr_histogram_async(vr_ctx* c, const vr_hist_desc* desc, void* d_counts, void* d_rows, void* stream)
{
    if (!c) return VR_ERR_INVALID_ARG;
    if (const int rc = check_hist(c, desc, d_counts, d_rows, "vr_histogram_async")) return rc;
    return enqueue_hist(c, *desc, d_counts, d_rows, stream ? (hipStream_t)stream : c->stream);
}

int vr_histogram(vr_ctx* c, const vr_hist_desc* desc, uint64_t* counts, vr_hist_row* rows)
{
    if (!c) return VR_ERR_INVALID_ARG;
    if (const int rc = check_hist(c, desc, counts, rows, "vr_histogram")) return rc;
    VR_HIP(c, hipSetDevice(c->device));
    const size_t cbytes = (size_t)VR_HIST_ROWS * desc->bins * sizeof(uint64_t), rbytes = VR_HIST_ROWS * sizeof(vr_hist_row);
    // (the buffer's earlier uses were synchronous on this stream; a smaller one is freed by the next draining call)
    if (const int rc = grow(c, c->d_hist_out, cbytes + rbytes, false)) return rc;
    char* d = static_cast<char*>(c->d_hist_out.p);
    if (const int rc = enqueue_hist(c, *desc, d, d + cbytes, c->stream)) return rc;
    VR_HIP(c, hipMemcpyAsync(counts, d, cbytes, hipMemcpyDeviceToHost, c->stream));
    VR_HIP(c, hipMemcpyAsync(rows, d + cbytes, rbytes, hipMemcpyDeviceToHost, c->stream));
    VR_HIP(c, hipStreamSynchronize(c->stream));
    return VR_OK;
}

int vr_hist_counters(vr_ctx* c, uint64_t out[3])
{
    if (!c) return VR_ERR_INVALID_ARG;
    if (!out) return fail(c, VR_ERR_INVALID_ARG, "vr_hist_counters: out is NULL");
    out[0] = out[1] = out[2] = 0;
    if (c->hist_buf < 0) return VR_OK;
    VR_HIP(c, hipSetDevice(c->device));
    (void)hipGetLastError();
    // the event behind the histogram (or behind a later launch in its record slot), then the context's own stream
    VR_HIP(c, hipEventSynchronize(c->slot[c->hist_buf].done));
    unsigned long long h[3] = {0, 0, 0};
    VR_HIP(c, hipMemcpyAsync(h, c->slot[c->hist_buf].hist_stats, sizeof h, hipMemcpyDeviceToHost, c->stream));
    VR_HIP(c, hipStreamSynchronize(c->stream));
    for (int i = 0; i < 3; ++i) out[i] = h[i];
    return VR_OK;
}

}  // extern "C"
