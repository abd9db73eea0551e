// vr_api_render.h -- a march launch: its arguments, the facts the kernel choice reads (choice_facts; the choice itself -- what may run,
// the prior, the candidates, what a flavour means, the launch shape -- is vr_choice.h, plain C++), the record slots (claim_slot /
// finish_slot), the launch itself, the launch-order sort behind it, counters and timing.  Part of vr_api.hip's translation unit.
#pragma once

namespace {

// (defined in vr_api_views.h)
ShadowKey shadow_key(const vr_ctx* c, const vr_uniforms& u);
size_t shadow_grid(const vr_ctx* c, int g[3]);
int prepare_shadow(vr_ctx* c, hipStream_t s, MarchParams& P, const ShadowKey& key, bool skip, bool off32);

int tiles_x_of(const vr_ctx* c) { return tiles_across(c->W); }
int tiles_y_of(const vr_ctx* c) { return tiles_across(c->H); }
int tile_count(const vr_ctx* c, int rank, int world) { return vr::tile_count(c->W, c->H, rank, world); }

bool is_identity(const float* m)
{
    for (int i = 0; i < 16; ++i)
        if (m[i] != ((i % 5 == 0) ? 1.0f : 0.0f)) return false;
    return true;
}

// Inverse of a column-major 4x4 in double precision (cofactors); false if singular / not finite.
bool invert4(const float* m, double* o)
{
    double a[16], inv[16];
    for (int i = 0; i < 16; ++i) a[i] = m[i];
    inv[0] = a[5] * a[10] * a[15] - a[5] * a[11] * a[14] - a[9] * a[6] * a[15] + a[9] * a[7] * a[14] + a[13] * a[6] * a[11] - a[13] * a[7] * a[10];
    inv[4] = -a[4] * a[10] * a[15] + a[4] * a[11] * a[14] + a[8] * a[6] * a[15] - a[8] * a[7] * a[14] - a[12] * a[6] * a[11] + a[12] * a[7] * a[10];
    inv[8] = a[4] * a[9] * a[15] - a[4] * a[11] * a[13] - a[8] * a[5] * a[15] + a[8] * a[7] * a[13] + a[12] * a[5] * a[11] - a[12] * a[7] * a[9];
    inv[12] = -a[4] * a[9] * a[14] + a[4] * a[10] * a[13] + a[8] * a[5] * a[14] - a[8] * a[6] * a[13] - a[12] * a[5] * a[10] + a[12] * a[6] * a[9];
    inv[1] = -a[1] * a[10] * a[15] + a[1] * a[11] * a[14] + a[9] * a[2] * a[15] - a[9] * a[3] * a[14] - a[13] * a[2] * a[11] + a[13] * a[3] * a[10];
    inv[5] = a[0] * a[10] * a[15] - a[0] * a[11] * a[14] - a[8] * a[2] * a[15] + a[8] * a[3] * a[14] + a[12] * a[2] * a[11] - a[12] * a[3] * a[10];
    inv[9] = -a[0] * a[9] * a[15] + a[0] * a[11] * a[13] + a[8] * a[1] * a[15] - a[8] * a[3] * a[13] - a[12] * a[1] * a[11] + a[12] * a[3] * a[9];
    inv[13] = a[0] * a[9] * a[14] - a[0] * a[10] * a[13] - a[8] * a[1] * a[14] + a[8] * a[2] * a[13] + a[12] * a[1] * a[10] - a[12] * a[2] * a[9];
    inv[2] = a[1] * a[6] * a[15] - a[1] * a[7] * a[14] - a[5] * a[2] * a[15] + a[5] * a[3] * a[14] + a[13] * a[2] * a[7] - a[13] * a[3] * a[6];
    inv[6] = -a[0] * a[6] * a[15] + a[0] * a[7] * a[14] + a[4] * a[2] * a[15] - a[4] * a[3] * a[14] - a[12] * a[2] * a[7] + a[12] * a[3] * a[6];
    inv[10] = a[0] * a[5] * a[15] - a[0] * a[7] * a[13] - a[4] * a[1] * a[15] + a[4] * a[3] * a[13] + a[12] * a[1] * a[7] - a[12] * a[3] * a[5];
    inv[14] = -a[0] * a[5] * a[14] + a[0] * a[6] * a[13] + a[4] * a[1] * a[14] - a[4] * a[2] * a[13] - a[12] * a[1] * a[6] + a[12] * a[2] * a[5];
    inv[3] = -a[1] * a[6] * a[11] + a[1] * a[7] * a[10] + a[5] * a[2] * a[11] - a[5] * a[3] * a[10] - a[9] * a[2] * a[7] + a[9] * a[3] * a[6];
    inv[7] = a[0] * a[6] * a[11] - a[0] * a[7] * a[10] - a[4] * a[2] * a[11] + a[4] * a[3] * a[10] + a[8] * a[2] * a[7] - a[8] * a[3] * a[6];
    inv[11] = -a[0] * a[5] * a[11] + a[0] * a[7] * a[9] + a[4] * a[1] * a[11] - a[4] * a[3] * a[9] - a[8] * a[1] * a[7] + a[8] * a[3] * a[5];
    inv[15] = a[0] * a[5] * a[10] - a[0] * a[6] * a[9] - a[4] * a[1] * a[10] + a[4] * a[2] * a[9] + a[8] * a[1] * a[6] - a[8] * a[2] * a[5];
    const double det = a[0] * inv[0] + a[1] * inv[4] + a[2] * inv[8] + a[3] * inv[12];
    if (!(det - det == 0.0) || det == 0.0) return false;
    for (int i = 0; i < 16; ++i) {
        o[i] = inv[i] / det;
        if (!(o[i] - o[i] == 0.0)) return false;
    }
    return true;
}

// Pixel rectangle outside which no ray can hit the box [-.5,.5]^2 x [-.25,.25]: the rays are defined by proj_inv and
// view_inv (setup_ray), so the box corners are projected with the inverses of exactly those.  With every corner in
// front of the eye the box projects inside the hull of its corners; 3 pixels of margin dwarf the rounding.  Anything
// doubtful (singular matrices, a corner at or behind the eye plane, non-finite numbers) -> the whole frame.
void hit_rectangle(const vr_uniforms& u, int W, int H, int rect[4])
{
    rect[0] = 0;
    rect[1] = 0;
    rect[2] = W - 1;
    rect[3] = H - 1;
    double proj[16], view[16];
    if (!invert4(u.proj_inv, proj) || !invert4(u.view_inv, view)) return;
    double x0 = 1e300, y0 = 1e300, x1 = -1e300, y1 = -1e300;
    for (int k = 0; k < 8; ++k) {
        const double wp[4] = {(k & 1) ? 0.5 : -0.5, (k & 2) ? 0.5 : -0.5, (k & 4) ? 0.25 : -0.25, 1.0};
        double e[4], cl[4];
        for (int r = 0; r < 4; ++r) e[r] = view[r] * wp[0] + view[4 + r] * wp[1] + view[8 + r] * wp[2] + view[12 + r] * wp[3];
        for (int r = 0; r < 4; ++r) cl[r] = proj[r] * e[0] + proj[4 + r] * e[1] + proj[8 + r] * e[2] + proj[12 + r] * e[3];
        if (!(cl[3] > 1e-9)) return;
        const double px = (cl[0] / cl[3] + 1.0) * 0.5 * W, py = (1.0 - cl[1] / cl[3]) * 0.5 * H;
        if (!(px - px == 0.0) || !(py - py == 0.0)) return;
        x0 = px < x0 ? px : x0;
        x1 = px > x1 ? px : x1;
        y0 = py < y0 ? py : y0;
        y1 = py > y1 ? py : y1;
    }
    auto clampd = [](double v, double lo, double hi) { return v < lo ? lo : (v > hi ? hi : v); };
    rect[0] = (int)clampd(x0 - 3.0, 0.0, (double)W);
    rect[1] = (int)clampd(y0 - 3.0, 0.0, (double)H);
    rect[2] = (int)clampd(x1 + 3.0, -1.0, (double)(W - 1));
    rect[3] = (int)clampd(y1 + 3.0, -1.0, (double)(H - 1));
}

// the fields of a launch's parameters that come from the uniforms of ONE frame
void fill_frame_params(MarchParams& P, const vr_uniforms& u)
{
    std::memcpy(P.proj_inv, u.proj_inv, sizeof P.proj_inv);
    std::memcpy(P.view_inv, u.view_inv, sizeof P.view_inv);
    hit_rectangle(u, P.W, P.H, P.rect);
    P.fragment_mode = u.fragment_mode;
    P.steps_count = u.steps_count;
    P.step_size = u.step_size;
    // IsInSampleCoords bounds, BasicVolumeApp.wgsl:73-74 (same f32 expressions as the shader)
    P.bmin[0] = 0.0f + u.clip_x[0]; P.bmin[1] = 0.0f + u.clip_y[0]; P.bmin[2] = 0.0f + u.clip_z[0];
    P.bmax[0] = 1.0f - u.clip_x[1]; P.bmax[1] = 1.0f - u.clip_y[1]; P.bmax[2] = 1.0f - u.clip_z[1];
    P.toggle_varstep = u.toggles[0];
    P.toggle_jitter = u.toggles[1];
    for (int i = 0; i < 3; ++i) {
        P.light_pos[i] = u.light_pos[i];
        P.light_amb[i] = u.light_ambient[i];
        P.light_dif[i] = u.light_diffuse[i];
        P.camera_pos[i] = u.camera_pos[i];
    }
}

// The kernel-time ring as tune_pick (vr_tuner.h) reads it: the span and the end of launch number L, 0 while its sort has not reported.
struct RingRecords {
    const KernelRing& ring;
    unsigned long long span_ticks(long long launch) const { return ring.span_ticks(KernelRing::slot(launch)); }
    unsigned long long end_ticks(long long launch) const { return ring.end_ticks(KernelRing::slot(launch)); }
};

// what a launch rendered, whatever kernel form it took (OrderSlot::scene_key: the key of the longest ray chain its sort reports)
// (a surface launch -- vr_set_output -- is a scene of its own: its chains say nothing about the colour launch's)
// (so is a launch between ray bounds -- vr_set_ray_bounds)
unsigned long long scene_key(const vr_ctx* c, const RenderRequest& R, bool surface, bool bounded)
{
    return ((unsigned long long)(R.variant | (surface ? 0x80 : 0) | (bounded ? 0x40 : 0)) << 16) ^ ((unsigned long long)R.world << 8) ^ (unsigned long long)R.rank ^ (R.packed ? 1ull << 63 : 0ull) ^
           ((unsigned long long)c->W << 40) ^ ((unsigned long long)c->H << 24);
}

// The arguments of a launch and the slots its shader samples (*nvol volumes); *off32: every one of them below 4 GiB.  Derives what the
// request does not say itself (R.surface, R.bounded) and refuses what these cannot do.
int check_render_args(vr_ctx* c, RenderRequest& R, int* nvol, bool* off32)
{
    // surface-position output (vr_set_output; a pick launch whatever the setting): the unlit / lit shader and the isosurface -- any
    // other variant is refused whatever the scene holds
    R.surface = c->output == VR_OUTPUT_SURFACE || R.pick_px[0] >= 0;
    if (R.surface && R.variant >= 0 && R.variant < VR_VARIANT_COUNT && !kShader[R.variant].surface)
        return fail(c, VR_ERR_UNSUPPORTED, "vr_render: surface output exists for BASIC, LIGHT and ISO only");
    // ray bounds (vr_set_ray_bounds; a pick launch ignores them): colour launches of one frame of the unlit shader and of the lit one
    // without shadows -- anything else is refused, never rendered with the occluder ignored
    R.bounded = (c->d_near || c->d_far) && R.pick_px[0] < 0;
    if (R.bounded && R.variant >= 0 && R.variant < VR_VARIANT_COUNT) {
        if (!kShader[R.variant].bounds) return fail(c, VR_ERR_UNSUPPORTED, "vr_render: ray bounds exist for BASIC and LIGHT only");
        if (R.surface) return fail(c, VR_ERR_UNSUPPORTED, "vr_render: ray bounds do not apply to surface output");
        if (R.variant == VR_VARIANT_LIGHT && c->shadows.div != 0)
            return fail(c, VR_ERR_UNSUPPORTED, "vr_render: ray bounds do not apply to LIGHT with shadows on");
        if (R.batch_u) return fail(c, VR_ERR_UNSUPPORTED, "vr_render: ray bounds do not apply to launches of several frames");
    }
    if (R.variant < 0 || R.variant >= VR_VARIANT_COUNT) return fail(c, VR_ERR_INVALID_ARG, "vr_render: bad variant");
    if (R.world < 1 || R.rank < 0 || R.rank >= R.world) return fail(c, VR_ERR_INVALID_ARG, "vr_render: bad rank/world");
    if (R.n_frames < 1 || R.n_frames > kBatchMax) return fail(c, VR_ERR_INVALID_ARG, "vr_render: 1 .. 4 frames per launch");
    if (R.batch_u) {
        if (!R.batch_out) return fail(c, VR_ERR_INVALID_ARG, "vr_render: a batch needs its output buffers");
        for (int f = 0; f < R.n_frames; ++f) {
            if (!R.batch_out[f]) return fail(c, VR_ERR_INVALID_ARG, "vr_render: output buffer " + std::to_string(f) + " of the batch is NULL");
            if (R.batch_u[f].steps_count < 0) return fail(c, VR_ERR_INVALID_ARG, "vr_render: negative steps_count");
            if (!is_identity(R.batch_u[f].model))  // (as vr_set_uniforms)
                return fail(c, VR_ERR_UNSUPPORTED, "vr_render: model matrix must be the identity (App/src/Application.cpp:489-492)");
        }
    } else {
        if (R.n_frames != 1) return fail(c, VR_ERR_INVALID_ARG, "vr_render: several frames per launch need their uniforms");
        if (!c->have_uniforms) return fail(c, VR_ERR_NOT_READY, "vr_render: vr_set_uniforms has not been called");
    }
    *nvol = kShader[R.variant].nvol;
    const int ntf = kShader[R.variant].ntf;
    *off32 = true;
    for (int i = 0; i < *nvol; ++i) {
        if (!c->vols[i].vol.data) return fail(c, VR_ERR_NOT_READY, "vr_render: volume slot " + std::to_string(i) + " is empty");
        if (c->vols[i].bytes() > 0xFFFFFFFFull) *off32 = false;
    }
    for (int i = 0; i < ntf; ++i)
        if (!c->tf[i].dev.opacity || !c->tf[i].dev.color)
            return fail(c, VR_ERR_NOT_READY, "vr_render: TF slot " + std::to_string(i) + " is empty");
    if ((R.batch_u ? R.batch_u[0] : c->u).steps_count < 0) return fail(c, VR_ERR_INVALID_ARG, "vr_render: negative steps_count");
    return VR_OK;
}

void fill_launch_params(const vr_ctx* c, MarchParams& P, const vr_uniforms& u0, int rank, int world, bool packed)
{
    std::memset(&P, 0, sizeof P);
    P.W = (int)c->W;
    P.H = (int)c->H;
    fill_frame_params(P, u0);
    for (int i = 0; i < VR_MAX_VOLUMES; ++i) P.vol[i] = linear_volume(c, i);
    for (int i = 0; i < VR_MAX_TFS; ++i) P.tf[i] = c->tf[i].dev;
    P.rank = rank;
    P.world = world;
    P.tiles_x = tiles_x_of(c);
    P.tiles_y = tiles_y_of(c);
    P.n_tiles = tile_count(c, rank, world);
    P.packed = packed ? 1 : 0;
    P.n_blocks = P.n_tiles * kBlocksPerTile;
    P.iso = c->iso;  // (every frame of a batch: fill_batch copies P)
}

// What the kernel choice (vr_choice.h) reads of a launch and of the context.  requested: the flavour asked for -- only the default
// choice looks the chain length up.
ChoiceFacts choice_facts(const vr_ctx* c, const RenderRequest& R, int requested)
{
    ChoiceFacts F = {};
    F.variant = R.variant, F.rank = R.rank, F.world = R.world, F.n_frames = R.n_frames;
    F.packed = R.packed, F.surface = R.surface, F.bounded = R.bounded;
    for (int i = 0; i < VR_MAX_VOLUMES; ++i) {
        const VolumeSlot& v = c->vols[i];
        F.vols[i] = {v.vol.nx, v.vol.ny, v.vol.nz, v.bricked.p != nullptr, v.bdens.p != nullptr, v.bricks.p != nullptr};
    }
    for (int i = 0; i < VR_MAX_TFS; ++i) {
        const TfSlot& t = c->tf[i];
        F.tf[i] = {t.dev.res_o, t.dev.res_c, t.zero_prefix, t.color_finite, t.opacity_finite};
    }
    F.layout_mode = c->layout_mode, F.p2_window = c->p2_window, F.n_cus = c->n_cus, F.W = c->W, F.H = c->H;
    F.frames_in_flight = c->frames_in_flight;
    F.shadows = c->shadows.div != 0;
    F.lights_finite = lights_finite(R.batch_u ? R.batch_u : &c->u, R.n_frames);
    F.active_fraction = c->skip.active_fraction;
    F.tuner_mode = c->tuner.mode;
    F.last_chain = requested == 0 ? c->order.last_chain(scene_key(c, R, false, false)) : 0;  // (the plain colour launch's key, always)
    F.brick_epoch = c->brick_epoch, F.tf_epoch = c->tf_epoch, F.arith = c->arith;
    return F;
}

// Claims the record slot of the next launch, *cb = order_seq % kInFlight.  (Record slot and order slot both derive from order_seq, which
// advances only once a launch has really been enqueued -- finish_slot: a failed enqueue cannot shift one against the other.)  The slot's
// previous launch (kInFlight launches ago, possibly on another stream) must have finished before its records are written again or
// re-allocated: this host wait is what bounds the launches in flight to kInFlight.  The sort that read those records is waited for on
// `s`, so that whoever takes the slot next may write them behind this launch's event -- at once, or, with `stale_sort`, by the caller
// (the march launch: reserve_block_counts, wait_for_order).
int claim_slot(vr_ctx* c, hipStream_t s, int* cb, const OrderSlot** stale_sort = nullptr)
{
    const int k = (int)(c->order_seq % (unsigned long long)kInFlight);
    *cb = k;
    if (c->slot[k].used) VR_HIP(c, hipEventSynchronize(c->slot[k].done));
    const OrderSlot* sort = nullptr;
    if (c->order_seq >= (unsigned long long)kInFlight) {
        const OrderSlot& po = c->order.ring[(c->order_seq - kInFlight) % kOrderRing];
        if (po.valid && po.seq + kInFlight == c->order_seq) sort = &po;
    }
    if (stale_sort) *stale_sort = sort;
    else if (sort) VR_HIP(c, hipStreamWaitEvent(s, sort->sorted, 0));
    return VR_OK;
}

// The march launch's records in its slot, n_records blocks.  *slot_sort (claim_slot) is waited for at once only when the buffer is
// re-allocated (the memset behind the allocation writes it).
int reserve_block_counts(vr_ctx* c, hipStream_t s, int k, size_t n_records, const OrderSlot** slot_sort)
{
    DevBuf<unsigned long long>& b = c->slot[k].block_counts;
    if (n_records * kBlockRecord > b.cap) {
        if (*slot_sort) VR_HIP(c, hipStreamWaitEvent(s, (*slot_sort)->sorted, 0));
        *slot_sort = nullptr;
        VR_HIP(c, b.reserve(n_records * kBlockRecord));
        VR_HIP(c, hipMemsetAsync(b, 0, n_records * kBlockRecord * sizeof(unsigned long long), s));
    }
    return VR_OK;
}

// The launch order an ordered launch takes (*order; nullptr = index order) and the one wait for a sort it implies.  The order: the most
// recent sort of a launch of the same shape (okey) that is three or four launches old (two or three more than the frames the caller
// says it keeps in flight, if that is more: with short frames -- C2, 0.08 ms -- the sort of the launch that finished one frame time ago
// is itself only just finishing) -- a younger one may still be waiting for its launch to finish (the sorts run on a side stream behind
// their launches; waiting for one would put a bubble into this stream, and with four frames in flight it would chain this launch behind
// the one three before it), an older one's buffer may be recycled under this launch; ordered behind it by its event (long complete by
// then).  A stream's wait for another stream's event costs the stream 5 us per launch even when the event completed long ago
// (tools/ubench/stream_gap.hip), so the wait for `slot_sort` is left out when the order's wait covers it: every sort runs on the one
// order stream, in the order of the launches.
int wait_for_order(vr_ctx* c, hipStream_t s, bool ordered, unsigned long long okey, const OrderSlot* slot_sort, const unsigned** order)
{
    *order = nullptr;
    if (ordered) {
        const unsigned long long age = (unsigned long long)(c->frames_in_flight + 2 > 3 ? c->frames_in_flight + 2 : 3);
        if (const OrderSlot* best = c->order.best(okey, c->order_seq, age)) {
            VR_HIP(c, hipStreamWaitEvent(s, best->sorted, 0));
            if (slot_sort && best->seq >= slot_sort->seq) slot_sort = nullptr;  // (covered: the order stream runs its sorts in order)
            *order = best->buf;
        }
    }
    if (slot_sort) VR_HIP(c, hipStreamWaitEvent(s, slot_sort->sorted, 0));
    return VR_OK;
}

// The sort behind an ordered march launch (finish_slot).
struct SortJob {
    unsigned long long okey, skey;  // OrderSlot::key, ::scene_key
    unsigned n_blocks;
    int ring;                       // the launch's KernelRing::slot
    bool time_with_events, pw;
};

// Gives record slot cb back behind the launch on `s` that claimed it: the slot's event, and then the next launch takes the next slots.
// For an ordered march launch (`sort`), in between: the sort of its n_blocks records on the order stream into order slot
// order_seq % kOrderRing -- the launch order of later launches; the longest chain (h_chain), and unless the launch is timed with events
// its span and end (KernelRing's h_span / h_end, slot `ring`); the persistent kernels' queue heads cleared.
int finish_slot(vr_ctx* c, hipStream_t s, int cb, const SortJob* sort = nullptr)
{
    LaunchOrder& O = c->order;
    OrderSlot& o = O.ring[c->order_seq % kOrderRing];
    if (sort) {
        o.valid = false;
        if (sort->n_blocks > o.buf.cap) VR_HIP(c, o.buf.reserve(sort->n_blocks));
        o.stream = s;
        o.key = sort->okey;
        o.scene_key = sort->skey;
        o.seq = c->order_seq;
        if (O.h_chain) O.h_chain[c->order_seq % kOrderRing] = 0;  // not known until this launch's sort has run
    }
    VR_HIP(c, hipEventRecord(c->slot[cb].done, s));
    c->slot[cb].used = true;
    if (sort) {
        const bool time_with_events = sort->time_with_events;
        VR_HIP(c, hipStreamWaitEvent(O.stream, c->slot[cb].done, 0));
        hipLaunchKernelGGL(order_blocks_kernel, dim3(1), dim3(1024), 0, O.stream, c->slot[cb].block_counts, (int)sort->n_blocks, o.buf,
                           O.h_chain ? O.h_chain + (c->order_seq % kOrderRing) : (unsigned*)nullptr,
                           (c->ring.h_span && !time_with_events) ? c->ring.h_span + sort->ring : (unsigned long long*)nullptr,
                           sort->pw ? c->d_pw_heads + (size_t)cb * 8 * 64 : (unsigned*)nullptr,
                           (c->ring.h_span && c->ring.h_end && !time_with_events) ? c->ring.h_end + sort->ring : (unsigned long long*)nullptr);
        VR_HIP(c, hipGetLastError());
        if (sort->pw) c->slot[cb].pw_heads_dirty = false;  // (the sort zeroes the heads behind the launch: the slot's next user finds them clean)
        VR_HIP(c, hipEventRecord(o.sorted, O.stream));
        o.valid = true;
    }
    ++c->order_seq;
    return VR_OK;
}

// The launch's frames (frame f: every n_frames-th group of 8 workgroups, MarchBatch), each with its own uniforms, output and records;
// the launch order (a heuristic of the shape) is shared.
const MarchBatch& fill_batch(MarchParams& P, int n_frames, const vr_uniforms* batch_u, void* const* batch_out, unsigned blocks_per_frame)
{
    static thread_local MarchBatch B;
    P.batch_n = (unsigned)n_frames;
    B.frame[0] = P;
    for (int f = 1; f < n_frames; ++f) {
        MarchParams& Pf = B.frame[f];
        Pf = P;
        fill_frame_params(Pf, batch_u[f]);
        Pf.out = (float4*)batch_out[f];
        Pf.block_counts = P.block_counts + (size_t)f * blocks_per_frame * kBlockRecord;
    }
    B.n_frames = (unsigned)n_frames;
    return B;
}

// the request of the vr_render* entry points: rank's share of a frame (packed: as tiles) on the caller's stream or the context's
RenderRequest render_request(const vr_ctx* c, int variant, int rank, int world, bool packed, void* out, void* stream, int n_frames = 1,
                             const vr_uniforms* batch_u = nullptr, void* const* batch_out = nullptr)
{
    RenderRequest R;
    R.variant = variant, R.rank = rank, R.world = world, R.packed = packed;
    R.out = (float4*)out;
    R.stream = stream ? (hipStream_t)stream : (hipStream_t)c->stream;
    R.n_frames = n_frames, R.batch_u = batch_u, R.batch_out = batch_out;
    return R;
}

// Enqueue one march launch (RenderRequest) on R.stream.
int enqueue_render(vr_ctx* c, RenderRequest R)
{
    int nvol;
    bool off32;
    if (const int rc = check_render_args(c, R, &nvol, &off32)) return rc;
    float4* out = R.out;
    hipStream_t s = R.stream;
    // shadows: every frame of the launch reads one light volume, of less than 4 GiB (a surface launch reads none)
    const bool shadowed = R.variant == VR_VARIANT_LIGHT && c->shadows.div != 0 && !R.surface;
    ShadowKey shadow_k;
    if (shadowed) {
        shadow_k = shadow_key(c, R.batch_u ? R.batch_u[0] : c->u);
        for (int f = 1; f < R.n_frames; ++f)
            if (!(shadow_key(c, R.batch_u[f]) == shadow_k))
                return fail(c, VR_ERR_UNSUPPORTED, "vr_render: the frames of a shadowed batch must share the light and the clip box");
        int g[3];
        if (shadow_grid(c, g) * sizeof(float) >= (1ull << 32))
            return fail(c, VR_ERR_UNSUPPORTED, "vr_render: the light volume would take 4 GiB or more (a larger divisor)");
    }
    c->shadows.cur = -1;
    if (R.batch_u) out = (float4*)R.batch_out[0];
    VR_HIP(c, hipSetDevice(c->device));
    (void)hipGetLastError();  // a stale error of somebody else's call must not be reported as a failed launch below
    VR_HIP(c, c->edits.order.order_behind(s));  // the launch comes after every asynchronous edit made so far

    MarchParams P;
    fill_launch_params(c, P, R.batch_u ? R.batch_u[0] : c->u, R.rank, R.world, R.packed);
    if (R.surface && R.variant != VR_VARIANT_ISO) P.iso = c->surf_tau;  // (these launches read no level)
    if (R.pick_px[0] >= 0)  // vr_pick: the one pixel's ray (a rectangle no larger than the one the box can be hit in)
        for (int a = 0; a < 2; ++a) {
            P.rect[a] = P.rect[a] > R.pick_px[a] ? P.rect[a] : R.pick_px[a];
            P.rect[2 + a] = P.rect[2 + a] < R.pick_px[a] ? P.rect[2 + a] : R.pick_px[a];
        }
    // the kernel choice: what can run, the skipping state (the prior reads its share of active bricks), the flavour
    const int requested = c->flavour == 0 ? c->default_flavour : c->flavour;
    ChoiceFacts F = choice_facts(c, R, requested);
    const Eligibility E = eligibility(F, requested);
    if (E.can_skip) {
        if (const int rc = prepare_skip(c, R.variant, s, P)) return rc;
        if (c->skip.pending) ++c->skip.unbounded_launches;
    }
    F.active_fraction = c->skip.active_fraction;  // (prepare_skip may just have learnt it)
    const Choice choice = choose_flavour(F, requested, E);
    const int fl = !choice.tune ? choice.prior
                                : tune_pick(c->tuner, RingRecords{c->ring}, c->last.ring_head, c->frames_in_flight, choice.key, choice.shape, choice.cand,
                                            choice.n, E.chain_known, c->ring.h_span && c->ring.h_end && !c->event_timing);
    c->last.flavour = fl;
    const KernelForm form = kernel_form(fl, R.variant);
    c->last.unmeasured = !form.measured();
    const float2* vrange = nullptr;
    if (form.skip && form.range_records() && E.indexable) {  // (else: the pair's form without skipping)
        vrange = prepare_proj(c, s, P);
        if (!vrange) return VR_ERR_HIP;
    }

    if (c->layout_mode == 0) use_bricked_copies(c, P);
    if (form.lut && P.vol[0].bricked) P.vol[0].lut = 1;  // (march_kernel fills the tables; every fetch of volume 0 goes through them)
    if (form.family == KernelForm::kBound) {  // the depth buffers, in the slots these shaders do not sample (vr_bound.h)
        P.vol[1].data = reinterpret_cast<const float4*>(c->d_near);
        P.vol[2].data = reinterpret_cast<const float4*>(c->d_far);
    }
    for (int i = 0; i < nvol; ++i)  // (a bricked copy is padded to whole bricks: a volume just below 4 GiB may cross the line)
        if (P.vol[i].bricked && bricked_grid(P.vol[i]).slots * 16 > 0xFFFFFFFFull) off32 = false;

    if (R.packed && !out) {
        size_t need = (size_t)P.n_tiles * kTile * kTile;
        if (need > c->d_tiles.cap) VR_HIP(c, c->d_tiles.reserve(need));
        out = c->d_tiles;
    } else if (!out) {
        out = c->d_frame;
    }
    P.out = out;
    c->last.tiles = R.packed ? P.n_tiles : 0;

    if (R.frame_events) VR_HIP(c, hipEventRecord(c->tm.ev_begin, s));
    // the skipping form of a pair runs with its records in place -- the projections' range records, else the distance field -- and
    // as the pair's other kernels without them
    const bool skip = form.skip && (form.range_records() ? vrange != nullptr : P.brick_dist != nullptr);
    if (P.n_blocks > 0) {
        // the light volume it reads: built here when its key has none (inside vr_last_timing's total, outside its kernel time)
        if (shadowed)
            if (const int rc = prepare_shadow(c, s, P, shadow_k, skip, off32)) return rc;
        const LaunchShape shape = launch_shape(form, F, E, off32, P.vol[0].lut != 0);
        const dim3 grid(shape.blocks);  // the LOGICAL blocks of a frame (records, launch order)
        if (R.n_frames > 1 && grid.x % 8u != 0) return fail(c, VR_ERR_INVALID_ARG, "vr_render: launch shape cannot carry several frames");
        const bool pw = shape.pw, ordered = shape.ordered;
        // the ring slots: record buffer, then the launch order and the sort waits (a launch order is kept per launch shape -- not per
        // flavour: the kernels that march one packet per wavefront -- 6, 12, 13, 16, 17 -- share the logical blocks, so an order sorted
        // behind one of them serves the others, and the measured choice tries them in turn on a live scene)
        int cb;
        const OrderSlot* slot_sort;
        if (const int rc = claim_slot(c, s, &cb, &slot_sort)) return rc;
        if (const int rc = reserve_block_counts(c, s, cb, (size_t)grid.x * (size_t)R.n_frames, &slot_sort)) return rc;
        P.block_counts = c->slot[cb].block_counts;
        c->last.cnt_buf = cb;
        const unsigned long long okey = ((unsigned long long)grid.x << 32) ^ ((unsigned long long)(64 * shape.wpb) << 20) ^
                                        ((unsigned long long)(R.variant | (R.surface ? 0x10 : 0) | (R.bounded ? 0x20 : 0)) << 16) ^ ((unsigned long long)R.world << 8) ^
                                        (unsigned long long)R.rank ^ (R.packed ? 1ull << 63 : 0ull);
        if (const int rc = wait_for_order(c, s, ordered, okey, slot_sort, &P.order)) return rc;

        const int ring = KernelRing::slot(c->last.ring_head);
        if (R.frame_events) VR_HIP(c, hipEventRecord(c->tm.ev_k0, s));
        // launches with a sort behind them are timed from their own records (order_blocks_kernel); events only otherwise
        const bool time_with_events = !(ordered && c->ring.h_span) || c->event_timing;
        c->ring.begin(ring, time_with_events);
        if (time_with_events) VR_HIP(c, hipEventRecord(c->ring.k0[ring], s));
        const MarchBatch& B = fill_batch(P, R.n_frames, R.batch_u, R.batch_out, grid.x);
        LaunchDesc L = {};
        L.variant = R.variant;
        L.family = form.family;
        L.off32 = off32;
        L.lanes = form.lanes;
        L.pipe = form.pipe;
        L.ltf = shape.ltf;
        L.p2_win = shape.p2_win;
        L.lds_bytes = shape.lds_bytes;
        L.grid = dim3(shape.grid);
        L.block = dim3(shape.block);
        L.vrange = vrange;
        L.skip = skip;
        L.surface = R.surface;
        if (pw) {  // persistent wavefronts: the workgroups take the logical blocks from the slot's queue
            L.queue = PwQueue{c->d_pw_heads + (size_t)cb * 8 * 64, grid.x, c->p2_window};
            if (c->slot[cb].pw_heads_dirty) VR_HIP(c, hipMemsetAsync(L.queue.heads, 0, 8 * 64 * sizeof(unsigned), s));
            c->slot[cb].pw_heads_dirty = true;  // (until the sort that clears them behind this launch has really been enqueued)
        }
        if (!(c->arith == VR_ARITH_FUSED ? vrf::launch_march(L, s, B) : vr::launch_march(L, s, B)))  // (never: tests/test_choice.py)
            return fail(c, VR_ERR_INTERNAL, "vr_render: no kernel for flavour " + std::to_string(fl) + " of variant " + std::to_string(R.variant));
        VR_HIP(c, hipGetLastError());
        mark_reads(c, P);
        if (time_with_events) VR_HIP(c, hipEventRecord(c->ring.k1[ring], s));

        const SortJob sort = {okey, scene_key(c, R, R.surface, R.bounded), grid.x, ring, time_with_events, pw};
        if (const int rc = finish_slot(c, s, cb, ordered ? &sort : nullptr)) return rc;
        if (R.frame_events) VR_HIP(c, hipEventRecord(c->tm.ev_k1, s));
        ++c->last.ring_head;
        c->last.cnt_blocks = (int)grid.x;
        c->last.cnt_offset = (size_t)(R.n_frames - 1) * grid.x * kBlockRecord;  // vr_last_counters: the LAST frame of the launch
    } else {
        c->last.cnt_blocks = 0;
        c->last.cnt_offset = 0;
        if (R.frame_events) {
            VR_HIP(c, hipEventRecord(c->tm.ev_k0, s));
            VR_HIP(c, hipEventRecord(c->tm.ev_k1, s));
        }
    }
    // the per-block counts are summed and copied to the host when somebody asks for them (fetch_counters)
    c->last.cnt_pending = true;
    if (R.frame_events) VR_HIP(c, hipEventRecord(c->tm.ev_end, s));
    c->last.timed = R.frame_events;
    return VR_OK;
}

// Sums the per-block counts of the last launch into h_counters (blocks until that launch has finished).
int fetch_counters(vr_ctx* c)
{
    if (!c->last.cnt_pending) return VR_OK;
    VR_HIP(c, hipSetDevice(c->device));
    (void)hipGetLastError();
    if (c->last.cnt_blocks > 0) {
        // the launch may have been enqueued on a stream of the caller's that no longer exists: wait for the event recorded
        // behind it (owned by the context; other launches in flight are not waited for), then use the context's own stream
        VR_HIP(c, hipEventSynchronize(c->slot[c->last.cnt_buf].done));
        hipLaunchKernelGGL(sum_block_counts_kernel, dim3(1), dim3(256), 0, c->stream, c->slot[c->last.cnt_buf].block_counts + c->last.cnt_offset,
                           c->last.cnt_blocks, c->d_counters);
        VR_HIP(c, hipGetLastError());
        VR_HIP(c, hipMemcpyAsync(c->h_counters, c->d_counters, 3 * sizeof(unsigned long long), hipMemcpyDeviceToHost,
                                 c->stream));
        VR_HIP(c, hipStreamSynchronize(c->stream));
    } else {
        c->h_counters[0] = c->h_counters[1] = c->h_counters[2] = 0;
    }
    c->last.cnt_pending = false;
    return VR_OK;
}

}  // namespace

extern "C" {

// vr_render / vr_render_tiles: one timed launch on the context's stream, waited for, its counters fetched
static int render_and_wait(vr_ctx* c, int variant, int rank, int world, bool packed)
{
    if (!c) return VR_ERR_INVALID_ARG;
    RenderRequest R = render_request(c, variant, rank, world, packed, nullptr, nullptr);
    R.frame_events = true;
    int rc = enqueue_render(c, R);
    if (rc != VR_OK) return rc;
    VR_HIP(c, hipStreamSynchronize(c->stream));
    return fetch_counters(c);
}

int vr_render(vr_ctx* c, int variant) { return render_and_wait(c, variant, 0, 1, false); }

int vr_tile_count(const vr_ctx* c, int rank, int world)
{
    if (!c || world < 1 || rank < 0 || rank >= world) return VR_ERR_INVALID_ARG;
    return tile_count(c, rank, world);
}

int vr_render_tiles(vr_ctx* c, int variant, int rank, int world) { return render_and_wait(c, variant, rank, world, true); }

int vr_render_async(vr_ctx* c, int variant, void* d_frame, void* stream)
{
    if (!c) return VR_ERR_INVALID_ARG;
    return enqueue_render(c, render_request(c, variant, 0, 1, false, d_frame, stream));
}

int vr_render_tiles_async(vr_ctx* c, int variant, int rank, int world, void* d_tiles, void* stream)
{
    if (!c) return VR_ERR_INVALID_ARG;
    return enqueue_render(c, render_request(c, variant, rank, world, true, d_tiles, stream));
}

int vr_render_batch_async(vr_ctx* c, int variant, int n_frames, const vr_uniforms* uniforms, void* const* d_frames, void* stream)
{
    if (!c) return VR_ERR_INVALID_ARG;
    if (!uniforms || !d_frames) return fail(c, VR_ERR_INVALID_ARG, "vr_render_batch_async: uniforms / buffers are NULL");
    return enqueue_render(c, render_request(c, variant, 0, 1, false, nullptr, stream, n_frames, uniforms, d_frames));
}

int vr_render_tiles_batch_async(vr_ctx* c, int variant, int rank, int world, int n_frames, const vr_uniforms* uniforms,
                                void* const* d_tiles, void* stream)
{
    if (!c) return VR_ERR_INVALID_ARG;
    if (!uniforms || !d_tiles) return fail(c, VR_ERR_INVALID_ARG, "vr_render_tiles_batch_async: uniforms / buffers are NULL");
    return enqueue_render(c, render_request(c, variant, rank, world, true, nullptr, stream, n_frames, uniforms, d_tiles));
}

int vr_last_timing(vr_ctx* c, float* kernel_ms, float* total_ms)
{
    if (!c) return VR_ERR_INVALID_ARG;
    if (!c->last.timed) return fail(c, VR_ERR_NOT_READY, "vr_last_timing: no vr_render / vr_render_tiles since the context was created or an *_async call");
    VR_HIP(c, hipSetDevice(c->device));
    VR_HIP(c, hipEventSynchronize(c->tm.ev_end));
    float k = 0.0f, t = 0.0f;
    VR_HIP(c, hipEventElapsedTime(&k, c->tm.ev_k0, c->tm.ev_k1));
    VR_HIP(c, hipEventElapsedTime(&t, c->tm.ev_begin, c->tm.ev_end));
    if (kernel_ms) *kernel_ms = k;
    if (total_ms) *total_ms = t;
    return VR_OK;
}

int vr_kernel_times(vr_ctx* c, float* out_ms, int capacity)
{
    if (!c) return VR_ERR_INVALID_ARG;
    if (!out_ms || capacity < 0) return fail(c, VR_ERR_INVALID_ARG, "vr_kernel_times: bad arguments");
    VR_HIP(c, hipSetDevice(c->device));
    const long long since = c->last.ring_head - c->ring.reported_from;  // launches since the last vr_reset_kernel_times
    long long have = since < kRing ? since : kRing;
    int n = (int)(have < capacity ? have : capacity);
    bool synced = false;
    for (int i = 0; i < n; ++i) {
        const int slot = KernelRing::slot(c->last.ring_head - n + i);
        if (!c->ring.by_events[slot]) {  // from the launch's records, written by the sort that runs behind it
            if (!synced) VR_HIP(c, hipStreamSynchronize(c->order.stream));
            synced = true;
            const unsigned long long ticks = c->ring.span_ticks(slot);
            out_ms[i] = ticks ? (float)((double)(ticks - 1) * 1.0e-5) : 0.0f;
            continue;
        }
        VR_HIP(c, hipEventSynchronize(c->ring.k1[slot]));
        VR_HIP(c, hipEventElapsedTime(&out_ms[i], c->ring.k0[slot], c->ring.k1[slot]));
    }
    return n;
}

int vr_set_kernel_timing(vr_ctx* c, int mode)
{
    if (!c) return VR_ERR_INVALID_ARG;
    if (mode != VR_TIMING_RECORDS && mode != VR_TIMING_EVENTS) return fail(c, VR_ERR_INVALID_ARG, "vr_set_kernel_timing: bad mode");
    c->event_timing = mode == VR_TIMING_EVENTS;
    return VR_OK;
}

int vr_reset_kernel_times(vr_ctx* c)
{
    if (!c) return VR_ERR_INVALID_ARG;
    // (sorts of earlier launches still report their launch's duration into the ring: let them finish first)
    VR_HIP(c, hipSetDevice(c->device));
    VR_HIP(c, hipStreamSynchronize(c->order.stream));
    // (the launch numbers go on: a running trial of the measured choice names its launches by them)
    c->ring.reported_from = c->last.ring_head;
    return VR_OK;
}

int vr_last_covered_pixels(vr_ctx* c, uint64_t* covered)
{
    uint64_t all[3];
    if (!c || !covered) return VR_ERR_INVALID_ARG;
    const int rc = vr_last_counters(c, all);
    if (rc == VR_OK) *covered = all[1];
    return rc;
}

int vr_last_counters(vr_ctx* c, uint64_t out[3])
{
    if (!c || !out) return VR_ERR_INVALID_ARG;
    VR_HIP(c, hipSetDevice(c->device));
    VR_HIP(c, hipStreamSynchronize(c->stream));
    int rc = fetch_counters(c);
    if (rc != VR_OK) return rc;
    out[0] = c->h_counters[0];
    out[1] = c->h_counters[1];
    out[2] = c->h_counters[2];
    return VR_OK;
}

int vr_last_block_trace(vr_ctx* c, uint64_t* out, int capacity)
{
    if (!c || capacity < 0 || (capacity > 0 && !out)) return VR_ERR_INVALID_ARG;
    VR_HIP(c, hipSetDevice(c->device));
    VR_HIP(c, hipDeviceSynchronize());
    const int n = c->last.cnt_blocks < capacity ? c->last.cnt_blocks : capacity;
    if (n > 0) {
        const unsigned long long* src = c->slot[c->last.cnt_buf].block_counts + c->last.cnt_offset;
        VR_HIP(c, hipMemcpy(out, src, (size_t)n * kBlockRecord * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    }
    return c->last.cnt_blocks;
}

int vr_last_kernel_flavour(vr_ctx* c)
{
    if (!c) return VR_ERR_INVALID_ARG;
    return c->last.flavour;
}

int vr_skip_field(vr_ctx* c, int variant, uint8_t* dist, size_t capacity, int dims[3], int box[6], uint64_t* active)
{
    if (!c) return VR_ERR_INVALID_ARG;
    if (variant < 0 || variant >= VR_VARIANT_COUNT) return fail(c, VR_ERR_INVALID_ARG, "vr_skip_field: bad variant");
    if (capacity > 0 && !dist) return fail(c, VR_ERR_INVALID_ARG, "vr_skip_field: dist is NULL");
    const int nvol = kShader[variant].nvol, ntf = kShader[variant].ntf;
    for (int i = 0; i < nvol; ++i)
        if (!c->vols[i].vol.data) return fail(c, VR_ERR_NOT_READY, "vr_skip_field: volume slot " + std::to_string(i) + " is empty");
    for (int i = 0; i < ntf; ++i)
        if (!c->tf[i].dev.opacity || !c->tf[i].dev.color) return fail(c, VR_ERR_NOT_READY, "vr_skip_field: TF slot " + std::to_string(i) + " is empty");
    if (const int rc = drain(c)) return rc;
    (void)hipGetLastError();
    const Eligibility E = eligibility(choice_facts(c, render_request(c, variant, 0, 1, false, nullptr, nullptr), 0), 0);
    if (!E.can_skip) return fail(c, VR_ERR_NOT_READY, "vr_skip_field: launches of this variant do not skip empty space now");
    MarchParams P;
    std::memset(&P, 0, sizeof P);
    if (const int rc = prepare_skip(c, variant, c->stream, P)) return rc;
    VR_HIP(c, hipStreamSynchronize(c->stream));
    const SkipField& F = c->skip;
    const float bs[3] = {P.bsx, P.bsy, P.bsz};
    c->skip.adopt(bs);
    if (F.pending) return fail(c, VR_ERR_HIP, "vr_skip_field: the field's count and box did not arrive");
    const size_t n = (size_t)F.bn[0] * F.bn[1] * F.bn[2];
    if (capacity > 0) VR_HIP(c, hipMemcpy(dist, F.brick_dist, capacity < n ? capacity : n, hipMemcpyDeviceToHost));
    if (dims)
        for (int a = 0; a < 3; ++a) dims[a] = F.bn[a];
    if (box)
        for (int a = 0; a < 6; ++a) box[a] = F.box[a];
    if (active) *active = F.active;
    return (int)n;
}

int vr_skip_hull(vr_ctx* c, int variant, int lo[13], int hi[13])
{
    // (the field is built and its summary adopted as vr_skip_field does it; its errors carry that name)
    const int n = vr_skip_field(c, variant, nullptr, 0, nullptr, nullptr, nullptr);
    if (n < 0) return n;
    static_assert(kHullDirs == 13, "include/vr.h documents 13 directions");
    for (int d = 0; d < kHullDirs; ++d) {
        if (lo) lo[d] = c->skip.hull_lo[d];
        if (hi) hi[d] = c->skip.hull_hi[d];
    }
    return VR_OK;
}

int vr_skip_indexable(uint16_t nx, uint16_t ny, uint16_t nz)
{
    return bricks_indexable(skip_bricks(nx), skip_bricks(ny), skip_bricks(nz)) ? 1 : 0;
}

int64_t vr_unbounded_box_launches(vr_ctx* c)
{
    if (!c) return VR_ERR_INVALID_ARG;
    return c->skip.unbounded_launches;
}

int vr_kernel_choice(vr_ctx* c, int flavours[6], float ms_per_launch[6], int* chosen)
{
    if (!c) return VR_ERR_INVALID_ARG;
    if (c->last.unmeasured) {  // (the projections', the isosurface's, the shadowed, the surface and the bounded forms)
        if (chosen) *chosen = -1;
        return 0;
    }
    const Trial* t = c->tuner.latest();
    if (chosen) *chosen = t ? t->choice : -1;
    if (!t) return 0;
    for (int i = 0; i < 6; ++i) {
        if (flavours) flavours[i] = i < t->n ? t->cand[i] : 0;
        if (ms_per_launch) ms_per_launch[i] = i < t->n ? t->cost[i] : 0.0f;
    }
    return t->n;
}

}  // extern "C"
