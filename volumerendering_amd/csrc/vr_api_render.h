// vr_api_render.h -- a march launch: its arguments, what may run (eligibility), the kernel choice, the record slots (claim_slot /
// finish_slot), the launch itself, the launch-order sort behind it, counters and timing.  Part of vr_api.hip's translation unit.
#pragma once

namespace {

// (defined in vr_api_views.h)
ShadowKey shadow_key(const vr_ctx* c, const vr_uniforms& u);
size_t shadow_grid(const vr_ctx* c, int g[3]);
int prepare_shadow(vr_ctx* c, hipStream_t s, MarchParams& P, const ShadowKey& key, bool skip, bool off32);

int tiles_x_of(const vr_ctx* c) { return (int)((c->W + kTile - 1) / kTile); }
int tiles_y_of(const vr_ctx* c) { return (int)((c->H + kTile - 1) / kTile); }

int tile_count(const vr_ctx* c, int rank, int world)
{
    int total = tiles_x_of(c) * tiles_y_of(c);
    if (rank >= total) return 0;
    return (total - rank + world - 1) / world;
}

bool is_identity(const float* m)
{
    for (int i = 0; i < 16; ++i)
        if (m[i] != ((i % 5 == 0) ? 1.0f : 0.0f)) return false;
    return true;
}

bool is_projection(int variant) { return variant == VR_VARIANT_MIP || variant == VR_VARIANT_MINIP || variant == VR_VARIANT_AVERAGE; }

// volumes / TF pairs each variant samples (vr.h slot tables)
void variant_needs(int variant, int* nvol, int* ntf)
{
    switch (variant) {
    case VR_VARIANT_BASIC:
    case VR_VARIANT_LIGHT:
    case VR_VARIANT_LIGHT_INSHADER:
    case VR_VARIANT_MIP:
    case VR_VARIANT_MINIP:
    case VR_VARIANT_AVERAGE:
    case VR_VARIANT_ISO: *nvol = 1; *ntf = 1; break;
    case VR_VARIANT_VOLUME_MASK: *nvol = 3; *ntf = 2; break;
    case VR_VARIANT_THREE_FILES: *nvol = 2; *ntf = 2; break;  // the mask (slot 2) is bound but never sampled
    case VR_VARIANT_MULTI_CTRT: *nvol = 2; *ntf = 2; break;
    case VR_VARIANT_ILLUSTRATIVE: *nvol = 2; *ntf = 2; break;
    default: *nvol = 2; *ntf = 1; break;  // TF_CALIB
    }
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

// rays per hardware lane (n_cus x 4 x 5 x 64) of `frames` launches of this rank's share of the frame: how full they keep the machine
double rays_per_lane(const vr_ctx* c, int rank, int world, int frames)
{
    const long long px = (long long)tile_count(c, rank, world) * kTile * kTile;
    return (double)px * frames / ((double)c->n_cus * 4.0 * 5.0 * 64.0);
}

// what a launch rendered, whatever kernel form it took (OrderSlot::scene_key: the key of the longest ray chain its sort reports)
// (a surface launch -- vr_set_output -- is a scene of its own: its chains say nothing about the colour launch's)
// (so is a launch between ray bounds -- vr_set_ray_bounds)
unsigned long long scene_key(const vr_ctx* c, const RenderRequest& R, bool surface, bool bounded)
{
    return ((unsigned long long)(R.variant | (surface ? 0x80 : 0) | (bounded ? 0x40 : 0)) << 16) ^ ((unsigned long long)R.world << 8) ^ (unsigned long long)R.rank ^ (R.packed ? 1ull << 63 : 0ull) ^
           ((unsigned long long)c->W << 40) ^ ((unsigned long long)c->H << 24);
}

// TF slot 0 fits a workgroup's LDS beside nothing else: one resolution for both tables, R <= 8190 (128 KiB)
bool tf0_fits_lds(const vr_ctx* c) { return c->tf[0].dev.res_o == c->tf[0].dev.res_c && c->tf[0].dev.res_o + 2 <= 8192; }

// The arguments of a launch and the slots its shader samples (*nvol volumes); *off32: every one of them below 4 GiB.  Derives what the
// request does not say itself (R.surface, R.bounded) and refuses what these cannot do.
int check_render_args(vr_ctx* c, RenderRequest& R, int* nvol, bool* off32)
{
    // surface-position output (vr_set_output; a pick launch whatever the setting): the unlit / lit shader and the isosurface -- any
    // other variant is refused whatever the scene holds
    R.surface = c->output == VR_OUTPUT_SURFACE || R.pick_px[0] >= 0;
    if (R.surface && R.variant >= 0 && R.variant < VR_VARIANT_COUNT && R.variant != VR_VARIANT_BASIC && R.variant != VR_VARIANT_LIGHT &&
        R.variant != VR_VARIANT_ISO)
        return fail(c, VR_ERR_UNSUPPORTED, "vr_render: surface output exists for BASIC, LIGHT and ISO only");
    // ray bounds (vr_set_ray_bounds; a pick launch ignores them): colour launches of one frame of the unlit shader and of the lit one
    // without shadows -- anything else is refused, never rendered with the occluder ignored
    R.bounded = (c->d_near || c->d_far) && R.pick_px[0] < 0;
    if (R.bounded && R.variant >= 0 && R.variant < VR_VARIANT_COUNT) {
        if (R.variant != VR_VARIANT_BASIC && R.variant != VR_VARIANT_LIGHT)
            return fail(c, VR_ERR_UNSUPPORTED, "vr_render: ray bounds exist for BASIC and LIGHT only");
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
    int ntf;
    variant_needs(R.variant, nvol, &ntf);
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

// What a launch could run, worked out once before the kernel choice (choose_flavour).
struct Eligibility {
    bool p2_ok;             // two steps ahead (16, 17) can run
    unsigned p2_lds;        // ... with this much dynamic LDS (TF slot 0 and the three axis tables)
    bool lut_ok;            // 18 can run
    unsigned lut_lds;       // ... with this much (the slot tables of volume 0)
    bool indexable;         // the skipping kernels can index volume 0's bricks (bricks_indexable): every skipping form needs it
    bool can_skip;          // exact empty-space skipping (prepare_skip)
    bool whole_frame;       // enough rays to fill the machine in one frame
    bool empty;             // the share holds no tile: nothing is launched
    unsigned chain_known;   // longest ray chain + 1 of the most recent launch of this scene shape whose sort has reported (0: none)
};

Eligibility eligibility(const vr_ctx* c, int requested, const RenderRequest& R)
{
    Eligibility E = {};
    // two steps ahead (16, 17; march_p2_kernel, vr_p2.h): lit / unlit shader and the three-volume composite (with its brick records:
    // choose_flavour); TF slot 0 (one resolution for both tables) and the three axis tables in LDS; the bricked copy with 32-bit slots,
    // rows and slabs of bricks below 2^24 slots; a volume of 4 GiB or more through a moving window of at least four z-slabs of bricks.
    // Launches of several frames and launches in flight included.
    const int sv = R.variant == VR_VARIANT_VOLUME_MASK ? 2 : 0;  // the volume whose density drives tf[0]'s opacity
    E.p2_ok = (R.variant == VR_VARIANT_LIGHT || R.variant == VR_VARIANT_BASIC || R.variant == VR_VARIANT_VOLUME_MASK) && tf0_fits_lds(c) &&
              c->layout_mode == 0 && c->vols[sv].bricked && c->vols[sv].bdens;
    if (E.p2_ok) {
        const DevVolume& v = c->vols[sv].vol;
        const BrickedGrid g = bricked_grid(v);
        const size_t slab = (size_t)g.nbx * g.nby * kVbN, window = R.variant == VR_VARIANT_BASIC ? 0x3fffffffull : 0x0fffffffull;
        const size_t lds = (size_t)(c->tf[0].dev.res_o + 2) * 16 + ((size_t)v.nx + v.ny + v.nz + 3) * 8;
        E.p2_ok = g.slots <= 0xFFFFFFFFull && slab < (1u << 24) && (c->p2_window ? c->p2_window / slab >= 3 : window / slab >= 4) && lds <= 160u * 1024u;
        E.p2_lds = (unsigned)lds;
    }
    // 18: march_kernel with the slot tables of volume 0 in its workgroup's LDS (make_cell_lut): the shaders that sample ONE volume, the
    // bricked copy with 32-bit slots
    E.lut_ok = (R.variant == VR_VARIANT_LIGHT || R.variant == VR_VARIANT_BASIC || R.variant == VR_VARIANT_LIGHT_INSHADER) && c->layout_mode == 0 &&
               c->vols[0].bricked && c->vols[0].bdens;
    if (E.lut_ok) {
        E.lut_lds = (unsigned)(((size_t)c->vols[0].vol.nx + c->vols[0].vol.ny + c->vols[0].vol.nz + 6) * 4);
        E.lut_ok = bricked_grid(c->vols[0].vol).slots <= 0xFFFFFFFFull && E.lut_lds <= 32u * 1024u;
    }
    // exact empty-space skipping: only for the shaders whose opacity is the CT table value alone, only when a zero-opacity sample is
    // provably the identity (finite colour table and light), and unless flavour 1 asks for the plain kernel (no rule of choose_flavour
    // turns another flavour into 1 or 1 into another)
    E.indexable = volume_bricks_indexable(c->vols[0].vol);
    E.can_skip = (R.variant == VR_VARIANT_BASIC || R.variant == VR_VARIANT_LIGHT || R.variant == VR_VARIANT_THREE_FILES ||
                  R.variant == VR_VARIANT_VOLUME_MASK || R.variant == VR_VARIANT_LIGHT_INSHADER) &&
                 requested != 1 && c->vols[sv].bricks && c->tf[0].zero_prefix >= 0 && c->tf[0].color_finite;
    for (int f = 0; f < R.n_frames; ++f) E.can_skip = E.can_skip && all_finite(R.batch_u ? R.batch_u[f].light_pos : c->u.light_pos, 12);
    // the kernels index bricks with 24-bit multiplies and 32-bit byte offsets
    E.can_skip = E.can_skip && volume_bricks_indexable(c->vols[sv].vol);
    if (R.variant == VR_VARIANT_THREE_FILES) E.can_skip = E.can_skip && c->tf[1].color_finite && c->tf[1].opacity_finite;
    if (R.variant == VR_VARIANT_VOLUME_MASK)  // mask and CT must share one grid so that one brick index serves both
        E.can_skip = E.can_skip && c->vols[0].bricks && c->vols[0].vol.nx == c->vols[2].vol.nx && c->vols[0].vol.ny == c->vols[2].vol.ny &&
                     c->vols[0].vol.nz == c->vols[2].vol.nz;
    E.whole_frame = rays_per_lane(c, R.rank, R.world, 1) >= 4.5;
    E.empty = tile_count(c, R.rank, R.world) == 0;
    E.chain_known = requested == 0 ? c->order.last_chain(scene_key(c, R, false, false)) : 0;  // (the plain colour launch's key, always)
    return E;
}

// The kernel form ("flavour") a launch runs: `fl` is the one asked for (vr_set_kernel_flavour, else VR_EXP_FLAVOUR), 0 = the default.
int choose_flavour(vr_ctx* c, int fl, const RenderRequest& R, const Eligibility& E)
{
    // The one-lane families come in pairs: 1 asks for the form without skipping (the odd flavour + 1), everything else runs as the
    // skipping one; nothing is measured.  The first row that applies decides (the isosurface's surface output keeps 21 / 22).
    const struct {
        bool applies;
        int skipping;
    } pairs[] = {
        {R.bounded, 27},                                              // the unlit / lit shader between ray bounds
        {R.surface && R.variant != VR_VARIANT_ISO, 25},               // the surface-position output of the unlit / lit shader
        {is_projection(R.variant), 19},                               // the projections
        {R.variant == VR_VARIANT_ISO, 21},                            // the isosurface
        {R.variant == VR_VARIANT_LIGHT && c->shadows.div != 0, 23},    // the shadowed lit shader
    };
    for (const auto& pr : pairs)
        if (pr.applies) return fl == 1 ? pr.skipping + 1 : pr.skipping;
    const bool auto_choice = fl == 0;
    const double rays = rays_per_lane(c, R.rank, R.world, c->frames_in_flight * R.n_frames);
    const bool short_chains = E.chain_known != 0 && E.chain_known - 1 < 128;
    if (auto_choice) {
        // Default: pick the lanes per ray from what will be on the machine.  With many rays per hardware lane the machine is
        // throughput-bound and one lane per ray does the least work; with few (a small frame, or one GPU's share of the
        // tiles) the frame waits for its longest rays, whose chains of dependent samples the depth-parallel kernel cuts to a
        // half or a quarter (vr_dp.h).  Two things refine the round-1 rule (thresholds measured on C3 at 1 / 2 / 4 / 8 ranks):
        //  * frames in flight: when the caller keeps several frames in flight on different streams (it says so with
        //    vr_hint_frames_in_flight; asking the events instead flushes the runtime's command batches and costs more than it
        //    tells) the other launches fill the machine as well, so the rays per lane count once per frame in flight (a
        //    rank's half of C3, two frames pipelined: 0.34 ms with one lane, 0.42 with two);
        //  * how long the chains really are (E.chain_known).  Chains too short to matter -- under 128 samples, 0.2 ms (C2: 102) --
        //    leave nothing for the depth-parallel kernels to cut (C2: 0.133 / 0.091 ms per frame with one lane, 0.153 / 0.123 with
        //    two), unless the launch is too small to fill the machine at all.
        // (two lanes per ray from 2 rays per lane on, four below: re-measured on the bricked layout -- a rank's quarter of C3
        // (1.6 rays per lane), one frame at a time: 0.274 ms with two lanes, 0.203 with four; a rank's half (3.2): 0.362 / 0.377;
        // a quarter with two launches in flight counts 3.2 and keeps two lanes: 0.190 / 0.217 per frame)
        fl = (rays >= 4.5 || (short_chains && rays >= 1.2)) ? 6 : (rays >= 2.0 ? 11 : 10);
    }
    // what a form runs as where it cannot run: persistent wavefronts (12, 13; vr_pw.h) exist for launches of one frame
    if ((fl == 12 || fl == 13) && R.n_frames != 1) fl = 6;
    if ((fl == 16 || fl == 17) && !E.p2_ok) fl = R.n_frames != 1 ? 6 : (fl == 16 ? 13 : 12);
    if (fl == 18 && !E.lut_ok) fl = 6;
    if (fl == 16 && R.variant == VR_VARIANT_VOLUME_MASK) fl = 17;  // (the composite's form is the skipping one: its mask records)
    // LDS tiles (15; vr_lt.h): the lit shader, launches of one frame
    if (fl == 15 && (R.n_frames != 1 || R.variant != VR_VARIANT_LIGHT)) fl = 6;
    // the illustrative shader's opacity reads the accumulated alpha: its steps cannot be sampled side by side
    if (R.variant == VR_VARIANT_ILLUSTRATIVE && (fl == 7 || fl == 8 || fl == 10 || fl == 11)) fl = 6;
    // the in-shader gradient variant (seven density fetches per sample) exists as the one-lane kernel only
    if (R.variant == VR_VARIANT_LIGHT_INSHADER && fl != 1 && fl != 12 && fl != 13 && fl != 18) fl = 6;
    if ((fl == 16 || fl == 17) && R.variant == VR_VARIANT_VOLUME_MASK && !E.can_skip)  // (no brick records: no on-demand mask fetch)
        fl = R.n_frames != 1 ? 6 : 12;
    if (!auto_choice) return fl;

    // Default choice, second part -- THE PRIOR: what runs before anything has been measured.  Whole frames of the lit / unlit shader
    // and of the composite, one launch at a time: the kernel with the corner loads two steps ahead (vr_p2.h) -- 17, or 16 where next to
    // nothing can be skipped (noisy air under the default ramp 2.95 -> 1.97 ms; C3 0.65 -> 0.51; C4 0.72 -> 0.57) -- unless an earlier
    // launch of this shape says its chains are short (C2, longest chain 102: a packet is too short for the pipeline's fill and a
    // dequeue, 0.111 -> 0.161).  The same with launches in flight and several frames per launch since the approach loop (C3 0.417 / 0.382
    // ms per frame against march_kernel's 0.464 / 0.445; C5 level); shares of a frame: the first part's choice.
    const bool p2_variant = R.variant == VR_VARIANT_LIGHT || R.variant == VR_VARIANT_BASIC || (R.variant == VR_VARIANT_VOLUME_MASK && E.can_skip);
    const bool nothing_to_skip = !E.can_skip || c->skip.active_fraction >= 0.9;  // (prepare_skip has measured the share of active bricks)
    if (fl == 6 && E.whole_frame && E.p2_ok && p2_variant) {
        if (nothing_to_skip && R.variant != VR_VARIANT_VOLUME_MASK) fl = 16;
        else if (!short_chains) fl = 17;
    }
    // (a share without a tile launches nothing and takes no launch number: a trial that counted it would name the next launch twice)
    if (!c->tuner.mode || E.empty) return fl;
    // ... and THE MEASURED CHOICE (tune_pick): the eligible forms take turns on the caller's own frames, the fastest by the launches'
    // own records stays.  Candidates: the prior; the two-steps-ahead kernel; the one-lane kernel; the depth-parallel kernel (launches
    // that leave the machine part empty) or the persistent kernel without the pipeline (the longest chains).
    int cand[6], n = 0;
    auto add = [&](int f) {
        for (int i = 0; i < n; ++i)
            if (cand[i] == f) return;
        if (n < 6) cand[n++] = f;
    };
    add(fl);
    if (E.p2_ok && p2_variant) add((nothing_to_skip && R.variant != VR_VARIANT_VOLUME_MASK) || !E.can_skip ? 16 : 17);
    add(6);
    if (E.lut_ok && E.lut_lds <= 8u * 1024u) add(18);  // (the one-lane kernel with its slot arithmetic from LDS tables; larger tables cost it wavefronts per CU: C5 4.2 vs 3.4 ms)
    const bool dp_variant = R.variant != VR_VARIANT_ILLUSTRATIVE && R.variant != VR_VARIANT_LIGHT_INSHADER;
    if (!E.whole_frame && dp_variant) add(rays >= 2.0 ? 11 : 10);
    else if (R.n_frames == 1 && (R.variant == VR_VARIANT_LIGHT || R.variant == VR_VARIANT_BASIC)) add(12);
    const unsigned long long shape = 0x9E3779B97F4A7C15ull * (((unsigned long long)R.variant << 56) ^ ((unsigned long long)R.world << 48) ^ ((unsigned long long)R.rank << 40) ^
                                                             ((unsigned long long)c->W << 24) ^ ((unsigned long long)c->H << 8) ^ (R.packed ? 0x80ull : 0ull) ^
                                                             ((unsigned long long)R.n_frames << 4) ^ (unsigned long long)c->frames_in_flight) | 1ull;
    const unsigned long long key = (shape ^ (c->brick_epoch * 0xD6E8FEB86659FD93ull) ^ (c->tf_epoch << 20) ^ ((unsigned long long)c->arith << 1) ^
                                    ((unsigned long long)c->layout_mode << 2)) | 1ull;
    const bool measurable = c->ring.h_span && c->ring.h_end && !c->event_timing;
    return tune_pick(c->tuner, RingRecords{c->ring}, c->last.ring_head, c->frames_in_flight, key, shape, cand, n, E.chain_known, measurable);
}

// What each flavour launches -- the one place a flavour's number is decoded.
struct KernelForm {
    LaunchDesc::Family family;
    int lanes;            // kDp: lanes per ray (vr_dp.h): 64 / 32 workgroups per tile
    bool pipe;            // kDp / kPw: the next round's / step's corner loads software-pipelined
    bool skip;            // the skipping flavour of a pair (17 of 16 / 17; 19, 21, 23, 25, 27 of the one-lane families): LaunchDesc::skip once
                          // its records are in place
    bool lut;             // kPlain: the slot tables of volume 0 in LDS
    unsigned pw_threads;  // kPw / kP2: threads per workgroup
    // what follows from the family
    bool range_records() const { return family == LaunchDesc::kProj || family == LaunchDesc::kIso; }  // skips by prepare_proj's records
    bool measured() const  // a candidate of the measured choice (the one-lane families never are)
    {
        return !(range_records() || family == LaunchDesc::kShadow || family == LaunchDesc::kSurf || family == LaunchDesc::kBound);
    }
};

KernelForm kernel_form(int fl, int variant)
{
    // (march_p2_kernel: two corner buffers, 3 wavefronts per SIMD at most; with every ray sampling all the time two per SIMD are faster
    // -- the corner data in flight is many times the L1 either way: noisy air 2.13 -> 2.04 ms.  The unlit shader's two buffers are 4-byte
    // densities, 101 VGPRs: 4 wavefronts per SIMD -- C2 one frame at a time 0.121 -> 0.113 ms, thin table 0.255 -> 0.239, four frames per
    // launch 0.070 -> 0.061: tools/experiments/s2h.sh.  Launches in flight: the same shape.  Two workgroups of 6 wavefronts do not share
    // a CU -- the second one's wavefronts would have to go 1-1-2-2 over the SIMDs where the dispatcher deals 2-2-1-1: measured 0.75 ms
    // per C3 frame, what one such workgroup per CU takes -- and two of 4 run at 8 wavefronts per CU: 0.63 against 0.54; three of 4, the
    // same 12 wavefronts per CU, take 0.79 ms one frame at a time and 0.62 in flight against 0.55 / 0.51: profiles/r04_p2_launch_shapes.txt)
    using D = LaunchDesc;
    switch (fl) {
    case 7: return {D::kDp, 4, false, false, false, 0u};
    case 8: return {D::kDp, 2, false, false, false, 0u};
    case 10: return {D::kDp, 4, true, false, false, 0u};
    case 11: return {D::kDp, 2, true, false, false, 0u};
    case 12: return {D::kPw, 0, false, false, false, 1024u};
    case 13: return {D::kPw, 0, true, false, false, 1024u};
    case 15: return {D::kLt, 0, false, false, false, 0u};
    case 16: return {D::kP2, 0, false, false, false, 512u};
    case 17: return {D::kP2, 0, false, true, false, variant == VR_VARIANT_BASIC ? 1024u : 768u};
    case 18: return {D::kPlain, 0, false, false, true, 0u};
    case 19:
    case 20: return {D::kProj, 0, false, fl == 19, false, 0u};
    case 21:
    case 22: return {D::kIso, 0, false, fl == 21, false, 0u};
    case 23:
    case 24: return {D::kShadow, 0, false, fl == 23, false, 0u};
    case 25:
    case 26: return {D::kSurf, 0, false, fl == 25, false, 0u};
    case 27:
    case 28: return {D::kBound, 0, false, fl == 27, false, 0u};
    default: return {D::kPlain, 0, false, false, false, 0u};  // 1, 6
    }
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
    Eligibility E = eligibility(c, requested, R);
    if (R.surface && R.variant != VR_VARIANT_ISO) {
        // The surface march skips by the distance field of BASIC / LIGHT under the weakest condition that is still exact: an inert
        // brick's samples have opacity exactly 0, which leaves the accumulated alpha as it is whatever the colour table and the
        // light hold -- neither is read.  So: the brick records, a zero prefix of the opacity table, the kernels' index range.
        E.can_skip = requested != 1 && c->vols[0].bricks && c->tf[0].zero_prefix >= 0 && E.indexable;
        E.chain_known = 0;
    }
    if (E.can_skip) {
        if (const int rc = prepare_skip(c, R.variant, s, P)) return rc;
        if (c->skip.pending) ++c->skip.unbounded_launches;
    }
    const int fl = choose_flavour(c, requested, R, E);
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
    if (form.family == LaunchDesc::kBound) {  // the depth buffers, in the slots these shaders do not sample (vr_bound.h)
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
        // the LOGICAL blocks (records, launch order): one wavefront per workgroup (launch order at wavefront granularity) -- except
        // for the depth-parallel kernels on large launches, where 4x the workgroups cost more at dispatch than the finer order gains
        // (C2: 32 768 workgroups of a 0.12 ms frame).  See map_pixel / map_pixel_dp.
        const int dp = form.family == LaunchDesc::kDp ? form.lanes : 0, wpb = dp && P.n_tiles * dp * 64 > 16384 ? 4 : 1;
        const dim3 block((unsigned)(64 * wpb));
        const dim3 grid((unsigned)(dp ? P.n_tiles * dp * 64 / wpb : (P.n_tiles + 7) / 8 * 8 * (64 / wpb)));
        if (R.n_frames > 1 && grid.x % 8u != 0) return fail(c, VR_ERR_INVALID_ARG, "vr_render: launch shape cannot carry several frames");
        const bool pw = form.family == LaunchDesc::kPw || form.family == LaunchDesc::kP2;
        // the ring slots: record buffer, then the launch order and the sort waits (a launch order is kept per launch shape -- not per
        // flavour: the kernels that march one packet per wavefront -- 6, 12, 13, 16, 17 -- share the logical blocks, so an order sorted
        // behind one of them serves the others, and the measured choice tries them in turn on a live scene)
        int cb;
        const OrderSlot* slot_sort;
        if (const int rc = claim_slot(c, s, &cb, &slot_sort)) return rc;
        if (const int rc = reserve_block_counts(c, s, cb, (size_t)grid.x * (size_t)R.n_frames, &slot_sort)) return rc;
        P.block_counts = c->slot[cb].block_counts;
        c->last.cnt_buf = cb;
        const unsigned long long okey = ((unsigned long long)grid.x << 32) ^ ((unsigned long long)block.x << 20) ^
                                        ((unsigned long long)(R.variant | (R.surface ? 0x10 : 0) | (R.bounded ? 0x20 : 0)) << 16) ^ ((unsigned long long)R.world << 8) ^
                                        (unsigned long long)R.rank ^ (R.packed ? 1ull << 63 : 0ull);
        const bool ordered = grid.x <= (unsigned)kOrderMaxBlocks && grid.x % 8u == 0;
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
        L.lds_bytes = P.vol[0].lut ? E.lut_lds : 0u;
        L.grid = dim3(grid.x * (unsigned)R.n_frames);
        L.block = block;
        L.vrange = vrange;
        L.skip = skip;
        L.surface = R.surface;
        if (pw) {
            // persistent wavefronts: `grid` stays the number of LOGICAL blocks (records, launch order); the launch itself is one
            // workgroup of form.pw_threads per CU (fewer when there are fewer packets), TF slot 0 in LDS when it fits
            const bool p2 = form.family == LaunchDesc::kP2;
            const unsigned per_wg = form.pw_threads / 64u, wgs = (grid.x * (unsigned)R.n_frames + per_wg - 1u) / per_wg;
            L.ltf = tf0_fits_lds(c);
            L.p2_win = p2 && (!off32 || c->p2_window != 0);
            L.lds_bytes = p2 ? E.p2_lds : (L.ltf ? (unsigned)(c->tf[0].dev.res_o + 2) * 16u : 0u);
            L.queue = PwQueue{c->d_pw_heads + (size_t)cb * 8 * 64, grid.x, c->p2_window};
            L.grid = dim3(wgs < (unsigned)c->n_cus ? wgs : (unsigned)c->n_cus);
            L.block = dim3(form.pw_threads);
            if (c->slot[cb].pw_heads_dirty) VR_HIP(c, hipMemsetAsync(L.queue.heads, 0, 8 * 64 * sizeof(unsigned), s));
            c->slot[cb].pw_heads_dirty = true;  // (until the sort that clears them behind this launch has really been enqueued)
        }
        if (c->arith == VR_ARITH_FUSED) vrf::launch_march(L, s, B);
        else vr::launch_march(L, s, B);
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
    int nvol, ntf;
    variant_needs(variant, &nvol, &ntf);
    for (int i = 0; i < nvol; ++i)
        if (!c->vols[i].vol.data) return fail(c, VR_ERR_NOT_READY, "vr_skip_field: volume slot " + std::to_string(i) + " is empty");
    for (int i = 0; i < ntf; ++i)
        if (!c->tf[i].dev.opacity || !c->tf[i].dev.color) return fail(c, VR_ERR_NOT_READY, "vr_skip_field: TF slot " + std::to_string(i) + " is empty");
    if (const int rc = drain(c)) return rc;
    (void)hipGetLastError();
    const Eligibility E = eligibility(c, 0, render_request(c, variant, 0, 1, false, nullptr, nullptr));
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
