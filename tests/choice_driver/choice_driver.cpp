// choice_driver.cpp -- the kernel choice (csrc/vr_choice.h) on the CPU, for tests/test_choice.py: eligibility, the prior and the
// candidates, the decoding of a flavour and the launch shape as functions of invented facts, and the sweep over all of them.
// Plain C++, no HIP: built with g++ into tests/_build/.
//
// The facts cross the C boundary as a struct of ints and doubles (CdFacts) that the test mirrors with ctypes; cd_run does what
// enqueue_render does between check_render_args and the launch: eligibility, choose_flavour, kernel_form and launch_shape of what the
// prior picks and of every candidate.
#include "vr_choice.h"

#include <cstdio>
#include <cstring>

using namespace vr;

extern "C" {

struct CdFacts {
    int variant, rank, world, n_frames, packed, surface, bounded;
    int vol[VR_MAX_VOLUMES][6];  // nx, ny, nz, bricked copy, its density plane, brick records
    int tf[VR_MAX_TFS][5];       // res_o, res_c, zero_prefix, color_finite, opacity_finite
    int layout_mode;
    unsigned p2_window;
    int n_cus;
    unsigned W, H;
    int frames_in_flight, shadows, lights_finite;
    double active_fraction;
    int tuner_mode;
    unsigned last_chain;
    unsigned long long brick_epoch, tf_epoch;
    int arith;
};

struct CdForm {
    int family, lanes, pipe, skip, lut;
    unsigned pw_threads;
    int measured, range_records;
};

struct CdShape {
    int wpb;
    unsigned blocks, block, grid;
    int ordered, pw, ltf, p2_win;
    unsigned lds_bytes;
};

struct CdOut {
    int p2_ok;
    unsigned p2_lds;
    int lut_ok;
    unsigned lut_lds;
    int indexable, can_skip, whole_frame, empty;
    unsigned chain_known;
    int prior, tune, n, cand[6];
    unsigned long long shape, key;
};

}  // extern "C"

namespace {

ChoiceFacts facts_of(const CdFacts& f)
{
    ChoiceFacts F = {};
    F.variant = f.variant, F.rank = f.rank, F.world = f.world, F.n_frames = f.n_frames;
    F.packed = f.packed != 0, F.surface = f.surface != 0, F.bounded = f.bounded != 0;
    for (int i = 0; i < VR_MAX_VOLUMES; ++i) F.vols[i] = {f.vol[i][0], f.vol[i][1], f.vol[i][2], f.vol[i][3] != 0, f.vol[i][4] != 0, f.vol[i][5] != 0};
    for (int i = 0; i < VR_MAX_TFS; ++i) F.tf[i] = {f.tf[i][0], f.tf[i][1], f.tf[i][2], f.tf[i][3] != 0, f.tf[i][4] != 0};
    F.layout_mode = f.layout_mode, F.p2_window = f.p2_window, F.n_cus = f.n_cus, F.W = f.W, F.H = f.H;
    F.frames_in_flight = f.frames_in_flight, F.shadows = f.shadows != 0, F.lights_finite = f.lights_finite != 0;
    F.active_fraction = f.active_fraction, F.tuner_mode = f.tuner_mode, F.last_chain = f.last_chain;
    F.brick_epoch = f.brick_epoch, F.tf_epoch = f.tf_epoch, F.arith = f.arith;
    return F;
}

// what enqueue_render works out before it decodes the flavour
void run(const ChoiceFacts& F, int requested, Eligibility* E, Choice* C)
{
    *E = eligibility(F, requested);
    *C = choose_flavour(F, requested, *E);
}

CdForm form_of(const KernelForm& k) { return {(int)k.family, k.lanes, k.pipe, k.skip, k.lut, k.pw_threads, k.measured(), k.range_records()}; }

CdShape shape_of(const LaunchShape& s) { return {s.wpb, s.blocks, s.block, s.grid, s.ordered, s.pw, s.ltf, s.p2_win, s.lds_bytes}; }

// ---- the sweep ------------------------------------------------------------------------------------------------------------------------
// Every variant x every requested flavour 0 .. 30 x a grid of the facts with a point on either side of every threshold of the rules.

struct VolCase {
    int dims[VR_MAX_VOLUMES][3];
    int have[VR_MAX_VOLUMES][3];  // bricked copy, its density plane, brick records
    int layout;
    unsigned p2_window;
};
struct TfCase {
    int t[VR_MAX_TFS][5];
};
struct ShareCase {
    unsigned W, H;
    int rank, world, n_cus;
};

#define ALL {1, 1, 1}, {1, 1, 1}, {1, 1, 1}
#define CUBE(n) {n, n, n}, {n, n, n}, {n, n, n}
const VolCase kVols[] = {
    {{CUBE(256)}, {ALL}, 0, 0},
    {{CUBE(256)}, {ALL}, 1, 0},                                         // not the bricked layout
    {{CUBE(256)}, {{0, 1, 1}, {1, 1, 1}, {0, 1, 1}}, 0, 0},             // no bricked copy
    {{CUBE(256)}, {{1, 0, 1}, {1, 1, 1}, {1, 0, 1}}, 0, 0},             // no density plane of it
    {{CUBE(256)}, {{1, 1, 0}, {1, 1, 1}, {1, 1, 1}}, 0, 0},             // no brick records of volume 0
    {{CUBE(256)}, {{1, 1, 1}, {1, 1, 1}, {1, 1, 0}}, 0, 0},             // ... of volume 2
    {{{256, 256, 256}, {256, 256, 256}, {256, 256, 252}}, {ALL}, 0, 0},  // the composite's grids differ
    {{{2048, 2048, 64}, {2048, 2048, 64}, {2048, 2048, 64}}, {ALL}, 0, 0},  // a slab of 2^24 slots
    {{{2048, 2044, 64}, {2048, 2044, 64}, {2048, 2044, 64}}, {ALL}, 0, 0},  // ... just below
    {{{1024, 1024, 1024}, {1024, 1024, 1024}, {1024, 1024, 1024}}, {ALL}, 0, 0},  // slab 2^22: the lit window holds 63 slabs, the unlit 255
    {{{2048, 2000, 64}, {2048, 2000, 64}, {2048, 2000, 64}}, {ALL}, 0, 0},  // slab 16 384 000: window / slab = 16 (lit), 65 (unlit)
    {{CUBE(256)}, {ALL}, 0, 3u * 262144u},                              // p2_window / slab = 3 (slab: 64 x 64 bricks x 64)
    {{CUBE(256)}, {ALL}, 0, 3u * 262144u - 1u},                         // ... = 2
    {{{680, 680, 682}, {680, 680, 682}, {680, 680, 682}}, {ALL}, 0, 0},  // slot tables of 8 192 bytes
    {{{680, 680, 683}, {680, 680, 683}, {680, 680, 683}}, {ALL}, 0, 0},  // ... 8 196
    {{{2728, 2728, 2730}, {2728, 2728, 2730}, {2728, 2728, 2730}}, {ALL}, 0, 0},  // ... 32 768 (and more than 2^32 slots)
    {{{8000, 186, 4}, {8000, 186, 4}, {8000, 186, 4}}, {ALL}, 0, 0},    // ... 32 784
    {{{8000, 182, 4}, {8000, 182, 4}, {8000, 182, 4}}, {ALL}, 0, 0},    // ... 32 768, few slots
    {{{1, 8196, 16384}, {1, 8196, 16384}, {1, 8196, 16384}}, {ALL}, 0, 0},  // bricks beyond the index limit
    {{{1, 8192, 16384}, {1, 8192, 16384}, {1, 8192, 16384}}, {ALL}, 0, 0},  // ... the last shape inside
    {{{1, 8196, 16384}, {256, 256, 256}, {256, 256, 256}}, {ALL}, 0, 0},  // ... volume 0 alone beyond it
    {{{19953, 4, 4}, {19953, 4, 4}, {19953, 4, 4}}, {ALL}, 0, 0},       // a 256-texel table and the axis tables: 160 KiB of LDS
    {{{19954, 4, 4}, {19954, 4, 4}, {19954, 4, 4}}, {ALL}, 0, 0},       // ... and 8 bytes
};
#define TF_OK {256, 256, 3, 1, 1}
const TfCase kTfs[] = {
    {{TF_OK, TF_OK}},
    {{{8190, 8190, 3, 1, 1}, TF_OK}},
    {{{8191, 8191, 3, 1, 1}, TF_OK}},
    {{{256, 128, 3, 1, 1}, TF_OK}},   // unequal resolutions
    {{{256, 256, -1, 1, 1}, TF_OK}},  // no zero prefix
    {{{256, 256, 0, 1, 1}, TF_OK}},
    {{{256, 256, 3, 0, 1}, TF_OK}},   // colour table not finite
    {{{256, 256, 3, 1, 0}, TF_OK}},   // (slot 0's opacity flag is read by nobody)
    {{TF_OK, {256, 256, 3, 0, 1}}},   // THREE_FILES' second table
    {{TF_OK, {256, 256, 3, 1, 0}}},
};
// 256 CUs: 327 680 hardware lanes, a tile is 4096 rays: 360 tiles are 4.5 rays per lane, 160 are 2.0, 96 are 1.2
const ShareCase kShares[] = {
    {64 * 360, 64, 0, 1, 256}, {64 * 359, 64, 0, 1, 256}, {64 * 160, 64, 0, 1, 256}, {64 * 159, 64, 0, 1, 256}, {64 * 96, 64, 0, 1, 256},
    {64 * 95, 64, 0, 1, 256},  {64 * 180, 64, 0, 1, 256}, {64 * 80, 64, 0, 1, 256},  {64 * 48, 64, 0, 1, 256},  {64 * 720, 64, 1, 2, 256},
    {1920, 1080, 0, 1, 256},   {1920, 1080, 3, 8, 256},   {64, 64, 1, 2, 256},       {100, 70, 3, 4, 256},      {1920, 1080, 0, 1, 64},
    // 16 384 workgroups of one wavefront: 64 tiles with four lanes per ray, 128 with two
    {64 * 64, 64, 0, 1, 256},  {64 * 65, 64, 0, 1, 256},  {64 * 128, 64, 0, 1, 256}, {64 * 129, 64, 0, 1, 256},
};
const unsigned kChains[] = {0, 128, 129, 4000};

struct Sweep {
    unsigned long long rows = 0, hash = 1469598103934665603ull;
    FILE* rows_to = nullptr;
    void word(unsigned long long v)
    {
        hash = (hash ^ v) * 1099511628211ull;
        hash ^= hash >> 29;
        if (rows_to) fprintf(rows_to, " %llx", v);
    }
    // one point: everything the launch path would work out from it
    void point(const ChoiceFacts& F, int requested)
    {
        Eligibility E;
        Choice C;
        run(F, requested, &E, &C);
        ++rows;
        word(E.p2_ok), word(E.p2_lds), word(E.lut_ok), word(E.lut_lds), word(E.indexable), word(E.can_skip), word(E.whole_frame), word(E.empty);
        word(E.chain_known), word((unsigned)C.prior), word(C.tune), word((unsigned)C.n), word(C.shape), word(C.key);
        for (int i = -1; i < C.n; ++i) {
            const int fl = i < 0 ? C.prior : C.cand[i];
            const KernelForm k = kernel_form(fl, F.variant);
            word((unsigned)fl), word(k.family), word((unsigned)k.lanes), word(k.pipe), word(k.skip), word(k.lut), word(k.pw_threads), word(k.measured());
            for (int off32 = 0; off32 < 2; ++off32) {
                const LaunchShape s = launch_shape(k, F, E, off32 != 0, k.lut);
                word((unsigned)s.wpb), word(s.blocks), word(s.block), word(s.grid), word(s.ordered), word(s.pw), word(s.ltf), word(s.p2_win), word(s.lds_bytes);
            }
        }
        if (rows_to) fprintf(rows_to, "\n");
    }
};

ChoiceFacts base_facts(int variant)
{
    ChoiceFacts F = {};
    F.variant = variant, F.world = 1, F.n_frames = 1, F.n_cus = 256, F.frames_in_flight = 1;
    F.lights_finite = true, F.active_fraction = 0.5, F.tuner_mode = 1;
    F.brick_epoch = 7, F.tf_epoch = 11;
    return F;
}
void set_vol(ChoiceFacts& F, const VolCase& v)
{
    for (int i = 0; i < VR_MAX_VOLUMES; ++i) F.vols[i] = {v.dims[i][0], v.dims[i][1], v.dims[i][2], v.have[i][0] != 0, v.have[i][1] != 0, v.have[i][2] != 0};
    F.layout_mode = v.layout, F.p2_window = v.p2_window;
}
void set_tf(ChoiceFacts& F, const TfCase& t)
{
    for (int i = 0; i < VR_MAX_TFS; ++i) F.tf[i] = {t.t[i][0], t.t[i][1], t.t[i][2], t.t[i][3] != 0, t.t[i][4] != 0};
}
void set_share(ChoiceFacts& F, const ShareCase& s) { F.W = s.W, F.H = s.H, F.rank = s.rank, F.world = s.world, F.n_cus = s.n_cus; }

// the points of (variant, requested): the launch facts crossed over a few scenes, then the scenes crossed over a few launches
template <class Visit>
void sweep_block(int variant, int requested, Visit&& visit)
{
    const int scenes[] = {0, 1, 4, 6, 14};  // of kVols (with kTfs[0] and, the third one, without a zero prefix)
    const struct {
        bool shadows;
        double active;
    } skips[] = {{false, 0.5}, {false, 0.9}, {false, 0.8999999}, {true, 0.5}};
    ChoiceFacts F = base_facts(variant);
    for (int kind = 0; kind < 3; ++kind)  // colour, surface, between ray bounds
        for (int frames = 1; frames <= 2; ++frames)
            for (int in_flight = 1; in_flight <= 2; ++in_flight)
                for (const auto& sh : kShares)
                    for (unsigned chain : kChains)
                        for (const auto& sk : skips)
                            for (int sc = 0; sc < 5; ++sc) {
                                    F.surface = kind == 1, F.bounded = kind == 2, F.n_frames = frames, F.frames_in_flight = in_flight;
                                    set_share(F, sh);
                                    F.last_chain = chain, F.shadows = sk.shadows, F.active_fraction = sk.active;
                                    set_vol(F, kVols[scenes[sc]]);
                                    set_tf(F, kTfs[sc == 2 ? 4 : 0]);
                                    F.packed = sh.world > 1, F.tuner_mode = 1, F.lights_finite = true, F.arith = 0;
                                    visit(F, requested);
                                }
    F = base_facts(variant);
    for (const auto& v : kVols)
        for (const auto& t : kTfs)
            for (int lights = 0; lights < 2; ++lights)
                for (int tune = 0; tune < 2; ++tune)
                    for (int launch = 0; launch < 6; ++launch) {
                        set_vol(F, v);
                        set_tf(F, t);
                        set_share(F, kShares[launch < 3 ? 0 : 3]);
                        F.n_frames = launch % 3 == 1 ? 2 : 1, F.frames_in_flight = launch % 3 == 2 ? 2 : 1;
                        F.lights_finite = lights != 0, F.tuner_mode = tune, F.arith = tune, F.last_chain = 0, F.active_fraction = 0.95;
                        visit(F, requested);
                    }
}

}  // namespace

extern "C" {

int cd_variants(void) { return VR_VARIANT_COUNT; }

// row `variant` of the traits table: nvol, ntf, projection, surface, bounds, skip_vol, forms
void cd_traits(int variant, int out[7])
{
    const ShaderTraits& T = kShader[variant];
    const int row[7] = {T.nvol, T.ntf, T.projection, T.surface, T.bounds, T.skip_vol, (int)T.forms};
    std::memcpy(out, row, sizeof row);
}
int cd_flavour_settable(int fl) { return flavour_in_range(fl) && !removed_flavour(fl); }
int cd_form_exists(int fl, int variant, int surface) { return form_exists(kernel_form(fl, variant), variant, surface != 0); }

// The soundness sweep: at every point that check_render_args lets through, does a kernel exist (form_exists: the table that vr_launch.h
// instantiates from) for what the prior picks and for every candidate?  Returns the number of points checked; *bad = how many failed,
// first[4] = variant, requested, flavour, index of the point in its block of the first of them.  A requested flavour that no caller
// can set (flavour_in_range, removed_flavour) is swept all the same and counted apart, in *bad_unsettable: 19 .. 28 name the one-lane
// families' kernels and pass through choose_flavour as they are, whatever the shader.
unsigned long long cd_soundness(unsigned long long* bad, int first[4], unsigned long long* bad_unsettable)
{
    unsigned long long total = 0;
    *bad = *bad_unsettable = 0;
    for (int variant = 0; variant < VR_VARIANT_COUNT; ++variant)
        for (int requested = 0; requested <= 30; ++requested) {
            int index = 0;
            sweep_block(variant, requested, [&](const ChoiceFacts& F, int r) {
                ++index;
                const ShaderTraits& T = kShader[F.variant];
                // (what check_render_args refuses is never chosen for)
                if ((F.surface && !T.surface) || (F.bounded && (!T.bounds || F.surface || (F.variant == VR_VARIANT_LIGHT && F.shadows) || F.n_frames > 1)))
                    return;
                Eligibility E;
                Choice C;
                run(F, r, &E, &C);
                ++total;
                for (int i = -1; i < C.n; ++i) {
                    const int fl = i < 0 ? C.prior : C.cand[i];
                    const KernelForm k = kernel_form(fl, F.variant);
                    // a candidate is one of the measured families, and the trial may run it in place of the prior
                    const bool ok = form_exists(k, F.variant, F.surface) && (i < 0 || k.measured()) && (!C.tune || kernel_form(C.prior, F.variant).measured());
                    if (ok) continue;
                    if (!flavour_in_range(r) || removed_flavour(r)) ++*bad_unsettable;
                    else if ((*bad)++ == 0) first[0] = variant, first[1] = r, first[2] = fl, first[3] = index - 1;
                }
            });
        }
    return total;
}
int cd_order_max_blocks(void) { return kOrderMaxBlocks; }

void cd_run(const CdFacts* f, int requested, CdOut* o)
{
    Eligibility E;
    Choice C;
    run(facts_of(*f), requested, &E, &C);
    *o = {E.p2_ok, E.p2_lds, E.lut_ok, E.lut_lds, E.indexable, E.can_skip, E.whole_frame, E.empty, E.chain_known, C.prior, C.tune, C.n, {}, C.shape, C.key};
    std::memcpy(o->cand, C.cand, sizeof C.cand);
}

void cd_form(int fl, int variant, CdForm* o) { *o = form_of(kernel_form(fl, variant)); }

// the shape of a launch of flavour fl (off32: every volume below 4 GiB)
void cd_shape(const CdFacts* f, int requested, int fl, int off32, CdShape* o)
{
    const ChoiceFacts F = facts_of(*f);
    const KernelForm k = kernel_form(fl, F.variant);
    *o = shape_of(launch_shape(k, F, eligibility(F, requested), off32 != 0, k.lut));
}

// lights: n frames of 12 floats (Light.Position, ambient, diffuse)
int cd_lights_finite(const float* lights, int n)
{
    vr_uniforms u[4] = {};
    for (int f = 0; f < n && f < 4; ++f) std::memcpy(u[f].light_pos, lights + 12 * f, 12 * sizeof(float));
    return lights_finite(u, n);
}

int cd_tile_count(unsigned W, unsigned H, int rank, int world) { return tile_count(W, H, rank, world); }
int cd_skip_indexable(int nx, int ny, int nz) { return volume_bricks_indexable(nx, ny, nz); }
unsigned long long cd_bricked_slots(int nx, int ny, int nz) { return bricked_grid(nx, ny, nz).slots; }

// The sweep as a dump: one line per (variant, requested) with the number of points and a hash of everything worked out at them; the
// rows themselves as well when rows_of_variant / rows_of_requested name a block.  Returns the number of points.
unsigned long long cd_dump(const char* path, int rows_of_variant, int rows_of_requested)
{
    FILE* out = fopen(path, "w");
    if (!out) return 0;
    unsigned long long total = 0;
    for (int variant = 0; variant < VR_VARIANT_COUNT; ++variant)
        for (int requested = 0; requested <= 30; ++requested) {
            Sweep s;
            if (variant == rows_of_variant && requested == rows_of_requested) s.rows_to = out;
            sweep_block(variant, requested, [&](const ChoiceFacts& F, int r) { s.point(F, r); });
            fprintf(out, "variant %d requested %d: %llu points, hash %016llx\n", variant, requested, s.rows, s.hash);
            total += s.rows;
        }
    fclose(out);
    return total;
}

}  // extern "C"
