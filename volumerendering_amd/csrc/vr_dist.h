// vr_dist.h -- exact signed distance maps of a mask contour on the device (vr_mask_distance, include/vr.h): the Euclidean distance
// transform of one contour of a mask slot, restricted to a box, on an anisotropic grid with integer spacings, written as f32 into one
// component of a volume slot.  Exact integer arithmetic up to the final square root: nothing can be fused, so vr_set_arithmetic plays no
// part and the kernels are compiled once, included by vr_api.hip alone.  The bit-rows, their pack and the box walk are vr_bitrows.h's.
//
// The transform is separable: D2(p) = min over y' of ((y - y') sy)^2 + [min over x' of ((x - x') sx)^2 in row y'], and the same once
// more along z.  A FIELD is one uint64_t per voxel of a region of the box (DistField), kDistNone where no source voxel has been met.
//
// x pass (dist_x_kernel): from the bit-rows bit_pack_kernel packed.  Persistent workgroups of four wavefronts, one wavefront per word
// of the region, one lane per voxel.  The nearest set bit at or left of a lane and at or right of it come from clz / ffs on the lane's
// own word; where the word has none on that side, from the nearest non-empty word of the row, which the wavefront looks for once for
// all its lanes (uniform loads).  The lane stores ((distance in voxels) * sx)^2, or kDistNone for a row without a set bit.  COMP: the
// source is the box's complement (~w within the region), which gives the INSIDE field -- the pattern of morph_dilate_kernel<COMP>.
//
// y and z passes (dist_line_kernel): the lower envelope of the parabolas f_i(u) = ((u - i) s)^2 + g(i) over the integers, Meijster's
// two scans, in place.  One lane per line, neighbouring lanes along x, so that every load and store of a wavefront is one run of 512
// bytes.  The forward scan keeps a stack of (apex i, g(i), first index t from which parabola i is the lowest); its top lives in
// registers, the rest in global scratch interleaved by lane (entry q of lane t at [q * lanes + t]).  Two parabolas i < u meet at
// Sep = floor((s^2 (u^2 - i^2) + g(u) - g(i)) / (2 s^2 (u - i))): with extent * spacing <= 2^30 per axis (checked by the host) every g
// is below 2^62, (s u)^2 below 2^60, and numerator and denominator fit int64_t.  Lines hold no parabola where g is kDistNone; a line
// without any keeps kDistNone.  The backward scan reads the stack alone, which is why the pass can write the line it read.
//
// Write (dist_write_kernel): the launch shape of morph_write_kernel, one wavefront per word of the box, one lane per voxel, ONE load of
// the field the voxel's value comes from, one 4-byte vector store into component dst_channel.  The limit, the square root, the scale
// and the sign are applied here.  The voxels that store BEYOND's value and the probe's count, minimum and maximum of D2out are added up
// per lane, folded across the wavefront once behind the loop and reported with one atomic each per wavefront.
//
// No kernel waits for another workgroup and nothing spins: the launch boundaries are the visibility points.
#pragma once
#include "vr_bitrows.h"

namespace vr {

// The device words of one vr_mask_distance: set by the host before the first kernel, read behind the packs and the write.
struct DistWords {
    CountBox src;    // |A'| and its bounding box, from the pack (starts as CountBox::empty())
    CountBox probe;  // where the probe's pack reports (only its packed bits are used)
    unsigned long long beyond;                           // voxels of the box that store BEYOND's value
    unsigned long long probe_voxels, probe_min, probe_max;  // of D2out over the probe (min starts as ~0, max as 0)
};

// One squared-distance field of a vr_mask_distance: uint64_t per voxel of a REGION of the box, x fastest, kDistNone = no source.
struct DistField {
    unsigned long long* d2;
    int lo[3], n[3];  // the region: first voxel and extent per axis (some n == 0: empty, nothing was computed)
};
// The x pass over the words of a field's region: from the bit-rows `bits` into F.d2.
struct DistXPass {
    const unsigned long long* bits;  // the packed operand A'
    DistField F;
    int ny, wx;                      // rows per slice and words per row of the bit-rows
    int rw0, rw;                     // the words of a row that meet the region: the first and their number ...
    unsigned long long words;        // ... and rw * rows * slices of the region
    unsigned long long spacing;      // of x
};
// One envelope pass along y or z: lane t works the line d2[(t / inner) * outer + t % inner + i * stride], i < n.
struct DistLine {
    unsigned long long* d2;
    unsigned long long lanes, inner, outer, stride;
    int n;
    unsigned long long spacing;      // of the line's axis
    unsigned long long* stack_g;     // the envelope's stacks, entry q of lane t at [q * lanes + t]: a parabola's g ...
    unsigned* stack_st;              // ... and its apex s | the first index t where it is the lowest << 16
};
// Kernel argument block of the write of a vr_mask_distance (vr_dist_desc of include/vr.h): passed by value.
struct DistParams {
    BitRows b;                        // the volume, the box and its words
    const unsigned long long* a;      // the packed operand A'
    const unsigned long long* probe;  // the packed probe, nullptr = none
    float4* dst;                      // the destination slot's x-fastest vec4 voxels ...
    int dst_channel;                  // ... and the component the distances go into
    DistField out, in;                // D2out and D2in (a field the mode does not need is empty and not read)
    int mode;                         // VR_DIST_OUTSIDE ..
    unsigned long long limit_sq;      // 0 = no limit
    float scale, beyond_value;        // (float)L * scale, or +inf
    DistWords* w;
};

constexpr unsigned long long kDistNone = ~0ull;  // no source voxel: BEYOND

__device__ __forceinline__ unsigned long long dist_sq(long long d) { return (unsigned long long)(d * d); }  // (|d| <= 2^30)

__device__ __forceinline__ unsigned long long wave_min_u64(unsigned long long v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const unsigned long long o = __shfl_down(v, off, 64);  // (every lane takes part; lane 0 holds the result)
        v = o < v ? o : v;
    }
    return v;
}
__device__ __forceinline__ unsigned long long wave_max_u64(unsigned long long v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const unsigned long long o = __shfl_down(v, off, 64);
        v = o > v ? o : v;
    }
    return v;
}

// the source bits of word xw of a row within the field's region along x; COMP: of the complement
template <bool COMP>
__device__ __forceinline__ unsigned long long dist_src_word(const DistXPass& X, const unsigned long long* row, int xw)
{
    const unsigned long long w = row[xw];
    return (COMP ? ~w : w) & bit_xmask(xw, X.F.lo[0], X.F.lo[0] + X.F.n[0]);
}

template <bool COMP>
__global__ __launch_bounds__(256) void dist_x_kernel(const DistXPass X)
{
    const unsigned lane = threadIdx.x & 63u;
    const unsigned wave = (unsigned)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const unsigned long long W = (unsigned long long)gridDim.x * 4ull;
    constexpr int kNone = 0x7fffffff;
    for (unsigned long long u = (unsigned long long)blockIdx.x * 4ull + wave; u < X.words; u += W) {
        const unsigned long long r = u / (unsigned)X.rw;
        const int xw = X.rw0 + (int)(u - r * (unsigned)X.rw);
        const unsigned long long sl = r / (unsigned)X.F.n[1];
        const int ry = (int)(r - sl * (unsigned)X.F.n[1]);  // row and slice within the region
        const unsigned long long* const row = X.bits + ((size_t)(X.F.lo[2] + (int)sl) * (size_t)X.ny + (size_t)(X.F.lo[1] + ry)) * (size_t)X.wx;
        const unsigned long long w = dist_src_word<COMP>(X, row, xw);
        // the nearest set bit in the words to the left and to the right of this one (wave-uniform)
        int left = kNone, right = kNone;
        for (int k = xw - 1; k >= X.rw0; --k) {
            const unsigned long long v = dist_src_word<COMP>(X, row, k);
            if (v != 0ull) {
                left = (k << 6) + 63 - __clzll((long long)v);
                break;
            }
        }
        for (int k = xw + 1; k < X.rw0 + X.rw; ++k) {
            const unsigned long long v = dist_src_word<COMP>(X, row, k);
            if (v != 0ull) {
                right = (k << 6) + __ffsll((long long)v) - 1;
                break;
            }
        }
        const int x = (xw << 6) + (int)lane;
        if (x >= X.F.lo[0] && x < X.F.lo[0] + X.F.n[0]) {
            const unsigned long long le = w & ((2ull << lane) - 1ull);  // the bits at or below the lane's (lane 63: all)
            const unsigned long long ge = w >> lane;                    // the bits at or above it, the lane's own at bit 0
            const int dl = le != 0ull ? (int)lane - (63 - __clzll((long long)le)) : (left != kNone ? x - left : kNone);
            const int dr = ge != 0ull ? __ffsll((long long)ge) - 1 : (right != kNone ? right - x : kNone);
            const int d = dl < dr ? dl : dr;
            const size_t idx = ((size_t)sl * (size_t)X.F.n[1] + (size_t)ry) * (size_t)X.F.n[0] + (size_t)(x - X.F.lo[0]);
            X.F.d2[idx] = d == kNone ? kDistNone : dist_sq((long long)d * (long long)X.spacing);
        }
    }
}

__global__ __launch_bounds__(64) void dist_line_kernel(const DistLine L)
{
    const unsigned long long t = (unsigned long long)blockIdx.x * 64ull + threadIdx.x;
    if (t >= L.lanes) return;
    const unsigned long long o = t / L.inner;
    unsigned long long* const line = L.d2 + (size_t)(o * L.outer + (t - o * L.inner));
    unsigned long long* const sg = L.stack_g + (size_t)t;
    unsigned* const st = L.stack_st + (size_t)t;
    const long long s = (long long)L.spacing;
    const int n = L.n;
    // the stack's top: apex ts, its g, and tt = the first index from which this parabola is the lowest
    int q = -1, ts = 0, tt = 0;
    unsigned long long tg = 0ull;
    for (int u = 0; u < n; ++u) {
        const unsigned long long gu = line[(size_t)u * (size_t)L.stride];
        if (gu == kDistNone) continue;
        while (q >= 0) {  // parabolas that u undercuts at their own first index leave the envelope
            if (dist_sq((long long)(tt - ts) * s) + tg <= dist_sq((long long)(tt - u) * s) + gu) break;
            if (--q >= 0) {
                const unsigned e = st[(size_t)q * (size_t)L.lanes];
                tg = sg[(size_t)q * (size_t)L.lanes];
                ts = (int)(e & 0xFFFFu);
                tt = (int)(e >> 16);
            }
        }
        long long first = 0;  // the first index from which u is the lowest
        if (q >= 0) {
            const long long su = (long long)u * s, si = (long long)ts * s;  // (both <= 2^30)
            const long long num = (su * su - si * si) + ((long long)gu - (long long)tg);  // (|.| < 2^60 + 2^62)
            const long long den = 2ll * s * (su - si);                                     // (0 < . <= 2^51)
            long long sep = num / den;
            if (num < 0 && sep * den != num) --sep;  // floor
            first = sep + 1;
        }
        if (first < (long long)n) {
            ++q;
            ts = u;
            tt = (int)first;  // (<= 65534: fits 16 bits, as does the apex)
            tg = gu;
            st[(size_t)q * (size_t)L.lanes] = (unsigned)ts | (unsigned)tt << 16;
            sg[(size_t)q * (size_t)L.lanes] = tg;
        }
    }
    if (q < 0) return;  // (no parabola: the line keeps kDistNone)
    for (int u = n - 1; u >= 0; --u) {
        line[(size_t)u * (size_t)L.stride] = dist_sq((long long)(u - ts) * s) + tg;
        if (u == tt && --q >= 0) {
            const unsigned e = st[(size_t)q * (size_t)L.lanes];
            tg = sg[(size_t)q * (size_t)L.lanes];
            ts = (int)(e & 0xFFFFu);
            tt = (int)(e >> 16);
        }
    }
}

// the field's value at voxel (x, y, z) of the box; `outside`: what it is known to be outside the region
__device__ __forceinline__ unsigned long long dist_field_at(const DistField& F, int x, int y, int z, unsigned long long outside)
{
    const int fx = x - F.lo[0], fy = y - F.lo[1], fz = z - F.lo[2];
    if (fx < 0 || fx >= F.n[0] || fy < 0 || fy >= F.n[1] || fz < 0 || fz >= F.n[2]) return outside;
    return F.d2[((size_t)fz * (size_t)F.n[1] + (size_t)fy) * (size_t)F.n[0] + (size_t)fx];
}

__global__ __launch_bounds__(256) void dist_write_kernel(const DistParams P)
{
    const unsigned lane = threadIdx.x & 63u;
    const unsigned wave = (unsigned)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    float* const out = reinterpret_cast<float*>(P.dst) + P.dst_channel;
    unsigned long long n_beyond = 0ull, n_probe = 0ull;     // (wave-uniform)
    unsigned long long p_min = kDistNone, p_max = 0ull;     // (per lane)
    const unsigned long long W = (unsigned long long)gridDim.x * 4ull;
    for (unsigned long long u = (unsigned long long)blockIdx.x * 4ull + wave; u < P.b.box_words; u += W) {
        int xw, y, z;
        bit_box_word(P.b, u, xw, y, z);
        const size_t word = ((size_t)z * (size_t)P.b.ny + (size_t)y) * (size_t)P.b.wx + (size_t)xw;
        const unsigned long long aw = P.a[word];
        const unsigned long long pw = P.probe ? P.probe[word] : 0ull;  // (zero outside the box)
        const unsigned long long box = bit_xmask(xw, P.b.lo[0], P.b.hi[0]);
        const bool in_box = (box >> lane) & 1ull, in_a = (aw >> lane) & 1ull;
        const int x = (xw << 6) + (int)lane;
        bool beyond = false;
        if (in_box) {
            // D2out is 0 in A' and D2in is 0 outside it; outside its region the OUTSIDE field is BEYOND (the INSIDE field's region holds A')
            const bool inside = P.mode == VR_DIST_INSIDE || (P.mode == VR_DIST_SIGNED && in_a);
            unsigned long long d2 = 0ull;
            if (inside ? in_a : !in_a) d2 = inside ? dist_field_at(P.in, x, y, z, kDistNone) : dist_field_at(P.out, x, y, z, kDistNone);
            if (P.limit_sq != 0ull && d2 != kDistNone && d2 > P.limit_sq) d2 = kDistNone;
            beyond = d2 == kDistNone;
            const float m = beyond ? P.beyond_value : sqrtf((float)d2) * P.scale;
            const size_t idx = ((size_t)z * (size_t)P.b.ny + (size_t)y) * (size_t)P.b.nx + (size_t)x;
            out[idx * 4u] = (P.mode == VR_DIST_SIGNED && in_a) ? -m : m;
            if ((pw >> lane) & 1ull) {  // (a probe comes with OUTSIDE or SIGNED only: d2 is D2out unless the voxel is in A', where that is 0)
                const unsigned long long d2out = in_a ? 0ull : d2;
                p_min = d2out < p_min ? d2out : p_min;
                p_max = d2out > p_max ? d2out : p_max;
            }
        }
        n_beyond += (unsigned long long)__popcll(vr_ballot(beyond));
        n_probe += (unsigned long long)__popcll(pw);
    }
    if (P.probe) {  // (uniform: every lane takes part in the folds)
        p_min = wave_min_u64(p_min);
        p_max = wave_max_u64(p_max);
    }
    if (lane == 0u) {
        if (n_beyond != 0ull) atomicAdd(&P.w->beyond, n_beyond);
        if (n_probe != 0ull) {
            atomicAdd(&P.w->probe_voxels, n_probe);
            atomicMin(&P.w->probe_min, p_min);
            atomicMax(&P.w->probe_max, p_max);
        }
    }
}

}  // namespace vr
