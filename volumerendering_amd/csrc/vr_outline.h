// vr_outline.h -- contour tracing on the device (vr_mask_outlines, include/vr.h): the inverse of vr_raster.h.  The contours of a mask
// slot, slice by slice, become closed rectilinear polygons: the cracks between voxels that are in and voxels that are not, linked into
// loops, each loop reduced to its corners.  Exact integer work on the BIT-ROWS of vr_bitrows.h: nothing can be fused, so vr_set_arithmetic
// plays no part and the kernels are compiled once, included by vr_api.hip alone.  No kernel walks a loop, waits for another workgroup or
// spins: a phase ends at a launch boundary.
//
// Lattice: vertex (i, j), 0 <= i <= nx, 0 <= j <= ny, is the lower-left corner of voxel (i, j).  A VERTEX ROW j lies between voxel rows
// j - 1 (A, below) and j (B, above); a call has rows lo[1] .. hi[1] of the box, ceil((nx + 1) / 64) VERTEX WORDS each (nx = 64 needs a
// second one), for every slice of the box and every contour traced: word u = ((c * slices + z) * rows + j) * vwx + vw.
//
// Corners (outline_corners_kernel): one lane per vertex word.  With SE = A, NE = B and SW, NW = the same shifted up by one bit with the
// carry of the word before, `one` = SW ^ SE ^ NW ^ NE (1 or 3 of the 2 x 2 voxels are in: one corner) and `two` = a diagonal pair is in
// (two corners).  Both masks are kept; the word's count popc(one) + 2 popc(two), scanned over all words (the scan of vr_scan.h: sums per
// tile of 1024, one workgroup over the sums, add back), numbers the CORNER NODES in the order contour, slice, key: a loop's smallest node is its
// smallest key and nothing is sorted.
//
// Link (outline_link_kernel): one lane per node.  Word and bit by two binary searches (the scanned bases, the word's counts); the edge
// that leaves: the one of the vertex, or at a saddle the smaller direction for the first node and the larger for the second.  Along +-x
// the next corner is the next set bit of one | two in the row's words, along +-y the same bit tested row by row.  At the arrival the
// edge that leaves is the vertex's only one, or at a saddle the left turn (SPLIT) / the right turn (JOIN); its node number comes from the
// word's base and a popcount of the bits below.  Stored: pred[successor] = node, the node's point in the caller's unit, its slice and
// contour.  The shoelace term of the edge, in lattice units, is summed per contour (64-bit integer adds commute: exact in any order).
//
// Rank (outline_rank_kernel, one launch per round r): pointer doubling over pred.  A node holds the smallest node of its backward window
// of 2^r nodes, the offset at which it lies (the smallest one on a tie: a window that wraps) and the node 2^r back.  A round joins the
// window with that of the jump target and squares the jump.  Once the windows cover the loops every node knows its loop's LEADER and
// its own rank behind it.  A round that changes nothing anywhere is the last one needed: along a loop, min over 2^r equals min over
// 2^(r+1) at every node only if every window already holds the loop's minimum.
//
// Emit: leaders flagged and scanned (the polygons, already in order), their point counts rank(pred(leader)) + 1 scanned (`first`);
// every node stores its point at first + rank, a leader the vr_polygon.
//
// Bit counts and searches are the compiler's builtins (__builtin_popcountll, __builtin_ctzll, ...), not HIP's __popcll / __ffsll /
// __clzll wrappers: further callers of the wrappers change how the compiler inlines them into dist_x_kernel and brick_dist_x_kernel,
// whose instructions then differ from the build before (tools/device_code_diff.py); with the builtins every older kernel is unchanged.
#pragma once
#include "vr_bitrows.h"

namespace vr {

// The vertex lattice of one vr_mask_outlines: passed by value inside the argument blocks.
struct OutlineGrid {
    BitRows b;                            // the volume, the box
    int nc;                               // contours traced ...
    int kmap[4];                          // ... and their numbers, ascending
    int vwx;                              // vertex words per vertex row: nx / 64 + 1
    unsigned rows, slices;                // vertex rows per slice (ny of the box + 1), slices of the box
    unsigned long long vwords;            // nc * slices * rows * vwx
    const unsigned long long* bits[4];    // the packed contours, by their place in kmap (zero outside the box)
    long long ox, oy, sx, sy;             // vertex (i, j) -> (ox + i * sx, oy + j * sy): the origin less the offset, the spacing
    int join;                             // VR_OUTLINE_JOIN
};

// The device words of one vr_mask_outlines.
struct OutlineWords {
    unsigned long long nodes, polygons, points;  // the totals of the three scans
    long long area2[4];                          // per contour number
    unsigned polygons_of[4], points_of[4];
    unsigned changed[32];                        // round r changed something
    CountBox packed[4];                          // the packs' counts and boxes, by place in kmap (each starts as CountBox::empty())
};

struct OutlineNodes {
    const ulonglong2* masks;  // per vertex word: (one, two)
    const unsigned* base;     // per vertex word: the nodes before it
    unsigned n;               // nodes
    unsigned* pred;
    int2* pt;
    unsigned* meta;           // slice | contour << 16
};

// ---- the lattice ---------------------------------------------------------------------------------------------------------------------

// word xw of voxel row y of slice z of packed contour c; zero outside the box's rows and the row's words
__device__ __forceinline__ unsigned long long outline_row_word(const OutlineGrid& G, int c, int z, int y, int xw)
{
    if (y < G.b.lo[1] || y >= G.b.hi[1] || xw < 0 || xw >= G.b.wx) return 0ull;
    return G.bits[c][((size_t)z * (size_t)G.b.ny + (size_t)y) * (size_t)G.b.wx + (size_t)xw];
}

// vertex word u -> contour place c, slice z, vertex row j, word vw
__device__ __forceinline__ void outline_word(const OutlineGrid& G, unsigned long long u, int& c, int& z, int& j, int& vw)
{
    unsigned long long t = u / (unsigned)G.vwx;
    vw = (int)(u - t * (unsigned)G.vwx);
    unsigned long long t2 = t / G.rows;
    j = G.b.lo[1] + (int)(t - t2 * G.rows);
    const unsigned long long t3 = t2 / G.slices;
    z = G.b.lo[2] + (int)(t2 - t3 * G.slices);
    c = (int)t3;
}

__device__ __forceinline__ unsigned long long outline_word_index(const OutlineGrid& G, int c, int z, int j, int vw)
{
    return (((unsigned long long)c * G.slices + (unsigned)(z - G.b.lo[2])) * G.rows + (unsigned)(j - G.b.lo[1])) * (unsigned)G.vwx + (unsigned)vw;
}

// the four voxels around the vertices of word vw of vertex row j: bit p = vertex 64 vw + p
struct OutlineQuad { unsigned long long sw, se, nw, ne; };
__device__ __forceinline__ OutlineQuad outline_quad(const OutlineGrid& G, int c, int z, int j, int vw)
{
    const unsigned long long a = outline_row_word(G, c, z, j - 1, vw), b = outline_row_word(G, c, z, j, vw);
    const unsigned long long ap = outline_row_word(G, c, z, j - 1, vw - 1), bp = outline_row_word(G, c, z, j, vw - 1);
    return {(a << 1) | (ap >> 63), a, (b << 1) | (bp >> 63), b};
}

// the directions (bit d: 0 = +x, 1 = +y, 2 = -x, 3 = -y) of the edges that leave vertex bit p of a quad, the voxel on their left
__device__ __forceinline__ unsigned outline_leaving(const OutlineQuad& q, int p)
{
    const unsigned sw = (unsigned)(q.sw >> p) & 1u, se = (unsigned)(q.se >> p) & 1u, nw = (unsigned)(q.nw >> p) & 1u, ne = (unsigned)(q.ne >> p) & 1u;
    return (ne & ~se & 1u) | ((nw & ~ne & 1u) << 1) | ((sw & ~nw & 1u) << 2) | ((se & ~sw & 1u) << 3);
}

__device__ __forceinline__ unsigned long long bits_below(int p) { return (1ull << p) - 1ull; }  // (p <= 63)

// the nodes of a word at vertices below bit p
__device__ __forceinline__ unsigned outline_nodes_below(ulonglong2 m, int p)
{
    const unsigned long long below = bits_below(p);
    return (unsigned)__builtin_popcountll(m.x & below) + 2u * (unsigned)__builtin_popcountll(m.y & below);
}

__global__ __launch_bounds__(256) void outline_corners_kernel(const OutlineGrid G, ulonglong2* masks, unsigned* counts)
{
    const unsigned long long stride = (unsigned long long)gridDim.x * 256ull;
    for (unsigned long long u = (unsigned long long)blockIdx.x * 256ull + threadIdx.x; u < G.vwords; u += stride) {
        int c, z, j, vw;
        outline_word(G, u, c, z, j, vw);
        const OutlineQuad q = outline_quad(G, c, z, j, vw);
        const unsigned long long one = q.sw ^ q.se ^ q.nw ^ q.ne;
        const unsigned long long two = (q.sw & q.ne & ~q.se & ~q.nw) | (q.se & q.nw & ~q.sw & ~q.ne);
        masks[u] = make_ulonglong2(one, two);
        counts[u] = (unsigned)__builtin_popcountll(one) + 2u * (unsigned)__builtin_popcountll(two);
    }
}

__global__ __launch_bounds__(256) void outline_link_kernel(const OutlineGrid G, const OutlineNodes N, OutlineWords* words)
{
    const unsigned lane = threadIdx.x & 63u;
    const unsigned long long stride = (unsigned long long)gridDim.x * 256ull;
    long long area[4] = {0, 0, 0, 0};  // by place in kmap
    for (unsigned long long id = (unsigned long long)blockIdx.x * 256ull + threadIdx.x; id < N.n; id += stride) {
        const unsigned n = (unsigned)id;
        // the node's word: the last one whose base is <= n (words without nodes share the base of the next word with some)
        unsigned long long lo = 0, hi = G.vwords - 1ull;
        while (lo < hi) {
            const unsigned long long mid = (lo + hi + 1ull) >> 1;
            if (N.base[mid] <= n) lo = mid;
            else hi = mid - 1ull;
        }
        const unsigned long long u = lo;
        const ulonglong2 m = N.masks[u];
        const unsigned r = n - N.base[u];
        int p0 = 0, p1 = 63;  // the first bit with more than r nodes at or below it
        while (p0 < p1) {
            const int mid = (p0 + p1) >> 1;
            const unsigned upto = (unsigned)__builtin_popcountll(m.x & (bits_below(mid) | (1ull << mid))) + 2u * (unsigned)__builtin_popcountll(m.y & (bits_below(mid) | (1ull << mid)));
            if (upto > r) p1 = mid;
            else p0 = mid + 1;
        }
        const int p = p0;
        const unsigned second = r - outline_nodes_below(m, p);  // 1: the second node of a saddle
        int c, z, j, vw;
        outline_word(G, u, c, z, j, vw);
        const int i = (vw << 6) + p;
        const unsigned out = outline_leaving(outline_quad(G, c, z, j, vw), p);
        const int d = second ? 31 - __builtin_clz(out) : __builtin_ctz(out);  // (out != 0: the vertex is a corner)

        // to the next corner along d
        int i2 = i, j2 = j, vw2 = vw, p2 = p;
        ulonglong2 m2 = m;
        unsigned long long u2 = u;
        bool found = true;
        if (d == 0 || d == 2) {
            const unsigned long long any = m.x | m.y;
            unsigned long long rest = d == 0 ? any & ~(bits_below(p) | (1ull << p)) : any & bits_below(p);
            while (rest == 0ull) {
                vw2 += d == 0 ? 1 : -1;
                if (vw2 < 0 || vw2 >= G.vwx) {
                    found = false;
                    break;
                }
                u2 = outline_word_index(G, c, z, j, vw2);
                m2 = N.masks[u2];
                rest = m2.x | m2.y;
            }
            if (found) {
                p2 = d == 0 ? __builtin_ctzll(rest) : 63 - __builtin_clzll(rest);  // (rest != 0)
                i2 = (vw2 << 6) + p2;
            }
        } else {
            for (;;) {
                j2 += d == 1 ? 1 : -1;
                if (j2 < G.b.lo[1] || j2 > G.b.hi[1]) {
                    found = false;
                    break;
                }
                u2 = outline_word_index(G, c, z, j2, vw);
                m2 = N.masks[u2];
                if (((m2.x | m2.y) >> p) & 1ull) break;
            }
        }
        if (!found) continue;  // (cannot happen: every chain of cracks ends in a corner of the lattice; nothing is written out of bounds)
        unsigned d2, second2 = 0u;
        if ((m2.x >> p2) & 1ull) {
            d2 = (unsigned)__builtin_ctz(outline_leaving(outline_quad(G, c, z, j2, vw2), p2) | 16u);  // (| 16: defined for no edge, which cannot be)
        } else {
            d2 = ((unsigned)d + (G.join ? 3u : 1u)) & 3u;
            second2 = d2 >> 1;
        }
        const unsigned succ = N.base[u2] + outline_nodes_below(m2, p2) + second2;
        if (succ < N.n) N.pred[succ] = n;
        N.pt[n] = make_int2((int)(G.ox + (long long)i * G.sx), (int)(G.oy + (long long)j * G.sy));
        N.meta[n] = (unsigned)z | ((unsigned)G.kmap[c] << 16);
        const long long cross = (long long)i * (long long)j2 - (long long)i2 * (long long)j;
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (k == c) area[k] += cross;
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if (k >= G.nc) break;  // (uniform)
        const unsigned long long sum = wave_sum_u64((unsigned long long)area[k]);
        if (lane == 0u && sum != 0ull) atomicAdd(reinterpret_cast<unsigned long long*>(&words->area2[G.kmap[k]]), sum);
    }
}

// ---- leader and rank ---------------------------------------------------------------------------------------------------------------

// a node's state: x = the smallest node of its window, y = the offset at which it lies, z = the node one window back
__global__ __launch_bounds__(256) void outline_rank_init_kernel(const unsigned* pred, unsigned n, uint4* st)
{
    const unsigned long long stride = (unsigned long long)gridDim.x * 256ull;
    for (unsigned long long i = (unsigned long long)blockIdx.x * 256ull + threadIdx.x; i < n; i += stride) st[i] = make_uint4((unsigned)i, 0u, pred[i], 0u);
}

__global__ __launch_bounds__(256) void outline_rank_kernel(const uint4* in, uint4* out, unsigned n, unsigned window, unsigned* changed)
{
    const unsigned long long stride = (unsigned long long)gridDim.x * 256ull;
    bool any = false;
    for (unsigned long long i = (unsigned long long)blockIdx.x * 256ull + threadIdx.x; i < n; i += stride) {
        uint4 s = in[i];
        const uint4 t = in[s.z];
        if (t.x < s.x) {  // (equal: the node's own offset is below the window, the other one is not)
            s.x = t.x;
            s.y = t.y + window;
            any = true;
        }
        s.z = t.z;
        out[i] = s;
    }
    if (any) *changed = 1u;  // (every writer stores the same value)
}

// ---- emit --------------------------------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(256) void outline_leaders_kernel(const uint4* st, unsigned n, unsigned* flags)
{
    const unsigned long long stride = (unsigned long long)gridDim.x * 256ull;
    for (unsigned long long i = (unsigned long long)blockIdx.x * 256ull + threadIdx.x; i < n; i += stride) flags[i] = st[i].x == (unsigned)i ? 1u : 0u;
}

// one lane: per contour, its nodes and the polygons led by them, from the two scans at the contours' first words
__global__ void outline_totals_kernel(const OutlineGrid G, const unsigned* base, const unsigned* pidx, OutlineWords* w)
{
    if (threadIdx.x != 0u || blockIdx.x != 0u) return;
    const unsigned long long per = G.vwords / (unsigned)G.nc;
    for (int c = 0; c < G.nc; ++c) {
        const unsigned n0 = base[(unsigned long long)c * per];
        const unsigned n1 = c + 1 < G.nc ? base[(unsigned long long)(c + 1) * per] : (unsigned)w->nodes;
        const unsigned q0 = n0 < (unsigned)w->nodes ? pidx[n0] : (unsigned)w->polygons;
        const unsigned q1 = n1 < (unsigned)w->nodes ? pidx[n1] : (unsigned)w->polygons;
        w->points_of[G.kmap[c]] = n1 - n0;
        w->polygons_of[G.kmap[c]] = q1 - q0;
    }
}

// pcount[polygon] = the points of the loop: the rank of the node before its leader, and one
__global__ __launch_bounds__(256) void outline_counts_kernel(const uint4* st, const unsigned* pred, const unsigned* pidx, unsigned n, unsigned* pcount)
{
    const unsigned long long stride = (unsigned long long)gridDim.x * 256ull;
    for (unsigned long long i = (unsigned long long)blockIdx.x * 256ull + threadIdx.x; i < n; i += stride)
        if (st[i].x == (unsigned)i) pcount[pidx[i]] = st[pred[i]].y + 1u;
}

__global__ __launch_bounds__(256) void outline_emit_kernel(const uint4* st, const OutlineNodes N, const unsigned* pidx, const unsigned* pfirst, int2* points,
                                                           vr_polygon* polygons)
{
    const unsigned long long stride = (unsigned long long)gridDim.x * 256ull;
    for (unsigned long long i = (unsigned long long)blockIdx.x * 256ull + threadIdx.x; i < N.n; i += stride) {
        const uint4 s = st[i];
        const unsigned q = pidx[s.x], first = pfirst[q];
        if ((unsigned long long)first + s.y < N.n) points[(size_t)first + s.y] = N.pt[i];  // (always: a rank is below its loop's length)
        if (s.x == (unsigned)i) {
            const unsigned meta = N.meta[i];
            vr_polygon g;
            g.first = first;
            g.count = st[N.pred[i]].y + 1u;
            g.slice = (int)(meta & 0xffffu);
            g.contour = (int)(meta >> 16);
            polygons[q] = g;
        }
    }
}

}  // namespace vr
