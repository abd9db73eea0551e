// vr_comp.h -- connected components of a mask contour on the device (vr_mask_components, include/vr.h).  Exact integer work on the
// BIT-ROWS of vr_bitrows.h: nothing can be fused, so vr_set_arithmetic plays no part and the kernels are compiled once, included by
// vr_api.hip alone.  There is one kernel form.  No kernel waits for another workgroup or spins on a word another workgroup writes: a
// phase ends at a launch boundary.
//
// Set: S is packed by bit_pack_kernel (background: complemented under the box mask, comp_complement_kernel); it is zero outside the box.
//
// Nodes (comp_starts_kernel, the scan of vr_scan.h, comp_runs_kernel): a NODE is a maximal run of set bits along x in one row of the
// box; it may span words.  The runs that start in a word are w & ~((w << 1) | carry), carry = bit 63 of the word before it in the row.
// The scan of the per-word start counts over the box's words, which bit_box_word numbers x-fastest, then y, then z, numbers the nodes in
// the order of their first voxels: node order is `first`-voxel order and nothing is ever sorted.  The run that holds a set bit x is the
// last one that starts at or below x in its row: node = base[word of x] + popc(starts of that word at or below x) - 1 (comp_node_at),
// also when it started in an earlier word.  A node stores its row of the box and its first and last x (two 32-bit words).
//
// Merge (comp_merge_kernel): one lane per node.  In each earlier row its connectivity names -- 6: (y-1, z), (y, z-1) over [a, b];
// 26: (y-1, z), (y-1, z-1), (y, z-1), (y+1, z-1) over [a-1, b+1]; 4 / 8: (y-1, z) alone -- the runs of (row & window) are the distinct
// runs that touch it; it unites with each: both walk to their roots, the larger root is hooked under the smaller with a fetch_min on
// its parent word, and if the value returned shows that it was no root any more the union goes on from that value (the link it had is
// kept by uniting what it pointed to).  Parents only ever decrease, so there is no cycle and a component's root is its smallest node.
// EVERY access to the parent array in this kernel is a relaxed agent-scope atomic: the L2s of the XCDs are not coherent with each other
// and a CU's L1 is never refreshed by another CU's stores.  A stale parent would still be an ancestor and cost a step; what decides is
// the atomic's return value.
//
// Flatten, number (comp_flatten_kernel, comp_leaders_kernel, the scan): every node gets its root; roots are flagged and scanned: label
// of a node = idx[root] + 1, the total is n_components.
//
// Statistics (comp_init_kernel, comp_stats_kernel): the table on the device is an array of vr_component.  A root sets its entry from
// its own run (`first` is the root's first voxel: no atomic), then every node adds its voxels and folds its run into the box and the
// faces with integer atomics, the mins, maxes and ors only where a (possibly stale, hence conservative) read shows they would change.
// The lanes of a wavefront that hold the label of its first node are folded with shuffles first and report once.
//
// Selection (comp_pass_kernel, comp_pick_kernel, comp_result_kernel): size window and faces per component on the device; for
// keep_largest the host picks the K winners from a copy of the passing sizes and hands their numbers back in an argument block.  |R|,
// its box and n_selected are folded from the table, a wavefront at a time.
//
// Expand and write (comp_expand_kernel, comp_write_kernel): the selected nodes OR their bits into R's rows; one wavefront per word of
// the box, one lane per voxel stores the contour through BitCombine and the label channel ((float)label in S, +0.0f elsewhere).
//
// Bit counts are the compiler's builtins, not HIP's wrappers (vr_outline.h says why).
#pragma once
#include "vr_bitrows.h"
#include "vr_outline.h"  // bits_below

namespace vr {

// The set and the box of one vr_mask_components: passed by value inside the argument blocks.
struct CompGrid {
    BitRows b;                     // the volume, the box and its words
    const unsigned long long* s;   // S, packed (wx * ny * nz words, zero outside the box)
    unsigned rows;                 // rows per slice of the box
    int conn;                      // VR_COMP_FACES ..
};

struct CompNodes {
    const unsigned* base;  // per word of the box: the nodes before it
    unsigned n;            // nodes
    unsigned* parent;      // the union-find forest; after the numbering: idx (the roots before a node)
    unsigned* root;        // after the flatten
    unsigned* row;         // the node's row of the box: (z - lo[2]) * rows + (y - lo[1])
    unsigned* ab;          // its first x | its last x << 16
};

// The device words of one vr_mask_components.
struct CompWords {
    unsigned long long nodes, components;  // the totals of the two scans
    unsigned long long pairs;              // (node, touching run in an earlier row) examined
    unsigned long long largest, selected;  // voxels of the biggest component; n_selected
    CountBox packed;                       // the pack's count and box (starts as CountBox::empty())
    CountBox result;                       // |R| and its box (starts as CountBox::empty())
};

// What selects a component, and the winners of keep_largest.
struct CompFilter {
    unsigned long long min_voxels, max_voxels;
    unsigned reject_faces;
    unsigned by_winners, n_winners;        // keep_largest: the winners below are the selection
    unsigned winners[VR_COMP_MAX_KEEP];
};

// Kernel argument block of the write.
struct CompWrite {
    float4* dst;                   // the destination slot's x-fastest vec4 voxels
    int dst_contour;               // -1: no contour
    int label_channel;             // -1: no label map
    const unsigned long long* r;   // R's rows
    BitCombine c;
};

__device__ __forceinline__ size_t comp_word_index(const BitRows& B, int xw, int y, int z)
{
    return ((size_t)z * (size_t)B.ny + (size_t)y) * (size_t)B.wx + (size_t)xw;
}

// word (xw, y, z) of the box's words (the inverse of bit_box_word)
__device__ __forceinline__ unsigned long long comp_box_word(const CompGrid& G, int xw, int y, int z)
{
    return ((unsigned long long)(unsigned)(z - G.b.lo[2]) * G.rows + (unsigned)(y - G.b.lo[1])) * (unsigned)G.b.bw + (unsigned)(xw - G.b.bw0);
}

// the runs that start in word w, `before` the word before it in its row (0 for the row's first)
__device__ __forceinline__ unsigned long long comp_starts(unsigned long long w, unsigned long long before) { return w & ~((w << 1) | (before >> 63)); }

// the node that holds set bit p of word (xw, y, z), whose bits are w and whose word before is `before`
__device__ __forceinline__ unsigned comp_node_at(const CompGrid& G, const unsigned* base, int xw, int y, int z, int p, unsigned long long w, unsigned long long before)
{
    const unsigned long long upto = bits_below(p) | (1ull << p);
    return base[comp_box_word(G, xw, y, z)] + (unsigned)__builtin_popcountll(comp_starts(w, before) & upto) - 1u;
}

__global__ __launch_bounds__(256) void comp_complement_kernel(const BitRows B, unsigned long long* bits)
{
    const unsigned long long stride = (unsigned long long)gridDim.x * 256ull;
    for (unsigned long long u = (unsigned long long)blockIdx.x * 256ull + threadIdx.x; u < B.box_words; u += stride) {
        int xw, y, z;
        bit_box_word(B, u, xw, y, z);
        const size_t i = comp_word_index(B, xw, y, z);
        bits[i] = ~bits[i] & bit_xmask(xw, B.lo[0], B.hi[0]);
    }
}

__global__ __launch_bounds__(256) void comp_starts_kernel(const CompGrid G, unsigned* counts)
{
    const unsigned long long stride = (unsigned long long)gridDim.x * 256ull;
    for (unsigned long long u = (unsigned long long)blockIdx.x * 256ull + threadIdx.x; u < G.b.box_words; u += stride) {
        int xw, y, z;
        bit_box_word(G.b, u, xw, y, z);
        const size_t i = comp_word_index(G.b, xw, y, z);
        const unsigned long long before = xw > 0 ? G.s[i - 1] : 0ull;
        counts[u] = (unsigned)__builtin_popcountll(comp_starts(G.s[i], before));
    }
}

// one lane per word of the box: the runs that start in it, followed to their ends
__global__ __launch_bounds__(256) void comp_runs_kernel(const CompGrid G, const CompNodes N)
{
    const unsigned long long stride = (unsigned long long)gridDim.x * 256ull;
    const int xw_end = G.b.bw0 + G.b.bw;
    for (unsigned long long u = (unsigned long long)blockIdx.x * 256ull + threadIdx.x; u < G.b.box_words; u += stride) {
        int xw, y, z;
        bit_box_word(G.b, u, xw, y, z);
        const size_t i = comp_word_index(G.b, xw, y, z);
        const unsigned long long w = G.s[i];
        unsigned long long st = comp_starts(w, xw > 0 ? G.s[i - 1] : 0ull);
        unsigned node = N.base[u];
        const unsigned row = (unsigned)(u / (unsigned)G.b.bw);
        while (st != 0ull) {
            const int p = __builtin_ctzll(st);
            st &= st - 1ull;
            const unsigned long long zeros = ~w & ~bits_below(p);  // (bit p is set: the zeros above it)
            int last;
            if (zeros != 0ull) {
                last = (xw << 6) + __builtin_ctzll(zeros) - 1;
            } else {
                last = (xw_end << 6) - 1;  // (to the end of the row's words, unless a word on the way has a zero)
                for (int xw2 = xw + 1; xw2 < xw_end; ++xw2) {
                    const unsigned long long z2 = ~G.s[i + (size_t)(xw2 - xw)];
                    if (z2 != 0ull) {
                        last = (xw2 << 6) + __builtin_ctzll(z2) - 1;
                        break;
                    }
                }
            }
            if (node < N.n) {  // (always: the scan counted these starts)
                N.parent[node] = node;
                N.row[node] = row;
                N.ab[node] = (unsigned)((xw << 6) + p) | ((unsigned)last << 16);
            }
            ++node;
        }
    }
}

__device__ __forceinline__ unsigned comp_parent(unsigned* parent, unsigned x)
{
    return __hip_atomic_load(&parent[x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__device__ __forceinline__ unsigned comp_find(unsigned* parent, unsigned x)
{
    for (;;) {
        const unsigned p = comp_parent(parent, x);
        if (p >= x) return x;  // (p == x: a root; p < x otherwise, so the walk ends)
        x = p;
    }
}

__device__ __forceinline__ void comp_unite(unsigned* parent, unsigned a, unsigned b)
{
    for (;;) {
        a = comp_find(parent, a);
        b = comp_find(parent, b);
        if (a == b) return;
        const unsigned big = a > b ? a : b, small = a > b ? b : a;
        const unsigned old = __hip_atomic_fetch_min(&parent[big], small, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (old == big) return;  // it was a root and hangs under `small` now
        a = old;                 // it hung under `old` (< big) already: whichever of the two links the word lost is made here
        b = small;
    }
}

__global__ __launch_bounds__(256) void comp_merge_kernel(const CompGrid G, const CompNodes N, CompWords* words)
{
    const unsigned lane = threadIdx.x & 63u;
    const unsigned long long stride = (unsigned long long)gridDim.x * 256ull;
    const bool plane = G.conn == VR_COMP_PLANE_FACES || G.conn == VR_COMP_PLANE_ALL;
    const bool all = G.conn == VR_COMP_ALL || G.conn == VR_COMP_PLANE_ALL;
    const int e = all ? 1 : 0;
    unsigned long long pairs = 0ull;
    for (unsigned long long id = (unsigned long long)blockIdx.x * 256ull + threadIdx.x; id < N.n; id += stride) {
        const unsigned n = (unsigned)id;
        const unsigned row = N.row[n], ab = N.ab[n];
        const int z = G.b.lo[2] + (int)(row / G.rows), y = G.b.lo[1] + (int)(row % G.rows);
        const int x0 = max((int)(ab & 0xffffu) - e, G.b.lo[0]), x1 = min((int)(ab >> 16) + e, G.b.hi[0] - 1);
        // the earlier rows: k = 0: (y-1, z); 1: (y, z-1); 2: (y-1, z-1); 3: (y+1, z-1)
        const int rows_named = plane ? 1 : (all ? 4 : 2);
        for (int k = 0; k < rows_named; ++k) {
            const int yy = k == 1 ? y : (k == 3 ? y + 1 : y - 1), zz = k == 0 ? z : z - 1;
            if (yy < G.b.lo[1] || yy >= G.b.hi[1] || zz < G.b.lo[2]) continue;
            const int xw0 = x0 >> 6, xw1 = x1 >> 6;
            const size_t i0 = comp_word_index(G.b, 0, yy, zz);
            unsigned long long before = xw0 > 0 ? G.s[i0 + (size_t)(xw0 - 1)] : 0ull;  // (the whole word: for the node's number)
            unsigned long long in_before = 0ull;                                        // (within the window: for the distinct runs)
            for (int xw = xw0; xw <= xw1; ++xw) {
                const unsigned long long w = G.s[i0 + (size_t)xw];
                const unsigned long long in = w & bit_xmask(xw, x0, x1 + 1);
                unsigned long long st = comp_starts(in, in_before);
                while (st != 0ull) {
                    const int p = __builtin_ctzll(st);
                    st &= st - 1ull;
                    const unsigned q = comp_node_at(G, N.base, xw, yy, zz, p, w, before);
                    if (q < N.n) comp_unite(N.parent, n, q);  // (always)
                    ++pairs;
                }
                before = w;
                in_before = in;
            }
        }
    }
    pairs = wave_sum_u64(pairs);
    if (lane == 0u && pairs != 0ull) atomicAdd(&words->pairs, pairs);
}

__global__ __launch_bounds__(256) void comp_flatten_kernel(const unsigned* parent, unsigned n, unsigned* root)
{
    const unsigned long long stride = (unsigned long long)gridDim.x * 256ull;
    for (unsigned long long i = (unsigned long long)blockIdx.x * 256ull + threadIdx.x; i < n; i += stride) {
        unsigned x = (unsigned)i;
        for (;;) {
            const unsigned p = parent[x];
            if (p >= x) break;  // (p == x: a root)
            x = p;
        }
        root[i] = x;
    }
}

__global__ __launch_bounds__(256) void comp_leaders_kernel(const unsigned* root, unsigned n, unsigned* flags)
{
    const unsigned long long stride = (unsigned long long)gridDim.x * 256ull;
    for (unsigned long long i = (unsigned long long)blockIdx.x * 256ull + threadIdx.x; i < n; i += stride) flags[i] = root[i] == (unsigned)i ? 1u : 0u;
}

// a node's row, run and the faces of the box it lies on
struct CompRun { int a, b, y, z; unsigned faces; };
__device__ __forceinline__ CompRun comp_run(const CompGrid& G, const CompNodes& N, unsigned n)
{
    const unsigned row = N.row[n], ab = N.ab[n];
    CompRun r;
    r.a = (int)(ab & 0xffffu);
    r.b = (int)(ab >> 16);
    r.z = G.b.lo[2] + (int)(row / G.rows);
    r.y = G.b.lo[1] + (int)(row % G.rows);
    r.faces = (r.a == G.b.lo[0] ? 1u : 0u) | (r.b == G.b.hi[0] - 1 ? 2u : 0u) | (r.y == G.b.lo[1] ? 4u : 0u) | (r.y == G.b.hi[1] - 1 ? 8u : 0u) |
              (r.z == G.b.lo[2] ? 16u : 0u) | (r.z == G.b.hi[2] - 1 ? 32u : 0u);
    return r;
}

// idx = N.parent after the numbering.  A root sets its component's entry from its own run.
__global__ __launch_bounds__(256) void comp_init_kernel(const CompGrid G, const CompNodes N, vr_component* table)
{
    const unsigned long long stride = (unsigned long long)gridDim.x * 256ull;
    for (unsigned long long i = (unsigned long long)blockIdx.x * 256ull + threadIdx.x; i < N.n; i += stride) {
        if (N.root[i] != (unsigned)i) continue;
        const CompRun r = comp_run(G, N, (unsigned)i);
        vr_component c;
        c.voxels = 0;
        c.lo[0] = c.first[0] = r.a, c.lo[1] = c.first[1] = r.y, c.lo[2] = c.first[2] = r.z;
        c.hi[0] = r.b + 1, c.hi[1] = r.y + 1, c.hi[2] = r.z + 1;
        c.faces = 0u;
        table[N.parent[i]] = c;
    }
}

// voxels, a box and faces into a component's entry.  A stale read of a word that only falls is >= its value, so skipping the atomic on
// `>=` is right; likewise for the words that only rise.
__device__ __forceinline__ void comp_fold(vr_component* c, unsigned long long voxels, const int lo[3], const int hi[3], unsigned faces)
{
    atomicAdd(reinterpret_cast<unsigned long long*>(&c->voxels), voxels);
    for (int a = 0; a < 3; ++a) {
        if (lo[a] < __hip_atomic_load(&c->lo[a], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMin(&c->lo[a], lo[a]);
        if (hi[a] > __hip_atomic_load(&c->hi[a], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(&c->hi[a], hi[a]);
    }
    if (faces & ~__hip_atomic_load(&c->faces, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicOr(&c->faces, faces);
}

// Every node folds its run into its component's entry.  Nodes are in raster order, so the 64 of a wavefront often belong to one
// component, and one big component would serialise every add on one address: the lanes that hold the label of the wavefront's first
// node are folded with shuffles and reported once, by lane 0; the others report alone.
__global__ __launch_bounds__(256) void comp_stats_kernel(const CompGrid G, const CompNodes N, vr_component* table)
{
    const unsigned lane = threadIdx.x & 63u;
    const unsigned long long stride = (unsigned long long)gridDim.x * 256ull;
    for (unsigned long long i0 = (unsigned long long)blockIdx.x * 256ull; i0 < N.n; i0 += stride) {  // (uniform: every lane takes part in the votes)
        const unsigned long long i = i0 + threadIdx.x;
        bool alone = i < N.n;
        unsigned c = 0u, faces = 0u;
        unsigned long long voxels = 0ull;
        int lo[3] = {0x7fffffff, 0x7fffffff, 0x7fffffff}, hi[3] = {0, 0, 0};
        if (alone) {
            const CompRun r = comp_run(G, N, (unsigned)i);
            c = N.parent[N.root[i]];
            voxels = (unsigned long long)(r.b - r.a + 1);
            lo[0] = r.a, lo[1] = r.y, lo[2] = r.z;
            hi[0] = r.b + 1, hi[1] = r.y + 1, hi[2] = r.z + 1;
            faces = r.faces;
        }
        const unsigned long long act = vr_ballot(alone);
        if (act == 0ull) continue;  // (uniform)
        const unsigned c0 = (unsigned)__shfl((int)c, __builtin_ctzll(act), 64);
        const bool shared = alone && c == c0;
        if (__builtin_popcountll(vr_ballot(shared)) > 1) {  // (uniform)
            unsigned long long v = wave_sum_u64(shared ? voxels : 0ull);
            unsigned f = shared ? faces : 0u;
            int l[3], h[3];
            for (int a = 0; a < 3; ++a) l[a] = shared ? lo[a] : 0x7fffffff, h[a] = shared ? hi[a] : 0;
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) {
                f |= (unsigned)__shfl_down((int)f, off, 64);
                for (int a = 0; a < 3; ++a) {
                    l[a] = min(l[a], __shfl_down(l[a], off, 64));
                    h[a] = max(h[a], __shfl_down(h[a], off, 64));
                }
            }
            if (lane == 0u) comp_fold(table + c0, v, l, h, f);
            alone = alone && !shared;
        }
        if (alone) comp_fold(table + c, voxels, lo, hi, faces);
    }
}

// per component: sel = it passes the window and the faces (0 when the winners decide), pass = its voxels if it passes, else 0
__global__ __launch_bounds__(256) void comp_pass_kernel(const vr_component* table, unsigned long long n, const CompFilter F, unsigned* sel,
                                                        unsigned long long* pass, CompWords* words)
{
    const unsigned lane = threadIdx.x & 63u;
    const unsigned long long stride = (unsigned long long)gridDim.x * 256ull;
    unsigned long long largest = 0ull;
    for (unsigned long long i = (unsigned long long)blockIdx.x * 256ull + threadIdx.x; i < n; i += stride) {
        const unsigned long long v = table[i].voxels;
        const bool ok = v >= F.min_voxels && v <= F.max_voxels && (table[i].faces & F.reject_faces) == 0u;
        sel[i] = ok && !F.by_winners ? 1u : 0u;
        if (F.by_winners) pass[i] = ok ? v : 0ull;  // (a component has a voxel: 0 is free)
        largest = v > largest ? v : largest;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const unsigned long long o = __shfl_down(largest, off, 64);
        largest = o > largest ? o : largest;
    }
    if (lane == 0u && largest != 0ull) atomicMax(&words->largest, largest);
}

__global__ void comp_pick_kernel(const CompFilter F, unsigned* sel)
{
    if (blockIdx.x == 0u && threadIdx.x < F.n_winners) sel[F.winners[threadIdx.x]] = 1u;
}

// n_selected, |R| and its box from the table
__global__ __launch_bounds__(256) void comp_result_kernel(const vr_component* table, unsigned long long n, const unsigned* sel, CompWords* words)
{
    const unsigned lane = threadIdx.x & 63u;
    const unsigned long long stride = (unsigned long long)gridDim.x * 256ull;
    CountBox b = CountBox::empty();
    unsigned long long count = 0ull;
    for (unsigned long long i = (unsigned long long)blockIdx.x * 256ull + threadIdx.x; i < n; i += stride) {
        if (!sel[i]) continue;
        ++count;
        b.voxels += table[i].voxels;
        for (int a = 0; a < 3; ++a) {
            b.lo[a] = min(b.lo[a], table[i].lo[a]);
            b.hi[a] = max(b.hi[a], table[i].hi[a]);
        }
    }
    count = wave_sum_u64(count);
    b.voxels = wave_sum_u64(b.voxels);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1)
        for (int a = 0; a < 3; ++a) {
            b.lo[a] = min(b.lo[a], __shfl_down(b.lo[a], off, 64));
            b.hi[a] = max(b.hi[a], __shfl_down(b.hi[a], off, 64));
        }
    if (lane == 0u && count != 0ull) {
        atomicAdd(&words->selected, count);
        report_count_box(&words->result, b.voxels, b.lo, b.hi);
    }
}

// the selected nodes OR their runs into R's rows (zeroed before)
__global__ __launch_bounds__(256) void comp_expand_kernel(const CompGrid G, const CompNodes N, const unsigned* sel, unsigned long long* r)
{
    const unsigned long long stride = (unsigned long long)gridDim.x * 256ull;
    for (unsigned long long i = (unsigned long long)blockIdx.x * 256ull + threadIdx.x; i < N.n; i += stride) {
        if (!sel[N.parent[N.root[i]]]) continue;
        const CompRun run = comp_run(G, N, (unsigned)i);
        const size_t i0 = comp_word_index(G.b, 0, run.y, run.z);
        for (int xw = run.a >> 6; xw <= run.b >> 6; ++xw) atomicOr(&r[i0 + (size_t)xw], bit_xmask(xw, run.a, run.b + 1));
    }
}

// one wavefront per word of the box, one lane per voxel: the contour through BitCombine, the label channel
__global__ __launch_bounds__(256) void comp_write_kernel(const CompGrid G, const CompNodes N, const CompWrite P)
{
    const unsigned lane = threadIdx.x & 63u;
    const unsigned wave = (unsigned)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    float* const out = reinterpret_cast<float*>(P.dst);
    const unsigned long long W = (unsigned long long)gridDim.x * 4ull;
    for (unsigned long long u = (unsigned long long)blockIdx.x * 4ull + wave; u < G.b.box_words; u += W) {
        int xw, y, z;
        bit_box_word(G.b, u, xw, y, z);
        const size_t wi = comp_word_index(G.b, xw, y, z);
        const unsigned long long box = bit_xmask(xw, G.b.lo[0], G.b.hi[0]);
        const size_t idx = ((size_t)z * (size_t)G.b.ny + (size_t)y) * (size_t)G.b.nx + (size_t)(xw << 6) + (size_t)lane;
        if (P.dst_contour >= 0) {
            const unsigned long long rw = P.r[wi];  // (zero outside the box)
            const unsigned long long st = P.c.stores(rw, box);
            if ((st >> lane) & 1ull) out[idx * 4u + (unsigned)P.dst_contour] = P.c.value((rw >> lane) & 1ull);
        }
        if (P.label_channel >= 0 && ((box >> lane) & 1ull)) {
            const unsigned long long w = G.s[wi];
            float label = 0.0f;
            if ((w >> lane) & 1ull) {
                const unsigned node = comp_node_at(G, N.base, xw, y, z, (int)lane, w, xw > 0 ? G.s[wi - 1] : 0ull);
                if (node < N.n) label = (float)(N.parent[N.root[node]] + 1u);  // (always; exact: n_components <= 2^24 was checked)
            }
            out[idx * 4u + (unsigned)P.label_channel] = label;
        }
    }
}

}  // namespace vr
