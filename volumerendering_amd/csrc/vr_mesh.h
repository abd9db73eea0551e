// vr_mesh.h -- surface extraction on the device (vr_volume_mesh, include/vr.h): the surface {value >= level} of one component of a slot
// inside a voxel box as an indexed triangle mesh, by MARCHING TETRAHEDRA on the Kuhn split of every cell.  The 3-D counterpart of
// vr_outline.h.  The combinatorics are exact integer work on bit-rows; a position is two subtractions and one IEEE division in f32 with
// nothing to fuse, so vr_set_arithmetic plays no part and the kernels are compiled once, included by vr_api.hip alone.  No kernel waits
// for another workgroup or spins: a phase ends at a launch boundary, and every output is a function of the inputs alone.
//
// Lattice: the points of the call, (hi - lo) + 2 cap per axis from e = lo - cap, packed into LATTICE ROWS of their own: word
// u = (lz * ln[1] + ly) * lw + w, bit i of word w = the point lx = 64 w + i (vr_bitrows.h's shape, but over the lattice, not the volume:
// the raster order of the words and their bits is then the order of include/vr.h's vertex keys, and a virtual point is a bit like any
// other).  Bits beyond ln[0] are zero.
//
// Pack (mesh_pack_kernel): one wavefront per word, one lane per point; the word is ONE 64-bit ballot of real && v >= level
// (VR_VARIANT_ISO's rule: equal is in, NaN is out; a virtual point is out).  Exact settling (channel 3, not vr_set_kernel_flavour(1)):
// a lane first reads the range record (min .a, max .a) of the voxel's own 4 x 4 x 4 brick (brick_range_kernel) and, unless it is the
// flagged (NaN, NaN) one,
//     max < level  ->  out          min >= level  ->  in
// and the voxel is not loaded.  This is exact: a record spans the voxels [4 b, min(4 b + 4, n - 1)]^3 -- the 5^3 voxels the brick's
// cells touch -- a superset of the brick's own, and is flagged whenever one of them is NaN, infinite or above 2^125 in magnitude; so the
// voxel v is a number with min <= v <= max and the comparisons are the voxel test's own (f32 compares are exact and transitive on
// numbers): max < level gives v < level, min >= level gives v >= level.  A NaN bound fails both and the voxel is loaded.  Hence a
// settled brick owns no crossing edge and no crossing cell: all the 5^3 points its cells touch got the same bit from the same record
// test or from their own value, which the record bounds.  Only REAL points are settled: with cap = 1 the virtual layer next to a box
// face is out whatever the records say, so a brick of ones there still emits its cap -- "all inside" is a statement about voxels, never
// about cells.
//
// Count (mesh_count_kernel): one lane per word.  The eight corner rows c_s of the cells whose origins are the word's points (s = the
// corner's offset x + 2 y + 4 z; a shift by one bit with the carry of the next word for x) give the seven CROSSING MASKS
// X_m = c_0 ^ c_m, masked to the edges (p, p + d) whose far end is a lattice point: bit i of X_m = the vertex of key (p, m).  The word's
// vertices are the popcounts of the seven; its triangles one per tetrahedron with an odd number of inside corners and two per tetrahedron
// with two, over the word's cells.  Two scans (scan_*_kernel, vr_scan.h) give every word its vertex base and triangle base in key
// order: nothing is sorted.  (Every lattice edge with both ends in a lattice of at least 2 points per axis belongs to some cell: the
// cell p - s for an s in {0,1}^3 with s . d = 0 that keeps the cell inside; a thinner lattice has no cells and the host stops there.)
//
// Vertices (mesh_vertex_kernel): one wavefront per word, one lane per point: id = the word's base + the crossings of all seven masks
// below the lane's bit + the earlier directions at the bit; t = (level - v_a) / (v_b - v_a), clamped, 0 or 1 at a virtual end.
//
// Triangles (mesh_triangle_kernel): one wavefront per word, one lane per cell.  A corner's inside bit is c_0 ^ X_s at the cell's bit; the
// vertex on edge (p, m) is found as above from the masks and the base of p's word (the word itself, the next one for bit 63, the rows
// above).  The case table and the orientation swaps (6 tetrahedra x 14 cases) are DERIVED at compile time (mesh_tables): the swap is
// the sign of ((p1 - p0) x (p2 - p0)) . (outside centroid - inside centroid) with the vertices at their edges' midpoints, in integers.
//
// Bit counts are the compiler's builtins, not HIP's wrappers (see vr_outline.h: the older kernels' listings must not move).
#pragma once
#include "vr_bitrows.h"

namespace vr {

// One vr_volume_mesh: passed by value.
struct MeshGrid {
    const float* val;              // component `channel` of the slot's first voxel; one voxel = 4 floats
    int nx, ny, nz;                // of the volume
    int lo[3], hi[3];              // the box: the real points
    int e[3], ln[3];               // the lattice: its first point (lo - cap) and its points per axis
    int lw;                        // words per lattice row: ceil(ln[0] / 64)
    unsigned long long words;      // lw * ln[1] * ln[2]
    float level;
    const float2* bricks;          // the slot's range records (channel 3, settling form), or nullptr
    int bnx, bny;
};

// The device words of one vr_volume_mesh.
struct MeshWords {
    unsigned long long stats[3];   // points of the box, voxels loaded, voxels settled
    unsigned long long inside;     // real points that are inside
    unsigned long long vertices, triangles;  // the totals of the two scans
    CountBox cells;                // the cells that emit (their origins); starts as CountBox::empty()
};

// ---- the tables, derived ---------------------------------------------------------------------------------------------------------------

// perm[T] = the axes (a, b, c) of tetrahedron T: q0 = o, q1 = q0 + e_a, q2 = q1 + e_b, q3 = o + (1,1,1).
// tri[c], c = the inside bits of (q0 .. q3): bits 0..1 the triangles (0, 1, 2), then their six vertices as edge numbers, 3 bits each
// (edge q_i q_j: 01 -> 0, 02 -> 1, 03 -> 2, 12 -> 3, 13 -> 4, 23 -> 5).  swap[T] bit c: the last two indices of the case's triangles
// are exchanged.
struct MeshTables {
    unsigned char perm[6][3];
    unsigned tri[16];
    unsigned short swap[6];
};

constexpr int mesh_edge(int i, int j)
{
    const int a = i < j ? i : j, b = i < j ? j : i;
    return a == 0 ? b - 1 : a == 1 ? b + 1 : 5;
}

constexpr MeshTables mesh_tables()
{
    MeshTables t = {};
    int n = 0;
    for (int a = 0; a < 3; ++a)  // lexicographic: xyz, xzy, yxz, yzx, zxy, zyx
        for (int b = 0; b < 3; ++b) {
            if (b == a) continue;
            t.perm[n][0] = (unsigned char)a, t.perm[n][1] = (unsigned char)b, t.perm[n][2] = (unsigned char)(3 - a - b);
            ++n;
        }
    for (int c = 1; c < 15; ++c) {
        int in[4] = {}, out[4] = {}, ni = 0, no = 0;
        for (int i = 0; i < 4; ++i) {
            if ((c >> i) & 1) in[ni++] = i;
            else out[no++] = i;
        }
        if (ni == 2) {  // inside i < j, outside k < l: (v_ik, v_il, v_jl), (v_ik, v_jl, v_jk)
            const int ik = mesh_edge(in[0], out[0]), il = mesh_edge(in[0], out[1]), jl = mesh_edge(in[1], out[1]), jk = mesh_edge(in[1], out[0]);
            t.tri[c] = 2u | (unsigned)ik << 2 | (unsigned)il << 5 | (unsigned)jl << 8 | (unsigned)ik << 11 | (unsigned)jl << 14 | (unsigned)jk << 17;
        } else {  // q_i alone, the others j < k < l: (v_ij, v_ik, v_il)
            const int i = ni == 1 ? in[0] : out[0];
            const int* o = ni == 1 ? out : in;
            t.tri[c] = 1u | (unsigned)mesh_edge(i, o[0]) << 2 | (unsigned)mesh_edge(i, o[1]) << 5 | (unsigned)mesh_edge(i, o[2]) << 8;
        }
    }
    const int ends[6][2] = {{0, 1}, {0, 2}, {0, 3}, {1, 2}, {1, 3}, {2, 3}};
    for (int T = 0; T < 6; ++T) {
        int q[4][3] = {};
        for (int i = 1; i < 4; ++i) {
            for (int a = 0; a < 3; ++a) q[i][a] = q[i - 1][a];
            q[i][t.perm[T][i - 1]] += 1;
        }
        for (int c = 1; c < 15; ++c) {
            int P[3][3] = {}, D[3] = {}, ni = 0;
            for (int i = 0; i < 4; ++i) ni += (c >> i) & 1;
            for (int v = 0; v < 3; ++v) {  // twice the midpoints of the first triangle's edges
                const int e = (int)((t.tri[c] >> (2 + 3 * v)) & 7u);
                for (int a = 0; a < 3; ++a) P[v][a] = q[ends[e][0]][a] + q[ends[e][1]][a];
            }
            for (int i = 0; i < 4; ++i)  // ni * (4 - ni) * (outside centroid - inside centroid)
                for (int a = 0; a < 3; ++a) D[a] += ((c >> i) & 1) ? -(4 - ni) * q[i][a] : ni * q[i][a];
            const int u[3] = {P[1][0] - P[0][0], P[1][1] - P[0][1], P[1][2] - P[0][2]};
            const int w[3] = {P[2][0] - P[0][0], P[2][1] - P[0][1], P[2][2] - P[0][2]};
            const int dot = (u[1] * w[2] - u[2] * w[1]) * D[0] + (u[2] * w[0] - u[0] * w[2]) * D[1] + (u[0] * w[1] - u[1] * w[0]) * D[2];
            if (dot < 0) t.swap[T] = (unsigned short)(t.swap[T] | (1u << c));
        }
    }
    return t;
}

constexpr MeshTables kMesh = mesh_tables();

// ---- the lattice -----------------------------------------------------------------------------------------------------------------------

// word u -> word w of row ly of slice lz
__device__ __forceinline__ void mesh_word(const MeshGrid& G, unsigned long long u, int& w, int& ly, int& lz)
{
    const unsigned long long row = u / (unsigned)G.lw;
    w = (int)(u - row * (unsigned)G.lw);
    const unsigned long long sl = row / (unsigned)G.ln[1];
    ly = (int)(row - sl * (unsigned)G.ln[1]);
    lz = (int)sl;
}

// the voxel behind lattice point (lx, ly, lz) is a real point: it lies in the box
__device__ __forceinline__ bool mesh_real(const MeshGrid& G, int x, int y, int z)
{
    return x >= G.lo[0] && x < G.hi[0] && y >= G.lo[1] && y < G.hi[1] && z >= G.lo[2] && z < G.hi[2];
}

__device__ __forceinline__ float mesh_value(const MeshGrid& G, int x, int y, int z)
{
    return G.val[(((size_t)z * (size_t)G.ny + (size_t)y) * (size_t)G.nx + (size_t)x) * 4u];
}

// the bits of word w whose points lx have lx + dx < ln[0]
__device__ __forceinline__ unsigned long long mesh_xmask(const MeshGrid& G, int w, int dx)
{
    const int n = G.ln[0] - (w << 6) - dx;
    return n <= 0 ? 0ull : n >= 64 ? ~0ull : ((1ull << n) - 1ull);
}

// word w of lattice row (ly, lz); zero beyond the lattice
__device__ __forceinline__ unsigned long long mesh_row(const MeshGrid& G, const unsigned long long* bits, int w, int ly, int lz)
{
    if (w >= G.lw || ly >= G.ln[1] || lz >= G.ln[2]) return 0ull;
    return bits[((size_t)lz * (size_t)G.ln[1] + (size_t)ly) * (size_t)G.lw + (size_t)w];
}

// corner s of the cells whose origins are the points of word (w, ly, lz): bit i = the point (64 w + i, ly, lz) + s
__device__ __forceinline__ unsigned long long mesh_corner(const MeshGrid& G, const unsigned long long* bits, int w, int ly, int lz, int s)
{
    const int y = ly + ((s >> 1) & 1), z = lz + (s >> 2);
    const unsigned long long a = mesh_row(G, bits, w, y, z);
    return (s & 1) ? (a >> 1) | (mesh_row(G, bits, w + 1, y, z) << 63) : a;
}

__device__ __forceinline__ int wave_min_i32(int v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = min(v, __shfl_xor(v, off, 64));  // (every lane takes part)
    return v;
}
__device__ __forceinline__ int wave_max_i32(int v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = max(v, __shfl_xor(v, off, 64));
    return v;
}

// ---- pack ------------------------------------------------------------------------------------------------------------------------------

template <bool PLAIN>
__global__ __launch_bounds__(256) void mesh_pack_kernel(const MeshGrid G, unsigned long long* bits, MeshWords* words)
{
    const unsigned lane = threadIdx.x & 63u;
    const unsigned wave = (unsigned)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    unsigned long long n_box = 0, n_load = 0, n_settled = 0, n_in = 0;  // per lane (n_in: lane 0)
    const unsigned long long W = (unsigned long long)gridDim.x * 4ull;
    for (unsigned long long u = (unsigned long long)blockIdx.x * 4ull + wave; u < G.words; u += W) {
        int w, ly, lz;
        mesh_word(G, u, w, ly, lz);
        const int x = G.e[0] + (w << 6) + (int)lane, y = G.e[1] + ly, z = G.e[2] + lz;
        bool in = false;
        if (mesh_real(G, x, y, z)) {  // (hi <= n: a voxel of the volume)
            bool settled = false;
            if constexpr (!PLAIN) {
                if (G.bricks) {
                    const float2 rec = G.bricks[((size_t)(z >> 2) * (size_t)G.bny + (size_t)(y >> 2)) * (size_t)G.bnx + (size_t)(x >> 2)];
                    const bool none = rec.y < G.level, every = rec.x >= G.level;  // (the flagged record fails both)
                    settled = none || every;
                    in = every;
                }
            }
            if (!settled) in = mesh_value(G, x, y, z) >= G.level;
            n_box += 1u;
            n_load += settled ? 0u : 1u;
            n_settled += settled ? 1u : 0u;
        }
        const unsigned long long word = vr_ballot(in);
        if (lane == 0u) {
            bits[u] = word;
            n_in += (unsigned long long)__builtin_popcountll(word);
        }
    }
    n_box = wave_sum_u64(n_box);
    n_load = wave_sum_u64(n_load);
    n_settled = wave_sum_u64(n_settled);
    if (lane == 0u) {
        if (n_box != 0ull) atomicAdd(&words->stats[0], n_box);
        if (n_load != 0ull) atomicAdd(&words->stats[1], n_load);
        if (n_settled != 0ull) atomicAdd(&words->stats[2], n_settled);
        if (n_in != 0ull) atomicAdd(&words->inside, n_in);
    }
}

// ---- count -----------------------------------------------------------------------------------------------------------------------------

// The masks of a word: m[0] = the cells that emit, m[1 .. 7] = the crossing masks X_m; stored as 8 words per lattice word.
__global__ __launch_bounds__(256) void mesh_count_kernel(const MeshGrid G, const unsigned long long* bits, unsigned long long* masks, unsigned* vcount,
                                                         unsigned* tcount, MeshWords* words)
{
    const unsigned lane = threadIdx.x & 63u;
    const unsigned long long stride = (unsigned long long)gridDim.x * 256ull;
    CountBox n = CountBox::empty();  // per lane
    for (unsigned long long u = (unsigned long long)blockIdx.x * 256ull + threadIdx.x; u < G.words; u += stride) {
        int w, ly, lz;
        mesh_word(G, u, w, ly, lz);
        unsigned long long c[8];
#pragma unroll
        for (int s = 0; s < 8; ++s) c[s] = mesh_corner(G, bits, w, ly, lz, s);
        const bool yok = ly + 1 < G.ln[1], zok = lz + 1 < G.ln[2];
        const unsigned long long x0 = mesh_xmask(G, w, 0), x1 = mesh_xmask(G, w, 1);
        unsigned nv = 0;
        unsigned long long any = 0ull;
#pragma unroll
        for (int m = 1; m < 8; ++m) {
            const bool ok = (!(m & 2) || yok) && (!(m & 4) || zok);
            const unsigned long long X = ok ? (c[0] ^ c[m]) & ((m & 1) ? x1 : x0) : 0ull;
            masks[u * 8ull + (unsigned)m] = X;
            nv += (unsigned)__builtin_popcountll(X);
            any |= X;
        }
        const unsigned long long cells = yok && zok ? x1 : 0ull;
        const unsigned long long active = any & cells;  // (a cell whose corners disagree has a corner that differs from c_0)
        masks[u * 8ull] = active;
        unsigned nt = 0;
#pragma unroll
        for (int T = 0; T < 6; ++T) {
            const int s1 = 1 << kMesh.perm[T][0], s2 = s1 | (1 << kMesh.perm[T][1]);
            const unsigned long long odd = c[0] ^ c[s1] ^ c[s2] ^ c[7];
            const unsigned long long two = ~odd & ((c[0] ^ c[s1]) | (c[0] ^ c[s2]) | (c[0] ^ c[7]));
            nt += (unsigned)__builtin_popcountll(odd & cells) + 2u * (unsigned)__builtin_popcountll(two & cells);
        }
        vcount[u] = nv;
        tcount[u] = nt;
        if (active != 0ull) {
            n.voxels += (unsigned long long)__builtin_popcountll(active);
            const int xa = G.e[0] + (w << 6);
            n.lo[0] = min(n.lo[0], xa + __builtin_ctzll(active));
            n.hi[0] = max(n.hi[0], xa + 64 - __builtin_clzll(active));
            n.lo[1] = min(n.lo[1], G.e[1] + ly);
            n.hi[1] = max(n.hi[1], G.e[1] + ly + 1);
            n.lo[2] = min(n.lo[2], G.e[2] + lz);
            n.hi[2] = max(n.hi[2], G.e[2] + lz + 1);
        }
    }
    n.voxels = wave_sum_u64(n.voxels);
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        n.lo[a] = wave_min_i32(n.lo[a]);
        n.hi[a] = wave_max_i32(n.hi[a]);
    }
    if (lane == 0u) report_count_box(&words->cells, n.voxels, n.lo, n.hi);
}

// ---- vertices --------------------------------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(256) void mesh_vertex_kernel(const MeshGrid G, const unsigned long long* masks, const unsigned* vbase, unsigned n_vertices,
                                                          float* vertices)
{
    const unsigned lane = threadIdx.x & 63u;
    const unsigned wave = (unsigned)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const unsigned long long below = (1ull << lane) - 1ull;
    const unsigned long long W = (unsigned long long)gridDim.x * 4ull;
    for (unsigned long long u = (unsigned long long)blockIdx.x * 4ull + wave; u < G.words; u += W) {
        unsigned long long X[8];
        unsigned long long any = 0ull;
#pragma unroll
        for (int m = 1; m < 8; ++m) {
            X[m] = masks[u * 8ull + (unsigned)m];
            any |= X[m];
        }
        if (((any >> lane) & 1ull) == 0ull) continue;
        unsigned id = vbase[u];
#pragma unroll
        for (int m = 1; m < 8; ++m) id += (unsigned)__builtin_popcountll(X[m] & below);
        int w, ly, lz;
        mesh_word(G, u, w, ly, lz);
        const int x = G.e[0] + (w << 6) + (int)lane, y = G.e[1] + ly, z = G.e[2] + lz;
        const bool ra = mesh_real(G, x, y, z);
        const float va = ra ? mesh_value(G, x, y, z) : 0.0f;
#pragma unroll
        for (int m = 1; m < 8; ++m) {
            if (((X[m] >> lane) & 1ull) == 0ull) continue;
            const int bx = x + (m & 1), by = y + ((m >> 1) & 1), bz = z + (m >> 2);
            float t;
            if (!ra) t = 1.0f;  // (the vertex sits on the real end)
            else if (!mesh_real(G, bx, by, bz)) t = 0.0f;
            else {
                const float vb = mesh_value(G, bx, by, bz);
                t = (G.level - va) / (vb - va);
                if (!(t >= 0.0f)) t = 0.0f;  // (NaN too)
                if (t > 1.0f) t = 1.0f;
            }
            if (id < n_vertices) {  // (always)
                float* const v = vertices + (size_t)id * 3u;
                v[0] = (m & 1) ? (float)x + t : (float)x;
                v[1] = (m & 2) ? (float)y + t : (float)y;
                v[2] = (m & 4) ? (float)z + t : (float)z;
            }
            ++id;
        }
    }
}

// ---- triangles -------------------------------------------------------------------------------------------------------------------------

__device__ __forceinline__ unsigned mesh_pick(const unsigned (&E)[6], unsigned k)
{
    return k == 0u ? E[0] : k == 1u ? E[1] : k == 2u ? E[2] : k == 3u ? E[3] : k == 4u ? E[4] : E[5];
}

// the vertex on the edge from corner P of the cell (P = 0 .. 6) along direction M: R = the vertices before the corner's point, B = the
// crossings at the point (bit m - 1 = X_m)
template <int P, int M>
__device__ __forceinline__ unsigned mesh_vid(const unsigned (&R)[7], const unsigned (&B)[7])
{
    return R[P] + (unsigned)__builtin_popcount(B[P] & ((1u << (M - 1)) - 1u));
}

// tetrahedron T of a cell whose corners' inside bits are in8 (bit s = corner s): its triangles from number tid on
template <int T>
__device__ __forceinline__ void mesh_tet(unsigned in8, const unsigned (&R)[7], const unsigned (&B)[7], unsigned& tid, unsigned n_triangles, unsigned* triangles)
{
    constexpr int s1 = 1 << kMesh.perm[T][0], s2 = s1 | (1 << kMesh.perm[T][1]);
    const unsigned c = (in8 & 1u) | (((in8 >> s1) & 1u) << 1) | (((in8 >> s2) & 1u) << 2) | (((in8 >> 7) & 1u) << 3);
    if (c == 0u || c == 15u) return;
    const unsigned E[6] = {mesh_vid<0, s1>(R, B),      mesh_vid<0, s2>(R, B),      mesh_vid<0, 7>(R, B),
                           mesh_vid<s1, s2 ^ s1>(R, B), mesh_vid<s1, 7 ^ s1>(R, B), mesh_vid<s2, 7 ^ s2>(R, B)};
    const unsigned code = kMesh.tri[c];
    const bool sw = ((unsigned)kMesh.swap[T] >> c) & 1u;
    const unsigned nt = code & 3u;
    for (unsigned k = 0; k < nt; ++k) {
        const unsigned sh = 2u + 9u * k;
        const unsigned a = mesh_pick(E, (code >> sh) & 7u), b = mesh_pick(E, (code >> (sh + 3u)) & 7u), d = mesh_pick(E, (code >> (sh + 6u)) & 7u);
        if (tid < n_triangles) {  // (always)
            unsigned* const t = triangles + (size_t)tid * 3u;
            t[0] = a;
            t[1] = sw ? d : b;
            t[2] = sw ? b : d;
        }
        ++tid;
    }
}

__global__ __launch_bounds__(256) void mesh_triangle_kernel(const MeshGrid G, const unsigned long long* bits, const unsigned long long* masks,
                                                            const unsigned* vbase, const unsigned* tbase, unsigned n_triangles, unsigned* triangles)
{
    const unsigned lane = threadIdx.x & 63u;
    const unsigned wave = (unsigned)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const unsigned long long below = (1ull << lane) - 1ull;
    const unsigned long long W = (unsigned long long)gridDim.x * 4ull;
    const unsigned long long urow = (unsigned)G.lw, uslice = (unsigned long long)(unsigned)G.lw * (unsigned)G.ln[1];
    for (unsigned long long u = (unsigned long long)blockIdx.x * 4ull + wave; u < G.words; u += W) {
        const unsigned long long active = masks[u * 8ull];
        if (((active >> lane) & 1ull) == 0ull) continue;  // (an active cell: every word and bit below exists)
        const unsigned long long c0 = bits[u];
        unsigned long long c[8];
        c[0] = c0;
#pragma unroll
        for (int m = 1; m < 8; ++m) c[m] = c0 ^ masks[u * 8ull + (unsigned)m];  // (exact at the bits of cells)
        // the triangles of the word's cells below this one
        unsigned tid = tbase[u];
        unsigned in8 = 0u;
#pragma unroll
        for (int s = 0; s < 8; ++s) in8 |= (unsigned)((c[s] >> lane) & 1ull) << s;
#pragma unroll
        for (int T = 0; T < 6; ++T) {
            const int s1 = 1 << kMesh.perm[T][0], s2 = s1 | (1 << kMesh.perm[T][1]);
            const unsigned long long odd = c[0] ^ c[s1] ^ c[s2] ^ c[7];
            const unsigned long long two = ~odd & ((c[0] ^ c[s1]) | (c[0] ^ c[s2]) | (c[0] ^ c[7]));
            tid += (unsigned)__builtin_popcountll(odd & active & below) + 2u * (unsigned)__builtin_popcountll(two & active & below);
        }
        // the seven corners an edge can start from: the vertices before their points, the crossings at them
        unsigned R[7], B[7];
#pragma unroll
        for (int s = 0; s < 7; ++s) {
            const unsigned bit = lane + (unsigned)(s & 1);
            const unsigned long long us = u + (bit >> 6) + ((s & 2) ? urow : 0ull) + ((s & 4) ? uslice : 0ull);
            const unsigned p = bit & 63u;
            const unsigned long long bl = (1ull << p) - 1ull;
            unsigned r = vbase[us], b = 0u;
#pragma unroll
            for (int m = 1; m < 8; ++m) {
                const unsigned long long X = masks[us * 8ull + (unsigned)m];
                r += (unsigned)__builtin_popcountll(X & bl);
                b |= (unsigned)((X >> p) & 1ull) << (m - 1);
            }
            R[s] = r;
            B[s] = b;
        }
        mesh_tet<0>(in8, R, B, tid, n_triangles, triangles);
        mesh_tet<1>(in8, R, B, tid, n_triangles, triangles);
        mesh_tet<2>(in8, R, B, tid, n_triangles, triangles);
        mesh_tet<3>(in8, R, B, tid, n_triangles, triangles);
        mesh_tet<4>(in8, R, B, tid, n_triangles, triangles);
        mesh_tet<5>(in8, R, B, tid, n_triangles, triangles);
    }
}

}  // namespace vr
