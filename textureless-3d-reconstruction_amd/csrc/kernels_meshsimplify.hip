// kernels_meshsimplify.hip -- vertex-clustering simplification of an indexed triangle mesh (tl3d_mesh_simplify_clusters; DESIGN.md
// section 4.2.2).  No reference code: the reference has no mesh.  The rules are ours (tests/mesh_simplify_reference.py restates them):
//   cell of a vertex, per axis, in fp64 with every operation rounded once: d = (double)x - o, i = floor(d / cell),
//   r = d - (double)i * cell, q = (int64)rint((r / cell) * 2^24); -2^20 <= i < 2^20; a cluster = the vertices of one (ix, iy, iz),
//   with a member count n, exact integer sums S = sum q and C = sum rgb; clusters are numbered in the order of their smallest member
//   (the leader); position = (float)(o + ((double)i + (double)S / ((double)n * 2^24)) * cell), colour = (2 C + n) / (2 n);
//   a triangle is mapped through vert_map, dropped when two mapped indices are equal (degenerate), and dropped when an earlier
//   triangle has the same canonical triple (its rotation with the smallest index first: duplicate); survivors keep input order.
// Quadric placement (tl3d_mesh_simplify_quadric; tests/mesh_simplify_quadric_reference.py restates it) changes only the position:
//   h = (q + 8192) >> 14 (arithmetic shift: 2^10 steps per cell); seen from a cell I a vertex is p = (i - I) * 1024 + h.  Every
//   corner k of every input triangle, with I = i(v_k): it contributes iff |i(v_j) - I| <= 3 on every axis for all three corners j
//   (else it is skipped and counted); N = (p1 - p0) x (p2 - p0), d = -(N . p0) in exact integers; N_a N_b (00, 01, 02, 11, 12, 22)
//   and d N_a go into the nine sums A, b of v_k's cluster (Lindstrom's area^2-weighted plane quadric, once per corner).
//       bound                         because
//       |p| <= 4097                   |i - I| <= 3, 0 <= h <= 1025 (q lies within [-8192, 2^24 + 8192) by far)
//       |N_a| < 2^27                  two products of differences <= 8194: 2 * 8194^2
//       |d| < 2^41                    3 * 2^27 * 4097
//       |N_a N_b| < 2^54, |d N_a| < 2^68
//       |sums| < 2^102                fewer than 3 * 2^32 < 2^34 terms: exact in signed 128 bits, hence order-free
//   solve, per cluster, fp64, every operation rounded once, dbl() as in kernels_meshsmooth.hip: A00 = A11 = A22 = 0 -> the mean
//   rule above (the same bytes).  Otherwise T = (dbl(A00) + dbl(A11)) + dbl(A22), M_ab = dbl(A_ab) / T, g_a = dbl(b_a) / T,
//   m_a = (double)S_a / ((double)n * 16384.0), K = M + reg I, r_a = reg m_a - g_a (Tikhonov towards the mean: K is SPD with
//   eigenvalues in [reg, 1 + reg], so no eigen-decomposition, no rank decision, no square root); K x = r by the adjugate in the
//   order ms_quadric_solve spells out, then ONE step of refinement, x += adj(K) (r - K x) / det, in the same order (the adjugate
//   alone is off by eps / reg^2 on a single plane); x_a clamped to [0, 1024] (a cluster with any axis clamped is counted; an x_a that is no
//   number -- det underflows for reg below 1e-100 or so -- is taken as 0 and counts as clamped);
//   position = (float)(o + ((double)i + x / 1024.0) * cell).
// Everything below is a function of the input alone: results come from integer atomicMin / atomicAdd only, which commute, and the
// compactions write at scanned offsets, so every run gives the same bytes.
//
// Passes, each its own launch on the context's stream (kernel boundaries are the ONLY ordering between them):
//   validate      largest triangle index (cc_validate_kernel) and the number of vertices without a cell; nothing indexed runs
//                 before the host has looked at both
//   insert        one thread per vertex: its key into the vertex table (keytab.h's kt_claim), slot[v] = where it sits,
//                 atomicMin(leader[slot], v)
//   leaders       leader[slot[v]] == v per chunk -> single-block scan -> vert_map[leader] = cluster number, in order (compact.h,
//                 as the triangle classes and the triangle write below)
//   accumulate    one thread per vertex: vert_map[v] = vert_map[leader], atomicAdd of 1, q and rgb into the cluster's seven words
//   quadrics      (quadric placement only) one thread per triangle: i, q of its three vertices again, the at most three
//                 (cluster, frame) contributions with equal clusters merged (k * term once), nine 128-bit adds each
//   tri insert    one thread per triangle: map, and unless degenerate its index into the triangle table (32-bit CAS EMPTY -> t, or
//                 atomicMin into a slot whose occupant has the same canonical triple)
//   tri classify  per chunk: degenerate / duplicate / survivor (the slot of its triple holds t itself) -> flag, counts
//   write         positions (mean, or the quadric solve) and colours per leader at its cluster number; surviving triangles at scanned offsets, mapped
//
// Proof obligations of the two tables.  H1, H3 and H5 of the vertex table (64-bit keys) are keytab.h's and are kept there: n_vert
// vertices bring at most n_vert keys into kt_slots(n_vert) slots.  The triangle table holds 32-bit triangle indices and compares
// canonical triples, so it has loops of its own, and they keep the same three lines: its slots change only by the CAS and the
// atomicMin of H2, n_tri triangles bring at most n_tri entries into kt_slots(n_tri) slots and both loops are bounded by the capacity,
// and a failed CAS is answered by looking at what it returned and probing on.  The lines that are this file's own, each kept by
// every statement that touches the words it names:
//   H2  a triangle slot only ever changes among         EMPTY -> t by CAS sets the slot's canonical triple; from then on only
//       triangles of ONE canonical triple.              atomicMin(slot, t') with triple(t') == triple(occupant) touches it.  So a
//                                                       stale read of a slot names a triangle of the right triple, and every probe
//                                                       sequence a thread has walked stays valid.
//   H4  results come only from integer min and add.     leader: atomicMin; n, S, C: atomicAdd on u64 (two's complement for S);
//                                                       triangle slots: atomicMin.  No float atomics anywhere.  A, b: 128 bits as
//                                                       two u64 words, old = atomicAdd(lo, t_lo), then atomicAdd(hi, t_hi + carry)
//                                                       with carry = (old + t_lo < old).  The adds on lo are serialised by the
//                                                       memory system in SOME order; in that order the word wraps exactly
//                                                       floor((sum of all t_lo) / 2^64) times, whatever the order, and the add
//                                                       that wraps it is the one that sees old + t_lo < old: one carry per wrap.
//                                                       So hi ends at sum t_hi + wraps and (hi, lo) is the sum mod 2^128, exact by
//                                                       the bounds above.  No CAS loop, nobody waits (H5).  (hi, lo) is read only
//                                                       behind the kernel boundary.
//   H6  WHICH slot a key or a triple lands in may       nothing that is written out depends on a slot index: slots are only
//       differ from run to run.                         compared for what they hold (leader, smallest triangle index).
#include "keytab.h"

namespace tl3d {

constexpr unsigned MS_EMPTY = 0xFFFFFFFFu;               // no vertex index (< 2^31) and no triangle index (< 2^32 - 1) equals it
constexpr double MS_Q = 16777216.0;                      // 2^24 steps per cell
enum : uint8_t { MS_DEGENERATE = 0, MS_DUPLICATE = 1, MS_SURVIVOR = 2 };

struct MsCell {
    double cell, o[3];
};

// i = floor(d / cell) per axis as a double; false when the vertex has no cell (not finite, or |i| beyond 2^20)
__device__ __forceinline__ bool ms_cell_of(const MsCell &g, const float *__restrict__ p, double d[3], double fi[3]) {
    bool ok = true;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        d[a] = (double)p[a] - g.o[a];
        fi[a] = floor(d[a] / g.cell);
        ok = ok && fi[a] >= -1048576.0 && fi[a] < 1048576.0;          // false for NaN and for an infinity
    }
    return ok;
}

// (63 bits: never KT_EMPTY)
__device__ __forceinline__ unsigned long long ms_key(const double fi[3]) {
    return ((unsigned long long)((long long)fi[0] + 1048576ll) << 42) | ((unsigned long long)((long long)fi[1] + 1048576ll) << 21) |
           (unsigned long long)((long long)fi[2] + 1048576ll);
}

// info[1] += vertices without a cell
__global__ __launch_bounds__(256) void ms_validate_kernel(MsCell g, const float *__restrict__ xyz, unsigned n, unsigned long long *__restrict__ info) {
    const unsigned v = blockIdx.x * 256u + threadIdx.x;
    bool bad = false;
    if (v < n) {
        double d[3], fi[3];
        bad = !ms_cell_of(g, xyz + 3ull * v, d, fi);
    }
    wave_count(bad, info + 1);
}

// (every vertex has a cell: the host has seen info[1] == 0)
__global__ __launch_bounds__(256) void ms_insert_kernel(MsCell g, const float *__restrict__ xyz, unsigned n, unsigned long long *keys,
                                                        unsigned *leader, unsigned long long mask, unsigned *__restrict__ slot) {
    const unsigned v = blockIdx.x * 256u + threadIdx.x;
    if (v >= n) return;
    double d[3], fi[3];
    ms_cell_of(g, xyz + 3ull * v, d, fi);
    bool won;
    const unsigned long long h = kt_claim(keys, mask, ms_key(fi), won);
    if (h == KT_NONE) return;                                          // (keytab.h H3: never)
    slot[v] = (unsigned)h;                                             // (capacity <= 2^32)
    atomicMin(leader + h, v);
}

__global__ __launch_bounds__(256) void ms_leader_count_kernel(const unsigned *__restrict__ slot, const unsigned *__restrict__ leader, unsigned n,
                                                              unsigned *__restrict__ chunk_counts) {
    __shared__ unsigned sm[4];
    unsigned c = 0;
    for_chunk([&](unsigned long long v) {
        if (v < n) c += leader[slot[v]] == (unsigned)v ? 1u : 0u;
    });
    c = block_sum(c, sm);
    if (threadIdx.x == 0) chunk_counts[blockIdx.x] = c;
}

// vert_map[leader] = its cluster's number: leaders in index order
__global__ __launch_bounds__(256) void ms_leader_write_kernel(const unsigned *__restrict__ slot, const unsigned *__restrict__ leader, unsigned n,
                                                              const unsigned long long *__restrict__ offsets, unsigned *__restrict__ vmap) {
    compact_chunk(
        n, offsets, [&](unsigned long long v) { return leader[slot[v]] == (unsigned)v ? 1u : 0u; },
        [&](unsigned long long v, unsigned long long o, unsigned) { vmap[v] = (unsigned)o; });
}

// acc[7 c ..] += (1, qx, qy, qz, r, g, b) of every member of cluster c; vert_map of the members that are no leaders.  A leader's
// vert_map word was written by the kernel before this one and is only read here; a member's word is written by its own thread.
__global__ __launch_bounds__(256) void ms_accumulate_kernel(MsCell g, const float *__restrict__ xyz, const uint8_t *__restrict__ rgb, unsigned n,
                                                            const unsigned *__restrict__ slot, const unsigned *__restrict__ leader,
                                                            unsigned *vmap, unsigned long long *__restrict__ acc) {
    const unsigned v = blockIdx.x * 256u + threadIdx.x;
    if (v >= n) return;
    const unsigned l = leader[slot[v]];
    const unsigned c = vmap[l];
    if (l != v) vmap[v] = c;
    double d[3], fi[3];
    ms_cell_of(g, xyz + 3ull * v, d, fi);
    unsigned long long *a = acc + 7ull * c;
    atomicAdd(a, 1ull);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const double r = d[k] - fi[k] * g.cell;
        const long long q = (long long)rint((r / g.cell) * MS_Q);
        atomicAdd(a + 1 + k, (unsigned long long)q);                   // two's complement: q may be slightly negative
    }
    if (rgb) {
#pragma unroll
        for (int k = 0; k < 3; ++k) atomicAdd(a + 4 + k, (unsigned long long)rgb[3ull * v + k]);
    }
}

// positions and colours, written by each cluster's leader at the cluster's number
__global__ __launch_bounds__(256) void ms_vert_write_kernel(MsCell g, const float *__restrict__ xyz, bool colours, unsigned n,
                                                            const unsigned *__restrict__ slot, const unsigned *__restrict__ leader,
                                                            const unsigned *__restrict__ vmap, const unsigned long long *__restrict__ acc,
                                                            float *__restrict__ out_xyz, uint8_t *__restrict__ out_rgb, unsigned long long cap) {
    const unsigned v = blockIdx.x * 256u + threadIdx.x;
    if (v >= n || leader[slot[v]] != v) return;
    const unsigned c = vmap[v];
    if (c >= cap) return;
    double d[3], fi[3];
    ms_cell_of(g, xyz + 3ull * v, d, fi);
    const unsigned long long *a = acc + 7ull * c;
    const unsigned long long cnt = a[0];
    const double den = (double)cnt * MS_Q;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const double f = (double)(long long)a[1 + k] / den;
        const double w = (fi[k] + f) * g.cell;
        out_xyz[3ull * c + k] = (float)(g.o[k] + w);
    }
    if (colours) {
#pragma unroll
        for (int k = 0; k < 3; ++k) out_rgb[3ull * c + k] = (uint8_t)((2ull * a[4 + k] + cnt) / (2ull * cnt));
    }
}

typedef __int128 i128;
typedef unsigned __int128 u128;
constexpr int MS_QWORDS = 18;                            // per cluster: (lo, hi) of A00 A01 A02 A11 A12 A22 b0 b1 b2

// dbl() of DESIGN.md section 4.2.3 (kernels_meshsmooth.hip's msm_dbl)
__device__ __forceinline__ double ms_dbl(i128 n) {
    const bool neg = n < 0;
    const u128 m = neg ? (u128)0 - (u128)n : (u128)n;
    const double d = (double)(u64)(m >> 64) * 18446744073709551616.0 + (double)(u64)m;
    return neg ? -d : d;
}

// rec (lo, hi) += t (H4: one carry per wrap of the low word; a zero word is not added)
__device__ __forceinline__ void ms_add128(u64 *rec, i128 t) {
    const u64 lo = (u64)(u128)t;
    u64 hi = (u64)((u128)t >> 64);
    if (lo) {
        const u64 old = atomicAdd(rec, lo);
        hi += old + lo < old ? 1ull : 0ull;
    }
    if (hi) atomicAdd(rec + 1, hi);
}

// qacc[18 c ..] += the plane quadric of triangle t seen from each of its corners' cells; info[4] += corners skipped by the span
// rule.  vert_map is final (the kernel before this one wrote it); every thread of the block reaches the wave sum at the end.
__global__ __launch_bounds__(256) void ms_quadric_kernel(MsCell g, const float *__restrict__ xyz, const unsigned *__restrict__ tri,
                                                         unsigned long long n_tri, const unsigned *__restrict__ vmap, u64 *qacc,
                                                         u64 *__restrict__ info) {
    const unsigned long long t = (unsigned long long)blockIdx.x * 256 + threadIdx.x;
    unsigned skipped = 0;
    if (t < n_tri) {
        int ci[3][3], h[3][3];                                         // cell index and 2^10-step coordinate of the corners
        unsigned c[3];
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const unsigned v = tri[3 * t + j];
            c[j] = vmap[v];
            double d[3], fi[3];
            ms_cell_of(g, xyz + 3ull * v, d, fi);
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                const double r = d[a] - fi[a] * g.cell;
                const long long q = (long long)rint((r / g.cell) * MS_Q);
                ci[j][a] = (int)fi[a];
                h[j][a] = (int)((q + 8192) >> 14);
            }
        }
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            // corners of one cluster share the frame and the term: the first of them adds mult times, the others nothing
            int mult = 1;
            bool first = true;
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                if (j < k && c[j] == c[k]) first = false;
                if (j > k && c[j] == c[k]) ++mult;
            }
            bool in_span = true;
            long long p[3][3];
#pragma unroll
            for (int j = 0; j < 3; ++j)
#pragma unroll
                for (int a = 0; a < 3; ++a) {
                    const int di = ci[j][a] - ci[k][a];
                    in_span = in_span && di >= -3 && di <= 3;
                    p[j][a] = (long long)di * 1024 + h[j][a];
                }
            if (!in_span) {
                ++skipped;
                continue;
            }
            if (!first) continue;
            long long e1[3], e2[3], N[3];
#pragma unroll
            for (int a = 0; a < 3; ++a) { e1[a] = p[1][a] - p[0][a]; e2[a] = p[2][a] - p[0][a]; }
            N[0] = e1[1] * e2[2] - e1[2] * e2[1];
            N[1] = e1[2] * e2[0] - e1[0] * e2[2];
            N[2] = e1[0] * e2[1] - e1[1] * e2[0];
            if (N[0] == 0 && N[1] == 0 && N[2] == 0) continue;         // zero area, or a vertex named twice: zeros
            const long long d = -(N[0] * p[0][0] + N[1] * p[0][1] + N[2] * p[0][2]);
            u64 *rec = qacc + (unsigned long long)MS_QWORDS * c[k];
            ms_add128(rec + 0, (i128)(mult * N[0] * N[0]));
            ms_add128(rec + 2, (i128)(mult * N[0] * N[1]));
            ms_add128(rec + 4, (i128)(mult * N[0] * N[2]));
            ms_add128(rec + 6, (i128)(mult * N[1] * N[1]));
            ms_add128(rec + 8, (i128)(mult * N[1] * N[2]));
            ms_add128(rec + 10, (i128)(mult * N[2] * N[2]));
#pragma unroll
            for (int a = 0; a < 3; ++a) ms_add128(rec + 12 + 2 * a, (i128)(mult * d) * (i128)N[a]);
        }
    }
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) skipped += __shfl_xor(skipped, s);
    if ((threadIdx.x & 63) == 0 && skipped) atomicAdd(info + 4, (u64)skipped);
}

__device__ __forceinline__ i128 ms_load128(const u64 *__restrict__ rec) { return (i128)(((u128)rec[1] << 64) | (u128)rec[0]); }

// x of (M + reg I) x = reg m - g in 2^10 steps per cell, clamped to the cell; false when the diagonal sums are all zero (mean rule)
__device__ __forceinline__ bool ms_quadric_solve(const u64 *__restrict__ rec, const double m[3], double reg, double x[3], bool &clamped) {
    const i128 A00 = ms_load128(rec), A11 = ms_load128(rec + 6), A22 = ms_load128(rec + 10);
    if (A00 == 0 && A11 == 0 && A22 == 0) return false;
    const double T = (ms_dbl(A00) + ms_dbl(A11)) + ms_dbl(A22);
    const double K00 = ms_dbl(A00) / T + reg, K01 = ms_dbl(ms_load128(rec + 2)) / T, K02 = ms_dbl(ms_load128(rec + 4)) / T;
    const double K11 = ms_dbl(A11) / T + reg, K12 = ms_dbl(ms_load128(rec + 8)) / T, K22 = ms_dbl(A22) / T + reg;
    double r[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) r[a] = reg * m[a] - ms_dbl(ms_load128(rec + 12 + 2 * a)) / T;
    const double c00 = K11 * K22 - K12 * K12, c01 = K02 * K12 - K01 * K22, c02 = K01 * K12 - K02 * K11;
    const double c11 = K00 * K22 - K02 * K02, c12 = K01 * K02 - K00 * K12, c22 = K00 * K11 - K01 * K01;
    const double det = (K00 * c00 + K01 * c01) + K02 * c02;
    x[0] = ((c00 * r[0] + c01 * r[1]) + c02 * r[2]) / det;
    x[1] = ((c01 * r[0] + c11 * r[1]) + c12 * r[2]) / det;
    x[2] = ((c02 * r[0] + c12 * r[1]) + c22 * r[2]) / det;
    // one step of refinement with the same adjugate: at rank 1 and 2 the cofactors and det cancel, and the first x carries it
    const double p0 = r[0] - ((K00 * x[0] + K01 * x[1]) + K02 * x[2]);
    const double p1 = r[1] - ((K01 * x[0] + K11 * x[1]) + K12 * x[2]);
    const double p2 = r[2] - ((K02 * x[0] + K12 * x[1]) + K22 * x[2]);
    x[0] = x[0] + ((c00 * p0 + c01 * p1) + c02 * p2) / det;
    x[1] = x[1] + ((c01 * p0 + c11 * p1) + c12 * p2) / det;
    x[2] = x[2] + ((c02 * p0 + c12 * p1) + c22 * p2) / det;
    clamped = false;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        if (!(x[a] >= 0.0)) { x[a] = 0.0; clamped = true; }            // (also what is no number)
        else if (x[a] > 1024.0) { x[a] = 1024.0; clamped = true; }
    }
    return true;
}

// ms_vert_write_kernel with the position from the cluster's quadric; info[5] += clusters placed by it, info[6] += clusters
// clamped: one add per block and word (nearly every wave holds a leader, and an add per wave on one address is what the launch
// then takes).  out_xyz == nullptr counts only (the capacity error still reports).  Every thread reaches the block sum.
__global__ __launch_bounds__(256) void ms_vert_write_quadric_kernel(MsCell g, double reg, const float *__restrict__ xyz, bool colours, unsigned n,
                                                                    const unsigned *__restrict__ slot, const unsigned *__restrict__ leader,
                                                                    const unsigned *__restrict__ vmap, const u64 *__restrict__ acc,
                                                                    const u64 *__restrict__ qacc, float *__restrict__ out_xyz,
                                                                    uint8_t *__restrict__ out_rgb, unsigned long long cap, u64 *__restrict__ info) {
    const unsigned v = blockIdx.x * 256u + threadIdx.x;
    bool placed = false, clamped = false;
    if (v < n && leader[slot[v]] == v) {
        const unsigned c = vmap[v];
        double d[3], fi[3], m[3], x[3];
        ms_cell_of(g, xyz + 3ull * v, d, fi);
        const u64 *a = acc + 7ull * c;
        const u64 cnt = a[0];
#pragma unroll
        for (int k = 0; k < 3; ++k) m[k] = (double)(long long)a[1 + k] / ((double)cnt * 16384.0);
        placed = ms_quadric_solve(qacc + (unsigned long long)MS_QWORDS * c, m, reg, x, clamped);
        if (out_xyz && c < cap) {
            const double den = (double)cnt * MS_Q;
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const double f = placed ? x[k] / 1024.0 : (double)(long long)a[1 + k] / den;
                const double w = (fi[k] + f) * g.cell;
                out_xyz[3ull * c + k] = (float)(g.o[k] + w);
            }
            if (colours) {
#pragma unroll
                for (int k = 0; k < 3; ++k) out_rgb[3ull * c + k] = (uint8_t)((2ull * a[4 + k] + cnt) / (2ull * cnt));
            }
        }
    }
    __shared__ unsigned sm[4];
    const unsigned both = block_sum((placed ? 1u : 0u) | (placed && clamped ? 1u << 16 : 0u), sm);      // (256 threads: two 16-bit counts)
    if (threadIdx.x == 0) {
        if (both & 0xFFFFu) atomicAdd(info + 5, (u64)(both & 0xFFFFu));
        if (both >> 16) atomicAdd(info + 6, (u64)(both >> 16));
    }
}

// the mapped triangle rotated so that its smallest index comes first; false when two indices are equal
__device__ __forceinline__ bool ms_canonical(const unsigned *__restrict__ tri, const unsigned *__restrict__ vmap, unsigned long long t,
                                             unsigned m[3], unsigned k[3]) {
    m[0] = vmap[tri[3 * t]]; m[1] = vmap[tri[3 * t + 1]]; m[2] = vmap[tri[3 * t + 2]];
    if (m[0] == m[1] || m[1] == m[2] || m[0] == m[2]) return false;
    if (m[0] < m[1] && m[0] < m[2]) { k[0] = m[0]; k[1] = m[1]; k[2] = m[2]; }
    else if (m[1] < m[2]) { k[0] = m[1]; k[1] = m[2]; k[2] = m[0]; }
    else { k[0] = m[2]; k[1] = m[0]; k[2] = m[1]; }
    return true;
}

__device__ __forceinline__ unsigned long long ms_triple_hash(const unsigned k[3]) {
    return kt_mix(kt_mix(((unsigned long long)k[1] << 32) | k[0]) + k[2]);
}

__global__ __launch_bounds__(256) void ms_tri_insert_kernel(const unsigned *__restrict__ tri, unsigned long long n_tri,
                                                            const unsigned *__restrict__ vmap, unsigned *ttab, unsigned long long mask) {
    const unsigned long long t = (unsigned long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= n_tri) return;
    unsigned m[3], k[3];
    if (!ms_canonical(tri, vmap, t, m, k)) return;
    unsigned long long h = ms_triple_hash(k) & mask;
    for (unsigned long long probe = 0; probe <= mask; ++probe) {       // (H3)
        unsigned cur = __hip_atomic_load(ttab + h, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (cur == MS_EMPTY) {
            cur = atomicCAS(ttab + h, MS_EMPTY, (unsigned)t);
            if (cur == MS_EMPTY) return;                               // the slot is this triple's from now on (H2)
        }
        unsigned om[3], ok[3];
        ms_canonical(tri, vmap, cur, om, ok);                          // (an occupant is never degenerate)
        if (ok[0] == k[0] && ok[1] == k[1] && ok[2] == k[2]) {
            atomicMin(ttab + h, (unsigned)t);                          // the first occurrence wins
            return;
        }
        h = (h + 1) & mask;
    }
}

// degenerate / duplicate / survivor of a triangle, from the finished table: walk t's probe sequence to the slot of its triple
__device__ __forceinline__ uint8_t ms_classify(const unsigned *__restrict__ tri, const unsigned *__restrict__ vmap, unsigned long long t,
                                               const unsigned *__restrict__ ttab, unsigned long long mask) {
    unsigned m[3], k[3];
    if (!ms_canonical(tri, vmap, t, m, k)) return MS_DEGENERATE;
    unsigned long long h = ms_triple_hash(k) & mask;
    for (unsigned long long probe = 0; probe <= mask; ++probe) {
        const unsigned cur = ttab[h];
        if (cur == (unsigned)t) return MS_SURVIVOR;
        if (cur == MS_EMPTY) break;                                    // (cannot happen: t's triple sits on this sequence)
        unsigned om[3], ok[3];
        ms_canonical(tri, vmap, cur, om, ok);
        if (ok[0] == k[0] && ok[1] == k[1] && ok[2] == k[2]) return MS_DUPLICATE;       // cur < t came first
        h = (h + 1) & mask;
    }
    return MS_DUPLICATE;
}

// flag[t], survivors per chunk, info[2] += degenerate, info[3] += duplicate
__global__ __launch_bounds__(256) void ms_tri_count_kernel(const unsigned *__restrict__ tri, unsigned long long n_tri,
                                                           const unsigned *__restrict__ vmap, const unsigned *__restrict__ ttab,
                                                           unsigned long long mask, uint8_t *__restrict__ flag,
                                                           unsigned *__restrict__ chunk_counts, unsigned long long *__restrict__ info) {
    __shared__ unsigned sm[4];
    unsigned ns = 0, ng = 0, nd = 0;
    for_chunk([&](unsigned long long t) {
        if (t < n_tri) {
            const uint8_t f = ms_classify(tri, vmap, t, ttab, mask);
            flag[t] = f;
            ns += f == MS_SURVIVOR ? 1u : 0u;
            ng += f == MS_DEGENERATE ? 1u : 0u;
            nd += f == MS_DUPLICATE ? 1u : 0u;
        }
    });
    ns = block_sum(ns, sm);
    ng = block_sum(ng, sm);
    nd = block_sum(nd, sm);
    if (threadIdx.x == 0) {
        chunk_counts[blockIdx.x] = ns;
        if (ng) atomicAdd(info + 2, (unsigned long long)ng);
        if (nd) atomicAdd(info + 3, (unsigned long long)nd);
    }
}

// survivors in input order, mapped but not rotated
__global__ __launch_bounds__(256) void ms_tri_write_kernel(const unsigned *__restrict__ tri, unsigned long long n_tri,
                                                           const unsigned *__restrict__ vmap, const uint8_t *__restrict__ flag,
                                                           const unsigned long long *__restrict__ offsets, unsigned *__restrict__ out_tri,
                                                           unsigned long long cap) {
    compact_chunk(
        n_tri, offsets, [&](unsigned long long t) { return flag[t] == MS_SURVIVOR ? 1u : 0u; },
        [&](unsigned long long t, unsigned long long o, unsigned) {
            if (o >= cap) return;
            out_tri[3 * o + 0] = vmap[tri[3 * t]]; out_tri[3 * o + 1] = vmap[tri[3 * t + 1]]; out_tri[3 * o + 2] = vmap[tri[3 * t + 2]];
        });
}

static MsCell ms_cell(double cell, const double o[3]) { return MsCell{cell, {o[0], o[1], o[2]}}; }

// info[1] = the number of vertices that are not finite or lie beyond 2^20 cells (the caller zeroed it)
int launch_ms_validate(hipStream_t s, double cell, const double o[3], const float *xyz, long long n_vert, unsigned long long *info) {
    if (n_vert <= 0) return TL3D_OK;
    hipLaunchKernelGGL(ms_validate_kernel, dim3(blocks_of((unsigned long long)n_vert, 256)), dim3(256), 0, s, ms_cell(cell, o), xyz,
                       (unsigned)n_vert, info);
    TL3D_HIP(hipGetLastError());
    return TL3D_OK;
}

// Vertices into clusters (validated input; keys / leader filled with 0xFF, vcap = kt_slots(n_vert) slots, acc with 0): slot, vert_map, the seven sums per
// cluster, leaders per chunk (vcounts) and their scan (voffsets, total behind the last chunk = the number of clusters).
int launch_ms_cluster(hipStream_t s, double cell, const double o[3], const float *xyz, const uint8_t *rgb, long long n_vert,
                      unsigned long long *keys, unsigned *leader, unsigned long long vcap, unsigned *slot, unsigned *vmap,
                      unsigned long long *acc, unsigned *vcounts, unsigned long long *voffsets) {
    if (n_vert <= 0) return TL3D_OK;
    const MsCell g = ms_cell(cell, o);
    const unsigned nv = (unsigned)n_vert, vb = blocks_of((unsigned long long)n_vert, 256), vchunks = chunks_of(n_vert);
    hipLaunchKernelGGL(ms_insert_kernel, dim3(vb), dim3(256), 0, s, g, xyz, nv, keys, leader, vcap - 1, slot);
    TL3D_HIP(hipGetLastError());
    hipLaunchKernelGGL(ms_leader_count_kernel, dim3(vchunks), dim3(256), 0, s, slot, leader, nv, vcounts);
    TL3D_HIP(hipGetLastError());
    int rc = launch_scan(s, vcounts, voffsets, (int)vchunks, voffsets + vchunks);
    if (rc) return rc;
    hipLaunchKernelGGL(ms_leader_write_kernel, dim3(vchunks), dim3(256), 0, s, slot, leader, nv, voffsets, vmap);
    TL3D_HIP(hipGetLastError());
    hipLaunchKernelGGL(ms_accumulate_kernel, dim3(vb), dim3(256), 0, s, g, xyz, rgb, nv, slot, leader, vmap, acc);
    TL3D_HIP(hipGetLastError());
    return TL3D_OK;
}

// qacc (zeroed, 18 words per vertex) += the corner quadrics of every triangle, info[4] += corners skipped; behind launch_ms_cluster
int launch_ms_quadrics(hipStream_t s, double cell, const double o[3], const float *xyz, const unsigned *tri, long long n_tri,
                       const unsigned *vmap, unsigned long long *qacc, unsigned long long *info) {
    if (n_tri <= 0) return TL3D_OK;
    hipLaunchKernelGGL(ms_quadric_kernel, dim3(blocks_of((unsigned long long)n_tri, 256)), dim3(256), 0, s, ms_cell(cell, o), xyz, tri,
                       (unsigned long long)n_tri, vmap, qacc, info);
    TL3D_HIP(hipGetLastError());
    return TL3D_OK;
}

// Triangles through vert_map into the table (filled with 0xFF), then flag[t], survivors per chunk (tcounts) and their scan,
// info[2] / info[3] = degenerate / duplicate
int launch_ms_triangles(hipStream_t s, const unsigned *tri, long long n_tri, const unsigned *vmap, unsigned *ttab, unsigned long long tcap,
                        uint8_t *flag, unsigned *tcounts, unsigned long long *toffsets, unsigned long long *info) {
    const unsigned tchunks = chunks_of(n_tri > 0 ? n_tri : 0);
    if (n_tri > 0) {
        hipLaunchKernelGGL(ms_tri_insert_kernel, dim3(blocks_of((unsigned long long)n_tri, 256)), dim3(256), 0, s, tri, (unsigned long long)n_tri,
                           vmap, ttab, tcap - 1);
        TL3D_HIP(hipGetLastError());
        hipLaunchKernelGGL(ms_tri_count_kernel, dim3(tchunks), dim3(256), 0, s, tri, (unsigned long long)n_tri, vmap, ttab, tcap - 1, flag,
                           tcounts, info);
        TL3D_HIP(hipGetLastError());
    }
    return launch_scan(s, tcounts, toffsets, (int)tchunks, toffsets + tchunks);         // (no triangle: the total is 0)
}

// qacc: the quadric sums (nullptr: mean placement); with them info[5] / info[6] += clusters placed by their quadric / clamped,
// and out_xyz == nullptr writes nothing and counts all the same
int launch_ms_write(hipStream_t s, double cell, const double o[3], const float *xyz, bool colours, long long n_vert, const unsigned *slot,
                    const unsigned *leader, const unsigned *vmap, const unsigned long long *acc, float *out_xyz, uint8_t *out_rgb,
                    unsigned long long vcap, const unsigned *tri, long long n_tri, const uint8_t *flag, const unsigned long long *toffsets,
                    unsigned *out_tri, unsigned long long tcap, const unsigned long long *qacc, double reg, unsigned long long *info) {
    if (n_vert > 0 && qacc) {
        hipLaunchKernelGGL(ms_vert_write_quadric_kernel, dim3(blocks_of((unsigned long long)n_vert, 256)), dim3(256), 0, s, ms_cell(cell, o), reg,
                           xyz, colours, (unsigned)n_vert, slot, leader, vmap, acc, qacc, out_xyz, out_rgb, vcap, info);
        TL3D_HIP(hipGetLastError());
    } else if (n_vert > 0 && vcap > 0) {
        hipLaunchKernelGGL(ms_vert_write_kernel, dim3(blocks_of((unsigned long long)n_vert, 256)), dim3(256), 0, s, ms_cell(cell, o), xyz, colours,
                           (unsigned)n_vert, slot, leader, vmap, acc, out_xyz, out_rgb, vcap);
        TL3D_HIP(hipGetLastError());
    }
    if (n_tri > 0 && tcap > 0) {
        hipLaunchKernelGGL(ms_tri_write_kernel, dim3(chunks_of(n_tri)), dim3(256), 0, s, tri, (unsigned long long)n_tri,
                           vmap, flag, toffsets, out_tri, tcap);
        TL3D_HIP(hipGetLastError());
    }
    return TL3D_OK;
}

}  // namespace tl3d
