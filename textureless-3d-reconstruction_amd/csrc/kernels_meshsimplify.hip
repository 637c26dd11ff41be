// kernels_meshsimplify.hip -- vertex-clustering simplification of an indexed triangle mesh (tl3d_mesh_simplify_clusters; DESIGN.md
// section 4.2.2).  No reference code: the reference has no mesh.  The rules are ours (tests/mesh_simplify_reference.py restates them):
//   cell of a vertex, per axis, in fp64 with every operation rounded once: d = (double)x - o, i = floor(d / cell),
//   r = d - (double)i * cell, q = (int64)rint((r / cell) * 2^24); -2^20 <= i < 2^20; a cluster = the vertices of one (ix, iy, iz),
//   with a member count n, exact integer sums S = sum q and C = sum rgb; clusters are numbered in the order of their smallest member
//   (the leader); position = (float)(o + ((double)i + (double)S / ((double)n * 2^24)) * cell), colour = (2 C + n) / (2 n);
//   a triangle is mapped through vert_map, dropped when two mapped indices are equal (degenerate), and dropped when an earlier
//   triangle has the same canonical triple (its rotation with the smallest index first: duplicate); survivors keep input order.
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
//   tri insert    one thread per triangle: map, and unless degenerate its index into the triangle table (32-bit CAS EMPTY -> t, or
//                 atomicMin into a slot whose occupant has the same canonical triple)
//   tri classify  per chunk: degenerate / duplicate / survivor (the slot of its triple holds t itself) -> flag, counts
//   write         positions and colours per leader at its cluster number; surviving triangles at scanned offsets, mapped
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
//                                                       triangle slots: atomicMin.  No float atomics anywhere.
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

int launch_ms_write(hipStream_t s, double cell, const double o[3], const float *xyz, bool colours, long long n_vert, const unsigned *slot,
                    const unsigned *leader, const unsigned *vmap, const unsigned long long *acc, float *out_xyz, uint8_t *out_rgb,
                    unsigned long long vcap, const unsigned *tri, long long n_tri, const uint8_t *flag, const unsigned long long *toffsets,
                    unsigned *out_tri, unsigned long long tcap) {
    if (n_vert > 0 && vcap > 0) {
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
