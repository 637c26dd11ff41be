// kernels_meshsmooth.hip -- Taubin smoothing and area-weighted vertex normals of an indexed triangle mesh over its adjacency
// (tl3d_mesh_smooth_taubin, tl3d_mesh_vertex_normals).  No reference code: the reference has no mesh.
// The rules are ours (tests/mesh_smooth_reference.py restates them with Python integers):
//   Q(x) = (int64)rint((double)x * 2^24)  (exact product, halves to even; |x| <= 2^20 m, so |Q| <= 2^44)
//   neighbours: u and v, u != v, that one triangle names together; N(v) holds each once, k = |N(v)| is the valence
//   step with factor s, per axis a: D_a = sum_{j in N(v)} Q(x_j,a) - k Q(x_v,a) in exact integers (up to 2^76: __int128),
//       x'_a = (float)((double)x_a + s * (dbl(D_a) / ((double)k * 2^24))), every fp64 operation rounded once; k = 0 copies
//   iteration = a step with lambda, then a step with mu, Jacobi (each step reads one buffer and writes the other)
//   face vector of (a, b, c): F = (Q(p_b) - Q(p_a)) x (Q(p_c) - Q(p_a)) in exact integers (each component below 2^92)
//   vertex normal: N_v = sum of F over the triangles that name v (below 2^123), n = dbl(N_v) per component,
//       L = sqrt((n_x n_x + n_y n_y) + n_z n_z), normal = (float)(n_a / L); (0, 0, 0) when N_v = 0
//   dbl(N): |N| = hi 2^64 + lo, both unsigned; (double)hi * 2^64 + (double)lo, negated when N < 0
// Every sum is an exact integer held in the registers of the thread (or wave) that owns the vertex, so the order in which a row
// lists its entries does not matter and nothing is sorted.
//
// Passes, each its own launch on the context's stream (kernel boundaries are the ONLY ordering between them):
//   validate      largest triangle index (cc_validate_kernel), vertices that are not finite or beyond 2^20 m; nothing indexed
//                 runs before the host has looked at both
//   edge insert   one thread per triangle corner pair: key (min, max) into the edge table (keytab.h's kt_claim); the thread whose
//                 CAS wins adds 1 to both endpoints' valence and counts the edge
//   rows          per-chunk sums of the valences (64-bit) -> single-block scan -> row[v] (compact.h's skeleton on block_excl)
//   edge fill     one thread per table slot: an occupied slot appends each endpoint to the other's row through the row's cursor
//   step          one thread per vertex gathers its row (a row longer than MSM_LONG_ROW is walked by the whole wave and summed by
//                 shuffles), 2 * iterations launches, no atomics but the OR of the divergence flag; a step that finds the flag of
//                 the step before it set copies its input through
//   normals       corner count -> rows -> corner fill (triangle ids per vertex) -> the same gather over incident triangles
//
// Proof obligations (numbering of DESIGN.md section 4.2.2).  H1, H3 and H5 of the edge table are keytab.h's and are kept there: a
// triangle brings at most three keys, 3 n_tri in all, into kt_slots(3 n_tri) slots.  The lines that are this file's own:
//   H4  results come only from integer add.             valence, cursors, edge count: atomicAdd; flags: atomicOr.  No float atomics.
//   H6  the order of a row may differ from run to run.  a row is only ever summed, in exact integers.
//   B1  a row is never written beyond its end.          valence[v] counts exactly the keys that name v (one winner per key), and the
//                                                       fill appends once per key and endpoint; the corner rows likewise (one count
//                                                       and one append per corner).  The fills ALSO compare the cursor with the count.
#include "keytab.h"

namespace tl3d {

typedef __int128 i128;
typedef unsigned __int128 u128;

constexpr double MSM_Q = 16777216.0;                     // 2^24 steps per metre
constexpr float MSM_RANGE = 1048576.0f;                  // |x| <= 2^20 m
constexpr unsigned MSM_LONG_ROW = 64;                    // rows longer than this are gathered by the wave

__device__ __forceinline__ long long msm_q(float x) { return (long long)rint((double)x * MSM_Q); }

__device__ __forceinline__ double msm_dbl(i128 n) {
    const bool neg = n < 0;
    const u128 m = neg ? (u128)0 - (u128)n : (u128)n;
    const double d = (double)(u64)(m >> 64) * 18446744073709551616.0 + (double)(u64)m;
    return neg ? -d : d;
}

// the sum of v over the wave, in every lane
__device__ __forceinline__ i128 msm_wave_sum(i128 v) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
        const u64 lo = __shfl_xor((u64)(u128)v, d), hi = __shfl_xor((u64)((u128)v >> 64), d);
        v += (i128)(((u128)hi << 64) | (u128)lo);
    }
    return v;
}

// info[1] += coordinates' vertices that are not finite or lie beyond 2^20 m
__global__ __launch_bounds__(256) void msm_validate_kernel(const float *__restrict__ xyz, unsigned n, u64 *__restrict__ info) {
    const unsigned v = blockIdx.x * 256u + threadIdx.x;
    bool bad = false;
    if (v < n) {
#pragma unroll
        for (int a = 0; a < 3; ++a) bad = bad || !(fabsf(xyz[3ull * v + a]) <= MSM_RANGE);          // true for NaN and for an infinity
    }
    wave_count(bad, info + 1);
}

// (every index is below n_vert: the host has seen info[0])
__global__ __launch_bounds__(256) void msm_edge_insert_kernel(const unsigned *__restrict__ tri, u64 n_pairs, u64 *keys, u64 mask,
                                                              unsigned *deg, u64 *__restrict__ info) {
    const u64 e = (u64)blockIdx.x * 256 + threadIdx.x;
    bool won = false;
    if (e < n_pairs) {
        const u64 t = e / 3;
        const unsigned c = (unsigned)(e - 3 * t);
        const unsigned u = tri[e], v = tri[3 * t + (c == 2 ? 0 : c + 1)];
        if (u != v) {
            kt_claim(keys, mask, ((u64)min(u, v) << 32) | (u64)max(u, v), won);         // (two indices below 2^31: never KT_EMPTY)
            if (won) {
                atomicAdd(deg + u, 1u);
                atomicAdd(deg + v, 1u);
            }
        }
    }
    wave_count(won, info + 2);
}

__global__ __launch_bounds__(256) void msm_row_count_kernel(const unsigned *__restrict__ cnt, unsigned n, u64 *__restrict__ chunk_counts) {
    __shared__ u64 sm[4];
    u64 c = 0;
    for_chunk([&](u64 v) {
        if (v < n) c += cnt[v];
    });
    c = block_sum(c, sm);
    if (threadIdx.x == 0) chunk_counts[blockIdx.x] = c;
}

// row[v] = the sum of cnt[] in front of v; cursor[v] = 0
__global__ __launch_bounds__(256) void msm_row_write_kernel(const unsigned *__restrict__ cnt, unsigned n, const u64 *__restrict__ offsets,
                                                            u64 *__restrict__ row, unsigned *__restrict__ cursor) {
    __shared__ u64 sm[4];
    u64 run = offsets[blockIdx.x];
    for_chunk([&](u64 v) {                                               // (the barrier rule: every thread scans, a vertex beyond the end counts 0)
        const u64 c = v < n ? (u64)cnt[v] : 0ull;
        u64 total;
        const u64 ex = block_excl(c, sm, total);
        if (v < n) {
            row[v] = run + ex;
            cursor[v] = 0u;
        }
        run += total;
    });
}

__global__ __launch_bounds__(256) void msm_edge_fill_kernel(const u64 *__restrict__ keys, u64 slots, const unsigned *__restrict__ deg,
                                                            const u64 *__restrict__ row, unsigned *cursor, unsigned *__restrict__ nbr) {
    const u64 h = (u64)blockIdx.x * 256 + threadIdx.x;
    if (h >= slots) return;
    const u64 key = keys[h];
    if (key == KT_EMPTY) return;
    const unsigned u = (unsigned)(key >> 32), v = (unsigned)key;
    unsigned p = atomicAdd(cursor + u, 1u);
    if (p < deg[u]) nbr[row[u] + p] = v;                                 // (B1: always)
    p = atomicAdd(cursor + v, 1u);
    if (p < deg[v]) nbr[row[v] + p] = u;
}

// one step: out = in + s * (mean of the neighbours - in), by the contract above; *flag_out |= 1 when a result leaves the range.
// *flag_in is the word the step before this one reported through (nobody writes it during this launch): once it is set, `in` holds
// a coordinate Q cannot take, so this and every later step copies its input through and passes the flag on -- Q is never fed
// a value beyond 2^20 m.
__global__ __launch_bounds__(256) void msm_step_kernel(const float *__restrict__ in, float *__restrict__ out, unsigned n,
                                                       const unsigned *__restrict__ deg, const u64 *__restrict__ row,
                                                       const unsigned *__restrict__ nbr, double s, const u64 *__restrict__ flag_in,
                                                       u64 *__restrict__ flag_out) {
    const unsigned v = blockIdx.x * 256u + threadIdx.x;
    const unsigned lane = threadIdx.x & 63;
    if (*flag_in) {                                                      // (uniform over the launch)
        if (v < n) {
#pragma unroll
            for (int a = 0; a < 3; ++a) out[3ull * v + a] = in[3ull * v + a];
        }
        if (threadIdx.x == 0 && blockIdx.x == 0) atomicOr(flag_out, 1ull);
        return;
    }
    u64 r0 = 0;
    unsigned k = 0;
    if (v < n) {
        r0 = row[v];
        k = deg[v];
    }
    i128 S[3] = {0, 0, 0};
    const bool lng = k > MSM_LONG_ROW;
    if (!lng) {
        for (unsigned j = 0; j < k; ++j) {
            const float *p = in + 3ull * nbr[r0 + j];
#pragma unroll
            for (int a = 0; a < 3; ++a) S[a] += msm_q(p[a]);
        }
    }
    // long rows, one after the other, by all 64 lanes (lanes beyond the end take part: no return above)
    for (u64 m = __ballot(lng); m; m &= m - 1) {
        const int owner = __ffsll((long long)m) - 1;
        const u64 o0 = __shfl(r0, owner);
        const unsigned ok = __shfl(k, owner);
        i128 P[3] = {0, 0, 0};
        for (unsigned j = lane; j < ok; j += 64) {
            const float *p = in + 3ull * nbr[o0 + j];
#pragma unroll
            for (int a = 0; a < 3; ++a) P[a] += msm_q(p[a]);
        }
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            P[a] = msm_wave_sum(P[a]);
            if ((int)lane == owner) S[a] = P[a];
        }
    }
    bool bad = false;
    if (v < n) {
        const double den = (double)k * MSM_Q;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const float x = in[3ull * v + a];
            float y = x;
            if (k) {
                const i128 D = S[a] - (i128)k * (i128)msm_q(x);
                const double t = msm_dbl(D) / den;
                const double w = s * t;
                y = (float)((double)x + w);
            }
            out[3ull * v + a] = y;
            bad = bad || !(fabsf(y) <= MSM_RANGE);
        }
    }
    if (__ballot(bad) && lane == 0) atomicOr(flag_out, 1ull);
}

// cnt[v] += 1 per corner that names v
__global__ __launch_bounds__(256) void msm_corner_count_kernel(const unsigned *__restrict__ tri, u64 n_corners, unsigned *cnt) {
    const u64 e = (u64)blockIdx.x * 256 + threadIdx.x;
    if (e < n_corners) atomicAdd(cnt + tri[e], 1u);
}

__global__ __launch_bounds__(256) void msm_corner_fill_kernel(const unsigned *__restrict__ tri, u64 n_corners, const unsigned *__restrict__ cnt,
                                                              const u64 *__restrict__ row, unsigned *cursor, unsigned *__restrict__ inc) {
    const u64 e = (u64)blockIdx.x * 256 + threadIdx.x;
    if (e >= n_corners) return;
    const unsigned v = tri[e];
    const unsigned p = atomicAdd(cursor + v, 1u);
    if (p < cnt[v]) inc[row[v] + p] = (unsigned)(e / 3);                  // (B1: always)
}

// N += the face vector of triangle t
__device__ __forceinline__ void msm_face_add(const float *__restrict__ xyz, const unsigned *__restrict__ tri, u64 t, i128 N[3]) {
    const float *pa = xyz + 3ull * tri[3 * t], *pb = xyz + 3ull * tri[3 * t + 1], *pc = xyz + 3ull * tri[3 * t + 2];
    long long e1[3], e2[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const long long qa = msm_q(pa[a]);
        e1[a] = msm_q(pb[a]) - qa;
        e2[a] = msm_q(pc[a]) - qa;
    }
    N[0] += (i128)e1[1] * e2[2] - (i128)e1[2] * e2[1];
    N[1] += (i128)e1[2] * e2[0] - (i128)e1[0] * e2[2];
    N[2] += (i128)e1[0] * e2[1] - (i128)e1[1] * e2[0];
}

// info[3] += vertices whose normal is (0, 0, 0)
__global__ __launch_bounds__(256) void msm_normal_kernel(const float *__restrict__ xyz, const unsigned *__restrict__ tri, unsigned n,
                                                         const unsigned *__restrict__ cnt, const u64 *__restrict__ row,
                                                         const unsigned *__restrict__ inc, float *__restrict__ out, u64 *__restrict__ info) {
    const unsigned v = blockIdx.x * 256u + threadIdx.x;
    const unsigned lane = threadIdx.x & 63;
    u64 r0 = 0;
    unsigned k = 0;
    if (v < n) {
        r0 = row[v];
        k = cnt[v];
    }
    i128 N[3] = {0, 0, 0};
    const bool lng = k > MSM_LONG_ROW;
    if (!lng)
        for (unsigned j = 0; j < k; ++j) msm_face_add(xyz, tri, inc[r0 + j], N);
    for (u64 m = __ballot(lng); m; m &= m - 1) {
        const int owner = __ffsll((long long)m) - 1;
        const u64 o0 = __shfl(r0, owner);
        const unsigned ok = __shfl(k, owner);
        i128 P[3] = {0, 0, 0};
        for (unsigned j = lane; j < ok; j += 64) msm_face_add(xyz, tri, inc[o0 + j], P);
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            P[a] = msm_wave_sum(P[a]);
            if ((int)lane == owner) N[a] = P[a];
        }
    }
    bool zero = false;
    if (v < n) {
        zero = N[0] == 0 && N[1] == 0 && N[2] == 0;
        float r[3] = {0.0f, 0.0f, 0.0f};
        if (!zero) {
            const double nx = msm_dbl(N[0]), ny = msm_dbl(N[1]), nz = msm_dbl(N[2]);
            const double L = sqrt((nx * nx + ny * ny) + nz * nz);
            r[0] = (float)(nx / L); r[1] = (float)(ny / L); r[2] = (float)(nz / L);
        }
#pragma unroll
        for (int a = 0; a < 3; ++a) out[3ull * v + a] = r[a];
    }
    wave_count(zero, info + 3);
}

// info[1] = the number of vertices that are not finite or lie beyond 2^20 m (the caller zeroed it)
int launch_msm_validate(hipStream_t s, const float *xyz, long long n_vert, unsigned long long *info) {
    if (n_vert <= 0) return TL3D_OK;
    hipLaunchKernelGGL(msm_validate_kernel, dim3(blocks_of((u64)n_vert, 256)), dim3(256), 0, s, xyz, (unsigned)n_vert, info);
    TL3D_HIP(hipGetLastError());
    return TL3D_OK;
}

// The unique edges of validated triangles into the table (filled with 0xFF; `slots` = kt_slots(3 n_tri)): deg[v] (zeroed by
// the caller) = valence, info[2] = edges
int launch_msm_edges(hipStream_t s, const unsigned *tri, long long n_tri, unsigned long long *keys, unsigned long long slots, unsigned *deg,
                     unsigned long long *info) {
    if (n_tri <= 0) return TL3D_OK;
    const u64 n_pairs = 3ull * (u64)n_tri;
    hipLaunchKernelGGL(msm_edge_insert_kernel, dim3(blocks_of(n_pairs, 256)), dim3(256), 0, s, tri, n_pairs, keys, slots - 1, deg, info);
    TL3D_HIP(hipGetLastError());
    return TL3D_OK;
}

// row[v] = the entries in front of v's row for rows of cnt[v] entries, cursor[v] = 0; ccounts / coffs: [chunks] / [chunks + 1]
int launch_msm_rows(hipStream_t s, const unsigned *cnt, long long n_vert, unsigned long long *ccounts, unsigned long long *coffs,
                    unsigned long long *row, unsigned *cursor) {
    if (n_vert <= 0) return TL3D_OK;
    const int chunks = chunks_of((u64)n_vert);
    hipLaunchKernelGGL(msm_row_count_kernel, dim3(chunks), dim3(256), 0, s, cnt, (unsigned)n_vert, ccounts);
    TL3D_HIP(hipGetLastError());
    const int rc = launch_scan(s, ccounts, coffs, chunks, coffs + chunks);
    if (rc) return rc;
    hipLaunchKernelGGL(msm_row_write_kernel, dim3(chunks), dim3(256), 0, s, cnt, (unsigned)n_vert, coffs, row, cursor);
    TL3D_HIP(hipGetLastError());
    return TL3D_OK;
}

int launch_msm_edge_fill(hipStream_t s, const unsigned long long *keys, unsigned long long slots, const unsigned *deg,
                         const unsigned long long *row, unsigned *cursor, unsigned *nbr) {
    hipLaunchKernelGGL(msm_edge_fill_kernel, dim3(blocks_of(slots, 256)), dim3(256), 0, s, keys, slots, deg, row, cursor, nbr);
    TL3D_HIP(hipGetLastError());
    return TL3D_OK;
}

// flag_in: the divergence word of the step before (zero in front of the first), flag_out: this step's; two words taken in turn
int launch_msm_step(hipStream_t s, const float *in, float *out, long long n_vert, const unsigned *deg, const unsigned long long *row,
                    const unsigned *nbr, double factor, const unsigned long long *flag_in, unsigned long long *flag_out) {
    if (n_vert <= 0) return TL3D_OK;
    hipLaunchKernelGGL(msm_step_kernel, dim3(blocks_of((u64)n_vert, 256)), dim3(256), 0, s, in, out, (unsigned)n_vert, deg, row, nbr, factor,
                       flag_in, flag_out);
    TL3D_HIP(hipGetLastError());
    return TL3D_OK;
}

// The triangles that name each vertex (validated indices; cnt zeroed by the caller): cnt, row, inc [3 n_tri]
int launch_msm_corners(hipStream_t s, const unsigned *tri, long long n_tri, long long n_vert, unsigned *cnt, unsigned long long *ccounts,
                       unsigned long long *coffs, unsigned long long *row, unsigned *cursor, unsigned *inc) {
    if (n_tri <= 0 || n_vert <= 0) return TL3D_OK;
    const u64 n_corners = 3ull * (u64)n_tri;
    hipLaunchKernelGGL(msm_corner_count_kernel, dim3(blocks_of(n_corners, 256)), dim3(256), 0, s, tri, n_corners, cnt);
    TL3D_HIP(hipGetLastError());
    const int rc = launch_msm_rows(s, cnt, n_vert, ccounts, coffs, row, cursor);
    if (rc) return rc;
    hipLaunchKernelGGL(msm_corner_fill_kernel, dim3(blocks_of(n_corners, 256)), dim3(256), 0, s, tri, n_corners, cnt, row, cursor, inc);
    TL3D_HIP(hipGetLastError());
    return TL3D_OK;
}

// info[3] = the vertices with a zero normal (the caller zeroed it)
int launch_msm_normals(hipStream_t s, const float *xyz, const unsigned *tri, long long n_vert, const unsigned *cnt, const unsigned long long *row,
                       const unsigned *inc, float *out, unsigned long long *info) {
    if (n_vert <= 0) return TL3D_OK;
    hipLaunchKernelGGL(msm_normal_kernel, dim3(blocks_of((u64)n_vert, 256)), dim3(256), 0, s, xyz, tri, (unsigned)n_vert, cnt, row, inc, out, info);
    TL3D_HIP(hipGetLastError());
    return TL3D_OK;
}

}  // namespace tl3d
