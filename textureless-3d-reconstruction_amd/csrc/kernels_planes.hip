// kernels_planes.hip -- planar regions of a point list with normals (tl3d_segment_planes; the definition is in
// tl3d.h).  No reference code: the reference never segments its cloud.  The rules are ours: smoothness-constrained region growing
// (PCL's RegionGrowing) as connected components of a symmetric link predicate, and a planarity test on each component's exact
// integer moments (the question Open3D's detect_planar_patches answers).
// Everything below is a function of the input alone: the link predicate is symmetric in IEEE arithmetic, integer atomics (min / CAS
// towards the smaller root, add) commute, the moments are exact integers, and the compactions write at scanned offsets.
//
// Passes, each its own launch on the context's stream (kernel boundaries are the ONLY ordering between them; I5 of unionfind.h):
//   bounds      points_bounds_finite (kernels_cellgrid.hip); the host refuses a non-finite coordinate, |x| >= 2^22, and a box too wide for the 64-bit sums
//   index       the cell index of cellgrid.h over all points (cell_index_build); the fill leaves in slot order the point with its original index and,
//               beside it, its normal with the eligibility flag in w (an ineligible point is indexed and skipped by its flag)
//   init        parent[i] = i, count[i] = 0
//   link        one thread per sorted slot (the lanes of a wave are neighbours in space and walk the same runs); the rows of cells
//               that the box [p - radius, p + radius] meets are one run each; for every j < i in reach: the predicate once, unite(i, j)
//   flatten     parent -> labels
//   count       count[label] += 1 over the eligible points; a wave walks 1024 consecutive slots, sums its own label in registers and
//               adds once, other labels one add per distinct label and group; info[0] += eligible points
//   candidates  roots with count >= min_points -> order-preserving ids (compact.h); info[1] += roots with a point (the regions)
//   moments     the eligible points of the candidates, the same walk: e = Q(p) - Q(seed); the lanes of a wave that share a label are
//               summed by shuffles and one lane adds the sums to the candidate's record with 64-bit integer atomics
//   planes      one thread per candidate: the fp64 sequence of the definition, the acceptance test, the plane record
//   accepted    second compaction: accepted candidates -> plane numbers, records to their place
//   write       plane_id[i] through the two maps
#include <math.h>
#include <stdio.h>
#include <stdlib.h>

#include "api_host.h"
#include "cellgrid.h"
#include "compact.h"
#include "sym3_eigen.h"
#include "unionfind.h"

namespace tl3d {

typedef __int128 pl_i128;
typedef unsigned __int128 pl_u128;
typedef unsigned long long pl_u64;

constexpr double PL_Q = 1048576.0;                      // 2^20 steps per metre
constexpr double PL_RANGE = 4194304.0;                  // |x| < 2^22 m: |Q| < 2^42, |e| < 2^43, e * e < 2^86, a sum of 2^31 of them < 2^117
constexpr double PL_NCLAMP = 2147483648.0;              // |N| <= 2^31 (normal components beyond 2^11 are clamped): a sum of 2^31 fits 64 bits
constexpr double PL_SUM_RANGE = 4611686018427387904.0;  // 2^62: n * (the box's largest extent in steps + 1) stays below it, so sum e fits 64 bits
constexpr int PL_REC = 20;                              // 64-bit words per record: count, 3 of e, 6 x (lo, hi) of e e, 3 of N, 1 spare

struct PlaneArgs {
    double r2, rpad, min_cos, max_offset, max_rms;
    long long min_points;
    int signed_normals;
};

// what the fill leaves at slot pos: the point and its index, and its normal with w = 1 for an eligible point, 0 otherwise
struct EmitPointNormal {
    float4 *__restrict__ sorted;
    float4 *__restrict__ snrm;
    const float *__restrict__ nrm;
    const float *__restrict__ curv;     // null, or compared with max_curv (> 0)
    double max_curv;
    __device__ __forceinline__ void operator()(unsigned pos, long long i, const float *__restrict__ p) const {
        const float nx = nrm[3 * i], ny = nrm[3 * i + 1], nz = nrm[3 * i + 2];
        const double l2 = (double)nx * (double)nx + (double)ny * (double)ny + (double)nz * (double)nz;
        bool ok = l2 > 0.0 && l2 < INFINITY;                           // false for a NaN
        if (curv) ok = ok && (double)curv[i] <= max_curv;              // false for a NaN
        sorted[pos] = make_float4(p[0], p[1], p[2], __int_as_float((int)i));
        snrm[pos] = make_float4(nx, ny, nz, ok ? 1.0f : 0.0f);
    }
};

__global__ __launch_bounds__(256) void pl_init_kernel(unsigned *__restrict__ parent, unsigned *__restrict__ count, unsigned n) {
    const unsigned v = blockIdx.x * 256u + threadIdx.x;
    if (v < n) {
        parent[v] = v;
        count[v] = 0u;
    }
}

// The link predicate between eligible points i and j, d = p_j - p_i.  Symmetric bit for bit: d^2 and the normals' product do not
// change when i and j swap, and the two offsets swap places (negating d negates every product and every rounded sum exactly).
__device__ __forceinline__ bool pl_linked(const PlaneArgs &a, double dx, double dy, double dz, double d2, const float4 &ni, const float4 &nj) {
    if (!(d2 <= a.r2)) return false;
    const double ax = (double)ni.x, ay = (double)ni.y, az = (double)ni.z, bx = (double)nj.x, by = (double)nj.y, bz = (double)nj.z;
    double s = ax * bx + ay * by + az * bz;
    if (!a.signed_normals) s = fabs(s);
    if (!(s >= a.min_cos)) return false;
    const double oi = fabs(ax * dx + ay * dy + az * dz), oj = fabs(bx * dx + by * dy + bz * dz);
    return oi <= a.max_offset && oj <= a.max_offset;
}

// Reach: every j the predicate can link has |x_j - x_i| <= radius (1 + 2^-51) per axis (its square is one term of a sum of
// non-negative terms that is <= the rounded radius^2), which is below rpad = radius (1 + 2^-40); x_i +- rpad rounds monotonely and
// cell_u is monotone, so j's cell lies between the cells of x_i - rpad and x_i + rpad on every axis, whatever the cell size: that
// is the ceil(radius / cell) reach, 27 cells for cell = radius.
__global__ __launch_bounds__(256) void pl_link_kernel(CellGrid g, PlaneArgs a, long long n, const unsigned *__restrict__ start,
                                                      const float4 *__restrict__ sorted, const float4 *__restrict__ snrm, unsigned *parent) {
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= n) return;
    const float4 ni = snrm[t];
    if (ni.w == 0.0f) return;
    const float4 me = sorted[t];
    const unsigned i = (unsigned)__float_as_int(me.w);
    const double px = (double)me.x, py = (double)me.y, pz = (double)me.z;
    const int x0 = cell_clampi(cell_u(px - a.rpad, g.ox, g.inv_cell), g.nx), x1 = cell_clampi(cell_u(px + a.rpad, g.ox, g.inv_cell), g.nx);
    const int y0 = cell_clampi(cell_u(py - a.rpad, g.oy, g.inv_cell), g.ny), y1 = cell_clampi(cell_u(py + a.rpad, g.oy, g.inv_cell), g.ny);
    const int z0 = cell_clampi(cell_u(pz - a.rpad, g.oz, g.inv_cell), g.nz), z1 = cell_clampi(cell_u(pz + a.rpad, g.oz, g.inv_cell), g.nz);
    for (int z = z0; z <= z1; ++z)
        for (int y = y0; y <= y1; ++y) {
            const long long row = ((long long)z * g.ny + y) * g.nx;
            const unsigned s = start[row + x0], e = start[row + x1 + 1];
            for (unsigned q = s; q < e; ++q) {
                const float4 p = sorted[q];
                const unsigned j = (unsigned)__float_as_int(p.w);
                if (j >= i) continue;                                  // a pair is tested once, by its larger index
                const double dx = (double)p.x - px, dy = (double)p.y - py, dz = (double)p.z - pz;
                const double d2 = dx * dx + dy * dy + dz * dz;
                if (!(d2 <= a.r2)) continue;
                const float4 nj = snrm[q];
                if (nj.w == 0.0f) continue;
                if (pl_linked(a, dx, dy, dz, d2, ni, nj)) cc_unite(parent, i, j);
            }
        }
}

__global__ __launch_bounds__(256) void pl_flatten_kernel(unsigned *parent, unsigned n) {
    const unsigned v = blockIdx.x * 256u + threadIdx.x;
    if (v >= n) return;
    const unsigned r = cc_find(parent, v);
    if (r < v) atomicMin(parent + v, r);
}

// The count and the moments walk the sorted list a wave at a time, PL_RUN groups of 64 consecutive slots per wave.  Slots in cell order
// mostly share ONE label over such a stretch: the label of the wave's first eligible point is its "own" label, whose lanes add up in
// their own registers and are summed across the wave and added to memory once, at the end; a lane with another label goes through
// the readfirstlane + ballot peel of cc_count_kernel there and then, one add per distinct label.  (One add per group of 64 puts the
// 62 500 groups of a 4 M cloud with four planes on the same four records.)
constexpr int PL_RUN = 16;
constexpr unsigned PL_NONE = 0xFFFFFFFFu;               // no label: indices stay below 2^31

__global__ __launch_bounds__(256) void pl_count_kernel(long long n, const float4 *__restrict__ sorted, const float4 *__restrict__ snrm,
                                                       const unsigned *__restrict__ label, unsigned *__restrict__ count,
                                                       pl_u64 *__restrict__ info) {
    const long long base = ((((long long)blockIdx.x * 256 + threadIdx.x) >> 6) * PL_RUN) * 64;
    const int lane = threadIdx.x & 63;
    unsigned own = PL_NONE, n_own = 0, n_live = 0;
    for (int it = 0; it < PL_RUN; ++it) {                              // every lane stays for every round: the shuffles need all 64
        const long long t = base + it * 64 + lane;
        const bool live = t < n && snrm[t].w != 0.0f;
        unsigned l = 0;
        if (live) l = label[(unsigned)__float_as_int(sorted[t].w)];
        pl_u64 todo = __ballot(live);
        if (own == PL_NONE && todo) own = (unsigned)__shfl((int)l, __ffsll((long long)todo) - 1);
        const bool fast = live && l == own;
        n_live += live ? 1u : 0u;
        n_own += fast ? 1u : 0u;
        todo &= ~__ballot(fast);
        while (todo) {                                                 // wave-uniform: one round per other label
            const int leader = __ffsll((long long)todo) - 1;
            const unsigned first = (unsigned)__shfl((int)l, leader);
            const pl_u64 same = __ballot(live && l == first);
            if (lane == leader) atomicAdd(count + first, (unsigned)__popcll(same));
            todo &= ~same;
        }
    }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
        n_own += __shfl_xor(n_own, d);
        n_live += __shfl_xor(n_live, d);
    }
    if (lane == 0) {
        if (n_own) atomicAdd(count + own, n_own);
        if (n_live) atomicAdd(info + 0, (pl_u64)n_live);
    }
}

__device__ __forceinline__ bool pl_is_candidate(const unsigned *__restrict__ label, const unsigned *__restrict__ count, unsigned long long v,
                                                long long min_points) {
    return label[v] == (unsigned)v && (long long)count[v] >= min_points;     // (min_points >= 3: a root without an eligible point is none)
}

// candidates per chunk; info[1] += regions of any size
__global__ __launch_bounds__(256) void pl_cand_count_kernel(const unsigned *__restrict__ label, const unsigned *__restrict__ count, unsigned n,
                                                            long long min_points, unsigned *__restrict__ chunk_counts,
                                                            pl_u64 *__restrict__ info) {
    __shared__ unsigned sm[4];
    unsigned nc = 0, nr = 0;
    for_chunk([&](unsigned long long v) {
        if (v < n) {
            nr += label[v] == (unsigned)v && count[v] > 0u ? 1u : 0u;
            nc += pl_is_candidate(label, count, v, min_points) ? 1u : 0u;
        }
    });
    nc = block_sum(nc, sm);
    nr = block_sum(nr, sm);
    if (threadIdx.x == 0) {
        chunk_counts[blockIdx.x] = nc;
        if (nr) atomicAdd(info + 1, (pl_u64)nr);
    }
}

// candidate ids in ascending label: cand_id[root] = id, cand_seed[id] = root (at most n / min_points of them: cap)
__global__ __launch_bounds__(256) void pl_cand_write_kernel(const unsigned *__restrict__ label, const unsigned *__restrict__ count, unsigned n,
                                                            long long min_points, const pl_u64 *__restrict__ offsets,
                                                            unsigned *__restrict__ cand_id, unsigned *__restrict__ cand_seed, pl_u64 cap) {
    compact_chunk(
        n, offsets, [&](unsigned long long v) { return pl_is_candidate(label, count, v, min_points) ? 1u : 0u; },
        [&](unsigned long long v, unsigned long long o, unsigned) {
            if (o >= cap) return;
            cand_id[v] = (unsigned)o;
            cand_seed[o] = (unsigned)v;
        });
}

__device__ __forceinline__ long long pl_q(float x) { return llrint((double)x * PL_Q); }
__device__ __forceinline__ long long pl_qn(float x) { return llrint(fmin(fmax((double)x * PL_Q, -PL_NCLAMP), PL_NCLAMP)); }

// the sums of v over the wave, in every lane (msm_wave_sum of kernels_meshsmooth.hip, and its 64-bit sibling)
__device__ __forceinline__ pl_i128 pl_wave_sum(pl_i128 v) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
        const pl_u64 lo = __shfl_xor((pl_u64)(pl_u128)v, d), hi = __shfl_xor((pl_u64)((pl_u128)v >> 64), d);
        v += (pl_i128)(((pl_u128)hi << 64) | (pl_u128)lo);
    }
    return v;
}
__device__ __forceinline__ long long pl_wave_sum(long long v) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d);
    return v;
}

// rec[0..1] += v as one 128-bit integer.  Exact whatever the order of the adds: the low word ends as the sum of all low halves mod
// 2^64 (atomic adds commute); an add carries exactly when it wraps the low word, which its returned old value shows, and the number
// of wraps over all adds is floor(sum of the low halves / 2^64) in any order; the high word ends as the sum of the high halves and of
// those carries mod 2^64.  Together: the two's-complement sum mod 2^128, and the true sum is below 2^117 in magnitude.
__device__ __forceinline__ void pl_add128(pl_u64 *rec, pl_i128 v) {
    const pl_u64 lo = (pl_u64)(pl_u128)v, hi = (pl_u64)((pl_u128)v >> 64);
    const pl_u64 old = atomicAdd(rec, lo);
    const pl_u64 carry = old + lo < old ? 1ull : 0ull;
    if (hi + carry) atomicAdd(rec + 1, hi + carry);
}

struct PlSums {                                         // of one label: sum e, sum N, sum e e (xx, yy, zz, xy, xz, yz), count
    long long e[3], m[3];
    pl_i128 q[6];
    unsigned c;
};

// every lane's sums over the wave; `leader` adds them to the label's record
__device__ __forceinline__ void pl_flush(const PlSums &v, int lane, int leader, pl_u64 *rec) {
    long long e[3], m[3];
    pl_i128 q[6];
    unsigned c = v.c;
#pragma unroll
    for (int a = 0; a < 3; ++a) { e[a] = pl_wave_sum(v.e[a]); m[a] = pl_wave_sum(v.m[a]); }
#pragma unroll
    for (int a = 0; a < 6; ++a) q[a] = pl_wave_sum(v.q[a]);
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) c += __shfl_xor(c, d);
    if (lane == leader) {
        atomicAdd(rec + 0, (pl_u64)c);
#pragma unroll
        for (int a = 0; a < 3; ++a) {                                  // two's complement, mod 2^64; the true sums fit: planes_run refuses a box where they might not
            atomicAdd(rec + 1 + a, (pl_u64)e[a]);
            atomicAdd(rec + 16 + a, (pl_u64)m[a]);
        }
#pragma unroll
        for (int a = 0; a < 6; ++a) pl_add128(rec + 4 + 2 * a, q[a]);
    }
}

// The walk of pl_count_kernel: the wave's own label is summed in the lanes' registers over the PL_RUN groups (at most 16 terms
// each: no overflow) and flushed once; other labels flush per group.  Every lane of the wave stays to the end: a lane without a
// point of a candidate adds zeros.
__global__ __launch_bounds__(256) void pl_moments_kernel(long long n, long long min_points, const float *__restrict__ xyz,
                                                         const float4 *__restrict__ sorted, const float4 *__restrict__ snrm,
                                                         const unsigned *__restrict__ label, const unsigned *__restrict__ count,
                                                         const unsigned *__restrict__ cand_id, pl_u64 *__restrict__ records) {
    const long long base = ((((long long)blockIdx.x * 256 + threadIdx.x) >> 6) * PL_RUN) * 64;
    const int lane = threadIdx.x & 63;
    unsigned own = PL_NONE;
    PlSums acc = {};
    for (int it = 0; it < PL_RUN; ++it) {
        const long long t = base + it * 64 + lane;
        bool live = t < n;
        float4 me = make_float4(0.f, 0.f, 0.f, 0.f), nm = make_float4(0.f, 0.f, 0.f, 0.f);
        if (live) nm = snrm[t];
        live = live && nm.w != 0.0f;
        unsigned l = 0;
        if (live) {
            me = sorted[t];
            l = label[(unsigned)__float_as_int(me.w)];
            live = (long long)count[l] >= min_points;
        }
        PlSums v = {};
        if (live) {
            const float *sp = xyz + 3 * (size_t)l;                     // the seed: the region's smallest index
            v.e[0] = pl_q(me.x) - pl_q(sp[0]); v.e[1] = pl_q(me.y) - pl_q(sp[1]); v.e[2] = pl_q(me.z) - pl_q(sp[2]);
            v.m[0] = pl_qn(nm.x); v.m[1] = pl_qn(nm.y); v.m[2] = pl_qn(nm.z);
            v.q[0] = (pl_i128)v.e[0] * v.e[0]; v.q[1] = (pl_i128)v.e[1] * v.e[1]; v.q[2] = (pl_i128)v.e[2] * v.e[2];
            v.q[3] = (pl_i128)v.e[0] * v.e[1]; v.q[4] = (pl_i128)v.e[0] * v.e[2]; v.q[5] = (pl_i128)v.e[1] * v.e[2];
            v.c = 1u;
        }
        pl_u64 todo = __ballot(live);
        if (own == PL_NONE && todo) own = (unsigned)__shfl((int)l, __ffsll((long long)todo) - 1);
        const bool fast = live && l == own;
        if (fast) {
#pragma unroll
            for (int a = 0; a < 3; ++a) { acc.e[a] += v.e[a]; acc.m[a] += v.m[a]; }
#pragma unroll
            for (int a = 0; a < 6; ++a) acc.q[a] += v.q[a];
            acc.c += 1u;
        }
        todo &= ~__ballot(fast);
        while (todo) {                                                 // wave-uniform: one round per other label
            const int leader = __ffsll((long long)todo) - 1;
            const unsigned first = (unsigned)__shfl((int)l, leader);
            const bool mine = live && l == first;
            PlSums w = {};
            if (mine) w = v;
            pl_flush(w, lane, leader, records + (size_t)PL_REC * cand_id[first]);
            todo &= ~__ballot(mine);
        }
    }
    if (own != PL_NONE) pl_flush(acc, lane, 0, records + (size_t)PL_REC * cand_id[own]);      // (own is wave-uniform)
}

// msm_dbl of kernels_meshsmooth.hip: a 128-bit integer as a double (the high and the low half converted, then one sum)
__device__ __forceinline__ double pl_dbl(pl_u64 lo, pl_u64 hi) {
    const pl_i128 v = (pl_i128)(((pl_u128)hi << 64) | (pl_u128)lo);
    const bool neg = v < 0;
    const pl_u128 m = neg ? (pl_u128)0 - (pl_u128)v : (pl_u128)v;
    const double d = (double)(pl_u64)(m >> 64) * 18446744073709551616.0 + (double)(pl_u64)m;
    return neg ? -d : d;
}

// one thread per candidate: the fixed fp64 sequence of the definition on the exact sums
__global__ __launch_bounds__(256) void pl_planes_kernel(unsigned ncand, PlaneArgs a, const float *__restrict__ xyz,
                                                        const unsigned *__restrict__ cand_seed, const pl_u64 *__restrict__ records,
                                                        tl3d_plane *__restrict__ tmp, unsigned *__restrict__ accept) {
    const unsigned c = blockIdx.x * 256u + threadIdx.x;
    if (c >= ncand) return;
    const pl_u64 *rec = records + (size_t)PL_REC * c;
    const unsigned seed = cand_seed[c];
    const double cnt = (double)rec[0];
    const double sx = (double)(long long)rec[1], sy = (double)(long long)rec[2], sz = (double)(long long)rec[3];
    const double mx = sx / cnt, my = sy / cnt, mz = sz / cnt;
    double cov[6];
    cov[0] = pl_dbl(rec[4], rec[5]) - sx * sx / cnt;
    cov[1] = pl_dbl(rec[6], rec[7]) - sy * sy / cnt;
    cov[2] = pl_dbl(rec[8], rec[9]) - sz * sz / cnt;
    cov[3] = pl_dbl(rec[10], rec[11]) - sx * sy / cnt;
    cov[4] = pl_dbl(rec[12], rec[13]) - sx * sz / cnt;
    cov[5] = pl_dbl(rec[14], rec[15]) - sy * sz / cnt;
    double lam[3], nv[3];
    sym3_smallest(cov, lam, nv);
    const double dn = nv[0] * (double)(long long)rec[16] + nv[1] * (double)(long long)rec[17] + nv[2] * (double)(long long)rec[18];
    const bool flip = dn < 0.0;
    const double nx = flip ? -nv[0] : nv[0], ny = flip ? -nv[1] : nv[1], nz = flip ? -nv[2] : nv[2];
    const float *sp = xyz + 3 * (size_t)seed;
    const double inv_q = 1.0 / PL_Q;
    const double cx = ((double)pl_q(sp[0]) + mx) * inv_q, cy = ((double)pl_q(sp[1]) + my) * inv_q, cz = ((double)pl_q(sp[2]) + mz) * inv_q;
    const double rms = sqrt(fmax(lam[0], 0.0) / cnt) * inv_q;
    tl3d_plane p;
    p.normal[0] = nx; p.normal[1] = ny; p.normal[2] = nz;
    p.d = nx * cx + ny * cy + nz * cz;
    p.centroid[0] = cx; p.centroid[1] = cy; p.centroid[2] = cz;
    p.rms = rms;
    p.count = (int64_t)rec[0];
    p.seed = (int64_t)seed;
    tmp[c] = p;
    accept[c] = lam[2] > 0.0 && (!(a.max_rms > 0.0) || rms <= a.max_rms) ? 1u : 0u;
}

__global__ __launch_bounds__(256) void pl_acc_count_kernel(const unsigned *__restrict__ accept, unsigned ncand, unsigned *__restrict__ chunk_counts) {
    __shared__ unsigned sm[4];
    unsigned na = 0;
    for_chunk([&](unsigned long long c) {
        if (c < ncand) na += accept[c];
    });
    na = block_sum(na, sm);
    if (threadIdx.x == 0) chunk_counts[blockIdx.x] = na;
}

// plane numbers in ascending label; the records only when all of them fit (*total <= cap): a call short of capacity writes none
__global__ __launch_bounds__(256) void pl_acc_write_kernel(const unsigned *__restrict__ accept, unsigned ncand, const pl_u64 *__restrict__ offsets,
                                                           const pl_u64 *__restrict__ total, pl_u64 cap, const tl3d_plane *__restrict__ tmp,
                                                           int *__restrict__ cand_plane, tl3d_plane *__restrict__ planes) {
    const bool fits = *total <= cap;
    compact_chunk(
        ncand, offsets,
        [&](unsigned long long c) {
            const unsigned acc = accept[c];
            if (!acc) cand_plane[c] = -1;
            return acc;
        },
        [&](unsigned long long c, unsigned long long o, unsigned) {
            cand_plane[c] = (int)o;
            if (fits) planes[o] = tmp[c];
        });
}

__global__ __launch_bounds__(256) void pl_write_kernel(long long n, long long min_points, const float4 *__restrict__ sorted,
                                                       const float4 *__restrict__ snrm, const unsigned *__restrict__ label,
                                                       const unsigned *__restrict__ count, const unsigned *__restrict__ cand_id,
                                                       const int *__restrict__ cand_plane, int *__restrict__ plane_id) {
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= n) return;
    const unsigned i = (unsigned)__float_as_int(sorted[t].w);
    int id = -1;
    if (snrm[t].w != 0.0f) {
        const unsigned l = label[i];
        if ((long long)count[l] >= min_points) id = cand_plane[cand_id[l]];
    }
    plane_id[i] = id;
}

// The passes' device times for tools/bench_cloud_planes.py: the experiments flavour, with TL3D_PLANES_TRACE=<file>, brackets the
// passes with events and appends one line of "name ms" pairs per call; the default library has an empty mark().
struct PlTrace {
#ifdef TL3D_EXPERIMENTS
    static constexpr int MAX = 12;
    hipStream_t s;
    const char *path = getenv("TL3D_PLANES_TRACE");
    hipEvent_t ev[MAX];
    const char *name[MAX];
    int n = 0;
    explicit PlTrace(hipStream_t s_) : s(s_) {}
    void mark(const char *what) {
        if (!path || n == MAX || hipEventCreate(&ev[n]) != hipSuccess) return;
        (void)hipEventRecord(ev[n], s);
        name[n++] = what;
    }
    ~PlTrace() {                                           // (the call has waited for the stream)
        FILE *f = path && n > 1 ? fopen(path, "a") : nullptr;
        for (int i = 1; i < n && f; ++i) {
            float ms = 0.f;
            (void)hipEventElapsedTime(&ms, ev[i - 1], ev[i]);
            fprintf(f, "%s %.4f%s", name[i], ms, i + 1 < n ? " " : "\n");
        }
        if (f) fclose(f);
        for (int i = 0; i < n; ++i) (void)hipEventDestroy(ev[i]);
    }
#else
    explicit PlTrace(hipStream_t) {}
    void mark(const char *) {}
#endif
};

// Every pointer is device memory but planes_hd (host or device, plane_cap records, may be null with plane_cap 0) and counts (host).
// counts: eligible points, regions, candidates, planes.  *short_cap: planes > plane_cap (plane_id and counts are written, no record).
// Waits for the stream at the bounds, at the candidate count and at the end.
int planes_run(tl3d_ctx *ctx, const float *xyz, const float *nrm, const float *curv, long long n, const tl3d_plane_params &prm, double cell,
               int *plane_id, tl3d_plane *planes_hd, long long plane_cap, long long counts[4], bool *short_cap) {
    hipStream_t s = ctx->stream;
    *short_cap = false;
    double mn[3], mx[3];
    unsigned long long bad = 0;
    int rc = points_bounds_finite(ctx, xyz, n, mn, mx, &bad);
    if (rc) return rc;
    if (bad) return set_err(TL3D_E_INVALID, "%llu points have a non-finite coordinate", bad);
    for (int a = 0; a < 3; ++a)
        if (!(fabs(mn[a]) < PL_RANGE && fabs(mx[a]) < PL_RANGE))
            return set_err(TL3D_E_INVALID, "coordinates reach %g m: plane segmentation needs |x| < 2^22 m", fmax(fabs(mn[a]), fabs(mx[a])));
    // |e_a| <= the box's extent on axis a in steps, + 1 for the two roundings; n of them must fit the 64-bit sums of sum e with room
    const double ext = fmax(mx[0] - mn[0], fmax(mx[1] - mn[1], mx[2] - mn[2]));
    if (!((double)n * (ext * PL_Q + 1.0) < PL_SUM_RANGE))
        return set_err(TL3D_E_INVALID, "%lld points over %g m: plane segmentation needs n * (extent * 2^20 + 1) < 2^62", n, ext);
    CellGrid g;
    cell_grid_fit(mn, mx, cell, &g);
    const size_t maxc = (size_t)(n / prm.min_points);                  // candidates have min_points points of their own each
    const size_t pchunks = (size_t)chunks_of((unsigned long long)n), cchunks = (size_t)chunks_of(maxc);
    const size_t outc = std::min((size_t)plane_cap, maxc);
    size_t bytes[20] = {0, 0, 0, 0,                              // 0-3 the index's tables (cell_table_bytes, below)
                        (size_t)n * sizeof(float4),              // 4 sorted      the fill, every slot
                        (size_t)n * sizeof(float4),              // 5 snrm        the fill, every slot
                        (size_t)n * sizeof(unsigned),            // 6 parent      init
                        (size_t)n * sizeof(unsigned),            // 7 count       init
                        (size_t)n * sizeof(unsigned),            // 8 cand_id     candidate roots only; read at candidate roots only
                        (pchunks + 1) * sizeof(unsigned),        // 9 point chunk counts
                        (pchunks + 1) * sizeof(pl_u64),          // 10 point chunk offsets and the total behind them
                        maxc * sizeof(unsigned),                 // 11 cand_seed
                        maxc * PL_REC * sizeof(pl_u64),          // 12 records    memset for the candidates there are
                        maxc * sizeof(tl3d_plane),               // 13 tmp planes planes kernel, every candidate
                        maxc * sizeof(unsigned),                 // 14 accept     planes kernel, every candidate
                        maxc * sizeof(int),                      // 15 cand_plane accepted write, every candidate
                        (cchunks + 1) * sizeof(unsigned),        // 16 candidate chunk counts
                        (cchunks + 1) * sizeof(pl_u64),          // 17 candidate chunk offsets and the total
                        outc * sizeof(tl3d_plane),               // 18 the records on their way out
                        8 * sizeof(pl_u64)};                     // 19 info       memset
    cell_table_bytes(cell_grid_cells(g), bytes);
    void *p[20];
    rc = scratch_carve(ctx, 0, bytes, 20, p, "plane segmentation scratch");
    if (rc) return rc;
    const CellTables t = CellTables::at(p);
    const unsigned *start = t.start;
    float4 *sorted = (float4 *)p[4], *snrm = (float4 *)p[5];
    unsigned *parent = (unsigned *)p[6], *count = (unsigned *)p[7], *cand_id = (unsigned *)p[8], *pcounts = (unsigned *)p[9];
    pl_u64 *poffs = (pl_u64 *)p[10];
    unsigned *cand_seed = (unsigned *)p[11];
    pl_u64 *records = (pl_u64 *)p[12];
    tl3d_plane *tmp = (tl3d_plane *)p[13];
    unsigned *accept = (unsigned *)p[14];
    int *cand_plane = (int *)p[15];
    unsigned *ccounts = (unsigned *)p[16];
    pl_u64 *coffs = (pl_u64 *)p[17];
    tl3d_plane *planes_dev = (tl3d_plane *)p[18];
    pl_u64 *info = (pl_u64 *)p[19];

    PlaneArgs a;
    a.r2 = prm.radius * prm.radius;
    a.rpad = prm.radius * (1.0 + 9.094947017729282e-13);              // 2^-40
    a.min_cos = prm.min_cos;
    a.max_offset = prm.max_offset;
    a.max_rms = prm.max_rms;
    a.min_points = prm.min_points;
    a.signed_normals = prm.signed_normals != 0;
    const bool use_curv = curv != nullptr && prm.max_curvature > 0.0;

    PlTrace trace(s);
    trace.mark("start");
    TL3D_HIP(hipMemsetAsync(info, 0, 8 * sizeof(pl_u64), s));
    rc = cell_index_build(s, g, xyz, n, t, true, EmitPointNormal{sorted, snrm, nrm, use_curv ? curv : nullptr, prm.max_curvature});
    if (rc) return rc;
    TL3D_HIP(hipGetLastError());
    const unsigned nb = (unsigned)((n + 255) / 256), un = (unsigned)n;
    trace.mark("index");
    hipLaunchKernelGGL(pl_init_kernel, dim3(nb), dim3(256), 0, s, parent, count, un);
    TL3D_HIP(hipGetLastError());
    hipLaunchKernelGGL(pl_link_kernel, dim3(nb), dim3(256), 0, s, g, a, n, start, sorted, snrm, parent);
    TL3D_HIP(hipGetLastError());
    trace.mark("init_link");
    hipLaunchKernelGGL(pl_flatten_kernel, dim3(nb), dim3(256), 0, s, parent, un);
    TL3D_HIP(hipGetLastError());
    const unsigned rb = (unsigned)((n + 256 * PL_RUN - 1) / (256 * PL_RUN));       // a wave walks PL_RUN groups of 64 slots
    hipLaunchKernelGGL(pl_count_kernel, dim3(rb), dim3(256), 0, s, n, sorted, snrm, parent, count, info);
    TL3D_HIP(hipGetLastError());
    trace.mark("flatten_count");
    hipLaunchKernelGGL(pl_cand_count_kernel, dim3((unsigned)pchunks), dim3(256), 0, s, parent, count, un, a.min_points, pcounts, info);
    TL3D_HIP(hipGetLastError());
    rc = launch_scan(s, pcounts, poffs, (int)pchunks, poffs + pchunks);
    if (rc) return rc;
    hipLaunchKernelGGL(pl_cand_write_kernel, dim3((unsigned)pchunks), dim3(256), 0, s, parent, count, un, a.min_points, poffs, cand_id, cand_seed,
                       (pl_u64)maxc);
    TL3D_HIP(hipGetLastError());
    trace.mark("candidates");
    pl_u64 h_info[2] = {0, 0}, h_cand = 0, h_planes = 0;
    TL3D_HIP(hipMemcpyAsync(h_info, info, sizeof(h_info), hipMemcpyDeviceToHost, s));
    TL3D_HIP(hipMemcpyAsync(&h_cand, poffs + pchunks, sizeof(h_cand), hipMemcpyDeviceToHost, s));
    TL3D_HIP(hipStreamSynchronize(s));
    if (h_cand > maxc) return set_err(TL3D_E_STATE, "%llu candidate regions of %lld points among %lld points", h_cand, a.min_points, n);
    const unsigned ncand = (unsigned)h_cand;
    if (ncand) {
        const unsigned cb = (unsigned)((ncand + 255) / 256), cc = (unsigned)chunks_of(ncand);
        TL3D_HIP(hipMemsetAsync(records, 0, (size_t)ncand * PL_REC * sizeof(pl_u64), s));
        hipLaunchKernelGGL(pl_moments_kernel, dim3(rb), dim3(256), 0, s, n, a.min_points, xyz, sorted, snrm, parent, count, cand_id, records);
        TL3D_HIP(hipGetLastError());
        trace.mark("moments");
        hipLaunchKernelGGL(pl_planes_kernel, dim3(cb), dim3(256), 0, s, ncand, a, xyz, cand_seed, records, tmp, accept);
        TL3D_HIP(hipGetLastError());
        hipLaunchKernelGGL(pl_acc_count_kernel, dim3(cc), dim3(256), 0, s, accept, ncand, ccounts);
        TL3D_HIP(hipGetLastError());
        rc = launch_scan(s, ccounts, coffs, (int)cc, coffs + cc);
        if (rc) return rc;
        hipLaunchKernelGGL(pl_acc_write_kernel, dim3(cc), dim3(256), 0, s, accept, ncand, coffs, coffs + cc, (pl_u64)outc, tmp, cand_plane, planes_dev);
        TL3D_HIP(hipGetLastError());
        TL3D_HIP(hipMemcpyAsync(&h_planes, coffs + cc, sizeof(h_planes), hipMemcpyDeviceToHost, s));
        trace.mark("planes_accepted");
    }
    hipLaunchKernelGGL(pl_write_kernel, dim3(nb), dim3(256), 0, s, n, a.min_points, sorted, snrm, parent, count, cand_id, cand_plane, plane_id);
    TL3D_HIP(hipGetLastError());
    trace.mark("write");
    TL3D_HIP(hipStreamSynchronize(s));
    counts[0] = (long long)h_info[0];
    counts[1] = (long long)h_info[1];
    counts[2] = (long long)h_cand;
    counts[3] = (long long)h_planes;
    if ((long long)h_planes > plane_cap) {
        *short_cap = true;
        return TL3D_OK;
    }
    if (h_planes) TL3D_HIP(hipMemcpy(planes_hd, planes_dev, (size_t)h_planes * sizeof(tl3d_plane), hipMemcpyDefault));
    return TL3D_OK;
}

}  // namespace tl3d
