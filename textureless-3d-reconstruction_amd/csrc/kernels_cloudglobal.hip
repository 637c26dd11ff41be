// kernels_cloudglobal.hip -- the global front end of the cloud registration (the four calls' contracts are in
// tl3d.h): voxel subsampling, FPFH descriptors, nearest-feature correspondences and RANSAC over three-correspondence samples.  No
// reference code: the reference never registers clouds; the definitions are PCL's / Open3D's, with every sequence pinned down so that
// tests/cloud_global_reference.py can restate it.  All arithmetic is fp64 on the f32 inputs converted exactly, one rounding per
// operation (-ffp-contract=off), sums in a stated order; integers wherever a count will do.
//   subsample  sub_claim_kernel: one kt_claim per point (key = the three lattice cells, 21 bits each) and an atomicMin of the point's
//              index on the slot's leader, an array of the call's own beside the table; a point is kept when it IS its slot's
//              leader, and the compaction skeleton (compact.h) lists the kept indices ascending.
//   fpfh       spfh_kernel<KMAX>: thread t serves the point in slot t of the cell order (as normals_kernel: the lanes of a wave are
//              neighbours in space).  The k best (d2, index) pairs in registers by cell_knn_search (cellgrid.h), normals_kernel's search;
//              the list goes to memory as [k][n] by slot (STORED, 4 B x k per point, so that the second pass need not search again:
//              a second pass that searched again took 1.8 x (k <= 32) to 2.1 x (k > 32) the whole call), and a rolled loop over it counts the pair features.  The 33 counters are
//              indexed by a computed bin: they live in LDS as bytes (a count is <= 64), [bin][thread], never in a per-thread array.
//              fpfh_kernel: the same thread order; 33 fp64 sums in registers under static indices over the stored list.
//   match      match_kernel<DMAX>: one thread per row of a, the row in registers as fp64 (static indices), b through LDS in tiles of
//              64 rows which every lane reads at the same address (a broadcast); tiles come in index order and the comparison is
//              strict, so an exact tie keeps the smaller index.
//   ransac     rs_pack_kernel: the correspondences' points as six doubles per pair (and the index check).  rs_draw_kernel: one thread
//              per hypothesis, the draw and the rejections; count[h] = -1 or 0.  The compaction skeleton lists the survivors.
//              rs_score_kernel: one wave per survivor (a fixed grid strides over them), the pose rebuilt by every lane from the three
//              pairs, ballot + popcount over the packed pairs, one 64-bit atomicMax of (count << 32) | (0xFFFFFFFF - h).
//              rs_finish_kernel: one thread rebuilds the winner's pose.  Counts are integers and the winner is a maximum: the same
//              bytes in every run.  No flags, no polls, no waiting on another workgroup anywhere in this file.
// Key table (keytab.h): the subsample inserts at most n distinct keys into kt_slots(n) slots (H3); the keys have bit 63 clear; the
// leader array is this file's own (H2): filled with 0xFF by the host, only ever lowered by atomicMin, read by later launches only.
#include <math.h>

#include "api_host.h"
#include "cellgrid.h"
#include "keytab.h"

namespace tl3d {

// ================================================================================================================= subsample
constexpr long long SUB_CELL_LIMIT = 1ll << 20;        // |cell| must stay below it: 21 bits per axis

__device__ __forceinline__ u64 sub_key(const float *__restrict__ p, double voxel) {
    const long long cx = (long long)floor((double)p[0] / voxel) + SUB_CELL_LIMIT;
    const long long cy = (long long)floor((double)p[1] / voxel) + SUB_CELL_LIMIT;
    const long long cz = (long long)floor((double)p[2] / voxel) + SUB_CELL_LIMIT;
    return (u64)cx | ((u64)cy << 21) | ((u64)cz << 42);                  // the host refused cells outside +-(2^20 - 1): 63 bits
}

__global__ __launch_bounds__(256) void sub_claim_kernel(const float *__restrict__ xyz, long long n, double voxel, u64 *keys, u64 mask,
                                                        unsigned *leader, unsigned *__restrict__ slot_of) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    bool won;
    const u64 h = kt_claim(keys, mask, sub_key(xyz + 3 * i, voxel), won);
    slot_of[i] = (unsigned)h;                                            // KT_NONE (never, H3) becomes a slot nobody leads
    if (h != KT_NONE) atomicMin(leader + h, (unsigned)i);
}

__device__ __forceinline__ unsigned sub_kept(const unsigned *__restrict__ slot_of, const unsigned *__restrict__ leader, u64 mask,
                                             unsigned long long i) {
    const unsigned s = slot_of[i];
    return ((u64)s <= mask && leader[s] == (unsigned)i) ? 1u : 0u;
}

__global__ __launch_bounds__(256) void sub_count_kernel(long long n, const unsigned *__restrict__ slot_of, const unsigned *__restrict__ leader,
                                                        u64 mask, unsigned *__restrict__ counts) {
    __shared__ unsigned sm[4];
    unsigned c = 0;
    for_chunk([&](unsigned long long idx) {
        if (idx < (unsigned long long)n) c += sub_kept(slot_of, leader, mask, idx);
    });
    const unsigned s = block_sum(c, sm);
    if (threadIdx.x == 0) counts[blockIdx.x] = s;
}

__global__ __launch_bounds__(256) void sub_write_kernel(long long n, const unsigned *__restrict__ slot_of, const unsigned *__restrict__ leader,
                                                        u64 mask, const unsigned long long *__restrict__ offsets, int *__restrict__ index_out) {
    compact_chunk((unsigned long long)n, offsets, [&](unsigned long long idx) { return sub_kept(slot_of, leader, mask, idx); },
                  [&](unsigned long long idx, unsigned long long o, unsigned) { index_out[o] = (int)idx; });
}

// device pointers; *kept: the number of indices written (waits for the stream).  slots = kt_slots(n), sized by the caller.
int voxel_subsample_run(tl3d_ctx *ctx, const float *xyz, long long n, double voxel, size_t slots, int *index_out, long long *kept) {
    hipStream_t s = ctx->stream;
    double mn[3], mx[3];
    unsigned long long bad = 0;
    int rc = points_bounds_finite(ctx, xyz, n, mn, mx, &bad);
    if (rc) return rc;
    if (bad) return set_err(TL3D_E_INVALID, "%llu points have a non-finite coordinate", bad);
    for (int a = 0; a < 3; ++a) {                                        // floor(x / voxel) is monotone in x: the box's corners bound every cell
        const double lo = floor(mn[a] / voxel), hi = floor(mx[a] / voxel);
        if (!(lo > -(double)SUB_CELL_LIMIT && hi < (double)SUB_CELL_LIMIT))
            return set_err(TL3D_E_INVALID, "voxel %g: the cloud spans lattice cells %g .. %g on axis %d; |cell| must stay below 2^20", voxel, lo, hi, a);
    }
    const int nch = chunks_of((unsigned long long)n);
    size_t bytes[5] = {slots * sizeof(u64), slots * sizeof(unsigned), (size_t)n * sizeof(unsigned), ((size_t)nch + 1) * sizeof(unsigned),
                       ((size_t)nch + 1) * sizeof(unsigned long long)};
    void *p[5];
    rc = scratch_carve(ctx, 0, bytes, 5, p, "voxel subsample scratch");
    if (rc) return rc;
    u64 *keys = (u64 *)p[0];
    unsigned *leader = (unsigned *)p[1], *slot_of = (unsigned *)p[2], *counts = (unsigned *)p[3];
    unsigned long long *offs = (unsigned long long *)p[4];
    rc = kt_reserve(ctx, keys, slots);                                   // every key EMPTY ...
    if (rc) return rc;
    TL3D_HIP(hipMemsetAsync(leader, 0xFF, bytes[1], s));                 // ... and every leader above every index
    const u64 mask = (u64)slots - 1;
    hipLaunchKernelGGL(sub_claim_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, xyz, n, voxel, keys, mask, leader, slot_of);
    hipLaunchKernelGGL(sub_count_kernel, dim3(nch), dim3(256), 0, s, n, slot_of, leader, mask, counts);
    TL3D_HIP(hipGetLastError());
    rc = launch_scan(s, counts, offs, nch, offs + nch);
    if (rc) return rc;
    hipLaunchKernelGGL(sub_write_kernel, dim3(nch), dim3(256), 0, s, n, slot_of, leader, mask, offs, index_out);
    TL3D_HIP(hipGetLastError());
    unsigned long long total = 0;
    TL3D_HIP(hipMemcpyAsync(&total, offs + nch, sizeof(total), hipMemcpyDeviceToHost, s));
    TL3D_HIP(hipStreamSynchronize(s));
    *kept = (long long)total;
    return TL3D_OK;
}

// ====================================================================================================================== fpfh
constexpr int FPFH_BINS = 33, FPFH_ROW = 34;           // the SPFH row: 33 counts and the number of counted pairs
constexpr double FPFH_PI = 3.14159265358979323846, FPFH_2PI = 6.28318530717958647692;

// bin of a feature whose scaled value is u = 11 (f - lo) / span
__device__ __forceinline__ int fp_bin(double u) { return (int)fmin(fmax(floor(u), 0.0), 10.0); }

// Pass one.  nbr [k][n] by slot: the members of the point's neighbourhood in list order, -1 where the list has no member (or the
// member was removed: d2 == 0, a zero normal).  spfh [n][34] by point index.
template <int KMAX>
__global__ __launch_bounds__(256) void spfh_kernel(CellGrid g, const float *__restrict__ xyz, const float *__restrict__ nrm, long long n, int k,
                                                   double md2, const unsigned *__restrict__ start, const float4 *__restrict__ sorted,
                                                   int *nbr, int *__restrict__ spfh) {
    __shared__ unsigned char sm_cnt[FPFH_BINS * 256];
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= n) return;                                                   // no barrier in this kernel: a thread's counters are its own
    const float4 me = sorted[t];
    const int qi = __float_as_int(me.w);
    const double px = (double)me.x, py = (double)me.y, pz = (double)me.z;

    double bd[KMAX];
    int bi[KMAX];
#pragma unroll
    for (int j = 0; j < KMAX; ++j) { bd[j] = INFINITY; bi[j] = 0x7fffffff; }
    cell_knn_search<KMAX>(g, start, sorted, px, py, pz, k, md2, bd, bi);
    // the list leaves the registers: the first k entries that exist and lie within the radius, less the point itself and its duplicates
#pragma unroll
    for (int j = 0; j < KMAX; ++j)
        if (j < k) nbr[(size_t)j * n + t] = (bi[j] != 0x7fffffff && bd[j] <= md2 && bd[j] > 0.0) ? bi[j] : -1;

    unsigned char *cnt = sm_cnt + threadIdx.x;                            // counter b of this thread: cnt[b * 256]
    for (int b = 0; b < FPFH_BINS; ++b) cnt[b * 256] = 0;
    const double nix = (double)nrm[3 * (size_t)qi], niy = (double)nrm[3 * (size_t)qi + 1], niz = (double)nrm[3 * (size_t)qi + 2];
    const bool have_normal = !(nix == 0.0 && niy == 0.0 && niz == 0.0);
    int m = 0;
    for (int j = 0; j < k; ++j) {
        const int jj = nbr[(size_t)j * n + t];                            // this thread's own store, read back in program order
        if (jj < 0) continue;
        const double njx = (double)nrm[3 * (size_t)jj], njy = (double)nrm[3 * (size_t)jj + 1], njz = (double)nrm[3 * (size_t)jj + 2];
        if (njx == 0.0 && njy == 0.0 && njz == 0.0) {                      // a member without a normal leaves the neighbourhood
            nbr[(size_t)j * n + t] = -1;
            continue;
        }
        if (!have_normal) continue;
        double dx = (double)xyz[3 * (size_t)jj] - px, dy = (double)xyz[3 * (size_t)jj + 1] - py, dz = (double)xyz[3 * (size_t)jj + 2] - pz;
        const double L = sqrt(dx * dx + dy * dy + dz * dz);
        const double a1 = (nix * dx + niy * dy + niz * dz) / L, a2 = (njx * dx + njy * dy + njz * dz) / L;
        const bool sw = fabs(a1) < fabs(a2);
        const double sx = sw ? njx : nix, sy = sw ? njy : niy, sz = sw ? njz : niz;        // ns
        const double tx = sw ? nix : njx, ty = sw ? niy : njy, tz = sw ? niz : njz;        // nt
        const double f3 = sw ? -a2 : a1;
        if (sw) { dx = -dx; dy = -dy; dz = -dz; }
        double vx = dy * sz - dz * sy, vy = dz * sx - dx * sz, vz = dx * sy - dy * sx;     // v = d x ns
        const double vl = sqrt(vx * vx + vy * vy + vz * vz);
        if (vl == 0.0) continue;
        vx /= vl; vy /= vl; vz /= vl;
        const double wx = sy * vz - sz * vy, wy = sz * vx - sx * vz, wz = sx * vy - sy * vx;   // w = ns x v
        const double f2 = vx * tx + vy * ty + vz * tz;
        const double f1 = atan2(wx * tx + wy * ty + wz * tz, sx * tx + sy * ty + sz * tz);
        const int b1 = fp_bin(11.0 * (f1 + FPFH_PI) / FPFH_2PI), b2 = fp_bin(11.0 * (f2 + 1.0) / 2.0), b3 = fp_bin(11.0 * (f3 + 1.0) / 2.0);
        cnt[b1 * 256] += 1;
        cnt[(11 + b2) * 256] += 1;
        cnt[(22 + b3) * 256] += 1;
        ++m;
    }
    int *row = spfh + (size_t)qi * FPFH_ROW;
    for (int b = 0; b < FPFH_BINS; ++b) row[b] = (int)cnt[b * 256];
    row[FPFH_BINS] = m;
}

// Pass two, the same thread order: S[b] over the stored list, each group of 11 scaled to 100, the point's own SPFH added.
__global__ __launch_bounds__(256) void fpfh_kernel(const float *__restrict__ xyz, long long n, int k, const float4 *__restrict__ sorted,
                                                   const int *__restrict__ nbr, const int *__restrict__ spfh, float *__restrict__ out) {
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= n) return;
    const float4 me = sorted[t];
    const int qi = __float_as_int(me.w);
    const double px = (double)me.x, py = (double)me.y, pz = (double)me.z;
    const int *own = spfh + (size_t)qi * FPFH_ROW;
    const int mi = own[FPFH_BINS];
    float *o = out + (size_t)qi * FPFH_BINS;
    if (mi == 0) {                                                        // (a point without a normal counted nothing)
#pragma unroll
        for (int b = 0; b < FPFH_BINS; ++b) o[b] = 0.0f;
        return;
    }
    double S[FPFH_BINS];
#pragma unroll
    for (int b = 0; b < FPFH_BINS; ++b) S[b] = 0.0;
    for (int j = 0; j < k; ++j) {
        const int jj = nbr[(size_t)j * n + t];
        if (jj < 0) continue;
        const int *row = spfh + (size_t)jj * FPFH_ROW;
        const int mj = row[FPFH_BINS];
        if (mj == 0) continue;
        const double dx = (double)xyz[3 * (size_t)jj] - px, dy = (double)xyz[3 * (size_t)jj + 1] - py, dz = (double)xyz[3 * (size_t)jj + 2] - pz;
        const double d2 = dx * dx + dy * dy + dz * dz, dm = (double)mj;
#pragma unroll
        for (int b = 0; b < FPFH_BINS; ++b) S[b] += (100.0 * (double)row[b] / dm) / d2;
    }
    const double dmi = (double)mi;
#pragma unroll
    for (int grp = 0; grp < 3; ++grp) {
        double sum = 0.0;
#pragma unroll
        for (int b = 0; b < 11; ++b) sum += S[11 * grp + b];
        const double f = sum > 0.0 ? 100.0 / sum : 1.0;
#pragma unroll
        for (int b = 0; b < 11; ++b) {
            const double v = sum > 0.0 ? S[11 * grp + b] * f : S[11 * grp + b];
            o[11 * grp + b] = (float)(v + 100.0 * (double)own[11 * grp + b] / dmi);
        }
    }
}

// device pointers; spfh_out may be null (the call's scratch holds the rows then)
int fpfh_run(tl3d_ctx *ctx, const float *xyz, const float *nrm, long long n, int k, double max_radius, double cell, float *fpfh_out, int *spfh_out) {
    hipStream_t s = ctx->stream;
    if (k > n) k = (int)n;
    double mn[3], mx[3];
    unsigned long long bad = 0;
    int rc = points_bounds_finite(ctx, xyz, n, mn, mx, &bad);
    if (rc) return rc;
    if (bad) return set_err(TL3D_E_INVALID, "%llu points have a non-finite coordinate", bad);
    CellGrid g;
    cell_grid_fit(mn, mx, cell, &g);
    size_t bytes[7];
    cell_table_bytes(cell_grid_cells(g), bytes);
    bytes[4] = (size_t)n * sizeof(float4);
    bytes[5] = (size_t)n * (size_t)k * sizeof(int);
    bytes[6] = spfh_out ? 0 : (size_t)n * FPFH_ROW * sizeof(int);
    void *p[7];
    rc = scratch_carve(ctx, 0, bytes, 7, p, "FPFH scratch");
    if (rc) return rc;
    const CellTables t = CellTables::at(p);
    float4 *sorted = (float4 *)p[4];
    int *nbr = (int *)p[5];
    int *spfh = spfh_out ? spfh_out : (int *)p[6];
    rc = cell_index_build(s, g, xyz, n, t, true, EmitPointIndex{sorted});
    if (rc) return rc;
    const unsigned nb = (unsigned)((n + 255) / 256);
    const double md2 = max_radius > 0.0 ? max_radius * max_radius : INFINITY;
    if (k <= 32)
        hipLaunchKernelGGL(spfh_kernel<32>, dim3(nb), dim3(256), 0, s, g, xyz, nrm, n, k, md2, t.start, sorted, nbr, spfh);
    else
        hipLaunchKernelGGL(spfh_kernel<64>, dim3(nb), dim3(256), 0, s, g, xyz, nrm, n, k, md2, t.start, sorted, nbr, spfh);
    TL3D_HIP(hipGetLastError());
    hipLaunchKernelGGL(fpfh_kernel, dim3(nb), dim3(256), 0, s, xyz, n, k, sorted, nbr, spfh, fpfh_out);
    TL3D_HIP(hipGetLastError());
    return TL3D_OK;
}

// ===================================================================================================================== match
constexpr int MATCH_TILE = 64;                         // rows of b per LDS tile: 64 x 64 x 4 B = 16 KB at the largest dim

template <int DMAX>
__global__ __launch_bounds__(256) void match_kernel(const float *__restrict__ fa, long long na, const float *__restrict__ fb, long long nb, int dim,
                                                    int *__restrict__ index_out, double *__restrict__ dist2_out) {
    __shared__ float sm_b[MATCH_TILE * DMAX];
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    const bool live = i < na;                              // every thread stays for the barriers
    double a[DMAX];
#pragma unroll
    for (int c = 0; c < DMAX; ++c) a[c] = (live && c < dim) ? (double)fa[(size_t)i * dim + c] : 0.0;
    double best = INFINITY;
    int best_i = nb > 0 ? 0 : -1;                          // row 0 until a row is STRICTLY nearer: all-inf or NaN distances keep it
    for (long long base = 0; base < nb; base += MATCH_TILE) {
        const int rows = (int)min((long long)MATCH_TILE, nb - base);
        __syncthreads();
        for (int e = threadIdx.x; e < rows * dim; e += 256) sm_b[e] = fb[(size_t)base * dim + e];     // the tile's rows are contiguous
        __syncthreads();
        for (int r = 0; r < rows; ++r) {
            const float *b = sm_b + r * dim;
            double d2 = 0.0;
#pragma unroll
            for (int c = 0; c < DMAX; ++c)
                if (c < dim) {
                    const double d = a[c] - (double)b[c];
                    d2 += d * d;
                }
            if (d2 < best) { best = d2; best_i = (int)(base + r); }
        }
    }
    if (live) {
        if (index_out) index_out[i] = best_i;
        if (dist2_out) dist2_out[i] = best;
    }
}

int feature_match_run(tl3d_ctx *ctx, const float *fa, long long na, const float *fb, long long nb, int dim, int *index_out, double *dist2_out) {
    const unsigned blocks = (unsigned)((na + 255) / 256);
    if (dim <= 33)
        hipLaunchKernelGGL(match_kernel<33>, dim3(blocks), dim3(256), 0, ctx->stream, fa, na, fb, nb, dim, index_out, dist2_out);
    else
        hipLaunchKernelGGL(match_kernel<64>, dim3(blocks), dim3(256), 0, ctx->stream, fa, na, fb, nb, dim, index_out, dist2_out);
    TL3D_HIP(hipGetLastError());
    return TL3D_OK;
}

// ==================================================================================================================== ransac
constexpr u64 RS_GOLDEN = 0x9E3779B97F4A7C15ull;
constexpr int RS_SCORE_BLOCKS = 8192;                  // the score kernel's grid at most: 4 waves each stride over the survivors

struct RsPose { double R[9], t[3]; };

// pairs: six doubles per correspondence (the source point, then the target point); *bad counts pairs with an index out of range,
// which get zeros
__global__ __launch_bounds__(256) void rs_pack_kernel(const float *__restrict__ src, long long n_src, const float *__restrict__ tgt, long long n_tgt,
                                                      const int *__restrict__ corr, long long m, double *__restrict__ pairs, u64 *bad) {
    const long long k = (long long)blockIdx.x * 256 + threadIdx.x;
    bool is_bad = false;
    if (k < m) {
        const long long a = corr[2 * k], b = corr[2 * k + 1];
        is_bad = a < 0 || a >= n_src || b < 0 || b >= n_tgt;
        double *o = pairs + 6 * (size_t)k;
        for (int c = 0; c < 3; ++c) {
            o[c] = is_bad ? 0.0 : (double)src[3 * (size_t)a + c];
            o[3 + c] = is_bad ? 0.0 : (double)tgt[3 * (size_t)b + c];
        }
    }
    wave_count(is_bad, bad);
}

__device__ __forceinline__ double rs_dot(const double a[3], const double b[3]) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }
__device__ __forceinline__ void rs_cross(const double a[3], const double b[3], double o[3]) {
    o[0] = a[1] * b[2] - a[2] * b[1];
    o[1] = a[2] * b[0] - a[0] * b[2];
    o[2] = a[0] * b[1] - a[1] * b[0];
}
// the frame [x y z] of three points as columns F[c][axis]; false: degenerate
__device__ __forceinline__ bool rs_triad(const double *p0, const double *p1, const double *p2, double x[3], double y[3], double z[3]) {
    double e1[3], e2[3];
    for (int c = 0; c < 3; ++c) { e1[c] = p1[c] - p0[c]; e2[c] = p2[c] - p0[c]; }
    const double l1 = sqrt(rs_dot(e1, e1));
    for (int c = 0; c < 3; ++c) x[c] = e1[c] / l1;
    rs_cross(x, e2, z);
    const double lz = sqrt(rs_dot(z, z));
    if (!(lz > 0.0)) return false;                                        // (also a NaN from l1 == 0, which the edge test excludes anyway)
    for (int c = 0; c < 3; ++c) z[c] /= lz;
    rs_cross(z, x, y);
    return true;
}
// Hypothesis h: the draw, the rejections and, when it passes, the pose.  The same sequence for the draw kernel, every lane of a scoring
// wave and the finish: all of them get the same bits.
__device__ __forceinline__ bool rs_hypothesis(u64 h, u64 seed, u64 m, double edge_ratio, const double *__restrict__ pairs, RsPose &P) {
    u64 id[3];
    for (int j = 0; j < 3; ++j) id[j] = kt_mix(seed + RS_GOLDEN * (3ull * h + (u64)j + 1ull)) % m;
    if (id[0] == id[1] || id[0] == id[2] || id[1] == id[2]) return false;
    const double *q0 = pairs + 6 * id[0], *q1 = pairs + 6 * id[1], *q2 = pairs + 6 * id[2];
    const double *qa[3] = {q0, q1, q2}, *qb[3] = {q1, q2, q0};
    for (int e = 0; e < 3; ++e) {
        double ds[3], dt[3];
        for (int c = 0; c < 3; ++c) { ds[c] = qb[e][c] - qa[e][c]; dt[c] = qb[e][3 + c] - qa[e][3 + c]; }
        const double ls = sqrt(rs_dot(ds, ds)), lt = sqrt(rs_dot(dt, dt));
        const double hi = fmax(ls, lt), lo = fmin(ls, lt);
        if (hi == 0.0 || lo < edge_ratio * hi) return false;
    }
    double xs[3], ys[3], zs[3], xt[3], yt[3], zt[3];
    if (!rs_triad(q0, q1, q2, xs, ys, zs) || !rs_triad(q0 + 3, q1 + 3, q2 + 3, xt, yt, zt)) return false;
    double ms[3], mt[3];
    for (int c = 0; c < 3; ++c) {
        ms[c] = ((q0[c] + q1[c]) + q2[c]) / 3.0;
        mt[c] = ((q0[3 + c] + q1[3 + c]) + q2[3 + c]) / 3.0;
    }
    for (int i = 0; i < 3; ++i) {
        for (int j = 0; j < 3; ++j) P.R[3 * i + j] = xt[i] * xs[j] + yt[i] * ys[j] + zt[i] * zs[j];      // R = F_t F_s^T
        P.t[i] = mt[i] - (P.R[3 * i] * ms[0] + P.R[3 * i + 1] * ms[1] + P.R[3 * i + 2] * ms[2]);
    }
    return true;
}

__global__ __launch_bounds__(256) void rs_draw_kernel(long long H, u64 seed, u64 m, double edge_ratio, const double *__restrict__ pairs,
                                                      int *__restrict__ count) {
    const long long h = (long long)blockIdx.x * 256 + threadIdx.x;
    if (h >= H) return;
    RsPose P;
    count[h] = rs_hypothesis((u64)h, seed, m, edge_ratio, pairs, P) ? 0 : -1;
}

__global__ __launch_bounds__(256) void rs_count_kernel(long long H, const int *__restrict__ count, unsigned *__restrict__ counts) {
    __shared__ unsigned sm[4];
    unsigned c = 0;
    for_chunk([&](unsigned long long idx) {
        if (idx < (unsigned long long)H && count[idx] == 0) ++c;
    });
    const unsigned s = block_sum(c, sm);
    if (threadIdx.x == 0) counts[blockIdx.x] = s;
}

__global__ __launch_bounds__(256) void rs_list_kernel(long long H, const int *__restrict__ count, const unsigned long long *__restrict__ offsets,
                                                      unsigned *__restrict__ passed) {
    compact_chunk((unsigned long long)H, offsets, [&](unsigned long long idx) { return count[idx] == 0 ? 1u : 0u; },
                  [&](unsigned long long idx, unsigned long long o, unsigned) { passed[o] = (unsigned)idx; });
}

// passed[*n_passed]: the survivors in ascending h (the list kernel has finished: a launch boundary lies between)
__global__ __launch_bounds__(256) void rs_score_kernel(const unsigned *__restrict__ passed, const unsigned long long *__restrict__ n_passed, u64 seed,
                                                       u64 m, double edge_ratio, double md2, const double *__restrict__ pairs, int *__restrict__ count,
                                                       u64 *best) {
    const unsigned long long np = *n_passed, waves = (unsigned long long)gridDim.x * 4;
    const int lane = threadIdx.x & 63;
    for (unsigned long long w = (unsigned long long)blockIdx.x * 4 + (threadIdx.x >> 6); w < np; w += waves) {
        const unsigned h = passed[w];
        RsPose P;
        rs_hypothesis((u64)h, seed, m, edge_ratio, pairs, P);               // it passed once: it passes again, the same bits
        unsigned c = 0;
        for (u64 base = 0; base < m; base += 64) {
            const u64 k = base + lane;
            bool in = false;
            if (k < m) {
                const double *q = pairs + 6 * k;
                const double ex = ((P.R[0] * q[0] + P.R[1] * q[1] + P.R[2] * q[2]) + P.t[0]) - q[3];
                const double ey = ((P.R[3] * q[0] + P.R[4] * q[1] + P.R[5] * q[2]) + P.t[1]) - q[4];
                const double ez = ((P.R[6] * q[0] + P.R[7] * q[1] + P.R[8] * q[2]) + P.t[2]) - q[5];
                in = ex * ex + ey * ey + ez * ez <= md2;
            }
            c += (unsigned)__popcll(__ballot(in));
        }
        if (lane == 0) {
            count[h] = (int)c;
            atomicMax(best, ((u64)c << 32) | (u64)(0xFFFFFFFFu - h));
        }
    }
}

// result: 16 doubles, T row-major (the identity when nothing passed)
__global__ void rs_finish_kernel(const u64 *__restrict__ best, const unsigned long long *__restrict__ n_passed, u64 seed, u64 m, double edge_ratio,
                                 const double *__restrict__ pairs, double *__restrict__ T) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    RsPose P;
    for (int i = 0; i < 9; ++i) P.R[i] = (i % 4 == 0) ? 1.0 : 0.0;
    P.t[0] = P.t[1] = P.t[2] = 0.0;
    if (*n_passed) rs_hypothesis((u64)(0xFFFFFFFFu - (unsigned)(*best & 0xFFFFFFFFull)), seed, m, edge_ratio, pairs, P);
    for (int i = 0; i < 3; ++i) {
        for (int j = 0; j < 3; ++j) T[4 * i + j] = P.R[3 * i + j];
        T[4 * i + 3] = P.t[i];
    }
    T[12] = T[13] = T[14] = 0.0;
    T[15] = 1.0;
}

// device pointers but out (host); count_out may be null.  m >= 1.
int ransac_run(tl3d_ctx *ctx, const float *src, long long n_src, const float *tgt, long long n_tgt, const int *corr, long long m,
               const tl3d_ransac_params &prm, tl3d_ransac_result *out, int *count_out) {
    hipStream_t s = ctx->stream;
    for (int side = 0; side < 2; ++side) {
        double mn[3], mx[3];
        unsigned long long bad = 0;
        const int rc = points_bounds_finite(ctx, side ? tgt : src, side ? n_tgt : n_src, mn, mx, &bad);
        if (rc) return rc;
        if (bad) return set_err(TL3D_E_INVALID, "%llu %s points have a non-finite coordinate", bad, side ? "target" : "source");
    }
    const long long H = prm.n_hypotheses;
    const int nch = chunks_of((unsigned long long)H);
    size_t bytes[6] = {(size_t)m * 6 * sizeof(double), count_out ? 0 : (size_t)H * sizeof(int), (size_t)H * sizeof(unsigned),
                       ((size_t)nch + 1) * sizeof(unsigned), ((size_t)nch + 1) * sizeof(unsigned long long), 18 * sizeof(double)};
    void *p[6];
    int rc = scratch_carve(ctx, 0, bytes, 6, p, "RANSAC scratch");
    if (rc) return rc;
    double *pairs = (double *)p[0];
    int *count = count_out ? count_out : (int *)p[1];
    unsigned *passed = (unsigned *)p[2], *counts = (unsigned *)p[3];
    unsigned long long *offs = (unsigned long long *)p[4];
    u64 *words = (u64 *)p[5];                                             // [0] bad pairs, [1] the winner's word, [2..17] T
    TL3D_HIP(hipMemsetAsync(words, 0, 2 * sizeof(u64), s));
    hipLaunchKernelGGL(rs_pack_kernel, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, s, src, n_src, tgt, n_tgt, corr, m, pairs, words);
    TL3D_HIP(hipGetLastError());
    u64 bad = 0;
    TL3D_HIP(hipMemcpyAsync(&bad, words, sizeof(bad), hipMemcpyDeviceToHost, s));
    TL3D_HIP(hipStreamSynchronize(s));
    if (bad) return set_err(TL3D_E_INVALID, "%llu correspondences name a point outside their cloud", bad);
    const double md2 = prm.max_dist * prm.max_dist;
    hipLaunchKernelGGL(rs_draw_kernel, dim3((unsigned)((H + 255) / 256)), dim3(256), 0, s, H, (u64)prm.seed, (u64)m, prm.edge_ratio, pairs, count);
    hipLaunchKernelGGL(rs_count_kernel, dim3(nch), dim3(256), 0, s, H, count, counts);
    TL3D_HIP(hipGetLastError());
    rc = launch_scan(s, counts, offs, nch, offs + nch);
    if (rc) return rc;
    hipLaunchKernelGGL(rs_list_kernel, dim3(nch), dim3(256), 0, s, H, count, offs, passed);
    const unsigned blocks = (unsigned)min((long long)RS_SCORE_BLOCKS, (H + 3) / 4);
    hipLaunchKernelGGL(rs_score_kernel, dim3(blocks), dim3(256), 0, s, passed, offs + nch, (u64)prm.seed, (u64)m, prm.edge_ratio, md2, pairs, count,
                       words + 1);
    hipLaunchKernelGGL(rs_finish_kernel, dim3(1), dim3(64), 0, s, words + 1, offs + nch, (u64)prm.seed, (u64)m, prm.edge_ratio, pairs,
                       (double *)(words + 2));
    TL3D_HIP(hipGetLastError());
    u64 h_words[17];
    unsigned long long n_passed = 0;
    TL3D_HIP(hipMemcpyAsync(h_words, words + 1, sizeof(h_words), hipMemcpyDeviceToHost, s));
    TL3D_HIP(hipMemcpyAsync(&n_passed, offs + nch, sizeof(n_passed), hipMemcpyDeviceToHost, s));
    TL3D_HIP(hipStreamSynchronize(s));
    memcpy(out->T, h_words + 1, 16 * sizeof(double));
    out->n_passed = (int64_t)n_passed;
    out->m = m;
    out->best_h = n_passed ? (int64_t)(0xFFFFFFFFu - (unsigned)(h_words[0] & 0xFFFFFFFFull)) : -1;
    out->inliers = n_passed ? (int64_t)(h_words[0] >> 32) : 0;
    out->status = n_passed ? 1 : 2;
    out->reserved = 0;
    return TL3D_OK;
}

}  // namespace tl3d
