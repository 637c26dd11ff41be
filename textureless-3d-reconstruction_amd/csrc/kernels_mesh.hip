// kernels_mesh.hip -- marching cubes over the TSDF channel (tl3d_extract_mesh).
//   t(v) = sum / (w * 32767) in fp64 through tsdf_record (free-space counts included); v is USABLE when w >= mw and |t| < 0.98
//   (the gate of TL3D_EXTRACT_TSDF) and INSIDE when t < 0.
//   vertex: one per voxel edge (v, v + e_axis) whose ends are both usable and differ in inside-ness, owned by v; position and
//       colour are extract_record's TSDF-mode expressions; order: owner record order, then axis x, y, z.
//   cell:  the cube whose lowest corner is v; meshed iff its 8 corners are usable and not all alike (mc_tables.h).
// Three passes over the records in chunks of EXTRACT_CHUNK on the compaction of compact.h (block counts -> single-block scan ->
// in-block wave scan for the write offsets): count (vertices and triangles), write vertices (and each owner's first vertex id into a u32
// scratch indexed like the TSDF pool: slot * 512 + in_brick), write triangles (edge -> owner -> first id + rank of the edge's axis
// among the owner's crossing axes).
#include "compact.h"

#define MC_CONST static __device__ const
#include "mc_tables.h"

namespace tl3d {

struct MeshArgs {
    int mw;                      // max(1, min_weight)
    int nx, ny, nz;
    long long lx, ly;            // keyed extraction: lattice dims along x and y (key = 3 * lattice linear index of the owner + axis)
};

// t of voxel (i, j, k), which must lie in the grid; returns usability
__device__ __forceinline__ bool load_t(const Grid &g, const int2 *__restrict__ tsdf, int mw, int i, int j, int k, double &t) {
    const int2 r = tsdf_record(g, tsdf, vox_index(i, j, k, g.nbx, g.nby));
    t = r.y > 0 ? (double)r.x / ((double)r.y * 32767.0) : 0.0;
    return r.y >= mw && fabs(t) < 0.98;
}

__device__ __forceinline__ int pick3(int a, int b, int c, int s) { return s == 0 ? a : (s == 1 ? b : c); }

// What record idx contributes.  vmask: bit e = the vertex on (v, v + e_e); tn[e] the far end's t when the bit is set.
// cas: the cell's corner case when it is meshed, else 0 (MC_TRI_COUNT[0] = 0).
struct RecInfo {
    int i, j, k;
    double t0;
    double tn[3];
    unsigned vmask;
    unsigned cas;
};

__device__ __forceinline__ void analyse(const Grid &g, const MeshArgs &a, const int2 *__restrict__ tsdf, size_t idx, RecInfo &r) {
    rec_coords(idx, g.nbx, g.nby, r.i, r.j, r.k);
    r.vmask = 0;
    r.cas = 0;
    if (!load_t(g, tsdf, a.mw, r.i, r.j, r.k, r.t0)) return;
    const bool in0 = r.t0 < 0.0;
    const bool hx = r.i + 1 < a.nx, hy = r.j + 1 < a.ny, hz = r.k + 1 < a.nz;
    bool ux = false, uy = false, uz = false;
    if (hx) ux = load_t(g, tsdf, a.mw, r.i + 1, r.j, r.k, r.tn[0]);
    if (hy) uy = load_t(g, tsdf, a.mw, r.i, r.j + 1, r.k, r.tn[1]);
    if (hz) uz = load_t(g, tsdf, a.mw, r.i, r.j, r.k + 1, r.tn[2]);
    const bool ix = ux && r.tn[0] < 0.0, iy = uy && r.tn[1] < 0.0, iz = uz && r.tn[2] < 0.0;
    r.vmask = (ux && ix != in0 ? 1u : 0u) | (uy && iy != in0 ? 2u : 0u) | (uz && iz != in0 ? 4u : 0u);
    if (!(hx && hy && hz && ux && uy && uz)) return;
    double t3, t5, t6, t7;
    if (!load_t(g, tsdf, a.mw, r.i + 1, r.j + 1, r.k, t3)) return;
    if (!load_t(g, tsdf, a.mw, r.i + 1, r.j, r.k + 1, t5)) return;
    if (!load_t(g, tsdf, a.mw, r.i, r.j + 1, r.k + 1, t6)) return;
    if (!load_t(g, tsdf, a.mw, r.i + 1, r.j + 1, r.k + 1, t7)) return;
    if (!in_core(g, r.i, r.j, r.k)) return;                         // a block meshes the cells its core owns (tl3d_set_block_core)
    r.cas = (in0 ? 1u : 0u) | (ix ? 2u : 0u) | (iy ? 4u : 0u) | (t3 < 0.0 ? 8u : 0u) | (iz ? 16u : 0u) | (t5 < 0.0 ? 32u : 0u) |
            (t6 < 0.0 ? 64u : 0u) | (t7 < 0.0 ? 128u : 0u);
}

__device__ __forceinline__ unsigned tri_count(unsigned cas) { return MC_TRI_COUNT[cas]; }

__global__ __launch_bounds__(256) void mesh_count_kernel(Grid g, MeshArgs a, const int2 *__restrict__ tsdf, size_t nvox,
                                                         unsigned *__restrict__ vcounts, unsigned *__restrict__ tcounts) {
    __shared__ unsigned sm[4];
    unsigned nv = 0, nt = 0;
    for_chunk([&](size_t idx) {
        if (idx < nvox) {
            RecInfo r;
            analyse(g, a, tsdf, idx, r);
            nv += (unsigned)__popc(r.vmask);
            nt += tri_count(r.cas);
        }
    });
    nv = block_sum(nv, sm);
    nt = block_sum(nt, sm);
    if (threadIdx.x == 0) {
        vcounts[blockIdx.x] = nv;
        tcounts[blockIdx.x] = nt;
    }
}

__global__ __launch_bounds__(256) void mesh_vert_kernel(Grid g, MeshArgs a, const int2 *__restrict__ tsdf,
                                                        const unsigned long long *__restrict__ cen, size_t nvox,
                                                        const unsigned long long *__restrict__ offsets, unsigned *__restrict__ first_id,
                                                        float *__restrict__ xyz, uint8_t *__restrict__ rgb, unsigned long long cap,
                                                        long long *__restrict__ keys) {
    const double org[3] = {g.oxd, g.oyd, g.ozd};
    const double off[3] = {g.offx, g.offy, g.offz};
    RecInfo r;                                                     // of the element at hand: filled by the count step, read by the emit step
    compact_chunk(
        nvox, offsets,
        [&](size_t idx) {
            analyse(g, a, tsdf, idx, r);
            return (unsigned)__popc(r.vmask);
        },
        [&](size_t idx, unsigned long long o, unsigned) {
            const unsigned slot = brick_slot(g.tsdf_tab, (unsigned)(idx >> 9));
            if (slot < SLOT_FULL) first_id[((size_t)slot << 9) | (idx & 511)] = (unsigned)o;
            const int ijk[3] = {r.i, r.j, r.k};
            int emitted = 0;
#pragma unroll
            for (int e = 0; e < 3; ++e) {
                if (!(r.vmask >> e & 1u)) continue;
                const unsigned long long oo = o + emitted;
                ++emitted;
                if (oo >= cap) continue;
                const double r0 = fabs(r.t0), r1 = fabs(r.tn[e]);
                const double frac = r0 / (r0 + r1);
#pragma unroll
                for (int ax = 0; ax < 3; ++ax) {
                    const double cc = org[ax] + ((off[ax] + (double)ijk[ax]) + 0.5) * g.vsd;     // lattice index: exact in fp64
                    xyz[3 * oo + ax] = (float)(ax == e ? cc + frac * g.vsd : cc);
                }
                if (keys)
                    keys[oo] = 3 * ((((long long)g.voz + r.k) * a.ly + ((long long)g.voy + r.j)) * a.lx + ((long long)g.vox + r.i)) + e;
                uint8_t col[3] = {128, 128, 128};
                if (cen) {
                    const size_t jdx = vox_index(r.i + (e == 0), r.j + (e == 1), r.k + (e == 2), g.nbx, g.nby);
                    const size_t first = (r0 <= r1) ? idx : jdx, second = (r0 <= r1) ? jdx : idx;
                    const unsigned long long *ra = cen_record(g, cen, first);
                    const unsigned long long na = ra ? ra[1] >> 32 : 0ull;
                    if (na > 0) {
                        mean_colour(ra, na, col);
                    } else {
                        const unsigned long long *rb = cen_record(g, cen, second);
                        const unsigned long long nb2 = rb ? rb[1] >> 32 : 0ull;
                        if (nb2 > 0) mean_colour(rb, nb2, col);
                    }
                }
                rgb[3 * oo + 0] = col[0]; rgb[3 * oo + 1] = col[1]; rgb[3 * oo + 2] = col[2];
            }
        });
}

// id of the vertex on edge e (mc_tables.h numbering) of the meshed cell of r: owner corner co, axis ax; the owner's vertices
// are consecutive from its first id in axis order, so the id is first + the number of the owner's crossing axes below ax.
// A crossing of the owner's edge along b < ax is read off the case when that edge belongs to the cell (co's bit b clear),
// else from the voxel beyond it (the owner itself is a usable corner).
__device__ __forceinline__ unsigned edge_vertex(const Grid &g, const MeshArgs &a, const int2 *__restrict__ tsdf,
                                                const unsigned *__restrict__ first_id, const RecInfo &r, unsigned e) {
    const int ax = (int)(e >> 2), q = (int)(e & 3);
    const int o0 = ax == 0 ? 1 : 0, o1 = ax == 2 ? 1 : 2;
    const int co = ((q & 1) << o0) | ((q >> 1) << o1);
    const int oi = r.i + (co & 1), oj = r.j + ((co >> 1) & 1), ok = r.k + ((co >> 2) & 1);
    const bool in_o = (r.cas >> co) & 1u;
    unsigned rank = 0;
#pragma unroll 1
    for (int b = 0; b < ax; ++b) {
        bool cross;
        if (!((co >> b) & 1)) {
            cross = (((r.cas >> (co | (1 << b))) & 1u) != 0) != in_o;
        } else {
            const int ni = oi + (b == 0), nj = oj + (b == 1), nk = ok + (b == 2);
            const int lim = pick3(a.nx, a.ny, a.nz, b), at = pick3(ni, nj, nk, b);
            double tn;
            cross = at < lim && load_t(g, tsdf, a.mw, ni, nj, nk, tn) && ((tn < 0.0) != in_o);
        }
        rank += cross ? 1u : 0u;
    }
    const size_t oidx = vox_index(oi, oj, ok, g.nbx, g.nby);
    const unsigned slot = brick_slot(g.tsdf_tab, (unsigned)(oidx >> 9));
    if (slot >= SLOT_FULL) return 0xffffffffu;                      // (cannot happen: a vertex owner is usable, its brick has records)
    return first_id[((size_t)slot << 9) | (oidx & 511)] + rank;
}

__global__ __launch_bounds__(256) void mesh_tri_kernel(Grid g, MeshArgs a, const int2 *__restrict__ tsdf, size_t nvox,
                                                       const unsigned long long *__restrict__ offsets,
                                                       const unsigned *__restrict__ first_id, unsigned *__restrict__ tris,
                                                       unsigned long long cap) {
    RecInfo r;                                                     // as in mesh_vert_kernel
    compact_chunk(
        nvox, offsets,
        [&](size_t idx) {
            analyse(g, a, tsdf, idx, r);
            return tri_count(r.cas);
        },
        [&](size_t, unsigned long long o, unsigned c) {
#pragma unroll 1
            for (unsigned t = 0; t < c; ++t) {
                if (o + t >= cap) break;
#pragma unroll
                for (int v = 0; v < 3; ++v)
                    tris[3 * (o + t) + v] = edge_vertex(g, a, tsdf, first_id, r, MC_TRI_EDGES[r.cas][3 * t + v]);
            }
        });
}

static MeshArgs mesh_args(const Grid &g, int min_weight, const long long *lat = nullptr) {
    return MeshArgs{min_weight < 1 ? 1 : min_weight, g.nx, g.ny, g.nz, lat ? lat[0] : 0ll, lat ? lat[1] : 0ll};
}

int launch_mesh_count(hipStream_t s, const Grid &g, int min_weight, const int2 *tsdf, unsigned *vcounts, unsigned *tcounts,
                      int nblocks) {
    const size_t nvox = (size_t)g.nx * g.ny * g.nz;
    hipLaunchKernelGGL(mesh_count_kernel, dim3(nblocks), dim3(256), 0, s, g, mesh_args(g, min_weight), tsdf, nvox, vcounts, tcounts);
    TL3D_HIP(hipGetLastError());
    return TL3D_OK;
}

int launch_mesh_write(hipStream_t s, const Grid &g, int min_weight, const int2 *tsdf, const unsigned long long *cen,
                      const unsigned long long *voffsets, const unsigned long long *toffsets, int nblocks, unsigned *first_id,
                      float *xyz, uint8_t *rgb, unsigned long long vcap, unsigned *tris, unsigned long long tcap,
                      long long *keys, const long long *lat) {
    const size_t nvox = (size_t)g.nx * g.ny * g.nz;
    const MeshArgs a = mesh_args(g, min_weight, lat);
    hipLaunchKernelGGL(mesh_vert_kernel, dim3(nblocks), dim3(256), 0, s, g, a, tsdf, cen, nvox, voffsets, first_id, xyz, rgb, vcap, keys);
    TL3D_HIP(hipGetLastError());
    hipLaunchKernelGGL(mesh_tri_kernel, dim3(nblocks), dim3(256), 0, s, g, a, tsdf, nvox, toffsets, first_id, tris, tcap);
    TL3D_HIP(hipGetLastError());
    return TL3D_OK;
}

}  // namespace tl3d
