// kernels_meshweld.hip -- the weld of the keyed meshes of a lattice's blocks (tl3d_mesh_weld_keyed).
// No reference code: the reference has no mesh.  The rules are lattice.weld_meshes' (the host weld is the yardstick, byte for byte):
//   owner voxel of a key: idx = key / 3, x = idx % Lx, y = (idx / Lx) % Ly, z = idx / (Lx Ly)
//   vertex v of part p is KEPT iff its owner voxel lies in the part's core [lo, hi); the output vertices are the kept ones in part
//   order, then vertex order; the output triangles are all triangles in part order, then triangle order, each corner replaced by
//   the output index of the kept vertex that has the corner's key
// The parts are addressed as ONE list of vertices and ONE list of triangles: element g of the list belongs to the part p with
// v0[p] <= g < v0[p + 1] (WeldPart: the part's arrays where the caller or the staging left them, and the sizes of the parts in
// front), found by a binary search over the n_parts descriptors.  No launch is per part.
//
// Passes, each its own launch on the context's stream (kernel boundaries are the ONLY ordering between them):
//   validate      triangle indices >= their part's n_vert and keys outside [0, 3 Lx Ly Lz) are counted; nothing indexed runs
//                 before the host has looked at both counts
//   own count     per chunk of EXTRACT_CHUNK vertices the kept ones -> single-block scan -> the offsets and the number kept
//   own write     compact.h's write pass: a kept vertex goes to its scanned offset o (xyz, rgb, key), vert_map[g] = o, and its
//                 thread inserts the key (keytab.h's kt_claim); the thread whose CAS wins stores o beside the key, a thread that
//                 finds its key there already counts a vertex owned twice; vert_map[g] = NONE for the others
//   resolve       one thread per triangle corner: vert_map of the corner's own vertex, one gather, answers every corner whose
//                 vertex is kept in the same part; only the others (halo corners) look their key up (kt_find), and one that
//                 reaches EMPTY counts an unowned corner; corner e of the one list is written at e
//
// Proof obligations (numbering of DESIGN.md section 4.2.2).  H1, H3 and H5 of the key table are keytab.h's and are kept there: only
// kept vertices insert, `kept` keys at most, into kt_slots(kept) slots.  The lines that are this file's own:
//   H2  the word beside a key is written once, by the   vals[h] is stored only by the thread whose CAS on keys[h] won, and read
//       winner, and read in a later launch.             only by wm_resolve_kernel.
//   H4  results come only from integer add and scans.   the offsets are a scan of integer counts, the two counts atomicAdd.  No
//                                                       float is computed at all: positions and colours are copied.
//   H6  the slot a key lands in may differ from run     nothing written out is a slot number: a corner takes vals[h] of the slot that
//       to run.                                         holds its key, and with no key owned twice that is one value wherever h is
//                                                       (with one owned twice the call fails and its arrays are unspecified).
//   B1  nothing is written beyond an output's end.      o < kept <= vert_cap (the host compares before the write pass, the kernel
//                                                       compares again); corners are written at e < 3 sum n_tri <= 3 tri_cap.
#include "keytab.h"

namespace tl3d {

constexpr unsigned WM_NONE = 0xffffffffu;                // vert_map: not kept; a corner: unowned

// the part that holds vertex g of the one list: the last p with v0[p] <= g (parts without vertices are stepped over)
__device__ __forceinline__ int wm_part_of_vertex(const WeldPart *__restrict__ parts, int n_parts, u64 g) {
    int lo = 0, hi = n_parts;                            // v0[lo] <= g < v0[hi] (v0[n_parts] = the total)
    while (hi - lo > 1) {
        const int m = (lo + hi) >> 1;
        if (parts[m].v0 <= g) lo = m; else hi = m;
    }
    return lo;
}
__device__ __forceinline__ int wm_part_of_triangle(const WeldPart *__restrict__ parts, int n_parts, u64 t) {
    int lo = 0, hi = n_parts;
    while (hi - lo > 1) {
        const int m = (lo + hi) >> 1;
        if (parts[m].t0 <= t) lo = m; else hi = m;
    }
    return lo;
}

// (a validated key: 0 <= key < 3 Lx Ly Lz)
__device__ __forceinline__ bool wm_owned(const WeldPart &p, long long key, u64 lx, u64 ly) {
    const u64 idx = (u64)key / 3;
    const u64 r = idx / lx;
    const long long x = (long long)(idx - r * lx);
    const u64 zz = r / ly;
    const long long y = (long long)(r - zz * ly), z = (long long)zz;
    return x >= p.lo[0] && x < p.hi[0] && y >= p.lo[1] && y < p.hi[1] && z >= p.lo[2] && z < p.hi[2];
}

// info[0] += triangle indices >= their part's n_vert, info[1] += keys outside [0, key_end), info[2] = max over the offending
// indices of (part << 32 | index), for the message
__global__ __launch_bounds__(256) void wm_validate_kernel(const WeldPart *__restrict__ parts, int n_parts, u64 n_vert, u64 n_corners,
                                                          u64 key_end, u64 *__restrict__ info) {
    const u64 g = (u64)blockIdx.x * 256 + threadIdx.x;
    bool bad_key = false, bad_idx = false;
    if (g < n_vert) {
        const WeldPart &p = parts[wm_part_of_vertex(parts, n_parts, g)];
        bad_key = (u64)p.key[g - p.v0] >= key_end;                         // (a negative key is a large unsigned one)
    }
    if (g < n_corners) {
        const int pi = wm_part_of_triangle(parts, n_parts, g / 3);
        const WeldPart &p = parts[pi];
        const unsigned i = p.tri[g - 3 * p.t0];
        bad_idx = (u64)i >= parts[pi + 1].v0 - p.v0;
        if (bad_idx) atomicMax(info + 2, ((u64)pi << 32) | (u64)i);
    }
    wave_count(bad_idx, info);
    wave_count(bad_key, info + 1);
}

__global__ __launch_bounds__(256) void wm_own_count_kernel(const WeldPart *__restrict__ parts, int n_parts, u64 n_vert, u64 lx, u64 ly,
                                                           unsigned *__restrict__ counts) {
    __shared__ unsigned sm[4];
    unsigned c = 0;
    for_chunk([&](u64 g) {
        if (g < n_vert) {
            const WeldPart &p = parts[wm_part_of_vertex(parts, n_parts, g)];
            c += wm_owned(p, p.key[g - p.v0], lx, ly) ? 1u : 0u;
        }
    });
    c = block_sum(c, sm);
    if (threadIdx.x == 0) counts[blockIdx.x] = c;
}

// key -> o into the table; *n_twice += 1 when the key is there already (a validated key is below 3 * 2^61: never KT_EMPTY)
__device__ __forceinline__ void wm_insert(u64 *keys, unsigned *__restrict__ vals, u64 mask, u64 key, unsigned o, u64 *n_twice) {
    bool won;
    const u64 h = kt_claim(keys, mask, key, won);
    if (won) vals[h] = o;                                                   // H2
    else if (h != KT_NONE) atomicAdd(n_twice, 1ull);                        // (KT_NONE: keytab.h H3, never)
}

__global__ __launch_bounds__(256) void wm_own_write_kernel(const WeldPart *__restrict__ parts, int n_parts, u64 n_vert, u64 lx, u64 ly,
                                                           const u64 *__restrict__ offsets, float *__restrict__ out_xyz,
                                                           uint8_t *__restrict__ out_rgb, long long *__restrict__ out_key, u64 vcap,
                                                           unsigned *__restrict__ vert_map, u64 *keys, unsigned *__restrict__ vals, u64 mask,
                                                           u64 *info) {
    const WeldPart *p = nullptr;
    u64 i = 0;
    long long key = 0;
    compact_chunk(
        n_vert, offsets,
        [&](u64 g) -> unsigned {
            p = parts + wm_part_of_vertex(parts, n_parts, g);
            i = g - p->v0;
            key = p->key[i];
            const bool own = wm_owned(*p, key, lx, ly);
            if (!own) vert_map[g] = WM_NONE;
            return own ? 1u : 0u;
        },
        [&](u64 g, u64 o, unsigned) {
            vert_map[g] = (unsigned)o;
            if (o >= vcap) return;                                          // (B1: never)
#pragma unroll
            for (int a = 0; a < 3; ++a) out_xyz[3 * o + a] = p->xyz[3 * i + a];
            if (out_rgb) {
#pragma unroll
                for (int a = 0; a < 3; ++a) out_rgb[3 * o + a] = p->rgb[3 * i + a];
            }
            if (out_key) out_key[o] = key;
            wm_insert(keys, vals, mask, (u64)key, (unsigned)o, info + 3);
        });
}

// (every index is below its part's n_vert: the host has seen info[0])
__global__ __launch_bounds__(256) void wm_resolve_kernel(const WeldPart *__restrict__ parts, int n_parts, u64 n_corners,
                                                         const unsigned *__restrict__ vert_map, const u64 *__restrict__ keys,
                                                         const unsigned *__restrict__ vals, u64 mask, unsigned *__restrict__ out_tri,
                                                         u64 *__restrict__ info) {
    const u64 e = (u64)blockIdx.x * 256 + threadIdx.x;
    bool unowned = false;
    if (e < n_corners) {
        const WeldPart &p = parts[wm_part_of_triangle(parts, n_parts, e / 3)];
        const unsigned i = p.tri[e - 3 * p.t0];
        unsigned o = vert_map[p.v0 + i];
        if (o == WM_NONE) {                                                 // a halo corner: by its key
            const u64 h = kt_find(keys, mask, (u64)p.key[i]);
            unowned = h == KT_NONE;
            if (!unowned) o = vals[h];
        }
        out_tri[e] = o;
    }
    wave_count(unowned, info + 4);
}

// info[0..2] (zeroed by the caller): bad indices, bad keys, the largest offender
int launch_wm_validate(hipStream_t s, const WeldPart *parts, int n_parts, unsigned long long n_vert, unsigned long long n_tri,
                       unsigned long long key_end, unsigned long long *info) {
    const u64 n = n_vert > 3 * n_tri ? n_vert : 3 * n_tri;
    if (n == 0) return TL3D_OK;
    hipLaunchKernelGGL(wm_validate_kernel, dim3(blocks_of(n, 256)), dim3(256), 0, s, parts, n_parts, n_vert, 3 * n_tri, key_end, info);
    TL3D_HIP(hipGetLastError());
    return TL3D_OK;
}

// counts [chunks], offsets [chunks + 1]: offsets[chunks] = the kept vertices
int launch_wm_own_count(hipStream_t s, const WeldPart *parts, int n_parts, unsigned long long n_vert, const long long lat[3], unsigned *counts,
                        unsigned long long *offsets) {
    const int chunks = chunks_of(n_vert);
    hipLaunchKernelGGL(wm_own_count_kernel, dim3(chunks), dim3(256), 0, s, parts, n_parts, n_vert, (u64)lat[0], (u64)lat[1], counts);
    TL3D_HIP(hipGetLastError());
    return launch_scan(s, counts, offsets, chunks, offsets + chunks);
}

// The kept vertices to their offsets and into the table (filled with 0xFF; `slots` = kt_slots(kept)), vert_map [n_vert];
// info[3] (zeroed by the caller) = vertices owned twice
int launch_wm_own_write(hipStream_t s, const WeldPart *parts, int n_parts, unsigned long long n_vert, const long long lat[3],
                        const unsigned long long *offsets, float *out_xyz, uint8_t *out_rgb, long long *out_key, unsigned long long vcap,
                        unsigned *vert_map, unsigned long long *keys, unsigned *vals, unsigned long long slots, unsigned long long *info) {
    hipLaunchKernelGGL(wm_own_write_kernel, dim3(chunks_of(n_vert)), dim3(256), 0, s, parts, n_parts, n_vert, (u64)lat[0], (u64)lat[1], offsets,
                       out_xyz, out_rgb, out_key, vcap, vert_map, keys, vals, slots - 1, info);
    TL3D_HIP(hipGetLastError());
    return TL3D_OK;
}

// out_tri [sum n_tri][3]; info[4] (zeroed by the caller) = unowned corners
int launch_wm_resolve(hipStream_t s, const WeldPart *parts, int n_parts, unsigned long long n_tri, const unsigned *vert_map,
                      const unsigned long long *keys, const unsigned *vals, unsigned long long slots, unsigned *out_tri, unsigned long long *info) {
    if (n_tri == 0) return TL3D_OK;
    hipLaunchKernelGGL(wm_resolve_kernel, dim3(blocks_of(3 * n_tri, 256)), dim3(256), 0, s, parts, n_parts, 3 * n_tri, vert_map, keys, vals,
                       slots - 1, out_tri, info);
    TL3D_HIP(hipGetLastError());
    return TL3D_OK;
}

}  // namespace tl3d
