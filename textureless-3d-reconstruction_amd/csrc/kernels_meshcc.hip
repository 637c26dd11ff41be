// kernels_meshcc.hip -- connected components of an indexed triangle list and the filter built on them (tl3d_mesh_components,
// tl3d_mesh_filter_components).  No reference code: the reference has no mesh.  The rules are ours:
//   two vertices are connected when one triangle names both (shared VERTICES, not shared edges); a component is a connected set of
//   vertices; label[v] = the smallest vertex index of v's component; a vertex no triangle names is a component of its own with
//   0 triangles; a triangle belongs to the component of its vertices; (a, a, b) counts as a triangle and connects a and b.
// Everything below is a function of the input alone: integer atomics (min / CAS towards the smaller root, add, max) commute, and
// the compaction writes at scanned offsets, so every run gives the same bytes.
//
// Passes, each its own launch on the context's stream (kernel boundaries are the ONLY ordering between them):
//   validate  max of all indices (nothing indexed runs before the host has compared it with n_vert)
//   init      parent[v] = v, tri_count[v] = 0
//   hook      one thread per triangle: unite(a, b), unite(b, c)
//   flatten   parent[v] = find(v): from here on parent IS the label array
//   count     tri_count[label] += 1, aggregated per wave
//   roots     number of components, largest component as one 64-bit max of (count << 32 | ~label): ties go to the smaller label
//   compact   kept vertices / triangles per chunk -> single-block scan -> order-preserving writes (compact.h)
//
// The union-find (cc_find / cc_unite) and the proof obligations I1-I6 that hook and flatten keep are in unionfind.h.
#include "compact.h"
#include "unionfind.h"

namespace tl3d {

__global__ __launch_bounds__(256) void cc_validate_kernel(const unsigned *__restrict__ idx, unsigned long long n,
                                                          unsigned *__restrict__ max_out) {
    unsigned m = 0;
    for (unsigned long long i = (unsigned long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (unsigned long long)gridDim.x * 256) m = max(m, idx[i]);
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) m = max(m, (unsigned)__shfl_down(m, d));
    if ((threadIdx.x & 63) == 0 && m) atomicMax(max_out, m);
}

__global__ __launch_bounds__(256) void cc_init_kernel(unsigned *__restrict__ parent, unsigned *__restrict__ count, unsigned n) {
    const unsigned v = blockIdx.x * 256u + threadIdx.x;
    if (v < n) {
        parent[v] = v;
        count[v] = 0u;
    }
}

__global__ __launch_bounds__(256) void cc_hook_kernel(const unsigned *__restrict__ tri, unsigned long long n_tri, unsigned *parent) {
    const unsigned long long t = (unsigned long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= n_tri) return;
    const unsigned a = tri[3 * t], b = tri[3 * t + 1], c = tri[3 * t + 2];
    if (a != b) cc_unite(parent, a, b);
    if (b != c) cc_unite(parent, b, c);
}

__global__ __launch_bounds__(256) void cc_flatten_kernel(unsigned *parent, unsigned n) {
    const unsigned v = blockIdx.x * 256u + threadIdx.x;
    if (v >= n) return;
    const unsigned r = cc_find(parent, v);
    if (r < v) atomicMin(parent + v, r);
}

// one add per distinct label of a wave: triangles come in record order, so a wave mostly holds one or two labels
__global__ __launch_bounds__(256) void cc_count_kernel(const unsigned *__restrict__ tri, unsigned long long n_tri,
                                                       const unsigned *__restrict__ label, unsigned *__restrict__ count) {
    const unsigned long long t = (unsigned long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= n_tri) return;
    const unsigned l = label[tri[3 * t]];
    const int lane = threadIdx.x & 63;
    bool todo = true;
    while (todo) {
        const unsigned first = (unsigned)__builtin_amdgcn_readfirstlane((int)l);
        const unsigned long long same = __ballot(l == first);          // among the lanes still in the loop
        if (l == first) {
            if (lane == __ffsll((long long)same) - 1) atomicAdd(count + first, (unsigned)__popcll(same));
            todo = false;
        }
    }
}

// info[1] += roots, info[2] = max over roots of (count << 32 | 0xFFFFFFFF - label)
__global__ __launch_bounds__(256) void cc_roots_kernel(const unsigned *__restrict__ label, const unsigned *__restrict__ count, unsigned n,
                                                       unsigned long long *__restrict__ info) {
    const unsigned v = blockIdx.x * 256u + threadIdx.x;
    const bool root = v < n && label[v] == v;
    unsigned long long key = root ? ((unsigned long long)count[v] << 32) | (unsigned long long)(0xFFFFFFFFu - v) : 0ull;
    unsigned c = root ? 1u : 0u;
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
        const unsigned long long ok = __shfl_down(key, d);
        key = ok > key ? ok : key;
        c += __shfl_down(c, d);
    }
    if ((threadIdx.x & 63) == 0 && c) {
        atomicAdd(info + 1, (unsigned long long)c);
        atomicMax(info + 2, key);
    }
}

struct CcKeep {
    long long min_tri;           // <= 0: every component
    int largest;                 // only the largest component (info[2], cc_roots_kernel), and only if it has a triangle
    const unsigned long long *info;
};

__device__ __forceinline__ bool cc_kept(const CcKeep &k, unsigned l, unsigned cnt) {
    if (k.min_tri > 0 && (long long)cnt < k.min_tri) return false;
    return !k.largest || (cnt > 0 && l == 0xFFFFFFFFu - (unsigned)k.info[2]);
}

// kept vertices per chunk, the caller's keep mask, and info[3] += kept components
__global__ __launch_bounds__(256) void cc_vert_count_kernel(CcKeep k, const unsigned *__restrict__ label, const unsigned *__restrict__ count,
                                                            unsigned n, unsigned *__restrict__ chunk_counts, uint8_t *__restrict__ keep_out,
                                                            unsigned long long *__restrict__ info) {
    __shared__ unsigned sm[4];
    unsigned nv = 0, nc = 0;
    for_chunk([&](unsigned long long v) {
        if (v < n) {
            const unsigned l = label[v];
            const bool keep = cc_kept(k, l, count[l]);
            nv += keep ? 1u : 0u;
            nc += keep && l == (unsigned)v ? 1u : 0u;
            if (keep_out) keep_out[v] = keep ? 1 : 0;
        }
    });
    nv = block_sum(nv, sm);
    nc = block_sum(nc, sm);
    if (threadIdx.x == 0) {
        chunk_counts[blockIdx.x] = nv;
        if (nc) atomicAdd(info + 3, (unsigned long long)nc);
    }
}

__global__ __launch_bounds__(256) void cc_tri_count_kernel(CcKeep k, const unsigned *__restrict__ tri, unsigned long long n_tri,
                                                           const unsigned *__restrict__ label, const unsigned *__restrict__ count,
                                                           unsigned *__restrict__ chunk_counts) {
    __shared__ unsigned sm[4];
    unsigned nt = 0;
    for_chunk([&](unsigned long long t) {
        if (t < n_tri) {
            const unsigned l = label[tri[3 * t]];
            nt += cc_kept(k, l, count[l]) ? 1u : 0u;
        }
    });
    nt = block_sum(nt, sm);
    if (threadIdx.x == 0) chunk_counts[blockIdx.x] = nt;
}

// kept vertices in order to [offset of the chunk + rank]; remap[v] = the new index of a kept vertex
__global__ __launch_bounds__(256) void cc_vert_write_kernel(CcKeep k, const unsigned *__restrict__ label, const unsigned *__restrict__ count,
                                                            unsigned n, const unsigned long long *__restrict__ offsets,
                                                            const float *__restrict__ xyz, const uint8_t *__restrict__ rgb,
                                                            float *__restrict__ out_xyz, uint8_t *__restrict__ out_rgb, unsigned long long cap,
                                                            unsigned *__restrict__ remap) {
    compact_chunk(
        n, offsets,
        [&](unsigned long long v) {
            const unsigned l = label[v];
            return cc_kept(k, l, count[l]) ? 1u : 0u;
        },
        [&](unsigned long long v, unsigned long long o, unsigned) {
            if (o >= cap) return;
            remap[v] = (unsigned)o;
            out_xyz[3 * o + 0] = xyz[3 * v + 0]; out_xyz[3 * o + 1] = xyz[3 * v + 1]; out_xyz[3 * o + 2] = xyz[3 * v + 2];
            if (rgb) { out_rgb[3 * o + 0] = rgb[3 * v + 0]; out_rgb[3 * o + 1] = rgb[3 * v + 1]; out_rgb[3 * o + 2] = rgb[3 * v + 2]; }
        });
}

__global__ __launch_bounds__(256) void cc_tri_write_kernel(CcKeep k, const unsigned *__restrict__ tri, unsigned long long n_tri,
                                                           const unsigned *__restrict__ label, const unsigned *__restrict__ count,
                                                           const unsigned long long *__restrict__ offsets, const unsigned *__restrict__ remap,
                                                           unsigned *__restrict__ out_tri, unsigned long long cap) {
    unsigned a = 0, b = 0, c = 0;                // of the triangle at hand: read by the count step, mapped by the emit step
    compact_chunk(
        n_tri, offsets,
        [&](unsigned long long t) {
            a = tri[3 * t]; b = tri[3 * t + 1]; c = tri[3 * t + 2];
            const unsigned l = label[a];
            return cc_kept(k, l, count[l]) ? 1u : 0u;
        },
        [&](unsigned long long, unsigned long long o, unsigned) {
            if (o >= cap) return;                // a kept triangle's vertices are kept: their remap entries were written
            out_tri[3 * o + 0] = remap[a]; out_tri[3 * o + 1] = remap[b]; out_tri[3 * o + 2] = remap[c];
        });
}

// info[0] (a u32 word) = the largest index of tri[0, 3 * n_tri); the caller zeroed it
int launch_cc_validate(hipStream_t s, const unsigned *tri, long long n_tri, unsigned long long *info) {
    if (n_tri <= 0) return TL3D_OK;
    const unsigned long long n = 3ull * (unsigned long long)n_tri;
    unsigned blocks = blocks_of(n, 256 * 8);
    if (blocks > 4096) blocks = 4096;
    hipLaunchKernelGGL(cc_validate_kernel, dim3(blocks), dim3(256), 0, s, tri, n, (unsigned *)info);
    TL3D_HIP(hipGetLastError());
    return TL3D_OK;
}

// parent -> labels, count[label] = triangles, info[1] = components, info[2] = key of the largest (indices already validated)
int launch_cc_label(hipStream_t s, const unsigned *tri, long long n_tri, long long n_vert, unsigned *parent, unsigned *count,
                    unsigned long long *info) {
    if (n_vert <= 0) return TL3D_OK;
    const unsigned nv = (unsigned)n_vert, vb = blocks_of((unsigned long long)n_vert, 256), tb = blocks_of((unsigned long long)n_tri, 256);
    hipLaunchKernelGGL(cc_init_kernel, dim3(vb), dim3(256), 0, s, parent, count, nv);
    TL3D_HIP(hipGetLastError());
    if (n_tri > 0) {
        hipLaunchKernelGGL(cc_hook_kernel, dim3(tb), dim3(256), 0, s, tri, (unsigned long long)n_tri, parent);
        TL3D_HIP(hipGetLastError());
        hipLaunchKernelGGL(cc_flatten_kernel, dim3(vb), dim3(256), 0, s, parent, nv);
        TL3D_HIP(hipGetLastError());
        hipLaunchKernelGGL(cc_count_kernel, dim3(tb), dim3(256), 0, s, tri, (unsigned long long)n_tri, parent, count);
        TL3D_HIP(hipGetLastError());
    }
    hipLaunchKernelGGL(cc_roots_kernel, dim3(vb), dim3(256), 0, s, parent, count, nv, info);
    TL3D_HIP(hipGetLastError());
    return TL3D_OK;
}

static CcKeep cc_keep(long long min_tri, int largest, const unsigned long long *info) { return CcKeep{min_tri, largest, info}; }

// per-chunk kept counts of vertices (vcounts) and triangles (tcounts); keep_out may be null; info[3] += kept components
int launch_cc_keep_count(hipStream_t s, long long min_tri, int largest, const unsigned *tri, long long n_tri, long long n_vert,
                         const unsigned *label, const unsigned *count, unsigned *vcounts, unsigned *tcounts, uint8_t *keep_out,
                         unsigned long long *info) {
    const CcKeep k = cc_keep(min_tri, largest, info);
    if (n_vert > 0) {
        hipLaunchKernelGGL(cc_vert_count_kernel, dim3(chunks_of(n_vert)), dim3(256), 0, s, k, label, count,
                           (unsigned)n_vert, vcounts, keep_out, info);
        TL3D_HIP(hipGetLastError());
    }
    if (n_tri > 0) {
        hipLaunchKernelGGL(cc_tri_count_kernel, dim3(chunks_of(n_tri)), dim3(256), 0, s, k, tri,
                           (unsigned long long)n_tri, label, count, tcounts);
        TL3D_HIP(hipGetLastError());
    }
    return TL3D_OK;
}

int launch_cc_compact(hipStream_t s, long long min_tri, int largest, const unsigned *tri, long long n_tri, long long n_vert,
                      const unsigned *label, const unsigned *count, const unsigned long long *voffsets, const unsigned long long *toffsets,
                      const float *xyz, const uint8_t *rgb, float *out_xyz, uint8_t *out_rgb, unsigned long long vcap, unsigned *out_tri,
                      unsigned long long tcap, unsigned *remap, const unsigned long long *info) {
    const CcKeep k = cc_keep(min_tri, largest, info);
    if (n_vert > 0 && vcap > 0) {
        hipLaunchKernelGGL(cc_vert_write_kernel, dim3(chunks_of(n_vert)), dim3(256), 0, s, k, label, count,
                           (unsigned)n_vert, voffsets, xyz, rgb, out_xyz, out_rgb, vcap, remap);
        TL3D_HIP(hipGetLastError());
    }
    if (n_tri > 0 && tcap > 0) {
        hipLaunchKernelGGL(cc_tri_write_kernel, dim3(chunks_of(n_tri)), dim3(256), 0, s, k, tri,
                           (unsigned long long)n_tri, label, count, toffsets, remap, out_tri, tcap);
        TL3D_HIP(hipGetLastError());
    }
    return TL3D_OK;
}

}  // namespace tl3d
