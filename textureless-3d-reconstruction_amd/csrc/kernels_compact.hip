// kernels_compact.hip -- the scan between the count pass and the write pass of the order-preserving compaction (compact.h): the
// per-chunk counts of one launch -> 64-bit offsets and the grand total.  One block: its callers (point and mesh extraction, the
// two mesh clean-up calls) have at most a few thousand chunks, the cell index (kernels_cellgrid.hip) at most 2^17 chunk sums.
#include "tl3d_internal.h"

namespace tl3d {

// single-block exclusive scan of n block counts -> 64-bit offsets (+ total); C: the counts' type (64-bit for the adjacency rows of
// kernels_meshsmooth.hip, where one chunk's count can pass 2^32)
template <class C>
__global__ __launch_bounds__(1024) void scan_kernel(const C *__restrict__ counts, unsigned long long *__restrict__ offsets,
                                                    int n, unsigned long long *__restrict__ total) {
    __shared__ unsigned long long part[1024];
    const int t = threadIdx.x;
    const int per = (n + 1023) / 1024;
    const int lo = t * per, hi = min(n, lo + per);
    unsigned long long s = 0;
    for (int i = lo; i < hi; ++i) s += counts[i];
    part[t] = s;
    __syncthreads();
    for (int off = 1; off < 1024; off <<= 1) {
        unsigned long long v = (t >= off) ? part[t - off] : 0ull;
        __syncthreads();
        part[t] += v;
        __syncthreads();
    }
    unsigned long long run = part[t] - s;          // exclusive prefix of this thread's span
    for (int i = lo; i < hi; ++i) {
        offsets[i] = run;
        run += counts[i];
    }
    if (t == 1023) *total = part[1023];
}

int launch_scan(hipStream_t s, const unsigned *counts, unsigned long long *offsets, int n, unsigned long long *total) {
    hipLaunchKernelGGL(scan_kernel<unsigned>, dim3(1), dim3(1024), 0, s, counts, offsets, n, total);
    TL3D_HIP(hipGetLastError());
    return TL3D_OK;
}

int launch_scan(hipStream_t s, const unsigned long long *counts, unsigned long long *offsets, int n, unsigned long long *total) {
    hipLaunchKernelGGL(scan_kernel<unsigned long long>, dim3(1), dim3(1024), 0, s, counts, offsets, n, total);
    TL3D_HIP(hipGetLastError());
    return TL3D_OK;
}

}  // namespace tl3d
