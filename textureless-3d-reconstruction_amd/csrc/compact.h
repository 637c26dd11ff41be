// compact.h -- the device half of the order-preserving compaction that point extraction, mesh extraction, the component filter and
// vertex clustering share (DESIGN.md sections 4, 4.2.1, 4.2.2).  A block of 256 threads owns a chunk of EXTRACT_CHUNK consecutive
// elements and walks it in eight iterations of 256, thread order = element order:
//   count pass   per-chunk totals (block_sum)                      -> counts[chunk]
//   scan         one single-block launch (kernels_compact.hip)     -> offsets[chunk], the grand total behind the last chunk
//   write pass   compact_chunk: an exclusive scan inside each iteration; element idx writes at offsets[chunk] + its rank
//
// THE BARRIER RULE.  block_sum and block_excl hold two __syncthreads() each, so every thread of the block must reach every call
// of them.  Hence: nothing inside a for_chunk body or in front of a block_sum returns or `continue`s; an element beyond the end
// counts 0 and still takes part.  compact_chunk upholds this for its callers (count and emit are only ever skipped, never the
// scan between them); a loop written by hand on block_excl has to uphold it itself.
#pragma once
#include "tl3d_internal.h"

namespace tl3d {

// block total of c over the 256 threads (every thread must call); T: unsigned, or unsigned long long where a chunk's total can
// pass 2^32 (the adjacency rows of kernels_meshsmooth.hip)
template <class T> __device__ __forceinline__ T block_sum(T c, T *sm) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) c += __shfl_down(c, d);
    if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = c;
    __syncthreads();
    const T s = sm[0] + sm[1] + sm[2] + sm[3];
    __syncthreads();
    return s;
}

// exclusive prefix of c over the block (thread order = element order inside one iteration) and the block's total
template <class T> __device__ __forceinline__ T block_excl(T c, T *sm, T &total) {
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    T inc = c;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const T tv = __shfl_up(inc, d);
        if (lane >= d) inc += tv;
    }
    if (lane == 63) sm[wid] = inc;
    __syncthreads();
    T wbase = 0;
    for (int w = 0; w < wid; ++w) wbase += sm[w];
    total = sm[0] + sm[1] + sm[2] + sm[3];
    __syncthreads();
    return wbase + inc - c;
}

// body(idx) for this thread's element of each of the chunk's eight iterations, in order; idx may lie beyond the end
template <class Body> __device__ __forceinline__ void for_chunk(Body body) {
    const unsigned long long base = (unsigned long long)blockIdx.x * EXTRACT_CHUNK;
#pragma unroll 1
    for (int it = 0; it < EXTRACT_CHUNK / 256; ++it) body(base + (unsigned long long)it * 256 + threadIdx.x);
}

// The write pass of one chunk.  count(idx) -> the number of outputs of element idx, asked only for idx < n; emit(idx, o, c) writes
// them at o, o + 1, .. o + c - 1 and is called only when c != 0.  What count finds out about an element and emit needs again lives
// in a local of the kernel that both lambdas capture by reference.
template <class Count, class Emit>
__device__ __forceinline__ void compact_chunk(unsigned long long n, const unsigned long long *__restrict__ offsets, Count count, Emit emit) {
    __shared__ unsigned sm[4];
    unsigned long long run = offsets[blockIdx.x];
    for_chunk([&](unsigned long long idx) {
        const unsigned c = idx < n ? count(idx) : 0u;
        unsigned total;
        const unsigned ex = block_excl(c, sm, total);
        if (c) emit(idx, run + ex, c);
        run += total;
    });
}

}  // namespace tl3d
