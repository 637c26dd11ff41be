// kernels_depthfilter.hip -- flying pixels and small regions of a depth image (tl3d_filter_depth, tl3d_filter_depth_slots; DESIGN.md
// section 4.7).  No reference code: the reference fuses its depth maps as they come.  The rules are in tl3d.h; in short
//   valid(p)      d_p is finite and > 0 (the f32 pixel itself, or the u16 millimetres converted exactly; never the metres copy)
//   linked(p, q)  both valid and fabsf(d_q - d_p) <= jump * fminf(d_p, d_q): one rounded difference, one rounded product, one compare
//   stage A       a valid p with fewer than min_support linked pixels in its (2r+1)^2 window of the INPUT image becomes 0
//   stage B       4-connected regions of linked survivors; a region of fewer than min_region pixels becomes 0
// The filter only ever writes zeros, and only over valid pixels: an invalid pixel keeps its bytes.
//
// Passes, each its own launch on the context's stream (kernel boundaries are the ONLY ordering between them); blockIdx.z is the frame
// of the batch, and every frame has its own parent / size / mask arrays and its own counters, so a result cannot depend on batching:
//   support   256 threads = a 64 x 16 pixel tile (a wave per row, four rows per thread), the tile + a halo of r staged in LDS as f32;
//             writes the stage-A MASK (0 invalid, 1 valid and dropped, 2 valid and kept), never the image: every support test reads
//             the input
//   init      parent[p] = p, size[p] = 0                                      (stage B only, as the next two)
//   hook      the unites of unionfind.h (obligations I1-I6).  A wave holds 64 consecutive pixels: a kept pixel linked to its left
//             neighbour unites with the first pixel of its run inside the wave (a tree of depth 1 instead of a chain), lane 0 with the
//             pixel in front of the wave; a kept pixel linked to the one below unites with it unless the square p-1, p, p+W-1, p+W
//             already joins them (p-1 ~ p, p-1 ~ p+W-1 by ITS unite, p+W-1 ~ p+W in the lower row).  The unites made span the same
//             graph as "every pixel with its right and lower neighbour", so the regions are the same.
//   count     size[find(p)] += 1: a wave walks eight strips of 64 pixels and carries (root, count) while the root stays the same, the
//             waves of a block merge what they carry in LDS: one add per 2048 pixels inside a large region; the roots are the regions
//   apply     zero where mask == 1, or mask == 2 and size[find(p)] < min_region
// Integer atomics commute and the output holds no label, so every order of the unites gives the same bytes.
// The counters {valid in, removed by A, regions, removed by B} of a frame are DF_SHARDS partial sums, each in a 128-B line of its
// own (a block adds to the shard of its number; the host sums them): one counter word per frame would serialise every block of the
// frame on one cache line.
#include <algorithm>
#include <vector>

#include "api_host.h"
#include "unionfind.h"

namespace tl3d {

constexpr int DF_TW = 64, DF_TH = 16;                // the support pass' pixel tile: 256 threads, a wave per row, four rows each
constexpr int DF_PER = 4;                            // strips of 256 pixels a block of the init and apply passes walks
constexpr int DF_SHARDS = 32, DF_SHARD_WORDS = 16;   // partial counters per frame, words (8 B) between two of them
constexpr int DF_STRIPS = 8;                         // strips of 256 pixels a block of the count pass walks

struct DfBatch {                                     // the frames of one launch
    void *img[DF_MAXBATCH];                          // [H][W] f32 or u16: read by support and hook, zeroed by apply
    float *f32[DF_MAXBATCH];                         // a u16 slot's f32 copy (zeroed with it), or null
    unsigned long long *cnt[DF_MAXBATCH];            // the frame's counters: [DF_SHARDS][DF_SHARD_WORDS], words 0..3 in use
};

template <class T> __device__ __forceinline__ float df_value(const T *img, size_t i);
template <> __device__ __forceinline__ float df_value<float>(const float *img, size_t i) { return img[i]; }
template <> __device__ __forceinline__ float df_value<uint16_t>(const uint16_t *img, size_t i) { return (float)img[i]; }   // exact

__device__ __forceinline__ bool df_valid(float d) { return d > 0.0f && d <= 3.402823466e+38f; }      // false for NaN
__device__ __forceinline__ bool df_linked(float dp, float dq, float jump) {                          // both valid, or dq NaN: false
    return fabsf(dq - dp) <= jump * fminf(dp, dq);
}

// the block's sums of a and b added to words wa and wb of the block's shard; every thread of the block calls it
__device__ __forceinline__ void df_count(unsigned long long *cnt, unsigned block_no, int wa, unsigned a, int wb, unsigned b) {
    __shared__ unsigned part[2][4];
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
        a += __shfl_down(a, d);
        b += __shfl_down(b, d);
    }
    if ((threadIdx.x & 63) == 0) {
        part[0][threadIdx.x >> 6] = a;
        part[1][threadIdx.x >> 6] = b;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long *dst = cnt + (size_t)(block_no % DF_SHARDS) * DF_SHARD_WORDS;
        const unsigned sa = part[0][0] + part[0][1] + part[0][2] + part[0][3], sb = part[1][0] + part[1][1] + part[1][2] + part[1][3];
        if (sa) atomicAdd(dst + wa, (unsigned long long)sa);
        if (sb) atomicAdd(dst + wb, (unsigned long long)sb);
    }
}

template <int R, class T>
__global__ __launch_bounds__(256) void df_support_kernel(DfBatch b, int W, int H, float jump, int min_support, uint8_t *__restrict__ mask) {
    constexpr int LW = DF_TW + 2 * R, LH = DF_TH + 2 * R;
    __shared__ float tile[LH][LW];
    const int f = blockIdx.z;
    const T *__restrict__ img = (const T *)b.img[f];
    const int x0 = blockIdx.x * DF_TW, y0 = blockIdx.y * DF_TH;
    for (int i = threadIdx.x; i < LW * LH; i += 256) {
        const int ly = i / LW, lx = i - ly * LW;
        const int x = x0 + lx - R, y = y0 + ly - R;
        // an invalid pixel, and one outside the image, is staged as NaN: it fails df_linked with every valid pixel (fminf gives the
        // valid operand, the difference is NaN, the compare false), so the window loop needs no validity test of its own
        const float v = (x >= 0 && x < W && y >= 0 && y < H) ? df_value<T>(img, (size_t)y * W + x) : 0.0f;
        tile[ly][lx] = df_valid(v) ? v : __builtin_nanf("");
    }
    __syncthreads();
    const int lx = threadIdx.x & (DF_TW - 1), x = x0 + lx;
    unsigned n_valid = 0, n_drop = 0;
    for (int ly = threadIdx.x / DF_TW; ly < DF_TH; ly += 256 / DF_TW) {
        const int y = y0 + ly;
        const bool in = x < W && y < H;
        const float dp = tile[ly + R][lx + R];
        const bool valid = in && dp == dp;
        int s = 0;
        if (valid) {
#pragma unroll
            for (int dy = -R; dy <= R; ++dy)
#pragma unroll
                for (int dx = -R; dx <= R; ++dx) {
                    if (dx == 0 && dy == 0) continue;
                    s += df_linked(dp, tile[ly + R + dy][lx + R + dx], jump) ? 1 : 0;
                }
        }
        const bool keep = valid && s >= min_support;
        if (in) mask[(size_t)f * W * H + (size_t)y * W + x] = valid ? (keep ? 2 : 1) : 0;
        n_valid += valid ? 1u : 0u;
        n_drop += (valid && !keep) ? 1u : 0u;
    }
    df_count(b.cnt[f], blockIdx.x + blockIdx.y * gridDim.x, 0, n_valid, 1, n_drop);
}

__global__ __launch_bounds__(256) void df_init_kernel(unsigned *__restrict__ parent, unsigned *__restrict__ size, unsigned npx) {
#pragma unroll
    for (int k = 0; k < DF_PER; ++k) {
        const unsigned long long p = ((unsigned long long)blockIdx.x * DF_PER + k) * 256u + threadIdx.x;
        if (p < npx) {
            const size_t o = (size_t)blockIdx.z * npx + p;
            parent[o] = (unsigned)p;
            size[o] = 0u;
        }
    }
}

template <class T>
__global__ __launch_bounds__(256) void df_hook_kernel(DfBatch b, int W, int H, float jump, const uint8_t *__restrict__ mask, unsigned *parent) {
    const unsigned npx = (unsigned)W * (unsigned)H;
    const unsigned p = blockIdx.x * 256u + threadIdx.x;                  // (no thread leaves before the ballots)
    const int f = blockIdx.z, lane = threadIdx.x & 63;
    const uint8_t *__restrict__ m = mask + (size_t)f * npx;
    const T *__restrict__ img = (const T *)b.img[f];
    unsigned *par = parent + (size_t)f * npx;
    const bool kept = p < npx && m[p] == 2;
    unsigned x = 0, y = 0;
    float dp = 0.0f, dlow = 0.0f;
    bool hl = false, vl = false;                                         // linked to the left neighbour, to the lower one
    if (kept) {
        y = p / (unsigned)W;
        x = p - y * (unsigned)W;
        dp = df_value<T>(img, p);
        hl = x > 0 && m[p - 1] == 2 && df_linked(dp, df_value<T>(img, p - 1), jump);
        if (y + 1 < (unsigned)H && m[p + W] == 2) {
            dlow = df_value<T>(img, (size_t)p + W);
            vl = df_linked(dp, dlow, jump);
        }
    }
    const unsigned long long hmask = __ballot(hl), vmask = __ballot(vl);
    if (!kept) return;
    if (hl) {
        if (lane == 0) {
            cc_unite(par, p, p - 1);
        } else {
            // the first lane of this lane's run: the highest lane <= this one that is not linked to its left inside the wave
            const unsigned long long heads = (~hmask | 1ull) & (~0ull >> (63 - lane));
            const int head = 63 - __clzll((long long)heads);
            cc_unite(par, p, p - (unsigned)(lane - head));
        }
    }
    if (vl) {
        // p-1 ~ p (hl: the same row), p-1 ~ p+W-1 (lane - 1 makes that unite, or finds it made the same way), p+W-1 ~ p+W: nothing to add
        const bool square = lane > 0 && hl && ((vmask >> (lane - 1)) & 1ull) && df_linked(df_value<T>(img, (size_t)p + W - 1), dlow, jump);
        if (!square) cc_unite(par, p, p + (unsigned)W);
    }
}

// size[root] += pixels of the root; cnt[2] += roots.  A block walks DF_STRIPS strips of 256 pixels; a wave carries the (root, count)
// of its last group from strip to strip and adds a group to memory only when another root takes its place; what the four waves
// still carry at the end is merged in LDS.
__global__ __launch_bounds__(256) void df_count_kernel(DfBatch b, unsigned npx, const uint8_t *__restrict__ mask, unsigned *parent,
                                                       unsigned *__restrict__ size) {
    __shared__ unsigned car_root[4], car_cnt[4];
    const int f = blockIdx.z, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint8_t *__restrict__ m = mask + (size_t)f * npx;
    unsigned *par = parent + (size_t)f * npx, *sz = size + (size_t)f * npx;
    unsigned roots = 0;
    unsigned carry_root = 0xFFFFFFFFu, carry_cnt = 0;                    // wave-uniform
    for (int s = 0; s < DF_STRIPS; ++s) {
        const unsigned long long p64 = ((unsigned long long)blockIdx.x * DF_STRIPS + s) * 256u + threadIdx.x;
        const bool kept = p64 < npx && m[p64] == 2;
        unsigned r = 0xFFFFFFFFu;
        if (kept) {
            r = cc_find(par, (unsigned)p64);
            roots += r == (unsigned)p64 ? 1u : 0u;
        }
        unsigned long long todo = __ballot(kept);
        while (todo) {                                                   // (wave-uniform loop: every lane takes part in the ballots)
            const int lead = __ffsll((long long)todo) - 1;
            const unsigned first = (unsigned)__shfl((int)r, lead);
            const unsigned long long same = __ballot(kept && r == first) & todo;
            const unsigned n = (unsigned)__popcll(same);
            if (first == carry_root) {
                carry_cnt += n;
            } else {
                if (carry_cnt && lane == 0) atomicAdd(sz + carry_root, carry_cnt);
                carry_root = first;
                carry_cnt = n;
            }
            todo &= ~same;
        }
    }
    if (lane == 0) {
        car_root[wave] = carry_root;
        car_cnt[wave] = carry_cnt;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            unsigned n = car_cnt[w];
            if (!n) continue;
#pragma unroll
            for (int v = w + 1; v < 4; ++v)
                if (car_cnt[v] && car_root[v] == car_root[w]) {
                    n += car_cnt[v];
                    car_cnt[v] = 0;
                }
            atomicAdd(sz + car_root[w], n);
        }
    }
    df_count(b.cnt[f], blockIdx.x, 2, roots, 3, 0u);
}

template <class T>
__global__ __launch_bounds__(256) void df_apply_kernel(DfBatch b, unsigned npx, long long min_region, const uint8_t *__restrict__ mask,
                                                       unsigned *parent, const unsigned *__restrict__ size) {
    const int f = blockIdx.z;
    unsigned n_small = 0;
#pragma unroll
    for (int k = 0; k < DF_PER; ++k) {
        const unsigned long long p = ((unsigned long long)blockIdx.x * DF_PER + k) * 256u + threadIdx.x;
        const unsigned m = p < npx ? mask[(size_t)f * npx + p] : 0u;
        bool small = false;
        if (m == 2 && min_region > 1) {
            const unsigned r = cc_find(parent + (size_t)f * npx, (unsigned)p);
            small = (long long)size[(size_t)f * npx + r] < min_region;
        }
        if (m == 1 || small) {
            ((T *)b.img[f])[p] = (T)0;
            if (b.f32[f]) b.f32[f][p] = 0.0f;
        }
        n_small += small ? 1u : 0u;
    }
    if (min_region > 1) df_count(b.cnt[f], blockIdx.x, 3, n_small, 2, 0u);
}

template <int R, class T> static void df_launch_support(hipStream_t s, dim3 g, const DfBatch &b, int W, int H, float jump, int ms, uint8_t *mask) {
    hipLaunchKernelGGL((df_support_kernel<R, T>), g, dim3(256), 0, s, b, W, H, jump, ms, mask);
}
template <class T> static void df_launch_support_r(hipStream_t s, dim3 g, int radius, const DfBatch &b, int W, int H, float jump, int ms, uint8_t *mask) {
    if (radius == 1) df_launch_support<1, T>(s, g, b, W, H, jump, ms, mask);
    else if (radius == 2) df_launch_support<2, T>(s, g, b, W, H, jump, ms, mask);
    else df_launch_support<3, T>(s, g, b, W, H, jump, ms, mask);
}

// Filters n images of the context's W x H in place on its stream.  img[i]: device f32 or u16 (kinds[i]); f32[i]: a u16 image's f32
// copy to zero with it, or null.  The parameters have been checked.  counts (host, [n][4]) may be null; with it the call waits.
int depth_filter_run(tl3d_ctx *ctx, int n, void *const *img, float *const *f32, const int *kinds, const tl3d_depth_filter_params &prm,
                     long long *counts) {
    if (n <= 0) return TL3D_OK;
    const int W = ctx->cam.W, H = ctx->cam.H;
    const size_t npx = (size_t)W * (size_t)H;
    if (npx == 0 || npx >= (1ull << 31)) return set_err(TL3D_E_INVALID, "a depth image of %zu pixels: the filter indexes 0 < W * H < 2^31", npx);
    const bool regions = prm.min_region > 1;
    // frames per launch: at most DF_MAXBATCH, and no more than keep the scratch below a quarter GiB (one frame always goes)
    int nb = (int)std::min<size_t>((size_t)DF_MAXBATCH, std::max<size_t>(1, ((size_t)1 << 28) / (npx * 9)));
    nb = std::min(nb, n);
    constexpr size_t frame_words = (size_t)DF_SHARDS * DF_SHARD_WORDS;
    const size_t bytes[4] = {(size_t)n * frame_words * sizeof(unsigned long long), (size_t)nb * npx, regions ? (size_t)nb * npx * 4 : 0,
                             regions ? (size_t)nb * npx * 4 : 0};
    void *arr[4];
    int rc = scratch_carve(ctx, 0, bytes, 4, arr, "depth filter scratch");
    if (rc) return rc;
    unsigned long long *d_cnt = (unsigned long long *)arr[0];
    uint8_t *mask = (uint8_t *)arr[1];
    unsigned *parent = (unsigned *)arr[2], *size = (unsigned *)arr[3];
    hipStream_t s = ctx->stream;
    TL3D_HIP(hipMemsetAsync(d_cnt, 0, bytes[0], s));
    const float jump = (float)prm.jump_rel;
    const unsigned lin = (unsigned)((npx + 255) / 256), strips = (unsigned)((npx + 256 * DF_STRIPS - 1) / (256 * DF_STRIPS));
    for (int i0 = 0; i0 < n;) {
        DfBatch b;
        memset(&b, 0, sizeof(b));
        int k = 0;
        while (i0 + k < n && k < nb && kinds[i0 + k] == kinds[i0]) {     // a launch holds one kind
            b.img[k] = img[i0 + k];
            b.f32[k] = f32 ? f32[i0 + k] : nullptr;
            b.cnt[k] = d_cnt + frame_words * (size_t)(i0 + k);
            ++k;
        }
        const bool u16 = kinds[i0] == TL3D_DEPTH_U16_MM;
        const dim3 gt((W + DF_TW - 1) / DF_TW, (H + DF_TH - 1) / DF_TH, k), gl(lin, 1, k), gs(strips, 1, k), gp((lin + DF_PER - 1) / DF_PER, 1, k);
        if (u16) df_launch_support_r<uint16_t>(s, gt, prm.radius, b, W, H, jump, prm.min_support, mask);
        else df_launch_support_r<float>(s, gt, prm.radius, b, W, H, jump, prm.min_support, mask);
        if (regions) {
            hipLaunchKernelGGL(df_init_kernel, gp, dim3(256), 0, s, parent, size, (unsigned)npx);
            if (u16) hipLaunchKernelGGL(df_hook_kernel<uint16_t>, gl, dim3(256), 0, s, b, W, H, jump, mask, parent);
            else hipLaunchKernelGGL(df_hook_kernel<float>, gl, dim3(256), 0, s, b, W, H, jump, mask, parent);
            hipLaunchKernelGGL(df_count_kernel, gs, dim3(256), 0, s, b, (unsigned)npx, mask, parent, size);
        }
        if (u16) hipLaunchKernelGGL(df_apply_kernel<uint16_t>, gp, dim3(256), 0, s, b, (unsigned)npx, (long long)prm.min_region, mask, parent, size);
        else hipLaunchKernelGGL(df_apply_kernel<float>, gp, dim3(256), 0, s, b, (unsigned)npx, (long long)prm.min_region, mask, parent, size);
        TL3D_HIP(hipGetLastError());
        i0 += k;
    }
    if (counts) {
        std::vector<unsigned long long> h((size_t)n * frame_words);
        TL3D_HIP(hipMemcpyAsync(h.data(), d_cnt, bytes[0], hipMemcpyDeviceToHost, s));
        TL3D_HIP(hipStreamSynchronize(s));
        for (int i = 0; i < n; ++i)
            for (int w = 0; w < 4; ++w) {
                unsigned long long sum = 0;
                for (int sh = 0; sh < DF_SHARDS; ++sh) sum += h[(size_t)i * frame_words + (size_t)sh * DF_SHARD_WORDS + w];
                counts[(size_t)i * 4 + w] = (long long)sum;
            }
    }
    return TL3D_OK;
}

}  // namespace tl3d
