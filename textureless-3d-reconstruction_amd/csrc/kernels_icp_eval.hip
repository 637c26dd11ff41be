// kernels_icp_eval.hip -- one point-to-plane pass for each of many pairs at GIVEN poses, no update (tl3d_icp_evaluate_pairs): the
// normal equations (A = sum J J^T, b = sum J r, e = sum r^2) and the counts of oracle/tl3d_oracle.c: icp_pass / orc_icp_sums.
// What a pose graph takes as the weight of an edge (the 6x6 A at the edge's pose) and what scores loop-closure candidates.
//
// The per-sample arithmetic and a workgroup's reduction are icp_accumulate_core (icp_sample.h), the code the registration kernels
// run: same source vertex (the window-averaged depth when normal smoothing is on), same fmaf chains, association, gate, residual
// and J, f32 values added as fp64 sums of fp64 products.
//
// Two launches on one stream, and nothing handed from workgroup to workgroup inside a launch:
//   icp_eval_kernel      grid = (members, pairs): workgroup (m, p) takes samples m * 256 + tid, + members * 256, ... of pair p and
//                        writes its 32 partial sums (21 + 6 + 1 sums, the two counts, two zeros) to slab[p][m][0..31];
//   icp_eval_sum_kernel  one wave per pair adds the pair's partials in member order.
// The kernel boundary orders the two.  `members` is a function of the level geometry (samples of a frame at the stride) only, so a
// pair's sums are bit for bit the same whatever batch it is in, wherever in the batch, in every run.
// Bytes per sampled pixel: 4 (source depth) + 16 (target normal + depth gather) = 20 B.
#include "tl3d_internal.h"
#include "icp_sample.h"

namespace tl3d {

constexpr int ICP_EVAL_RAY_TAB_MAX = 12288;                // floats of LDS for the pixel-ray factors (48 KB), as the batched registration

// TAB: the pixel-ray factors of the W columns and H rows sit in dynamic LDS (icp_accumulate_core: ray_tab)
template <bool TAB>
__global__ __launch_bounds__(256, 2) void icp_eval_kernel(Cam cam, const IcpEvalPair *__restrict__ pairs, float mind, float maxd, float md2,
                                                          int stride, int Ws, int Hs, double *__restrict__ slab) {
    __shared__ double sm[4][ICP_SLAB];
    __shared__ double tot[ICP_SLAB];
    extern __shared__ float eval_ray_tab[];                // TAB: [W] x factors, then [H] y factors
    const int tid = threadIdx.x;
    if (TAB) {
        for (int i = tid; i < cam.W; i += 256) eval_ray_tab[i] = ((float)i - cam.cx) / cam.fx;
        for (int i = tid; i < cam.H; i += 256) eval_ray_tab[cam.W + i] = ((float)i - cam.cy) / cam.fy;
        __syncthreads();
    }
    const int pair = blockIdx.y, member = blockIdx.x, members = gridDim.x;
    const IcpEvalPair *pr = pairs + pair;
    // the pose is the same in every lane: scalar registers
    auto uni = [](float x) { return __uint_as_float(__builtin_amdgcn_readfirstlane(__float_as_uint(x))); };
    float r[9], t[3];
    r[0] = uni(pr->T[0]); r[1] = uni(pr->T[1]); r[2] = uni(pr->T[2]);  t[0] = uni(pr->T[3]);
    r[3] = uni(pr->T[4]); r[4] = uni(pr->T[5]); r[5] = uni(pr->T[6]);  t[1] = uni(pr->T[7]);
    r[6] = uni(pr->T[8]); r[7] = uni(pr->T[9]); r[8] = uni(pr->T[10]); t[2] = uni(pr->T[11]);
    const float sc = uni(pr->scale);
    icp_accumulate_core<false, TAB>(cam, pr->depth_src, pr->nmap_tgt, sc, mind, maxd, md2, stride, Ws, Hs, r, t, member, members, pr->src_pm, sm, tot,
                                    nullptr, eval_ray_tab);
    if (tid < ICP_EVAL_SUMS) slab[((size_t)pair * members + member) * ICP_EVAL_SUMS + tid] = tot[tid];
}

// out[pair][c] = slab[pair][0][c] + slab[pair][1][c] + ... in member order: lane c < 32 of the pair's wave owns component c
__global__ __launch_bounds__(64) void icp_eval_sum_kernel(const double *__restrict__ slab, int members, double *__restrict__ out) {
    const int pair = blockIdx.x, c = threadIdx.x;
    if (c >= ICP_EVAL_SUMS) return;
    const double *p = slab + (size_t)pair * members * ICP_EVAL_SUMS + c;
    double s = 0.0;
    int m = 0;
    for (; m + 8 <= members; m += 8) {                     // loads batched 8 deep, added in order
        double v[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) v[k] = p[(size_t)(m + k) * ICP_EVAL_SUMS];
#pragma unroll
        for (int k = 0; k < 8; ++k) s += v[k];
    }
    for (; m < members; ++m) s += p[(size_t)m * ICP_EVAL_SUMS];
    out[(size_t)pair * ICP_EVAL_SUMS + c] = s;
}

int icp_eval_members(int Ws, int Hs) {
    long long m = ((long long)Ws * Hs + ICP_EVAL_SAMPLES_PER_MEMBER - 1) / ICP_EVAL_SAMPLES_PER_MEMBER;
    if (m < 1) m = 1;
    if (m > ICP_EVAL_MEMBERS_CAP) m = ICP_EVAL_MEMBERS_CAP;
    return (int)m;
}

// pairs, slab ([n_pairs][members][32]) and out ([n_pairs][32]) are device memory; n_pairs <= 65535 (grid.y)
int launch_icp_eval(hipStream_t s, const Cam &cam, const IcpEvalPair *pairs, int n_pairs, int members, float mind, float maxd, float md2, int stride,
                    int Ws, int Hs, double *slab, double *out) {
    if (n_pairs <= 0) return TL3D_OK;
    const bool tab = cam.W + cam.H <= ICP_EVAL_RAY_TAB_MAX;
    const size_t lds = tab ? (size_t)(cam.W + cam.H) * sizeof(float) : 0;
    if (tab)
        hipLaunchKernelGGL(icp_eval_kernel<true>, dim3(members, n_pairs), dim3(256), lds, s, cam, pairs, mind, maxd, md2, stride, Ws, Hs, slab);
    else
        hipLaunchKernelGGL(icp_eval_kernel<false>, dim3(members, n_pairs), dim3(256), 0, s, cam, pairs, mind, maxd, md2, stride, Ws, Hs, slab);
    TL3D_HIP(hipGetLastError());
    hipLaunchKernelGGL(icp_eval_sum_kernel, dim3(n_pairs), dim3(64), 0, s, slab, members, out);
    TL3D_HIP(hipGetLastError());
    return TL3D_OK;
}

}  // namespace tl3d
