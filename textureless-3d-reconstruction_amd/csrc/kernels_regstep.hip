// kernels_regstep.hip -- the step behind a pass of tracking (kernels_track.hip), of the joint colour registration (kernels_rgbd.hip)
// and of cloud registration (kernels_cloudicp.hip).  A step is ONE wave per pair, after the pass on the same stream: it adds the
// pass's partials in member order (lane c owns sum c), keeps them in the pair's state and, for STEP_ITERATE, solves the damped system
// (reg_solve.h) and updates the pose in device memory; the other kinds end a level (StepKind, tl3d_internal.h).  Everything a step
// reads was written by earlier launches and everything it writes is read by later ones: plain stores (the agent-scope hand-off inside
// a launch is the pairwise ICP's, kernels_icp.hip: icp_finish).
// The rules exist once, below.  What the three registrations do NOT share is at their kernels' call sites:
//   correspondences an iteration needs    tracking 8, colour and cloud 6 (fewer: the run fails)
//   the update's sign                     tracking applies -x: its Jacobian moves the point, not the camera (kernels_track.hip, SIGN)
//   the system                            colour solves A_g + w A_p, formed in fp64 from its 64 sums; the others solve their sums
//   unknowns                              the cloud step alone has the 7-unknown (scale) instantiation
#include "tl3d_internal.h"
#include "reg_solve.h"

namespace tl3d {

// a run that is over, or a level that has converged or failed, makes its remaining launches return at once
__device__ __forceinline__ bool step_idle(const IcpState *state, StepKind kind) { return state->over || (kind == STEP_ITERATE && state->done); }

// component c of a pair's sums: its `members` partials of WIDTH doubles, in member order
template <int WIDTH>
__device__ __forceinline__ double step_member_sum(const double *__restrict__ slab, int members, int c) {
    double s = 0.0;
    for (int m = 0; m < members; ++m) s += slab[(size_t)m * WIDTH + c];
    return s;
}

// lane 0, STEP_END_LEVEL / STEP_END_RUN: the run is over behind its last level, a failed one, or one that ended with fewer than 8
// correspondences; else the next level starts with done / status / iters_run re-armed
__device__ __forceinline__ void step_end_level(IcpState *state, StepKind kind, double n_corr) {
    if (threadIdx.x != 0) return;
    if (kind == STEP_END_RUN || state->status == 2 || n_corr < 8.0) {
        state->over = 1;
    } else {
        state->done = 0;
        state->status = 0;
        state->iters_run = 0;
    }
}

// The whole wave, STEP_ITERATE.  sys: a[21] b[6] laid out as the head of IcpState::sums (LDS); with SCALE all 40 sums, scale column
// included.  Fewer than `floor` correspondences or an unsolvable system fail the run: status 2, T the last good pose.  Else
// T <- exp(x) T (NEGATE: exp(-x)), with SCALE scale <- scale exp(x[6]), one more iteration run, and |x|_max < eps ends the level
// (status 1).  The 6 x 6 system is solved on the wave, the 7 x 7 one on lane 0 (and only that instantiation carries its scratch).
template <bool SCALE, bool NEGATE>
__device__ __forceinline__ void step_solve_update(IcpState *state, double n_corr, double floor, const double *sys, double damping, double eps,
                                                  double eig_rel) {
    constexpr int N = SCALE ? 7 : 6;
    double x[N];
    int fail = 0;
    if (SCALE) {
        if (threadIdx.x == 0) fail = (n_corr < floor) ? 1 : solve7_serial(sys, damping, eig_rel, x);
    } else {
        fail = (n_corr < floor) ? 1 : solve6_wave(sys, sys + 21, damping, eig_rel, x);      // wave-uniform
    }
    if (threadIdx.x != 0) return;
    if (fail) {
        state->done = 1;
        state->status = 2;
        return;
    }
    double mx = 0.0;
    for (int i = 0; i < N; ++i) {
        mx = fmax(mx, fabs(x[i]));
        if (NEGATE) x[i] = -x[i];
    }
    se3_apply(x, state->T);
    if (SCALE) state->scale = state->scale * exp(x[6]);
    state->iters_run = state->iters_run + 1;
    if (mx < eps) {
        state->done = 1;
        state->status = 1;
    }
}

__global__ __launch_bounds__(64) void track_step_kernel(const double *__restrict__ slab, int members, IcpState *state, double damping, double eps,
                                                        double eig_rel, StepKind kind) {
    if (step_idle(state, kind)) return;
    __shared__ double sums[TRACK_SUMS];
    const int c = threadIdx.x;
    if (c < TRACK_SUMS) state->sums[c] = sums[c] = step_member_sum<TRACK_SUMS>(slab, members, c);
    __syncthreads();
    if (kind != STEP_ITERATE) return step_end_level(state, kind, sums[ICP_SUM_CORR]);
    step_solve_update<false, true>(state, sums[ICP_SUM_CORR], 8.0, sums, damping, eps, eig_rel);
}

// one wave per pair; lane c owns sum c of the 64: [0, 32) to the pair's IcpState, [32, 64) to RgbdState::photo.  Damping and the
// eigenvalue cutoff act on the joint system A_g + weight A_p, b_g + weight b_p (a product, then a sum); the floor counts the
// GEOMETRIC correspondences.
__global__ __launch_bounds__(64) void rgbd_step_kernel(const double *__restrict__ slab, int members, RgbdState *states, double weight, double damping,
                                                       double eps, double eig_rel, StepKind kind) {
    RgbdState *st = states + blockIdx.x;
    IcpState *state = &st->icp;
    if (step_idle(state, kind)) return;
    __shared__ double sums[RGBD_SUMS];
    __shared__ double joint[27];
    const int c = threadIdx.x;
    sums[c] = step_member_sum<RGBD_SUMS>(slab + (size_t)blockIdx.x * members * RGBD_SUMS, members, c);
    if (c < 32) state->sums[c] = sums[c];
    else st->photo[c - 32] = sums[c];
    __syncthreads();
    if (kind != STEP_ITERATE) return step_end_level(state, kind, sums[ICP_SUM_CORR]);
    if (c < 27) joint[c] = sums[c] + weight * sums[32 + c];
    __syncthreads();
    step_solve_update<false, false>(state, sums[ICP_SUM_CORR], 6.0, joint, damping, eps, eig_rel);
}

// SCALE: the level estimates the source's scale (the 7 x 7 system).  The pass's J is the Jacobian for moving the SOURCE point by
// exp(x), and T maps source to target: no sign change.
template <bool SCALE>
__global__ __launch_bounds__(64) void cloud_step_kernel(const double *__restrict__ slab, int members, IcpState *state, double damping, double eps,
                                                        double eig_rel, StepKind kind) {
    if (step_idle(state, kind)) return;
    __shared__ double sums[CLOUD_SUMS];
    const int c = threadIdx.x;
    if (c < CLOUD_SUMS) state->sums[c] = sums[c] = step_member_sum<CLOUD_SUMS>(slab, members, c);
    __syncthreads();
    if (kind != STEP_ITERATE) return step_end_level(state, kind, sums[ICP_SUM_CORR]);
    step_solve_update<SCALE, false>(state, sums[ICP_SUM_CORR], 6.0, sums, damping, eps, eig_rel);
}

int launch_track_step(hipStream_t s, const double *slab, int members, IcpState *state, double damping, double eps, double eig_rel, StepKind kind) {
    hipLaunchKernelGGL(track_step_kernel, dim3(1), dim3(64), 0, s, slab, members, state, damping, eps, eig_rel, kind);
    TL3D_HIP(hipGetLastError());
    return TL3D_OK;
}

int launch_rgbd_step(hipStream_t s, const double *slab, int n_pairs, int members, RgbdState *states, double photo_weight, double damping,
                     double eps, double eig_rel, StepKind kind) {
    if (n_pairs <= 0) return TL3D_OK;
    hipLaunchKernelGGL(rgbd_step_kernel, dim3(n_pairs), dim3(64), 0, s, slab, members, states, photo_weight, damping, eps, eig_rel, kind);
    TL3D_HIP(hipGetLastError());
    return TL3D_OK;
}

int launch_cloud_step(hipStream_t s, const double *slab, int members, IcpState *state, int est_scale, double damping, double eps, double eig_rel,
                      StepKind kind) {
    hipLaunchKernelGGL(est_scale ? cloud_step_kernel<true> : cloud_step_kernel<false>, dim3(1), dim3(64), 0, s, slab, members, state, damping, eps,
                       eig_rel, kind);
    TL3D_HIP(hipGetLastError());
    return TL3D_OK;
}

}  // namespace tl3d
