// reg_solve.h -- what every registration's solve step shares (device only): the damped 6 x 6 solve on one wave (direct LDL^T path,
// else Jacobi eigen-decomposition with the relative eigenvalue cutoff), the serial solve for up to 7 unknowns (Sim(3)), the
// write-through state stores and the pose update T <- exp(x) T.  Sequences = oracle/tl3d_oracle.c (solve6, solve_n, se3_apply).
// Used by kernels_icp.hip (pairwise ICP: icp_finish) and kernels_regstep.hip (the steps of tracking, colour and cloud registration).
#pragma once
#include "tl3d_internal.h"

namespace tl3d {

// 1/x and 1/sqrt(x) to ~1e-16 relative: hardware seed + two Newton steps (no IEEE division / square-root sequence)
__device__ __forceinline__ double fast_rcp(double x) {
    double y = __builtin_amdgcn_rcp(x);
    double e = fma(-x, y, 1.0);
    y = fma(y, e, y);
    e = fma(-x, y, 1.0);
    return fma(y, e, y);
}
__device__ __forceinline__ double fast_rsq(double x) {
    double y = __builtin_amdgcn_rsq(x);
    double e = fma(-x * y, y, 1.0);
    y = fma(0.5 * y, e, y);
    e = fma(-x * y, y, 1.0);
    return fma(0.5 * y, e, y);
}

// Direct path of oracle/tl3d_oracle.c: solve6_direct, same sequence.  Every lane runs it redundantly (no shuffles, all
// indices static): ~250 dependent-ish fp64 operations instead of the eigen-decomposition's ~30 rounds of cross-lane
// exchanges (18 of the 34 us of an iteration).  Returns 1 and x when it applies; 0 -> the caller runs solve6_wave.
__device__ __forceinline__ int solve6_direct(const double *__restrict__ a21, const double *__restrict__ b, double lam,
                                             double eig_rel, double x[6]) {
    double A[6][6], L[6][6], M[6][6], d[6];
    {
        int m = 0;
#pragma unroll
        for (int i = 0; i < 6; ++i)
#pragma unroll
            for (int j = i; j < 6; ++j) { const double e = a21[m++]; A[i][j] = e; A[j][i] = e; }
#pragma unroll
        for (int i = 0; i < 6; ++i) A[i][i] += lam;
    }
    double tr = 0.0;
#pragma unroll
    for (int i = 0; i < 6; ++i) tr += A[i][i];
    bool ok = true;
#pragma unroll
    for (int j = 0; j < 6; ++j) {
        double s = A[j][j];
#pragma unroll
        for (int k = 0; k < j; ++k) s -= (L[j][k] * L[j][k]) * d[k];
        ok = ok && (s > 0.0);
        d[j] = s;
#pragma unroll
        for (int i = j + 1; i < 6; ++i) {
            double t = A[i][j];
#pragma unroll
            for (int k = 0; k < j; ++k) t -= (L[i][k] * L[j][k]) * d[k];
            L[i][j] = t / s;
        }
    }
    if (!ok) return 0;                                       // uniform: every lane holds the same numbers
#pragma unroll
    for (int i = 0; i < 6; ++i)
#pragma unroll
        for (int j = 0; j < i; ++j) {
            double t = L[i][j];
#pragma unroll
            for (int k = j + 1; k < i; ++k) t += L[i][k] * M[k][j];
            M[i][j] = -t;
        }
    double tinv = 0.0;
#pragma unroll
    for (int j = 0; j < 6; ++j) {
        double s = 1.0 / d[j];
#pragma unroll
        for (int i = j + 1; i < 6; ++i) s += (M[i][j] * M[i][j]) / d[i];
        tinv += s;
    }
    if (!(tinv > 0.0) || !(1.0 / tinv > eig_rel * tr)) return 0;
    double y[6];
#pragma unroll
    for (int i = 0; i < 6; ++i) {
        double t = -b[i];
#pragma unroll
        for (int j = 0; j < i; ++j) t += M[i][j] * -b[j];
        y[i] = t / d[i];
    }
#pragma unroll
    for (int j = 0; j < 6; ++j) {
        double t = y[j];
#pragma unroll
        for (int i = j + 1; i < 6; ++i) t += M[i][j] * y[i];
        x[j] = t;
    }
    return 1;
}

// Same algorithm and the same arithmetic order as oracle/tl3d_oracle.c: solve6 (cyclic Jacobi, 12 sweeps, relative
// eigenvalue cutoff), spread over the lanes of one wave: lane k (< 6) keeps row k of A and row k of V in registers; a
// sweep's rotations run three at a time on disjoint index pairs (see the loop), partners swap rows through shuffles.
// All 64 lanes execute every shuffle (EXEC full); lanes >= 6 carry zeros.
// Returns 0 on success; x[k] is valid on every lane (k < 6).
__device__ __forceinline__ int solve6_wave(const double *__restrict__ a21, const double *__restrict__ b, double damping,
                                           double eig_rel, double x[6]) {
    const int lane = threadIdx.x & 63;
    double a[6], v[6];
    double tr = 0.0;
    {
        int m = 0;
#pragma unroll
        for (int i = 0; i < 6; ++i)
#pragma unroll
            for (int j = i; j < 6; ++j) {
                const double e = a21[m++];
                if (lane == i) a[j] = e;
                if (lane == j) a[i] = e;
            }
    }
    tr = ((((a21[0] + a21[6]) + a21[11]) + a21[15]) + a21[18]) + a21[20];      // A00+A11+...+A55 in index order
    if (!(tr > 0.0)) return 1;
    const double lam = damping * (tr / 6.0);
    if (solve6_direct(a21, b, lam, eig_rel, x)) return 0;                     // well conditioned: nothing would be truncated
#pragma unroll
    for (int j = 0; j < 6; ++j) {
        if (lane >= 6) a[j] = 0.0;
        if (lane == j) a[j] += lam;
        v[j] = (lane == j) ? 1.0 : 0.0;
    }
    // Round-robin order: a sweep is 5 rounds of 3 rotations on disjoint pairs (the oracle's RR table).  Lane i < 6 computes
    // the angle of the pair it belongs to, so a round costs one chain of fp64 div/sqrt instead of three; the (c, s) of the
    // three pairs are then broadcast, every lane rotates its row's columns, and partners exchange rows.
    for (int sweep = 0; sweep < 12; ++sweep) {
        double offmax = 0.0;
#pragma unroll
        for (int k = 0; k < 6; ++k)
            if (k != lane && fabs(a[k]) > offmax) offmax = fabs(a[k]);          // lanes >= 6 hold zeros
#pragma unroll
        for (int d = 1; d < 8; d <<= 1) offmax = fmax(offmax, __shfl_xor(offmax, d));
        offmax = __shfl(offmax, 0);
        if (!(offmax > 1e-15 * tr)) break;                          // wave-uniform; same rule as the oracle
#pragma unroll
        for (int r = 0; r < 5; ++r) {
            // pairs of round r as compile-time constants
            constexpr int RP[5][3] = {{0, 1, 2}, {0, 3, 1}, {0, 2, 1}, {0, 1, 4}, {0, 2, 3}};
            constexpr int RQ[5][3] = {{5, 4, 3}, {4, 5, 2}, {3, 4, 5}, {2, 3, 5}, {1, 5, 4}};
            int partner = lane;
#pragma unroll
            for (int u = 0; u < 3; ++u) {
                if (lane == RP[r][u]) partner = RQ[r][u];
                if (lane == RQ[r][u]) partner = RP[r][u];
            }
            const bool isp = lane < partner;
            double my_diag = 0.0, my_off = 0.0;
#pragma unroll
            for (int k = 0; k < 6; ++k) {
                if (k == lane) my_diag = a[k];
                if (k == partner && partner != lane) my_off = a[k];
            }
            const double partner_diag = __shfl(my_diag, partner);
            const double off_p = __shfl(my_off, partner);               // the lower lane's A[p][q] is the pivot for both
            const double app = isp ? my_diag : partner_diag, aqq = isp ? partner_diag : my_diag;
            const double apq = isp ? my_off : off_p;
            // Rotation (c, s) of the pair.  A Jacobi sweep only needs c^2 + s^2 = 1 to rounding and an angle close to the
            // annihilating one (its error is squared away by the next sweep), so the reciprocals and square roots are the
            // hardware approximations + two Newton steps (~1e-16 relative) instead of IEEE sequences: the dependent chain of
            // a round shrinks from ~150 to ~30 fp64 instructions (the solve was 18 of the 34 us of an iteration).  The
            // eigenpairs the iteration converges to are the same to rounding; the oracle keeps exact divisions.
            double c = 1.0, sn = 0.0;
            if (lane < 6 && !(fabs(apq) < 1e-300)) {
                const double theta = (aqq - app) * fast_rcp(2.0 * apq);
                const double h2 = fma(theta, theta, 1.0);
                const double t = (theta >= 0.0 ? 1.0 : -1.0) * fast_rcp(fabs(theta) + h2 * fast_rsq(h2));
                c = fast_rsq(fma(t, t, 1.0));
                sn = t * c;
            }
#pragma unroll
            for (int u = 0; u < 3; ++u) {                               // columns of every row
                const double cu = __shfl(c, RP[r][u]), su = __shfl(sn, RP[r][u]);
                const double akp = a[RP[r][u]], akq = a[RQ[r][u]];
                a[RP[r][u]] = cu * akp - su * akq;
                a[RQ[r][u]] = su * akp + cu * akq;
                const double vkp = v[RP[r][u]], vkq = v[RQ[r][u]];
                v[RP[r][u]] = cu * vkp - su * vkq;
                v[RQ[r][u]] = su * vkp + cu * vkq;
            }
#pragma unroll
            for (int k = 0; k < 6; ++k) {                               // rows: partners exchange
                const double other = __shfl(a[k], partner);
                const double np_ = c * a[k] - sn * other;               // this lane is p: c*row_p - s*row_q
                const double nq_ = sn * other + c * a[k];               // this lane is q: s*row_p + c*row_q
                if (partner != lane) a[k] = isp ? np_ : nq_;
            }
        }
    }
    double lam_e[6], lmax = 0.0;
#pragma unroll
    for (int e = 0; e < 6; ++e) {
        lam_e[e] = __shfl(a[e], e);
        if (lam_e[e] > lmax) lmax = lam_e[e];
    }
    if (!(lmax > 0.0)) return 1;
    double xk = 0.0;
    int used = 0;
    const double bk = (lane < 6) ? b[lane] : 0.0;
#pragma unroll
    for (int e = 0; e < 6; ++e) {
        const double l = lam_e[e];
        if (!(l > eig_rel * lmax) || !(l > 0.0)) continue;            // wave-uniform
        // proj = sum_k V[k][e] * b[k], k = 0..5 in order (as the oracle)
        double proj = 0.0;
#pragma unroll
        for (int k = 0; k < 6; ++k) proj += __shfl(v[e] * bk, k);
        const double coef = -proj / l;
        xk += coef * v[e];
        ++used;
    }
#pragma unroll
    for (int k = 0; k < 6; ++k) x[k] = __shfl(xk, k);
    return used == 0;
}

// The solve for n <= 7 unknowns (Sim(3): pose + log-scale), on ONE lane: oracle/tl3d_oracle.c solve_n, same sequence (direct
// LDL^T path when no eigen-direction can be truncated, else row-cyclic Jacobi with the relative eigenvalue cutoff).
static __device__ int solve_n_serial(int n, const double *ap, const double *b, double damping, double eig_rel, double *x) {
    double A[7][7], V[7][7], L[7][7], M[7][7], d[7];
    int m = 0;
    double tr = 0.0;
    for (int i = 0; i < n; ++i)
        for (int j = i; j < n; ++j) { A[i][j] = A[j][i] = ap[m++]; }
    for (int i = 0; i < n; ++i) tr += A[i][i];
    if (!(tr > 0.0)) return 1;
    const double lam = damping * (tr / (double)n);
    for (int i = 0; i < n; ++i) A[i][i] += lam;
    tr = 0.0;
    for (int i = 0; i < n; ++i) tr += A[i][i];
    {
        int ok = 1;
        for (int j = 0; j < n && ok; ++j) {
            double s = A[j][j];
            for (int k = 0; k < j; ++k) s -= (L[j][k] * L[j][k]) * d[k];
            if (!(s > 0.0)) { ok = 0; break; }
            d[j] = s;
            for (int i = j + 1; i < n; ++i) {
                double t = A[i][j];
                for (int k = 0; k < j; ++k) t -= (L[i][k] * L[j][k]) * d[k];
                L[i][j] = t / s;
            }
        }
        if (ok) {
            for (int i = 0; i < n; ++i)
                for (int j = 0; j < i; ++j) {
                    double t = L[i][j];
                    for (int k = j + 1; k < i; ++k) t += L[i][k] * M[k][j];
                    M[i][j] = -t;
                }
            double tinv = 0.0;
            for (int j = 0; j < n; ++j) {
                double s = 1.0 / d[j];
                for (int i = j + 1; i < n; ++i) s += (M[i][j] * M[i][j]) / d[i];
                tinv += s;
            }
            if (tinv > 0.0 && 1.0 / tinv > eig_rel * tr) {
                double y[7];
                for (int i = 0; i < n; ++i) {
                    double t = -b[i];
                    for (int j = 0; j < i; ++j) t += M[i][j] * -b[j];
                    y[i] = t / d[i];
                }
                for (int j = 0; j < n; ++j) {
                    double t = y[j];
                    for (int i = j + 1; i < n; ++i) t += M[i][j] * y[i];
                    x[j] = t;
                }
                return 0;
            }
        }
    }
    for (int i = 0; i < n; ++i)
        for (int j = 0; j < n; ++j) V[i][j] = (i == j) ? 1.0 : 0.0;
    for (int sweep = 0; sweep < 16; ++sweep) {
        double offmax = 0.0;
        for (int i = 0; i < n; ++i)
            for (int k = 0; k < n; ++k)
                if (k != i && fabs(A[i][k]) > offmax) offmax = fabs(A[i][k]);
        if (!(offmax > 1e-15 * tr)) break;
        for (int pp = 0; pp < n - 1; ++pp)
            for (int q = pp + 1; q < n; ++q) {
                const double apq = A[pp][q];
                if (fabs(apq) < 1e-300) continue;
                const double theta = (A[q][q] - A[pp][pp]) / (2.0 * apq);
                const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
                const double cs = 1.0 / sqrt(t * t + 1.0), sn = t * cs;
                for (int k = 0; k < n; ++k) {
                    const double akp = A[k][pp], akq = A[k][q];
                    A[k][pp] = cs * akp - sn * akq;
                    A[k][q] = sn * akp + cs * akq;
                    const double vkp = V[k][pp], vkq = V[k][q];
                    V[k][pp] = cs * vkp - sn * vkq;
                    V[k][q] = sn * vkp + cs * vkq;
                }
                for (int k = 0; k < n; ++k) {
                    const double apk = A[pp][k], aqk = A[q][k];
                    A[pp][k] = cs * apk - sn * aqk;
                    A[q][k] = sn * apk + cs * aqk;
                }
            }
    }
    double lmax = 0.0;
    for (int i = 0; i < n; ++i) if (A[i][i] > lmax) lmax = A[i][i];
    if (!(lmax > 0.0)) return 1;
    for (int i = 0; i < n; ++i) x[i] = 0.0;
    int used = 0;
    for (int e = 0; e < n; ++e) {
        const double l = A[e][e];
        if (!(l > eig_rel * lmax) || !(l > 0.0)) continue;
        double proj = 0.0;
        for (int k = 0; k < n; ++k) proj += V[k][e] * b[k];
        const double coef = -proj / l;
        for (int k = 0; k < n; ++k) x[k] += coef * V[k][e];
        ++used;
    }
    return used == 0;
}

// the 7x7 system from the sums (layout of IcpState::sums): rows 0..5 = the pose block with the scale column appended
static __device__ int solve7_serial(const double *sums, double damping, double eig_rel, double x[7]) {
    double ap[28], b[7];
    int m = 0, k = 0;
    for (int i = 0; i < 6; ++i) {
        for (int j = i; j < 6; ++j) ap[k++] = sums[m++];
        ap[k++] = sums[32 + i];
    }
    ap[k++] = sums[38];
    for (int i = 0; i < 6; ++i) b[i] = sums[21 + i];
    b[6] = sums[39];
    return solve_n_serial(7, ap, b, damping, eig_rel, x);
}

// State words another workgroup of the same launch reads next (batched runs): write-through (agent-scope) stores, so that
// they need no L2 write-back before the hand-off; the reader acquires as before.
template <typename V> __device__ __forceinline__ void st_agent(V *p, V v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
template <typename V> __device__ __forceinline__ V ld_agent(const V *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

static __device__ void se3_apply(const double x[6], double *T, float *T_f32 = nullptr) {
    const double wx = x[0], wy = x[1], wz = x[2];
    const double th2 = wx * wx + wy * wy + wz * wz;
    const double th = sqrt(th2);
    double a, bq;
    if (th < 1e-12) { a = 1.0; bq = 0.5; } else { a = sin(th) / th; bq = (1.0 - cos(th)) / th2; }
    const double K[9] = {0, -wz, wy, wz, 0, -wx, -wy, wx, 0};
    double K2[9], dR[9], Tn[16];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
            double s = 0;
            for (int k = 0; k < 3; ++k) s += K[3 * i + k] * K[3 * k + j];
            K2[3 * i + j] = s;
        }
    for (int i = 0; i < 9; ++i) dR[i] = (i % 4 == 0 ? 1.0 : 0.0) + a * K[i] + bq * K2[i];
    for (int i = 0; i < 3; ++i) {
        for (int j = 0; j < 4; ++j) {
            double s = 0;
            for (int k = 0; k < 3; ++k) s += dR[3 * i + k] * T[4 * k + j];
            Tn[4 * i + j] = s;
        }
        Tn[4 * i + 3] += x[3 + i];
    }
    Tn[12] = 0; Tn[13] = 0; Tn[14] = 0; Tn[15] = 1;
    for (int i = 0; i < 16; ++i) st_agent(T + i, Tn[i]);
    if (T_f32)
        for (int i = 0; i < 12; ++i) T_f32[i] = (float)Tn[i];
}

}  // namespace tl3d
