// sym3_eigen.h -- eigen-decomposition of one symmetric 3x3 matrix in fp64 by cyclic Jacobi rotations, for one thread
// (kernels_normals.hip: the covariance of a point's neighbourhood).  Host and device: the same IEEE operations in the same order
// (the library is built with -ffp-contract=off), so a CPU program checks what the kernel runs.
//
// Why Jacobi: the closed-form (trigonometric) eigenvalues lose half the digits when two eigenvalues are close, and the eigenvector
// taken from them by cross products loses the rest; a Jacobi rotation is an orthogonal similarity, so every sweep is backward
// stable (the result is the exact decomposition of A + E with |E| a few ulp of |A|) whatever the spectrum looks like.  A pair whose
// off-diagonal entry is exactly 0 is left alone, so a matrix with an exactly zero row (points in an axis-aligned plane or on an
// axis-aligned line) keeps that axis as an exact eigenvector with an exactly zero eigenvalue.
#pragma once
#include <math.h>

#if defined(__HIPCC__)
#define SYM3_HD __host__ __device__ __forceinline__
#else
#define SYM3_HD inline
#endif

namespace tl3d {

constexpr int SYM3_SWEEPS = 8;          // 3x3: quadratic convergence; 4 sweeps reached fp64 on 20 000 covariances with gaps down to 7.6e-9 of
                                        // the largest eigenvalue (3 did not); twice that, and a converged sweep is three skipped rotations

// one rotation in the (p, q) plane that zeroes apq; arp / arq: the third row's entries; v*: the eigenvector matrix's columns p and q
SYM3_HD void sym3_rotate(double &app, double &aqq, double &apq, double &arp, double &arq, double &v0p, double &v0q, double &v1p, double &v1q,
                         double &v2p, double &v2q) {
    if (apq == 0.0) return;
    const double theta = (aqq - app) / (2.0 * apq);
    // the smaller root of t^2 + 2 theta t - 1 = 0: |t| <= 1, a rotation by at most 45 degrees.  theta^2 overflows to +inf for a
    // vanishing apq: t = 0 then, and dropping apq is an error far below an ulp of the diagonal.
    const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
    const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
    const double h = t * apq;
    app -= h;
    aqq += h;
    apq = 0.0;
    const double rp = arp, rq = arq;
    arp = c * rp - s * rq;
    arq = s * rp + c * rq;
    double a = v0p, b = v0q;
    v0p = c * a - s * b; v0q = s * a + c * b;
    a = v1p; b = v1q;
    v1p = c * a - s * b; v1q = s * a + c * b;
    a = v2p; b = v2q;
    v2p = c * a - s * b; v2q = s * a + c * b;
}

SYM3_HD double sym3_pick(bool s1, bool s2, double a, double b, double c) { return s2 ? c : (s1 ? b : a); }

// a: xx, yy, zz, xy, xz, yz of the matrix.  Out: lam[3] ascending, and n[3] = the unit eigenvector of lam[0] (of the eigenvalues
// that compare equal, the one of the lowest axis wins: a fixed choice, the same in every run).
SYM3_HD void sym3_smallest(const double a[6], double lam[3], double n[3]) {
    double a00 = a[0], a11 = a[1], a22 = a[2], a01 = a[3], a02 = a[4], a12 = a[5];
    double v00 = 1.0, v01 = 0.0, v02 = 0.0, v10 = 0.0, v11 = 1.0, v12 = 0.0, v20 = 0.0, v21 = 0.0, v22 = 1.0;
    for (int sweep = 0; sweep < SYM3_SWEEPS; ++sweep) {
        sym3_rotate(a00, a11, a01, a02, a12, v00, v01, v10, v11, v20, v21);
        sym3_rotate(a00, a22, a02, a01, a12, v00, v02, v10, v12, v20, v22);
        sym3_rotate(a11, a22, a12, a01, a02, v01, v02, v11, v12, v21, v22);
    }
    // (selects over values: picking a column through `if` made the compiler index the nine entries in scratch memory)
    const bool s1 = a11 < a00, s2 = a22 < (s1 ? a11 : a00);
    const double l0 = sym3_pick(s1, s2, a00, a11, a22);
    const double x = sym3_pick(s1, s2, v00, v01, v02), y = sym3_pick(s1, s2, v10, v11, v12), z = sym3_pick(s1, s2, v20, v21, v22);
    const double l2 = fmax(a00, fmax(a11, a22));
    // the middle one without a subtraction: the median of three
    const double l1 = fmax(fmin(a00, a11), fmin(fmax(a00, a11), a22));
    lam[0] = l0; lam[1] = l1; lam[2] = l2;
    const double inv = 1.0 / sqrt(x * x + y * y + z * z);          // the columns are unit to a few ulp; this takes those off
    n[0] = x * inv; n[1] = y * inv; n[2] = z * inv;
}

}  // namespace tl3d
