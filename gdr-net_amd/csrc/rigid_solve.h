// The closed form of rigid.hip: the proper rotation R and the translation t that minimise sum |R m + t - c|^2, from the centroids and the 3x3
// cross-covariance of the pairs (Horn 1987, "Closed-form solution of absolute orientation using unit quaternions").  fp64, host and device, every
// index a compile-time constant behind the unrolled loops (nothing here goes to scratch).
//
// With S = sum (m - mbar)(c - cbar)^T the optimal unit quaternion is the eigenvector of the largest eigenvalue of the symmetric 4x4 matrix N(S)
// below.  Its eigenvalues are, with s1 >= s2 >= s3 >= 0 the singular values of S and s = sign(det S),
//     s1 + s2 + s s3,  s1 - s2 - s s3,  -s1 + s2 - s s3,  -s1 - s2 + s s3,
// so the two largest add up to 2 s1 and lie 2 (s2 + s s3) apart: the optimum is unique iff that gap is positive, whatever the sign of det S (a
// reflected optimum needs no special case: a quaternion always gives det +1) and whatever the rank (a coplanar set has s3 = 0 and a gap of
// 2 s2).  The set is DEGENERATE -- collinear, a repeated point, or a reflected set whose two small singular values cancel -- iff
//     gap <= 2e-9 * s1      i.e.  s2 + s s3 <= 1e-9 s1,
// a design constant that leaves seven digits above the fp64 rounding of the sums.  The eigen-decomposition is cyclic Jacobi with a FIXED number of
// sweeps (RIGID_SWEEPS x 6 rotations, a rotation skipped only where its off-diagonal entry is exactly 0): the same operations for every input.
#pragma once

#define RIGID_HD __host__ __device__ __forceinline__

namespace {

constexpr int RIGID_SWEEPS = 6;           // quadratic convergence: a 4x4 is at fp64 rounding after 5 cyclic sweeps (2e-6 after 4); one more for margin
constexpr double RIGID_GAP = 2e-9;        // the degeneracy rule above

RIGID_HD bool rigid_finite(double v) { return v - v == 0.0; }

// one Jacobi rotation in the (P, Q) plane of the symmetric A (full storage), accumulated into the columns of V
template <int P, int Q>
RIGID_HD void rigid_jacobi_rotate(double (&A)[4][4], double (&V)[4][4]) {
    const double apq = A[P][Q];
    if (apq == 0.0) return;
    const double theta = (A[Q][Q] - A[P][P]) / (2.0 * apq);
    const double tt = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));   // (theta = +-inf: 0)
    const double c = 1.0 / sqrt(tt * tt + 1.0), s = tt * c;
#pragma unroll
    for (int k = 0; k < 4; ++k) {   // A <- A J
        const double akp = A[k][P], akq = A[k][Q];
        A[k][P] = c * akp - s * akq;
        A[k][Q] = s * akp + c * akq;
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {   // A <- J^T A
        const double apk = A[P][k], aqk = A[Q][k];
        A[P][k] = c * apk - s * aqk;
        A[Q][k] = s * apk + c * aqk;
    }
    A[P][Q] = A[Q][P] = 0.0;        // (what the rotation was chosen for, exactly)
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const double vkp = V[k][P], vkq = V[k][Q];
        V[k][P] = c * vkp - s * vkq;
        V[k][Q] = s * vkp + c * vkq;
    }
}

// R (row-major), t from the centroids mbar, cbar and S[a * 3 + b] = sum (m - mbar)_a (c - cbar)_b.  false: degenerate or non-finite (R, t untouched).
RIGID_HD bool rigid_solve(const double* S, const double* mbar, const double* cbar, double* R, double* t) {
    double A[4][4], V[4][4];
    A[0][0] = S[0] + S[4] + S[8];
    A[1][1] = S[0] - S[4] - S[8];
    A[2][2] = -S[0] + S[4] - S[8];
    A[3][3] = -S[0] - S[4] + S[8];
    A[0][1] = A[1][0] = S[5] - S[7];
    A[0][2] = A[2][0] = S[6] - S[2];
    A[0][3] = A[3][0] = S[1] - S[3];
    A[1][2] = A[2][1] = S[1] + S[3];
    A[1][3] = A[3][1] = S[6] + S[2];
    A[2][3] = A[3][2] = S[5] + S[7];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) V[i][j] = i == j ? 1.0 : 0.0;
    for (int sweep = 0; sweep < RIGID_SWEEPS; ++sweep) {
        rigid_jacobi_rotate<0, 1>(A, V);
        rigid_jacobi_rotate<0, 2>(A, V);
        rigid_jacobi_rotate<0, 3>(A, V);
        rigid_jacobi_rotate<1, 2>(A, V);
        rigid_jacobi_rotate<1, 3>(A, V);
        rigid_jacobi_rotate<2, 3>(A, V);
    }
    // the largest eigenvalue (ties: the lowest index), its eigenvector and the runner-up
    double best = A[0][0], second = -INFINITY;
    double q[4] = {V[0][0], V[1][0], V[2][0], V[3][0]};
#pragma unroll
    for (int k = 1; k < 4; ++k) {
        const double l = A[k][k];
        if (l > best) {
            second = best;
            best = l;
#pragma unroll
            for (int i = 0; i < 4; ++i) q[i] = V[i][k];
        } else if (l > second) {
            second = l;
        }
    }
    const double s1 = 0.5 * (best + second), gap = best - second;
    if (!(gap > RIGID_GAP * s1)) return false;   // (NaN anywhere: degenerate)
    const double qn = 1.0 / sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
    const double w = q[0] * qn, x = q[1] * qn, y = q[2] * qn, z = q[3] * qn;
    double Rn[9];
    Rn[0] = 1.0 - 2.0 * (y * y + z * z);
    Rn[1] = 2.0 * (x * y - w * z);
    Rn[2] = 2.0 * (x * z + w * y);
    Rn[3] = 2.0 * (x * y + w * z);
    Rn[4] = 1.0 - 2.0 * (x * x + z * z);
    Rn[5] = 2.0 * (y * z - w * x);
    Rn[6] = 2.0 * (x * z - w * y);
    Rn[7] = 2.0 * (y * z + w * x);
    Rn[8] = 1.0 - 2.0 * (x * x + y * y);
    double tn[3], chk = 0.0;
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        tn[r] = cbar[r] - (Rn[r * 3] * mbar[0] + Rn[r * 3 + 1] * mbar[1] + Rn[r * 3 + 2] * mbar[2]);
        chk += tn[r] + Rn[r * 3] + Rn[r * 3 + 1] + Rn[r * 3 + 2];
    }
    if (!rigid_finite(chk)) return false;
#pragma unroll
    for (int k = 0; k < 9; ++k) R[k] = Rn[k];
#pragma unroll
    for (int k = 0; k < 3; ++k) t[k] = tn[k];
    return true;
}

// the closed form on three pairs (the minimal sample): m, c = [3][3]
RIGID_HD bool rigid_from_three(const double* m, const double* c, double* R, double* t) {
    double mbar[3], cbar[3], S[9];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        mbar[k] = (m[k] + m[3 + k] + m[6 + k]) / 3.0;
        cbar[k] = (c[k] + c[3 + k] + c[6 + k]) / 3.0;
    }
#pragma unroll
    for (int k = 0; k < 9; ++k) S[k] = 0.0;
#pragma unroll
    for (int p = 0; p < 3; ++p)
#pragma unroll
        for (int a = 0; a < 3; ++a)
#pragma unroll
            for (int b = 0; b < 3; ++b) S[a * 3 + b] += (m[p * 3 + a] - mbar[a]) * (c[p * 3 + b] - cbar[b]);
    return rigid_solve(S, mbar, cbar, R, t);
}

}  // namespace
