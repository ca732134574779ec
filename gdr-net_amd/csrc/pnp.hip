// Batched PnP-RANSAC and iterative PnP on the device for gfx950: the step the reference's evaluator runs per RoI on the host with OpenCV between
// the 2D-3D correspondences and the pose metrics (cfg.TEST.USE_PNP) --
//   GDRN_Evaluator.process_pnp_ransac                  core/gdrn_modeling/gdrn_evaluator.py:316-392 -> lib/pysixd/misc.py:145-194
//   process_net_and_pnp, pnp_type "ransac" / "iter"    gdrn_evaluator.py:187-307
// -- for a whole batch: one workgroup per RoI, no host loop.  Every pose computation is fp64 (cv2 converts to double); the correspondences are read as
// they are stored (fp32 from gdrn_correspondences, or fp64) and widened exactly.
//   pnp_ransac_kernel   `iters` hypotheses per RoI: 4 distinct samples from a counter-based hash, P3P (Grunert's quartic, solved by Ferrari's method
//                       and polished by Newton steps) on three of them, the root with the smallest reprojection error on the fourth; all
//                       hypotheses scored against all points staged through LDS, integer inlier counts; highest count wins, ties to the lowest index.
//   pnp_refine_kernel   Levenberg-Marquardt on the 6-vector (left rotation increment, translation) over the winner's inliers, inliers re-selected,
//                       refined once more (mode 0), or over all valid points from the caller's pose (mode 1).  Sums are reduced in a fixed order
//                       (wave xor tree, then the four waves through LDS): no floating-point atomics, the same call gives the same bits.
// This is not cv2's algorithm (EPnP, its own RNG and a 0.99-confidence early stop): results are pinned to geometry, not to cv2 output.
// (The file has no 16-bit code: both library builds compile the same thing.)
#include "common.h"
#include "geom64.h"
#include "ransac_draw.h"
#include "../../include/gdrn_hip.h"

namespace {

constexpr int PNP_THREADS = 256;
constexpr int PNP_HYP = 256;          // hypotheses per pass over the points (their 3x4 projection matrices: 24 KB of LDS)
constexpr int PNP_WIN = 16;           // doubles per RoI in the workspace: R (9), t (3), the winner's count, padding
constexpr double PNP_STEP_TOL = 1e-10;

template <typename T> struct PnpTile;                                   // points per LDS tile: 20 KB either way
template <> struct PnpTile<float> { static constexpr int N = 1024; };
template <> struct PnpTile<double> { static constexpr int N = 512; };

PNP_HD void pnp_cross(const double* a, const double* b, double* c) {
    c[0] = a[1] * b[2] - a[2] * b[1];
    c[1] = a[2] * b[0] - a[0] * b[2];
    c[2] = a[0] * b[1] - a[1] * b[0];
}
PNP_HD double pnp_dot(const double* a, const double* b) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }
PNP_HD bool pnp_finite(double v) { return v - v == 0.0; }

PNP_HD bool pnp_inv3(const double* K, double* Ki) {
    double c0[3], c1[3], c2[3];
    pnp_cross(K + 3, K + 6, c0);
    pnp_cross(K + 6, K, c1);
    pnp_cross(K, K + 3, c2);
    const double det = pnp_dot(K, c0);
    const double s = 1.0 / det;
    for (int i = 0; i < 3; ++i) {
        Ki[i * 3 + 0] = c0[i] * s;
        Ki[i * 3 + 1] = c1[i] * s;
        Ki[i * 3 + 2] = c2[i] * s;
    }
    return pnp_finite(s) && det != 0.0;
}

// pixel position of the camera-frame point Xc under K (general 3x3); false behind the camera
PNP_HD bool pnp_project(const double* K, const double* Xc, double* u, double* v) {
    const double p0 = pnp_dot(K, Xc), p1 = pnp_dot(K + 3, Xc), p2 = pnp_dot(K + 6, Xc);
    *u = p0 / p2;
    *v = p1 / p2;
    return p2 > 0.0;
}

PNP_HD void pnp_xform(const double* R, const double* t, const double* X, double* Xc) {
    const V3 c = xform(R, t, load3(X));
    Xc[0] = c.x, Xc[1] = c.y, Xc[2] = c.z;
}

// squared reprojection error [px^2] of one correspondence, +inf behind the camera (NaN stays NaN: every comparison with it is false)
PNP_HD double pnp_err2(const double* K, const double* R, const double* t, const double* X, double u, double v) {
    double Xc[3], pu, pv;
    pnp_xform(R, t, X, Xc);
    const bool front = pnp_project(K, Xc, &pu, &pv);
    const double du = pu - u, dv = pv - v;
    const double e = du * du + dv * dv;
    return front ? e : (e == e ? INFINITY : e);
}

// the real root of x^3 + a2 x^2 + a1 x + a0 that is the largest
PNP_HD double pnp_cubic_largest(double a2, double a1, double a0) {
    const double Q = (3.0 * a1 - a2 * a2) / 9.0, Rr = (9.0 * a2 * a1 - 27.0 * a0 - 2.0 * a2 * a2 * a2) / 54.0;
    const double D = Q * Q * Q + Rr * Rr;
    double x;
    if (D >= 0.0) {
        const double sd = sqrt(D);
        x = cbrt(Rr + sd) + cbrt(Rr - sd) - a2 / 3.0;
    } else {
        const double th = acos(fmin(1.0, fmax(-1.0, Rr / sqrt(-Q * Q * Q))));
        x = 2.0 * sqrt(-Q) * cos(th / 3.0) - a2 / 3.0;
    }
    for (int it = 0; it < 2; ++it) {   // Newton polish
        const double f = ((x + a2) * x + a1) * x + a0, df = (3.0 * x + 2.0 * a2) * x + a1;
        const double xn = x - f / df;
        if (df != 0.0 && pnp_finite(xn)) x = xn;
    }
    return x;
}

// real roots of c[4] y^4 + ... + c[0] (Ferrari, each polished by Newton steps on the quartic); returns their number
PNP_HD int pnp_quartic(const double* c, double* roots) {
    const double a = c[3] / c[4], b = c[2] / c[4], cc = c[1] / c[4], d = c[0] / c[4];
    if (!(pnp_finite(a) && pnp_finite(b) && pnp_finite(cc) && pnp_finite(d))) return 0;
    const double a2 = a * a;
    const double p = b - 0.375 * a2, q = cc - 0.5 * a * b + 0.125 * a2 * a, r = d - 0.25 * a * cc + 0.0625 * a2 * b - (3.0 / 256.0) * a2 * a2;
    const double scale = fabs(p) + sqrt(fabs(r)) + cbrt(q * q);   // ~ z^2
    int n = 0;
    double m = pnp_cubic_largest(p, 0.25 * p * p - r, -0.125 * q * q);
    if (!(m > 1e-14 * scale)) {   // q ~ 0: biquadratic z^4 + p z^2 + r
        double disc = p * p - 4.0 * r;
        if (disc < 0.0 && disc > -1e-12 * (p * p + fabs(r))) disc = 0.0;
        if (disc >= 0.0) {
            const double sd = sqrt(disc);
            for (int s = 0; s < 2; ++s) {
                const double z2 = 0.5 * (-p + (s ? -sd : sd));
                if (z2 >= 0.0) {
                    roots[n++] = sqrt(z2);
                    roots[n++] = -sqrt(z2);
                }
            }
        }
    } else {
        const double s = sqrt(2.0 * m);
        for (int k = 0; k < 2; ++k) {   // z^2 -+ s z + p/2 + m +- q/(2s)
            const double B = k ? s : -s, C = 0.5 * p + m + (k ? -q : q) / (2.0 * s);
            double disc = B * B - 4.0 * C;
            if (disc < 0.0 && disc > -1e-12 * (B * B + fabs(C))) disc = 0.0;
            if (disc >= 0.0) {
                const double sd = sqrt(disc);
                const double qq = -0.5 * (B + (B >= 0.0 ? sd : -sd));   // the stable pair
                roots[n++] = qq;
                roots[n++] = qq != 0.0 ? C / qq : 0.0;
            }
        }
    }
    for (int i = 0; i < n; ++i) {
        double y = roots[i] - 0.25 * a;
        for (int it = 0; it < 3; ++it) {
            const double f = (((y + a) * y + b) * y + cc) * y + d, df = ((4.0 * y + 3.0 * a) * y + 2.0 * b) * y + cc;
            const double yn = y - f / df;
            if (df != 0.0 && pnp_finite(yn)) y = yn;
        }
        roots[i] = y;
    }
    return n;
}

// orthonormal frame of three points: e1 along p1 - p0, e3 normal to the triangle, e2 = e3 x e1 (rows of F)
PNP_HD void pnp_frame(const double* p0, const double* p1, const double* p2, double* F) {
    double d1[3], d2[3];
    for (int k = 0; k < 3; ++k) {
        d1[k] = p1[k] - p0[k];
        d2[k] = p2[k] - p0[k];
    }
    const double n1 = 1.0 / sqrt(pnp_dot(d1, d1));
    for (int k = 0; k < 3; ++k) F[k] = d1[k] * n1;
    pnp_cross(F, d2, F + 6);
    const double n3 = 1.0 / sqrt(pnp_dot(F + 6, F + 6));
    for (int k = 0; k < 3; ++k) F[6 + k] *= n3;
    pnp_cross(F + 6, F, F + 3);
}

// P3P: model points P[3][3], unit bearings f[3][3].  With s_i the depths along the bearings, x = s2/s1 and y = s3/s1 satisfy two conics (the law
// of cosines on the three sides); their difference is linear in x, x = Nq(y) / Dl(y), which turns the second conic into a quartic in y (Grunert).
// Each admissible root gives the camera-frame triangle, hence (R, t); the one with the smallest reprojection error on the fourth
// correspondence (X4, u4, v4) under K is kept.  Returns false when the sample is degenerate (collinear, no admissible root, non-finite).
PNP_HD bool pnp_p3p(const double* P, const double* f, const double* K, const double* X4, double u4, double v4, double* R, double* t) {
    double d[3];
    for (int k = 0; k < 3; ++k) d[k] = P[3 + k] - P[6 + k];
    const double a2 = pnp_dot(d, d);
    for (int k = 0; k < 3; ++k) d[k] = P[k] - P[6 + k];
    const double b2 = pnp_dot(d, d);
    for (int k = 0; k < 3; ++k) d[k] = P[k] - P[3 + k];
    const double c2 = pnp_dot(d, d);
    double e1[3], e2[3], nrm[3];
    for (int k = 0; k < 3; ++k) {
        e1[k] = P[3 + k] - P[k];
        e2[k] = P[6 + k] - P[k];
    }
    pnp_cross(e1, e2, nrm);
    if (!(pnp_dot(nrm, nrm) > 1e-20 * c2 * b2)) return false;   // collinear (or a repeated point, or NaN)
    const double ca = pnp_dot(f + 3, f + 6), cb = pnp_dot(f, f + 6), cg = pnp_dot(f, f + 3);
    // x (2 b2 (y ca - cg)) = (c2 - a2)(1 + y^2 - 2 y cb) - b2 (1 - y^2)
    const double Nq[3] = {(c2 - a2) - b2, -2.0 * (c2 - a2) * cb, (c2 - a2) + b2};
    const double Dl[2] = {-2.0 * b2 * cg, 2.0 * b2 * ca};
    // b2 (D^2 + N^2 - 2 cg N D) - c2 (1 - 2 cb y + y^2) D^2 = 0
    double DD[3] = {Dl[0] * Dl[0], 2.0 * Dl[0] * Dl[1], Dl[1] * Dl[1]};
    double c[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
    for (int i = 0; i < 3; ++i) {
        c[i] += b2 * DD[i];
        for (int j = 0; j < 3; ++j) c[i + j] += b2 * Nq[i] * Nq[j];
        for (int j = 0; j < 2; ++j) c[i + j] -= 2.0 * b2 * cg * Nq[i] * Dl[j];
    }
    const double W[3] = {1.0, -2.0 * cb, 1.0};
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) c[i + j] -= c2 * W[i] * DD[j];
    double roots[4];
    const int nr = pnp_quartic(c, roots);
    double Fm[9];
    pnp_frame(P, P + 3, P + 6, Fm);
    double best = INFINITY;
    for (int i = 0; i < nr; ++i) {
        const double y = roots[i];
        const double x = ((Nq[2] * y + Nq[1]) * y + Nq[0]) / (Dl[1] * y + Dl[0]);
        const double den = 1.0 + y * y - 2.0 * y * cb;
        if (!(y > 0.0 && x > 0.0 && den > 0.0)) continue;
        const double s1 = sqrt(b2 / den), s2 = x * s1, s3 = y * s1;
        double C[9], Fc[9], Rc[9], tc[3];
        for (int k = 0; k < 3; ++k) {
            C[k] = s1 * f[k];
            C[3 + k] = s2 * f[3 + k];
            C[6 + k] = s3 * f[6 + k];
        }
        pnp_frame(C, C + 3, C + 6, Fc);
        for (int r = 0; r < 3; ++r)   // R = Fc^T Fm
            for (int q = 0; q < 3; ++q) Rc[r * 3 + q] = Fc[r] * Fm[q] + Fc[3 + r] * Fm[3 + q] + Fc[6 + r] * Fm[6 + q];
        for (int k = 0; k < 3; ++k) tc[k] = C[k] - pnp_dot(Rc + 3 * k, P);
        const double e = pnp_err2(K, Rc, tc, X4, u4, v4);
        if (e < best) {
            best = e;
            for (int k = 0; k < 9; ++k) R[k] = Rc[k];
            for (int k = 0; k < 3; ++k) t[k] = tc[k];
        }
    }
    double chk = 0.0;
    for (int k = 0; k < 9; ++k) chk += R[k];
    return best < INFINITY && pnp_finite(chk + t[0] + t[1] + t[2]);
}

// hypothesis h of RoI n (count >= 4 correspondences at img / mod): false = degenerate
template <typename T>
PNP_HD bool pnp_hypothesis(const T* img, const T* mod, int count, const double* K, const double* Ki, unsigned long long seed, int n, int h,
                           double* R, double* t) {
    int idx[4];
    if (!pnp_sample<4>(seed, n, h, count, idx)) return false;
    double P[9], f[9], X4[3];
    for (int s = 0; s < 3; ++s) {
        const double u = (double)img[(size_t)idx[s] * 2], v = (double)img[(size_t)idx[s] * 2 + 1];
        const double uv1[3] = {u, v, 1.0};
        double b[3];
        for (int k = 0; k < 3; ++k) {
            P[s * 3 + k] = (double)mod[(size_t)idx[s] * 3 + k];
            b[k] = pnp_dot(Ki + 3 * k, uv1);
        }
        const double nb = 1.0 / sqrt(pnp_dot(b, b));
        for (int k = 0; k < 3; ++k) f[s * 3 + k] = b[k] * nb;
    }
    for (int k = 0; k < 3; ++k) X4[k] = (double)mod[(size_t)idx[3] * 3 + k];
    for (int k = 0; k < 9; ++k) R[k] = 0.0;
    t[0] = t[1] = t[2] = 0.0;
    return pnp_p3p(P, f, K, X4, (double)img[(size_t)idx[3] * 2], (double)img[(size_t)idx[3] * 2 + 1], R, t);
}

// R <- exp([w]x) R (Rodrigues; series below 1e-4 rad: finite at 0, and nothing here is singular near pi)
PNP_HD void pnp_rotate_left(const double* w, const double* R, double* out) {
    const double th2 = pnp_dot(w, w), th = sqrt(th2);
    double A, B;
    if (th < 1e-4) {
        A = 1.0 - th2 / 6.0 * (1.0 - th2 / 20.0);
        B = 0.5 - th2 / 24.0 * (1.0 - th2 / 30.0);
    } else {
        const double sh = sin(0.5 * th);
        A = sin(th) / th;
        B = 2.0 * sh * sh / th2;
    }
    double E[9];
    E[0] = 1.0 - B * (w[1] * w[1] + w[2] * w[2]);
    E[1] = -A * w[2] + B * w[0] * w[1];
    E[2] = A * w[1] + B * w[0] * w[2];
    E[3] = A * w[2] + B * w[0] * w[1];
    E[4] = 1.0 - B * (w[0] * w[0] + w[2] * w[2]);
    E[5] = -A * w[0] + B * w[1] * w[2];
    E[6] = -A * w[1] + B * w[0] * w[2];
    E[7] = A * w[0] + B * w[1] * w[2];
    E[8] = 1.0 - B * (w[0] * w[0] + w[1] * w[1]);
    for (int r = 0; r < 3; ++r)
        for (int q = 0; q < 3; ++q) out[r * 3 + q] = E[r * 3] * R[q] + E[r * 3 + 1] * R[3 + q] + E[r * 3 + 2] * R[6 + q];
}

// index of (i, j), i <= j, in the packed upper triangle of a 6x6
PNP_HD int pnp_tri(int i, int j) { return i * 6 - i * (i - 1) / 2 + (j - i); }

// (A + lambda diag(A)) x = -g by Cholesky; A packed upper (21).  false: not positive definite / non-finite
PNP_HD bool pnp_solve6(const double* A, const double* g, double lambda, double* x) {
    double L[36];
    for (int i = 0; i < 6; ++i)
        for (int j = 0; j <= i; ++j) {
            double s = A[pnp_tri(j, i)];
            if (i == j) s += lambda * s;
            for (int k = 0; k < j; ++k) s -= L[i * 6 + k] * L[j * 6 + k];
            if (i == j) {
                if (!(s > 0.0) || !pnp_finite(s)) return false;
                L[i * 6 + i] = sqrt(s);
            } else {
                L[i * 6 + j] = s / L[j * 6 + j];
            }
        }
    double y[6];
    for (int i = 0; i < 6; ++i) {
        double s = -g[i];
        for (int k = 0; k < i; ++k) s -= L[i * 6 + k] * y[k];
        y[i] = s / L[i * 6 + i];
    }
    for (int i = 5; i >= 0; --i) {
        double s = y[i];
        for (int k = i + 1; k < 6; ++k) s -= L[k * 6 + i] * x[k];
        x[i] = s / L[i * 6 + i];
    }
    double chk = 0.0;
    for (int i = 0; i < 6; ++i) chk += x[i];
    return pnp_finite(chk);
}

// one correspondence's terms of the normal equations at (R, t): acc[0..20] += J^T J (packed upper), acc[21..26] += J^T r, acc[27] += |r|^2, with
// r = projection - observation [px] and J its derivative in (w, dt) of  Xc = exp([w]x) R X + t + dt  at 0.
PNP_HD void pnp_accumulate(const double* K, const double* R, const double* t, const double* X, double u, double v, double* acc) {
    double Xc[3];
    pnp_xform(R, t, X, Xc);
    const double Y[3] = {Xc[0] - t[0], Xc[1] - t[1], Xc[2] - t[2]};
    const double p0 = pnp_dot(K, Xc), p1 = pnp_dot(K + 3, Xc), p2 = pnp_dot(K + 6, Xc);
    const double iz = 1.0 / p2, pu = p0 * iz, pv = p1 * iz;
    double J[2][6];
    for (int k = 0; k < 3; ++k) {
        J[0][3 + k] = (K[k] - pu * K[6 + k]) * iz;
        J[1][3 + k] = (K[3 + k] - pv * K[6 + k]) * iz;
    }
    pnp_cross(Y, &J[0][3], &J[0][0]);   // g . (w x Y) = w . (Y x g)
    pnp_cross(Y, &J[1][3], &J[1][0]);
    const double ru = pu - u, rv = pv - v;
#pragma unroll
    for (int i = 0; i < 6; ++i)
#pragma unroll
        for (int j = i; j < 6; ++j) acc[pnp_tri(i, j)] += J[0][i] * J[0][j] + J[1][i] * J[1][j];
#pragma unroll
    for (int i = 0; i < 6; ++i) acc[21 + i] += J[0][i] * ru + J[1][i] * rv;
    acc[27] += ru * ru + rv * rv;
}

// the workgroup's LDS of the refinement kernel
struct PnpRefineLds {
    double red[4][28];
    double sum[28];      // block totals of the last pass
    double cand[12];     // pose the next pass evaluates
    double cur[12];      // last accepted pose ...
    double curA[28];     // ... and its normal equations / cost
    double lambda, step;
    int state;           // 0 running, 1 converged / stopped, 2 failed (non-finite)
    int have_cur;
    int count;
};

// block-wide sums of acc[0..27] into L.sum, fixed order; ends with a barrier
__device__ __forceinline__ void pnp_block_sum28(const double* acc, PnpRefineLds& L) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < 28; ++k) {
        const double s = wave_sum_f64(acc[k]);
        if (lane == 0) L.red[wave][k] = s;
    }
    __syncthreads();
    if (threadIdx.x < 28) L.sum[threadIdx.x] = (L.red[0][threadIdx.x] + L.red[1][threadIdx.x]) + (L.red[2][threadIdx.x] + L.red[3][threadIdx.x]);
    __syncthreads();
}

// Levenberg-Marquardt from the pose in L.cand over the points with mask[i] != 0 (mask == nullptr: all `count` points).  Every pass evaluates the
// candidate pose; thread 0 accepts it when the cost did not grow (lambda / 10) or rejects it (lambda * 10), solves the damped normal equations of
// the accepted pose and proposes the next candidate.  Stops after a step below PNP_STEP_TOL (rotation [rad], translation relative to |t|), which is
// still applied, or after max_iter passes.  The result is left in L.cur; false when nothing finite came out.  Called by the whole workgroup.
template <typename T>
__device__ bool pnp_lm(const T* __restrict__ img, const T* __restrict__ mod, const unsigned char* mask, int count, const double* K, int max_iter,
                       PnpRefineLds& L) {
    const int tid = threadIdx.x;
    if (tid == 0) {
        L.lambda = 1e-3;
        L.state = 0;
        L.have_cur = 0;
    }
    __syncthreads();
    for (int pass = 0; pass < max_iter; ++pass) {
        double R[9], t[3], acc[28];
#pragma unroll
        for (int k = 0; k < 9; ++k) R[k] = L.cand[k];
#pragma unroll
        for (int k = 0; k < 3; ++k) t[k] = L.cand[9 + k];
#pragma unroll
        for (int k = 0; k < 28; ++k) acc[k] = 0.0;
        for (int i = tid; i < count; i += PNP_THREADS) {
            if (mask != nullptr && mask[i] == 0) continue;
            const double X[3] = {(double)mod[(size_t)i * 3], (double)mod[(size_t)i * 3 + 1], (double)mod[(size_t)i * 3 + 2]};
            pnp_accumulate(K, R, t, X, (double)img[(size_t)i * 2], (double)img[(size_t)i * 2 + 1], acc);
        }
        pnp_block_sum28(acc, L);
        if (tid == 0) {
            const double F = L.sum[27];
            bool accept = pnp_finite(F) && (!L.have_cur || F <= L.curA[27]);
            if (accept) {
                for (int k = 0; k < 12; ++k) L.cur[k] = L.cand[k];
                for (int k = 0; k < 28; ++k) L.curA[k] = L.sum[k];
                if (L.have_cur) L.lambda = fmax(L.lambda * 0.1, 1e-15);
                L.have_cur = 1;
            } else if (!L.have_cur) {
                L.state = 2;   // the start itself is not finite
            } else {
                L.lambda *= 10.0;
                if (L.lambda > 1e10) L.state = 1;   // no downhill step left
            }
            if (L.state == 0) {
                double x[6];
                bool solved = false;
                for (int tries = 0; tries < 12 && !solved; ++tries) {
                    solved = pnp_solve6(L.curA, L.curA + 21, L.lambda, x);
                    if (!solved) L.lambda *= 10.0;
                }
                if (!solved) {
                    L.state = 1;   // singular normal equations (e.g. fewer than 3 usable points): keep the accepted pose
                } else {
                    pnp_rotate_left(x, L.cur, L.cand);
                    for (int k = 0; k < 3; ++k) L.cand[9 + k] = L.cur[9 + k] + x[3 + k];
                    const double tn = sqrt(pnp_dot(L.cur + 9, L.cur + 9));
                    const double step = fmax(sqrt(pnp_dot(x, x)), sqrt(pnp_dot(x + 3, x + 3)) / fmax(tn, 1e-300));
                    if (step < PNP_STEP_TOL) {
                        for (int k = 0; k < 12; ++k) L.cur[k] = L.cand[k];
                        L.state = 1;
                    }
                }
            }
        }
        __syncthreads();
        if (L.state != 0) break;   // (uniform: read behind the barrier)
    }
    __syncthreads();
    double chk = 0.0;
#pragma unroll
    for (int k = 0; k < 12; ++k) chk += L.cur[k];
    return L.have_cur != 0 && L.state != 2 && pnp_finite(chk);
}

// inliers of the pose L.cur: mask[i] = (z > 0 and squared pixel error < thr2) for i < count; the count and the inliers' squared error sum are left
// in L.count and L.sum[27].  thr2 < 0: no gate (every valid point counts, mask untouched).  Called by the whole workgroup.
template <typename T>
__device__ void pnp_select(const T* __restrict__ img, const T* __restrict__ mod, unsigned char* mask, int count, const double* K, double thr2,
                           PnpRefineLds& L) {
    const int tid = threadIdx.x;
    double R[9], t[3], acc[28];
#pragma unroll
    for (int k = 0; k < 9; ++k) R[k] = L.cur[k];
#pragma unroll
    for (int k = 0; k < 3; ++k) t[k] = L.cur[9 + k];
#pragma unroll
    for (int k = 0; k < 28; ++k) acc[k] = 0.0;
    for (int i = tid; i < count; i += PNP_THREADS) {
        const double X[3] = {(double)mod[(size_t)i * 3], (double)mod[(size_t)i * 3 + 1], (double)mod[(size_t)i * 3 + 2]};
        double Xc[3], pu, pv;
        pnp_xform(R, t, X, Xc);
        const bool front = pnp_project(K, Xc, &pu, &pv);
        const double du = pu - (double)img[(size_t)i * 2], dv = pv - (double)img[(size_t)i * 2 + 1];
        const double e = du * du + dv * dv;
        const bool in = thr2 < 0.0 ? true : (front && e < thr2);
        if (thr2 >= 0.0) mask[i] = in ? 1 : 0;
        if (in) {
            acc[26] += 1.0;   // (exact: a count below 2^53)
            acc[27] += e;
        }
    }
    pnp_block_sum28(acc, L);
    if (tid == 0) L.count = (int)L.sum[26];
    __syncthreads();
}

// One workgroup per RoI: hypotheses in chunks of PNP_HYP, each chunk scored against all points.  win[n] = (R, t, count) of the best hypothesis;
// count 0 when there is none.
template <typename T>
__global__ __launch_bounds__(PNP_THREADS) void pnp_ransac_kernel(const T* __restrict__ img_pts, const T* __restrict__ model_pts,
                                                                 const int* __restrict__ counts, const double* __restrict__ Kmat, int stride,
                                                                 double thr2, int iters, unsigned long long seed, double* __restrict__ win) {
    constexpr int TILE = PnpTile<T>::N;
    __shared__ double hyp[PNP_HYP * 12];   // K [R | t] of the chunk's hypotheses, NaN for a degenerate one
    __shared__ T s_img[TILE * 2];
    __shared__ T s_mod[TILE * 3];
    __shared__ int cnt[PNP_HYP];
    __shared__ unsigned long long best_key;
    __shared__ double best_pose[12];
    const int n = blockIdx.x, tid = threadIdx.x;
    const int count = min(max(counts[n], 0), stride);
    double* w = win + (size_t)n * PNP_WIN;
    if (count < 4) {   // (uniform over the workgroup)
        if (tid < PNP_WIN) w[tid] = 0.0;
        return;
    }
    const T* img = img_pts + (size_t)n * stride * 2;
    const T* mod = model_pts + (size_t)n * stride * 3;
    double K[9], Ki[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) K[k] = Kmat[(size_t)n * 9 + k];
    const bool k_ok = pnp_inv3(K, Ki);
    if (tid == 0) best_key = 0ull;
    if (tid < 12) best_pose[tid] = 0.0;
    for (int h0 = 0; h0 < iters; h0 += PNP_HYP) {
        const int nh = min(PNP_HYP, iters - h0);
        __syncthreads();   // the previous chunk has been consumed
        cnt[tid] = 0;
        double R[9], t[3];
        if (tid < nh) {
            const bool ok = k_ok && pnp_hypothesis(img, mod, count, K, Ki, seed, n, h0 + tid, R, t);
#pragma unroll
            for (int r = 0; r < 3; ++r) {
#pragma unroll
                for (int q = 0; q < 3; ++q)
                    hyp[tid * 12 + r * 4 + q] = ok ? K[r * 3] * R[q] + K[r * 3 + 1] * R[3 + q] + K[r * 3 + 2] * R[6 + q] : __builtin_nan("");
                hyp[tid * 12 + r * 4 + 3] = ok ? pnp_dot(K + r * 3, t) : __builtin_nan("");
            }
        }
        __syncthreads();
        // P = the power of two >= nh hypothesis lanes, 256 / P groups of threads share the tile's points between them
        int lg = 0;
        while ((1 << lg) < nh) ++lg;
        const int P = 1 << lg, G = PNP_THREADS >> lg, h = tid & (P - 1), g = tid >> lg;
        double M[12];
#pragma unroll
        for (int k = 0; k < 12; ++k) M[k] = hyp[(h < nh ? h : 0) * 12 + k];
        int local = 0;
        for (int t0 = 0; t0 < count; t0 += TILE) {
            const int c = min(TILE, count - t0);
            __syncthreads();   // the previous tile has been consumed
            for (int j = tid; j < c * 2; j += PNP_THREADS) s_img[j] = img[(size_t)t0 * 2 + j];
            for (int j = tid; j < c * 3; j += PNP_THREADS) s_mod[j] = mod[(size_t)t0 * 3 + j];
            __syncthreads();
            if (h < nh) {
                for (int j = g; j < c; j += G) {
                    const double X = (double)s_mod[j * 3], Y = (double)s_mod[j * 3 + 1], Z = (double)s_mod[j * 3 + 2];
                    const double u = (double)s_img[j * 2], v = (double)s_img[j * 2 + 1];
                    const double pw = fma(M[8], X, fma(M[9], Y, fma(M[10], Z, M[11])));
                    const double du = fma(M[0], X, fma(M[1], Y, fma(M[2], Z, M[3]))) - u * pw;
                    const double dv = fma(M[4], X, fma(M[5], Y, fma(M[6], Z, M[7]))) - v * pw;
                    local += (pw > 0.0 && du * du + dv * dv < thr2 * pw * pw) ? 1 : 0;   // the division-free form of the gate
                }
            }
        }
        if (h < nh && local > 0) atomicAdd(&cnt[h], local);   // integers: exact, order-free
        __syncthreads();
        unsigned long long key = 0ull;
        if (tid < nh) {
            key = ((unsigned long long)(unsigned)cnt[tid] << 32) | (unsigned long long)(0xFFFFFFFFu - (unsigned)(h0 + tid));
            if (cnt[tid] > 0) atomicMax(&best_key, key);   // highest count, then lowest index
        }
        __syncthreads();
        if (tid < nh && cnt[tid] > 0 && key == best_key) {   // at most one thread: the key carries the index
#pragma unroll
            for (int k = 0; k < 9; ++k) best_pose[k] = R[k];
#pragma unroll
            for (int k = 0; k < 3; ++k) best_pose[9 + k] = t[k];
        }
    }
    __syncthreads();
    if (tid < 12) w[tid] = best_pose[tid];
    else if (tid == 12) w[12] = (double)(unsigned)(best_key >> 32);
    else if (tid < PNP_WIN) w[tid] = 0.0;
}

// One workgroup per RoI.  mode 0: from the RANSAC winner in win[n] -- inliers of the winner, refine on them, re-select, refine once more, and the
// mask / count / rms of the pose that is returned.  mode 1: from the caller's (R, t) over all valid points, no gate.  A row that cannot be solved
// keeps the caller's R and t and gets ok = 0 (num_inliers 0, mask 0, rms NaN).  mask is [N][stride] (mode 0: never NULL, the host passes scratch).
template <typename T>
__global__ __launch_bounds__(PNP_THREADS) void pnp_refine_kernel(const T* __restrict__ img_pts, const T* __restrict__ model_pts,
                                                                 const int* __restrict__ counts, const double* __restrict__ Kmat, int stride,
                                                                 int mode, double thr2, int max_iter, const double* __restrict__ win,
                                                                 double* __restrict__ R_io, double* __restrict__ t_io, int* __restrict__ ok,
                                                                 int* __restrict__ num_inliers, unsigned char* __restrict__ mask_all,
                                                                 double* __restrict__ rms) {
    __shared__ PnpRefineLds L;
    const int n = blockIdx.x, tid = threadIdx.x;
    const int count = min(max(counts[n], 0), stride);
    const T* img = img_pts + (size_t)n * stride * 2;
    const T* mod = model_pts + (size_t)n * stride * 3;
    unsigned char* mask = mask_all ? mask_all + (size_t)n * stride : nullptr;
    double K[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) K[k] = Kmat[(size_t)n * 9 + k];
    bool good = count >= 4;
    if (mode == 0) good = good && win[(size_t)n * PNP_WIN + 12] >= 4.0;
    if (good) {   // (every condition below is uniform over the workgroup)
        if (tid < 12) L.cur[tid] = mode == 0 ? win[(size_t)n * PNP_WIN + tid] : (tid < 9 ? R_io[(size_t)n * 9 + tid] : t_io[(size_t)n * 3 + tid - 9]);
        __syncthreads();
        if (mode == 0) {
            for (int round = 0; round < 2 && good; ++round) {
                pnp_select(img, mod, mask, count, K, thr2, L);
                good = L.count >= 4;
                if (good) {
                    if (tid < 12) L.cand[tid] = L.cur[tid];
                    __syncthreads();
                    good = pnp_lm(img, mod, mask, count, K, max_iter, L);
                }
            }
            if (good) {
                pnp_select(img, mod, mask, count, K, thr2, L);
                good = L.count >= 4;
            }
        } else {
            if (tid < 12) L.cand[tid] = L.cur[tid];
            __syncthreads();
            good = pnp_lm(img, mod, (const unsigned char*)nullptr, count, K, max_iter, L);
            if (good) pnp_select(img, mod, (unsigned char*)nullptr, count, K, -1.0, L);
        }
        if (good) good = pnp_finite(L.sum[27]);
    }
    __syncthreads();
    if (good) {
        if (tid < 9) R_io[(size_t)n * 9 + tid] = L.cur[tid];
        else if (tid < 12) t_io[(size_t)n * 3 + tid - 9] = L.cur[tid];
    }
    if (tid == 0) {
        ok[n] = good ? 1 : 0;
        if (num_inliers) num_inliers[n] = good ? L.count : 0;
        if (rms) rms[n] = good ? sqrt(L.sum[27] / (double)L.count) : __builtin_nan("");
    }
    if (mode == 0 && mask)   // rows beyond counts[n] are no inliers; an unsolved RoI has none
        for (int i = good ? count + tid : tid; i < stride; i += PNP_THREADS) mask[i] = 0;
}

int pnp_counts_ok(const int* counts_host, int N, int stride) {
    for (int i = 0; i < N; ++i)
        if (counts_host[i] < 0 || counts_host[i] > stride) return 0;
    return 1;
}

long long pnp_win_bytes(int N) { return (((long long)N * PNP_WIN * (long long)sizeof(double)) + 255) / 256 * 256; }

template <typename T>
int pnp_ransac_launch(const T* img_pts, const T* model_pts, const int* counts, const int* counts_host, const double* K, int N, int stride,
                      double reproj_err, int iters, unsigned long long seed, int max_iter, double* R, double* t, int* ok, int* num_inliers,
                      unsigned char* inlier_mask, double* rms, void* workspace, void* stream) {
    if (!img_pts || !model_pts || !counts || !counts_host || !K || !R || !t || !ok || !num_inliers || !workspace) return GDRN_ERR_ARG;
    if (N <= 0 || stride <= 0 || iters <= 0 || max_iter <= 0 || !(reproj_err > 0.0)) return GDRN_ERR_ARG;
    if (!pnp_counts_ok(counts_host, N, stride)) return GDRN_ERR_ARG;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    double* win = reinterpret_cast<double*>(workspace);
    unsigned char* mask = inlier_mask ? inlier_mask : reinterpret_cast<unsigned char*>(workspace) + pnp_win_bytes(N);
    const double thr2 = reproj_err * reproj_err;
    GDRN_LAUNCH((pnp_ransac_kernel<T>), dim3(N), dim3(PNP_THREADS), 0, st, img_pts, model_pts, counts, K, stride, thr2, iters, seed, win);
    GDRN_CHECK_LAUNCH();
    GDRN_LAUNCH((pnp_refine_kernel<T>), dim3(N), dim3(PNP_THREADS), 0, st, img_pts, model_pts, counts, K, stride, 0, thr2, max_iter,
                (const double*)win, R, t, ok, num_inliers, mask, rms);
    GDRN_CHECK_LAUNCH();
    return GDRN_OK;
}

template <typename T>
int pnp_refine_launch(const T* img_pts, const T* model_pts, const int* counts, const int* counts_host, const double* K, int N, int stride,
                      int max_iter, double* R, double* t, int* ok, double* rms, void* stream) {
    if (!img_pts || !model_pts || !counts || !counts_host || !K || !R || !t || !ok) return GDRN_ERR_ARG;
    if (N <= 0 || stride <= 0 || max_iter <= 0) return GDRN_ERR_ARG;
    if (!pnp_counts_ok(counts_host, N, stride)) return GDRN_ERR_ARG;
    GDRN_LAUNCH((pnp_refine_kernel<T>), dim3(N), dim3(PNP_THREADS), 0, reinterpret_cast<hipStream_t>(stream), img_pts, model_pts, counts, K,
                stride, 1, -1.0, max_iter, (const double*)nullptr, R, t, ok, (int*)nullptr, (unsigned char*)nullptr, rms);
    GDRN_CHECK_LAUNCH();
    return GDRN_OK;
}

}  // namespace

extern "C" long long gdrn_pnp_workspace_bytes(int N, int stride, int iters) {
    if (N <= 0 || stride <= 0 || iters <= 0) return GDRN_ERR_ARG;
    return pnp_win_bytes(N) + (long long)N * stride;   // the winners + an inlier mask for the calls that pass none
}

extern "C" int gdrn_pnp_ransac(const float* img_pts, const float* model_pts, const int* counts, const int* counts_host, const double* K, int N,
                               int stride, double reproj_err, int iters, unsigned long long seed, int max_iter, double* R, double* t, int* ok,
                               int* num_inliers, unsigned char* inlier_mask, double* rms, void* workspace, void* stream) {
    return pnp_ransac_launch<float>(img_pts, model_pts, counts, counts_host, K, N, stride, reproj_err, iters, seed, max_iter, R, t, ok, num_inliers,
                                    inlier_mask, rms, workspace, stream);
}

extern "C" int gdrn_pnp_ransac_f64(const double* img_pts, const double* model_pts, const int* counts, const int* counts_host, const double* K, int N,
                                   int stride, double reproj_err, int iters, unsigned long long seed, int max_iter, double* R, double* t, int* ok,
                                   int* num_inliers, unsigned char* inlier_mask, double* rms, void* workspace, void* stream) {
    return pnp_ransac_launch<double>(img_pts, model_pts, counts, counts_host, K, N, stride, reproj_err, iters, seed, max_iter, R, t, ok, num_inliers,
                                     inlier_mask, rms, workspace, stream);
}

extern "C" int gdrn_pnp_refine(const float* img_pts, const float* model_pts, const int* counts, const int* counts_host, const double* K, int N,
                               int stride, int max_iter, double* R, double* t, int* ok, double* rms, void* workspace, void* stream) {
    (void)workspace;
    return pnp_refine_launch<float>(img_pts, model_pts, counts, counts_host, K, N, stride, max_iter, R, t, ok, rms, stream);
}

extern "C" int gdrn_pnp_refine_f64(const double* img_pts, const double* model_pts, const int* counts, const int* counts_host, const double* K, int N,
                                   int stride, int max_iter, double* R, double* t, int* ok, double* rms, void* workspace, void* stream) {
    (void)workspace;
    return pnp_refine_launch<double>(img_pts, model_pts, counts, counts_host, K, N, stride, max_iter, R, t, ok, rms, stream);
}
