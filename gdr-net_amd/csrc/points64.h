// What the per-point fp64 evaluation kernels (pose_metrics.hip, bop_metrics.hip, sixd_scores.hip) share beyond geom64.h: the rotation error, the
// exact nearest-neighbour tile loop of adi, the pose of a symmetry transformation under the ground truth and the projected point.  Include after
// common.h and geom64.h, and -- like geom64.h -- BEFORE a file switches floating-point contraction off: every function here is compiled the same
// way in every file that includes it, so a quantity two kernels both compute through one of them is the same bits in both.
#pragma once

namespace {

// pose_error.py:400-415: rad2deg(arccos(clamp(0.5 (min(tr(A B^T), 3) - 1), -1, 1)))
__device__ __forceinline__ double re_deg(const double* A, const double* B) {
    double tr = 0.0;
#pragma unroll
    for (int i = 0; i < 9; ++i) tr += A[i] * B[i];
    tr = tr <= 3.0 ? tr : 3.0;
    const double c = fmin(1.0, fmax(-1.0, 0.5 * (tr - 1.0)));
    return acos(c) * (180.0 / 3.14159265358979323846);
}

// np.linalg.norm of a 3-vector (te, and the point distance of add)
__device__ __forceinline__ double norm3(double x, double y, double z) { return sqrt(x * x + y * y + z * z); }

// The nearest estimate-posed point of each of a thread's G ground-truth-posed points g[]: ALL n points of the class stream through LDS in tiles of
// TILE (posed once on the way in by the THREADS threads of the workgroup, every LDS read a broadcast), best[] keeps the smallest SQUARED distance
// (start it at INFINITY).  Reached by the whole workgroup or by none of it (barriers).  Rows beyond n are never read.
template <int G, int TILE, int THREADS>
__device__ __forceinline__ void nearest_sq_tiles(const double* __restrict__ P, int n, const double* Re, const double* te, const V3* g, double* best,
                                                 double* sx, double* sy, double* sz, int tid) {
    for (int t0 = 0; t0 < n; t0 += TILE) {
        const int cnt = min(TILE, n - t0);
        __syncthreads();   // the previous tile has been consumed
        for (int j = tid; j < cnt; j += THREADS) {
            const V3 pe = xform(Re, te, load3(P + (size_t)(t0 + j) * 3));
            sx[j] = pe.x;
            sy[j] = pe.y;
            sz[j] = pe.z;
        }
        __syncthreads();
#pragma unroll 4
        for (int j = 0; j < cnt; ++j) {
            const double ex = sx[j], ey = sy[j], ez = sz[j];
#pragma unroll
            for (int u = 0; u < G; ++u) {
                const double dx = g[u].x - ex, dy = g[u].y - ey, dz = g[u].z - ez;
                best[u] = fmin(best[u], dx * dx + dy * dy + dz * dz);
            }
        }
    }
}

// misc.project_pts (misc.py:511-525): P = K [R | t] (3 x 4), then P [p, 1] divided by its third row
__device__ __forceinline__ void make_proj(const double* K, const double* R, const double* t, double* P) {
#pragma unroll
    for (int r = 0; r < 3; ++r) {
#pragma unroll
        for (int q = 0; q < 3; ++q) P[r * 4 + q] = fma(K[r * 3 + 0], R[q], fma(K[r * 3 + 1], R[3 + q], K[r * 3 + 2] * R[6 + q]));
        P[r * 4 + 3] = fma(K[r * 3 + 0], t[0], fma(K[r * 3 + 1], t[1], K[r * 3 + 2] * t[2]));
    }
}
__device__ __forceinline__ void project(const double* P, V3 p, double& u, double& v) {
    const double a = fma(P[0], p.x, fma(P[1], p.y, fma(P[2], p.z, P[3])));
    const double b = fma(P[4], p.x, fma(P[5], p.y, fma(P[6], p.z, P[7])));
    const double w = fma(P[8], p.x, fma(P[9], p.y, fma(P[10], p.z, P[11])));
    u = a / w;
    v = b / w;
}

// the pose of symmetry (S, ts) of a class under the ground truth: R_gt S, R_gt ts + t_gt (pose_error.py:149-150)
__device__ __forceinline__ void sym_gt_pose(const double* Rg, const double* tg, const double* S, const double* ts, double* R, double* t) {
#pragma unroll
    for (int r = 0; r < 3; ++r) {
#pragma unroll
        for (int q = 0; q < 3; ++q) R[r * 3 + q] = fma(Rg[r * 3 + 0], S[q], fma(Rg[r * 3 + 1], S[3 + q], Rg[r * 3 + 2] * S[6 + q]));
        t[r] = fma(Rg[r * 3 + 0], ts[0], fma(Rg[r * 3 + 1], ts[1], Rg[r * 3 + 2] * ts[2])) + tg[r];
    }
}

// maximum / minimum that keep a NaN once they have seen one (fmax / fmin drop it): a NaN pose gives a NaN error
__device__ __forceinline__ double nanmax(double m, double d) { return (d > m || d != d) ? d : m; }
__device__ __forceinline__ double nanmin(double m, double d) { return (d < m || d != d) ? d : m; }

}  // namespace
