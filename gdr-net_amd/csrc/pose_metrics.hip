// On-device pose-error metrics of the GDR-Net evaluation for gfx950: what the reference's evaluator computes on the host, one instance at a time,
// right after inference (GDRN_EvaluatorCustom._eval_predictions, core/gdrn_modeling/gdrn_custom_evaluator.py:493-670) --
//   te, re            lib/pysixd/pose_error.py:400-436
//   get_closest_rot   core/utils/pose_utils.py:430-454 (symmetric classes: the ground-truth rotation times the symmetry with the smallest re)
//   arp_2d ("proj")   pose_error.py:439-444, against the closest ground-truth rotation
//   add / adi ("ad")  pose_error.py:297-337: adi for the symmetric classes, against the PLAIN ground-truth rotation (evaluator :573-575); the
//                     reference builds a SciPy KD-tree per instance, here an exact brute-force nearest neighbour (same minimum, O(n^2) fp64)
// -- and the 15 recall flags of :593-611 accumulated per class.  Everything is fp64 like the reference's numpy: the flags are threshold decisions
// on these numbers.  No floating-point atomics: per-workgroup partial sums go to a caller-owned workspace and are added up in a fixed order,
// two runs give the same bits.  (The file has no 16-bit code: both library builds compile the same thing.)
#include "common.h"
#include "geom64.h"
#include "points64.h"
#include "../../include/gdrn_hip.h"

namespace {

constexpr int PM_THREADS = 256;
constexpr int PM_G = 4;                        // ground-truth-posed points a thread keeps in registers
constexpr int PM_SLAB = PM_THREADS * PM_G;     // points of one workgroup
constexpr int PM_TILE = 512;                   // estimate-posed points per LDS tile (3 x 4 KiB)
constexpr int PM_FLAGS = 15;

// (re_deg, pose_error.py:400-415, and the adi tile loop: points64.h)

// One thread per row: te, the closest ground-truth rotation (kept in rsel[row][9] for the point kernel) and re.
__global__ __launch_bounds__(PM_THREADS) void pose_row_kernel(const double* __restrict__ R_est, const double* __restrict__ t_est,
                                                              const double* __restrict__ R_gt, const double* __restrict__ t_gt,
                                                              const int* __restrict__ labels, const int* __restrict__ is_sym,
                                                              const double* __restrict__ sym, const int* __restrict__ nsym, int Kmax, int C,
                                                              int N, double* __restrict__ err, double* __restrict__ rsel) {
    const int i = blockIdx.x * PM_THREADS + threadIdx.x;
    if (i >= N) return;
    const int c = labels[i];
    double* e = err + (size_t)i * 4;
    if (c < 0 || c >= C) {   // (the host wrapper refuses such a label before the launch: never index a table with it)
        e[0] = e[1] = e[2] = e[3] = __builtin_nan("");
        return;
    }
    double Re[9], Rg[9], Rb[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) {
        Re[k] = R_est[(size_t)i * 9 + k];
        Rg[k] = R_gt[(size_t)i * 9 + k];
        Rb[k] = Rg[k];
    }
    const double d0 = t_gt[i * 3 + 0] - t_est[i * 3 + 0], d1 = t_gt[i * 3 + 1] - t_est[i * 3 + 1], d2 = t_gt[i * 3 + 2] - t_est[i * 3 + 2];
    double best = re_deg(Re, Rg);
    if (is_sym[c] && sym != nullptr) {
        const int ns = min(max(nsym[c], 0), Kmax);
        for (int s = 0; s < ns; ++s) {
            const double* S = sym + ((size_t)c * Kmax + s) * 9;
            double Rs[9];   // R_gt S_s
#pragma unroll
            for (int r = 0; r < 3; ++r)
#pragma unroll
                for (int q = 0; q < 3; ++q) Rs[r * 3 + q] = Rg[r * 3 + 0] * S[0 * 3 + q] + Rg[r * 3 + 1] * S[1 * 3 + q] + Rg[r * 3 + 2] * S[2 * 3 + q];
            const double cur = re_deg(Re, Rs);
            if (cur < best) {   // strictly smaller, in the order of the table
                best = cur;
#pragma unroll
                for (int k = 0; k < 9; ++k) Rb[k] = Rs[k];
            }
        }
    }
    e[1] = best;
    e[2] = norm3(d0, d1, d2);
#pragma unroll
    for (int k = 0; k < 9; ++k) rsel[(size_t)i * 9 + k] = Rb[k];
}

// One workgroup per (slab of PM_SLAB model points, row).  Every thread poses PM_G points of the slab three ways (estimate, ground truth, closest
// ground truth) and adds their reprojection distance -- and, for a non-symmetric class, their 3D distance (add) -- to the slab's sums.  For a
// symmetric class the ground-truth-posed points stay in registers while ALL the class's estimate-posed points stream through LDS in tiles of
// PM_TILE (posed once on the way in, every LDS read a broadcast): the running minimum is a squared distance, one sqrt per point at the end (adi).
// Table rows beyond npts[c] are never read into a sum or a minimum: the slab's tail threads carry valid = false, the tile loop stops at npts.
__global__ __launch_bounds__(PM_THREADS) void pose_points_kernel(const double* __restrict__ R_est, const double* __restrict__ t_est,
                                                                 const double* __restrict__ R_gt, const double* __restrict__ t_gt,
                                                                 const double* __restrict__ Kmat, const int* __restrict__ labels,
                                                                 const double* __restrict__ pts, const int* __restrict__ npts,
                                                                 const int* __restrict__ is_sym, int n_max, int C,
                                                                 const double* __restrict__ rsel, double* __restrict__ partial, int slabs) {
    __shared__ double sx[PM_TILE], sy[PM_TILE], sz[PM_TILE];
    __shared__ double red[4];
    const int row = blockIdx.y, slab = blockIdx.x, tid = threadIdx.x;
    const int c = labels[row];
    if (c < 0 || c >= C) return;
    const int n = min(npts[c], n_max);
    const int base = slab * PM_SLAB;
    if (base >= n) return;   // (the finalise pass reads the slabs below ceil(n / PM_SLAB) only)
    const bool symc = is_sym[c] != 0;
    double Re[9], Rg[9], Rs[9], Km[9], te[3], tg[3];
#pragma unroll
    for (int k = 0; k < 9; ++k) {
        Re[k] = R_est[(size_t)row * 9 + k];
        Rg[k] = R_gt[(size_t)row * 9 + k];
        Rs[k] = rsel[(size_t)row * 9 + k];
        Km[k] = Kmat[(size_t)row * 9 + k];
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        te[k] = t_est[row * 3 + k];
        tg[k] = t_gt[row * 3 + k];
    }
    const double zero3[3] = {0.0, 0.0, 0.0};
    const double* P = pts + (size_t)c * n_max * 3;
    V3 g[PM_G];
    bool valid[PM_G];
    double s_ad = 0.0, s_pr = 0.0;
#pragma unroll
    for (int u = 0; u < PM_G; ++u) {
        const int idx = base + u * PM_THREADS + tid;
        valid[u] = idx < n;
        V3 p = {0.0, 0.0, 0.0};
        if (valid[u]) p = load3(P + (size_t)idx * 3);
        const V3 pe = xform(Re, te, p);
        g[u] = xform(Rg, tg, p);
        const V3 ps = xform(Rs, tg, p);
        if (valid[u]) {
            // transform_pts_Rt_2d (pose_error.py:277-294): K (R p + t), divided by the third row
            const V3 ue = xform(Km, zero3, pe), ug = xform(Km, zero3, ps);
            const double du = ue.x / ue.z - ug.x / ug.z, dv = ue.y / ue.z - ug.y / ug.z;
            s_pr += sqrt(du * du + dv * dv);
            if (!symc) {
                const double dx = pe.x - g[u].x, dy = pe.y - g[u].y, dz = pe.z - g[u].z;
                s_ad += norm3(dx, dy, dz);
            }
        }
    }
    if (symc) {   // (uniform over the workgroup: the barriers below are reached by all of it or none)
        double best[PM_G];
#pragma unroll
        for (int u = 0; u < PM_G; ++u) best[u] = INFINITY;
        nearest_sq_tiles<PM_G, PM_TILE, PM_THREADS>(P, n, Re, te, g, best, sx, sy, sz, tid);
#pragma unroll
        for (int u = 0; u < PM_G; ++u)
            if (valid[u]) s_ad += sqrt(best[u]);
    }
    s_ad = block_sum_256_f64(s_ad, red);
    s_pr = block_sum_256_f64(s_pr, red);
    if (tid == 0) {
        double* o = partial + ((size_t)row * slabs + slab) * 2;
        o[0] = s_ad;
        o[1] = s_pr;
    }
}

// One thread per row: the slabs' sums in slab order, divided by the point count.
__global__ __launch_bounds__(PM_THREADS) void pose_finalize_kernel(const int* __restrict__ labels, const int* __restrict__ npts, int n_max, int C,
                                                                   int N, const double* __restrict__ partial, int slabs,
                                                                   double* __restrict__ err) {
    const int i = blockIdx.x * PM_THREADS + threadIdx.x;
    if (i >= N) return;
    const int c = labels[i];
    if (c < 0 || c >= C) return;
    const int n = min(npts[c], n_max);
    const int used = (n + PM_SLAB - 1) / PM_SLAB;
    double s_ad = 0.0, s_pr = 0.0;
    for (int s = 0; s < used; ++s) {
        s_ad += partial[((size_t)i * slabs + s) * 2 + 0];
        s_pr += partial[((size_t)i * slabs + s) * 2 + 1];
    }
    err[(size_t)i * 4 + 0] = s_ad / (double)n;
    err[(size_t)i * 4 + 3] = s_pr / (double)n;
}

// One workgroup per class: the 15 recall flags of its rows (gdrn_custom_evaluator.py:593-611, strict <) counted in LDS, the re / te sums reduced in
// a fixed order, then added to the caller's running state by this workgroup alone (launches on one stream follow each other: no global atomics).
__global__ __launch_bounds__(PM_THREADS) void pose_recall_kernel(const double* __restrict__ err, const int* __restrict__ labels, int N,
                                                                 const double* __restrict__ diameter, long long* __restrict__ hits,
                                                                 long long* __restrict__ seen, double* __restrict__ re_sum,
                                                                 double* __restrict__ te_sum, long long* __restrict__ err_cnt) {
    __shared__ int cnt[PM_FLAGS + 1];
    __shared__ double red[4];
    const int c = blockIdx.x, tid = threadIdx.x;
    if (tid <= PM_FLAGS) cnt[tid] = 0;
    __syncthreads();
    const double d = diameter[c];
    double s_re = 0.0, s_te = 0.0;
    for (int i = tid; i < N; i += PM_THREADS) {
        if (labels[i] != c) continue;
        const double ad = err[(size_t)i * 4 + 0], re = err[(size_t)i * 4 + 1], te = err[(size_t)i * 4 + 2], pr = err[(size_t)i * 4 + 3];
        const bool f[PM_FLAGS] = {ad < 0.02 * d, ad < 0.05 * d, ad < 0.1 * d,
                                  re < 2.0 && te < 0.02, re < 5.0 && te < 0.05, re < 10.0 && te < 0.1,
                                  re < 2.0, re < 5.0, re < 10.0,
                                  te < 0.02, te < 0.05, te < 0.1,
                                  pr < 2.0, pr < 5.0, pr < 10.0};
#pragma unroll
        for (int k = 0; k < PM_FLAGS; ++k)
            if (f[k]) atomicAdd(&cnt[k], 1);
        atomicAdd(&cnt[PM_FLAGS], 1);
        s_re += re;
        s_te += te;
    }
    s_re = block_sum_256_f64(s_re, red);
    s_te = block_sum_256_f64(s_te, red);   // (its first barrier also orders the LDS counters)
    if (tid < PM_FLAGS) hits[(size_t)c * PM_FLAGS + tid] += cnt[tid];
    if (tid == PM_FLAGS) {
        seen[c] += cnt[PM_FLAGS];
        err_cnt[c] += cnt[PM_FLAGS];
        re_sum[c] += s_re;
        te_sum[c] += s_te;
    }
}

}  // namespace

extern "C" long long gdrn_pose_metrics_workspace_bytes(int N, int n_max) {
    if (N <= 0 || n_max <= 0) return GDRN_ERR_ARG;
    const long long slabs = (n_max + PM_SLAB - 1) / PM_SLAB;
    return (long long)N * (9 + 2 * slabs) * (long long)sizeof(double);
}

extern "C" int gdrn_pose_errors(const double* R_est, const double* t_est, const double* R_gt, const double* t_gt, const double* K,
                                const int* labels, const int* labels_host, int N, const double* pts, const int* npts, int n_max,
                                const int* is_sym, const double* sym, const int* nsym, int Kmax, int C, double* err, void* workspace,
                                void* stream) {
    if (!R_est || !t_est || !R_gt || !t_gt || !K || !labels || !labels_host || !pts || !npts || !is_sym || !err || !workspace) return GDRN_ERR_ARG;
    if (N <= 0 || n_max <= 0 || C <= 0 || Kmax < 0 || (Kmax > 0 && (!sym || !nsym))) return GDRN_ERR_ARG;
    if (!host_in_range(labels_host, N, C)) return GDRN_ERR_ARG;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const int slabs = cdiv(n_max, PM_SLAB);
    double* rsel = reinterpret_cast<double*>(workspace);
    double* partial = rsel + (size_t)N * 9;
    GDRN_LAUNCH(pose_row_kernel, dim3(cdiv(N, PM_THREADS)), dim3(PM_THREADS), 0, st, R_est, t_est, R_gt, t_gt, labels, is_sym,
                Kmax > 0 ? sym : nullptr, nsym, Kmax, C, N, err, rsel);
    GDRN_CHECK_LAUNCH();
    GDRN_LAUNCH(pose_points_kernel, dim3(slabs, N), dim3(PM_THREADS), 0, st, R_est, t_est, R_gt, t_gt, K, labels, pts, npts, is_sym, n_max, C,
                rsel, partial, slabs);
    GDRN_CHECK_LAUNCH();
    GDRN_LAUNCH(pose_finalize_kernel, dim3(cdiv(N, PM_THREADS)), dim3(PM_THREADS), 0, st, labels, npts, n_max, C, N, partial, slabs, err);
    GDRN_CHECK_LAUNCH();
    return GDRN_OK;
}

extern "C" int gdrn_pose_recall_accumulate(const double* err, const int* labels, const int* labels_host, int N, const double* diameter, int C,
                                           long long* hits, long long* seen, double* re_sum, double* te_sum, long long* err_cnt,
                                           void* stream) {
    if (!err || !labels || !labels_host || !diameter || !hits || !seen || !re_sum || !te_sum || !err_cnt || N <= 0 || C <= 0) return GDRN_ERR_ARG;
    if (!host_in_range(labels_host, N, C)) return GDRN_ERR_ARG;
    GDRN_LAUNCH(pose_recall_kernel, dim3(C), dim3(PM_THREADS), 0, reinterpret_cast<hipStream_t>(stream), err, labels, N, diameter, hits, seen,
                re_sum, te_sum, err_cnt);
    GDRN_CHECK_LAUNCH();
    return GDRN_OK;
}
