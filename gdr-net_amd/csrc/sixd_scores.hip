// The pose errors and recall counts behind the reference's YCB-V tables for gfx950: what it gets by writing a CSV and running the toolkit's scripts
// on the host, one estimate at a time (ERROR_TYPES = "AUCadd,AUCadi,AUCad,ad,ABSadd,ABSadi,ABSad" in every configs/gdrn/ycbv* file, and the
// default "projS", "ad", "reteS" of core/gdrn_modeling/test_utils.py:246-248) --
//   add AND adi of every row    lib/pysixd/pose_error.py:297-337 as eval_calc_errors.py:395-406 calls them (plain ground truth) -> gdrn_ad_errors
//   re_sym / te_sym / arp_2d_sym  pose_error.py:184-234 as eval_calc_errors.py:412-448 calls them, each the minimum over the class's
//                                 symmetry transformations                                                                       -> gdrn_sym_errors
//   the "correct" decisions of pose_matching.match_poses (:68, strict <) under the thresholds of eval_pose_results_more.py:64-93 with the
//   normalisations of eval_calc_scores.py:238-250, counted per class                                                 -> gdrn_score_recall_accumulate
// -- for a whole batch of estimates per call.  Everything is fp64 like the reference's numpy, lengths in metres.  No floating-point atomics: sums
// are per-workgroup partials added in a fixed order, minima are finished in slab order, counts are integers; two runs give the same bits.  Each
// per-row result is written once, by a plain vector store.  The adi tile loop, the rotation error and the projected point are the ones of
// pose_metrics.hip and bop_metrics.hip (points64.h).  (No 16-bit code: both library builds compile the same thing.)
#include "common.h"
#include "geom64.h"
#include "points64.h"
#include "../../include/gdrn_hip.h"

namespace {

constexpr int SX_THREADS = 256;
// adi: 4 ground-truth-posed points per thread in registers, 512 estimate-posed points per LDS tile (3 x 4 KiB) -- the shape pose_metrics.hip
// measured for the same loop: per LDS broadcast read of one estimate point (3 ds_read_b64, the same address in all 64 lanes: one pass each, no bank
// conflict) a thread issues 4 x 7 fp64 VALU operations, so the fp64 pipe and not LDS is the limit; more points per thread only add registers.
constexpr int AD_G = 4;
constexpr int AD_SLAB = SX_THREADS * AD_G;     // points of one workgroup (GDRN_SIXD_AD_SLAB)
constexpr int AD_TILE = 512;                   // estimate-posed points per LDS tile (GDRN_SIXD_AD_TILE)
constexpr int SY_SLAB = GDRN_SIXD_SYM_SLAB;    // symmetry transformations per workgroup
constexpr int NF = GDRN_SIXD_NFLAGS;
static_assert(AD_SLAB == GDRN_SIXD_AD_SLAB && AD_TILE == GDRN_SIXD_AD_TILE, "the header documents these sizes");

// ---- add and adi ----

// One workgroup per (slab of AD_SLAB model points, row): every thread poses AD_G points of the slab under the estimate and the ground truth and
// adds their distance (add); the ground-truth-posed ones stay in registers while ALL the class's estimate-posed points stream through LDS
// (nearest_sq_tiles: the running minimum is a squared distance, one sqrt per point at the end: adi).  Table rows beyond npts[c] are never read
// into a sum or a minimum: the slab's tail threads carry valid = false, the tile loop stops at npts.
__global__ __launch_bounds__(SX_THREADS) void ad_points_kernel(const double* __restrict__ R_est, const double* __restrict__ t_est,
                                                               const double* __restrict__ R_gt, const double* __restrict__ t_gt,
                                                               const int* __restrict__ labels, const double* __restrict__ pts,
                                                               const int* __restrict__ npts, int n_max, int C, double* __restrict__ partial,
                                                               int slabs) {
    __shared__ double sx[AD_TILE], sy[AD_TILE], sz[AD_TILE];
    __shared__ double red[4];
    const int row = blockIdx.y, slab = blockIdx.x, tid = threadIdx.x;
    const int c = labels[row];
    if (c < 0 || c >= C) return;   // (the host side of the entry point refuses such a label before the launch: never index a table with it)
    const int n = min(npts[c], n_max);
    const int base = slab * AD_SLAB;
    if (base >= n) return;   // uniform over the workgroup (the finish pass reads the slabs below ceil(n / AD_SLAB) only)
    double Re[9], Rg[9], te[3], tg[3];
#pragma unroll
    for (int k = 0; k < 9; ++k) {
        Re[k] = R_est[(size_t)row * 9 + k];
        Rg[k] = R_gt[(size_t)row * 9 + k];
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        te[k] = t_est[(size_t)row * 3 + k];
        tg[k] = t_gt[(size_t)row * 3 + k];
    }
    const double* P = pts + (size_t)c * n_max * 3;
    V3 g[AD_G];
    bool valid[AD_G];
    double best[AD_G];
    double s_add = 0.0, s_adi = 0.0;
#pragma unroll
    for (int u = 0; u < AD_G; ++u) {
        const int idx = base + u * SX_THREADS + tid;
        valid[u] = idx < n;
        V3 p = {0.0, 0.0, 0.0};
        if (valid[u]) p = load3(P + (size_t)idx * 3);
        const V3 pe = xform(Re, te, p);
        g[u] = xform(Rg, tg, p);
        if (valid[u]) {
            const double dx = pe.x - g[u].x, dy = pe.y - g[u].y, dz = pe.z - g[u].z;
            s_add += norm3(dx, dy, dz);
        }
        best[u] = INFINITY;
    }
    nearest_sq_tiles<AD_G, AD_TILE, SX_THREADS>(P, n, Re, te, g, best, sx, sy, sz, tid);
#pragma unroll
    for (int u = 0; u < AD_G; ++u)
        if (valid[u]) s_adi += sqrt(best[u]);
    s_add = block_sum_256_f64(s_add, red);
    s_adi = block_sum_256_f64(s_adi, red);
    if (tid == 0) {
        double* o = partial + ((size_t)row * slabs + slab) * 2;
        o[0] = s_add;
        o[1] = s_adi;
    }
}

// One thread per row: the slabs' sums in slab order, divided by the point count.
__global__ __launch_bounds__(SX_THREADS) void ad_finish_kernel(const int* __restrict__ labels, const int* __restrict__ npts, int n_max, int C, int N,
                                                               const double* __restrict__ partial, int slabs, double* __restrict__ err) {
    const int i = blockIdx.x * SX_THREADS + threadIdx.x;
    if (i >= N) return;
    const int c = labels[i];
    double s_add = __builtin_nan(""), s_adi = __builtin_nan("");
    if (c >= 0 && c < C) {
        const int n = min(npts[c], n_max);
        const int used = (n + AD_SLAB - 1) / AD_SLAB;
        s_add = 0.0;
        s_adi = 0.0;
        for (int s = 0; s < used; ++s) {
            s_add += partial[((size_t)i * slabs + s) * 2 + 0];
            s_adi += partial[((size_t)i * slabs + s) * 2 + 1];
        }
        s_add = s_add / (double)n;
        s_adi = s_adi / (double)n;
    }
    err[(size_t)i * 2 + 0] = s_add;
    err[(size_t)i * 2 + 1] = s_adi;
}

// ---- re_sym, te_sym, arp_2d_sym ----

// pose_error.te_sym (pose_error.py:206-221) AS IT RUNS: it adds the flattened t_gt [3] to the column R_gt t_S [3,1], which numpy broadcasts to the
// 3 x 3 matrix M[i][j] = (R_gt t_S)[i] + t_gt[j] - t_est[j], and returns M's Frobenius norm -- not the distance of two translations (for a class
// with the identity only it is sqrt(3) |t_gt - t_est|).  The toolkit's teS / reteS decisions are taken on this value, so it is the one computed here.
__device__ __forceinline__ double te_sym_as_run(const double* Rg, const double* ts, const double* tg, const double* te) {
    double s = 0.0;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const double a = fma(Rg[i * 3 + 0], ts[0], fma(Rg[i * 3 + 1], ts[1], Rg[i * 3 + 2] * ts[2]));
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const double d = (a + tg[j]) - te[j];
            s += d * d;
        }
    }
    return sqrt(s);
}

// The projections of the estimate-posed points, once per row: est[row][2][n_max] = u, v (structure of arrays: coalesced both ways).
__global__ __launch_bounds__(SX_THREADS) void sym_est_kernel(const double* __restrict__ R_est, const double* __restrict__ t_est,
                                                             const double* __restrict__ Km, const int* __restrict__ labels,
                                                             const double* __restrict__ pts, const int* __restrict__ npts, int n_max, int C,
                                                             double* __restrict__ est) {
    const int row = blockIdx.y, j = blockIdx.x * SX_THREADS + threadIdx.x;
    const int c = labels[row];
    if (c < 0 || c >= C) return;
    if (j >= min(npts[c], n_max)) return;
    double R[9], K[9], t[3], P[12];
#pragma unroll
    for (int k = 0; k < 9; ++k) {
        R[k] = R_est[(size_t)row * 9 + k];
        K[k] = Km[(size_t)row * 9 + k];
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) t[k] = t_est[(size_t)row * 3 + k];
    make_proj(K, R, t, P);
    double u, v;
    project(P, load3(pts + ((size_t)c * n_max + j) * 3), u, v);
    double* o = est + (size_t)row * 2 * n_max + j;
    o[0] = u;
    o[(size_t)n_max] = v;
}

// Workgroup (slab of SY_SLAB symmetry transformations, row).  Per transformation the rotation error of its pose under the ground truth and the
// reference's te_sym (a few operations, the same in every thread) and the mean over the class's points of the image distance to the estimate's projection:
// two transformations per pass over the points (the second of an odd tail repeats the first: a minimum does not mind), per-thread sums reduced
// over the workgroup in a fixed order.  The slab's minima, taken in the order of the table, go to partial[row][slab][3].  Table rows beyond
// npts[c] and transformations beyond nsym[c] are never read.
__global__ __launch_bounds__(SX_THREADS) void sym_walk_kernel(const double* __restrict__ R_est, const double* __restrict__ t_est,
                                                              const double* __restrict__ R_gt, const double* __restrict__ t_gt,
                                                              const double* __restrict__ Km, const int* __restrict__ labels,
                                                              const double* __restrict__ pts, const int* __restrict__ npts, int n_max, int C,
                                                              const double* __restrict__ sym_R, const double* __restrict__ sym_t,
                                                              const int* __restrict__ nsym, int S_max, const double* __restrict__ est,
                                                              double* __restrict__ partial, int slabs) {
    __shared__ double red[4];
    const int row = blockIdx.y, slab = blockIdx.x, tid = threadIdx.x;
    const int c = labels[row];
    if (c < 0 || c >= C) return;
    const int n = min(npts[c], n_max), ns = min(max(nsym[c], 0), S_max);
    const int k0 = slab * SY_SLAB;
    if (k0 >= ns) return;   // uniform over the workgroup (the finish pass reads the slabs below ceil(ns / SY_SLAB) only)
    const int kend = min(k0 + SY_SLAB, ns);
    double Re[9], Rg[9], K[9], te[3], tg[3];
#pragma unroll
    for (int k = 0; k < 9; ++k) {
        Re[k] = R_est[(size_t)row * 9 + k];
        Rg[k] = R_gt[(size_t)row * 9 + k];
        K[k] = Km[(size_t)row * 9 + k];
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        te[k] = t_est[(size_t)row * 3 + k];
        tg[k] = t_gt[(size_t)row * 3 + k];
    }
    const double* P0 = pts + (size_t)c * n_max * 3;
    const double* E = est + (size_t)row * 2 * n_max;
    double best_re = INFINITY, best_te = INFINITY, best_pr = INFINITY;
    for (int k = k0; k < kend; k += 2) {
        const int ka = k, kb = min(k + 1, kend - 1);
        double Ra[9], ta[3], Pa[12], Rb[9], tb[3], Pb[12];
        sym_gt_pose(Rg, tg, sym_R + ((size_t)c * S_max + ka) * 9, sym_t + ((size_t)c * S_max + ka) * 3, Ra, ta);
        sym_gt_pose(Rg, tg, sym_R + ((size_t)c * S_max + kb) * 9, sym_t + ((size_t)c * S_max + kb) * 3, Rb, tb);
        make_proj(K, Ra, ta, Pa);
        make_proj(K, Rb, tb, Pb);
        best_re = nanmin(nanmin(best_re, re_deg(Re, Ra)), re_deg(Re, Rb));   // in the order of the table
        best_te = nanmin(nanmin(best_te, te_sym_as_run(Rg, sym_t + ((size_t)c * S_max + ka) * 3, tg, te)),
                         te_sym_as_run(Rg, sym_t + ((size_t)c * S_max + kb) * 3, tg, te));
        double s_a = 0.0, s_b = 0.0;
        for (int j = tid; j < n; j += SX_THREADS) {
            const V3 p = load3(P0 + (size_t)j * 3);
            const double eu = E[j], ev = E[(size_t)n_max + j];
            double u, v;
            project(Pa, p, u, v);
            double du = eu - u, dv = ev - v;
            s_a += sqrt(du * du + dv * dv);
            project(Pb, p, u, v);
            du = eu - u;
            dv = ev - v;
            s_b += sqrt(du * du + dv * dv);
        }
        s_a = block_sum_256_f64(s_a, red);
        s_b = block_sum_256_f64(s_b, red);
        best_pr = nanmin(nanmin(best_pr, s_a / (double)n), s_b / (double)n);
    }
    if (tid == 0) {
        double* o = partial + ((size_t)row * slabs + slab) * 3;
        o[0] = best_re;
        o[1] = best_te;
        o[2] = best_pr;
    }
}

// One thread per row: the slabs' minima in slab order.
__global__ __launch_bounds__(SX_THREADS) void sym_finish_kernel(const int* __restrict__ labels, const int* __restrict__ nsym, int S_max, int C,
                                                                int N, const double* __restrict__ partial, int slabs,
                                                                double* __restrict__ err) {
    const int i = blockIdx.x * SX_THREADS + threadIdx.x;
    if (i >= N) return;
    const int c = labels[i];
    double b[3] = {__builtin_nan(""), __builtin_nan(""), __builtin_nan("")};
    if (c >= 0 && c < C) {
        const int ns = min(max(nsym[c], 0), S_max);
        const int used = (ns + SY_SLAB - 1) / SY_SLAB;
        if (used > 0) b[0] = b[1] = b[2] = INFINITY;
        for (int s = 0; s < used; ++s) {
#pragma unroll
            for (int q = 0; q < 3; ++q) b[q] = nanmin(b[q], partial[((size_t)i * slabs + s) * 3 + q]);
        }
    }
#pragma unroll
    for (int q = 0; q < 3; ++q) err[(size_t)i * 3 + q] = b[q];
}

// ---- recall counts ----

// One workgroup per class: the strict-< decisions of its rows (pose_matching.py:68) counted in LDS, then added to the caller's running state by
// this workgroup alone (launches on one stream follow each other: no global atomics).  Lengths arrive in metres: the toolkit's "mm / 10" is
// "m * 100" here, its thresholds are centimetres.  The column order is the one gdrn_hip.h documents.
__global__ __launch_bounds__(SX_THREADS) void score_recall_kernel(const double* __restrict__ ad, const double* __restrict__ sym,
                                                                  const int* __restrict__ labels, int N, const double* __restrict__ diameter,
                                                                  const int* __restrict__ ad_is_adi, long long* __restrict__ hits,
                                                                  long long* __restrict__ seen) {
    __shared__ int cnt[NF + 1];
    const int c = blockIdx.x, tid = threadIdx.x;
    if (tid <= NF) cnt[tid] = 0;
    __syncthreads();
    const double d = diameter[c];
    const bool use_adi = ad_is_adi[c] != 0;
    for (int i = tid; i < N; i += SX_THREADS) {
        if (labels[i] != c) continue;
        const double add = ad[(size_t)i * 2 + 0], adi = ad[(size_t)i * 2 + 1];
        const double re = sym[(size_t)i * 3 + 0], te_cm = sym[(size_t)i * 3 + 1] * 100.0, pr = sym[(size_t)i * 3 + 2];
        const double cm[3] = {add * 100.0, adi * 100.0, (use_adi ? adi : add) * 100.0};   // AUC / ABS add, adi, ad
        const double rel[2] = {add / d, adi / d};                                           // eval_calc_scores.py:239-243
        const double th3[3] = {2.0, 5.0, 10.0}, thd[3] = {0.02, 0.05, 0.1};
#pragma unroll
        for (int q = 0; q < 3; ++q) {
            for (int k = 0; k < 10; ++k)
                if (cm[q] < (double)(k + 1)) atomicAdd(&cnt[q * 10 + k], 1);   // np.linspace(1, 10, 10)
            if (cm[q] < 2.0) atomicAdd(&cnt[30 + q], 1);
        }
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            if (rel[0] < thd[k]) atomicAdd(&cnt[33 + k], 1);
            if (rel[1] < thd[k]) atomicAdd(&cnt[36 + k], 1);
            if (re < th3[k]) atomicAdd(&cnt[39 + k], 1);
            if (te_cm < th3[k]) atomicAdd(&cnt[42 + k], 1);
            if (re < th3[k] && te_cm < th3[k]) atomicAdd(&cnt[45 + k], 1);
            if (pr < th3[k]) atomicAdd(&cnt[48 + k], 1);
        }
        atomicAdd(&cnt[NF], 1);
    }
    __syncthreads();
    if (tid < NF) hits[(size_t)c * NF + tid] += cnt[tid];
    if (tid == NF) seen[c] += cnt[NF];
}

}  // namespace

extern "C" long long gdrn_ad_errors_workspace_bytes(int N, int n_max) {
    if (N <= 0 || n_max <= 0) return GDRN_ERR_ARG;
    const long long slabs = ((long long)n_max + AD_SLAB - 1) / AD_SLAB;
    return (long long)N * 2 * slabs * (long long)sizeof(double);
}

extern "C" int gdrn_ad_errors(const double* R_est, const double* t_est, const double* R_gt, const double* t_gt, const int* labels,
                              const int* labels_host, int N, const double* pts, const int* npts, int n_max, int C, double* err, void* workspace,
                              void* stream) {
    if (!R_est || !t_est || !R_gt || !t_gt || !labels || !labels_host || !pts || !npts || !err || !workspace) return GDRN_ERR_ARG;
    if (N <= 0 || n_max <= 0 || C <= 0) return GDRN_ERR_ARG;
    if (!host_in_range(labels_host, N, C)) return GDRN_ERR_ARG;
    if (N > 65535 || n_max > 0x7fffffff - AD_SLAB) return GDRN_ERR_SHAPE;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const int slabs = cdiv(n_max, AD_SLAB);
    double* partial = reinterpret_cast<double*>(workspace);
    GDRN_LAUNCH(ad_points_kernel, dim3(slabs, N), dim3(SX_THREADS), 0, st, R_est, t_est, R_gt, t_gt, labels, pts, npts, n_max, C, partial, slabs);
    GDRN_CHECK_LAUNCH();
    GDRN_LAUNCH(ad_finish_kernel, dim3(cdiv(N, SX_THREADS)), dim3(SX_THREADS), 0, st, labels, npts, n_max, C, N, partial, slabs, err);
    GDRN_CHECK_LAUNCH();
    return GDRN_OK;
}

extern "C" long long gdrn_sym_errors_workspace_bytes(int N, int n_max, int S_max) {
    if (N <= 0 || n_max <= 0 || S_max <= 0) return GDRN_ERR_ARG;
    const long long slabs = ((long long)S_max + SY_SLAB - 1) / SY_SLAB;
    return (long long)N * (2LL * n_max + 3 * slabs) * (long long)sizeof(double);
}

extern "C" int gdrn_sym_errors(const double* R_est, const double* t_est, const double* R_gt, const double* t_gt, const double* K, const int* labels,
                               const int* labels_host, int N, const double* pts, const int* npts, int n_max, const double* sym_R,
                               const double* sym_t, const int* nsym, int S_max, int C, double* err, void* workspace, void* stream) {
    if (!R_est || !t_est || !R_gt || !t_gt || !K || !labels || !labels_host || !pts || !npts || !sym_R || !sym_t || !nsym || !err || !workspace)
        return GDRN_ERR_ARG;
    if (N <= 0 || n_max <= 0 || S_max <= 0 || C <= 0) return GDRN_ERR_ARG;
    if (!host_in_range(labels_host, N, C)) return GDRN_ERR_ARG;
    if (N > 65535 || S_max > 0x7fffffff - SY_SLAB || n_max > 0x7fffffff - SX_THREADS) return GDRN_ERR_SHAPE;
    const int slabs = cdiv(S_max, SY_SLAB);
    if (slabs > 65535) return GDRN_ERR_SHAPE;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    double* est = reinterpret_cast<double*>(workspace);
    double* partial = est + (size_t)N * 2 * n_max;
    GDRN_LAUNCH(sym_est_kernel, dim3(cdiv(n_max, SX_THREADS), N), dim3(SX_THREADS), 0, st, R_est, t_est, K, labels, pts, npts, n_max, C, est);
    GDRN_CHECK_LAUNCH();
    GDRN_LAUNCH(sym_walk_kernel, dim3(slabs, N), dim3(SX_THREADS), 0, st, R_est, t_est, R_gt, t_gt, K, labels, pts, npts, n_max, C, sym_R, sym_t,
                nsym, S_max, est, partial, slabs);
    GDRN_CHECK_LAUNCH();
    GDRN_LAUNCH(sym_finish_kernel, dim3(cdiv(N, SX_THREADS)), dim3(SX_THREADS), 0, st, labels, nsym, S_max, C, N, partial, slabs, err);
    GDRN_CHECK_LAUNCH();
    return GDRN_OK;
}

extern "C" int gdrn_score_recall_accumulate(const double* ad_err, const double* sym_err, const int* labels, const int* labels_host, int N,
                                            const double* diameter, const int* ad_is_adi, int C, long long* hits, long long* seen, void* stream) {
    if (!ad_err || !sym_err || !labels || !labels_host || !diameter || !ad_is_adi || !hits || !seen || N <= 0 || C <= 0) return GDRN_ERR_ARG;
    if (!host_in_range(labels_host, N, C)) return GDRN_ERR_ARG;
    GDRN_LAUNCH(score_recall_kernel, dim3(C), dim3(SX_THREADS), 0, reinterpret_cast<hipStream_t>(stream), ad_err, sym_err, labels, N, diameter,
                ad_is_adi, hits, seen);
    GDRN_CHECK_LAUNCH();
    return GDRN_OK;
}
