// The three BOP pose errors and their recall counts for gfx950: what the reference gets by writing a CSV and running the BOP toolkit's scripts
// on the host (core/gdrn_modeling/gdrn_evaluator.py:437-514 -> lib/pysixd/scripts/eval_pose_results_more.py -> eval_calc_errors.py:344-372,
// eval_calc_scores.py) --
//   vsd     lib/pysixd/pose_error.py:84-126 with visibility.py:27-36,72-73 ("bop19") and misc.depth_im_to_dist_im_fast (misc.py:565-588), on depth
//           maps that are already rendered (gdrn_render_depth)                                                    -> gdrn_vsd
//   mssd    pose_error.py:131-153, mspd :156-179, the minimum over the class's symmetry transformations           -> gdrn_mssd_mspd
//   the "correct" decisions of eval_calc_scores.py:239-250 under the ten thresholds of eval_pose_results_more.py:58-63, counted per class
//                                                                                                                 -> gdrn_bop_recall_accumulate
// -- for a whole batch of estimates per call.  Every decision and every output is fp64 like the reference's numpy, except the visibility
// difference of VSD, which the reference takes on fp32 casts and so does this.  No floating-point atomics: counts are integers, fp64 sums are
// per-workgroup partials added in a fixed order, minima are finished in slab order; repeated calls give the same bits.
//
// Floating-point contraction is OFF for this file: a*a + b*b + c*c is three products and two sums, as numpy evaluates it, and every fused
// operation is an explicit fma().  (No 16-bit code: both library builds compile the same thing.)
#include "common.h"
#include "geom64.h"
#include "points64.h"
#include "dist64.h"
#include "../../include/gdrn_hip.h"

#pragma clang fp contract(off)

namespace {

constexpr int BM_THREADS = 256;
constexpr int BM_WAVES = BM_THREADS / 64;
constexpr int VSD_PPT = 8;                           // pixels per thread
constexpr int VSD_CHUNK = BM_THREADS * VSD_PPT;      // pixels per workgroup
constexpr int VSD_MAX_T = GDRN_VSD_MAX_TAUS;
constexpr int MS_SLAB = 8;                           // symmetry transformations per workgroup
constexpr int NTH = GDRN_BOP_NTH;

// (misc.project_pts as make_proj / project, the pose of a symmetry under the ground truth and the NaN-keeping nanmax / nanmin: points64.h)

__device__ __forceinline__ double wave_nanmax(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = nanmax(v, __shfl_xor(v, o, 64));
    return v;
}

// ---- VSD ----

__global__ __launch_bounds__(BM_THREADS) void vsd_clear_kernel(long long* __restrict__ counts, long long n) {
    const long long i = (long long)blockIdx.x * BM_THREADS + threadIdx.x;
    if (i < n) counts[i] = 0;
}

// (misc.depth_im_to_dist_im_fast per pixel: dist_of, dist64.h)

// Workgroup (chunk of VSD_CHUNK pixels, row).  Per pixel the two visibility masks; union, union - intersection and the per-tau step costs are
// counted per wave by ballot / popcount, gathered in LDS and added to the row's counters with one integer atomic per workgroup and counter.
// The truncated-linear costs (cost_type tlinear) are summed per wave in an xor tree, per workgroup in wave order, and written to
// partial[row][chunk][t]: the finish pass adds the chunks in chunk order.  A pixel whose two model depths are both 0 is in neither mask.
__global__ __launch_bounds__(BM_THREADS) void vsd_pixels_kernel(const float* __restrict__ depth_est, const float* __restrict__ depth_gt,
                                                                const float* __restrict__ depth_test, const int* __restrict__ frame, int F,
                                                                const double* __restrict__ Km, const double* __restrict__ diameter, int HW, int W,
                                                                float delta, const double* __restrict__ taus, int T, int tlinear, int normalized,
                                                                unsigned long long* __restrict__ counts, double* __restrict__ partial, int chunks) {
    __shared__ int cnt[2 + VSD_MAX_T];
    __shared__ double wsum[BM_WAVES][VSD_MAX_T];
    __shared__ double s_tau[VSD_MAX_T];
    const int row = blockIdx.y, chunk = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int f = frame[row];
    if (f < 0 || f >= F) return;   // (the host side of the entry point refuses such a frame before the launch)
    if (tid < 2 + T) cnt[tid] = 0;
    if (tid < T) {
        s_tau[tid] = taus[tid];
#pragma unroll
        for (int w = 0; w < BM_WAVES; ++w) wsum[w][tid] = 0.0;
    }
    __syncthreads();
    const double* K = Km + (size_t)row * 9;
    const double fx = K[0], cx = K[2], fy = K[4], cy = K[5];
    const double diam = diameter[row];
    const float* de = depth_est + (size_t)row * HW;
    const float* dg = depth_gt + (size_t)row * HW;
    const float* dt = depth_test + (size_t)f * HW;
    for (int u = 0; u < VSD_PPT; ++u) {
        const int p = chunk * VSD_CHUNK + u * BM_THREADS + tid;
        float ze = 0.f, zg = 0.f;
        if (p < HW) {
            ze = de[p];
            zg = dg[p];
        }
        const bool any = ze != 0.f || zg != 0.f;
        if (__ballot(any) == 0ull) continue;   // uniform over the wave
        bool vis_g = false, vis_e = false;
        double dist_g = 0.0, dist_e = 0.0;
        if (any) {
            const int y = p / W, x = p - y * W;
            const double X = ((double)x - cx) / fx, Y = ((double)y - cy) / fy;
            const double dist_t = dist_of(X, Y, dt[p]);
            dist_g = dist_of(X, Y, zg);
            dist_e = dist_of(X, Y, ze);
            const float ft = (float)dist_t;
            const float diff_g = (float)dist_g - ft, diff_e = (float)dist_e - ft;   // visibility.py:35: on the fp32 casts
            const bool hole = dist_t == 0.0;
            vis_g = (diff_g <= delta || hole) && dist_g > 0.0;
            vis_e = ((diff_e <= delta || hole) && dist_e > 0.0) || (vis_g && dist_e > 0.0);
        }
        const bool inter = vis_g && vis_e;
        const unsigned long long bu = __ballot(vis_g || vis_e), bi = __ballot(inter);
        if (lane == 0 && bu != 0ull) {
            atomicAdd(&cnt[0], __popcll(bu));
            atomicAdd(&cnt[1], __popcll(bu) - __popcll(bi));
        }
        if (bi == 0ull) continue;
        double dists = fabs(dist_g - dist_e);
        if (normalized) dists = dists / diam;
        for (int t = 0; t < T; ++t) {
            const double tau = s_tau[t];
            const unsigned long long bs = __ballot(inter && dists >= tau);
            if (lane == 0 && bs != 0ull) atomicAdd(&cnt[2 + t], __popcll(bs));
            if (tlinear) {
                double c = 0.0;
                if (inter) {
                    c = dists / tau;
                    c = c > 1.0 ? 1.0 : c;
                }
                c = wave_sum_f64(c);
                if (lane == 0) wsum[wave][t] += c;   // this wave's slot only
            }
        }
    }
    __syncthreads();
    if (tid < 2 + T && cnt[tid] != 0) atomicAdd(counts + (size_t)row * (2 + T) + tid, (unsigned long long)cnt[tid]);
    if (tlinear && tid < T) partial[((size_t)row * chunks + chunk) * T + tid] = (wsum[0][tid] + wsum[1][tid]) + (wsum[2][tid] + wsum[3][tid]);
}

// One thread per row: err = (sum of costs + (union - intersection)) / union, 1 when the union is empty.
__global__ __launch_bounds__(BM_THREADS) void vsd_finish_kernel(const int* __restrict__ frame, int F, int N, int T, int tlinear,
                                                                const long long* __restrict__ counts, const double* __restrict__ partial,
                                                                int chunks, double* __restrict__ err) {
    const int i = blockIdx.x * BM_THREADS + threadIdx.x;
    if (i >= N) return;
    double* e = err + (size_t)i * T;
    if (frame[i] < 0 || frame[i] >= F) {
        for (int t = 0; t < T; ++t) e[t] = __builtin_nan("");
        return;
    }
    const long long* c = counts + (size_t)i * (2 + T);
    const long long uni = c[0], comp = c[1];
    for (int t = 0; t < T; ++t) {
        if (uni == 0) {
            e[t] = 1.0;
        } else if (!tlinear) {
            e[t] = (double)(c[2 + t] + comp) / (double)uni;
        } else {
            double s = 0.0;
            for (int k = 0; k < chunks; ++k) s += partial[((size_t)i * chunks + k) * T + t];
            e[t] = (s + (double)comp) / (double)uni;
        }
    }
}

// ---- MSSD / MSPD ----

// The estimate-posed points and their projections, once per row: est[row][5][n_max] = x, y, z, u, v (structure of arrays: coalesced both ways).
__global__ __launch_bounds__(BM_THREADS) void ms_est_kernel(const double* __restrict__ R_est, const double* __restrict__ t_est,
                                                            const double* __restrict__ Km, const int* __restrict__ labels,
                                                            const double* __restrict__ pts, const int* __restrict__ npts, int n_max, int C,
                                                            double* __restrict__ est) {
    const int row = blockIdx.y, j = blockIdx.x * BM_THREADS + threadIdx.x;
    const int c = labels[row];
    if (c < 0 || c >= C) return;   // (the host side refuses such a label before the launch: never index a table with it)
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
    const V3 p = load3(pts + ((size_t)c * n_max + j) * 3);
    const V3 e = xform(R, t, p);
    double u, v;
    project(P, p, u, v);
    double* o = est + (size_t)row * 5 * n_max + j;
    o[0] = e.x;
    o[(size_t)n_max] = e.y;
    o[(size_t)2 * n_max] = e.z;
    o[(size_t)3 * n_max] = u;
    o[(size_t)4 * n_max] = v;
}

// the pose of symmetry k of the class under the ground truth: R_gt S_k, R_gt t_k + t_gt (pose_error.py:149-150), and its projection matrix
__device__ __forceinline__ void sym_pose(const double* Rg, const double* tg, const double* K, const double* S, const double* ts, double* R, double* t,
                                         double* P) {
    sym_gt_pose(Rg, tg, S, ts, R, t);
    make_proj(K, R, t, P);
}

// Workgroup (slab of MS_SLAB symmetry transformations, row).  Two transformations per pass over the class's points (the second of an odd tail
// repeats the first: a minimum does not mind): per point the squared distance in 3D and in the image to the estimate's, a running maximum per
// thread, reduced over the workgroup; the slab's minimum over its transformations goes to partial[row][slab][2] (squared).  Table rows beyond
// npts[c] and transformations beyond nsym[c] are never read.
__global__ __launch_bounds__(BM_THREADS) void ms_sym_kernel(const double* __restrict__ R_gt, const double* __restrict__ t_gt,
                                                            const double* __restrict__ Km, const int* __restrict__ labels,
                                                            const double* __restrict__ pts, const int* __restrict__ npts, int n_max, int C,
                                                            const double* __restrict__ sym_R, const double* __restrict__ sym_t,
                                                            const int* __restrict__ nsym, int S_max, const double* __restrict__ est,
                                                            double* __restrict__ partial, int slabs) {
    __shared__ double red[BM_WAVES][4];
    const int row = blockIdx.y, slab = blockIdx.x, tid = threadIdx.x;
    const int c = labels[row];
    if (c < 0 || c >= C) return;
    const int n = min(npts[c], n_max), ns = min(max(nsym[c], 0), S_max);
    const int k0 = slab * MS_SLAB;
    if (k0 >= ns) return;   // uniform over the workgroup (the finish pass reads the slabs below ceil(ns / MS_SLAB) only)
    const int kend = min(k0 + MS_SLAB, ns);
    double Rg[9], K[9], tg[3];
#pragma unroll
    for (int k = 0; k < 9; ++k) {
        Rg[k] = R_gt[(size_t)row * 9 + k];
        K[k] = Km[(size_t)row * 9 + k];
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) tg[k] = t_gt[(size_t)row * 3 + k];
    const double* P0 = pts + (size_t)c * n_max * 3;
    const double* E = est + (size_t)row * 5 * n_max;
    double best3 = INFINITY, best2 = INFINITY;
    for (int k = k0; k < kend; k += 2) {
        const int ka = k, kb = min(k + 1, kend - 1);
        double Ra[9], ta[3], Pa[12], Rb[9], tb[3], Pb[12];
        sym_pose(Rg, tg, K, sym_R + ((size_t)c * S_max + ka) * 9, sym_t + ((size_t)c * S_max + ka) * 3, Ra, ta, Pa);
        sym_pose(Rg, tg, K, sym_R + ((size_t)c * S_max + kb) * 9, sym_t + ((size_t)c * S_max + kb) * 3, Rb, tb, Pb);
        double m[4] = {0.0, 0.0, 0.0, 0.0};   // max squared distance: a 3D, a image, b 3D, b image
        for (int j = tid; j < n; j += BM_THREADS) {
            const V3 p = {P0[(size_t)j * 3 + 0], P0[(size_t)j * 3 + 1], P0[(size_t)j * 3 + 2]};
            const double ex = E[j], ey = E[(size_t)n_max + j], ez = E[(size_t)2 * n_max + j], eu = E[(size_t)3 * n_max + j],
                         ev = E[(size_t)4 * n_max + j];
            double u, v;
            const V3 ga = xform(Ra, ta, p);
            double dx = ex - ga.x, dy = ey - ga.y, dz = ez - ga.z;
            m[0] = nanmax(m[0], (dx * dx + dy * dy) + dz * dz);
            project(Pa, p, u, v);
            dx = eu - u;
            dy = ev - v;
            m[1] = nanmax(m[1], dx * dx + dy * dy);
            const V3 gb = xform(Rb, tb, p);
            dx = ex - gb.x;
            dy = ey - gb.y;
            dz = ez - gb.z;
            m[2] = nanmax(m[2], (dx * dx + dy * dy) + dz * dz);
            project(Pb, p, u, v);
            dx = eu - u;
            dy = ev - v;
            m[3] = nanmax(m[3], dx * dx + dy * dy);
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) m[q] = wave_nanmax(m[q]);
        __syncthreads();   // the previous pass has been read
        if ((tid & 63) == 0) {
#pragma unroll
            for (int q = 0; q < 4; ++q) red[tid >> 6][q] = m[q];
        }
        __syncthreads();
#pragma unroll
        for (int q = 0; q < 4; ++q) m[q] = nanmax(nanmax(red[0][q], red[1][q]), nanmax(red[2][q], red[3][q]));
        best3 = nanmin(nanmin(best3, m[0]), m[2]);   // in the order of the table
        best2 = nanmin(nanmin(best2, m[1]), m[3]);
    }
    if (tid == 0) {
        double* o = partial + ((size_t)row * slabs + slab) * 2;
        o[0] = best3;
        o[1] = best2;
    }
}

// One thread per row: the slabs' minima in slab order, one sqrt each.
__global__ __launch_bounds__(BM_THREADS) void ms_finish_kernel(const int* __restrict__ labels, const int* __restrict__ nsym, int S_max, int C, int N,
                                                               const double* __restrict__ partial, int slabs, double* __restrict__ err) {
    const int i = blockIdx.x * BM_THREADS + threadIdx.x;
    if (i >= N) return;
    const int c = labels[i];
    double b3 = __builtin_nan(""), b2 = __builtin_nan("");
    if (c >= 0 && c < C) {
        const int ns = min(max(nsym[c], 0), S_max);
        const int used = (ns + MS_SLAB - 1) / MS_SLAB;
        if (used > 0) {
            b3 = INFINITY;
            b2 = INFINITY;
        }
        for (int s = 0; s < used; ++s) {
            b3 = nanmin(b3, partial[((size_t)i * slabs + s) * 2 + 0]);
            b2 = nanmin(b2, partial[((size_t)i * slabs + s) * 2 + 1]);
        }
    }
    err[(size_t)i * 2 + 0] = sqrt(b3);
    err[(size_t)i * 2 + 1] = sqrt(b2);
}

// ---- recall counts ----

// One workgroup per class: the strict-< decisions of its rows counted in LDS, then added to the caller's running state by this workgroup alone
// (launches on one stream follow each other: no global atomics).
__global__ __launch_bounds__(BM_THREADS) void bop_recall_kernel(const double* __restrict__ vsd, int T, const double* __restrict__ ms,
                                                                const int* __restrict__ labels, int N, const double* __restrict__ diameter,
                                                                double im_factor, const double* __restrict__ ths_vsd,
                                                                const double* __restrict__ ths_mssd, const double* __restrict__ ths_mspd,
                                                                long long* __restrict__ hits_vsd, long long* __restrict__ hits_mssd,
                                                                long long* __restrict__ hits_mspd, long long* __restrict__ seen) {
    __shared__ int cnt[VSD_MAX_T * NTH + 2 * NTH + 1];
    __shared__ double th[3][NTH];
    const int c = blockIdx.x, tid = threadIdx.x;
    const int nv = T * NTH, total = nv + 2 * NTH + 1;
    for (int k = tid; k < total; k += BM_THREADS) cnt[k] = 0;
    if (tid < NTH) {
        th[0][tid] = ths_vsd[tid];
        th[1][tid] = ths_mssd[tid];
        th[2][tid] = ths_mspd[tid];
    }
    __syncthreads();
    const double d = diameter[c];
    for (int i = tid; i < N; i += BM_THREADS) {
        if (labels[i] != c) continue;
        for (int t = 0; t < T; ++t) {
            const double e = vsd[(size_t)i * T + t];
#pragma unroll
            for (int k = 0; k < NTH; ++k)
                if (e < th[0][k]) atomicAdd(&cnt[t * NTH + k], 1);
        }
        const double e3 = ms[(size_t)i * 2 + 0] / d, e2 = im_factor * ms[(size_t)i * 2 + 1];   // eval_calc_scores.py:243,250
#pragma unroll
        for (int k = 0; k < NTH; ++k) {
            if (e3 < th[1][k]) atomicAdd(&cnt[nv + k], 1);
            if (e2 < th[2][k]) atomicAdd(&cnt[nv + NTH + k], 1);
        }
        atomicAdd(&cnt[nv + 2 * NTH], 1);
    }
    __syncthreads();
    for (int k = tid; k < total; k += BM_THREADS) {
        const int v = cnt[k];
        if (k < nv) hits_vsd[(size_t)c * nv + k] += v;
        else if (k < nv + NTH) hits_mssd[(size_t)c * NTH + (k - nv)] += v;
        else if (k < nv + 2 * NTH) hits_mspd[(size_t)c * NTH + (k - nv - NTH)] += v;
        else seen[c] += v;
    }
}

long long vsd_chunks(int H, int W) { return ((long long)H * W + VSD_CHUNK - 1) / VSD_CHUNK; }

bool vsd_shape_ok(int N, int H, int W, int T) {
    return N > 0 && H > 0 && W > 0 && T > 0;
}

// what the launches can index: H * W in an int with room for a chunk, the chunk count in a grid dimension, rows in grid.y
bool vsd_shape_fits(int N, int H, int W, int T) {
    return (long long)H * W <= 0x7fffffffLL - VSD_CHUNK && N <= 65535 && T <= VSD_MAX_T;
}

}  // namespace

extern "C" long long gdrn_vsd_workspace_bytes(int N, int H, int W, int T) {
    if (!vsd_shape_ok(N, H, W, T)) return GDRN_ERR_ARG;
    if (!vsd_shape_fits(N, H, W, T)) return GDRN_ERR_SHAPE;
    return (long long)N * vsd_chunks(H, W) * T * (long long)sizeof(double);
}

extern "C" int gdrn_vsd(const float* depth_est, const float* depth_gt, const float* depth_test, const int* frame, const int* frame_host, int F,
                        const double* K, const double* diameter, int N, int H, int W, double delta, const double* taus, int T, int cost_type,
                        int normalized_by_diameter, double* err, long long* counts, void* workspace, void* stream) {
    if (!depth_est || !depth_gt || !depth_test || !frame || !frame_host || !K || !diameter || !taus || !err || !counts || !workspace) return GDRN_ERR_ARG;
    if (!vsd_shape_ok(N, H, W, T) || F <= 0 || (cost_type != GDRN_VSD_STEP && cost_type != GDRN_VSD_TLINEAR)) return GDRN_ERR_ARG;
    if (!host_in_range(frame_host, N, F)) return GDRN_ERR_ARG;
    if (!vsd_shape_fits(N, H, W, T)) return GDRN_ERR_SHAPE;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const int chunks = (int)vsd_chunks(H, W);
    const long long nc = (long long)N * (2 + T);
    const int tlinear = cost_type == GDRN_VSD_TLINEAR;
    GDRN_LAUNCH(vsd_clear_kernel, dim3((unsigned)((nc + BM_THREADS - 1) / BM_THREADS)), dim3(BM_THREADS), 0, st, counts, nc);
    GDRN_CHECK_LAUNCH();
    GDRN_LAUNCH(vsd_pixels_kernel, dim3(chunks, N), dim3(BM_THREADS), 0, st, depth_est, depth_gt, depth_test, frame, F, K, diameter, H * W, W,
                (float)delta, taus, T, tlinear, normalized_by_diameter ? 1 : 0, reinterpret_cast<unsigned long long*>(counts),
                reinterpret_cast<double*>(workspace), chunks);
    GDRN_CHECK_LAUNCH();
    GDRN_LAUNCH(vsd_finish_kernel, dim3(cdiv(N, BM_THREADS)), dim3(BM_THREADS), 0, st, frame, F, N, T, tlinear, counts,
                reinterpret_cast<const double*>(workspace), chunks, err);
    GDRN_CHECK_LAUNCH();
    return GDRN_OK;
}

extern "C" long long gdrn_mssd_mspd_workspace_bytes(int N, int n_max, int S_max) {
    if (N <= 0 || n_max <= 0 || S_max <= 0) return GDRN_ERR_ARG;
    const long long slabs = (S_max + MS_SLAB - 1) / MS_SLAB;
    return (long long)N * (5LL * n_max + 2 * slabs) * (long long)sizeof(double);
}

extern "C" int gdrn_mssd_mspd(const double* R_est, const double* t_est, const double* R_gt, const double* t_gt, const double* K, const int* labels,
                              const int* labels_host, int N, const double* pts, const int* npts, int n_max, const double* sym_R,
                              const double* sym_t, const int* nsym, int S_max, int C, double* err, void* workspace, void* stream) {
    if (!R_est || !t_est || !R_gt || !t_gt || !K || !labels || !labels_host || !pts || !npts || !sym_R || !sym_t || !nsym || !err || !workspace)
        return GDRN_ERR_ARG;
    if (N <= 0 || n_max <= 0 || S_max <= 0 || C <= 0) return GDRN_ERR_ARG;
    if (!host_in_range(labels_host, N, C)) return GDRN_ERR_ARG;
    const int slabs = cdiv(S_max, MS_SLAB);
    if (N > 65535 || slabs > 65535 || cdiv(n_max, BM_THREADS) > 0x7fffffff / 2) return GDRN_ERR_SHAPE;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    double* est = reinterpret_cast<double*>(workspace);
    double* partial = est + (size_t)N * 5 * n_max;
    GDRN_LAUNCH(ms_est_kernel, dim3(cdiv(n_max, BM_THREADS), N), dim3(BM_THREADS), 0, st, R_est, t_est, K, labels, pts, npts, n_max, C, est);
    GDRN_CHECK_LAUNCH();
    GDRN_LAUNCH(ms_sym_kernel, dim3(slabs, N), dim3(BM_THREADS), 0, st, R_gt, t_gt, K, labels, pts, npts, n_max, C, sym_R, sym_t, nsym, S_max, est,
                partial, slabs);
    GDRN_CHECK_LAUNCH();
    GDRN_LAUNCH(ms_finish_kernel, dim3(cdiv(N, BM_THREADS)), dim3(BM_THREADS), 0, st, labels, nsym, S_max, C, N, partial, slabs, err);
    GDRN_CHECK_LAUNCH();
    return GDRN_OK;
}

extern "C" int gdrn_bop_recall_accumulate(const double* vsd_err, int T, const double* mssd_mspd_err, const int* labels, const int* labels_host,
                                          int N, const double* diameter, int C, double im_width, const double* ths_vsd, const double* ths_mssd,
                                          const double* ths_mspd, long long* hits_vsd, long long* hits_mssd, long long* hits_mspd,
                                          long long* seen, void* stream) {
    if (!vsd_err || !mssd_mspd_err || !labels || !labels_host || !diameter || !ths_vsd || !ths_mssd || !ths_mspd || !hits_vsd || !hits_mssd ||
        !hits_mspd || !seen)
        return GDRN_ERR_ARG;
    if (N <= 0 || C <= 0 || T <= 0 || !(im_width > 0.0)) return GDRN_ERR_ARG;
    if (!host_in_range(labels_host, N, C)) return GDRN_ERR_ARG;
    if (T > VSD_MAX_T) return GDRN_ERR_SHAPE;
    GDRN_LAUNCH(bop_recall_kernel, dim3(C), dim3(BM_THREADS), 0, reinterpret_cast<hipStream_t>(stream), vsd_err, T, mssd_mspd_err, labels, N,
                diameter, 640.0 / im_width, ths_vsd, ths_mssd, ths_mspd, hits_vsd, hits_mssd, hits_mspd, seen);
    GDRN_CHECK_LAUNCH();
    return GDRN_OK;
}
