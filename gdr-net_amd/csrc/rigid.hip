// Pose from depth and object-coordinate maps on the device for gfx950: batched 3D-3D RANSAC, the RGB-D counterpart of pnp.hip.  The network predicts
// a metric model point for every pixel of the RoI (gdrn_correspondences extracts them); with a depth frame each correspondence also has a metric
// camera point, and the pose follows in closed form (rigid_solve.h) inside a RANSAC: no render, no iteration.  The reference is RGB-only
// (WITH_DEPTH = False) and has no counterpart; results are pinned to geometry and to an fp64 host restatement (tests/rigid_host.py).
// One workgroup of 256 threads per RoI, no host loop, nothing read back; every pose computation is fp64.
//   rigid_backproject_kernel  nearest-pixel depth lookup of every correspondence, the camera point on the ray of the correspondence's own (u, v), the
//                             valid rows compacted to the front in their input order (ballot + prefix scan: no atomics), NaN behind them.
//   rigid_ransac_kernel       `iters` hypotheses per RoI in chunks of 256: 3 distinct samples from the counter-based hash of ransac_draw.h, the
//                             closed form on them; all hypotheses scored against all pairs staged through LDS tiles (every load of a tile in
//                             flight before its first LDS write, four pairs scored at a time: one wave per SIMD has nothing else to hide
//                             latency behind), integer inlier counts; highest count wins, ties to the lowest index.
//   rigid_refine_kernel       mode 0: inliers of the winner, closed form on them, inliers re-selected, closed form once more, and the mask / count /
//                             rms of the pose that is returned.  mode 1: the closed form over all rows, no gate.
// Sums are reduced in a fixed order (wave xor tree, then the four waves through LDS): no floating-point atomics, the same call gives the same bits.
// (The file has no 16-bit code: both library builds compile the same thing.)
#include "common.h"
#include "geom64.h"
#include "ransac_draw.h"
#include "rigid_solve.h"
#include "../../include/gdrn_hip.h"

namespace {

constexpr int RIGID_THREADS = 256;
constexpr int RIGID_HYP = 256;      // hypotheses per pass over the points ([R | t] each: 24 KB of LDS)
constexpr int RIGID_TILE = 512;     // pairs per LDS tile (camera + model point, fp64: 24 KB)
constexpr int RIGID_STAGE = RIGID_TILE * 3 / RIGID_THREADS;   // doubles of a tile each thread stages, per array
constexpr int RIGID_WIN = 16;       // doubles per RoI in the workspace: R (9), t (3), the winner's count, padding
constexpr int RIGID_MIN = 3;        // pairs of a minimal sample, and the fewest inliers a pose may rest on
constexpr int RIGID_SUMS = 9;       // the widest block sum: the 9 entries of the cross-covariance

// squared distance [m^2] of the posed model point from its camera point (NaN stays NaN: every comparison with it is false)
__device__ __forceinline__ double rigid_err2(const double* R, const double* t, V3 m, V3 c) {
    const V3 p = xform(R, t, m);
    const double dx = p.x - c.x, dy = p.y - c.y, dz = p.z - c.z;
    return fma(dx, dx, fma(dy, dy, dz * dz));
}

// inverse of a general 3x3 by cofactors; false for a singular or non-finite one
__device__ __forceinline__ bool rigid_inv3(const double* K, double* Ki) {
    const double c00 = K[4] * K[8] - K[5] * K[7], c01 = K[5] * K[6] - K[3] * K[8], c02 = K[3] * K[7] - K[4] * K[6];
    const double det = K[0] * c00 + K[1] * c01 + K[2] * c02;
    const double s = 1.0 / det;
    Ki[0] = c00 * s;
    Ki[1] = (K[2] * K[7] - K[1] * K[8]) * s;
    Ki[2] = (K[1] * K[5] - K[2] * K[4]) * s;
    Ki[3] = c01 * s;
    Ki[4] = (K[0] * K[8] - K[2] * K[6]) * s;
    Ki[5] = (K[2] * K[3] - K[0] * K[5]) * s;
    Ki[6] = c02 * s;
    Ki[7] = (K[1] * K[6] - K[0] * K[7]) * s;
    Ki[8] = (K[0] * K[4] - K[1] * K[3]) * s;
    double chk = 0.0;
#pragma unroll
    for (int k = 0; k < 9; ++k) chk += Ki[k];
    return det != 0.0 && rigid_finite(chk);
}

// One workgroup per RoI.  Passes of 256 rows: every thread decides its row, a ballot per wave and the waves' totals through LDS give each valid row
// its place behind the valid rows before it -- the input order is kept.
__global__ __launch_bounds__(RIGID_THREADS) void rigid_backproject_kernel(const float* __restrict__ img_pts, const float* __restrict__ model_pts,
                                                                          const int* __restrict__ counts, const float* __restrict__ depth,
                                                                          const int* __restrict__ frame, int F, int H, int W,
                                                                          const double* __restrict__ Kmat, int stride, double* __restrict__ cam,
                                                                          double* __restrict__ mod, int* __restrict__ counts_out) {
    __shared__ int wave_total[4];
    const int n = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int count = min(max(counts[n], 0), stride);
    const int fr = frame[n];
    const float* img = img_pts + (size_t)n * stride * 2;
    const float* mdl = model_pts + (size_t)n * stride * 3;
    double* cam_o = cam + (size_t)n * stride * 3;
    double* mod_o = mod + (size_t)n * stride * 3;
    double K[9], Ki[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) K[k] = Kmat[(size_t)n * 9 + k];
    const bool usable = rigid_inv3(K, Ki) && fr >= 0 && fr < F;   // (the host checked the frame: a second fence in front of the depth read)
    const float* dmap = depth + (size_t)(usable ? fr : 0) * H * W;
    int base = 0;   // valid rows before this pass (uniform over the workgroup)
    for (int j0 = 0; j0 < count; j0 += RIGID_THREADS) {
        const int j = j0 + tid;
        bool valid = false;
        double P[3] = {0.0, 0.0, 0.0}, X[3] = {0.0, 0.0, 0.0};
        if (usable && j < count) {
            const double u = (double)img[(size_t)j * 2], v = (double)img[(size_t)j * 2 + 1];
#pragma unroll
            for (int k = 0; k < 3; ++k) X[k] = (double)mdl[(size_t)j * 3 + k];
            const double fx = floor(u + 0.5), fy = floor(v + 0.5);   // the nearest pixel; NaN fails the range test
            if (rigid_finite(u + v + X[0] + X[1] + X[2]) && fx >= 0.0 && fx < (double)W && fy >= 0.0 && fy < (double)H) {
                const float df = dmap[(size_t)(int)fy * W + (int)fx];
                const double d = (double)df;
                if (rigid_finite(d) && d > 0.0) {
                    const double rx = fma(Ki[0], u, fma(Ki[1], v, Ki[2])), ry = fma(Ki[3], u, fma(Ki[4], v, Ki[5]));
                    const double rz = fma(Ki[6], u, fma(Ki[7], v, Ki[8]));
                    const double s = d / rz;   // the point of the ray whose z is d
                    P[0] = rx * s, P[1] = ry * s, P[2] = d;
                    valid = rigid_finite(P[0] + P[1]);
                }
            }
        }
        const unsigned long long ballot = __ballot(valid);
        const int before = __popcll(ballot & ((1ull << lane) - 1ull));
        __syncthreads();   // the previous pass's totals have been read
        if (lane == 0) wave_total[wave] = __popcll(ballot);
        __syncthreads();
        int off = base;
        for (int w = 0; w < wave; ++w) off += wave_total[w];
        if (valid) {
            const size_t o = (size_t)(off + before) * 3;
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                cam_o[o + k] = P[k];
                mod_o[o + k] = X[k];
            }
        }
        base += wave_total[0] + wave_total[1] + wave_total[2] + wave_total[3];
    }
    const double nan = __builtin_nan("");
    for (int i = base * 3 + tid; i < stride * 3; i += RIGID_THREADS) {
        cam_o[i] = nan;
        mod_o[i] = nan;
    }
    if (tid == 0) counts_out[n] = base;
}

// the workgroup's LDS of the refinement kernel
struct RigidLds {
    double red[4][RIGID_SUMS];
    double sum[RIGID_SUMS];   // block totals of the last pass
    double cur[12];           // the pose: R (9), t (3)
    int count;
    int good;
};

// block-wide sums of acc[0..K-1] into L.sum, fixed order; ends with a barrier
template <int K>
__device__ __forceinline__ void rigid_block_sum(const double* acc, RigidLds& L) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const double s = wave_sum_f64(acc[k]);
        if (lane == 0) L.red[wave][k] = s;
    }
    __syncthreads();
    if (threadIdx.x < K) L.sum[threadIdx.x] = (L.red[0][threadIdx.x] + L.red[1][threadIdx.x]) + (L.red[2][threadIdx.x] + L.red[3][threadIdx.x]);
    __syncthreads();
}

// the closed form over the pairs with mask[i] != 0 (mask == nullptr: all `count` pairs): centroids, then the cross-covariance about them, then
// thread 0 solves.  The pose is left in L.cur; false for fewer than 3 pairs, a degenerate set or a non-finite result.  Called by the whole workgroup.
__device__ bool rigid_fit_block(const double* __restrict__ cam, const double* __restrict__ mod, const unsigned char* mask, int count, RigidLds& L) {
    const int tid = threadIdx.x;
    double acc[RIGID_SUMS];
#pragma unroll
    for (int k = 0; k < RIGID_SUMS; ++k) acc[k] = 0.0;
#pragma unroll 4
    for (int i = tid; i < count; i += RIGID_THREADS) {   // (no branch around the loads: a row that is left out adds exact zeros)
        const bool in = mask == nullptr || mask[i] != 0;
        const V3 m = load3(mod + (size_t)i * 3), c = load3(cam + (size_t)i * 3);
        acc[0] += in ? m.x : 0.0, acc[1] += in ? m.y : 0.0, acc[2] += in ? m.z : 0.0;
        acc[3] += in ? c.x : 0.0, acc[4] += in ? c.y : 0.0, acc[5] += in ? c.z : 0.0;
        acc[6] += in ? 1.0 : 0.0;   // (exact: a count below 2^53)
    }
    rigid_block_sum<7>(acc, L);
    const double cnt = L.sum[6];
    if (!(cnt >= (double)RIGID_MIN)) return false;   // (uniform: read behind the barrier)
    const double mbar[3] = {L.sum[0] / cnt, L.sum[1] / cnt, L.sum[2] / cnt}, cbar[3] = {L.sum[3] / cnt, L.sum[4] / cnt, L.sum[5] / cnt};
    __syncthreads();   // L.sum has been read by everyone
#pragma unroll
    for (int k = 0; k < RIGID_SUMS; ++k) acc[k] = 0.0;
#pragma unroll 4
    for (int i = tid; i < count; i += RIGID_THREADS) {
        const bool in = mask == nullptr || mask[i] != 0;
        const V3 m = load3(mod + (size_t)i * 3), c = load3(cam + (size_t)i * 3);
        const double dm[3] = {in ? m.x - mbar[0] : 0.0, in ? m.y - mbar[1] : 0.0, in ? m.z - mbar[2] : 0.0};
        const double dc[3] = {in ? c.x - cbar[0] : 0.0, in ? c.y - cbar[1] : 0.0, in ? c.z - cbar[2] : 0.0};
#pragma unroll
        for (int a = 0; a < 3; ++a)
#pragma unroll
            for (int b = 0; b < 3; ++b) acc[a * 3 + b] = fma(dm[a], dc[b], acc[a * 3 + b]);
    }
    rigid_block_sum<9>(acc, L);
    if (tid == 0) {
        double S[9], R[9], t[3];
#pragma unroll
        for (int k = 0; k < 9; ++k) S[k] = L.sum[k];
        const bool ok = rigid_solve(S, mbar, cbar, R, t);
        if (ok) {
#pragma unroll
            for (int k = 0; k < 9; ++k) L.cur[k] = R[k];
#pragma unroll
            for (int k = 0; k < 3; ++k) L.cur[9 + k] = t[k];
        }
        L.good = ok ? 1 : 0;
    }
    __syncthreads();
    return L.good != 0;
}

// inliers of the pose L.cur: mask[i] = (squared distance < thr2) for i < count; the count and the inliers' squared distance sum are left in L.count
// and L.sum[1].  thr2 < 0: no gate (every row counts, mask untouched).  Called by the whole workgroup.
__device__ void rigid_select(const double* __restrict__ cam, const double* __restrict__ mod, unsigned char* mask, int count, double thr2,
                             RigidLds& L) {
    const int tid = threadIdx.x;
    double R[9], t[3], acc[2] = {0.0, 0.0};
#pragma unroll
    for (int k = 0; k < 9; ++k) R[k] = L.cur[k];
#pragma unroll
    for (int k = 0; k < 3; ++k) t[k] = L.cur[9 + k];
#pragma unroll 4
    for (int i = tid; i < count; i += RIGID_THREADS) {
        const double e = rigid_err2(R, t, load3(mod + (size_t)i * 3), load3(cam + (size_t)i * 3));
        const bool in = thr2 < 0.0 ? true : e < thr2;
        if (thr2 >= 0.0) mask[i] = in ? 1 : 0;
        acc[0] += in ? 1.0 : 0.0;   // (exact: a count below 2^53)
        acc[1] += in ? e : 0.0;
    }
    rigid_block_sum<2>(acc, L);
    if (tid == 0) L.count = (int)L.sum[0];
    __syncthreads();
}

// One workgroup per RoI: hypotheses in chunks of RIGID_HYP, each chunk scored against all pairs.  win[n] = (R, t, count) of the best hypothesis;
// count 0 when there is none.
__global__ __launch_bounds__(RIGID_THREADS) void rigid_ransac_kernel(const double* __restrict__ cam_pts, const double* __restrict__ mod_pts,
                                                                     const int* __restrict__ counts, int stride, double thr2, int iters,
                                                                     unsigned long long seed, double* __restrict__ win) {
    __shared__ double hyp[RIGID_HYP * 12];   // [R | t] of the chunk's hypotheses, NaN for a degenerate one
    __shared__ double s_cam[RIGID_TILE * 3];
    __shared__ double s_mod[RIGID_TILE * 3];
    __shared__ int cnt[RIGID_HYP];
    __shared__ unsigned long long best_key;
    __shared__ double best_pose[12];
    const int n = blockIdx.x, tid = threadIdx.x;
    const int count = min(max(counts[n], 0), stride);
    double* w = win + (size_t)n * RIGID_WIN;
    if (count < RIGID_MIN) {   // (uniform over the workgroup)
        if (tid < RIGID_WIN) w[tid] = 0.0;
        return;
    }
    const double* cam = cam_pts + (size_t)n * stride * 3;
    const double* mod = mod_pts + (size_t)n * stride * 3;
    if (tid == 0) best_key = 0ull;
    if (tid < 12) best_pose[tid] = 0.0;
    for (int h0 = 0; h0 < iters; h0 += RIGID_HYP) {
        const int nh = min(RIGID_HYP, iters - h0);
        __syncthreads();   // the previous chunk has been consumed
        cnt[tid] = 0;
        double R[9], t[3];
        if (tid < nh) {
            int idx[3];
            bool ok = pnp_sample<3>(seed, n, h0 + tid, count, idx);
            if (ok) {
                double m[9], c[9];
#pragma unroll
                for (int s = 0; s < 3; ++s)
#pragma unroll
                    for (int k = 0; k < 3; ++k) {
                        m[s * 3 + k] = mod[(size_t)idx[s] * 3 + k];
                        c[s * 3 + k] = cam[(size_t)idx[s] * 3 + k];
                    }
                ok = rigid_from_three(m, c, R, t);
            }
#pragma unroll
            for (int k = 0; k < 9; ++k) hyp[tid * 12 + k] = ok ? R[k] : __builtin_nan("");
#pragma unroll
            for (int k = 0; k < 3; ++k) hyp[tid * 12 + 9 + k] = ok ? t[k] : __builtin_nan("");
        }
        __syncthreads();
        // P = the power of two >= nh hypothesis lanes, 256 / P groups of threads share the tile's pairs between them
        int lg = 0;
        while ((1 << lg) < nh) ++lg;
        const int P = 1 << lg, G = RIGID_THREADS >> lg, h = tid & (P - 1), g = tid >> lg;
        double M[12];
#pragma unroll
        for (int k = 0; k < 12; ++k) M[k] = hyp[(h < nh ? h : 0) * 12 + k];
        int local = 0;
        for (int t0 = 0; t0 < count; t0 += RIGID_TILE) {
            const int c = min(RIGID_TILE, count - t0);
            __syncthreads();   // the previous tile has been consumed
            double rc[RIGID_STAGE], rm[RIGID_STAGE];   // (all loads of the tile in flight before the first LDS write)
#pragma unroll
            for (int k = 0; k < RIGID_STAGE; ++k) {
                const int j = tid + k * RIGID_THREADS;
                rc[k] = j < c * 3 ? cam[(size_t)t0 * 3 + j] : 0.0;
                rm[k] = j < c * 3 ? mod[(size_t)t0 * 3 + j] : 0.0;
            }
#pragma unroll
            for (int k = 0; k < RIGID_STAGE; ++k) {
                const int j = tid + k * RIGID_THREADS;
                if (j < c * 3) {
                    s_cam[j] = rc[k];
                    s_mod[j] = rm[k];
                }
            }
            __syncthreads();
            if (h < nh) {
                int j = g;
                for (; j + 3 * G < c; j += 4 * G) {   // four independent pairs in flight: one wave per SIMD has nothing else to hide the LDS reads behind
                    double e[4];
#pragma unroll
                    for (int q = 0; q < 4; ++q) e[q] = rigid_err2(M, M + 9, load3(s_mod + (j + q * G) * 3), load3(s_cam + (j + q * G) * 3));
#pragma unroll
                    for (int q = 0; q < 4; ++q) local += e[q] < thr2 ? 1 : 0;
                }
                for (; j < c; j += G) local += rigid_err2(M, M + 9, load3(s_mod + j * 3), load3(s_cam + j * 3)) < thr2 ? 1 : 0;
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
    else if (tid < RIGID_WIN) w[tid] = 0.0;
}

// One workgroup per RoI.  mode 0: from the RANSAC winner in win[n] -- inliers of the winner, closed form on them, re-select, closed form once more,
// and the mask / count / rms of the pose that is returned.  mode 1: the closed form over all rows, no gate.  A RoI that cannot be solved keeps the
// caller's R and t and gets ok = 0 (num_inliers 0, mask 0, rms NaN).  mask is [N][stride] (mode 0: never NULL, the host passes scratch).
__global__ __launch_bounds__(RIGID_THREADS) void rigid_refine_kernel(const double* __restrict__ cam_pts, const double* __restrict__ mod_pts,
                                                                     const int* __restrict__ counts, int stride, int mode, double thr2,
                                                                     const double* __restrict__ win, double* __restrict__ R_io,
                                                                     double* __restrict__ t_io, int* __restrict__ ok, int* __restrict__ num_inliers,
                                                                     unsigned char* __restrict__ mask_all, double* __restrict__ rms) {
    __shared__ RigidLds L;
    const int n = blockIdx.x, tid = threadIdx.x;
    const int count = min(max(counts[n], 0), stride);
    const double* cam = cam_pts + (size_t)n * stride * 3;
    const double* mod = mod_pts + (size_t)n * stride * 3;
    unsigned char* mask = mask_all ? mask_all + (size_t)n * stride : nullptr;
    bool good = count >= RIGID_MIN;
    if (mode == 0) good = good && win[(size_t)n * RIGID_WIN + 12] >= (double)RIGID_MIN;
    if (good) {   // (every condition below is uniform over the workgroup)
        if (mode == 0) {
            if (tid < 12) L.cur[tid] = win[(size_t)n * RIGID_WIN + tid];
            __syncthreads();
            for (int round = 0; round < 2 && good; ++round) {
                rigid_select(cam, mod, mask, count, thr2, L);
                good = L.count >= RIGID_MIN && rigid_fit_block(cam, mod, mask, count, L);
            }
            if (good) {
                rigid_select(cam, mod, mask, count, thr2, L);
                good = L.count >= RIGID_MIN;
            }
        } else {
            good = rigid_fit_block(cam, mod, (const unsigned char*)nullptr, count, L);
            if (good) rigid_select(cam, mod, (unsigned char*)nullptr, count, -1.0, L);
        }
        if (good) good = rigid_finite(L.sum[1]);
    }
    __syncthreads();
    if (good) {
        if (tid < 9) R_io[(size_t)n * 9 + tid] = L.cur[tid];
        else if (tid < 12) t_io[(size_t)n * 3 + tid - 9] = L.cur[tid];
    }
    if (tid == 0) {
        ok[n] = good ? 1 : 0;
        if (num_inliers) num_inliers[n] = good ? L.count : 0;
        if (rms) rms[n] = good ? sqrt(L.sum[1] / (double)L.count) : __builtin_nan("");
    }
    if (mode == 0 && mask)   // rows beyond counts[n] are no inliers; an unsolved RoI has none
        for (int i = good ? count + tid : tid; i < stride; i += RIGID_THREADS) mask[i] = 0;
}

long long rigid_win_bytes(int N) { return (((long long)N * RIGID_WIN * (long long)sizeof(double)) + 255) / 256 * 256; }

}  // namespace

extern "C" int gdrn_backproject_points(const float* img_pts, const float* model_pts, const int* counts, const float* depth, const int* frame,
                                       const int* frame_host, int F, int H, int W, const double* K, int N, int stride, double* cam, double* mod,
                                       int* counts_out, void* stream) {
    if (!img_pts || !model_pts || !counts || !depth || !frame || !frame_host || !K || !cam || !mod || !counts_out) return GDRN_ERR_ARG;
    if (N <= 0 || stride <= 0 || F <= 0 || H <= 0 || W <= 0) return GDRN_ERR_ARG;
    if ((long long)H * W >= (1ll << 31) || (long long)stride * 3 >= (1ll << 31)) return GDRN_ERR_SHAPE;
    if (!host_in_range(frame_host, N, F)) return GDRN_ERR_ARG;
    GDRN_LAUNCH(rigid_backproject_kernel, dim3(N), dim3(RIGID_THREADS), 0, reinterpret_cast<hipStream_t>(stream), img_pts, model_pts, counts, depth,
                frame, F, H, W, K, stride, cam, mod, counts_out);
    GDRN_CHECK_LAUNCH();
    return GDRN_OK;
}

extern "C" long long gdrn_rigid_workspace_bytes(int N, int stride, int iters) {
    if (N <= 0 || stride <= 0 || iters <= 0) return GDRN_ERR_ARG;
    return rigid_win_bytes(N) + (long long)N * stride;   // the winners + an inlier mask for the calls that pass none
}

extern "C" int gdrn_rigid_ransac(const double* cam, const double* mod, const int* counts, int N, int stride, double dist_thr, int iters,
                                 unsigned long long seed, double* R, double* t, int* ok, int* num_inliers, unsigned char* inlier_mask, double* rms,
                                 void* workspace, void* stream) {
    if (!cam || !mod || !counts || !R || !t || !ok || !num_inliers || !workspace) return GDRN_ERR_ARG;
    if (N <= 0 || stride <= 0 || iters <= 0 || !(dist_thr > 0.0) || !rigid_finite(dist_thr)) return GDRN_ERR_ARG;
    if ((long long)stride * 3 >= (1ll << 31)) return GDRN_ERR_SHAPE;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    double* win = reinterpret_cast<double*>(workspace);
    unsigned char* mask = inlier_mask ? inlier_mask : reinterpret_cast<unsigned char*>(workspace) + rigid_win_bytes(N);
    const double thr2 = dist_thr * dist_thr;
    GDRN_LAUNCH(rigid_ransac_kernel, dim3(N), dim3(RIGID_THREADS), 0, st, cam, mod, counts, stride, thr2, iters, seed, win);
    GDRN_CHECK_LAUNCH();
    GDRN_LAUNCH(rigid_refine_kernel, dim3(N), dim3(RIGID_THREADS), 0, st, cam, mod, counts, stride, 0, thr2, (const double*)win, R, t, ok,
                num_inliers, mask, rms);
    GDRN_CHECK_LAUNCH();
    return GDRN_OK;
}

extern "C" int gdrn_rigid_fit(const double* cam, const double* mod, const int* counts, int N, int stride, double* R, double* t, int* ok, double* rms,
                              void* stream) {
    if (!cam || !mod || !counts || !R || !t || !ok) return GDRN_ERR_ARG;
    if (N <= 0 || stride <= 0) return GDRN_ERR_ARG;
    if ((long long)stride * 3 >= (1ll << 31)) return GDRN_ERR_SHAPE;
    GDRN_LAUNCH(rigid_refine_kernel, dim3(N), dim3(RIGID_THREADS), 0, reinterpret_cast<hipStream_t>(stream), cam, mod, counts, stride, 1, -1.0,
                (const double*)nullptr, R, t, ok, (int*)nullptr, (unsigned char*)nullptr, rms);
    GDRN_CHECK_LAUNCH();
    return GDRN_OK;
}
