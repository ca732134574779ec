// What the depth refinement's passes share (csrc/icp.hip, csrc/silhouette.hip): the launch shape of an accumulate pass, its band fold, the band
// combine with the kernel behind a stand-alone accumulate, the init kernel of a loop, and the solve-and-update step with the rules stated with
// gdrn_icp_step in include/gdrn_hip.h.  Included behind `#pragma clang fp contract(off)`: the operation sequence is the contract.
#pragma once

namespace {

constexpr int ICP_THREADS = 256;
constexpr int ICP_WAVES = ICP_THREADS / 64;
constexpr int ICP_BAND_ROWS = 16;               // rows of one workgroup's band
constexpr int ICP_SUMS = 28;                    // 21 of A (packed upper, row-major), 6 of b, 1 of sq
constexpr double ICP_PIVOT_MIN = 1e-9;          // smallest accepted Cholesky pivot of the Jacobi-scaled matrix
constexpr double ICP_STEP_TOL = 1e-10;          // the PnP refinement's stop rule
constexpr double ICP_SMALL_ANGLE = 1e-12;       // below: exp(w) = I + [w]x

__host__ __device__ __forceinline__ int icp_bands(int H) { return (H + ICP_BAND_ROWS - 1) / ICP_BAND_ROWS; }

// index of (i, j), i <= j, in the packed upper triangle of a 6x6
__host__ __device__ __forceinline__ int icp_tri(int i, int j) { return i * 6 - i * (i - 1) / 2 + (j - i); }

// The end of an accumulate pass, called by every lane of workgroup (band, instance i) with its 28 sums and its pair count: the slab
// sums[i][band][28] and cnts[i][band] in a fixed order (xor tree per wave, four waves in LDS).  The count first: a band without a pair (most of a
// frame) writes its zeros without the fold.
__device__ __forceinline__ void icp_fold_band(const double (&acc)[ICP_SUMS], int n_pairs, double (&red)[ICP_WAVES][ICP_SUMS],
                                              int (&red_n)[ICP_WAVES], int i, int band, int nb, double* __restrict__ sums,
                                              int* __restrict__ cnts) {
    static_assert(ICP_WAVES == 4, "the sums below name four waves");
    const int tid = threadIdx.x;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) n_pairs += __shfl_xor(n_pairs, o, 64);
    if ((tid & 63) == 0) red_n[tid >> 6] = n_pairs;
    __syncthreads();
    const int total = (red_n[0] + red_n[1]) + (red_n[2] + red_n[3]);
    double* slab = sums + ((size_t)i * nb + band) * ICP_SUMS;
    if (tid == 0) cnts[(size_t)i * nb + band] = total;
    if (total == 0) {   // uniform over the workgroup
        if (tid < ICP_SUMS) slab[tid] = 0.0;
        return;
    }
#pragma unroll
    for (int k = 0; k < ICP_SUMS; ++k) {
        const double s = wave_sum_f64(acc[k]);
        if ((tid & 63) == 0) red[tid >> 6][k] = s;
    }
    __syncthreads();
    if (tid < ICP_SUMS) slab[tid] = (red[0][tid] + red[1][tid]) + (red[2][tid] + red[3][tid]);
}

// sum k of instance i over its bands, ascending: the one combine, wherever it runs
__device__ __forceinline__ double icp_combine(const double* __restrict__ sums, int i, int nb, int k) {
    const double* s = sums + (size_t)i * nb * ICP_SUMS + k;
    double v = s[0];
    for (int b = 1; b < nb; ++b) v += s[(size_t)b * ICP_SUMS];
    return v;
}
__device__ __forceinline__ int icp_combine_n(const int* __restrict__ cnts, int i, int nb) {
    int v = 0;
    for (int b = 0; b < nb; ++b) v += cnts[(size_t)i * nb + b];
    return v;
}

// behind a stand-alone accumulate: the slabs into sys [N][28] and pairs [N]; one wave per instance
__global__ __launch_bounds__(64) void icp_combine_kernel(const double* __restrict__ sums, const int* __restrict__ cnts, int nb,
                                                          double* __restrict__ sys, int* __restrict__ pairs) {
    const int i = blockIdx.x, lane = threadIdx.x;
    if (lane < ICP_SUMS) sys[(size_t)i * ICP_SUMS + lane] = icp_combine(sums, i, nb, lane);
    else if (lane == ICP_SUMS) pairs[i] = icp_combine_n(cnts, i, nb);
}

// the defaults of an instance no system was accumulated for (iters == 0), and the running state.  sil_pairs / sil_rms are NULL together: the
// loop without a silhouette term
__global__ __launch_bounds__(ICP_THREADS) void icp_init_kernel(int N, int* __restrict__ state, int* __restrict__ ok, int* __restrict__ iters_done,
                                                                int* __restrict__ pairs, double* __restrict__ rms, int* __restrict__ sil_pairs,
                                                                double* __restrict__ sil_rms) {
    const int i = blockIdx.x * ICP_THREADS + threadIdx.x;
    if (i >= N) return;
    const double nan = __longlong_as_double(0x7ff8000000000000LL);
    state[(size_t)i * 2 + 0] = GDRN_ICP_RUNNING;
    state[(size_t)i * 2 + 1] = 0;
    ok[i] = 1;
    iters_done[i] = 0;
    pairs[i] = 0;
    rms[i] = nan;
    if (sil_pairs == nullptr) return;
    sil_pairs[i] = 0;
    sil_rms[i] = nan;
}

// xi of A xi = -b through the Cholesky factor of S A S, S = diag(A_ii^-1/2); false: degenerate (a diagonal entry <= 0 or a pivot < ICP_PIVOT_MIN,
// NaNs included)
__device__ bool icp_solve(const double* A, const double* b, double* xi) {
    double s[6], L[36], y[6];
    for (int k = 0; k < 6; ++k) {
        const double d = A[icp_tri(k, k)];
        if (!(d > 0.0)) return false;
        s[k] = 1.0 / sqrt(d);
    }
    for (int r = 0; r < 6; ++r)
        for (int c = 0; c <= r; ++c) {
            double v = r == c ? 1.0 : (s[c] * A[icp_tri(c, r)]) * s[r];
            for (int k = 0; k < c; ++k) v -= L[r * 6 + k] * L[c * 6 + k];
            if (r == c) {
                if (!(v >= ICP_PIVOT_MIN)) return false;
                L[r * 6 + r] = sqrt(v);
            } else {
                L[r * 6 + c] = v / L[c * 6 + c];
            }
        }
    for (int r = 0; r < 6; ++r) {
        double v = -(s[r] * b[r]);
        for (int k = 0; k < r; ++k) v -= L[r * 6 + k] * y[k];
        y[r] = v / L[r * 6 + r];
    }
    for (int r = 5; r >= 0; --r) {
        double v = y[r];
        for (int k = r + 1; k < 6; ++k) v -= L[k * 6 + r] * xi[k];
        xi[r] = v / L[r * 6 + r];
    }
    double chk = 0.0;
    for (int r = 0; r < 6; ++r) {
        xi[r] *= s[r];
        chk += xi[r];
    }
    return chk - chk == 0.0;   // finite
}

// E = exp([w]x) (Rodrigues; I + [w]x below ICP_SMALL_ANGLE)
__device__ void icp_exp(const double* w, double* E) {
    const double th2 = (w[0] * w[0] + w[1] * w[1]) + w[2] * w[2], th = sqrt(th2);
    double A = 1.0, B = 0.0;
    if (!(th < ICP_SMALL_ANGLE)) {
        const double sh = sin(0.5 * th);
        A = sin(th) / th;
        B = 2.0 * sh * sh / th2;
    }
    E[0] = 1.0 - B * (w[1] * w[1] + w[2] * w[2]);
    E[1] = -A * w[2] + B * w[0] * w[1];
    E[2] = A * w[1] + B * w[0] * w[2];
    E[3] = A * w[2] + B * w[0] * w[1];
    E[4] = 1.0 - B * (w[0] * w[0] + w[2] * w[2]);
    E[5] = -A * w[0] + B * w[1] * w[2];
    E[6] = -A * w[1] + B * w[0] * w[2];
    E[7] = A * w[0] + B * w[1] * w[2];
    E[8] = 1.0 - B * (w[0] * w[0] + w[1] * w[1]);
}

// Lane 0 of an instance's wave, from its combined system sys[28] and pair count n: DEGENERATE, or the solve, the left-multiplied update and the
// stop rule.  ok / iters_done may be NULL together.
__device__ void icp_solve_and_update(const double* sys, int n, int min_pairs, int i, double* __restrict__ Rm, double* __restrict__ tv,
                                     int* __restrict__ state, int* __restrict__ ok, int* __restrict__ iters_done) {
    double xi[6];
    if (n < min_pairs || !icp_solve(sys, sys + 21, xi)) {
        state[(size_t)i * 2] = GDRN_ICP_DEGENERATE;
        if (ok != nullptr) ok[i] = 0;
        return;
    }
    double R[9], t[3], E[9];
    for (int k = 0; k < 9; ++k) R[k] = Rm[(size_t)i * 9 + k];
    for (int k = 0; k < 3; ++k) t[k] = tv[(size_t)i * 3 + k];
    icp_exp(xi, E);
    for (int r = 0; r < 3; ++r) {
        for (int q = 0; q < 3; ++q) Rm[(size_t)i * 9 + r * 3 + q] = (E[r * 3] * R[q] + E[r * 3 + 1] * R[3 + q]) + E[r * 3 + 2] * R[6 + q];
        tv[(size_t)i * 3 + r] = ((E[r * 3] * t[0] + E[r * 3 + 1] * t[1]) + E[r * 3 + 2] * t[2]) + xi[3 + r];
    }
    const int steps = state[(size_t)i * 2 + 1] + 1;
    state[(size_t)i * 2 + 1] = steps;
    if (iters_done != nullptr) iters_done[i] = steps;
    const double wn = sqrt((xi[0] * xi[0] + xi[1] * xi[1]) + xi[2] * xi[2]), vn = sqrt((xi[3] * xi[3] + xi[4] * xi[4]) + xi[5] * xi[5]);
    const double tn = sqrt((t[0] * t[0] + t[1] * t[1]) + t[2] * t[2]);
    if (wn < ICP_STEP_TOL && vn < ICP_STEP_TOL * tn) state[(size_t)i * 2] = GDRN_ICP_CONVERGED;
}

}  // namespace
