// Hypothesis verification for gfx950, the step behind the ICP of icp.hip: how well does each candidate pose explain the observed depth frame and
// the observed instance mask, and which candidate of a detection explains them best --
//   (rendered depth, observed depth, observed mask) -> nine integer counts per candidate                   -> gdrn_verify_maps
//   counts -> one fp64 score and an ok flag per candidate                                                   -> gdrn_verify_score
//   (score, ok, group) -> the best candidate of every group and its score                                   -> gdrn_verify_select
//   render, count, score on one stream without a host read                                                  -> gdrn_verify_poses
// The reference has no counterpart (it is RGB-only); the arithmetic is stated with the entry points in include/gdrn_hip.h and restated on the
// host in tests/verify_host.py.
//
// The counting pass: a workgroup takes a chunk of VF_CHUNK pixels of ONE candidate (scalar loads per lane, so neither W, H * W nor a base needs
// any alignment), laid out as cou_pixels_kernel is.  A lane loads its VF_PPT render depths and its VF_PPT mask bytes before it looks at any of
// them; the observed depth is read only where the render is covered, the mask over the whole frame (mask_px needs every pixel).  A wave counts
// with ballots and popcounts and folds the lanes' quantised residuals through shuffles, the waves meet in LDS, and the workgroup adds to the
// candidate's seven running integers with at most one integer atomic per quantity -- none from a workgroup that saw neither a covered nor a
// mask pixel.  All of it is integers: the result does not depend on the launch shape or on any order, and repeated calls give the same bits.
//
// The selection: two integer atomics per eligible row -- atomicMax of the order-preserving key of its score on the group's slot (which is the
// best_score output itself), then atomicMin of the row index among the rows that hold the maximum.  No floating-point atomics anywhere.
//
// Floating-point contraction is OFF for this file: the score is one fixed fp64 operation sequence, which the host restatement repeats.
// (No 16-bit code: both library builds compile the same thing.)
#include "common.h"
#include "geom64.h"
#include "../../include/gdrn_hip.h"

#include <limits.h>

#pragma clang fp contract(off)

#include "render_loop.h"

namespace {

constexpr int VF_THREADS = 256;
constexpr int VF_PPT = 8;                          // pixels per thread: that many render loads (and mask loads) in flight per lane
constexpr int VF_CHUNK = VF_THREADS * VF_PPT;      // pixels per workgroup
constexpr int VF_ACC = 8;                          // int32 slots per candidate: inlier, occluded, violated, unknown, mask_px, inter, sum_q (2 slots)
constexpr int VF_COUNTS = 8;                       // the counts output: covered, inlier, occluded, violated, unknown, visible, mask_px, inter
constexpr double VF_Q = 1048576.0;                 // 2^20: the residual's quantum is tau-independent, 2^-20 m

// fp32 bits.  covered: > 0 as IEEE compares it (positive subnormals and +inf are; +-0, negatives and NaNs are not).  usable: finite and > 0.
// Decided on the bit pattern, so the denormal mode of a floating-point compare never enters.
__device__ __forceinline__ bool vf_covered(unsigned bits) { return bits - 1u < 0x7f800000u; }
__device__ __forceinline__ bool vf_usable(unsigned bits) { return bits - 1u < 0x7f7fffffu; }

// Workgroup (chunk, candidate).  acc [N][VF_ACC] int32, zero before the launch.  MASK: mask_obs [M][HW] bytes, mask_index (NULL: row i) [N].
template <bool MASK>
__global__ __launch_bounds__(VF_THREADS) void vf_count_kernel(const unsigned* __restrict__ depth_ren, const unsigned* __restrict__ depth_scene,
                                                               const int* __restrict__ frame, int F, const unsigned char* __restrict__ mask_obs,
                                                               const int* __restrict__ mask_index, int M, int HW, double tau,
                                                               int* __restrict__ acc) {
    __shared__ unsigned s_cnt[7];
    const int i = blockIdx.y, tid = threadIdx.x;
    const int f = frame[i];
    if (f < 0 || f >= F) return;                     // (the host side of the entry point refuses such a frame before the launch)
    int mi = 0;
    if (MASK) {
        mi = mask_index != nullptr ? mask_index[i] : i;
        if (mi < 0 || mi >= M) return;
    }
    const unsigned p0 = blockIdx.x * (unsigned)VF_CHUNK + tid, n_px = (unsigned)HW;   // (H * W + VF_CHUNK fits an unsigned: vf_frame_ok)
    if (tid < 7) s_cnt[tid] = 0u;
    __syncthreads();
    const unsigned* ren = depth_ren + (size_t)i * HW;
    const unsigned* sc = depth_scene + (size_t)f * HW;
    const unsigned char* mk = mask_obs + (size_t)mi * HW;
    unsigned z[VF_PPT], s[VF_PPT];
    unsigned char m[VF_PPT];
#pragma unroll
    for (int u = 0; u < VF_PPT; ++u) {               // all render and mask loads first
        const unsigned p = p0 + u * VF_THREADS;
        z[u] = p < n_px ? ren[p] : 0u;
        m[u] = (MASK && p < n_px) ? mk[p] : (unsigned char)0;
    }
#pragma unroll
    for (int u = 0; u < VF_PPT; ++u) s[u] = vf_covered(z[u]) ? sc[p0 + u * VF_THREADS] : 0u;   // (a covered pixel lies inside the row)
    int n_in = 0, n_occ = 0, n_vio = 0, n_unk = 0, n_mask = 0, n_inter = 0;   // uniform over the wave
    unsigned q = 0u;                                 // the lane's quantised residuals: at most VF_PPT * 2^20
#pragma unroll
    for (int u = 0; u < VF_PPT; ++u) {
        const bool cov = vf_covered(z[u]), use = cov && vf_usable(s[u]), msk = m[u] != 0;
        const double e = (double)__uint_as_float(z[u]) - (double)__uint_as_float(s[u]);   // exact
        const bool inl = use && fabs(e) <= tau, occ = use && e > tau, vio = use && e < -tau;
        if (inl) q += (unsigned)(long long)floor(fabs(e) * VF_Q);
        n_in += __popcll(__ballot(inl));
        n_occ += __popcll(__ballot(occ));
        n_vio += __popcll(__ballot(vio));
        n_unk += __popcll(__ballot(cov && !use));
        n_mask += __popcll(__ballot(msk));
        n_inter += __popcll(__ballot(msk && cov && !occ));
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) q += __shfl_xor(q, o, 64);   // at most 64 * VF_PPT * 2^20 = 2^29
    if ((tid & 63) == 0) {
        if (n_in != 0) atomicAdd(&s_cnt[0], (unsigned)n_in);
        if (n_occ != 0) atomicAdd(&s_cnt[1], (unsigned)n_occ);
        if (n_vio != 0) atomicAdd(&s_cnt[2], (unsigned)n_vio);
        if (n_unk != 0) atomicAdd(&s_cnt[3], (unsigned)n_unk);
        if (n_mask != 0) atomicAdd(&s_cnt[4], (unsigned)n_mask);
        if (n_inter != 0) atomicAdd(&s_cnt[5], (unsigned)n_inter);
        if (q != 0u) atomicAdd(&s_cnt[6], q);        // at most VF_CHUNK * 2^20 = 2^31
    }
    __syncthreads();
    int* a = acc + (size_t)i * VF_ACC;
    if (tid < 6) {
        if (s_cnt[tid] != 0u) atomicAdd(a + tid, (int)s_cnt[tid]);
    } else if (tid == 6) {
        if (s_cnt[6] != 0u) atomicAdd(reinterpret_cast<unsigned long long*>(a + 6), (unsigned long long)s_cnt[6]);
    }
}

// One thread per candidate: the running integers into the outputs, covered and visible derived.
__global__ __launch_bounds__(VF_THREADS) void vf_counts_kernel(const int* __restrict__ acc, int N, int* __restrict__ counts,
                                                                long long* __restrict__ sum_q) {
    const int i = blockIdx.x * VF_THREADS + threadIdx.x;
    if (i >= N) return;
    const int* a = acc + (size_t)i * VF_ACC;
    const int inl = a[0], occ = a[1], vio = a[2], unk = a[3];
    const int covered = ((inl + occ) + vio) + unk;
    int* c = counts + (size_t)i * VF_COUNTS;
    c[0] = covered;
    c[1] = inl;
    c[2] = occ;
    c[3] = vio;
    c[4] = unk;
    c[5] = covered - occ;
    c[6] = a[4];
    c[7] = a[5];
    sum_q[i] = *reinterpret_cast<const long long*>(a + 6);
}

__device__ __forceinline__ double vf_neg_inf() { return __longlong_as_double((long long)0xfff0000000000000ULL); }

// One thread per candidate: the score, the operation sequence of include/gdrn_hip.h.
__global__ __launch_bounds__(VF_THREADS) void vf_score_kernel(const int* __restrict__ counts, const long long* __restrict__ sum_q, int N,
                                                               int has_mask, double tau, double penalty, int min_covered,
                                                               double* __restrict__ score, int* __restrict__ ok) {
    const int i = blockIdx.x * VF_THREADS + threadIdx.x;
    if (i >= N) return;
    const int* c = counts + (size_t)i * VF_COUNTS;
    const int covered = c[0], inlier = c[1], violated = c[3], visible = c[5], mask_px = c[6], inter = c[7];
    if (covered < min_covered) {
        ok[i] = 0;
        score[i] = vf_neg_inf();
        return;
    }
    const double tq = tau * VF_Q;
    const double fit = (double)inlier - (double)sum_q[i] / tq;
    double iou = 1.0;
    if (has_mask) {
        const int uni = visible + mask_px - inter;
        iou = uni > 0 ? (double)inter / (double)uni : 0.0;
    }
    ok[i] = 1;
    score[i] = (iou * fit - penalty * (double)violated) / (double)covered;
}

// Order-preserving map of the fp64 bits to unsigned: the sign bit of a non-negative flipped, all bits of a negative inverted (-0.0 sorts below
// +0.0).  No value that compares equal to itself maps to 0, the empty slot.
__device__ __forceinline__ unsigned long long vf_key(double v) {
    const unsigned long long b = (unsigned long long)__double_as_longlong(v);
    return (b >> 63) ? ~b : (b | 0x8000000000000000ULL);
}
__device__ __forceinline__ double vf_value(unsigned long long k) {
    return __longlong_as_double((long long)((k >> 63) ? (k & 0x7fffffffffffffffULL) : ~k));
}
__device__ __forceinline__ bool vf_eligible(const double* score, const int* ok, const int* group, int G, int i) {
    const int g = group[i];
    return ok[i] != 0 && score[i] == score[i] && g >= 0 && g < G;   // (the host side refuses a group out of range before the launch)
}

__global__ __launch_bounds__(VF_THREADS) void vf_select_init_kernel(int G, unsigned long long* __restrict__ key, int* __restrict__ best) {
    const int g = blockIdx.x * VF_THREADS + threadIdx.x;
    if (g >= G) return;
    key[g] = 0ull;
    best[g] = INT_MAX;
}
__global__ __launch_bounds__(VF_THREADS) void vf_select_max_kernel(const double* __restrict__ score, const int* __restrict__ ok,
                                                                    const int* __restrict__ group, int N, int G, unsigned long long* __restrict__ key) {
    const int i = blockIdx.x * VF_THREADS + threadIdx.x;
    if (i >= N || !vf_eligible(score, ok, group, G, i)) return;
    atomicMax(key + group[i], vf_key(score[i]));
}
__global__ __launch_bounds__(VF_THREADS) void vf_select_row_kernel(const double* __restrict__ score, const int* __restrict__ ok,
                                                                    const int* __restrict__ group, int N, int G,
                                                                    const unsigned long long* __restrict__ key, int* __restrict__ best) {
    const int i = blockIdx.x * VF_THREADS + threadIdx.x;
    if (i >= N || !vf_eligible(score, ok, group, G, i)) return;
    if (vf_key(score[i]) == key[group[i]]) atomicMin(best + group[i], i);   // the lowest row among those that hold the maximum
}
// key [G] and best_score [G] are the same memory: the slot's key is replaced by the value it encodes
__global__ __launch_bounds__(VF_THREADS) void vf_select_final_kernel(int G, unsigned long long* __restrict__ key, int* __restrict__ best) {
    const int g = blockIdx.x * VF_THREADS + threadIdx.x;
    if (g >= G) return;
    const unsigned long long k = key[g];
    double* out = reinterpret_cast<double*>(key) + g;
    if (k == 0ull) {
        best[g] = -1;
        *out = vf_neg_inf();
    } else {
        *out = vf_value(k);
    }
}

bool vf_frame_ok(int N, int H, int W) { return N >= 0 && H >= 1 && W >= 1 && (long long)H * W <= 0x7fffffffLL - 1024; }   // the ICP's limit
bool vf_tau_ok(double tau) { return tau > 0.0 && tau <= 1.0; }
bool vf_score_scalars_ok(double tau, double penalty, int min_covered) {
    return vf_tau_ok(tau) && penalty >= 0.0 && penalty < __builtin_inf() && min_covered >= 1;
}

// the mask arguments: none at all (mask_obs NULL), or M >= 1 masks with both copies of the index vector -- or neither, which means M == N, row i
struct VfMask {
    const unsigned char* mask_obs;
    const int *mask_index, *mask_index_host;
    int M;
};
int vf_mask_check(const VfMask& m, int N) {
    if (!m.mask_obs) return GDRN_OK;
    if (m.M < 1 || (m.mask_index == nullptr) != (m.mask_index_host == nullptr)) return GDRN_ERR_ARG;
    if (!m.mask_index) return m.M == N ? GDRN_OK : GDRN_ERR_ARG;
    return host_in_range(m.mask_index_host, N, m.M) ? GDRN_OK : GDRN_ERR_ARG;
}

// clear the running integers, count, write the counts.  The grid: chunks in x, candidates in y (N <= 65535).
int vf_launch_maps(const float* depth_ren, const float* depth_scene, const int* frame, int F, const VfMask& m, int N, int H, int W, double tau,
                   int* counts, long long* sum_q, void* workspace, hipStream_t st) {
    int* acc = reinterpret_cast<int*>(workspace);
    if (hipMemsetAsync(acc, 0, (size_t)N * VF_ACC * sizeof(int), st) != hipSuccess) return GDRN_ERR_LAUNCH;
    const int HW = H * W;
    const dim3 grid((unsigned)(((long long)HW + VF_CHUNK - 1) / VF_CHUNK), N);
    const unsigned* ren = reinterpret_cast<const unsigned*>(depth_ren);
    const unsigned* sc = reinterpret_cast<const unsigned*>(depth_scene);
    if (m.mask_obs)
        GDRN_LAUNCH(vf_count_kernel<true>, grid, dim3(VF_THREADS), 0, st, ren, sc, frame, F, m.mask_obs, m.mask_index, m.M, HW, tau, acc);
    else
        GDRN_LAUNCH(vf_count_kernel<false>, grid, dim3(VF_THREADS), 0, st, ren, sc, frame, F, (const unsigned char*)nullptr, (const int*)nullptr, 0, HW,
                    tau, acc);
    GDRN_CHECK_LAUNCH();
    GDRN_LAUNCH(vf_counts_kernel, dim3(cdiv(N, VF_THREADS)), dim3(VF_THREADS), 0, st, (const int*)acc, N, counts, sum_q);
    GDRN_CHECK_LAUNCH();
    return GDRN_OK;
}

int vf_launch_score(const int* counts, const long long* sum_q, int N, int has_mask, double tau, double penalty, int min_covered, double* score,
                    int* ok, hipStream_t st) {
    GDRN_LAUNCH(vf_score_kernel, dim3(cdiv(N, VF_THREADS)), dim3(VF_THREADS), 0, st, counts, sum_q, N, has_mask, tau, penalty, min_covered, score, ok);
    GDRN_CHECK_LAUNCH();
    return GDRN_OK;
}

}  // namespace

extern "C" long long gdrn_verify_workspace_bytes(int N, int H, int W) {
    if (!vf_frame_ok(N, H, W)) return GDRN_ERR_ARG;
    return (long long)N * VF_ACC * (long long)sizeof(int);
}

extern "C" int gdrn_verify_maps(const float* depth_ren, const float* depth_scene, const int* frame, const int* frame_host, int F,
                                const unsigned char* mask_obs, const int* mask_index, const int* mask_index_host, int M, int N, int H, int W,
                                double tau, int* counts, long long* sum_q, void* workspace, void* stream) {
    if (!vf_frame_ok(N, H, W) || F < 0 || !vf_tau_ok(tau)) return GDRN_ERR_ARG;
    if (N == 0) return GDRN_OK;
    if (!depth_ren || !depth_scene || !frame || !frame_host || !counts || !sum_q || !workspace || ((size_t)workspace & 7)) return GDRN_ERR_ARG;
    if (N > 65535) return GDRN_ERR_SHAPE;   // the candidates are the grid's second dimension
    if (!host_in_range(frame_host, N, F)) return GDRN_ERR_ARG;
    const VfMask m = {mask_obs, mask_index, mask_index_host, M};
    const int bad = vf_mask_check(m, N);
    if (bad != GDRN_OK) return bad;
    return vf_launch_maps(depth_ren, depth_scene, frame, F, m, N, H, W, tau, counts, sum_q, workspace, reinterpret_cast<hipStream_t>(stream));
}

extern "C" int gdrn_verify_score(const int* counts, const long long* sum_q, int N, int has_mask, double tau, double penalty, int min_covered,
                                 double* score, int* ok, void* stream) {
    if (N < 0 || !vf_score_scalars_ok(tau, penalty, min_covered)) return GDRN_ERR_ARG;
    if (N == 0) return GDRN_OK;
    if (!counts || !sum_q || !score || !ok) return GDRN_ERR_ARG;
    return vf_launch_score(counts, sum_q, N, has_mask != 0, tau, penalty, min_covered, score, ok, reinterpret_cast<hipStream_t>(stream));
}

extern "C" int gdrn_verify_select(const double* score, const int* ok, const int* group, const int* group_host, int N, int G, int* best,
                                  double* best_score, void* stream) {
    if (N < 0 || G < 0) return GDRN_ERR_ARG;
    if (N > 0 && (!score || !ok || !group || !group_host)) return GDRN_ERR_ARG;
    if (N > 0 && !host_in_range(group_host, N, G)) return GDRN_ERR_ARG;
    if (G == 0) return GDRN_OK;
    if (!best || !best_score || ((size_t)best_score & 7)) return GDRN_ERR_ARG;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    unsigned long long* key = reinterpret_cast<unsigned long long*>(best_score);
    GDRN_LAUNCH(vf_select_init_kernel, dim3(cdiv(G, VF_THREADS)), dim3(VF_THREADS), 0, st, G, key, best);
    GDRN_CHECK_LAUNCH();
    if (N > 0) {
        GDRN_LAUNCH(vf_select_max_kernel, dim3(cdiv(N, VF_THREADS)), dim3(VF_THREADS), 0, st, score, ok, group, N, G, key);
        GDRN_CHECK_LAUNCH();
        GDRN_LAUNCH(vf_select_row_kernel, dim3(cdiv(N, VF_THREADS)), dim3(VF_THREADS), 0, st, score, ok, group, N, G, (const unsigned long long*)key,
                    best);
        GDRN_CHECK_LAUNCH();
    }
    GDRN_LAUNCH(vf_select_final_kernel, dim3(cdiv(G, VF_THREADS)), dim3(VF_THREADS), 0, st, G, key, best);
    GDRN_CHECK_LAUNCH();
    return GDRN_OK;
}

extern "C" int gdrn_verify_poses(const double* verts, const int* faces, const int* vert_off, const int* nverts, const int* face_off,
                                 const int* nfaces, int C, int f_max, const int* labels, const int* labels_host, const double* R, const double* t,
                                 const double* K, int N, const float* depth_scene, const int* frame, const int* frame_host, int F, int H, int W,
                                 double near, double far, const unsigned char* mask_obs, const int* mask_index, const int* mask_index_host, int M,
                                 double tau, double penalty, int min_covered, float* depth_ren_scratch, int* counts, long long* sum_q,
                                 double* score, int* ok, void* workspace, void* stream) {
    const RenderRows rows = {verts, faces, vert_off, nverts, face_off, nfaces, C, f_max, labels, labels_host, R, t, K, N, H, W, near, far};
    const RenderScene scene = {depth_scene, frame, frame_host, F};
    if (!vf_frame_ok(N, H, W) || !vf_score_scalars_ok(tau, penalty, min_covered)) return GDRN_ERR_ARG;
    if (!loop_scalars_ok(rows, scene)) return GDRN_ERR_ARG;
    if (N == 0) return GDRN_OK;
    if (!depth_ren_scratch || !counts || !sum_q || !score || !ok || !workspace || ((size_t)workspace & 7)) return GDRN_ERR_ARG;
    int bad = loop_rows_check(rows, scene);
    if (bad != GDRN_OK) return bad;
    const VfMask m = {mask_obs, mask_index, mask_index_host, M};
    bad = vf_mask_check(m, N);
    if (bad != GDRN_OK) return bad;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    bad = render_into(rows, depth_ren_scratch, stream);
    if (bad != GDRN_OK) return bad;
    bad = vf_launch_maps(depth_ren_scratch, depth_scene, frame, F, m, N, H, W, tau, counts, sum_q, workspace, st);
    if (bad != GDRN_OK) return bad;
    return vf_launch_score(counts, sum_q, N, mask_obs != nullptr, tau, penalty, min_covered, score, ok, st);
}
