// Complement-over-union pose errors for gfx950: the one family of lib/pysixd/scripts/eval_calc_errors.py's error types that bop_metrics.hip,
// pose_metrics.hip and sixd_scores.hip leave out (lib/pysixd/pose_error.py:466-589) --
//   cus / cou_mask      1 - |est and gt| / |est or gt| of two silhouettes (depth renders > 0, or masks != 0)        -> gdrn_cou_maps, err[.][0]
//   cou_bb_proj         1 - iou of the silhouettes' bounding boxes (misc.calc_2d_bbox_xywh + misc.iou, :644, :809)   -> gdrn_cou_maps, err[.][1]
//   cou_bb              1 - iou of two given x, y, w, h boxes                                                       -> gdrn_cou_bb
// -- for a whole batch per call.  gdrn_cou_maps reads each map once: a workgroup takes a chunk of ONE row's pixels (scalar loads per lane, so
// neither H * W nor the maps' base needs any alignment and nothing straddles two rows), a wave counts with ballots and popcounts and folds its
// lanes' box bounds through shuffles, the waves meet in LDS, and the workgroup adds to the row's ten running integers with at most one integer
// atomic per quantity -- none from a workgroup that saw no covered pixel.  (One atomic per WAVE and quantity was measured first: the ten integers
// of a row share a cache line, and 64 estimates at 480 x 640 then spent more time queueing on 64 lines than reading the maps.)  Counts and
// bounds are integers: the result does not depend on the launch shape or on any order, and repeated calls give the same bits.  A finalize
// launch of one thread per row turns them into the outputs.  The rules are stated with the entry points in include/gdrn_hip.h.
//
// Floating-point contraction is OFF for this file, as in the other evaluation files: the box IoU is the operation sequence of misc.iou in fp64.
// (No 16-bit code: both library builds compile the same thing.)
#include "common.h"
#include "../../include/gdrn_hip.h"

#include <limits.h>

#pragma clang fp contract(off)

namespace {

constexpr int CU_THREADS = 256;
constexpr int CU_WAVES = CU_THREADS / 64;
constexpr int CU_PPT = 8;                          // pixels per thread
constexpr int CU_CHUNK = CU_THREADS * CU_PPT;      // pixels per workgroup
constexpr int CU_ACC = 10;                         // per row: |and|, |or|, est x1 y1 x2 y2, gt x1 y1 x2 y2

// fp32 bits: covered iff the value is > 0 as IEEE compares it -- positive subnormals and +inf are, +-0, negatives and NaNs are not -- decided on
// the bit pattern (0x00000001 .. 0x7f800000), so the denormal mode of a floating-point compare never enters.  Bytes: covered iff non-zero.
__device__ __forceinline__ bool covered(unsigned bits) { return bits - 1u < 0x7f800000u; }
__device__ __forceinline__ bool covered(unsigned char b) { return b != 0; }

__device__ __forceinline__ int wave_min(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = min(v, __shfl_xor(v, o, 64));
    return v;
}
__device__ __forceinline__ int wave_max(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = max(v, __shfl_xor(v, o, 64));
    return v;
}

__global__ __launch_bounds__(CU_THREADS) void cou_init_kernel(int* __restrict__ acc, int N) {
    const int i = blockIdx.x * CU_THREADS + threadIdx.x;
    if (i >= N) return;
    int* a = acc + (size_t)i * CU_ACC;
    a[0] = 0;
    a[1] = 0;
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        a[2 + 4 * k + 0] = INT_MAX;
        a[2 + 4 * k + 1] = INT_MAX;
        a[2 + 4 * k + 2] = INT_MIN;
        a[2 + 4 * k + 3] = INT_MIN;
    }
}

// Workgroup blockIdx.x = row * bpi + chunk: CU_CHUNK pixels of one row's H x W slice of both maps.  E = unsigned (the bits of an fp32 depth) or
// unsigned char (a mask byte).
template <typename E>
__global__ __launch_bounds__(CU_THREADS) void cou_pixels_kernel(const E* __restrict__ est, const E* __restrict__ gt, int HW, int W, int bpi,
                                                                int* __restrict__ acc) {
    __shared__ int s_cnt[2];
    __shared__ int s_box[CU_WAVES][8];
    const int row = blockIdx.x / bpi, tid = threadIdx.x;
    const int p0 = (blockIdx.x - row * bpi) * CU_CHUNK + tid;
    if (tid < 2) s_cnt[tid] = 0;
    __syncthreads();
    const E* e = est + (size_t)row * HW;
    const E* g = gt + (size_t)row * HW;
    E ve[CU_PPT], vg[CU_PPT];
#pragma unroll
    for (int u = 0; u < CU_PPT; ++u) {   // all loads first: sixteen in flight per lane
        const int p = p0 + u * CU_THREADS;
        ve[u] = p < HW ? e[p] : (E)0;
        vg[u] = p < HW ? g[p] : (E)0;
    }
    int n_and = 0, n_or = 0;                       // uniform over the wave
    unsigned long long any_e = 0ull, any_g = 0ull;
    int ex1 = INT_MAX, ey1 = INT_MAX, ex2 = INT_MIN, ey2 = INT_MIN, gx1 = INT_MAX, gy1 = INT_MAX, gx2 = INT_MIN, gy2 = INT_MIN;
#pragma unroll
    for (int u = 0; u < CU_PPT; ++u) {
        const bool ce = covered(ve[u]), cg = covered(vg[u]);   // (beyond the row: the value is 0, not covered)
        const unsigned long long be = __ballot(ce), bg = __ballot(cg);
        n_and += __popcll(be & bg);
        n_or += __popcll(be | bg);
        any_e |= be;
        any_g |= bg;
        if (ce || cg) {
            const int p = p0 + u * CU_THREADS;
            const int y = p / W, x = p - y * W;
            if (ce) {
                ex1 = min(ex1, x);
                ey1 = min(ey1, y);
                ex2 = max(ex2, x);
                ey2 = max(ey2, y);
            }
            if (cg) {
                gx1 = min(gx1, x);
                gy1 = min(gy1, y);
                gx2 = max(gx2, x);
                gy2 = max(gy2, y);
            }
        }
    }
    // the wave's counts and boxes into LDS (a wave without a covered pixel leaves the identities), then one fold per workgroup
    if (any_e != 0ull) {
        ex1 = wave_min(ex1);
        ey1 = wave_min(ey1);
        ex2 = wave_max(ex2);
        ey2 = wave_max(ey2);
    }
    if (any_g != 0ull) {
        gx1 = wave_min(gx1);
        gy1 = wave_min(gy1);
        gx2 = wave_max(gx2);
        gy2 = wave_max(gy2);
    }
    if ((tid & 63) == 0) {
        if (n_and != 0) atomicAdd(&s_cnt[0], n_and);
        if (n_or != 0) atomicAdd(&s_cnt[1], n_or);
        int* b = s_box[tid >> 6];
        b[0] = ex1;
        b[1] = ey1;
        b[2] = ex2;
        b[3] = ey2;
        b[4] = gx1;
        b[5] = gy1;
        b[6] = gx2;
        b[7] = gy2;
    }
    __syncthreads();
    if (s_cnt[1] == 0) return;                     // uniform over the workgroup: nothing of either silhouette in this chunk, no atomic
    int* a = acc + (size_t)row * CU_ACC;
    if (tid < 2 && s_cnt[tid] != 0) atomicAdd(a + tid, s_cnt[tid]);
    if (tid < 8) {                                 // thread k: bound k of (est x1 y1 x2 y2, gt x1 y1 x2 y2) over the waves
        const bool lower = (tid & 3) < 2;
        int v = s_box[0][tid];
#pragma unroll
        for (int w = 1; w < CU_WAVES; ++w) v = lower ? min(v, s_box[w][tid]) : max(v, s_box[w][tid]);
        if (lower) {
            if (v != INT_MAX) atomicMin(a + 2 + tid, v);
        } else {
            if (v != INT_MIN) atomicMax(a + 2 + tid, v);
        }
    }
}

// misc.iou (lib/pysixd/misc.py:809-836) of two x, y, w, h boxes, operation for operation in fp64: corners x + w, the intersection counted only
// when both of its sides are > 0, the denominator (area_a + area_b) - area_inter.  A NaN anywhere gives 0.
__device__ __forceinline__ double iou_xywh(const double* a, const double* b) {
#pragma unroll
    for (int k = 0; k < 4; ++k)
        if (a[k] != a[k] || b[k] != b[k]) return 0.0;
    const double brax = a[0] + a[2], bray = a[1] + a[3], brbx = b[0] + b[2], brby = b[1] + b[3];
    const double tlx = fmax(a[0], b[0]), tly = fmax(a[1], b[1]);
    const double brx = fmin(brax, brbx), bry = fmin(bray, brby);
    const double w = brx - tlx, h = bry - tly;
    if (!(w > 0.0 && h > 0.0)) return 0.0;
    const double area_inter = w * h, area_a = a[2] * a[3], area_b = b[2] * b[3];
    return area_inter / ((area_a + area_b) - area_inter);
}

// One thread per row: counts, the boxes with the empty encoding (0, 0, -1, -1), and the two errors.
__global__ __launch_bounds__(CU_THREADS) void cou_finalize_kernel(const int* __restrict__ acc, int N, double* __restrict__ err,
                                                                  int* __restrict__ counts, int* __restrict__ boxes) {
    const int i = blockIdx.x * CU_THREADS + threadIdx.x;
    if (i >= N) return;
    const int* a = acc + (size_t)i * CU_ACC;
    const int n_and = a[0], n_or = a[1];
    counts[(size_t)i * 2 + 0] = n_and;
    counts[(size_t)i * 2 + 1] = n_or;
    double xywh[2][4];
    bool empty[2];
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        int x1 = a[2 + 4 * k + 0], y1 = a[2 + 4 * k + 1], x2 = a[2 + 4 * k + 2], y2 = a[2 + 4 * k + 3];
        empty[k] = x2 == INT_MIN;
        if (empty[k]) {
            x1 = 0;
            y1 = 0;
            x2 = -1;
            y2 = -1;
        }
        int* b = boxes + (size_t)i * 8 + 4 * k;
        b[0] = x1;
        b[1] = y1;
        b[2] = x2;
        b[3] = y2;
        xywh[k][0] = (double)x1;                   // misc.calc_2d_bbox_xywh, clip=False
        xywh[k][1] = (double)y1;
        xywh[k][2] = (double)(x2 - x1 + 1);
        xywh[k][3] = (double)(y2 - y1 + 1);
    }
    err[(size_t)i * 2 + 0] = n_or > 0 ? 1.0 - (double)n_and / (double)n_or : 1.0;
    err[(size_t)i * 2 + 1] = (empty[0] || empty[1]) ? 1.0 : 1.0 - iou_xywh(xywh[0], xywh[1]);
}

__global__ __launch_bounds__(CU_THREADS) void cou_bb_kernel(const double* __restrict__ bb_est, const double* __restrict__ bb_gt, int N,
                                                            double* __restrict__ err) {
    const int i = blockIdx.x * CU_THREADS + threadIdx.x;
    if (i >= N) return;
    double a[4], b[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        a[k] = bb_est[(size_t)i * 4 + k];
        b[k] = bb_gt[(size_t)i * 4 + k];
    }
    err[i] = 1.0 - iou_xywh(a, b);
}

}  // namespace

extern "C" long long gdrn_cou_maps_workspace_bytes(int N) {
    if (N < 0) return GDRN_ERR_ARG;
    return (long long)N * CU_ACC * (long long)sizeof(int);
}

extern "C" int gdrn_cou_maps(const void* est, const void* gt, int kind, int N, int H, int W, double* err, int* counts, int* boxes, void* workspace,
                             void* stream) {
    if (kind != GDRN_COU_DEPTH && kind != GDRN_COU_MASK) return GDRN_ERR_ARG;
    if (N < 0 || H < 1 || W < 1) return GDRN_ERR_ARG;
    const long long hw = (long long)H * W;
    if (hw > 0x7fffffffLL - CU_CHUNK) return GDRN_ERR_ARG;   // H * W in an int, with room for a chunk
    if (N == 0) return GDRN_OK;
    if (!est || !gt || !err || !counts || !boxes || !workspace) return GDRN_ERR_ARG;
    const long long bpi = (hw + CU_CHUNK - 1) / CU_CHUNK;
    if ((long long)N * bpi > 0x7fffffffLL) return GDRN_ERR_SHAPE;   // the workgroups of the pixel pass within a grid dimension
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    int* acc = reinterpret_cast<int*>(workspace);
    GDRN_LAUNCH(cou_init_kernel, dim3(cdiv(N, CU_THREADS)), dim3(CU_THREADS), 0, st, acc, N);
    GDRN_CHECK_LAUNCH();
    const dim3 grid((unsigned)((long long)N * bpi));
    if (kind == GDRN_COU_DEPTH)
        GDRN_LAUNCH(cou_pixels_kernel<unsigned>, grid, dim3(CU_THREADS), 0, st, reinterpret_cast<const unsigned*>(est),
                    reinterpret_cast<const unsigned*>(gt), (int)hw, W, (int)bpi, acc);
    else
        GDRN_LAUNCH(cou_pixels_kernel<unsigned char>, grid, dim3(CU_THREADS), 0, st, reinterpret_cast<const unsigned char*>(est),
                    reinterpret_cast<const unsigned char*>(gt), (int)hw, W, (int)bpi, acc);
    GDRN_CHECK_LAUNCH();
    GDRN_LAUNCH(cou_finalize_kernel, dim3(cdiv(N, CU_THREADS)), dim3(CU_THREADS), 0, st, acc, N, err, counts, boxes);
    GDRN_CHECK_LAUNCH();
    return GDRN_OK;
}

extern "C" int gdrn_cou_bb(const double* bb_est, const double* bb_gt, int N, double* err, void* stream) {
    if (N < 0) return GDRN_ERR_ARG;
    if (N == 0) return GDRN_OK;
    if (!bb_est || !bb_gt || !err) return GDRN_ERR_ARG;
    GDRN_LAUNCH(cou_bb_kernel, dim3(cdiv(N, CU_THREADS)), dim3(CU_THREADS), 0, reinterpret_cast<hipStream_t>(stream), bb_est, bb_gt, N, err);
    GDRN_CHECK_LAUNCH();
    return GDRN_OK;
}
