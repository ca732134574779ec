// Coarse depth alignment of estimated poses for gfx950, the step in front of the ICP of icp.hip: shift every estimate along its viewing ray by
// the MEDIAN difference between the observed and the rendered depth --
//   (rendered depth, observed depth) -> the median offset, the pair and coverage counts of every estimate    -> gdrn_depth_offset
//   render, offset, shift, `rounds` times on one stream without a host read                                 -> gdrn_depth_align
// The reference has no counterpart (it is RGB-only); the arithmetic is stated with the entry points in include/gdrn_hip.h and restated on the
// host in tests/align_host.py.
//
// The median is an exact order statistic: ranks (n - 1) / 2 and n / 2 of the n differences of an instance's pairs.  Two launches find them:
//
// The compact pass: one workgroup per (instance, band of DA_BAND_ROWS rows), laid out as icp_accumulate_kernel is.  A lane walks the band with
// stride 256, DA_PPT render depths in flight, reads the observed depth only where the render is covered, and appends the order-preserving key of
// every pair's difference to a stage in LDS (an integer LDS atomic hands out the slot).  A stage that could overflow at the next step, and the
// last one, are flushed: ONE integer atomicAdd on the instance's cursor reserves the range of its key list in the workspace, coalesced stores
// fill it.  The renders and the frames are streamed once; the list of an instance holds its pairs in an order that changes from call to call,
// which no rank depends on.
//
// The select pass: one workgroup per instance, radix selection over its list in three levels of 11 + 11 + 10 bits.  Per level an integer
// histogram in LDS of the keys that carry the prefix fixed so far, then one wave per rank scans the bins (256 partial sums, a shuffle scan over
// 64 lanes, a walk of at most 4 + 8 entries).  The two ranks are followed independently -- with an even n they can part at any level, the first
// included -- and share one histogram for as long as their prefixes agree.  The last level yields the two keys, hence the two values.
//
// Only integer atomics: the same call gives the same bits, and the instances of a batch cannot influence each other.  The shift kernel, one
// lane per instance, applies the offset and writes the outputs.
//
// Floating-point contraction is OFF for this file: the shift is one fixed operation sequence, which the host restatement repeats.
// (No 16-bit code: both library builds compile the same thing.)
#include "common.h"
#include "geom64.h"
#include "../../include/gdrn_hip.h"

#pragma clang fp contract(off)

#include "render_loop.h"

namespace {

constexpr int DA_THREADS = 256;
constexpr int DA_BAND_ROWS = 16;                  // rows of one workgroup's band
constexpr int DA_PPT = 4;                         // render depths a lane loads before it looks at any of them
constexpr int DA_CHUNK = DA_THREADS * DA_PPT;     // pixels of one step of the band walk: the most keys a step can add
constexpr int DA_STAGE = 2 * DA_CHUNK;            // keys the LDS stage holds
constexpr int DA_SEL_THREADS = 1024;
constexpr int DA_PARTS = 256;                     // partial sums per histogram
constexpr int DA_BINS = 2048;                     // bins of the widest level

__host__ __device__ __forceinline__ int da_bands(int H) { return (H + DA_BAND_ROWS - 1) / DA_BAND_ROWS; }

// Order-preserving map of the fp32 bits to unsigned: the sign bit of a non-negative flipped, all bits of a negative inverted.  (-0.0 would sort
// below +0.0 here; it cannot arise: a difference sc - ren of two positive values that is zero is +0.0 in round-to-nearest.)
__device__ __forceinline__ unsigned da_key(float d) {
    const unsigned b = __float_as_uint(d);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float da_value(unsigned k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k); }

__device__ __forceinline__ double da_nan() { return __longlong_as_double(0x7ff8000000000000LL); }

// the stage's `fill` keys into the instance's list behind one reservation; every lane of the workgroup calls it (fill is uniform)
__device__ __forceinline__ void da_flush(const unsigned* stage, int fill, int* cursor, unsigned* list, int* s_base) {
    const int tid = threadIdx.x;
    if (tid == 0) *s_base = atomicAdd(cursor, fill);
    __syncthreads();
    const int base = *s_base;
    for (int k = tid; k < fill; k += DA_THREADS) list[base + k] = stage[k];
    __syncthreads();
}

// Workgroup (band, instance): pixels [y0 * W, y1 * W) of the instance's render.  keys [N][H * W] uint32, cnt [N][2] int32 = (pairs, covered),
// zero before the launch.  state (NULL: every instance runs) [N] int32: an instance whose state is not 0 is frozen and left alone.
__global__ __launch_bounds__(DA_THREADS) void da_compact_kernel(const float* __restrict__ depth_ren, const float* __restrict__ depth_scene,
                                                                 const int* __restrict__ frame, int F, int H, int W, double gate,
                                                                 const int* __restrict__ state, unsigned* __restrict__ keys, int* __restrict__ cnt) {
    __shared__ unsigned stage[DA_STAGE];
    __shared__ int s_fill, s_base, red_c[DA_THREADS / 64];
    const int band = blockIdx.x, i = blockIdx.y, tid = threadIdx.x;
    if (state != nullptr && state[i] != 0) return;   // uniform over the workgroup
    const int f = frame[i];
    if (f < 0 || f >= F) return;                     // (the host side of the entry point refuses such a frame before the launch)
    const int y0 = band * DA_BAND_ROWS, y1 = min(y0 + DA_BAND_ROWS, H);
    const float* ren = depth_ren + (size_t)i * H * W;
    const float* sc = depth_scene + (size_t)f * H * W;
    unsigned* list = keys + (size_t)i * H * W;
    if (tid == 0) s_fill = 0;
    __syncthreads();
    const int p1 = y1 * W;
    int covered = 0, fill = 0;
    for (int q = y0 * W; q < p1; q += DA_CHUNK) {    // a uniform trip count: the body holds barriers
        float z[DA_PPT], s[DA_PPT];
#pragma unroll
        for (int u = 0; u < DA_PPT; ++u) {           // all render loads first: DA_PPT in flight per lane
            const int p = q + tid + u * DA_THREADS;
            z[u] = p < p1 ? ren[p] : 0.f;
        }
#pragma unroll
        for (int u = 0; u < DA_PPT; ++u) s[u] = z[u] > 0.f ? sc[q + tid + u * DA_THREADS] : 0.f;
#pragma unroll
        for (int u = 0; u < DA_PPT; ++u) {
            if (!(z[u] > 0.f)) continue;
            ++covered;
            if (!(s[u] > 0.f)) continue;
            const float d = s[u] - z[u];             // one fp32 subtraction
            if (!(fabs((double)d) <= gate)) continue;
            stage[atomicAdd(&s_fill, 1)] = da_key(d);
        }
        __syncthreads();
        fill = s_fill;
        __syncthreads();                             // every lane has read s_fill before one of them adds to it again
        if (fill > DA_STAGE - DA_CHUNK) {            // uniform: the next step might not fit
            da_flush(stage, fill, cnt + (size_t)i * 2, list, &s_base);
            if (tid == 0) s_fill = 0;
            fill = 0;
            __syncthreads();
        }
    }
    if (fill > 0) da_flush(stage, fill, cnt + (size_t)i * 2, list, &s_base);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) covered += __shfl_xor(covered, o, 64);
    if ((tid & 63) == 0) red_c[tid >> 6] = covered;
    __syncthreads();
    if (tid == 0) {
        const int total = (red_c[0] + red_c[1]) + (red_c[2] + red_c[3]);
        if (total > 0) atomicAdd(cnt + (size_t)i * 2 + 1, total);
    }
}

// One workgroup per instance: the keys of ranks (n - 1) / 2 and n / 2 of its list, off_tmp[i] = half the sum of their values.  An instance with
// fewer than min_pairs pairs, or a frozen one, is left alone (the shift kernel reads the count itself).
__global__ __launch_bounds__(DA_SEL_THREADS) void da_select_kernel(const unsigned* __restrict__ keys, const int* __restrict__ cnt, int HW,
                                                                    int min_pairs, const int* __restrict__ state, double* __restrict__ off_tmp) {
    __shared__ unsigned hist[2][DA_BINS];
    __shared__ unsigned part[2][DA_PARTS];
    __shared__ unsigned s_bin[2], s_rank[2];
    const int i = blockIdx.x, tid = threadIdx.x;
    if (state != nullptr && state[i] != 0) return;   // uniform over the workgroup
    const int n = cnt[(size_t)i * 2];
    if (n < min_pairs || n < 1) return;
    const unsigned* list = keys + (size_t)i * HW;
    unsigned rank[2] = {(unsigned)(n - 1) / 2u, (unsigned)n / 2u};
    unsigned prefix[2] = {0u, 0u};
#pragma unroll 1
    for (int level = 0; level < 3; ++level) {
        const int shift = level == 0 ? 21 : level == 1 ? 10 : 0;
        const int bits = level == 2 ? 10 : 11;
        const unsigned nbins = 1u << bits;
        const bool same = prefix[0] == prefix[1];    // one histogram serves both ranks
        for (int k = tid; k < 2 * DA_BINS; k += DA_SEL_THREADS) (&hist[0][0])[k] = 0u;
        __syncthreads();
        for (int k = tid; k < n; k += DA_SEL_THREADS) {
            const unsigned key = list[k];
            const unsigned upper = level == 0 ? 0u : key >> (shift + bits);   // the bits the levels before this one fixed
            const unsigned bin = (key >> shift) & (nbins - 1u);
            if (upper == prefix[0]) atomicAdd(&hist[0][bin], 1u);
            if (!same && upper == prefix[1]) atomicAdd(&hist[1][bin], 1u);
        }
        __syncthreads();
        const int per = (int)nbins / DA_PARTS;   // 8 or 4 bins to a partial sum
        if (tid < 2 * DA_PARTS) {
            const int h = tid / DA_PARTS, c = tid % DA_PARTS;
            unsigned sum = 0u;
            for (int j = 0; j < per; ++j) sum += hist[h][c * per + j];
            part[h][c] = sum;
        }
        __syncthreads();
        if (tid < 128) {                              // wave 0 follows the lower rank, wave 1 the upper
            const int r = tid >> 6, lane = tid & 63, h = same ? 0 : r;
            const unsigned target = r ? rank[1] : rank[0];
            unsigned sum = 0u;
            for (int j = 0; j < 4; ++j) sum += part[h][lane * 4 + j];
            unsigned incl = sum;
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const unsigned v = __shfl_up(incl, o, 64);
                if (lane >= o) incl += v;
            }
            const unsigned excl = incl - sum;
            if (excl <= target && target < incl) {    // one lane: the counts of the lanes before it do not reach the rank, its own do
                unsigned rem = target - excl;
                int c = lane * 4;
                for (int j = 0; j < 3 && rem >= part[h][c]; ++j) rem -= part[h][c++];
                int bin = c * per;
                for (int j = 0; j < per - 1 && rem >= hist[h][bin]; ++j) rem -= hist[h][bin++];
                s_bin[r] = (unsigned)bin;
                s_rank[r] = rem;
            }
        }
        __syncthreads();
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            prefix[r] = (prefix[r] << bits) | s_bin[r];
            rank[r] = s_rank[r];
        }
    }
    if (tid == 0) off_tmp[i] = 0.5 * ((double)da_value(prefix[0]) + (double)da_value(prefix[1]));
}

// the defaults of an instance no round was evaluated for (rounds == 0), and the running state
__global__ __launch_bounds__(DA_THREADS) void da_init_kernel(int N, int* __restrict__ state, int* __restrict__ ok, int* __restrict__ pairs,
                                                              int* __restrict__ covered, double* __restrict__ offset) {
    const int i = blockIdx.x * DA_THREADS + threadIdx.x;
    if (i >= N) return;
    state[i] = 0;
    ok[i] = 1;
    pairs[i] = 0;
    covered[i] = 0;
    offset[i] = da_nan();
}

// One lane per instance: the outputs of this round, and (t != NULL) the shift along the viewing ray.  A frozen instance is left alone, outputs
// included; an instance with too few pairs is frozen (state != NULL) and keeps its translation bit for bit.
__global__ __launch_bounds__(DA_THREADS) void da_shift_kernel(int N, const int* __restrict__ cnt, const double* __restrict__ off_tmp, int min_pairs,
                                                               double* __restrict__ tv, int* __restrict__ state, int* __restrict__ ok,
                                                               int* __restrict__ pairs, int* __restrict__ covered, double* __restrict__ offset) {
    const int i = blockIdx.x * DA_THREADS + threadIdx.x;
    if (i >= N) return;
    if (state != nullptr && state[i] != 0) return;
    const int n = cnt[(size_t)i * 2];
    pairs[i] = n;
    covered[i] = cnt[(size_t)i * 2 + 1];
    if (n < min_pairs) {
        ok[i] = 0;
        offset[i] = da_nan();
        if (state != nullptr) state[i] = 1;
        return;
    }
    const double off = off_tmp[i];
    ok[i] = 1;
    offset[i] = off;
    if (tv == nullptr) return;
    double* t = tv + (size_t)i * 3;
    const double tx = t[0], ty = t[1], tz = t[2];
    const double s = off / tz;
    t[0] = tx + s * tx;   // the model origin keeps its image
    t[1] = ty + s * ty;
    t[2] = tz + off;
}

bool da_frame_ok(int N, int H, int W) { return N >= 0 && H >= 1 && W >= 1 && (long long)H * W <= 0x7fffffffLL - DA_CHUNK; }

// the workspace: off_tmp [N] fp64 | cnt [N][2] int32 | state [N] int32 (+ 4 bytes when N is odd) | keys [N][H * W] uint32
struct DaWs {
    double* off_tmp;
    int* cnt;
    int* state;
    unsigned* keys;
};
DaWs da_carve(void* workspace, int N) {
    DaWs w;
    w.off_tmp = reinterpret_cast<double*>(workspace);
    w.cnt = reinterpret_cast<int*>(w.off_tmp + N);
    w.state = w.cnt + (size_t)N * 2;
    w.keys = reinterpret_cast<unsigned*>(w.state + (size_t)N + (N & 1));
    return w;
}

// one evaluation on the maps: clear the counters, compact, select, then the shift kernel (tv and state NULL: outputs only)
int da_launch_offset(const float* depth_ren, const float* depth_scene, const int* frame, int F, int N, int H, int W, double gate, int min_pairs,
                     double* tv, int* state, int* ok, int* pairs, int* covered, double* offset, const DaWs& w, hipStream_t st) {
    if (hipMemsetAsync(w.cnt, 0, (size_t)N * 2 * sizeof(int), st) != hipSuccess) return GDRN_ERR_LAUNCH;
    GDRN_LAUNCH(da_compact_kernel, dim3(da_bands(H), N), dim3(DA_THREADS), 0, st, depth_ren, depth_scene, frame, F, H, W, gate,
                (const int*)state, w.keys, w.cnt);
    GDRN_CHECK_LAUNCH();
    GDRN_LAUNCH(da_select_kernel, dim3(N), dim3(DA_SEL_THREADS), 0, st, (const unsigned*)w.keys, (const int*)w.cnt, H * W, min_pairs,
                (const int*)state, w.off_tmp);
    GDRN_CHECK_LAUNCH();
    GDRN_LAUNCH(da_shift_kernel, dim3(cdiv(N, DA_THREADS)), dim3(DA_THREADS), 0, st, N, (const int*)w.cnt, (const double*)w.off_tmp, min_pairs, tv,
                state, ok, pairs, covered, offset);
    GDRN_CHECK_LAUNCH();
    return GDRN_OK;
}

}  // namespace

extern "C" long long gdrn_depth_align_workspace_bytes(int N, int H, int W) {
    if (!da_frame_ok(N, H, W)) return GDRN_ERR_ARG;
    const long long n = N;
    return n * (long long)sizeof(double) + (n * 3 + (n & 1)) * (long long)sizeof(int) + n * H * W * (long long)sizeof(unsigned);
}

extern "C" int gdrn_depth_offset(const float* depth_ren, const float* depth_scene, const int* frame, const int* frame_host, int F, int N, int H,
                                 int W, double gate, int min_pairs, double* offset, int* pairs, int* covered, int* ok, void* workspace,
                                 void* stream) {
    if (!da_frame_ok(N, H, W) || F < 0 || !(gate > 0.0) || min_pairs < 1) return GDRN_ERR_ARG;
    if (N == 0) return GDRN_OK;
    if (!depth_ren || !depth_scene || !frame || !frame_host || !offset || !pairs || !covered || !ok || !workspace || ((size_t)workspace & 7))
        return GDRN_ERR_ARG;
    if (N > 65535) return GDRN_ERR_SHAPE;   // the instances are the grid's second dimension
    if (!host_in_range(frame_host, N, F)) return GDRN_ERR_ARG;
    const DaWs w = da_carve(workspace, N);
    return da_launch_offset(depth_ren, depth_scene, frame, F, N, H, W, gate, min_pairs, nullptr, nullptr, ok, pairs, covered, offset, w,
                            reinterpret_cast<hipStream_t>(stream));
}

extern "C" int gdrn_depth_align(const double* verts, const int* faces, const int* vert_off, const int* nverts, const int* face_off,
                                const int* nfaces, int C, int f_max, const int* labels, const int* labels_host, const double* R, double* t,
                                const double* K, int N, const float* depth_scene, const int* frame, const int* frame_host, int F, int H, int W,
                                double near, double far, int rounds, double gate, int min_pairs, float* depth_ren_scratch, int* ok, int* pairs,
                                int* covered, double* offset, void* workspace, void* stream) {
    const RenderRows rows = {verts, faces, vert_off, nverts, face_off, nfaces, C, f_max, labels, labels_host, R, t, K, N, H, W, near, far};
    const RenderScene scene = {depth_scene, frame, frame_host, F};
    if (!da_frame_ok(N, H, W) || rounds < 0 || min_pairs < 1 || !(gate > 0.0)) return GDRN_ERR_ARG;
    if (!loop_scalars_ok(rows, scene)) return GDRN_ERR_ARG;
    if (N == 0) return GDRN_OK;
    if (!depth_ren_scratch || !ok || !pairs || !covered || !offset || !workspace || ((size_t)workspace & 7)) return GDRN_ERR_ARG;
    int bad = loop_rows_check(rows, scene);
    if (bad != GDRN_OK) return bad;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const DaWs w = da_carve(workspace, N);
    GDRN_LAUNCH(da_init_kernel, dim3(cdiv(N, DA_THREADS)), dim3(DA_THREADS), 0, st, N, w.state, ok, pairs, covered, offset);
    GDRN_CHECK_LAUNCH();
    for (int r = 0; r < rounds; ++r) {
        bad = render_into(rows, depth_ren_scratch, stream);
        if (bad != GDRN_OK) return bad;
        bad = da_launch_offset(depth_ren_scratch, depth_scene, frame, F, N, H, W, gate, min_pairs, t, w.state, ok, pairs, covered, offset, w, st);
        if (bad != GDRN_OK) return bad;
    }
    return GDRN_OK;
}
