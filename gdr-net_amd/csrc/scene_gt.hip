// Per-instance scene ground truth for gfx950: what the BOP toolkit's offline pass writes next to a dataset and every dataset file under
// core/gdrn_modeling/datasets/ reads back (lm_pbr.py:143-178) -- mask/*.png, mask_visib/*.png and the records of scene_gt_info.json (bbox_obj,
// bbox_visib, px_count_all, px_count_valid, px_count_visib, visib_fract) -- from depth renders that are already on the device:
//   the instance rendered on a canvas with a margin round the image (gdrn_render_depth)         -> gdrn_scene_gt_canvas
//   the scene depth of a frame without a depth image: the nearest of its annotated instances    -> gdrn_scene_gt_compose
//   visibility._estimate_visib_mask (lib/pysixd/visibility.py:29-36, "bop19" and "bop18") on
//   misc.depth_im_to_dist_im_fast distances, the counts, the boxes and the fraction             -> gdrn_scene_gt_visibility
// The rules are stated with the entry points in include/gdrn_hip.h.  All three are pixel passes that read every depth value once and write every
// output once; counts are ballots / popcounts gathered in LDS and added with one integer atomic per workgroup and counter, bounds are wave
// minima / maxima finished with integer atomicMin / atomicMax: no floating-point atomics, repeated calls give the same bits.  A thread's pixels
// are a flat index into the map, so waves straddle rows and the edges of the window; no width needs to be a multiple of anything.
//
// Floating-point contraction is OFF for this file, as in bop_metrics.hip, whose distance (dist64.h) and visibility difference (on the fp32
// casts) this shares.  (No 16-bit code: both library builds compile the same thing.)
#include "common.h"
#include "geom64.h"
#include "dist64.h"
#include "../../include/gdrn_hip.h"

#include <limits.h>

#pragma clang fp contract(off)

namespace {

constexpr int SG_THREADS = 256;
constexpr int SG_WAVES = SG_THREADS / 64;
constexpr int SG_PPT = 8;                          // pixels per thread
constexpr int SG_CHUNK = SG_THREADS * SG_PPT;      // pixels per workgroup
constexpr int SG_MAX_SIDE = 1 << 20;               // image side and margin: coordinates stay far inside an int

struct Box { int x1, y1, x2, y2; };

__device__ __forceinline__ Box box_empty() { return Box{INT_MAX, INT_MAX, INT_MIN, INT_MIN}; }
__device__ __forceinline__ void box_add(Box& b, int x, int y) {
    b.x1 = min(b.x1, x);
    b.y1 = min(b.y1, y);
    b.x2 = max(b.x2, x);
    b.y2 = max(b.y2, y);
}
__device__ __forceinline__ Box wave_box(Box b) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        b.x1 = min(b.x1, __shfl_xor(b.x1, o, 64));
        b.y1 = min(b.y1, __shfl_xor(b.y1, o, 64));
        b.x2 = max(b.x2, __shfl_xor(b.x2, o, 64));
        b.y2 = max(b.y2, __shfl_xor(b.y2, o, 64));
    }
    return b;
}

// The workgroup's box into the row's running box: lane 0 of every wave leaves its wave's box in LDS, the first four threads fold the waves and
// issue one atomic each.  `any` (uniform over the workgroup) says whether there is anything to add.  s_box: SG_WAVES x 4 ints of LDS.
__device__ __forceinline__ void block_box_to_global(Box b, int (*s_box)[4], int* __restrict__ out) {
    const int tid = threadIdx.x;
    b = wave_box(b);
    if ((tid & 63) == 0) {
        s_box[tid >> 6][0] = b.x1;
        s_box[tid >> 6][1] = b.y1;
        s_box[tid >> 6][2] = b.x2;
        s_box[tid >> 6][3] = b.y2;
    }
    __syncthreads();
    if (tid < 4) {
        int v = s_box[0][tid];
#pragma unroll
        for (int w = 1; w < SG_WAVES; ++w) v = tid < 2 ? min(v, s_box[w][tid]) : max(v, s_box[w][tid]);
        if (tid < 2) {
            if (v != INT_MAX) atomicMin(out + tid, v);
        } else {
            if (v != INT_MIN) atomicMax(out + tid, v);
        }
    }
}

// counts[n] = 0, boxes[n] = the empty running box
__global__ __launch_bounds__(SG_THREADS) void sg_init_kernel(int* __restrict__ c0, int* __restrict__ c1, int* __restrict__ box, int n) {
    const int i = blockIdx.x * SG_THREADS + threadIdx.x;
    if (i >= n) return;
    c0[i] = 0;
    if (c1) c1[i] = 0;
    box[i * 4 + 0] = INT_MAX;
    box[i * 4 + 1] = INT_MAX;
    box[i * 4 + 2] = INT_MIN;
    box[i * 4 + 3] = INT_MIN;
}

// Workgroup (chunk of SG_CHUNK canvas pixels, instance).  The canvas is (H + 2 py) x Wc, Wc = W + 2 px; the image is its central window.
__global__ __launch_bounds__(SG_THREADS) void sg_canvas_kernel(const float* __restrict__ canvas, int HWc, int Wc, int H, int W, int px, int py,
                                                               float* __restrict__ depth, int* __restrict__ count_all,
                                                               int* __restrict__ bbox_obj) {
    __shared__ int s_cnt;
    __shared__ int s_box[SG_WAVES][4];
    const int row = blockIdx.y, tid = threadIdx.x, lane = tid & 63;
    const int p0 = blockIdx.x * SG_CHUNK + tid;
    if (tid == 0) s_cnt = 0;
    __syncthreads();
    const float* src = canvas + (size_t)row * HWc;
    float* dst = depth + (size_t)row * H * W;
    float z[SG_PPT];
#pragma unroll
    for (int u = 0; u < SG_PPT; ++u) {   // all loads first: eight in flight per lane
        const int p = p0 + u * SG_THREADS;
        z[u] = p < HWc ? src[p] : 0.f;
    }
    Box b = box_empty();
    int cnt = 0;
#pragma unroll
    for (int u = 0; u < SG_PPT; ++u) {
        const int p = p0 + u * SG_THREADS;   // (beyond the canvas: z = 0 and a row below the window, so nothing below fires)
        const int yc = p / Wc, xc = p - yc * Wc;
        const int x = xc - px, y = yc - py;   // image coordinates
        if (x >= 0 && x < W && y >= 0 && y < H) dst[y * W + x] = z[u];
        if (z[u] != 0.f) box_add(b, x, y);
        cnt += __popcll(__ballot(z[u] != 0.f));   // uniform over the wave
    }
    if (lane == 0 && cnt != 0) atomicAdd(&s_cnt, cnt);
    __syncthreads();
    if (s_cnt == 0) return;   // uniform over the workgroup: nothing of the object in this chunk
    if (tid == 0) atomicAdd(count_all + row, s_cnt);
    block_box_to_global(b, s_box, bbox_obj + (size_t)row * 4);
}

// Workgroup (chunk of SG_CHUNK image pixels, frame): the smallest non-zero depth over the frame's instances inst[off[f] .. off[f + 1]).  A minimum:
// the order of the list does not matter.  A frame without instances is all 0.
__global__ __launch_bounds__(SG_THREADS) void sg_compose_kernel(const float* __restrict__ depth, const int* __restrict__ off,
                                                                const int* __restrict__ inst, int N, int HW, float* __restrict__ scene) {
    const int f = blockIdx.y;
    const int p0 = blockIdx.x * SG_CHUNK + threadIdx.x;
    const int j0 = off[f], j1 = off[f + 1];
    float best[SG_PPT];
#pragma unroll
    for (int u = 0; u < SG_PPT; ++u) best[u] = 0.f;
    for (int j = j0; j < j1; ++j) {
        const int i = inst[j];
        if (i < 0 || i >= N) continue;   // (the host side of the entry point refuses such a table before the launch)
        const float* d = depth + (size_t)i * HW;
#pragma unroll
        for (int u = 0; u < SG_PPT; ++u) {
            const int p = p0 + u * SG_THREADS;
            const float z = p < HW ? d[p] : 0.f;
            if (z != 0.f && (best[u] == 0.f || z < best[u])) best[u] = z;
        }
    }
#pragma unroll
    for (int u = 0; u < SG_PPT; ++u) {
        const int p = p0 + u * SG_THREADS;
        if (p < HW) scene[(size_t)f * HW + p] = best[u];
    }
}

// Workgroup (chunk of SG_CHUNK image pixels, instance): mask = depth != 0; the two distances and the mode's rule where the mask is set.
__global__ __launch_bounds__(SG_THREADS) void sg_visib_kernel(const float* __restrict__ depth, const float* __restrict__ scene,
                                                              const int* __restrict__ frame, int F, const double* __restrict__ Km, int HW, int W,
                                                              float delta, int bop18, unsigned char* __restrict__ mask,
                                                              unsigned char* __restrict__ mask_visib, int* __restrict__ count_valid,
                                                              int* __restrict__ count_visib, int* __restrict__ bbox_visib) {
    __shared__ int s_cnt[2];
    __shared__ int s_box[SG_WAVES][4];
    const int row = blockIdx.y, tid = threadIdx.x, lane = tid & 63;
    const int f = frame[row];
    if (f < 0 || f >= F) return;   // (the host side of the entry point refuses such a frame before the launch)
    const int p0 = blockIdx.x * SG_CHUNK + tid;
    if (tid < 2) s_cnt[tid] = 0;
    __syncthreads();
    const double* K = Km + (size_t)row * 9;
    const double fx = K[0], cx = K[2], fy = K[4], cy = K[5];
    const float* dg = depth + (size_t)row * HW;
    const float* ds = scene + (size_t)f * HW;
    unsigned char* m = mask + (size_t)row * HW;
    unsigned char* mv = mask_visib + (size_t)row * HW;
    float zg[SG_PPT], zs[SG_PPT];
#pragma unroll
    for (int u = 0; u < SG_PPT; ++u) {
        const int p = p0 + u * SG_THREADS;
        zg[u] = p < HW ? dg[p] : 0.f;
        zs[u] = p < HW ? ds[p] : 0.f;
    }
    Box b = box_empty();
    int n_valid = 0, n_visib = 0;
#pragma unroll
    for (int u = 0; u < SG_PPT; ++u) {
        const int p = p0 + u * SG_THREADS;
        const bool cov = zg[u] != 0.f;
        bool vis = false;
        if (cov) {
            const int y = p / W, x = p - y * W;
            const double X = ((double)x - cx) / fx, Y = ((double)y - cy) / fy;
            const double dist_g = dist_of(X, Y, zg[u]), dist_s = dist_of(X, Y, zs[u]);
            const float diff = (float)dist_g - (float)dist_s;   // visibility.py:31,35: on the fp32 casts
            vis = bop18 ? (dist_s > 0.0 && dist_g > 0.0 && diff <= delta) : ((diff <= delta || dist_s == 0.0) && dist_g > 0.0);
            if (vis) box_add(b, x, y);
        }
        if (p < HW) {
            m[p] = cov ? 1 : 0;
            mv[p] = vis ? 1 : 0;
        }
        n_valid += __popcll(__ballot(cov && zs[u] > 0.f));
        n_visib += __popcll(__ballot(vis));
    }
    if (lane == 0) {
        if (n_valid != 0) atomicAdd(&s_cnt[0], n_valid);
        if (n_visib != 0) atomicAdd(&s_cnt[1], n_visib);
    }
    __syncthreads();
    if (tid == 0 && s_cnt[0] != 0) atomicAdd(count_valid + row, s_cnt[0]);
    if (s_cnt[1] == 0) return;   // uniform over the workgroup
    if (tid == 0) atomicAdd(count_visib + row, s_cnt[1]);
    block_box_to_global(b, s_box, bbox_visib + (size_t)row * 4);
}

// One thread per instance: the empty-box encoding (0, 0, -1, -1) and visib_fract = px_count_visib / px_count_all, 0 for an empty canvas.
__global__ __launch_bounds__(SG_THREADS) void sg_finish_kernel(const int* __restrict__ count_all, const int* __restrict__ count_visib,
                                                               int* __restrict__ bbox_obj, int* __restrict__ bbox_visib,
                                                               double* __restrict__ visib_fract, int N) {
    const int i = blockIdx.x * SG_THREADS + threadIdx.x;
    if (i >= N) return;
    const int all = count_all[i], vis = count_visib[i];
    int* boxes[2] = {bbox_obj + (size_t)i * 4, bbox_visib + (size_t)i * 4};
    const int cnt[2] = {all, vis};
#pragma unroll
    for (int k = 0; k < 2; ++k)
        if (cnt[k] <= 0) {
            boxes[k][0] = 0;
            boxes[k][1] = 0;
            boxes[k][2] = -1;
            boxes[k][3] = -1;
        }
    visib_fract[i] = all > 0 ? (double)vis / (double)all : 0.0;
}

bool sg_sizes_ok(int N, int H, int W, int px, int py) {
    return N > 0 && H > 0 && W > 0 && px >= 0 && py >= 0 && H <= SG_MAX_SIDE && W <= SG_MAX_SIDE && px <= SG_MAX_SIDE && py <= SG_MAX_SIDE;
}

// what the launches can index: the canvas in an int with room for a chunk, instances in grid.y
bool sg_sizes_fit(int N, int H, int W, int px, int py) {
    return ((long long)H + 2LL * py) * ((long long)W + 2LL * px) <= 0x7fffffffLL - SG_CHUNK && N <= 65535;
}

int sg_chunks(long long pixels) { return (int)((pixels + SG_CHUNK - 1) / SG_CHUNK); }

}  // namespace

extern "C" int gdrn_scene_gt_canvas(const float* canvas, int N, int H, int W, int pad_x, int pad_y, float* depth, int* px_count_all, int* bbox_obj,
                                    void* stream) {
    if (!canvas || !depth || !px_count_all || !bbox_obj) return GDRN_ERR_ARG;
    if (!sg_sizes_ok(N, H, W, pad_x, pad_y)) return GDRN_ERR_ARG;
    if (!sg_sizes_fit(N, H, W, pad_x, pad_y)) return GDRN_ERR_SHAPE;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const int Wc = W + 2 * pad_x, HWc = (H + 2 * pad_y) * Wc;
    GDRN_LAUNCH(sg_init_kernel, dim3(cdiv(N, SG_THREADS)), dim3(SG_THREADS), 0, st, px_count_all, (int*)nullptr, bbox_obj, N);
    GDRN_CHECK_LAUNCH();
    GDRN_LAUNCH(sg_canvas_kernel, dim3(sg_chunks(HWc), N), dim3(SG_THREADS), 0, st, canvas, HWc, Wc, H, W, pad_x, pad_y, depth, px_count_all,
                bbox_obj);
    GDRN_CHECK_LAUNCH();
    return GDRN_OK;
}

extern "C" int gdrn_scene_gt_compose(const float* depth, const int* inst_off, const int* inst_off_host, const int* inst, const int* inst_host, int F,
                                     int N, int H, int W, float* depth_scene, void* stream) {
    if (!depth || !inst_off || !inst_off_host || !inst || !inst_host || !depth_scene) return GDRN_ERR_ARG;
    if (!sg_sizes_ok(N, H, W, 0, 0) || F <= 0) return GDRN_ERR_ARG;
    if (inst_off_host[0] != 0 || inst_off_host[F] != N) return GDRN_ERR_ARG;
    for (int f = 0; f < F; ++f)
        if (inst_off_host[f + 1] < inst_off_host[f]) return GDRN_ERR_ARG;
    if (!host_in_range(inst_host, N, N)) return GDRN_ERR_ARG;
    if (!sg_sizes_fit(N, H, W, 0, 0) || F > 65535) return GDRN_ERR_SHAPE;
    GDRN_LAUNCH(sg_compose_kernel, dim3(sg_chunks((long long)H * W), F), dim3(SG_THREADS), 0, reinterpret_cast<hipStream_t>(stream), depth, inst_off,
                inst, N, H * W, depth_scene);
    GDRN_CHECK_LAUNCH();
    return GDRN_OK;
}

extern "C" int gdrn_scene_gt_visibility(const float* depth, const float* depth_scene, const int* frame, const int* frame_host, int F, const double* K,
                                        int N, int H, int W, double delta, int visib_mode, unsigned char* mask, unsigned char* mask_visib,
                                        const int* px_count_all, int* px_count_valid, int* px_count_visib, int* bbox_obj, int* bbox_visib,
                                        double* visib_fract, void* stream) {
    if (!depth || !depth_scene || !frame || !frame_host || !K || !mask || !mask_visib || !px_count_all || !px_count_valid || !px_count_visib ||
        !bbox_obj || !bbox_visib || !visib_fract)
        return GDRN_ERR_ARG;
    if (!sg_sizes_ok(N, H, W, 0, 0) || F <= 0 || !(delta >= 0.0)) return GDRN_ERR_ARG;
    if (visib_mode != GDRN_VISIB_BOP19 && visib_mode != GDRN_VISIB_BOP18) return GDRN_ERR_ARG;
    if (!host_in_range(frame_host, N, F)) return GDRN_ERR_ARG;
    if (!sg_sizes_fit(N, H, W, 0, 0)) return GDRN_ERR_SHAPE;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    GDRN_LAUNCH(sg_init_kernel, dim3(cdiv(N, SG_THREADS)), dim3(SG_THREADS), 0, st, px_count_valid, px_count_visib, bbox_visib, N);
    GDRN_CHECK_LAUNCH();
    GDRN_LAUNCH(sg_visib_kernel, dim3(sg_chunks((long long)H * W), N), dim3(SG_THREADS), 0, st, depth, depth_scene, frame, F, K, H * W, W,
                (float)delta, visib_mode == GDRN_VISIB_BOP18 ? 1 : 0, mask, mask_visib, px_count_valid, px_count_visib, bbox_visib);
    GDRN_CHECK_LAUNCH();
    GDRN_LAUNCH(sg_finish_kernel, dim3(cdiv(N, SG_THREADS)), dim3(SG_THREADS), 0, st, px_count_all, px_count_visib, bbox_obj, bbox_visib,
                visib_fract, N);
    GDRN_CHECK_LAUNCH();
    return GDRN_OK;
}
