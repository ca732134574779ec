// Silhouette term of the depth refinement for gfx950: the contour of the observed instance mask pulls the contour of the render, which fixes the
// directions a flat-faced object leaves to the point-to-plane term of csrc/icp.hip --
//   (observed mask, observed depth) -> exact squared distance to, and index of, the nearest observed contour pixel  -> gdrn_sil_contour_transform
//   (rendered depth, that transform) -> the 6 x 6 point-to-ray normal equations of every estimate                   -> gdrn_sil_accumulate
//   depth system + weight * silhouette system, then the step of gdrn_icp_step                                        -> gdrn_icp_step_sil
//   the transform once, then render, both accumulations and the combined step `iters` times on one stream           -> gdrn_icp_refine_sil
// The reference has no counterpart; the rules are stated with the entry points in include/gdrn_hip.h and restated on the host in
// tests/sil_host.py.
//
// The transform, three launches, all in integers:
//   contour  one lane per pixel: the 4-neighbour rule and the occluder exclusion -> a byte per pixel; the count by one integer atomic per wave.
//   column   one lane per column walks it down and up: the signed row offset to the nearest contour pixel of the column (the upper one on a
//            tie), SIL_NONE without one.  Lanes are adjacent columns: every step is one coalesced row segment.
//   row      one workgroup per (256 pixels of a row): the row's offsets go through LDS in tiles of SIL_TILE columns (any W), and a lane minimises
//            the key (dx^2 + dy^2, linear index of the contour pixel) over the columns.  The key is a total order, so the walk order is free: a
//            lane starts from its own column and skips every group of SIL_GROUP columns that holds no contour pixel (a ballot while the tile is
//            loaded: most of a row is empty) or lies further away than its best so far.  All lanes of a wave read the same LDS word at a time
//            (a broadcast, no bank conflict).
// A column's nearest contour pixel is the only one of the column that can be the nearest of a pixel of the row, and the upper one of two has the
// smaller index: the minimum over the columns is the minimum over all contour pixels, ties included.
//
// The accumulate pass is the ICP's: one workgroup per (instance, band of 16 rows), 28 fp64 sums and a count per lane, folded in a fixed order
// (xor tree per wave, four waves in LDS) into the band's slab by the ICP's own fold (csrc/icp_shared.h); the slabs are combined in ascending
// order at the next launch boundary, by the same device function in the stand-alone combine and in the step's prologue.  No floating-point
// atomics.
//
// Floating-point contraction is OFF for this file, as for icp.hip.  (No 16-bit code: both library builds compile the same thing.)
#include <climits>

#include "common.h"
#include "geom64.h"
#include "../../include/gdrn_hip.h"

#pragma clang fp contract(off)

#include "raster64.h"
#include "icp_shared.h"
#include "render_loop.h"

namespace {

constexpr int SIL_THREADS = 256;      // lanes of a workgroup of the transform kernels (the accumulate pass has the ICP's launch shape: ICP_*)
constexpr int SIL_TILE = 2048;        // columns of a row held in LDS at a time (8 KiB)
constexpr int SIL_GROUP = 32;         // columns a lane skips or walks as one
constexpr int SIL_NONE = INT_MAX;     // column offset: no contour pixel in the column
constexpr int SIL_MAX_SIDE = 16384;   // 2 * 16383^2 < 2^31: d2 fits
static_assert(SIL_GROUP == 32 && SIL_TILE % SIL_THREADS == 0, "a wave loads two whole groups at a time");

// grid (cdiv(H W, 256), N).  flags [N][H][W] uint8, contour [N] int32 (zeroed before the launch)
__global__ __launch_bounds__(SIL_THREADS) void sil_contour_kernel(const unsigned char* __restrict__ mask, const float* __restrict__ depth_scene,
                                                                   const int* __restrict__ frame, int F, int H, int W,
                                                                   unsigned char* __restrict__ flags, int* __restrict__ contour) {
    const int i = blockIdx.y, p = blockIdx.x * SIL_THREADS + threadIdx.x, f = frame[i];
    bool on = false;
    if (p < H * W && f >= 0 && f < F) {   // (the host side of the entry point refuses such a frame before the launch)
        const unsigned char* m = mask + (size_t)i * H * W;
        if (m[p] != 0) {
            const float* zs = depth_scene + (size_t)f * H * W;
            const int y = p / W, x = p - y * W;
            const float zp = zs[p];
            bool occluder = false;
            auto look = [&](int q) {
                if (m[q] != 0) return;
                on = true;
                const float zq = zs[q];
                if (zq > 0.f && zp > 0.f && zq < zp) occluder = true;
            };
            if (x > 0) look(p - 1);
            if (x < W - 1) look(p + 1);
            if (y > 0) look(p - W);
            if (y < H - 1) look(p + W);
            on = on && !occluder;
        }
    }
    if (p < H * W) flags[(size_t)i * H * W + p] = on ? 1 : 0;
    const int n = __popcll(__ballot(on));
    if ((threadIdx.x & 63) == 0 && n > 0) atomicAdd(contour + i, n);
}

// grid (cdiv(W, 256), N): lane = column.  dyc [N][H][W] int32
__global__ __launch_bounds__(SIL_THREADS) void sil_column_kernel(const unsigned char* __restrict__ flags, int H, int W, int* __restrict__ dyc) {
    const int i = blockIdx.y, x = blockIdx.x * SIL_THREADS + threadIdx.x;
    if (x >= W) return;
    const unsigned char* fl = flags + (size_t)i * H * W + x;
    int* out = dyc + (size_t)i * H * W + x;
    int last = -1;
    for (int y = 0; y < H; ++y) {   // the nearest at or above
        if (fl[(size_t)y * W] != 0) last = y;
        out[(size_t)y * W] = last >= 0 ? last - y : SIL_NONE;
    }
    int next = -1;
    for (int y = H - 1; y >= 0; --y) {   // the nearest below, where it is strictly nearer
        if (fl[(size_t)y * W] != 0) next = y;
        if (next < 0) continue;
        const int above = out[(size_t)y * W], below = next - y;
        if (above == SIL_NONE || below < -above) out[(size_t)y * W] = below;
    }
}

// grid (cdiv(W, 256), H, N): lane = pixel (x, y).  d2, nearest [N][H][W] int32
__global__ __launch_bounds__(SIL_THREADS) void sil_row_kernel(const int* __restrict__ dyc, int H, int W, int* __restrict__ d2,
                                                               int* __restrict__ nearest) {
    __shared__ int s_dy[SIL_TILE];
    __shared__ unsigned s_any[SIL_TILE / SIL_GROUP];   // per group: which of its columns hold a contour pixel
    const int i = blockIdx.z, y = blockIdx.y, x = blockIdx.x * SIL_THREADS + threadIdx.x;
    const int* row = dyc + ((size_t)i * H + y) * W;
    int best = INT_MAX, best_idx = -1;
    if (x < W) {
        const int a = row[x];
        if (a != SIL_NONE) {
            best = a * a;
            best_idx = (y + a) * W + x;
        }
    }
    for (int t0 = 0; t0 < W; t0 += SIL_TILE) {
        const int t1 = min(t0 + SIL_TILE, W);
        __syncthreads();   // the previous tile has been read
        const int kend = (t1 - t0 + 63) & ~63;
        for (int k = threadIdx.x; k < kend; k += SIL_THREADS) {   // (whole waves: the ballot below needs every lane)
            const int a = t0 + k < t1 ? row[t0 + k] : SIL_NONE;
            s_dy[k] = a;
            const unsigned long long any = __ballot(a != SIL_NONE);   // lanes 0 .. 31 are one group, lanes 32 .. 63 the next
            if ((threadIdx.x & 31) == 0) s_any[k / SIL_GROUP] = (unsigned)(any >> (threadIdx.x & 32));
        }
        __syncthreads();
        if (x >= W) continue;
        for (int lo = t0; lo < t1; lo += SIL_GROUP) {
            if (s_any[(lo - t0) / SIL_GROUP] == 0u) continue;             // uniform: most of a row holds nothing
            const int hi = min(lo + SIL_GROUP, t1);
            const int gap = x < lo ? lo - x : x >= hi ? x - hi + 1 : 0;   // the nearest column of the group
            if (gap * gap > best) continue;                                // (equal: a tie may have the smaller index)
            for (int c = lo; c < hi; ++c) {
                const int a = s_dy[c - t0];
                if (a == SIL_NONE) continue;
                const int dx = x - c, v = dx * dx + a * a, idx = (y + a) * W + c;
                if (v < best || (v == best && idx < best_idx)) {
                    best = v;
                    best_idx = idx;
                }
            }
        }
    }
    if (x < W) {
        d2[((size_t)i * H + y) * W + x] = best;
        nearest[((size_t)i * H + y) * W + x] = best_idx;
    }
}

// Workgroup (band, instance): pixels [y0 * W, y1 * W) of the instance's render.  sums [N][nb][28] fp64, cnts [N][nb] int32.
__global__ __launch_bounds__(ICP_THREADS) void sil_accumulate_kernel(const float* __restrict__ depth_ren, const float* __restrict__ depth_scene,
                                                                      const int* __restrict__ frame, int F, const double* __restrict__ Km,
                                                                      const int* __restrict__ d2, const int* __restrict__ nearest, int H, int W,
                                                                      double gate2, double dist_gate, double* __restrict__ sums,
                                                                      int* __restrict__ cnts) {
    __shared__ double red[ICP_WAVES][ICP_SUMS];
    __shared__ int red_n[ICP_WAVES];
    const int band = blockIdx.x, i = blockIdx.y, nb = gridDim.x, tid = threadIdx.x;
    const int y0 = band * ICP_BAND_ROWS, y1 = min(y0 + ICP_BAND_ROWS, H);
    const int f = frame[i];
    double acc[ICP_SUMS];
#pragma unroll
    for (int k = 0; k < ICP_SUMS; ++k) acc[k] = 0.0;
    int n_pairs = 0;
    if (f >= 0 && f < F) {   // (the host side of the entry point refuses such a frame before the launch)
        const float* ren = depth_ren + (size_t)i * H * W;
        const float* sc = depth_scene + (size_t)f * H * W;
        const int* dd = d2 + (size_t)i * H * W;
        const int* nn = nearest + (size_t)i * H * W;
        const Cam cam = load_cam(Km + (size_t)i * 9);
        const int p1 = y1 * W;
        for (int p = y0 * W + tid; p < p1; p += ICP_THREADS) {   // a lane's pixels in ascending order
            const float zr_f = ren[p];
            if (!(zr_f > 0.f)) continue;
            const int y = p / W, x = p - y * W;
            const bool edge = (x > 0 && !(ren[p - 1] > 0.f)) || (x < W - 1 && !(ren[p + 1] > 0.f)) || (y > 0 && !(ren[p - W] > 0.f)) ||
                              (y < H - 1 && !(ren[p + W] > 0.f));
            if (!edge) continue;
            const float zs_f = sc[p];
            const double z = (double)zr_f;
            if (zs_f > 0.f && (double)zs_f < z - dist_gate) continue;   // hidden in the observation
            const int c = nn[p];
            if (c < 0 || !((double)dd[p] <= gate2)) continue;
            const int cy = c / W, cx = c - cy * W;
            double dx, dy, gx, gy;
            pixel_ray(cam, x, y, dx, dy);
            pixel_ray(cam, cx, cy, gx, gy);
            const V3 P = {z * dx, z * dy, z};
            const V3 n1 = {1.0, 0.0, -gx}, n2 = {0.0, 1.0, -gy};
            const V3 c1 = cross(P, n1), c2 = cross(P, n2);
            const double r1 = z * (dx - gx), r2 = z * (dy - gy);
            const double J1[6] = {c1.x, c1.y, c1.z, n1.x, n1.y, n1.z}, J2[6] = {c2.x, c2.y, c2.z, n2.x, n2.y, n2.z};
#pragma unroll
            for (int g = 0; g < 6; ++g)
#pragma unroll
                for (int h = g; h < 6; ++h) {
                    acc[icp_tri(g, h)] += J1[g] * J1[h];
                    acc[icp_tri(g, h)] += J2[g] * J2[h];
                }
#pragma unroll
            for (int g = 0; g < 6; ++g) {
                acc[21 + g] += J1[g] * r1;
                acc[21 + g] += J2[g] * r2;
            }
            acc[27] += r1 * r1;
            acc[27] += r2 * r2;
            ++n_pairs;
        }
    }
    icp_fold_band(acc, n_pairs, red, red_n, i, band, nb, sums, cnts);
}

// One wave per instance.  Prologue: the silhouette sums over their nb bands (nb = 1: a combined system as it is), then entry by entry
// sys = sys_depth + weight * sys_sil and pairs = pairs_depth + pairs_sil.  A frozen instance is left alone, outputs included.  The six output
// pointers may be NULL together (the stand-alone gdrn_icp_step_sil).
__global__ __launch_bounds__(64) void sil_step_kernel(const double* __restrict__ sys_depth, const int* __restrict__ pairs_depth,
                                                       const double* __restrict__ sums, const int* __restrict__ cnts, int nb, double weight,
                                                       int min_pairs, double* __restrict__ Rm, double* __restrict__ tv, int* __restrict__ state,
                                                       int* __restrict__ ok, int* __restrict__ iters_done, int* __restrict__ pairs_out,
                                                       double* __restrict__ rms, int* __restrict__ sil_pairs, double* __restrict__ sil_rms) {
    __shared__ double sys[ICP_SUMS];
    __shared__ double s_sq_sil;
    __shared__ int s_pairs_sil;
    const int i = blockIdx.x, lane = threadIdx.x;
    if (state[(size_t)i * 2] != GDRN_ICP_RUNNING) return;   // uniform over the wave
    if (lane < ICP_SUMS) {
        const double s = icp_combine(sums, i, nb, lane);
        sys[lane] = sys_depth[(size_t)i * ICP_SUMS + lane] + weight * s;
        if (lane == ICP_SUMS - 1) s_sq_sil = s;
    } else if (lane == ICP_SUMS) {
        s_pairs_sil = icp_combine_n(cnts, i, nb);
    }
    __syncthreads();
    if (lane != 0) return;
    const int nd = pairs_depth[i], ns = s_pairs_sil;
    if (ok != nullptr) {
        pairs_out[i] = nd;
        rms[i] = sqrt(sys_depth[(size_t)i * ICP_SUMS + 27] / (double)nd);   // 0 / 0 = NaN without a pair
        sil_pairs[i] = ns;
        sil_rms[i] = sqrt(s_sq_sil / (double)ns);
    }
    icp_solve_and_update(sys, nd + ns, min_pairs, i, Rm, tv, state, ok, iters_done);
}

bool sil_frame_ok(int N, int H, int W) { return N >= 0 && H >= 1 && W >= 1 && (long long)H * W <= 0x7fffffffLL - 1024; }
bool sil_weight_ok(double w) { return w >= 0.0 && w <= 1.7976931348623157e308; }

long long sil_pad8(long long b) { return (b + 7) & ~7LL; }

// the workspace: sums [N][nb][28] fp64 | sys_depth [N][28] fp64 | the ICP's own (padded to 8 bytes) | d2, nearest, dyc [N][H][W] int32 |
// cnts [N][nb] | state [N][2] | pairs_depth [N] | contour [N] int32 | flags [N][H][W] uint8
struct SilWs {
    double* sums;
    double* sys_depth;
    void* icp;
    int* d2;
    int* nearest;
    int* dyc;
    int* cnts;
    int* state;
    int* pairs_depth;
    int* contour;
    unsigned char* flags;
};
long long sil_bytes(int N, int H, int W) {
    const long long nb = icp_bands(H), px = (long long)N * H * W;
    return (long long)N * (nb + 1) * ICP_SUMS * (long long)sizeof(double) + sil_pad8(gdrn_icp_workspace_bytes(N, H, W)) +
           (3 * px + (long long)N * (nb + 4)) * (long long)sizeof(int) + px;
}
SilWs sil_carve(void* workspace, int N, int H, int W) {
    const size_t nb = icp_bands(H), px = (size_t)N * H * W;
    SilWs w;
    char* p = reinterpret_cast<char*>(workspace);
    w.sums = reinterpret_cast<double*>(p);
    p += (size_t)N * nb * ICP_SUMS * sizeof(double);
    w.sys_depth = reinterpret_cast<double*>(p);
    p += (size_t)N * ICP_SUMS * sizeof(double);
    w.icp = p;
    p += sil_pad8(gdrn_icp_workspace_bytes(N, H, W));
    w.d2 = reinterpret_cast<int*>(p);
    w.nearest = w.d2 + px;
    w.dyc = w.nearest + px;
    w.cnts = w.dyc + px;
    w.state = w.cnts + (size_t)N * nb;
    w.pairs_depth = w.state + (size_t)N * 2;
    w.contour = w.pairs_depth + N;
    w.flags = reinterpret_cast<unsigned char*>(w.contour + N);
    return w;
}

int sil_launch_transform(const unsigned char* mask, const float* depth_scene, const int* frame, int F, int N, int H, int W, int* d2, int* nearest,
                         int* contour, const SilWs& w, hipStream_t st) {
    if (hipMemsetAsync(contour, 0, (size_t)N * sizeof(int), st) != hipSuccess) return GDRN_ERR_LAUNCH;
    GDRN_LAUNCH(sil_contour_kernel, dim3(cdiv(H * W, SIL_THREADS), N), dim3(SIL_THREADS), 0, st, mask, depth_scene, frame, F, H, W, w.flags,
                contour);
    GDRN_CHECK_LAUNCH();
    GDRN_LAUNCH(sil_column_kernel, dim3(cdiv(W, SIL_THREADS), N), dim3(SIL_THREADS), 0, st, w.flags, H, W, w.dyc);
    GDRN_CHECK_LAUNCH();
    GDRN_LAUNCH(sil_row_kernel, dim3(cdiv(W, SIL_THREADS), H, N), dim3(SIL_THREADS), 0, st, w.dyc, H, W, d2, nearest);
    GDRN_CHECK_LAUNCH();
    return GDRN_OK;
}

int sil_launch_accumulate(const float* depth_ren, const float* depth_scene, const int* frame, int F, const double* K, const int* d2,
                          const int* nearest, int N, int H, int W, double sil_gate, double dist_gate, const SilWs& w, hipStream_t st) {
    GDRN_LAUNCH(sil_accumulate_kernel, dim3(icp_bands(H), N), dim3(ICP_THREADS), 0, st, depth_ren, depth_scene, frame, F, K, d2, nearest, H, W,
                sil_gate * sil_gate, dist_gate, w.sums, w.cnts);
    GDRN_CHECK_LAUNCH();
    return GDRN_OK;
}

}  // namespace

extern "C" long long gdrn_sil_workspace_bytes(int N, int H, int W) {
    if (!sil_frame_ok(N, H, W)) return GDRN_ERR_ARG;
    if (H > SIL_MAX_SIDE || W > SIL_MAX_SIDE) return GDRN_ERR_SHAPE;
    return sil_bytes(N, H, W);
}

extern "C" int gdrn_sil_contour_transform(const unsigned char* mask_obs, const float* depth_scene, const int* frame, const int* frame_host, int F,
                                          int N, int H, int W, int* d2, int* nearest, int* contour, void* workspace, void* stream) {
    if (!sil_frame_ok(N, H, W) || F < 0) return GDRN_ERR_ARG;
    if (H > SIL_MAX_SIDE || W > SIL_MAX_SIDE) return GDRN_ERR_SHAPE;
    if (N == 0) return GDRN_OK;
    if (!mask_obs || !depth_scene || !frame || !frame_host || !d2 || !nearest || !contour || !workspace || ((size_t)workspace & 7))
        return GDRN_ERR_ARG;
    if (N > 65535) return GDRN_ERR_SHAPE;   // the instances are a grid dimension
    if (!host_in_range(frame_host, N, F)) return GDRN_ERR_ARG;
    const SilWs w = sil_carve(workspace, N, H, W);
    return sil_launch_transform(mask_obs, depth_scene, frame, F, N, H, W, d2, nearest, contour, w, reinterpret_cast<hipStream_t>(stream));
}

extern "C" int gdrn_sil_accumulate(const float* depth_ren, const float* depth_scene, const int* frame, const int* frame_host, int F, const double* K,
                                   const int* d2, const int* nearest, int N, int H, int W, double sil_gate, double dist_gate, double* sys,
                                   int* pairs, void* workspace, void* stream) {
    if (!sil_frame_ok(N, H, W) || F < 0 || !(sil_gate > 0.0) || !(dist_gate > 0.0)) return GDRN_ERR_ARG;
    if (H > SIL_MAX_SIDE || W > SIL_MAX_SIDE) return GDRN_ERR_SHAPE;
    if (N == 0) return GDRN_OK;
    if (!depth_ren || !depth_scene || !frame || !frame_host || !K || !d2 || !nearest || !sys || !pairs || !workspace || ((size_t)workspace & 7))
        return GDRN_ERR_ARG;
    if (N > 65535) return GDRN_ERR_SHAPE;
    if (!host_in_range(frame_host, N, F)) return GDRN_ERR_ARG;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const SilWs w = sil_carve(workspace, N, H, W);
    const int bad = sil_launch_accumulate(depth_ren, depth_scene, frame, F, K, d2, nearest, N, H, W, sil_gate, dist_gate, w, st);
    if (bad != GDRN_OK) return bad;
    GDRN_LAUNCH(icp_combine_kernel, dim3(N), dim3(64), 0, st, w.sums, w.cnts, icp_bands(H), sys, pairs);
    GDRN_CHECK_LAUNCH();
    return GDRN_OK;
}

extern "C" int gdrn_icp_step_sil(const double* sys_depth, const int* pairs_depth, const double* sys_sil, const int* pairs_sil, double weight, int N,
                                 int min_pairs, double* R, double* t, int* state, void* stream) {
    if (N < 0 || min_pairs < 6 || !sil_weight_ok(weight)) return GDRN_ERR_ARG;
    if (N == 0) return GDRN_OK;
    if (!sys_depth || !pairs_depth || !sys_sil || !pairs_sil || !R || !t || !state) return GDRN_ERR_ARG;
    GDRN_LAUNCH(sil_step_kernel, dim3(N), dim3(64), 0, reinterpret_cast<hipStream_t>(stream), sys_depth, pairs_depth, sys_sil, pairs_sil, 1, weight,
                min_pairs, R, t, state, (int*)nullptr, (int*)nullptr, (int*)nullptr, (double*)nullptr, (int*)nullptr, (double*)nullptr);
    GDRN_CHECK_LAUNCH();
    return GDRN_OK;
}

extern "C" int gdrn_icp_refine_sil(const double* verts, const int* faces, const int* vert_off, const int* nverts, const int* face_off,
                                   const int* nfaces, int C, int f_max, const int* labels, const int* labels_host, double* R, double* t,
                                   const double* K, int N, const float* depth_scene, const int* frame, const int* frame_host, int F,
                                   const unsigned char* mask_obs, int H, int W, double near, double far, int iters, double dist_gate,
                                   double normal_gate, int min_pairs, double sil_weight, double sil_gate, float* depth_ren_scratch, int* ok,
                                   int* iters_done, int* pairs, double* rms, int* sil_pairs, double* sil_rms, void* workspace, void* stream) {
    const RenderRows rows = {verts, faces, vert_off, nverts, face_off, nfaces, C, f_max, labels, labels_host, R, t, K, N, H, W, near, far};
    const RenderScene scene = {depth_scene, frame, frame_host, F};
    if (!sil_frame_ok(N, H, W) || iters < 0 || min_pairs < 6 || !(dist_gate > 0.0) || !(normal_gate > 0.0)) return GDRN_ERR_ARG;
    if (!sil_weight_ok(sil_weight) || !(sil_gate > 0.0)) return GDRN_ERR_ARG;
    if (!loop_scalars_ok(rows, scene)) return GDRN_ERR_ARG;
    if (H > SIL_MAX_SIDE || W > SIL_MAX_SIDE) return GDRN_ERR_SHAPE;
    if (N == 0) return GDRN_OK;
    if (!mask_obs || !depth_ren_scratch || !ok || !iters_done || !pairs || !rms || !sil_pairs || !sil_rms || !workspace || ((size_t)workspace & 7))
        return GDRN_ERR_ARG;
    int bad = loop_rows_check(rows, scene);
    if (bad != GDRN_OK) return bad;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const int nb = icp_bands(H);
    const SilWs w = sil_carve(workspace, N, H, W);
    GDRN_LAUNCH(icp_init_kernel, dim3(cdiv(N, ICP_THREADS)), dim3(ICP_THREADS), 0, st, N, w.state, ok, iters_done, pairs, rms, sil_pairs, sil_rms);
    GDRN_CHECK_LAUNCH();
    if (iters == 0) return GDRN_OK;
    bad = sil_launch_transform(mask_obs, depth_scene, frame, F, N, H, W, w.d2, w.nearest, w.contour, w, st);
    if (bad != GDRN_OK) return bad;
    for (int it = 0; it < iters; ++it) {
        bad = render_into(rows, depth_ren_scratch, stream);
        if (bad != GDRN_OK) return bad;
        bad = gdrn_icp_accumulate(depth_ren_scratch, depth_scene, frame, frame_host, F, K, N, H, W, dist_gate, normal_gate, w.sys_depth,
                                  w.pairs_depth, w.icp, stream);
        if (bad != GDRN_OK) return bad;
        bad = sil_launch_accumulate(depth_ren_scratch, depth_scene, frame, F, K, w.d2, w.nearest, N, H, W, sil_gate, dist_gate, w, st);
        if (bad != GDRN_OK) return bad;
        GDRN_LAUNCH(sil_step_kernel, dim3(N), dim3(64), 0, st, w.sys_depth, w.pairs_depth, w.sums, w.cnts, nb, sil_weight, min_pairs, R, t, w.state,
                    ok, iters_done, pairs, rms, sil_pairs, sil_rms);
        GDRN_CHECK_LAUNCH();
    }
    return GDRN_OK;
}
