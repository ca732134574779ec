// Depth refinement of estimated poses for gfx950: projective point-to-plane ICP of a batch of estimates against observed depth frames --
//   (rendered depth, observed depth) -> the 6 x 6 normal equations of every estimate                       -> gdrn_icp_accumulate
//   solve, left-multiplied pose update, stop rule                                                          -> gdrn_icp_step
//   render, accumulate, step, `iters` times on one stream without a host read                              -> gdrn_icp_refine
// The reference has no counterpart (it is RGB-only); the arithmetic is stated with the entry points in include/gdrn_hip.h and restated on the
// host in tests/icp_host.py.
//
// The accumulate pass: one workgroup per (instance, band of ICP_BAND_ROWS rows).  A band is a contiguous range of the instance's render; a lane
// walks it with stride 256 (coalesced fp32 loads), reads the five observed depths of a pixel only where the render is covered (the neighbours
// come from L2), builds the observation's normal on the fly and keeps 28 fp64 sums (21 of J J^T, 6 of J r, 1 of r^2) and the pair count.
// ICP_PPT render depths are loaded before the first is looked at, so that a lane has that many loads in flight over a body that diverges.  The
// workgroup folds them in a fixed order (xor tree per wave, four waves in LDS) and writes its slab; a band without a pair writes zeros without
// the fold.  No floating-point atomics, no counters: the slabs are combined band by band, in ascending order, at the next launch boundary -- in
// the prologue of the step kernel inside gdrn_icp_refine, by a combine launch of its own behind a stand-alone gdrn_icp_accumulate -- with one
// and the same device function, so both give the same bits.  Every slab is written by every call: the workspace needs no initialisation.
//
// The step kernel: one wave per instance; lane k < 28 combines sum k over the bands, lane 28 the counts, lane 0 solves.
//
// Floating-point contraction is OFF for this file: a pixel's terms are one fixed operation sequence, which the host restatement repeats.
// (No 16-bit code: both library builds compile the same thing.)
#include "common.h"
#include "geom64.h"
#include "../../include/gdrn_hip.h"

#pragma clang fp contract(off)

#include "raster64.h"
#include "icp_shared.h"
#include "render_loop.h"

namespace {

constexpr int ICP_PPT = 4;                      // render depths a lane loads before it looks at any of them

// Workgroup (band, instance): pixels [y0 * W, y1 * W) of the instance's render.  sums [N][nb][28] fp64, cnts [N][nb] int32.
__global__ __launch_bounds__(ICP_THREADS) void icp_accumulate_kernel(const float* __restrict__ depth_ren, const float* __restrict__ depth_scene,
                                                                      const int* __restrict__ frame, int F, const double* __restrict__ Km, int H,
                                                                      int W, double dist_gate, double normal_gate, double* __restrict__ sums,
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
        const Cam cam = load_cam(Km + (size_t)i * 9);
        const int p1 = y1 * W;
        for (int p0 = y0 * W + tid; p0 < p1; p0 += ICP_THREADS * ICP_PPT) {
            float z[ICP_PPT];
#pragma unroll
            for (int u = 0; u < ICP_PPT; ++u) {   // all loads first: ICP_PPT in flight per lane
                const int p = p0 + u * ICP_THREADS;
                z[u] = p < p1 ? ren[p] : 0.f;
            }
#pragma unroll 1
            for (int u = 0; u < ICP_PPT; ++u) {   // one copy of the body; a lane's pixels in ascending order
                static_assert(ICP_PPT == 4, "the select below names z[0] .. z[3]");
                const float zr_f = u == 0 ? z[0] : u == 1 ? z[1] : u == 2 ? z[2] : z[3];
                if (!(zr_f > 0.f)) continue;
                const int p = p0 + u * ICP_THREADS;
                const int y = p / W, x = p - y * W;
                if (x == 0 || y == 0 || x == W - 1 || y == H - 1) continue;   // the five-point stencil stays inside the frame
                const double zr = (double)zr_f, zc = (double)sc[p];
                const double zl = (double)sc[p - 1], zg = (double)sc[p + 1], zu = (double)sc[p - W], zd = (double)sc[p + W];
                if (!(zc > 0.0 && zl > 0.0 && zg > 0.0 && zu > 0.0 && zd > 0.0)) continue;
                if (!(fabs(zl - zc) <= normal_gate && fabs(zg - zc) <= normal_gate && fabs(zu - zc) <= normal_gate && fabs(zd - zc) <= normal_gate))
                    continue;
                const double e = zr - zc;   // exact: the difference of two fp32 values
                if (!(fabs(e) <= dist_gate)) continue;
                double dx, dy, lx, ly, gx, gy, ux, uy, wx, wy;
                pixel_ray(cam, x, y, dx, dy);
                pixel_ray(cam, x - 1, y, lx, ly);
                pixel_ray(cam, x + 1, y, gx, gy);
                pixel_ray(cam, x, y - 1, ux, uy);
                pixel_ray(cam, x, y + 1, wx, wy);
                const V3 a = {zg * gx - zl * lx, zg * gy - zl * ly, zg - zl};
                const V3 b = {zd * wx - zu * ux, zd * wy - zu * uy, zd - zu};
                const V3 c = cross(a, b);
                const double len = sqrt((c.x * c.x + c.y * c.y) + c.z * c.z);
                if (!(len > 0.0)) continue;
                const V3 n = {c.x / len, c.y / len, c.z / len};
                const double r = e * ((n.x * dx + n.y * dy) + n.z);   // n . (p - q), p - q = (depth_ren - depth_scene) d
                const V3 pm = {zr * dx, zr * dy, zr};
                const V3 pn = cross(pm, n);
                const double J[6] = {pn.x, pn.y, pn.z, n.x, n.y, n.z};
#pragma unroll
                for (int g = 0; g < 6; ++g)
#pragma unroll
                    for (int h = g; h < 6; ++h) acc[icp_tri(g, h)] += J[g] * J[h];
#pragma unroll
                for (int g = 0; g < 6; ++g) acc[21 + g] += J[g] * r;
                acc[27] += r * r;
                ++n_pairs;
            }
        }
    }
    icp_fold_band(acc, n_pairs, red, red_n, i, band, nb, sums, cnts);
}

// One wave per instance.  Prologue: the instance's sums over its nb bands (nb = 1: a combined system as it is).  A frozen instance (state != running)
// is left alone, outputs included.  ok / iters_done / pairs_out / rms may be NULL together (the stand-alone gdrn_icp_step).
__global__ __launch_bounds__(64) void icp_step_kernel(const double* __restrict__ sums, const int* __restrict__ cnts, int nb, int min_pairs,
                                                       double* __restrict__ Rm, double* __restrict__ tv, int* __restrict__ state,
                                                       int* __restrict__ ok, int* __restrict__ iters_done, int* __restrict__ pairs_out,
                                                       double* __restrict__ rms) {
    __shared__ double sys[ICP_SUMS];
    __shared__ int s_pairs;
    const int i = blockIdx.x, lane = threadIdx.x;
    if (state[(size_t)i * 2] != GDRN_ICP_RUNNING) return;   // uniform over the wave
    if (lane < ICP_SUMS) sys[lane] = icp_combine(sums, i, nb, lane);
    else if (lane == ICP_SUMS) s_pairs = icp_combine_n(cnts, i, nb);
    __syncthreads();
    if (lane != 0) return;
    const int n = s_pairs;
    if (ok != nullptr) {
        pairs_out[i] = n;
        rms[i] = sqrt(sys[27] / (double)n);   // 0 / 0 = NaN without a pair
    }
    icp_solve_and_update(sys, n, min_pairs, i, Rm, tv, state, ok, iters_done);
}

bool icp_frame_ok(int N, int H, int W) { return N >= 0 && H >= 1 && W >= 1 && (long long)H * W <= 0x7fffffffLL - ICP_THREADS * ICP_PPT; }

// the workspace: sums [N][nb][28] fp64 | state [N][2] int32 | cnts [N][nb] int32
struct IcpWs {
    double* sums;
    int* state;
    int* cnts;
};
IcpWs icp_carve(void* workspace, int N, int nb) {
    IcpWs w;
    w.sums = reinterpret_cast<double*>(workspace);
    w.state = reinterpret_cast<int*>(w.sums + (size_t)N * nb * ICP_SUMS);
    w.cnts = w.state + (size_t)N * 2;
    return w;
}

int icp_launch_accumulate(const float* depth_ren, const float* depth_scene, const int* frame, int F, const double* K, int N, int H, int W,
                          double dist_gate, double normal_gate, const IcpWs& w, hipStream_t st) {
    GDRN_LAUNCH(icp_accumulate_kernel, dim3(icp_bands(H), N), dim3(ICP_THREADS), 0, st, depth_ren, depth_scene, frame, F, K, H, W, dist_gate,
                normal_gate, w.sums, w.cnts);
    GDRN_CHECK_LAUNCH();
    return GDRN_OK;
}

}  // namespace

extern "C" long long gdrn_icp_workspace_bytes(int N, int H, int W) {
    if (!icp_frame_ok(N, H, W)) return GDRN_ERR_ARG;
    const long long nb = icp_bands(H);
    return (long long)N * nb * ICP_SUMS * (long long)sizeof(double) + (long long)N * (2 + nb) * (long long)sizeof(int);
}

extern "C" int gdrn_icp_accumulate(const float* depth_ren, const float* depth_scene, const int* frame, const int* frame_host, int F, const double* K,
                                   int N, int H, int W, double dist_gate, double normal_gate, double* sys, int* pairs, void* workspace,
                                   void* stream) {
    if (!icp_frame_ok(N, H, W) || F < 0 || !(dist_gate > 0.0) || !(normal_gate > 0.0)) return GDRN_ERR_ARG;
    if (N == 0) return GDRN_OK;
    if (!depth_ren || !depth_scene || !frame || !frame_host || !K || !sys || !pairs || !workspace || ((size_t)workspace & 7)) return GDRN_ERR_ARG;
    if (N > 65535) return GDRN_ERR_SHAPE;   // the instances are the grid's second dimension
    if (!host_in_range(frame_host, N, F)) return GDRN_ERR_ARG;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const int nb = icp_bands(H);
    const IcpWs w = icp_carve(workspace, N, nb);
    const int bad = icp_launch_accumulate(depth_ren, depth_scene, frame, F, K, N, H, W, dist_gate, normal_gate, w, st);
    if (bad != GDRN_OK) return bad;
    GDRN_LAUNCH(icp_combine_kernel, dim3(N), dim3(64), 0, st, w.sums, w.cnts, nb, sys, pairs);
    GDRN_CHECK_LAUNCH();
    return GDRN_OK;
}

extern "C" int gdrn_icp_step(const double* sys, const int* pairs, int N, int min_pairs, double* R, double* t, int* state, void* stream) {
    if (N < 0 || min_pairs < 6) return GDRN_ERR_ARG;
    if (N == 0) return GDRN_OK;
    if (!sys || !pairs || !R || !t || !state) return GDRN_ERR_ARG;
    GDRN_LAUNCH(icp_step_kernel, dim3(N), dim3(64), 0, reinterpret_cast<hipStream_t>(stream), sys, pairs, 1, min_pairs, R, t, state,
                (int*)nullptr, (int*)nullptr, (int*)nullptr, (double*)nullptr);
    GDRN_CHECK_LAUNCH();
    return GDRN_OK;
}

extern "C" int gdrn_icp_refine(const double* verts, const int* faces, const int* vert_off, const int* nverts, const int* face_off,
                               const int* nfaces, int C, int f_max, const int* labels, const int* labels_host, double* R, double* t,
                               const double* K, int N, const float* depth_scene, const int* frame, const int* frame_host, int F, int H, int W,
                               double near, double far, int iters, double dist_gate, double normal_gate, int min_pairs, float* depth_ren_scratch,
                               int* ok, int* iters_done, int* pairs, double* rms, void* workspace, void* stream) {
    const RenderRows rows = {verts, faces, vert_off, nverts, face_off, nfaces, C, f_max, labels, labels_host, R, t, K, N, H, W, near, far};
    const RenderScene scene = {depth_scene, frame, frame_host, F};
    if (!icp_frame_ok(N, H, W) || iters < 0 || min_pairs < 6 || !(dist_gate > 0.0) || !(normal_gate > 0.0)) return GDRN_ERR_ARG;
    if (!loop_scalars_ok(rows, scene)) return GDRN_ERR_ARG;
    if (N == 0) return GDRN_OK;
    if (!depth_ren_scratch || !ok || !iters_done || !pairs || !rms || !workspace || ((size_t)workspace & 7)) return GDRN_ERR_ARG;
    int bad = loop_rows_check(rows, scene);
    if (bad != GDRN_OK) return bad;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const int nb = icp_bands(H);
    const IcpWs w = icp_carve(workspace, N, nb);
    GDRN_LAUNCH(icp_init_kernel, dim3(cdiv(N, ICP_THREADS)), dim3(ICP_THREADS), 0, st, N, w.state, ok, iters_done, pairs, rms, (int*)nullptr,
                (double*)nullptr);
    GDRN_CHECK_LAUNCH();
    for (int it = 0; it < iters; ++it) {
        bad = render_into(rows, depth_ren_scratch, stream);
        if (bad != GDRN_OK) return bad;
        bad = icp_launch_accumulate(depth_ren_scratch, depth_scene, frame, F, K, N, H, W, dist_gate, normal_gate, w, st);
        if (bad != GDRN_OK) return bad;
        GDRN_LAUNCH(icp_step_kernel, dim3(N), dim3(64), 0, st, w.sums, w.cnts, nb, min_pairs, R, t, w.state, ok, iters_done, pairs, rms);
        GDRN_CHECK_LAUNCH();
    }
    return GDRN_OK;
}
