// Batched depth rasterizer and object-coordinate (xyz) target generation for gfx950: what the reference produces in an offline pass per annotated
// instance (tools/lm/lm_pbr_1_gen_xyz_crop.py) --
//   an OpenGL render of the object's depth under the ground-truth pose                      -> gdrn_render_depth
//   misc.calc_xyz_bp_fast(depth, R, t, K) (lib/pysixd/misc.py:288-316) + mask2bbox_xyxy     -> gdrn_xyz_from_depth
//   (lib/utils/mask_utils.py:39-44), the "not visible" record of the tool's :142-150
// -- for a whole batch of instances per call; and the same walk with 64-bit keys, depth bits above the winning face's index, for the shaded
// renderer (shade.hip) -> gdrn_render_visibility.  The rasterizer's rules are geometric and stated in include/gdrn_hip.h: integer-pixel rays
// d = K^-1 [x, y, 1], coverage from the signs of d . (p x q) per edge (no perspective divide, inclusive edges, both windings), depth from the
// ray-plane intersection, all of it fp64 with one rounding to fp32, the nearest fragment kept by an unsigned atomic min on the fp32 bits.
//
// Floating-point contraction is OFF for this file and every fused operation is an explicit fma(): a pixel's edge value is then one fixed
// operation sequence on (ray, the edge's two camera-space vertices in ascending index order), whichever code path, triangle or launch shape
// evaluates it -- the watertightness and order-independence guarantees rest on that.  (No 16-bit code: both library builds compile the same thing.)
#include "common.h"
#include "geom64.h"
#include "../../include/gdrn_hip.h"

#pragma clang fp contract(off)

#include "raster64.h"
#include "render_loop.h"

namespace {

constexpr int RD_THREADS = 256;                 // faces per workgroup: one lane sets up one triangle
constexpr int RD_WAVES = RD_THREADS / 64;
constexpr int RD_SMALL = 64;                    // screen boxes of up to this many pixels are walked by the lane that set the triangle up
constexpr unsigned RD_INF_BITS = 0x7f800000u;   // +inf: the cleared depth buffer
constexpr int RD_MAX_SPLIT = 16;
constexpr int RD_TARGET_WGS = 1024;             // (4 per CU) below this many workgroups the tile walk of the large triangles is split further

// what a fragment needs of its triangle (sorted vertices a < b < c by index): the three edge normals a x b, b x c, a x c (ascending pairs), the plane
// normal n = (b - a) x (c - a), n . a, and the clipped screen box
struct Tri {
    double e0x, e0y, e0z, e1x, e1y, e1z, e2x, e2y, e2z, nx, ny, nz, na;
    int x0, y0, x1, y1, face, pad_;
};

// One fragment: coverage, depth, depth test.  `buf` is the instance's H x W slice: fp32 bit patterns (Key = unsigned, gdrn_render_depth) or
// visibility keys (Key = unsigned long long, gdrn_render_visibility: the same bits in the upper half, the face index within the class below them --
// the smallest key is the nearest fp32 depth and, among equal depths, the lowest face index).  Everything up to the store is the same code.
template <typename Key>
__device__ __forceinline__ void fragment(const Tri& T, const Cam& cam, int x, int y, int W, double far, Key* __restrict__ buf) {
    double dx, dy;
    pixel_ray(cam, x, y, dx, dy);
    const double w0 = fma(dx, T.e0x, fma(dy, T.e0y, T.e0z));        // d . (a x b)
    const double w1 = fma(dx, T.e1x, fma(dy, T.e1y, T.e1z));        // d . (b x c)
    const double w2 = -fma(dx, T.e2x, fma(dy, T.e2y, T.e2z));       // d . (c x a) = -(d . (a x c)), exactly
    const bool in = (w0 >= 0.0 && w1 >= 0.0 && w2 >= 0.0) || (w0 <= 0.0 && w1 <= 0.0 && w2 <= 0.0);
    if (!in) return;
    const double den = fma(dx, T.nx, fma(dy, T.ny, T.nz));          // n . d
    if (den == 0.0) return;
    const double z = T.na / den;
    if (z > far) return;
    const float zf = (float)z;                                      // the one rounding
    if (!(zf > 0.f && zf < INFINITY)) return;                       // the unsigned order of the bits is the order of the values for positive floats only
    if constexpr (sizeof(Key) == 8) atomicMin(buf + (size_t)y * W + x, ((Key)__float_as_uint(zf) << 32) | (Key)(unsigned)T.face);
    else atomicMin(buf + (size_t)y * W + x, __float_as_uint(zf));
}

__global__ __launch_bounds__(RD_THREADS) void render_clear_kernel(unsigned* __restrict__ buf, size_t n) {
    const size_t i = (size_t)blockIdx.x * RD_THREADS + threadIdx.x;
    if (i < n) buf[i] = RD_INF_BITS;
}

// the cleared visibility buffer: ~0, which is also what a pixel without a fragment keeps (no resolve pass)
__global__ __launch_bounds__(RD_THREADS) void render_clear_keys_kernel(unsigned long long* __restrict__ buf, size_t n) {
    const size_t i = (size_t)blockIdx.x * RD_THREADS + threadIdx.x;
    if (i < n) buf[i] = ~0ull;
}

__global__ __launch_bounds__(RD_THREADS) void render_resolve_kernel(unsigned* __restrict__ buf, size_t n) {
    const size_t i = (size_t)blockIdx.x * RD_THREADS + threadIdx.x;
    if (i < n && buf[i] == RD_INF_BITS) buf[i] = 0u;   // nothing drawn: 0.0f
}

// Workgroup (instance i, chunk of RD_THREADS faces, split s of gridDim.z).  Level 1: every lane sets up one triangle; a small screen box is walked
// by that lane (split 0 only), a large one is queued in LDS.  Level 2: the queued triangles are walked in 8 x 8 pixel tiles, one tile per wave step,
// lane = pixel; a triangle's tiles are dealt round-robin to the RD_WAVES * gridDim.z waves that hold this chunk, by a rule of (face, tile)
// alone -- the order in which a workgroup's queue fills differs from workgroup to workgroup.  The depth test is an
// atomic min and a fragment's value does not depend on who computes it, so every distribution gives the same bits.
template <typename Key>
__global__ __launch_bounds__(RD_THREADS) void render_raster_kernel(const double* __restrict__ verts, const int* __restrict__ faces,
                                                                   const int* __restrict__ vert_off, const int* __restrict__ nverts,
                                                                   const int* __restrict__ face_off, const int* __restrict__ nfaces, int C,
                                                                   const int* __restrict__ labels, const double* __restrict__ Rm,
                                                                   const double* __restrict__ tv, const double* __restrict__ Km, int H, int W,
                                                                   double near, double far, Key* __restrict__ depth) {
    __shared__ Tri queue[RD_THREADS];
    __shared__ int nqueue;
    const int i = blockIdx.x, chunk = blockIdx.y, split = blockIdx.z, tid = threadIdx.x;
    const int c = labels[i];
    if (c < 0 || c >= C) return;   // (the host side of the entry point refuses such a label before the launch)
    const int nf = nfaces[c], nv = nverts[c];
    if (chunk * RD_THREADS >= nf) return;   // uniform over the workgroup: no barrier has been reached
    if (tid == 0) nqueue = 0;
    __syncthreads();
    double R[9], t[3];
#pragma unroll
    for (int k = 0; k < 9; ++k) R[k] = Rm[(size_t)i * 9 + k];
#pragma unroll
    for (int k = 0; k < 3; ++k) t[k] = tv[(size_t)i * 3 + k];
    const Cam cam = load_cam(Km + (size_t)i * 9);
    Key* buf = depth + (size_t)i * H * W;

    const int f = chunk * RD_THREADS + tid;
    bool small = false;
    Tri T;
    if (f < nf) {
        const int* fp = faces + ((size_t)face_off[c] + f) * 3;
        int ia = fp[0], ib = fp[1], ic = fp[2], tmp;
        if (ia > ib) { tmp = ia; ia = ib; ib = tmp; }   // canonical order: ascending vertex indices
        if (ib > ic) { tmp = ib; ib = ic; ic = tmp; }
        if (ia > ib) { tmp = ia; ia = ib; ib = tmp; }
        if (ia >= 0 && ic < nv) {   // (MeshTable range-checks the indices on the host)
            const double* vb = verts + (size_t)vert_off[c] * 3;
            const V3 a = xform(R, t, load3(vb + (size_t)ia * 3)), b = xform(R, t, load3(vb + (size_t)ib * 3)), cc = xform(R, t, load3(vb + (size_t)ic * 3));
            if (a.z >= near && b.z >= near && cc.z >= near) {   // a vertex in front of the near plane drops the whole triangle (no clipping)
                const V3 ab = {b.x - a.x, b.y - a.y, b.z - a.z}, ac = {cc.x - a.x, cc.y - a.y, cc.z - a.z};
                const V3 n = cross(ab, ac);
                if (n.x != 0.0 || n.y != 0.0 || n.z != 0.0) {
                    const V3 e0 = cross(a, b), e1 = cross(b, cc), e2 = cross(a, cc);
                    T = Tri{e0.x, e0.y, e0.z, e1.x, e1.y, e1.z, e2.x, e2.y, e2.z, n.x, n.y, n.z, fma(n.x, a.x, fma(n.y, a.y, n.z * a.z)), 0, 0, 0, 0, f, 0};
                    // screen box of the projected vertices, one pixel of slack for the rounding of the projection, clipped to the frame
                    const double ua = (cam.fx * a.x + cam.sk * a.y) / a.z + cam.cx, va = cam.fy * a.y / a.z + cam.cy;
                    const double ub = (cam.fx * b.x + cam.sk * b.y) / b.z + cam.cx, vb2 = cam.fy * b.y / b.z + cam.cy;
                    const double uc = (cam.fx * cc.x + cam.sk * cc.y) / cc.z + cam.cx, vc = cam.fy * cc.y / cc.z + cam.cy;
                    const double ulo = fmin(ua, fmin(ub, uc)) - 1.0, uhi = fmax(ua, fmax(ub, uc)) + 1.0;
                    const double vlo = fmin(va, fmin(vb2, vc)) - 1.0, vhi = fmax(va, fmax(vb2, vc)) + 1.0;
                    // (comparisons written so that a NaN bound gives an empty box)
                    if (ulo <= (double)(W - 1) && uhi >= 0.0 && vlo <= (double)(H - 1) && vhi >= 0.0) {
                        T.x0 = (int)floor(fmax(ulo, 0.0));
                        T.y0 = (int)floor(fmax(vlo, 0.0));
                        T.x1 = (int)ceil(fmin(uhi, (double)(W - 1)));
                        T.y1 = (int)ceil(fmin(vhi, (double)(H - 1)));
                        const long long area = (long long)(T.x1 - T.x0 + 1) * (T.y1 - T.y0 + 1);
                        if (area <= RD_SMALL) small = true;
                        else queue[atomicAdd(&nqueue, 1)] = T;   // at most one entry per lane: never more than RD_THREADS
                    }
                }
            }
        }
    }
    if (small && split == 0)
        for (int y = T.y0; y <= T.y1; ++y)
            for (int x = T.x0; x <= T.x1; ++x) fragment(T, cam, x, y, W, far, buf);
    __syncthreads();
    const int nq = nqueue;
    const int lane = tid & 63;
    const long long me = (long long)split * RD_WAVES + (tid >> 6), stride = (long long)gridDim.z * RD_WAVES;
    for (int q = 0; q < nq; ++q) {
        const Tri& Q = queue[q];
        const int tx = (Q.x1 - Q.x0 + 8) >> 3, ty = (Q.y1 - Q.y0 + 8) >> 3;
        const long long tiles = (long long)tx * ty;
        // tile k of face f belongs to wave (f + k) mod stride: a rule every workgroup of the chunk evaluates alike, whatever order its own queue
        // filled in (the rotation by f spreads triangles of fewer tiles than waves)
        long long first = (me - Q.face) % stride;
        if (first < 0) first += stride;
        for (long long tile = first; tile < tiles; tile += stride) {
            const int x = Q.x0 + (int)(tile % tx) * 8 + (lane & 7), y = Q.y0 + (int)(tile / tx) * 8 + (lane >> 3);
            if (x <= Q.x1 && y <= Q.y1) fragment(Q, cam, x, y, W, far, buf);
        }
    }
}

// ---- calc_xyz_bp_fast + mask2bbox_xyxy ----

__global__ __launch_bounds__(RD_THREADS) void xyz_init_kernel(int* __restrict__ xyxy, int N, int H, int W) {
    const int i = blockIdx.x * RD_THREADS + threadIdx.x;
    if (i >= N) return;
    xyxy[(size_t)i * 4 + 0] = W;
    xyxy[(size_t)i * 4 + 1] = H;
    xyxy[(size_t)i * 4 + 2] = -1;
    xyxy[(size_t)i * 4 + 3] = -1;
}

__device__ __forceinline__ int wave_min_i(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = min(v, __shfl_xor(v, o, 64));
    return v;
}
__device__ __forceinline__ int wave_max_i(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = max(v, __shfl_xor(v, o, 64));
    return v;
}

// One thread per pixel, `bpi` workgroups per instance.  xyz = R^T (depth K^-1 [x, y, 1] - t) in fp64, times the mask depth != 0; the mask's
// bounds: a wave's min / max through shuffles, then one integer atomic per wave and bound.
__global__ __launch_bounds__(RD_THREADS) void xyz_pixels_kernel(const float* __restrict__ depth, const double* __restrict__ Rm,
                                                                const double* __restrict__ tv, const double* __restrict__ Km, int H, int W,
                                                                int bpi, float* __restrict__ xyz, unsigned char* __restrict__ mask,
                                                                int* __restrict__ xyxy) {
    const int i = blockIdx.x / bpi;
    const int p = (blockIdx.x - i * bpi) * RD_THREADS + threadIdx.x;
    const int HW = H * W;
    int lx = W, ly = H, hx = -1, hy = -1;
    if (p < HW) {
        const size_t g = (size_t)i * HW + p;
        const float zf = depth[g];
        const bool m = zf != 0.f;
        float o0 = 0.f, o1 = 0.f, o2 = 0.f;
        if (m) {
            const int y = p / W, x = p - y * W;
            const Cam cam = load_cam(Km + (size_t)i * 9);
            const double* R = Rm + (size_t)i * 9;
            const double* t = tv + (size_t)i * 3;
            double dx, dy;
            pixel_ray(cam, x, y, dx, dy);
            const double z = (double)zf;
            const double px = z * dx - t[0], py = z * dy - t[1], pz = z - t[2];
            o0 = (float)fma(R[0], px, fma(R[3], py, R[6] * pz));
            o1 = (float)fma(R[1], px, fma(R[4], py, R[7] * pz));
            o2 = (float)fma(R[2], px, fma(R[5], py, R[8] * pz));
            lx = hx = x;
            ly = hy = y;
        }
        xyz[g * 3 + 0] = o0;
        xyz[g * 3 + 1] = o1;
        xyz[g * 3 + 2] = o2;
        mask[g] = m ? 1 : 0;
    }
    lx = wave_min_i(lx);
    ly = wave_min_i(ly);
    hx = wave_max_i(hx);
    hy = wave_max_i(hy);
    if ((threadIdx.x & 63) == 0 && hx >= 0) {
        int* b = xyxy + (size_t)i * 4;
        atomicMin(b + 0, lx);
        atomicMin(b + 1, ly);
        atomicMax(b + 2, hx);
        atomicMax(b + 3, hy);
    }
}

// the tool's record of an instance that is not visible (:142-150): the whole frame as the box
__global__ __launch_bounds__(RD_THREADS) void xyz_finalize_kernel(int* __restrict__ xyxy, int* __restrict__ visible, int N, int H, int W) {
    const int i = blockIdx.x * RD_THREADS + threadIdx.x;
    if (i >= N) return;
    int* b = xyxy + (size_t)i * 4;
    const bool vis = b[2] >= 0;
    if (!vis) {
        b[0] = 0;
        b[1] = 0;
        b[2] = W - 1;
        b[3] = H - 1;
    }
    visible[i] = vis ? 1 : 0;
}

bool frame_ok(int N, int H, int W) { return N > 0 && H > 0 && W > 0; }

// what the launches can index: H * W in an int, the pixel count of the batch in workgroups of RD_THREADS within a grid dimension
bool frame_fits(int N, int H, int W) {
    const long long hw = (long long)H * W;
    return hw <= 0x7fffffffLL - RD_THREADS && (long long)N * ((hw + RD_THREADS - 1) / RD_THREADS) <= 0x7fffffffLL;
}

// the argument rules the two rasterizer entry points share; `out` is the depth or the visibility buffer (csrc/render_loop.h states the rules
// of the rows once, for these and for the loops that render)
int raster_args(const RenderRows& a, const void* out) {
    if (!rows_pointers_ok(a) || !out) return GDRN_ERR_ARG;
    if (!frame_ok(a.N, a.H, a.W) || !rows_scalars_ok(a)) return GDRN_ERR_ARG;
    if (!host_in_range(a.labels_host, a.N, a.C)) return GDRN_ERR_ARG;
    if (!frame_fits(a.N, a.H, a.W) || cdiv(a.f_max, RD_THREADS) > 65535) return GDRN_ERR_SHAPE;
    return GDRN_OK;
}

// few workgroups (few instances of small meshes: their triangles are the large ones): split the tile walk further
int raster_split(int N, int chunks) {
    const long long wgs = (long long)N * chunks;
    int split = 1;
    if (wgs < RD_TARGET_WGS) split = (int)((RD_TARGET_WGS + wgs - 1) / wgs);
    return split > RD_MAX_SPLIT ? RD_MAX_SPLIT : split;
}

}  // namespace

extern "C" int gdrn_render_depth(const double* verts, const int* faces, const int* vert_off, const int* nverts, const int* face_off,
                                 const int* nfaces, int C, int f_max, const int* labels, const int* labels_host, const double* R,
                                 const double* t, const double* K, int N, int H, int W, double near, double far, float* depth, void* stream) {
    const int bad = raster_args({verts, faces, vert_off, nverts, face_off, nfaces, C, f_max, labels, labels_host, R, t, K, N, H, W, near, far}, depth);
    if (bad != GDRN_OK) return bad;
    const int chunks = cdiv(f_max, RD_THREADS);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const size_t n = (size_t)N * H * W;
    const unsigned blocks = (unsigned)((n + RD_THREADS - 1) / RD_THREADS);
    unsigned* bits = reinterpret_cast<unsigned*>(depth);
    GDRN_LAUNCH(render_clear_kernel, dim3(blocks), dim3(RD_THREADS), 0, st, bits, n);
    GDRN_CHECK_LAUNCH();
    GDRN_LAUNCH(render_raster_kernel<unsigned>, dim3(N, chunks, raster_split(N, chunks)), dim3(RD_THREADS), 0, st, verts, faces, vert_off, nverts,
                face_off, nfaces, C, labels, R, t, K, H, W, near, far, bits);
    GDRN_CHECK_LAUNCH();
    GDRN_LAUNCH(render_resolve_kernel, dim3(blocks), dim3(RD_THREADS), 0, st, bits, n);
    GDRN_CHECK_LAUNCH();
    return GDRN_OK;
}

// The rasterizer's walk with 64-bit keys: one pass, one 64-bit unsigned atomic min per fragment.
extern "C" int gdrn_render_visibility(const double* verts, const int* faces, const int* vert_off, const int* nverts, const int* face_off,
                                      const int* nfaces, int C, int f_max, const int* labels, const int* labels_host, const double* R,
                                      const double* t, const double* K, int N, int H, int W, double near, double far, unsigned long long* vis,
                                      void* stream) {
    const int bad = raster_args({verts, faces, vert_off, nverts, face_off, nfaces, C, f_max, labels, labels_host, R, t, K, N, H, W, near, far}, vis);
    if (bad != GDRN_OK) return bad;
    const int chunks = cdiv(f_max, RD_THREADS);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const size_t n = (size_t)N * H * W;
    GDRN_LAUNCH(render_clear_keys_kernel, dim3((unsigned)((n + RD_THREADS - 1) / RD_THREADS)), dim3(RD_THREADS), 0, st, vis, n);
    GDRN_CHECK_LAUNCH();
    GDRN_LAUNCH(render_raster_kernel<unsigned long long>, dim3(N, chunks, raster_split(N, chunks)), dim3(RD_THREADS), 0, st, verts, faces, vert_off,
                nverts, face_off, nfaces, C, labels, R, t, K, H, W, near, far, vis);
    GDRN_CHECK_LAUNCH();
    return GDRN_OK;
}

extern "C" int gdrn_xyz_from_depth(const float* depth, const double* R, const double* t, const double* K, int N, int H, int W, float* xyz,
                                   unsigned char* mask, int* xyxy, int* visible, void* stream) {
    if (!depth || !R || !t || !K || !xyz || !mask || !xyxy || !visible || !frame_ok(N, H, W)) return GDRN_ERR_ARG;
    if (!frame_fits(N, H, W)) return GDRN_ERR_SHAPE;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const int bpi = (int)(((long long)H * W + RD_THREADS - 1) / RD_THREADS);
    GDRN_LAUNCH(xyz_init_kernel, dim3(cdiv(N, RD_THREADS)), dim3(RD_THREADS), 0, st, xyxy, N, H, W);
    GDRN_CHECK_LAUNCH();
    GDRN_LAUNCH(xyz_pixels_kernel, dim3((unsigned)((long long)N * bpi)), dim3(RD_THREADS), 0, st, depth, R, t, K, H, W, bpi, xyz, mask, xyxy);
    GDRN_CHECK_LAUNCH();
    GDRN_LAUNCH(xyz_finalize_kernel, dim3(cdiv(N, RD_THREADS)), dim3(RD_THREADS), 0, st, xyxy, visible, N, H, W);
    GDRN_CHECK_LAUNCH();
    return GDRN_OK;
}
