// Shaded colour frames of posed meshes for gfx950: what the reference draws with lib/meshrenderer/meshrenderer_phong.py (render, render_many) and
// shader/depth_shader_phong.{vs,frag} -- vertex-colour Phong shading and a z-test between several posed objects in one image -- from the visibility
// buffers of gdrn_render_visibility (csrc/render.hip): gdrn_shade_frames.  The rules are stated with the entry point in include/gdrn_hip.h.
//
// One thread per frame pixel, a flat index over the F * H * W pixels of the call.  A thread reads its pixel's 8-byte key of every instance of its frame
// (a wave reads 512 contiguous bytes per instance, eight instances in flight), keeps the nearest one, rebuilds that face's camera-space vertices exactly as the rasterizer set
// them up, and evaluates ray, depth, weights and lighting in fp64.  depth / index / face leave as one dword per lane, 256 contiguous bytes per
// wave.  The 3-byte maps (rgb, the normal map, the background read) are repacked over the four lanes of a quad with one shuffle, so that three lanes
// of four move one aligned dword each -- 192 contiguous bytes per wave and store instruction instead of 3 x 64 single bytes.  Only the last,
// incomplete quad of a call moves bytes.  No scratch memory, no atomics, no read-back: repeated calls give the same bits.
//
// Floating-point contraction is OFF for this file and every fused operation is an explicit fma(), as in render.hip, whose vertex transform, sorted
// vertex order, ray and edge values this repeats.  (No 16-bit code: both library builds compile the same thing.)
#include "common.h"
#include "geom64.h"
#include "../../include/gdrn_hip.h"

#include <stdint.h>

#pragma clang fp contract(off)

#include "raster64.h"

namespace {

constexpr int SH_THREADS = 256;
constexpr unsigned SH_NONE = 0xffffffffu;   // the upper half of an empty key
constexpr int SH_AHEAD = 8;                 // keys of a frame's instances in flight per lane

__device__ __forceinline__ double dot3(V3 p, V3 q) { return fma(p.x, q.x, fma(p.y, q.y, p.z * q.z)); }
// p / |p|, the zero vector for |p| == 0
__device__ __forceinline__ V3 unit3(V3 p) {
    const double l = sqrt(dot3(p, p));
    return l > 0.0 ? V3{p.x / l, p.y / l, p.z / l} : V3{0.0, 0.0, 0.0};
}
// floor(255 v + 0.5) for v in [0, 1]; anything else (a NaN from a degenerate face) clamps into the byte
__device__ __forceinline__ unsigned quant(double v) {
    const double q = floor(fma(255.0, v, 0.5));
    return q >= 0.0 ? (q <= 255.0 ? (unsigned)q : 255u) : 0u;
}

// the three bytes of every pixel of a quad (lane & 3 = pixel, `v` = b0 | b1 << 8 | b2 << 16) as three dwords: lane j < 3 stores bytes 4j .. 4j + 3
// of the quad's 12.  `g` = the lane's flat pixel index, `total` = the pixels of the call; every lane of the wave calls this.
__device__ __forceinline__ void store_rgb_quad(unsigned char* __restrict__ out, long long g, long long total, unsigned v) {
    const int j = threadIdx.x & 3;
    const unsigned next = __shfl_down(v, 1, 64);   // (lane 3 of a quad never uses it)
    const long long q0 = g - j;                    // the quad's first pixel: a multiple of 4, so byte 3 q0 is dword-aligned
    if (q0 + 3 < total) {
        if (j < 3) reinterpret_cast<unsigned*>(out + 3 * q0)[j] = (v >> (8 * j)) | (next << (24 - 8 * j));
    } else if (g < total) {
        out[3 * g + 0] = (unsigned char)v;
        out[3 * g + 1] = (unsigned char)(v >> 8);
        out[3 * g + 2] = (unsigned char)(v >> 16);
    }
}

// the reverse: the lane's three bytes of a [total][3] byte map
__device__ __forceinline__ unsigned load_rgb_quad(const unsigned char* __restrict__ in, long long g, long long total) {
    const int j = threadIdx.x & 3;
    const long long q0 = g - j;
    const bool whole = q0 + 3 < total;
    unsigned d = 0u;
    if (whole && j < 3) d = reinterpret_cast<const unsigned*>(in + 3 * q0)[j];
    const unsigned prev = __shfl_up(d, 1, 64);   // (lane 0 of a quad never uses it)
    if (whole) return j == 0 ? (d & 0xffffffu) : (((prev >> (32 - 8 * j)) | (d << (8 * j))) & 0xffffffu);
    if (g < total) return (unsigned)in[3 * g] | ((unsigned)in[3 * g + 1] << 8) | ((unsigned)in[3 * g + 2] << 16);
    return 0u;
}

__global__ __launch_bounds__(SH_THREADS) void shade_kernel(const unsigned long long* __restrict__ vis, const double* __restrict__ verts,
                                                           const int* __restrict__ faces, const int* __restrict__ vert_off,
                                                           const int* __restrict__ nverts, const int* __restrict__ face_off,
                                                           const int* __restrict__ nfaces, const double* __restrict__ normals,
                                                           const double* __restrict__ colors, int C, const int* __restrict__ labels,
                                                           const double* __restrict__ Rm, const double* __restrict__ tv,
                                                           const double* __restrict__ Km, const int* __restrict__ off, const int* __restrict__ inst,
                                                           int N, int HW, int W, long long total, const double* __restrict__ light,
                                                           const double* __restrict__ phong, const unsigned char* __restrict__ background,
                                                           unsigned char* __restrict__ rgb, float* __restrict__ depth, int* __restrict__ index,
                                                           int* __restrict__ face_out, unsigned char* __restrict__ normal_map) {
    const long long g = (long long)blockIdx.x * SH_THREADS + threadIdx.x;
    const bool live = g < total;
    const int f = live ? (int)(g / HW) : 0;
    const int p = live ? (int)(g - (long long)f * HW) : 0;

    // instance: the smallest fp32 depth, the first in input order among equals
    unsigned best = SH_NONE, bface = 0u;
    int bi = -1;
    if (live) {
        // SH_AHEAD keys are loaded before the first is compared: one 8-byte load per lane and dependent step leaves the pass waiting on HBM latency
        const int j1 = off[f + 1];
        for (int j = off[f]; j < j1; j += SH_AHEAD) {
            unsigned long long key[SH_AHEAD];
            int row[SH_AHEAD];
#pragma unroll
            for (int u = 0; u < SH_AHEAD; ++u) {
                row[u] = j + u < j1 ? inst[j + u] : -1;
                // (a row outside [0, N): the host side of the entry point refuses such a table before the launch)
                key[u] = row[u] >= 0 && row[u] < N ? vis[(size_t)row[u] * HW + p] : ~0ull;
            }
#pragma unroll
            for (int u = 0; u < SH_AHEAD; ++u) {   // in input order: the empty key's upper half is never below `best`
                const unsigned zb = (unsigned)(key[u] >> 32);
                if (zb < best) {
                    best = zb;
                    bface = (unsigned)key[u];
                    bi = row[u];
                }
            }
        }
    }
    // a key this library did not write: a label, face or vertex outside the table leaves the pixel empty
    int ia = 0, ib = 0, ic = 0, c = 0;
    if (bi >= 0) {
        c = labels[bi];
        bool ok = c >= 0 && c < C;
        if (ok) ok = bface < (unsigned)nfaces[c];
        if (ok) {
            const int* fp = faces + ((size_t)face_off[c] + bface) * 3;
            int tmp;
            ia = fp[0], ib = fp[1], ic = fp[2];
            if (ia > ib) { tmp = ia; ia = ib; ib = tmp; }   // ascending vertex indices, as the rasterizer
            if (ib > ic) { tmp = ib; ib = ic; ic = tmp; }
            if (ia > ib) { tmp = ia; ia = ib; ib = tmp; }
            ok = ia >= 0 && ic < nverts[c];
        }
        if (!ok) bi = -1;
    }

    unsigned px_rgb = 0u, px_nrm = 0u;
    float zf = 0.f;
    if (bi >= 0) {
        double R[9], t[3];
#pragma unroll
        for (int k = 0; k < 9; ++k) R[k] = Rm[(size_t)bi * 9 + k];
#pragma unroll
        for (int k = 0; k < 3; ++k) t[k] = tv[(size_t)bi * 3 + k];
        const Cam cam = load_cam(Km + (size_t)bi * 9);
        const size_t v0 = (size_t)vert_off[c];
        const double* vb = verts + v0 * 3;
        const V3 a = xform(R, t, load3(vb + (size_t)ia * 3)), b = xform(R, t, load3(vb + (size_t)ib * 3)), cc = xform(R, t, load3(vb + (size_t)ic * 3));
        // the rasterizer's ray and edge values
        const int y = p / W, x = p - y * W;
        double dx, dy;
        pixel_ray(cam, x, y, dx, dy);
        const V3 e0 = cross(a, b), e1 = cross(b, cc), e2 = cross(a, cc);
        const double w0 = fma(dx, e0.x, fma(dy, e0.y, e0.z));     // d . (a x b): the weight of c
        const double w1 = fma(dx, e1.x, fma(dy, e1.y, e1.z));     // d . (b x c): the weight of a
        const double w2 = -fma(dx, e2.x, fma(dy, e2.y, e2.z));    // d . (c x a): the weight of b
        const double ws = (w1 + w2) + w0;
        const double wa = w1 / ws, wb = w2 / ws, wc = w0 / ws;
        const V3 ab = {b.x - a.x, b.y - a.y, b.z - a.z}, ac = {cc.x - a.x, cc.y - a.y, cc.z - a.z};
        const V3 n = cross(ab, ac);
        const double z = fma(n.x, a.x, fma(n.y, a.y, n.z * a.z)) / fma(dx, n.x, fma(dy, n.y, n.z));
        const V3 P = {z * dx, z * dy, z};
        // colour and normal of the pixel
        const double* cb = colors + v0 * 3;
        const double* nb = normals + v0 * 3;
        const V3 ca = load3(cb + (size_t)ia * 3), cB = load3(cb + (size_t)ib * 3), cC = load3(cb + (size_t)ic * 3);
        const V3 na = load3(nb + (size_t)ia * 3), nB = load3(nb + (size_t)ib * 3), nC = load3(nb + (size_t)ic * 3);
        const V3 col = {fma(wa, ca.x, fma(wb, cB.x, wc * cC.x)), fma(wa, ca.y, fma(wb, cB.y, wc * cC.y)), fma(wa, ca.z, fma(wb, cB.z, wc * cC.z))};
        const V3 nm = {fma(wa, na.x, fma(wb, nB.x, wc * nC.x)), fma(wa, na.y, fma(wb, nB.y, wc * nC.y)), fma(wa, na.z, fma(wb, nB.z, wc * nC.z))};
        const V3 Nn = unit3(V3{fma(R[0], nm.x, fma(R[1], nm.y, R[2] * nm.z)), fma(R[3], nm.x, fma(R[4], nm.y, R[5] * nm.z)),
                               fma(R[6], nm.x, fma(R[7], nm.y, R[8] * nm.z))});
        const double* lp = light + (size_t)f * 3;
        const V3 L = unit3(V3{lp[0] - P.x, lp[1] - P.y, lp[2] - P.z});
        const V3 V = unit3(V3{-P.x, -P.y, -P.z});
        const double nl = dot3(Nn, L);
        const double diff = fmax(nl, 0.0);
        const V3 Rv = {fma(2.0 * nl, Nn.x, -L.x), fma(2.0 * nl, Nn.y, -L.y), fma(2.0 * nl, Nn.z, -L.z)};
        const double spec = fmax(dot3(Rv, V), 0.0);   // (not gated on N . L > 0: depth_shader_phong.frag:26)
        const double* ph = phong + (size_t)f * 3;
        const double s = fma(ph[2], spec, fma(ph[1], diff, ph[0]));
        px_rgb = quant(fmin(1.0, s * col.x)) | (quant(fmin(1.0, s * col.y)) << 8) | (quant(fmin(1.0, s * col.z)) << 16);
        px_nrm = quant(fma(0.5, Nn.x, 0.5)) | (quant(fma(0.5, Nn.y, 0.5)) << 8) | (quant(fma(0.5, Nn.z, 0.5)) << 16);
        zf = __uint_as_float(best);
    }
    // (wave-uniform branches: the quad helpers shuffle)
    if (background) {
        const unsigned bg = load_rgb_quad(background, g, total);
        if (bi < 0) px_rgb = bg;
    }
    store_rgb_quad(rgb, g, total, px_rgb);
    if (normal_map) store_rgb_quad(normal_map, g, total, px_nrm);
    if (live) {
        depth[g] = zf;
        index[g] = bi;
        if (face_out) face_out[g] = bi >= 0 ? (int)bface : -1;
    }
}

}  // namespace

extern "C" int gdrn_shade_frames(const unsigned long long* vis, const double* verts, const int* faces, const int* vert_off, const int* nverts,
                                 const int* face_off, const int* nfaces, const double* normals, const double* colors, int C, const int* labels,
                                 const int* labels_host, const double* R, const double* t, const double* K, const int* inst_off,
                                 const int* inst_off_host, const int* inst, const int* inst_host, int F, int N, int H, int W, const double* light,
                                 const double* phong, const unsigned char* background, unsigned char* rgb, float* depth, int* index, int* face,
                                 unsigned char* normal_map, void* stream) {
    if (!verts || !faces || !vert_off || !nverts || !face_off || !nfaces || !normals || !colors || !inst_off || !inst_off_host || !light || !phong ||
        !rgb || !depth || !index)
        return GDRN_ERR_ARG;
    if (F <= 0 || N < 0 || H <= 0 || W <= 0 || C <= 0) return GDRN_ERR_ARG;
    if (((uintptr_t)rgb | (uintptr_t)normal_map | (uintptr_t)background) & 3) return GDRN_ERR_ARG;   // the 3-byte maps move as aligned dwords
    if (N > 0 && (!vis || !labels || !labels_host || !R || !t || !K || !inst || !inst_host)) return GDRN_ERR_ARG;
    if (inst_off_host[0] != 0 || inst_off_host[F] != N) return GDRN_ERR_ARG;
    for (int f = 0; f < F; ++f)
        if (inst_off_host[f + 1] < inst_off_host[f]) return GDRN_ERR_ARG;
    if (N > 0 && (!host_in_range(inst_host, N, N) || !host_in_range(labels_host, N, C))) return GDRN_ERR_ARG;
    // what the launch can index: H * W in an int, the pixels of the call in workgroups of SH_THREADS within a grid dimension
    const long long hw = (long long)H * W, total = hw * F;
    if (hw > 0x7fffffffLL || (total + SH_THREADS - 1) / SH_THREADS > 0x7fffffffLL) return GDRN_ERR_SHAPE;
    GDRN_LAUNCH(shade_kernel, dim3((unsigned)((total + SH_THREADS - 1) / SH_THREADS)), dim3(SH_THREADS), 0, reinterpret_cast<hipStream_t>(stream), vis,
                verts, faces, vert_off, nverts, face_off, nfaces, normals, colors, C, labels, R, t, K, inst_off, inst, N, (int)hw, W, total, light, phong,
                background, rgb, depth, index, face, normal_map);
    GDRN_CHECK_LAUNCH();
    return GDRN_OK;
}
