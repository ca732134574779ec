// Shaded colour frames of posed meshes for gfx950: what the reference draws with lib/meshrenderer/meshrenderer_phong.py (render, render_many) and
// shader/depth_shader_phong.{vs,frag} -- vertex-colour Phong shading and a z-test between several posed objects in one image -- from the visibility
// buffers of gdrn_render_visibility (csrc/render.hip): gdrn_shade_frames.  gdrn_shade_frames_tex is the same pass with the light model of the BOP
// renderer lib/pysixd/renderer_py.py: a UV texture instead of vertex colours where the class has one, Phong or flat shading, no specular term.  The
// two kernels share the winner pick, the table checks and the geometry as device functions.  The rules are stated with the entry points in
// include/gdrn_hip.h.
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

// ---- what the two shade passes share: the winner of a pixel, the checks of its key against the table, the geometry of the winning face ----

struct Winner { unsigned best, bface; int bi; };   // the fp32 depth bits and the face of the winning key; bi: the instance's row, -1 = nothing drawn

// instance: the smallest fp32 depth, the first in input order among equals
__device__ __forceinline__ Winner pick_winner(const unsigned long long* __restrict__ vis, const int* __restrict__ off, const int* __restrict__ inst,
                                              int N, int HW, int f, int p, bool live) {
    Winner w = {SH_NONE, 0u, -1};
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
                if (zb < w.best) {
                    w.best = zb;
                    w.bface = (unsigned)key[u];
                    w.bi = row[u];
                }
            }
        }
    }
    return w;
}

// a key this library did not write: a label, face or vertex outside the table leaves the pixel empty (bi = -1).  ia <= ib <= ic: the face's vertex
// indices in ascending order, as the rasterizer; c: the class
__device__ __forceinline__ void check_face(Winner& w, const int* __restrict__ labels, int C, const int* __restrict__ faces,
                                           const int* __restrict__ face_off, const int* __restrict__ nfaces, const int* __restrict__ nverts, int& ia,
                                           int& ib, int& ic, int& c) {
    ia = ib = ic = c = 0;
    if (w.bi >= 0) {
        c = labels[w.bi];
        bool ok = c >= 0 && c < C;
        if (ok) ok = w.bface < (unsigned)nfaces[c];
        if (ok) {
            const int* fp = faces + ((size_t)face_off[c] + w.bface) * 3;
            int tmp;
            ia = fp[0], ib = fp[1], ic = fp[2];
            if (ia > ib) { tmp = ia; ia = ib; ib = tmp; }   // ascending vertex indices, as the rasterizer
            if (ib > ic) { tmp = ib; ib = ic; ic = tmp; }
            if (ia > ib) { tmp = ia; ia = ib; ib = tmp; }
            ok = ia >= 0 && ic < nverts[c];
        }
        if (!ok) w.bi = -1;
    }
}

// the winning face at the pixel: the pose's rotation, the camera-space vertices, the ray (dx, dy, 1), the normalised weights of a, b, c, the face
// normal n = (b - a) x (c - a), nd = n . d, z = (n . a) / nd and P = z d
struct Geom {
    double R[9];
    V3 a, b, cc, n, P;
    double dx, dy, wa, wb, wc, nd, z;
};

__device__ __forceinline__ Geom face_geometry(const double* __restrict__ vb, const double* __restrict__ Rm, const double* __restrict__ tv,
                                              const double* __restrict__ Km, int bi, int ia, int ib, int ic, int p, int W) {
    Geom g;
    double t[3];
#pragma unroll
    for (int k = 0; k < 9; ++k) g.R[k] = Rm[(size_t)bi * 9 + k];
#pragma unroll
    for (int k = 0; k < 3; ++k) t[k] = tv[(size_t)bi * 3 + k];
    const Cam cam = load_cam(Km + (size_t)bi * 9);
    g.a = xform(g.R, t, load3(vb + (size_t)ia * 3)), g.b = xform(g.R, t, load3(vb + (size_t)ib * 3)), g.cc = xform(g.R, t, load3(vb + (size_t)ic * 3));
    // the rasterizer's ray and edge values
    const int y = p / W, x = p - y * W;
    pixel_ray(cam, x, y, g.dx, g.dy);
    const V3 e0 = cross(g.a, g.b), e1 = cross(g.b, g.cc), e2 = cross(g.a, g.cc);
    const double w0 = fma(g.dx, e0.x, fma(g.dy, e0.y, e0.z));     // d . (a x b): the weight of c
    const double w1 = fma(g.dx, e1.x, fma(g.dy, e1.y, e1.z));     // d . (b x c): the weight of a
    const double w2 = -fma(g.dx, e2.x, fma(g.dy, e2.y, e2.z));    // d . (c x a): the weight of b
    const double ws = (w1 + w2) + w0;
    g.wa = w1 / ws, g.wb = w2 / ws, g.wc = w0 / ws;
    const V3 ab = {g.b.x - g.a.x, g.b.y - g.a.y, g.b.z - g.a.z}, ac = {g.cc.x - g.a.x, g.cc.y - g.a.y, g.cc.z - g.a.z};
    g.n = cross(ab, ac);
    g.nd = fma(g.dx, g.n.x, fma(g.dy, g.n.y, g.n.z));
    g.z = fma(g.n.x, g.a.x, fma(g.n.y, g.a.y, g.n.z * g.a.z)) / g.nd;
    g.P = V3{g.z * g.dx, g.z * g.dy, g.z};
    return g;
}

// wa A + wb B + wc C per component, the one nesting of every interpolated attribute
__device__ __forceinline__ V3 interp3(const Geom& g, const double* __restrict__ tab, int ia, int ib, int ic) {
    const V3 A = load3(tab + (size_t)ia * 3), B = load3(tab + (size_t)ib * 3), Cv = load3(tab + (size_t)ic * 3);
    return V3{fma(g.wa, A.x, fma(g.wb, B.x, g.wc * Cv.x)), fma(g.wa, A.y, fma(g.wb, B.y, g.wc * Cv.y)), fma(g.wa, A.z, fma(g.wb, B.z, g.wc * Cv.z))};
}

// unit(R n_interp): the interpolated vertex normal in camera coordinates
__device__ __forceinline__ V3 phong_normal(const Geom& g, const double* __restrict__ nb, int ia, int ib, int ic) {
    const V3 nm = interp3(g, nb, ia, ib, ic);
    return unit3(V3{fma(g.R[0], nm.x, fma(g.R[1], nm.y, g.R[2] * nm.z)), fma(g.R[3], nm.x, fma(g.R[4], nm.y, g.R[5] * nm.z)),
                    fma(g.R[6], nm.x, fma(g.R[7], nm.y, g.R[8] * nm.z))});
}

__device__ __forceinline__ unsigned quant_normal(V3 Nn) {
    return quant(fma(0.5, Nn.x, 0.5)) | (quant(fma(0.5, Nn.y, 0.5)) << 8) | (quant(fma(0.5, Nn.z, 0.5)) << 16);
}

// the tail of both passes: background, the 3-byte maps through the quad helpers, the dword maps.  (wave-uniform branches: the quad helpers shuffle)
__device__ __forceinline__ void store_pixel(long long g, long long total, bool live, const Winner& w, unsigned px_rgb, unsigned px_nrm,
                                            const unsigned char* __restrict__ background, unsigned char* __restrict__ rgb, float* __restrict__ depth,
                                            int* __restrict__ index, int* __restrict__ face_out, unsigned char* __restrict__ normal_map) {
    if (background) {
        const unsigned bg = load_rgb_quad(background, g, total);
        if (w.bi < 0) px_rgb = bg;
    }
    store_rgb_quad(rgb, g, total, px_rgb);
    if (normal_map) store_rgb_quad(normal_map, g, total, px_nrm);
    if (live) {
        depth[g] = w.bi >= 0 ? __uint_as_float(w.best) : 0.f;
        index[g] = w.bi;
        if (face_out) face_out[g] = w.bi >= 0 ? (int)w.bface : -1;
    }
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
    Winner w = pick_winner(vis, off, inst, N, HW, f, p, live);
    int ia, ib, ic, c;
    check_face(w, labels, C, faces, face_off, nfaces, nverts, ia, ib, ic, c);

    unsigned px_rgb = 0u, px_nrm = 0u;
    if (w.bi >= 0) {
        const size_t v0 = (size_t)vert_off[c];
        const Geom ge = face_geometry(verts + v0 * 3, Rm, tv, Km, w.bi, ia, ib, ic, p, W);
        // colour and normal of the pixel
        const V3 col = interp3(ge, colors + v0 * 3, ia, ib, ic);
        const V3 Nn = phong_normal(ge, normals + v0 * 3, ia, ib, ic);
        const double* lp = light + (size_t)f * 3;
        const V3 L = unit3(V3{lp[0] - ge.P.x, lp[1] - ge.P.y, lp[2] - ge.P.z});
        const V3 V = unit3(V3{-ge.P.x, -ge.P.y, -ge.P.z});
        const double nl = dot3(Nn, L);
        const double diff = fmax(nl, 0.0);
        const V3 Rv = {fma(2.0 * nl, Nn.x, -L.x), fma(2.0 * nl, Nn.y, -L.y), fma(2.0 * nl, Nn.z, -L.z)};
        const double spec = fmax(dot3(Rv, V), 0.0);   // (not gated on N . L > 0: depth_shader_phong.frag:26)
        const double* ph = phong + (size_t)f * 3;
        const double s = fma(ph[2], spec, fma(ph[1], diff, ph[0]));
        px_rgb = quant(fmin(1.0, s * col.x)) | (quant(fmin(1.0, s * col.y)) << 8) | (quant(fmin(1.0, s * col.z)) << 16);
        px_nrm = quant_normal(Nn);
    }
    store_pixel(g, total, live, w, px_rgb, px_nrm, background, rgb, depth, index, face_out, normal_map);
}

// ---- the BOP renderer's light model with UV textures and flat shading (lib/pysixd/renderer_py.py): gdrn_shade_frames_tex ----

// rint(255 v), round-half-to-even (np.round); anything outside the byte (a NaN from a degenerate face) clamps into it
__device__ __forceinline__ unsigned quant_even(double v) {
    const double q = rint(255.0 * v);
    return q >= 0.0 ? (q <= 255.0 ? (unsigned)q : 255u) : 0u;
}

// min(max(x, 0), hi) as an int: clamped in fp64, so that no |x| overflows the conversion (a NaN gives 0)
__device__ __forceinline__ int clamp_index(double x, int hi) { return (int)fmin(fmax(x, 0.0), (double)hi); }

__device__ __forceinline__ V3 texel3(unsigned t) { return V3{(double)(t & 0xffu), (double)((t >> 8) & 0xffu), (double)((t >> 16) & 0xffu)}; }

// the base colour of a textured class at (u, v): `tx` = the class's h x w texels in file order (row 0 = the top of the image); v = 0 is the
// bottom row, clamp-to-edge in both directions
template <int FILTER>
__device__ __forceinline__ V3 sample_texture(const unsigned* __restrict__ tx, int h, int w, double u, double v) {
    V3 s;
    if (FILTER == GDRN_TEXFILTER_NEAREST) {
        const int i = clamp_index(floor(u * (double)w), w - 1), j = clamp_index(floor(v * (double)h), h - 1);
        s = texel3(tx[(size_t)(h - 1 - j) * w + i]);
    } else {
        const double x = u * (double)w - 0.5, y = v * (double)h - 0.5;
        const double xf = floor(x), yf = floor(y);
        const double fx = x - xf, fy = y - yf;
        const int i0 = clamp_index(xf, w - 1), i1 = clamp_index(xf + 1.0, w - 1);
        const int j0 = clamp_index(yf, h - 1), j1 = clamp_index(yf + 1.0, h - 1);
        const unsigned* r0 = tx + (size_t)(h - 1 - j0) * w;
        const unsigned* r1 = tx + (size_t)(h - 1 - j1) * w;
        const V3 t00 = texel3(r0[i0]), t10 = texel3(r0[i1]), t01 = texel3(r1[i0]), t11 = texel3(r1[i1]);
        // x first, then y, on the byte values: every step is exact where the weights are dyadic
        const V3 lo = {fma(fx, t10.x - t00.x, t00.x), fma(fx, t10.y - t00.y, t00.y), fma(fx, t10.z - t00.z, t00.z)};
        const V3 hi = {fma(fx, t11.x - t01.x, t01.x), fma(fx, t11.y - t01.y, t01.y), fma(fx, t11.z - t01.z, t01.z)};
        s = V3{fma(fy, hi.x - lo.x, lo.x), fma(fy, hi.y - lo.y, lo.y), fma(fy, hi.z - lo.z, lo.z)};
    }
    return V3{s.x / 255.0, s.y / 255.0, s.z / 255.0};
}

template <int SHADING, int FILTER>
__global__ __launch_bounds__(SH_THREADS) void shade_tex_kernel(const unsigned long long* __restrict__ vis, const double* __restrict__ verts,
                                                               const int* __restrict__ faces, const int* __restrict__ vert_off,
                                                               const int* __restrict__ nverts, const int* __restrict__ face_off,
                                                               const int* __restrict__ nfaces, const double* __restrict__ normals,
                                                               const double* __restrict__ colors, const double* __restrict__ uvs,
                                                               const unsigned* __restrict__ texels, const int* __restrict__ tex, int C,
                                                               const int* __restrict__ labels, const double* __restrict__ Rm,
                                                               const double* __restrict__ tv, const double* __restrict__ Km,
                                                               const int* __restrict__ off, const int* __restrict__ inst, int N, int HW, int W,
                                                               long long total, const double* __restrict__ light, const double* __restrict__ ambient,
                                                               const unsigned char* __restrict__ background,
                                                               unsigned char* __restrict__ rgb, float* __restrict__ depth, int* __restrict__ index,
                                                               int* __restrict__ face_out, unsigned char* __restrict__ normal_map) {
    const long long g = (long long)blockIdx.x * SH_THREADS + threadIdx.x;
    const bool live = g < total;
    const int f = live ? (int)(g / HW) : 0;
    const int p = live ? (int)(g - (long long)f * HW) : 0;
    Winner w = pick_winner(vis, off, inst, N, HW, f, p, live);
    int ia, ib, ic, c;
    check_face(w, labels, C, faces, face_off, nfaces, nverts, ia, ib, ic, c);

    unsigned px_rgb = 0u, px_nrm = 0u;
    if (w.bi >= 0) {
        const size_t v0 = (size_t)vert_off[c];
        const Geom ge = face_geometry(verts + v0 * 3, Rm, tv, Km, w.bi, ia, ib, ic, p, W);
        V3 Nn;
        if (SHADING == GDRN_SHADING_FLAT) {   // the face normal, turned towards the camera: n . d <= 0
            Nn = unit3(ge.n);
            if (ge.nd > 0.0) Nn = V3{-Nn.x, -Nn.y, -Nn.z};
        } else {
            Nn = phong_normal(ge, normals + v0 * 3, ia, ib, ic);
        }
        const double* lp = light + (size_t)f * 3;
        const V3 L = unit3(V3{lp[0] - ge.P.x, lp[1] - ge.P.y, lp[2] - ge.P.z});
        const double lw = fmin(1.0, ambient[f] + fmax(dot3(Nn, L), 0.0));
        const int th = tex[(size_t)c * 3 + 1], tw = tex[(size_t)c * 3 + 2];
        V3 col;
        if (th > 0) {   // (the host side of the entry point refuses a texture that does not lie within texels)
            const double* ub = uvs + v0 * 2;
            const double u = fma(ge.wa, ub[(size_t)ia * 2], fma(ge.wb, ub[(size_t)ib * 2], ge.wc * ub[(size_t)ic * 2]));
            const double v = fma(ge.wa, ub[(size_t)ia * 2 + 1], fma(ge.wb, ub[(size_t)ib * 2 + 1], ge.wc * ub[(size_t)ic * 2 + 1]));
            col = sample_texture<FILTER>(texels + (size_t)tex[(size_t)c * 3], th, tw, u, v);
        } else {
            col = interp3(ge, colors + v0 * 3, ia, ib, ic);
        }
        px_rgb = quant_even(lw * col.x) | (quant_even(lw * col.y) << 8) | (quant_even(lw * col.z) << 16);
        px_nrm = quant_normal(Nn);
    }
    store_pixel(g, total, live, w, px_rgb, px_nrm, background, rgb, depth, index, face_out, normal_map);
}

// the host-side checks both entry points share; `hw` / `total`: the pixels of a frame and of the call
int check_frames_args(const void* vis, const void* verts, const void* faces, const void* vert_off, const void* nverts, const void* face_off,
                      const void* nfaces, const void* normals, const void* colors, int C, const int* labels, const int* labels_host, const void* R,
                      const void* t, const void* K, const int* inst_off, const int* inst_off_host, const int* inst, const int* inst_host, int F, int N,
                      int H, int W, const void* light, const void* weights, const void* background, const void* rgb, const void* depth,
                      const void* index, const void* normal_map, long long& hw, long long& total) {
    if (!verts || !faces || !vert_off || !nverts || !face_off || !nfaces || !normals || !colors || !inst_off || !inst_off_host || !light || !weights ||
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
    hw = (long long)H * W, total = hw * F;
    if (hw > 0x7fffffffLL || (total + SH_THREADS - 1) / SH_THREADS > 0x7fffffffLL) return GDRN_ERR_SHAPE;
    return GDRN_OK;
}

}  // namespace

extern "C" int gdrn_shade_frames(const unsigned long long* vis, const double* verts, const int* faces, const int* vert_off, const int* nverts,
                                 const int* face_off, const int* nfaces, const double* normals, const double* colors, int C, const int* labels,
                                 const int* labels_host, const double* R, const double* t, const double* K, const int* inst_off,
                                 const int* inst_off_host, const int* inst, const int* inst_host, int F, int N, int H, int W, const double* light,
                                 const double* phong, const unsigned char* background, unsigned char* rgb, float* depth, int* index, int* face,
                                 unsigned char* normal_map, void* stream) {
    long long hw, total;
    const int st = check_frames_args(vis, verts, faces, vert_off, nverts, face_off, nfaces, normals, colors, C, labels, labels_host, R, t, K, inst_off,
                                     inst_off_host, inst, inst_host, F, N, H, W, light, phong, background, rgb, depth, index, normal_map, hw, total);
    if (st != GDRN_OK) return st;
    GDRN_LAUNCH(shade_kernel, dim3((unsigned)((total + SH_THREADS - 1) / SH_THREADS)), dim3(SH_THREADS), 0, reinterpret_cast<hipStream_t>(stream), vis,
                verts, faces, vert_off, nverts, face_off, nfaces, normals, colors, C, labels, R, t, K, inst_off, inst, N, (int)hw, W, total, light, phong,
                background, rgb, depth, index, face, normal_map);
    GDRN_CHECK_LAUNCH();
    return GDRN_OK;
}

extern "C" int gdrn_shade_frames_tex(const unsigned long long* vis, const double* verts, const int* faces, const int* vert_off, const int* nverts,
                                     const int* face_off, const int* nfaces, const double* normals, const double* colors, const double* uvs,
                                     const unsigned int* texels, const int* tex, const int* tex_host, int n_texels, int C, const int* labels,
                                     const int* labels_host, const double* R, const double* t, const double* K, const int* inst_off,
                                     const int* inst_off_host, const int* inst, const int* inst_host, int F, int N, int H, int W, const double* light,
                                     const double* ambient, int shading, int filter, const unsigned char* background, unsigned char* rgb, float* depth,
                                     int* index, int* face, unsigned char* normal_map, void* stream) {
    if (!uvs || !tex || !tex_host || n_texels < 0 || (n_texels > 0 && !texels)) return GDRN_ERR_ARG;
    if ((shading != GDRN_SHADING_PHONG && shading != GDRN_SHADING_FLAT) || (filter != GDRN_TEXFILTER_NEAREST && filter != GDRN_TEXFILTER_BILINEAR))
        return GDRN_ERR_ARG;
    long long hw, total;
    const int st = check_frames_args(vis, verts, faces, vert_off, nverts, face_off, nfaces, normals, colors, C, labels, labels_host, R, t, K, inst_off,
                                     inst_off_host, inst, inst_host, F, N, H, W, light, ambient, background, rgb, depth, index, normal_map, hw, total);
    if (st != GDRN_OK) return st;
    for (int c = 0; c < C; ++c) {   // every texture lies within texels: offset >= 0, offset + h w <= n_texels, h and w both 0 or both in [1, 16384]
        const long long o = tex_host[3 * c], h = tex_host[3 * c + 1], w = tex_host[3 * c + 2];
        if (o < 0 || h < 0 || w < 0 || h > GDRN_TEX_MAX_SIDE || w > GDRN_TEX_MAX_SIDE || (h == 0) != (w == 0) || o + h * w > n_texels)
            return GDRN_ERR_ARG;
    }
    // shading and filter are uniform per call: one instantiation each, no branch and no registers for the path not taken
#define GDRN_TEX_LAUNCH(S, T)                                                                                                                         \
    GDRN_LAUNCH((shade_tex_kernel<S, T>), dim3((unsigned)((total + SH_THREADS - 1) / SH_THREADS)), dim3(SH_THREADS), 0,                             \
                reinterpret_cast<hipStream_t>(stream), vis, verts, faces, vert_off, nverts, face_off, nfaces, normals, colors, uvs, texels, tex, C, labels, \
                R, t, K, inst_off, inst, N, (int)hw, W, total, light, ambient, background, rgb, depth, index, face, normal_map)
    if (shading == GDRN_SHADING_PHONG) {
        if (filter == GDRN_TEXFILTER_NEAREST) GDRN_TEX_LAUNCH(GDRN_SHADING_PHONG, GDRN_TEXFILTER_NEAREST);
        else GDRN_TEX_LAUNCH(GDRN_SHADING_PHONG, GDRN_TEXFILTER_BILINEAR);
    } else {
        if (filter == GDRN_TEXFILTER_NEAREST) GDRN_TEX_LAUNCH(GDRN_SHADING_FLAT, GDRN_TEXFILTER_NEAREST);
        else GDRN_TEX_LAUNCH(GDRN_SHADING_FLAT, GDRN_TEXFILTER_BILINEAR);
    }
#undef GDRN_TEX_LAUNCH
    GDRN_CHECK_LAUNCH();
    return GDRN_OK;
}
