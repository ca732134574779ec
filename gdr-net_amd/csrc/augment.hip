// Background replacement and colour augmentation of whole training frames for gfx950: the host-side block the reference runs per sample between
// decoding and cropping, for a batch of frames (of any sizes) per launch, with the frames, masks and background bank resident in HBM:
//   replace_bg / get_bg_image + TRUNCATE_FG          core/base_data_loader.py:320-403, core/utils/data_utils.py:161-187 (cv2.resize, 8-bit bilinear)
//   INPUT.COLOR_AUG_CODE (imgaug Sequential)         core/gdrn_modeling/data_loader.py:337-343 -- CoarseDropout, GaussianBlur, then the point
//                                                    operations (Add, Invert, Multiply, LinearContrast) as one 3 x 256 table per frame
// The arithmetic is specified stage by stage in include/gdrn_hip.h; every stage is integer or strictly ordered fp32 / fp64, so the output is
// bit-identical to the host restatement (tests/aug_host.py) as long as no FMA contraction happens -- hence the pragma below.
// Two launches: aug_mask_cuts_kernel (bounding box of the mask -> kept row / column range, one workgroup per frame) and aug_frames_kernel (one
// workgroup per 32 x 32 output tile: background sample + composite + dropout into LDS with a halo of the blur radius, the two blur passes through
// a second LDS buffer, the table, the stores).  These kernels are gather / HBM bound; there is nothing here for the matrix cores.
#include "common.h"
#include "../../include/gdrn_hip.h"

#include <limits.h>
#include <math.h>

#pragma clang fp contract(off)

namespace {

constexpr int TILE = 32;
constexpr int RMAX = GDRN_AUG_MAX_RADIUS;
constexpr int HALO = TILE + 2 * RMAX;   // 40: widest staged region
constexpr int CUT_THREADS = 1024;

__device__ __forceinline__ void found(int y, int x, int& rmin, int& rmax, int& cmin, int& cmax) {
    rmin = min(rmin, y);
    rmax = max(rmax, y);
    cmin = min(cmin, x);
    cmax = max(cmax, x);
}

// one workgroup per frame: inclusive bounds of mask != 0 (integers), then the TRUNCATE_FG cut of replace_bg in fp64 -> kept half-open ranges
__global__ __launch_bounds__(CUT_THREADS) void aug_mask_cuts_kernel(const gdrn_aug_task* __restrict__ tasks, int* __restrict__ cuts) {
    __shared__ int box[4];
    const int n = blockIdx.x;
    const unsigned char* __restrict__ mask = tasks[n].mask;
    if (!mask) return;   // (uniform over the workgroup)
    const int H = tasks[n].H, W = tasks[n].W;
    if (threadIdx.x == 0) { box[0] = INT_MAX; box[1] = -1; box[2] = INT_MAX; box[3] = -1; }
    __syncthreads();
    int rmin = INT_MAX, rmax = -1, cmin = INT_MAX, cmax = -1;
    const long long total = (long long)H * W;
    const bool aligned = (reinterpret_cast<uintptr_t>(mask) & 7) == 0;
    for (long long i = (long long)threadIdx.x * 8; i < total; i += (long long)CUT_THREADS * 8) {
        const int cnt = (int)(total - i < 8 ? total - i : 8);
        unsigned long long w = 0;
        if (aligned && cnt == 8) {
            w = *reinterpret_cast<const unsigned long long*>(mask + i);
        } else {
            for (int k = 0; k < cnt; k++) w |= (unsigned long long)mask[i + k] << (8 * k);
        }
        if (w) {
            int y = (int)(i / W), x = (int)(i - (long long)y * W);
            for (int k = 0; k < cnt; k++) {
                if ((w >> (8 * k)) & 0xff) found(y, x, rmin, rmax, cmin, cmax);
                if (++x == W) { x = 0; ++y; }
            }
        }
    }
    if (rmax >= 0) {
        atomicMin(&box[0], rmin);
        atomicMax(&box[1], rmax);
        atomicMin(&box[2], cmin);
        atomicMax(&box[3], cmax);
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    int r0 = 0, r1 = H, c0 = 0, c1 = W;
    if (box[1] < 0) {
        r1 = 0;   // empty mask: nothing is kept, the whole frame becomes background
        c1 = 0;
    } else {
        const double u = tasks[n].trunc_u;
        const double lo_r = (double)box[0], hi_r = (double)box[1], lo_c = (double)box[2], hi_c = (double)box[3];
        const double c_h = 0.5 * (double)(box[0] + box[1]), c_w = 0.5 * (double)(box[2] + box[3]);
        switch (tasks[n].trunc_mode) {
            case 0: r0 = (int)(lo_r + (c_h - lo_r) * u); break;    // block upper: rows < k cleared
            case 1: r1 = (int)(c_h + (hi_r - c_h) * u); break;     // block bottom: rows >= k cleared
            case 2: c0 = (int)(lo_c + (c_w - lo_c) * u); break;    // block left
            case 3: c1 = (int)(c_w + (hi_c - c_w) * u); break;     // block right
            default: break;
        }
        r0 = min(max(r0, 0), H);
        r1 = min(max(r1, 0), H);
        c0 = min(max(c0, 0), W);
        c1 = min(max(c1, 0), W);
    }
    int* o = cuts + (size_t)n * 4;
    o[0] = r0; o[1] = r1; o[2] = c0; o[3] = c1;
}

// cv2.resize's INTER_LINEAR source position and 11-bit weights of destination coordinate d (n source samples)
__device__ __forceinline__ void lin_coord(int d, double inv, int n, int& s, int& a0, int& a1) {
    float f = (float)(((double)d + 0.5) * inv - 0.5);
    float fl = floorf(f);
    fl = fminf(fmaxf(fl, -1.f), 1.0e9f);   // (keeps the int conversion defined; anything outside is clamped just below anyway)
    int si = (int)fl;
    f -= (float)si;
    if (si < 0) { si = 0; f = 0.f; }
    if (si >= n - 1) { si = n - 1; f = 0.f; }
    s = si;
    a0 = (int)rintf((1.f - f) * 2048.f);
    a1 = (int)rintf(f * 2048.f);
}

struct Rgb {
    int c[3];
};

// stages background sample .. dropout for frame pixel (y, x); interior: (y, x) is an output pixel of this tile (mask_trunc is written once)
__device__ __forceinline__ Rgb composed_pixel(const gdrn_aug_task& t, const unsigned char* __restrict__ aux, const int* cut, int y, int x, bool interior) {
    Rgb v;
    const size_t p = (size_t)y * t.W + x;
    bool fg = true;
    if (t.mask) {
        fg = t.mask[p] != 0 && y >= cut[0] && y < cut[1] && x >= cut[2] && x < cut[3];
        if (interior && t.mask_trunc) t.mask_trunc[p] = fg ? 1 : 0;
    }
    if (fg) {
        const unsigned char* q = t.frame + p * 3;
        v.c[0] = q[0]; v.c[1] = q[1]; v.c[2] = q[2];
    } else if (y < t.oh && x < t.ow) {
        int sx, a0, a1, sy, b0, b1;
        lin_coord(x, t.inv_scale, t.cw, sx, a0, a1);
        lin_coord(y, t.inv_scale, t.ch, sy, b0, b1);
        const int sx1 = min(sx + 1, t.cw - 1), sy1 = min(sy + 1, t.ch - 1);
        const unsigned char* r0 = t.bg + (size_t)sy * t.bg_w * 3;
        const unsigned char* r1 = t.bg + (size_t)sy1 * t.bg_w * 3;
#pragma unroll
        for (int c = 0; c < 3; c++) {
            const int S0 = r0[sx * 3 + c] * a0 + r0[sx1 * 3 + c] * a1;
            const int S1 = r1[sx * 3 + c] * a0 + r1[sx1 * 3 + c] * a1;
            v.c[c] = min((((b0 * (S0 >> 4)) >> 16) + ((b1 * (S1 >> 4)) >> 16) + 2) >> 2, 255);   // (cv2 saturates; the weights never get there)
        }
    } else {
        v.c[0] = v.c[1] = v.c[2] = 0;
    }
    if (t.gh > 0) {
        const int cy = min((int)floor((double)y * (double)t.gh / (double)t.H), t.gh - 1);
        const int cx = min((int)floor((double)x * (double)t.gw / (double)t.W), t.gw - 1);
        if (aux[(size_t)t.keep_off + (size_t)cy * t.gw + cx] == 0) v.c[0] = v.c[1] = v.c[2] = 0;
    }
    return v;
}

__device__ __forceinline__ void store_pixel(const gdrn_aug_task& t, const unsigned char* __restrict__ aux, int y, int x, const Rgb& v) {
    unsigned char* o = t.out + ((size_t)y * t.W + x) * 3;
    if (t.lut_off >= 0) {
        const unsigned char* lut = aux + t.lut_off;
        o[0] = lut[v.c[0]];
        o[1] = lut[256 + v.c[1]];
        o[2] = lut[512 + v.c[2]];
    } else {
        o[0] = (unsigned char)v.c[0];
        o[1] = (unsigned char)v.c[1];
        o[2] = (unsigned char)v.c[2];
    }
}

// reflect-101 of a coordinate at most r outside [0, n), n > r; anything further out (tile overhang past the frame) is reported as -1
__device__ __forceinline__ int reflect101(int v, int n) {
    if (v < 0) v = -v;
    if (v >= n) v = 2 * n - 2 - v;
    return (v >= 0 && v < n) ? v : -1;
}

__global__ __launch_bounds__(256) void aug_frames_kernel(const gdrn_aug_task* __restrict__ tasks, const unsigned char* __restrict__ aux,
                                                         const int* __restrict__ cuts) {
    __shared__ uchar4 staged[HALO * HALO];       // composed pixels of the tile + halo
    __shared__ float hpass[3][HALO * TILE];      // horizontal pass, planar
    __shared__ float wts[2 * RMAX + 1];
    const int n = blockIdx.z;
    const gdrn_aug_task t = tasks[n];
    const int x0 = blockIdx.x * TILE, y0 = blockIdx.y * TILE;
    if (x0 >= t.W || y0 >= t.H) return;   // the grid is sized by the largest frame of the batch (uniform exit)
    int cut[4] = {0, 0, 0, 0};
    if (t.mask) {
#pragma unroll
        for (int k = 0; k < 4; k++) cut[k] = cuts[(size_t)n * 4 + k];
    }
    const int r = t.blur_r;
    if (r == 0) {   // no halo, no passes
        for (int i = threadIdx.x; i < TILE * TILE; i += 256) {
            const int y = y0 + i / TILE, x = x0 + i % TILE;
            if (y < t.H && x < t.W) store_pixel(t, aux, y, x, composed_pixel(t, aux, cut, y, x, true));
        }
        return;
    }
    const int side = TILE + 2 * r, taps = 2 * r + 1;
    if (threadIdx.x < taps) wts[threadIdx.x] = tasks[n].blur_w[threadIdx.x];
    for (int i = threadIdx.x; i < side * side; i += 256) {
        const int ry = i / side, rx = i - ry * side;
        const int uy = y0 + ry - r, ux = x0 + rx - r;
        const int gy = reflect101(uy, t.H), gx = reflect101(ux, t.W);
        uchar4 s = make_uchar4(0, 0, 0, 0);
        if (gy >= 0 && gx >= 0) {
            const bool interior = ry >= r && ry < r + TILE && rx >= r && rx < r + TILE && uy < t.H && ux < t.W;
            const Rgb v = composed_pixel(t, aux, cut, gy, gx, interior);
            s = make_uchar4((unsigned char)v.c[0], (unsigned char)v.c[1], (unsigned char)v.c[2], 0);
        }
        staged[ry * HALO + rx] = s;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < side * TILE; i += 256) {
        const int ry = i / TILE, ox = i % TILE;
        const uchar4* row = staged + ry * HALO + ox;
        float a0 = wts[0] * (float)row[0].x, a1 = wts[0] * (float)row[0].y, a2 = wts[0] * (float)row[0].z;
        for (int k = 1; k < taps; k++) {
            const float w = wts[k];
            a0 = a0 + w * (float)row[k].x;
            a1 = a1 + w * (float)row[k].y;
            a2 = a2 + w * (float)row[k].z;
        }
        hpass[0][i] = a0;
        hpass[1][i] = a1;
        hpass[2][i] = a2;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < TILE * TILE; i += 256) {
        const int oy = i / TILE, ox = i % TILE;
        const int y = y0 + oy, x = x0 + ox;
        if (y >= t.H || x >= t.W) continue;
        Rgb v;
#pragma unroll
        for (int c = 0; c < 3; c++) {
            const float* col = hpass[c] + oy * TILE + ox;
            float a = wts[0] * col[0];
            for (int k = 1; k < taps; k++) a = a + wts[k] * col[k * TILE];
            v.c[c] = (int)fminf(fmaxf(rintf(a), 0.f), 255.f);
        }
        store_pixel(t, aux, y, x, v);
    }
}

// the argument checks of both entry points, on the host copy of the table
int check_tasks(const gdrn_aug_task* th, int B, long long aux_bytes, bool frames, int* max_h, int* max_w, bool* any_mask) {
    int status = GDRN_OK;
    *max_h = *max_w = 0;
    *any_mask = false;
    for (int i = 0; i < B; i++) {
        const gdrn_aug_task& t = th[i];
        if (t.H <= 0 || t.W <= 0) return GDRN_ERR_ARG;
        if (t.mask) {
            *any_mask = true;
            if (t.trunc_mode < 0 || t.trunc_mode > 4 || !(t.trunc_u >= 0.0 && t.trunc_u <= 1.0)) return GDRN_ERR_ARG;
        }
        *max_h = t.H > *max_h ? t.H : *max_h;
        *max_w = t.W > *max_w ? t.W : *max_w;
        if (!frames) continue;
        if (!t.frame || !t.out || t.out == t.frame) return GDRN_ERR_ARG;
        if (t.mask) {
            if (!t.bg || t.bg_h <= 0 || t.bg_w <= 0 || t.ch <= 0 || t.ch > t.bg_h || t.cw <= 0 || t.cw > t.bg_w) return GDRN_ERR_ARG;
            if (t.oh < 0 || t.oh > t.H || t.ow < 0 || t.ow > t.W || !(t.inv_scale > 0.0) || !(t.inv_scale < 1.0e6)) return GDRN_ERR_ARG;
        } else if (t.mask_trunc) {
            return GDRN_ERR_ARG;
        }
        if (t.gh != 0 || t.gw != 0 || t.keep_off != -1) {
            if (t.gh <= 0 || t.gw <= 0 || t.keep_off < 0) return GDRN_ERR_ARG;
            if ((long long)t.gh * t.gw > GDRN_AUG_MAX_CELLS) status = GDRN_ERR_SHAPE;
            else if ((long long)t.keep_off + (long long)t.gh * t.gw > aux_bytes) return GDRN_ERR_ARG;
        }
        if (t.lut_off != -1 && (t.lut_off < 0 || (long long)t.lut_off + 768 > aux_bytes)) return GDRN_ERR_ARG;
        if (t.blur_r < 0) return GDRN_ERR_ARG;
        if (t.blur_r > GDRN_AUG_MAX_RADIUS) status = GDRN_ERR_SHAPE;
        else if (t.blur_r > 0 && (t.H <= t.blur_r || t.W <= t.blur_r)) return GDRN_ERR_ARG;
    }
    return status;
}

}  // namespace

extern "C" int gdrn_aug_mask_cuts(const gdrn_aug_task* tasks_dev, const gdrn_aug_task* tasks_host, int B, int* cuts, void* stream) {
    if (!tasks_dev || !tasks_host || !cuts || B <= 0) return GDRN_ERR_ARG;
    if (B > 65535) return GDRN_ERR_SHAPE;
    int mh, mw;
    bool any_mask;
    const int st = check_tasks(tasks_host, B, 0, false, &mh, &mw, &any_mask);
    if (st != GDRN_OK) return st;
    if (!any_mask) return GDRN_OK;
    GDRN_LAUNCH(aug_mask_cuts_kernel, dim3(B), dim3(CUT_THREADS), 0, reinterpret_cast<hipStream_t>(stream), tasks_dev, cuts);
    GDRN_CHECK_LAUNCH();
    return GDRN_OK;
}

extern "C" int gdrn_aug_frames(const gdrn_aug_task* tasks_dev, const gdrn_aug_task* tasks_host, int B, const unsigned char* aux,
                               long long aux_bytes, const int* cuts, void* stream) {
    if (!tasks_dev || !tasks_host || B <= 0 || aux_bytes < 0 || (aux_bytes > 0 && !aux)) return GDRN_ERR_ARG;
    if (B > 65535) return GDRN_ERR_SHAPE;
    int mh, mw;
    bool any_mask;
    const int st = check_tasks(tasks_host, B, aux_bytes, true, &mh, &mw, &any_mask);
    if (st != GDRN_OK) return st;
    if (any_mask && !cuts) return GDRN_ERR_ARG;
    if (cdiv(mh, TILE) > 65535) return GDRN_ERR_SHAPE;
    GDRN_LAUNCH(aug_frames_kernel, dim3(cdiv(mw, TILE), cdiv(mh, TILE), B), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), tasks_dev, aux,
                cuts);
    GDRN_CHECK_LAUNCH();
    return GDRN_OK;
}
