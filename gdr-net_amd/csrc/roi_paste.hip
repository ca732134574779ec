// Predicted instance masks in the frame for gfx950, the link between the network's mask head (postproc.hip ends at a [res][res] probability map
// in crop coordinates) and the steps that take an observed mask in frame coordinates (silhouette.hip, verify.hip, cou_metrics.hip, rle.hip) --
//   the largest 8-connected blob of every thresholded map                                                   -> gdrn_roi_components
//   B maps pasted into B frame-size masks, with area and box                                                -> gdrn_roi_paste_masks
//   the same paste with every frame pixel given to at most one RoI, and the index map of the winners        -> gdrn_roi_paste_exclusive
// The reference has no counterpart on the path; the arithmetic is stated with the entry points in include/gdrn_hip.h and restated on the host in
// tests/paste_host.py.  The paste is the inverse of the IDEAL crop map of get_affine_transform(center, scale, 0, res) -- crop index res / 2 at the
// centre, integer coordinates are pixel centres, zero border -- not of the 1/1024 fixed-point walk roi.hip follows for the forward crop.
//
// Components: one workgroup per RoI, the res^2 labels in LDS.  A foreground pixel starts as its own label (its row-major index); a round hooks the
// root of every pixel under the smallest label among its 8 neighbours (integer atomicMin in LDS) and then shortens every chain to its root.  Labels
// only fall and a root that was hooked never is a root again, so at most res^2 rounds change anything: the loop carries that bound explicitly.  The
// fixed point -- every pixel labelled with the smallest index of its component -- does not depend on the order in which the atomics land.
//
// Paste: a lane owns vectors of 16 consecutive bytes of ONE mask (row-major over H * W, so a vector may run over a row end); over 90 % of them lie
// wholly outside the RoI's square and cost two fp64 coordinates and a 16-byte store of zeros.  Inside, a pixel is four fp32 taps and the fixed
// fp64 sequence of the header.  A mask whose first byte is not 16-byte aligned (H * W no multiple of 16, or such a base) is written bytewise.
// Area and box: per lane, then LDS, then one integer atomic per workgroup and quantity, none from a workgroup without a set pixel.
//
// Exclusive paste: a gather.  A lane owns one vector of FRAME pixels and walks the rows of its frame in ascending order (CSR, built and checked
// on the host), keeping the greatest p above the threshold and its row per pixel -- strictly greater replaces, so equal p stays with the lowest
// row -- then walks the rows again and writes each row's vector, zeros included.  No atomics on values, no workspace, no influence across frames.
//
// Floating-point contraction is OFF for this file: p is one fixed fp64 operation sequence, which the host restatement repeats.
// (No 16-bit code: both library builds compile the same thing.)
#include "common.h"
#include "geom64.h"
#include "../../include/gdrn_hip.h"

#include <limits.h>

#pragma clang fp contract(off)

namespace {

constexpr int RP_THREADS = 256;
constexpr int RP_MAX_RES = 64;
constexpr int RP_VEC = 16;                        // pixels (bytes of a mask) per vector
constexpr int RP_VPT = 4;                         // vectors per lane of the plain paste: 64 bytes of stores in flight

// a non-finite value counts as 0; decided on the bit pattern
__device__ __forceinline__ float rp_finite_or_zero(float v) { return (__float_as_uint(v) & 0x7f800000u) == 0x7f800000u ? 0.f : v; }

// ---------------------------------------------------------------------------------------------------------------------
// components
// ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(RP_THREADS) void rp_components_kernel(const float* __restrict__ prob, int res, float thr, float* __restrict__ filtered,
                                                                    int* __restrict__ num_comp, int* __restrict__ kept_px) {
    __shared__ int s_lab[RP_MAX_RES * RP_MAX_RES];   // -1: background; otherwise a pixel of the same component with an index <= the pixel's own
    __shared__ int s_cnt[RP_MAX_RES * RP_MAX_RES];
    __shared__ int s_changed, s_ncomp;
    __shared__ unsigned s_best;
    const int b = blockIdx.x, tid = threadIdx.x, n = res * res;
    const float* pr = prob + (size_t)b * n;
    volatile int* lab = s_lab;                       // (chains are read while other lanes shorten them: every value met is an ancestor)
    for (int p = tid; p < n; p += RP_THREADS) {
        s_lab[p] = rp_finite_or_zero(pr[p]) > thr ? p : -1;
        s_cnt[p] = 0;
    }
    if (tid == 0) {
        s_ncomp = 0;
        s_best = 0u;
    }
    __syncthreads();
    for (int round = 0; round < n; ++round) {        // at most n rounds change anything (see above); no input makes this spin
        if (tid == 0) s_changed = 0;
        __syncthreads();
        for (int p = tid; p < n; p += RP_THREADS) {
            const int l = lab[p];
            if (l < 0) continue;
            const int y = p / res, x = p - y * res;
            int m = l;
            for (int dy = -1; dy <= 1; ++dy) {
                const int yy = y + dy;
                if (yy < 0 || yy >= res) continue;
                for (int dx = -1; dx <= 1; ++dx) {
                    const int xx = x + dx;
                    if (xx < 0 || xx >= res) continue;
                    const int lq = lab[yy * res + xx];
                    if (lq >= 0 && lq < m) m = lq;
                }
            }
            if (m < l) {
                atomicMin(&s_lab[l], m);
                s_changed = 1;
            }
        }
        __syncthreads();
        if (s_changed == 0) break;                   // uniform over the workgroup
        for (int p = tid; p < n; p += RP_THREADS) {
            int l = lab[p];
            if (l < 0) continue;
            for (int k = 0; k < n; ++k) {            // a chain falls strictly: fewer than n links
                const int up = lab[l];
                if (up == l) break;
                l = up;
            }
            lab[p] = l;
        }
        __syncthreads();
    }
    for (int p = tid; p < n; p += RP_THREADS) {
        const int l = s_lab[p];
        if (l >= 0) atomicAdd(&s_cnt[l], 1);
    }
    __syncthreads();
    for (int p = tid; p < n; p += RP_THREADS) {
        if (s_lab[p] != p) continue;                 // a root: the lowest row-major index of its component
        atomicAdd(&s_ncomp, 1);
        atomicMax(&s_best, ((unsigned)s_cnt[p] << 12) | (unsigned)(RP_MAX_RES * RP_MAX_RES - 1 - p));   // most pixels, then the lowest index
    }
    __syncthreads();
    const unsigned best = s_best;                    // 0: no component at all
    const int keep = best != 0u ? RP_MAX_RES * RP_MAX_RES - 1 - (int)(best & 4095u) : -2;
    float* out = filtered + (size_t)b * n;
    for (int p = tid; p < n; p += RP_THREADS) out[p] = s_lab[p] == keep ? pr[p] : 0.f;
    if (tid == 0) {
        num_comp[b] = s_ncomp;
        kept_px[b] = (int)(best >> 12);
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// paste
// ---------------------------------------------------------------------------------------------------------------------
struct RpGeo {
    const float* map;
    double cx, cy, k, half;
    int res;
};

// geom [B][3] fp64 = cx, cy, scale
__device__ __forceinline__ RpGeo rp_geo(const float* __restrict__ map, const double* __restrict__ geom, int n, int res) {
    RpGeo g;
    g.map = map + (size_t)n * res * res;
    g.cx = geom[(size_t)n * 3];
    g.cy = geom[(size_t)n * 3 + 1];
    g.k = (double)res / geom[(size_t)n * 3 + 2];
    g.half = 0.5 * (double)res;
    g.res = res;
    return g;
}
__device__ __forceinline__ double rp_coord(int c, double centre, const RpGeo& g) { return ((double)c - centre) * g.k + g.half; }
// -1 < u < res; false for a NaN (a pixel that is not inside is 0 and reads nothing)
__device__ __forceinline__ bool rp_inside(double u, const RpGeo& g) { return u > -1.0 && u < (double)g.res; }
__device__ __forceinline__ double rp_tap(const RpGeo& g, int v, int u) {
    if ((unsigned)v >= (unsigned)g.res || (unsigned)u >= (unsigned)g.res) return 0.0;
    return (double)rp_finite_or_zero(g.map[v * g.res + u]);
}
// p of a pixel with rp_inside(u) and rp_inside(v): the operation sequence of include/gdrn_hip.h
__device__ __forceinline__ double rp_value(const RpGeo& g, double u, double v) {
    const double u0 = floor(u), v0 = floor(v);
    const double fu = u - u0, fv = v - v0;
    const int iu = (int)u0, iv = (int)v0;            // within [-1, res - 1]
    const double m00 = rp_tap(g, iv, iu), m01 = rp_tap(g, iv, iu + 1), m10 = rp_tap(g, iv + 1, iu), m11 = rp_tap(g, iv + 1, iu + 1);
    const double a = m00 * (1.0 - fu) + m01 * fu;
    const double b = m10 * (1.0 - fu) + m11 * fu;
    return a * (1.0 - fv) + b * fv;
}

// f(j, x, y, p) for every pixel j of the vector [q0, q0 + 16) of one H x W map that lies inside the RoI's square (q0 < n_px; pixels at n_px and
// beyond do not exist).  A vector within one row is tested as a whole first: u does not fall as x grows.
template <class Fn>
__device__ __forceinline__ void rp_walk(const RpGeo& g, unsigned q0, unsigned n_px, int W, Fn&& f) {
    int y = (int)(q0 / (unsigned)W), x = (int)(q0 - (unsigned)y * (unsigned)W);
    double v = rp_coord(y, g.cy, g);
    if (x + RP_VEC <= W) {
        if (!rp_inside(v, g)) return;
        if (rp_coord(x + RP_VEC - 1, g.cx, g) <= -1.0 || rp_coord(x, g.cx, g) >= (double)g.res) return;
    }
#pragma unroll
    for (int j = 0; j < RP_VEC; ++j) {
        if (q0 + (unsigned)j < n_px) {
            const double u = rp_coord(x, g.cx, g);
            if (rp_inside(u, g) && rp_inside(v, g)) f(j, x, y, rp_value(g, u, v));
        }
        if (++x == W) {
            x = 0;
            ++y;
            v = rp_coord(y, g.cy, g);
        }
    }
}

// the 16 bytes of a vector from its 16 bits; whole and aligned: one 16-byte store
__device__ __forceinline__ unsigned rp_spread4(unsigned b) { return (b & 1u) | ((b & 2u) << 7) | ((b & 4u) << 14) | ((b & 8u) << 21); }
__device__ __forceinline__ void rp_store(unsigned char* __restrict__ out, bool aligned, unsigned q0, unsigned n_px, unsigned bits) {
    if (aligned && q0 + RP_VEC <= n_px) {
        *reinterpret_cast<uint4*>(out + q0) = make_uint4(rp_spread4(bits), rp_spread4(bits >> 4), rp_spread4(bits >> 8), rp_spread4(bits >> 12));
        return;
    }
#pragma unroll
    for (int j = 0; j < RP_VEC; ++j)
        if (q0 + (unsigned)j < n_px) out[q0 + j] = (unsigned char)((bits >> j) & 1u);
}

struct RpBox {
    int cnt, x1, y1, x2, y2;
    __device__ __forceinline__ void clear() { cnt = 0; x1 = INT_MAX; y1 = INT_MAX; x2 = -1; y2 = -1; }
    __device__ __forceinline__ void add(int x, int y) {
        ++cnt;
        x1 = min(x1, x); y1 = min(y1, y); x2 = max(x2, x); y2 = max(y2, y);
    }
};
__device__ __forceinline__ void rp_box_clear(int* s) { s[0] = 0; s[1] = INT_MAX; s[2] = INT_MAX; s[3] = -1; s[4] = -1; }
__device__ __forceinline__ void rp_box_fold(int* s, const RpBox& b) {      // LDS
    if (b.cnt == 0) return;
    atomicAdd(&s[0], b.cnt);
    atomicMin(&s[1], b.x1);
    atomicMin(&s[2], b.y1);
    atomicMax(&s[3], b.x2);
    atomicMax(&s[4], b.y2);
}
// lanes 0..4 of a workgroup: its five quantities onto the row's, unless it saw no set pixel
__device__ __forceinline__ void rp_box_flush(const int* s, int q, int* __restrict__ area, int* __restrict__ bbox, int n) {
    if (s[0] == 0) return;
    if (q == 0) atomicAdd(&area[n], s[0]);
    else if (q <= 2) atomicMin(&bbox[(size_t)n * 4 + (q - 1)], s[q]);
    else atomicMax(&bbox[(size_t)n * 4 + (q - 1)], s[q]);
}

__global__ __launch_bounds__(RP_THREADS) void rp_stats_init_kernel(int* __restrict__ area, int* __restrict__ bbox, int B) {
    const int n = blockIdx.x * RP_THREADS + threadIdx.x;
    if (n >= B) return;
    area[n] = 0;
    bbox[(size_t)n * 4 + 0] = INT_MAX;
    bbox[(size_t)n * 4 + 1] = INT_MAX;
    bbox[(size_t)n * 4 + 2] = -1;
    bbox[(size_t)n * 4 + 3] = -1;
}
__global__ __launch_bounds__(RP_THREADS) void rp_stats_final_kernel(const int* __restrict__ area, int* __restrict__ bbox, int B, int H, int W) {
    const int n = blockIdx.x * RP_THREADS + threadIdx.x;
    if (n >= B || area[n] != 0) return;
    bbox[(size_t)n * 4 + 0] = 0;   // an empty mask: the whole frame, as gdrn_rle_count writes it
    bbox[(size_t)n * 4 + 1] = 0;
    bbox[(size_t)n * 4 + 2] = W - 1;
    bbox[(size_t)n * 4 + 3] = H - 1;
}

// Workgroup blockIdx.x = n * bpi + chunk: RP_THREADS * RP_VPT vectors of mask n.
__global__ __launch_bounds__(RP_THREADS) void rp_paste_kernel(const float* __restrict__ map, const double* __restrict__ geom, int res, unsigned n_px,
                                                               int W, unsigned nvec, int bpi, double thr, unsigned char* __restrict__ mask,
                                                               int* __restrict__ area, int* __restrict__ bbox) {
    __shared__ int s_box[5];
    const int n = blockIdx.x / bpi, chunk = blockIdx.x - n * bpi, tid = threadIdx.x;
    if (tid == 0) rp_box_clear(s_box);
    __syncthreads();
    const RpGeo g = rp_geo(map, geom, n, res);
    unsigned char* out = mask + (size_t)n * n_px;
    const bool aligned = (reinterpret_cast<uintptr_t>(out) & 15) == 0;
    RpBox box;
    box.clear();
#pragma unroll
    for (int i = 0; i < RP_VPT; ++i) {
        const unsigned k = ((unsigned)chunk * RP_VPT + i) * RP_THREADS + tid;
        if (k >= nvec) continue;
        const unsigned q0 = k * RP_VEC;
        unsigned bits = 0u;
        rp_walk(g, q0, n_px, W, [&](int j, int x, int y, double p) {
            if (p > thr) {
                bits |= 1u << j;
                box.add(x, y);
            }
        });
        rp_store(out, aligned, q0, n_px, bits);
    }
    rp_box_fold(s_box, box);
    __syncthreads();
    if (tid < 5) rp_box_flush(s_box, tid, area, bbox, n);
}

// Workgroup blockIdx.x = f * bpi + chunk: RP_THREADS vectors of frame f.  csr [F + 1 + B] int32: the offsets of the frames, then the rows of
// frame 0, frame 1, ... each in ascending order (gdrn_roi_paste_exclusive compares its host copy with frame_host before the launch).
__global__ __launch_bounds__(RP_THREADS) void rp_exclusive_kernel(const float* __restrict__ map, const double* __restrict__ geom,
                                                                   const int* __restrict__ csr, int B, int F, int res, unsigned n_px, int W,
                                                                   unsigned nvec, int bpi, double thr, int* __restrict__ index,
                                                                   unsigned char* __restrict__ mask, int* __restrict__ area, int* __restrict__ bbox) {
    __shared__ int s_box[2][5];
    const int f = blockIdx.x / bpi, chunk = blockIdx.x - f * bpi, tid = threadIdx.x;
    if (tid < 2) rp_box_clear(s_box[tid]);
    __syncthreads();
    const unsigned k = (unsigned)chunk * RP_THREADS + tid;
    const bool active = k < nvec;
    const unsigned q0 = k * RP_VEC;
    const int beg = max(csr[f], 0), end = min(csr[f + 1], B);
    const int* rows = csr + (F + 1);
    double best_p[RP_VEC];
    int best_n[RP_VEC];
#pragma unroll
    for (int j = 0; j < RP_VEC; ++j) {
        best_p[j] = 0.0;
        best_n[j] = -1;
    }
    for (int i = beg; i < end; ++i) {
        const int n = rows[i];
        if (!active || n < 0 || n >= B) continue;
        const RpGeo g = rp_geo(map, geom, n, res);
        rp_walk(g, q0, n_px, W, [&](int j, int, int, double p) {
            if (p > thr && (best_n[j] < 0 || p > best_p[j])) {   // strictly greater: equal p stays with the lower row
                best_p[j] = p;
                best_n[j] = n;
            }
        });
    }
    if (active) {
        int* idx = index + (size_t)f * n_px + q0;
        if (q0 + RP_VEC <= n_px && (reinterpret_cast<uintptr_t>(idx) & 15) == 0) {
#pragma unroll
            for (int j = 0; j < RP_VEC; j += 4) *reinterpret_cast<int4*>(idx + j) = make_int4(best_n[j], best_n[j + 1], best_n[j + 2], best_n[j + 3]);
        } else {
#pragma unroll
            for (int j = 0; j < RP_VEC; ++j)
                if (q0 + (unsigned)j < n_px) idx[j] = best_n[j];
        }
    }
    const int y0 = active ? (int)(q0 / (unsigned)W) : 0, x0 = active ? (int)(q0 - (unsigned)y0 * (unsigned)W) : 0;
    for (int i = beg; i < end; ++i) {                // uniform over the workgroup: one barrier per row
        const int n = rows[i];
        const bool valid = n >= 0 && n < B;          // (uniform; the host side has checked the list)
        int* s = s_box[(i - beg) & 1];
        if (active && valid) {
            unsigned bits = 0u;
#pragma unroll
            for (int j = 0; j < RP_VEC; ++j) bits |= (best_n[j] == n ? 1u : 0u) << j;
            unsigned char* out = mask + (size_t)n * n_px;
            rp_store(out, (reinterpret_cast<uintptr_t>(out) & 15) == 0, q0, n_px, bits);
            if (bits != 0u) {
                RpBox box;
                box.clear();
                int x = x0, y = y0;
#pragma unroll
                for (int j = 0; j < RP_VEC; ++j) {
                    if ((bits >> j) & 1u) box.add(x, y);
                    if (++x == W) {
                        x = 0;
                        ++y;
                    }
                }
                rp_box_fold(s, box);
            }
        }
        __syncthreads();
        if (valid && tid < 5) {
            rp_box_flush(s, tid, area, bbox, n);
            // the slot is cleared behind its flush by the lanes that read it, and used again two rows on, behind the next row's barrier
            s[tid] = tid == 0 ? 0 : (tid <= 2 ? INT_MAX : -1);
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------------------------
bool rp_finite(double v) { return fabs(v) < __builtin_inf(); }   // false for a NaN
bool rp_thr_ok(float thr) { return thr >= 0.f && thr < __builtin_inff(); }
bool rp_res_ok(int res) { return res >= 2 && res <= RP_MAX_RES; }
// n maps of H x W: n >= 0, both sides >= 1, fewer than 2^31 pixels in all
bool rp_frames_ok(int n, int H, int W) {
    if (n < 0 || H < 1 || W < 1) return false;
    const long long hw = (long long)H * W;
    return hw < (1LL << 31) && (long long)n * hw < (1LL << 31);
}
bool rp_geom_ok(const double* geom_host, int B) {
    for (int n = 0; n < B; ++n) {
        const double cx = geom_host[(size_t)n * 3], cy = geom_host[(size_t)n * 3 + 1], scale = geom_host[(size_t)n * 3 + 2];
        if (!rp_finite(cx) || !rp_finite(cy) || !rp_finite(scale) || !(scale > 0.0)) return false;
    }
    return true;
}
// csr_host is exactly the CSR of frame_host: offsets from the counts, the rows of every frame in ascending order
bool rp_csr_ok(const int* frame_host, const int* csr_host, int B, int F) {
    if (csr_host[0] != 0 || csr_host[F] != B) return false;
    for (int f = 0; f < F; ++f)
        if (csr_host[f + 1] < csr_host[f]) return false;
    const int* rows = csr_host + (F + 1);
    for (int f = 0; f < F; ++f)
        for (int i = csr_host[f]; i < csr_host[f + 1]; ++i) {
            const int n = rows[i];
            if (n < 0 || n >= B || frame_host[n] != f || (i > csr_host[f] && rows[i - 1] >= n)) return false;
        }
    return true;
}

int rp_stats_init(int* area, int* bbox, int B, hipStream_t st) {
    GDRN_LAUNCH(rp_stats_init_kernel, dim3(cdiv(B, RP_THREADS)), dim3(RP_THREADS), 0, st, area, bbox, B);
    GDRN_CHECK_LAUNCH();
    return GDRN_OK;
}
int rp_stats_final(int* area, int* bbox, int B, int H, int W, hipStream_t st) {
    GDRN_LAUNCH(rp_stats_final_kernel, dim3(cdiv(B, RP_THREADS)), dim3(RP_THREADS), 0, st, (const int*)area, bbox, B, H, W);
    GDRN_CHECK_LAUNCH();
    return GDRN_OK;
}

}  // namespace

extern "C" int gdrn_roi_components(const float* prob, int B, int res, float thr, float* filtered, int* num_comp, int* kept_px, void* stream) {
    if (B < 0 || !rp_res_ok(res) || !rp_thr_ok(thr) || !rp_frames_ok(B, res, res)) return GDRN_ERR_ARG;
    if (B == 0) return GDRN_OK;
    if (!prob || !filtered || !num_comp || !kept_px) return GDRN_ERR_ARG;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    GDRN_LAUNCH(rp_components_kernel, dim3(B), dim3(RP_THREADS), 0, st, prob, res, thr, filtered, num_comp, kept_px);
    GDRN_CHECK_LAUNCH();
    return GDRN_OK;
}

extern "C" int gdrn_roi_paste_masks(const float* map, const double* geom, const double* geom_host, int B, int res, int H, int W, float thr,
                                    unsigned char* mask, int* area, int* bbox, void* stream) {
    if (B < 0 || !rp_res_ok(res) || !rp_frames_ok(B, H, W) || !rp_thr_ok(thr)) return GDRN_ERR_ARG;
    if (B == 0) return GDRN_OK;
    if (!map || !geom || !geom_host || !mask || !area || !bbox) return GDRN_ERR_ARG;
    if (!rp_geom_ok(geom_host, B)) return GDRN_ERR_ARG;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    int bad = rp_stats_init(area, bbox, B, st);
    if (bad != GDRN_OK) return bad;
    const unsigned n_px = (unsigned)H * (unsigned)W, nvec = (n_px + RP_VEC - 1) / RP_VEC;
    const int bpi = (int)((nvec + RP_THREADS * RP_VPT - 1) / (RP_THREADS * RP_VPT));
    GDRN_LAUNCH(rp_paste_kernel, dim3((unsigned)B * (unsigned)bpi), dim3(RP_THREADS), 0, st, map, geom, res, n_px, W, nvec, bpi, (double)thr, mask, area,
                bbox);
    GDRN_CHECK_LAUNCH();
    return rp_stats_final(area, bbox, B, H, W, st);
}

extern "C" int gdrn_roi_paste_exclusive(const float* map, const double* geom, const double* geom_host, const int* frame_host, const int* csr,
                                        const int* csr_host, int B, int F, int res, int H, int W, float thr, int* index, unsigned char* mask,
                                        int* area, int* bbox, void* stream) {
    if (B < 0 || F < 0 || !rp_res_ok(res) || !rp_frames_ok(B, H, W) || !rp_frames_ok(F, H, W) || !rp_thr_ok(thr)) return GDRN_ERR_ARG;
    if (B == 0) return GDRN_OK;                      // nothing is written, the index map included
    if (!frame_host || !host_in_range(frame_host, B, F)) return GDRN_ERR_ARG;
    if (!map || !geom || !geom_host || !csr || !csr_host || !index || !mask || !area || !bbox) return GDRN_ERR_ARG;
    if (!rp_geom_ok(geom_host, B) || !rp_csr_ok(frame_host, csr_host, B, F)) return GDRN_ERR_ARG;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const int bad = rp_stats_init(area, bbox, B, st);
    if (bad != GDRN_OK) return bad;
    const unsigned n_px = (unsigned)H * (unsigned)W, nvec = (n_px + RP_VEC - 1) / RP_VEC;
    const int bpi = (int)((nvec + RP_THREADS - 1) / RP_THREADS);
    GDRN_LAUNCH(rp_exclusive_kernel, dim3((unsigned)F * (unsigned)bpi), dim3(RP_THREADS), 0, st, map, geom, csr, B, F, res, n_px, W, nvec, bpi,
                (double)thr, index, mask, area, bbox);
    GDRN_CHECK_LAUNCH();
    return rp_stats_final(area, bbox, B, H, W, st);
}
