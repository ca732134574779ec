// COCO run-length masks (maskApi's compressed RLE strings) for gfx950, both ways, for a batch of masks of any sizes per call: what the reference
// does per sample on the host with pycocotools -- cocosegm2mask / rle2mask (lib/utils/mask_utils.py:93-125, core/gdrn_modeling/data_loader.py:79,
// 326,332) on the way in, binary_mask_to_rle (mask_utils.py:54-66, gdrn_evaluator.py:695-697) on the way out -- and mask2bbox_xyxy
// (mask_utils.py:39-44) with the pixel count.  The format is specified in include/gdrn_hip.h; everything here is integer and exact.
//   decode   rle_parse_kernel  one workgroup per mask walks the string in chunks of 1024 characters: token ends, token values, the two interleaved
//                              delta chains and the run ends as block scans whose state is carried from chunk to chunk in registers
//            rle_fill_kernel   one workgroup per 64 x 64 tile: a thread owns 16 rows of one column, finds its run by binary search and walks the
//                              runs down; the tile goes through LDS so that the row-major stores are 16 bytes wide
//   encode   rle_count_kernel  the same tiling read row-major (16-byte loads) into LDS: transitions per (column, 16-row segment), area and bounds
//            rle_scan_kernel   one workgroup per mask: exclusive scan of the segment counts in scan order (column-major)
//            rle_count_kernel<EMIT>  the segments again, each writing its transition positions behind its scanned offset
//            rle_string_kernel one workgroup per mask: counts = position differences, deltas, token lengths, their scan, the characters; run
//                              once for the lengths (which the host reads to size the strings exactly) and once to write
// No workgroup waits for another one: what crosses workgroups is a launch boundary.  Fill and count move the mask bytes once (HBM bound); parse,
// scan and string are single-workgroup loops per mask (latency bound, hidden by the batch).  Nothing here is for the matrix cores.
#include "common.h"
#include "../../include/gdrn_hip.h"

#include <limits.h>
#include <string.h>

namespace {

constexpr int TILE = 64;         // tile side of fill / count
constexpr int SEG = 16;          // rows of a column one thread walks
constexpr int LDW = TILE + 16;   // LDS row pitch: 64 bytes + one 16-byte access (rows stay 16-byte aligned, pitch not a power of two)
constexpr int NT = 1024;         // threads of the per-mask kernels
constexpr int MAX_GROUPS = 13;   // 5-bit groups of a token that can reach a 64-bit value (a legal 32-bit count has at most 7)

typedef unsigned long long u64;

struct Chains {   // odd / even delta chain contributions of a token (uint32 arithmetic: maskApi's counts are uint)
    unsigned odd, even;
};
__device__ __forceinline__ Chains operator+(Chains a, Chains b) { return Chains{a.odd + b.odd, a.even + b.even}; }

template <typename T>
__device__ __forceinline__ T shfl_up_words(T v, int o) {
    constexpr int NW = sizeof(T) / 4;
    unsigned w[NW];
    memcpy(w, &v, sizeof(T));
#pragma unroll
    for (int k = 0; k < NW; k++) w[k] = __shfl_up(w[k], o, 64);
    T r;
    memcpy(&r, w, sizeof(T));
    return r;
}

// inclusive scan over the NT threads of the workgroup; total = the sum over all of them.  red: NT / 64 elements of LDS.
template <typename T>
__device__ __forceinline__ T block_scan(T v, T* red, T& total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const T u = shfl_up_words(v, o);
        if (lane >= o) v = u + v;
    }
    __syncthreads();   // (red may still be read by the previous scan)
    if (lane == 63) red[wave] = v;
    __syncthreads();
    T pre = T(), tot = T();
    for (int w = 0; w < NT / 64; w++) {
        const T r = red[w];
        if (w < wave) pre = pre + r;
        tot = tot + r;
    }
    total = tot;
    return pre + v;
}

// ---- decode ------------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(NT) void rle_parse_kernel(const gdrn_rle_task* __restrict__ tasks, const unsigned char* __restrict__ strings,
                                                       int* __restrict__ run_ends, int* __restrict__ nruns, long long* __restrict__ totals) {
    __shared__ int red_n[NT / 64];
    __shared__ Chains red_c[NT / 64];
    __shared__ u64 red_e[NT / 64];
    const int n = blockIdx.x;
    const gdrn_rle_task t = tasks[n];
    const unsigned char* __restrict__ s = strings + t.str_off;
    const u64 hw = (u64)t.h * (u64)t.w;
    int* __restrict__ ends = run_ends + t.run_off;
    int ntok = 0;              // tokens before this chunk
    Chains chain = {0u, 0u};   // counts[last odd index], counts[last even index >= 2] before this chunk
    u64 end = 0;               // end of the last run before this chunk
    for (int base = 0; base < t.str_len; base += NT) {
        const int i = base + (int)threadIdx.x;
        bool is_end = false;
        unsigned val = 0;
        if (i < t.str_len) {
            const int c = (int)s[i] - 48;
            is_end = (c & 0x20) == 0;
            if (is_end) {   // the token's groups are s[i - k .. i], least significant first (read back through the cache: no carry needed)
                int k = 0;
                while (k < MAX_GROUPS - 1 && i - k - 1 >= 0 && (((int)s[i - k - 1] - 48) & 0x20)) k++;
                long long x = 0;
                for (int g = 0; g <= k; g++) x |= (long long)(((int)s[i - k + g] - 48) & 0x1f) << (5 * g);
                if ((c & 0x10) && 5 * (k + 1) < 64) x |= -(1LL << (5 * (k + 1)));
                val = (unsigned)x;
            }
        }
        int tot_n;
        const int tix = ntok + block_scan<int>(is_end ? 1 : 0, red_n, tot_n) - 1;   // this token's index
        Chains mine = {0u, 0u};
        if (is_end && tix >= 1) {
            if (tix & 1) mine.odd = val;
            else mine.even = val;
        }
        Chains tot_c;
        const Chains inc = block_scan<Chains>(mine, red_c, tot_c);
        unsigned cnt = 0;
        if (is_end) cnt = tix == 0 ? val : (tix & 1) ? chain.odd + inc.odd : chain.even + inc.even;
        u64 tot_e;
        const u64 e = end + block_scan<u64>((u64)cnt, red_e, tot_e);
        if (is_end) ends[tix] = (int)(e < hw ? e : hw);   // tix < str_len: a token has at least one character
        ntok += tot_n;
        chain = chain + tot_c;
        end += tot_e;
    }
    if (threadIdx.x == 0) {
        nruns[n] = ntok;
        totals[n] = (long long)end;
    }
}

__global__ __launch_bounds__(256) void rle_fill_kernel(const gdrn_rle_task* __restrict__ tasks, const int* __restrict__ run_ends,
                                                       const int* __restrict__ nruns) {
    __shared__ __attribute__((aligned(16))) unsigned char tile[TILE * LDW];
    const int n = blockIdx.z;
    const gdrn_rle_task t = tasks[n];
    const int x0 = blockIdx.x * TILE, y0 = blockIdx.y * TILE;
    if (x0 >= t.w || y0 >= t.h) return;   // the grid is sized by the largest mask of the batch (uniform exit)
    const int* __restrict__ ends = run_ends + t.run_off;
    const int nr = nruns[n];
    const int col = threadIdx.x & 63, sg = threadIdx.x >> 6;
    const int x = x0 + col, ys = y0 + sg * SEG;
    if (x < t.w && ys < t.h) {
        int p = x * t.h + ys;   // scan-order index of the first pixel (h w < 2^31)
        int lo = 0, hi = nr;    // first run whose end lies behind p; nr: past the last run, zeros
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (ends[mid] > p) hi = mid;
            else lo = mid + 1;
        }
        int k = lo, e = k < nr ? ends[k] : INT_MAX;
        const int rows = min(SEG, t.h - ys);
        for (int r = 0; r < rows; r++, p++) {
            while (p >= e) {   // (zero-length runs are stepped over here)
                ++k;
                e = k < nr ? ends[k] : INT_MAX;
            }
            tile[(sg * SEG + r) * LDW + col] = (unsigned char)(k < nr ? (k & 1) : 0);
        }
    }
    __syncthreads();
    const int r = threadIdx.x >> 2, xs = x0 + (threadIdx.x & 3) * 16, y = y0 + r;
    if (y < t.h && xs < t.w) {
        unsigned char* dst = t.mask + (size_t)y * t.w + xs;
        const unsigned char* src = tile + r * LDW + (threadIdx.x & 3) * 16;
        if (xs + 16 <= t.w && (reinterpret_cast<uintptr_t>(dst) & 15) == 0) {
            *reinterpret_cast<uint4*>(dst) = *reinterpret_cast<const uint4*>(src);
        } else {
            const int cnt = min(16, t.w - xs);
            for (int j = 0; j < cnt; j++) dst[j] = src[j];
        }
    }
}

// ---- encode ------------------------------------------------------------------------------------------------------------------------------------
__global__ void rle_stats_init_kernel(int* __restrict__ area, int* __restrict__ bbox, int N) {
    const int n = blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= N) return;
    area[n] = 0;
    bbox[n * 4 + 0] = INT_MAX;
    bbox[n * 4 + 1] = INT_MAX;
    bbox[n * 4 + 2] = -1;
    bbox[n * 4 + 3] = -1;
}

__global__ void rle_stats_final_kernel(const gdrn_rle_task* __restrict__ tasks, const int* __restrict__ area, int* __restrict__ bbox, int N) {
    const int n = blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= N || area[n] != 0) return;
    bbox[n * 4 + 0] = 0;   // an empty mask: the whole frame, as gdrn_xyz_from_depth writes it
    bbox[n * 4 + 1] = 0;
    bbox[n * 4 + 2] = tasks[n].w - 1;
    bbox[n * 4 + 3] = tasks[n].h - 1;
}

__device__ __forceinline__ unsigned nonzero_bytes(unsigned w) {   // every non-zero byte -> 1
    return ((w | ((w & 0x7f7f7f7fu) + 0x7f7f7f7fu)) >> 7) & 0x01010101u;
}

// EMIT = false: seg[segment] = its transition count (seg may be NULL), area / bbox atomics (area may be NULL).
// EMIT = true:  seg holds the scanned offsets; the segment's transition positions go to positions[run_off + offset ...].
template <bool EMIT>
__global__ __launch_bounds__(256) void rle_count_kernel(const gdrn_rle_task* __restrict__ tasks, int* __restrict__ seg, int* __restrict__ area,
                                                        int* __restrict__ bbox, int* __restrict__ positions) {
    __shared__ __attribute__((aligned(16))) unsigned char tile[(TILE + 1) * LDW];   // row 0: the predecessors of the tile's first row
    __shared__ int box[5];
    const int n = blockIdx.z;
    const gdrn_rle_task t = tasks[n];
    const int x0 = blockIdx.x * TILE, y0 = blockIdx.y * TILE;
    if (x0 >= t.w || y0 >= t.h) return;
    const unsigned char* __restrict__ m = t.mask;
    if (!EMIT && threadIdx.x == 0) { box[0] = 0; box[1] = INT_MAX; box[2] = INT_MAX; box[3] = -1; box[4] = -1; }
    for (int i = threadIdx.x; i < (TILE + 1) * 4; i += 256) {
        const int r = i >> 2, xs = x0 + (i & 3) * 16, y = y0 + r - 1;
        unsigned char* dst = tile + r * LDW + (i & 3) * 16;
        if (xs >= t.w || y >= t.h) continue;
        const int cnt = min(16, t.w - xs);
        if (y < 0) {   // above row 0: the last pixel of the previous column; pixel (0, 0) follows a 0
            for (int j = 0; j < cnt; j++) {
                const int x = xs + j;
                dst[j] = (x > 0 && m[(long long)(t.h - 1) * t.sy + (long long)(x - 1) * t.sx] != 0) ? 1 : 0;
            }
            continue;
        }
        const unsigned char* src = m + (long long)y * t.sy + (long long)xs * t.sx;
        if (t.sx == 1 && cnt == 16 && (reinterpret_cast<uintptr_t>(src) & 15) == 0) {
            const uint4 v = *reinterpret_cast<const uint4*>(src);
            *reinterpret_cast<uint4*>(dst) = make_uint4(nonzero_bytes(v.x), nonzero_bytes(v.y), nonzero_bytes(v.z), nonzero_bytes(v.w));
        } else {
            for (int j = 0; j < cnt; j++) dst[j] = src[(long long)j * t.sx] != 0 ? 1 : 0;
        }
    }
    __syncthreads();
    const int col = threadIdx.x & 63, sg = threadIdx.x >> 6;
    const int x = x0 + col, ys = y0 + sg * SEG;
    if (x < t.w && ys < t.h) {
        const int nsy = (t.h + SEG - 1) / SEG;
        const long long sidx = t.seg_off + (long long)x * nsy + ys / SEG;
        const int rows = min(SEG, t.h - ys);
        const long long cap = (long long)t.h * t.w;   // positions of a mask: at most h w transitions (+ 1 slot)
        int off = 0;
        if (EMIT) off = seg[sidx];
        int prev = tile[(sg * SEG) * LDW + col];
        int trans = 0, ones = 0, ymin = INT_MAX, ymax = -1;
        for (int r = 0; r < rows; r++) {
            const int cur = tile[(sg * SEG + r + 1) * LDW + col];
            if (cur != prev) {
                if (EMIT) {
                    const long long o = (long long)off + trans;
                    if (o >= 0 && o <= cap) positions[t.run_off + o] = x * t.h + ys + r;   // (guard: the mask changed between the two passes)
                }
                ++trans;
            }
            if (!EMIT && cur) {
                ++ones;
                ymin = min(ymin, ys + r);
                ymax = ys + r;
            }
            prev = cur;
        }
        if (!EMIT) {
            if (seg) seg[sidx] = trans;
            if (area && ones) {
                atomicAdd(&box[0], ones);
                atomicMin(&box[1], x);
                atomicMin(&box[2], ymin);
                atomicMax(&box[3], x);
                atomicMax(&box[4], ymax);
            }
        }
    }
    if (EMIT || !area) return;
    __syncthreads();
    if (threadIdx.x == 0 && box[0] > 0) {
        atomicAdd(&area[n], box[0]);
        atomicMin(&bbox[n * 4 + 0], box[1]);
        atomicMin(&bbox[n * 4 + 1], box[2]);
        atomicMax(&bbox[n * 4 + 2], box[3]);
        atomicMax(&bbox[n * 4 + 3], box[4]);
    }
}

__global__ __launch_bounds__(NT) void rle_scan_kernel(const gdrn_rle_task* __restrict__ tasks, int* __restrict__ seg, int* __restrict__ ntrans) {
    __shared__ int red[NT / 64];
    const int n = blockIdx.x;
    const gdrn_rle_task t = tasks[n];
    const long long nseg = (long long)t.w * ((t.h + SEG - 1) / SEG);
    int* __restrict__ s = seg + t.seg_off;
    int carry = 0;
    for (long long base = 0; base < nseg; base += NT) {
        const long long i = base + threadIdx.x;
        const int v = i < nseg ? s[i] : 0;
        int tot;
        const int inc = block_scan<int>(v, red, tot);
        if (i < nseg) s[i] = carry + inc - v;
        carry += tot;
    }
    if (threadIdx.x == 0) ntrans[n] = carry;
}

template <bool WRITE>
__global__ __launch_bounds__(NT) void rle_string_kernel(const gdrn_rle_task* __restrict__ tasks, const int* __restrict__ ntrans,
                                                        const int* __restrict__ positions, const long long* __restrict__ str_offsets,
                                                        unsigned char* __restrict__ strings, long long strings_bytes,
                                                        long long* __restrict__ lengths) {
    __shared__ u64 red[NT / 64];
    const int n = blockIdx.x;
    const gdrn_rle_task t = tasks[n];
    const long long hw = (long long)t.h * t.w;
    const int* __restrict__ pos = positions + t.run_off;
    long long T = ntrans[n];
    T = T < 0 ? 0 : T > hw ? hw : T;
    auto P = [&](long long j) -> long long { return j < 0 ? 0 : j >= T ? hw : (long long)pos[j]; };   // P(-1) = 0, P(T) = h w
    long long room = 0;
    unsigned char* dst = nullptr;
    if (WRITE) {
        const long long o0 = str_offsets[n], o1 = str_offsets[n + 1];
        if (o0 >= 0 && o1 >= o0 && o1 <= strings_bytes) {   // (room stays 0 otherwise: nothing is written)
            room = o1 - o0;
            dst = strings + o0;
        }
    }
    u64 carry = 0;
    for (long long base = 0; base <= T; base += NT) {   // T + 1 counts
        const long long i = base + threadIdx.x;
        int len = 0;
        int x = 0;
        if (i <= T) {
            const long long c = P(i) - P(i - 1);
            x = (int)(i > 2 ? c - (P(i - 2) - P(i - 3)) : c);   // counts < 2^31: the difference fits
            int v = x;
            bool more = true;
            while (more) {   // rleToString: 1 .. 7 groups for an int32
                const int g = v & 0x1f;
                v >>= 5;     // arithmetic
                more = (g & 0x10) ? v != -1 : v != 0;
                ++len;
            }
        }
        u64 tot;
        const u64 inc = block_scan<u64>((u64)len, red, tot);
        if (WRITE && len > 0) {
            const long long off = (long long)(carry + inc) - len;
            if (off + len <= room) {
                int v = x;
                for (int k = 0; k < len; k++) {
                    int g = v & 0x1f;
                    v >>= 5;
                    if (k + 1 < len) g |= 0x20;
                    dst[off + k] = (unsigned char)(g + 48);
                }
            }
        }
        carry += tot;
    }
    if (!WRITE && threadIdx.x == 0) lengths[n] = (long long)carry;
}

// the argument checks on the host copy of the table; decode: the string / run-end ranges and a contiguous mask, else the segment / position ranges
int check_tasks(const gdrn_rle_task* th, int N, bool decode, long long strings_bytes, long long run_cap, long long seg_cap, int* max_h, int* max_w) {
    int status = GDRN_OK;
    *max_h = *max_w = 0;
    for (int i = 0; i < N; i++) {
        const gdrn_rle_task& t = th[i];
        if (!t.mask || t.h <= 0 || t.w <= 0) return GDRN_ERR_ARG;
        const long long hw = (long long)t.h * t.w;
        if (hw >= (1LL << 31)) {
            status = GDRN_ERR_SHAPE;
            continue;
        }
        *max_h = t.h > *max_h ? t.h : *max_h;
        *max_w = t.w > *max_w ? t.w : *max_w;
        if (decode) {
            if (t.sx != 1 || t.sy != t.w) return GDRN_ERR_ARG;
            if (t.str_len < 0 || t.str_off < 0 || t.str_off + t.str_len > strings_bytes) return GDRN_ERR_ARG;
            if (t.run_off < 0 || t.run_off + t.str_len > run_cap) return GDRN_ERR_ARG;
        } else {
            const long long nseg = (long long)t.w * ((t.h + SEG - 1) / SEG);
            if (seg_cap >= 0 && (t.seg_off < 0 || t.seg_off + nseg > seg_cap)) return GDRN_ERR_ARG;
            if (run_cap >= 0 && (t.run_off < 0 || t.run_off + hw + 1 > run_cap)) return GDRN_ERR_ARG;
        }
    }
    return status;
}

}  // namespace

extern "C" int gdrn_rle_decode(const gdrn_rle_task* tasks_dev, const gdrn_rle_task* tasks_host, int N, const unsigned char* strings,
                               long long strings_bytes, int* run_ends, long long run_cap, int* nruns, long long* totals, void* stream) {
    if (!tasks_dev || !tasks_host || N <= 0 || !strings || strings_bytes < 0 || !run_ends || run_cap < 0 || !nruns || !totals) return GDRN_ERR_ARG;
    if (N > 65535) return GDRN_ERR_SHAPE;
    int mh, mw;
    const int st = check_tasks(tasks_host, N, true, strings_bytes, run_cap, -1, &mh, &mw);
    if (st != GDRN_OK) return st;
    if (cdiv(mh, TILE) > 65535) return GDRN_ERR_SHAPE;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    GDRN_LAUNCH(rle_parse_kernel, dim3(N), dim3(NT), 0, s, tasks_dev, strings, run_ends, nruns, totals);
    GDRN_CHECK_LAUNCH();
    GDRN_LAUNCH(rle_fill_kernel, dim3(cdiv(mw, TILE), cdiv(mh, TILE), N), dim3(256), 0, s, tasks_dev, run_ends, nruns);
    GDRN_CHECK_LAUNCH();
    return GDRN_OK;
}

extern "C" int gdrn_rle_count(const gdrn_rle_task* tasks_dev, const gdrn_rle_task* tasks_host, int N, int* seg_counts, long long seg_cap, int* area,
                              int* bbox, void* stream) {
    if (!tasks_dev || !tasks_host || N <= 0 || (!seg_counts && !area) || (seg_counts && seg_cap < 0) || (!area != !bbox)) return GDRN_ERR_ARG;
    if (N > 65535) return GDRN_ERR_SHAPE;
    int mh, mw;
    const int st = check_tasks(tasks_host, N, false, 0, -1, seg_counts ? seg_cap : -1, &mh, &mw);
    if (st != GDRN_OK) return st;
    if (cdiv(mh, TILE) > 65535) return GDRN_ERR_SHAPE;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (area) {
        GDRN_LAUNCH(rle_stats_init_kernel, dim3(cdiv(N, 256)), dim3(256), 0, s, area, bbox, N);
        GDRN_CHECK_LAUNCH();
    }
    GDRN_LAUNCH(rle_count_kernel<false>, dim3(cdiv(mw, TILE), cdiv(mh, TILE), N), dim3(256), 0, s, tasks_dev, seg_counts, area, bbox,
                static_cast<int*>(nullptr));
    GDRN_CHECK_LAUNCH();
    if (area) {
        GDRN_LAUNCH(rle_stats_final_kernel, dim3(cdiv(N, 256)), dim3(256), 0, s, tasks_dev, static_cast<const int*>(area), bbox, N);
        GDRN_CHECK_LAUNCH();
    }
    return GDRN_OK;
}

extern "C" int gdrn_rle_positions(const gdrn_rle_task* tasks_dev, const gdrn_rle_task* tasks_host, int N, int* seg_counts, long long seg_cap,
                                  int* ntrans, int* positions, long long pos_cap, void* stream) {
    if (!tasks_dev || !tasks_host || N <= 0 || !seg_counts || seg_cap < 0 || !ntrans || !positions || pos_cap < 0) return GDRN_ERR_ARG;
    if (N > 65535) return GDRN_ERR_SHAPE;
    int mh, mw;
    const int st = check_tasks(tasks_host, N, false, 0, pos_cap, seg_cap, &mh, &mw);
    if (st != GDRN_OK) return st;
    if (cdiv(mh, TILE) > 65535) return GDRN_ERR_SHAPE;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    GDRN_LAUNCH(rle_scan_kernel, dim3(N), dim3(NT), 0, s, tasks_dev, seg_counts, ntrans);
    GDRN_CHECK_LAUNCH();
    GDRN_LAUNCH(rle_count_kernel<true>, dim3(cdiv(mw, TILE), cdiv(mh, TILE), N), dim3(256), 0, s, tasks_dev, seg_counts, static_cast<int*>(nullptr),
                static_cast<int*>(nullptr), positions);
    GDRN_CHECK_LAUNCH();
    return GDRN_OK;
}

extern "C" int gdrn_rle_string(const gdrn_rle_task* tasks_dev, const gdrn_rle_task* tasks_host, int N, const int* ntrans, const int* positions,
                               long long pos_cap, const long long* str_offsets, unsigned char* strings, long long strings_bytes,
                               long long* lengths, void* stream) {
    if (!tasks_dev || !tasks_host || N <= 0 || !ntrans || !positions || pos_cap < 0) return GDRN_ERR_ARG;
    if ((str_offsets != nullptr) != (strings != nullptr) || (str_offsets == nullptr) == (lengths == nullptr) || strings_bytes < 0) return GDRN_ERR_ARG;
    if (N > 65535) return GDRN_ERR_SHAPE;
    int mh, mw;
    const int st = check_tasks(tasks_host, N, false, 0, pos_cap, -1, &mh, &mw);
    if (st != GDRN_OK) return st;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (str_offsets) {
        GDRN_LAUNCH(rle_string_kernel<true>, dim3(N), dim3(NT), 0, s, tasks_dev, ntrans, positions, str_offsets, strings, strings_bytes,
                    static_cast<long long*>(nullptr));
    } else {
        GDRN_LAUNCH(rle_string_kernel<false>, dim3(N), dim3(NT), 0, s, tasks_dev, ntrans, positions, static_cast<const long long*>(nullptr),
                    static_cast<unsigned char*>(nullptr), 0LL, lengths);
    }
    GDRN_CHECK_LAUNCH();
    return GDRN_OK;
}
