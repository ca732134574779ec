// Model preparation for gfx950: the per-object tables every data-side and evaluation-side module takes as constructor arguments, computed for all
// C objects of a dataset per call from their packed vertices (pts [C][n_max][3] fp64, npts [C]) -- what the reference gets from offline passes:
//   bounds    per-axis minimum, maximum (exact) and mean (fp64, fixed order) of the vertices: the extents of data_loader.py:243-276 and
//             misc.get_bbox3d_and_center (lib/pysixd/misc.py:982-1030)
//   fps       the index sequence of sample_farthest_points_init_center (core/csrc/fps/src/farthest_point_sampling.cpp:122-160), bit for bit:
//             vertices rounded to fp32, start = the point farthest from (max + min) * 0.5f of the fp32 box, squared distance (dx dx + dy dy) + dz dz
//             in fp32, running minimum per point, strict arg-max with the lowest index among equal maxima and index 0 when nothing is above 0
//   diameter  the maximum over all vertex pairs of (dx dx + dy dy) + dz dz in fp64: misc.calc_pts_diameter (misc.py:952-966) before its sqrt
// Floating-point contraction is OFF for this file: both distances are the reference's operation sequences, multiplications and additions
// rounded one by one.  (No 16-bit code: both library builds compile the same thing.)
//
// fps_kernel: one workgroup of 1024 threads per object, all K iterations in one launch.  An iteration is "update the running minima against the
// last pick, arg-max": every thread folds its points into one 64-bit key (distance bits << 32 | ~index -- non-negative floats order like their
// bits, so the largest key is the largest distance and among equals the lowest index; a distance that is not above 0 enters as 0, so with nothing
// above 0 the largest key is point 0's), a wave reduction over the 64 lanes, the 16 wave winners with their coordinates through LDS (double
// buffered: one barrier per iteration; a slot is rewritten two barriers after its last read).  Objects of up to FPS_REG_MAX points keep points and minima in registers; larger ones keep them as
// float4 (x, y, z, minimum) in the caller's workspace, each element read and written by the same thread in every iteration.  No workgroup
// waits for another one; every loop is bounded by K or by the point count.  Latency bound by design: one workgroup per object.
// diameter_kernel: the pair matrix in tiles of 512 x 512, every unordered tile pair once (tile a with tiles a, a + 1, .., a + nt / 2 cyclically);
// the j tile is staged in LDS as fp64, a thread holds two i points in registers; block maximum, then one atomicMax on the bit pattern
// (non-negative doubles order like unsigned 64-bit integers).  fp64 VALU bound.
#include "common.h"
#include "geom64.h"
#include "../../include/gdrn_hip.h"

#include <float.h>

#pragma clang fp contract(off)

namespace {

typedef unsigned long long u64;

constexpr int FPS_NT = 1024;                   // threads of the workgroup of an object
constexpr int FPS_WAVES = FPS_NT / 64;
static_assert(FPS_WAVES == 16, "fps_block_best reduces the wave winners over 16 lanes");
constexpr int FPS_R = 16;                      // points a thread keeps in registers
constexpr int FPS_REG_MAX = FPS_NT * FPS_R;    // the largest object of the register path
constexpr int BD_NT = 1024;                    // threads of bounds_kernel
constexpr int DM_NT = 256;                     // threads of diameter_kernel
constexpr int DM_G = 2;                        // i points of a thread
constexpr int DM_TILE = DM_NT * DM_G;          // tile side

__device__ __forceinline__ u64 shfl_xor_u64(u64 v, int o) {
    const unsigned lo = __shfl_xor((unsigned)v, o, 64), hi = __shfl_xor((unsigned)(v >> 32), o, 64);
    return ((u64)hi << 32) | lo;
}

// ---- bounds ------------------------------------------------------------------------------------------------------------------------------------
// out [C][9] = min xyz, max xyz, mean xyz.  The sums: thread t adds its points t, t + 1024, .. in ascending order, the 64 lanes of a wave by the
// xor tree, the 16 waves in ascending order.
__global__ __launch_bounds__(BD_NT) void bounds_kernel(const double* __restrict__ pts, const int* __restrict__ npts, int n_max,
                                                       double* __restrict__ out) {
    __shared__ double red[9][BD_NT / 64];
    const int c = blockIdx.x;
    const int n = min(max(npts[c], 1), n_max);
    const double* __restrict__ p = pts + (size_t)c * n_max * 3;
    double v[9];   // min, max, sum
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        v[a] = p[a];   // point 0: every object has one
        v[3 + a] = p[a];
        v[6 + a] = 0.0;
    }
    for (int i = threadIdx.x; i < n; i += BD_NT) {
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const double x = p[(size_t)i * 3 + a];
            v[a] = x < v[a] ? x : v[a];
            v[3 + a] = x > v[3 + a] ? x : v[3 + a];
            v[6 + a] += x;
        }
    }
#pragma unroll
    for (int a = 0; a < 3; ++a) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const double lo = __shfl_xor(v[a], o, 64), hi = __shfl_xor(v[3 + a], o, 64);
            v[a] = lo < v[a] ? lo : v[a];
            v[3 + a] = hi > v[3 + a] ? hi : v[3 + a];
        }
        v[6 + a] = wave_sum_f64(v[6 + a]);
    }
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int k = 0; k < 9; ++k) red[k][threadIdx.x >> 6] = v[k];
    }
    __syncthreads();
    if (threadIdx.x < 9) {
        const int k = threadIdx.x;
        double r = red[k][0];
        for (int w = 1; w < BD_NT / 64; ++w) {
            const double x = red[k][w];
            r = k < 3 ? (x < r ? x : r) : k < 6 ? (x > r ? x : r) : r + x;
        }
        out[(size_t)c * 9 + k] = k < 6 ? r : r / (double)n;
    }
}

// ---- farthest-point sampling ---------------------------------------------------------------------------------------------------------------------
// the running minimum of a point against the last pick q, and the point folded into the thread's best key
__device__ __forceinline__ void fps_point(float px, float py, float pz, float& md, int i, float qx, float qy, float qz, u64& best) {
    const float dx = px - qx, dy = py - qy, dz = pz - qz;
    const float d = (dx * dx + dy * dy) + dz * dz;
    if (d < md) md = d;
    const u64 key = ((u64)(md > 0.f ? __float_as_uint(md) : 0u) << 32) | (u64)(0xffffffffu - (unsigned)i);
    best = key > best ? key : best;
}

__device__ __forceinline__ unsigned fps_index(u64 key) { return 0xffffffffu - (unsigned)key; }

struct FpsSlot {   // a wave's winner
    u64 key;
    float x, y, z, pad_;
};

__device__ __forceinline__ u64 fps_wave_max(u64 v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const u64 other = shfl_xor_u64(v, o);
        v = other > v ? other : v;
    }
    return v;
}

// the workgroup's winner from the FPS_WAVES slots, behind the barrier that follows their writes: one slot per lane of a DPP row, four xor steps
// (every row does the same)
__device__ __forceinline__ FpsSlot fps_block_best(const FpsSlot* slots) {
    int w = threadIdx.x & 15;
    u64 k = slots[w].key;
#pragma unroll
    for (int o = 8; o > 0; o >>= 1) {
        const u64 ok = shfl_xor_u64(k, o);
        const int ow = __shfl_xor(w, o, 64);
        if (ok > k || (ok == k && ow < w)) {
            k = ok;
            w = ow;
        }
    }
    return slots[w];
}

__global__ __launch_bounds__(FPS_NT) void fps_kernel(const double* __restrict__ pts, const int* __restrict__ npts, int n_max, int K,
                                                     float4* __restrict__ ws, int* __restrict__ idx, double* __restrict__ xyz) {
    __shared__ FpsSlot slots[2][FPS_WAVES];
    __shared__ float box[6][FPS_WAVES];
    const int c = blockIdx.x, tid = threadIdx.x;
    int n = min(max(npts[c], 1), n_max);
    if (!ws) n = min(n, FPS_REG_MAX);   // (the host wrapper refuses a larger object without a workspace)
    const double* __restrict__ p = pts + (size_t)c * n_max * 3;
    const bool in_regs = n <= FPS_REG_MAX;   // (the same for the whole workgroup)
    float4* __restrict__ w = ws + (size_t)c * n_max;
    float px[FPS_R], py[FPS_R], pz[FPS_R], md[FPS_R];
    // the points as fp32 (round to nearest even) and their box
    float lo[3], hi[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) lo[a] = hi[a] = (float)p[a];
    auto widen = [&](float x, float y, float z) {
        lo[0] = fminf(lo[0], x); lo[1] = fminf(lo[1], y); lo[2] = fminf(lo[2], z);
        hi[0] = fmaxf(hi[0], x); hi[1] = fmaxf(hi[1], y); hi[2] = fmaxf(hi[2], z);
    };
    if (in_regs) {
#pragma unroll
        for (int r = 0; r < FPS_R; ++r) {
            const int i = r * FPS_NT + tid;
            px[r] = py[r] = pz[r] = 0.f;
            md[r] = FLT_MAX;
            if (i < n) {
                px[r] = (float)p[(size_t)i * 3 + 0];
                py[r] = (float)p[(size_t)i * 3 + 1];
                pz[r] = (float)p[(size_t)i * 3 + 2];
                widen(px[r], py[r], pz[r]);
            }
        }
    } else {
        for (int i = tid; i < n; i += FPS_NT) {
            const float x = (float)p[(size_t)i * 3 + 0], y = (float)p[(size_t)i * 3 + 1], z = (float)p[(size_t)i * 3 + 2];
            widen(x, y, z);
            w[i] = make_float4(x, y, z, FLT_MAX);
        }
    }
#pragma unroll
    for (int a = 0; a < 3; ++a) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            lo[a] = fminf(lo[a], __shfl_xor(lo[a], o, 64));
            hi[a] = fmaxf(hi[a], __shfl_xor(hi[a], o, 64));
        }
    }
    if ((tid & 63) == 0) {
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            box[a][tid >> 6] = lo[a];
            box[3 + a][tid >> 6] = hi[a];
        }
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < FPS_WAVES; ++j) {
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            lo[a] = fminf(lo[a], box[a][j]);
            hi[a] = fmaxf(hi[a], box[3 + a][j]);
        }
    }
    // the first "pick" is the box centre: minima start at FLT_MAX, so the first update leaves the distances to it
    float qx = (hi[0] + lo[0]) * 0.5f, qy = (hi[1] + lo[1]) * 0.5f, qz = (hi[2] + lo[2]) * 0.5f;
    for (int k = 0; k < K; ++k) {
        u64 mine = 0;
        if (in_regs) {
#pragma unroll
            for (int r = 0; r < FPS_R; ++r) {
                if (r * FPS_NT < n) {   // (uniform)
                    const int i = r * FPS_NT + tid;
                    if (i < n) fps_point(px[r], py[r], pz[r], md[r], i, qx, qy, qz, mine);
                }
            }
        } else {
            for (int i = tid; i < n; i += FPS_NT) {
                const float4 v = w[i];
                float m = v.w;
                fps_point(v.x, v.y, v.z, m, i, qx, qy, qz, mine);
                if (m != v.w) w[i].w = m;
            }
        }
        // the wave's winner with its coordinates into the wave's slot: its index is the same in every lane, so which register holds the point
        // is a uniform choice; the lane that owns the point writes (a wave without points: lane 0, key 0)
        const u64 wmax = fps_wave_max(mine);
        const unsigned wi = __builtin_amdgcn_readfirstlane(fps_index(wmax));
        FpsSlot* slot = &slots[k & 1][tid >> 6];
        if (wmax == 0) {
            if ((tid & 63) == 0) *slot = FpsSlot{0ull, 0.f, 0.f, 0.f, 0.f};
        } else if (in_regs) {
            float x = 0.f, y = 0.f, z = 0.f;
#pragma unroll
            for (int r = 0; r < FPS_R; ++r) {
                if ((int)(wi / FPS_NT) == r) {   // (uniform)
                    x = px[r];
                    y = py[r];
                    z = pz[r];
                }
            }
            if ((int)(wi % FPS_NT) == tid) *slot = FpsSlot{wmax, x, y, z, 0.f};
        } else if ((int)(wi % FPS_NT) == tid) {
            const float4 v = w[wi];   // (this lane's own element)
            *slot = FpsSlot{wmax, v.x, v.y, v.z, 0.f};
        }
        __syncthreads();
        const FpsSlot b = fps_block_best(slots[k & 1]);
        qx = b.x;
        qy = b.y;
        qz = b.z;
        if (tid == 0) {
            idx[(size_t)c * K + k] = (int)fps_index(b.key);
            if (xyz) {
                double* o = xyz + ((size_t)c * K + k) * 3;
                o[0] = (double)qx;
                o[1] = (double)qy;
                o[2] = (double)qz;
            }
        }
    }
}

// ---- diameter ----------------------------------------------------------------------------------------------------------------------------------
__global__ void diameter_init_kernel(u64* __restrict__ max_sq, int C) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c < C) max_sq[c] = 0ull;
}

// tiles per side and tile pairs of an object of n points: tile a meets the tiles a + d (mod nt), d = 0 .. nt / 2
__host__ __device__ __forceinline__ long long dm_tiles(int n) { return ((long long)n + DM_TILE - 1) / DM_TILE; }
__host__ __device__ __forceinline__ long long dm_pairs(int n) {
    const long long nt = dm_tiles(n);
    return nt * (nt / 2 + 1);
}

__global__ __launch_bounds__(DM_NT) void diameter_kernel(const double* __restrict__ pts, const int* __restrict__ npts, int n_max, int C,
                                                         u64* __restrict__ max_sq) {
    __shared__ double tx[DM_TILE], ty[DM_TILE], tz[DM_TILE];
    __shared__ double red[DM_NT / 64];
    // which object this workgroup belongs to: the prefix of the tile-pair counts, walked (C steps at most)
    long long t = blockIdx.x;
    int c = 0, n = 1;
    for (; c < C; ++c) {
        n = min(max(npts[c], 1), n_max);
        const long long cnt = dm_pairs(n);
        if (t < cnt) break;
        t -= cnt;
    }
    if (c >= C) return;
    const long long nt = dm_tiles(n), wdt = nt / 2 + 1;
    const long long a = t / wdt, d = t % wdt;
    if ((nt & 1) == 0 && d == nt / 2 && a >= nt / 2) return;   // an even count: the opposite tile pair is met from its lower tile
    const long long b = (a + d) % nt;
    const double* __restrict__ p = pts + (size_t)c * n_max * 3;
    // rows beyond the object's last point repeat that point: a pair of the object either way, and the padding of the table is never read
    for (int j = threadIdx.x; j < DM_TILE; j += DM_NT) {
        const long long src = min(b * DM_TILE + j, (long long)n - 1);
        tx[j] = p[src * 3 + 0];
        ty[j] = p[src * 3 + 1];
        tz[j] = p[src * 3 + 2];
    }
    double ix[DM_G], iy[DM_G], iz[DM_G], m[DM_G];
#pragma unroll
    for (int g = 0; g < DM_G; ++g) {
        const long long src = min(a * DM_TILE + g * DM_NT + threadIdx.x, (long long)n - 1);
        ix[g] = p[src * 3 + 0];
        iy[g] = p[src * 3 + 1];
        iz[g] = p[src * 3 + 2];
        m[g] = 0.0;
    }
    __syncthreads();
    const int nj = (int)min((long long)DM_TILE, (long long)n - b * DM_TILE);   // >= 1
    for (int j = 0; j < nj; ++j) {
        const double x = tx[j], y = ty[j], z = tz[j];
#pragma unroll
        for (int g = 0; g < DM_G; ++g) {
            const double dx = ix[g] - x, dy = iy[g] - y, dz = iz[g] - z;
            const double s = (dx * dx + dy * dy) + dz * dz;
            m[g] = s > m[g] ? s : m[g];
        }
    }
    double v = m[0];
#pragma unroll
    for (int g = 1; g < DM_G; ++g) v = m[g] > v ? m[g] : v;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const double u = __shfl_xor(v, o, 64);
        v = u > v ? u : v;
    }
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int k = 1; k < DM_NT / 64; ++k) v = red[k] > v ? red[k] : v;
        atomicMax(&max_sq[c], (u64)__double_as_longlong(v));
    }
}

// what every entry point checks before its first launch
int check_models(const void* pts, const int* npts, const int* npts_host, int C, int n_max) {
    if (!pts || !npts || !npts_host || C < 1 || n_max < 1) return GDRN_ERR_ARG;
    for (int c = 0; c < C; ++c)
        if (npts_host[c] < 1 || npts_host[c] > n_max) return GDRN_ERR_ARG;
    if ((long long)n_max * 3 >= (1LL << 31) || C > 65535) return GDRN_ERR_SHAPE;
    return GDRN_OK;
}

}  // namespace

extern "C" long long gdrn_model_prep_workspace_bytes(int C, int n_max, int K) {
    if (C < 1 || n_max < 1 || K < 1 || (long long)n_max * 3 >= (1LL << 31) || C > 65535) return -1;
    return n_max > FPS_REG_MAX ? (long long)C * n_max * (long long)sizeof(float4) : 0;
}

extern "C" int gdrn_model_bounds(const double* pts, const int* npts, const int* npts_host, int C, int n_max, double* bounds, void* stream) {
    const int st = check_models(pts, npts, npts_host, C, n_max);
    if (st != GDRN_OK) return st;
    if (!bounds) return GDRN_ERR_ARG;
    GDRN_LAUNCH(bounds_kernel, dim3(C), dim3(BD_NT), 0, reinterpret_cast<hipStream_t>(stream), pts, npts, n_max, bounds);
    GDRN_CHECK_LAUNCH();
    return GDRN_OK;
}

extern "C" int gdrn_model_fps(const double* pts, const int* npts, const int* npts_host, int C, int n_max, int K, int* idx, double* xyz,
                              void* workspace, void* stream) {
    const int st = check_models(pts, npts, npts_host, C, n_max);
    if (st != GDRN_OK) return st;
    if (K < 1 || !idx) return GDRN_ERR_ARG;
    bool large = false;
    for (int c = 0; c < C; ++c) large = large || npts_host[c] > FPS_REG_MAX;
    if (large && (!workspace || (reinterpret_cast<uintptr_t>(workspace) & 15))) return GDRN_ERR_ARG;
    GDRN_LAUNCH(fps_kernel, dim3(C), dim3(FPS_NT), 0, reinterpret_cast<hipStream_t>(stream), pts, npts, n_max, K,
                static_cast<float4*>(workspace), idx, xyz);
    GDRN_CHECK_LAUNCH();
    return GDRN_OK;
}

extern "C" int gdrn_model_diameter(const double* pts, const int* npts, const int* npts_host, int C, int n_max, double* max_sq, void* stream) {
    const int st = check_models(pts, npts, npts_host, C, n_max);
    if (st != GDRN_OK) return st;
    if (!max_sq) return GDRN_ERR_ARG;
    long long blocks = 0;
    for (int c = 0; c < C; ++c) blocks += dm_pairs(npts_host[c]);
    if (blocks > 0xffffffffLL / DM_NT) return GDRN_ERR_SHAPE;   // (a launch holds fewer than 2^32 threads)
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    GDRN_LAUNCH(diameter_init_kernel, dim3(cdiv(C, 256)), dim3(256), 0, s, reinterpret_cast<u64*>(max_sq), C);
    GDRN_CHECK_LAUNCH();
    GDRN_LAUNCH(diameter_kernel, dim3((unsigned)blocks), dim3(DM_NT), 0, s, pts, npts, n_max, C, reinterpret_cast<u64*>(max_sq));
    GDRN_CHECK_LAUNCH();
    return GDRN_OK;
}
