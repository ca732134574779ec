// Head tail (slice / softmax / concat / extent scaling) and map losses of the GDR-Net RoI path for gfx950 -- forward and backward, no host
// synchronisation.  Reference call sites: GDRN.py:156-169 (glue), conv_pnp_net.py:121-125, GDRN.py:345-400 (losses).
#include "head_tail.h"

namespace {

// ------------------------------------------------------------------------------------------ head tail fwd
template <typename T>
__global__ __launch_bounds__(256) void head_tail_fwd_kernel(const float* __restrict__ head, int hs,
                                                            const float* __restrict__ coord2d,
                                                            const float* __restrict__ extents, T* __restrict__ pnp, int pcs,
                                                            int N, int HW, int nreg, int write_pad) {
    const int q = threadIdx.x & 15;
    const long long M = (long long)N * HW;
    const long long g0 = ((long long)blockIdx.x * blockDim.x + threadIdx.x) >> 4;
    const long long ng = ((long long)gridDim.x * blockDim.x) >> 4;
    for (long long m = g0; m < M; m += ng) {
        const int n = (int)(m / HW), pix = (int)(m - (long long)n * HW);
        const float* h = head + m * hs;
        float r[4], mx = -INFINITY;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            r[j] = (q + 16 * j < nreg) ? h[5 + q + 16 * j] : -INFINITY;
            mx = fmaxf(mx, r[j]);
        }
        mx = row16_max(mx);
        float e[4], se = 0.f;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            e[j] = (q + 16 * j < nreg) ? expf(r[j] - mx) : 0.f;
            se += e[j];
        }
        se = row16_sum(se);
        T* o = pnp + m * pcs;
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (q + 16 * j < nreg) st1<T>(o + 5 + q + 16 * j, e[j] / se);
        if (q < 3) st1<T>(o + q, (h[1 + q] - 0.5f) * extents[n * 3 + q]);
        else if (q < 5) st1<T>(o + q, coord2d[((size_t)n * 2 + (q - 3)) * HW + pix]);
        if (write_pad)   // (GDRN_PREZEROED: the pad channels are the caller's, as on the 64-region path)
            for (int c = 5 + nreg + q; c < pcs; c += 16) st1<T>(o + c, 0.f);
    }
}

// ------------------------------------------------------------------------------------------ head tail fwd, nreg == 64
// The lane map of tail64_store / tail64_loss (head_tail.h): the softmax lands as one 4-channel store per lane, and in train mode (LOSS) the same
// pass accumulates the map losses of gdrn_map_loss_fwd -- the logits are read once instead of twice and the two kernels' ~40 scalar loads / stores
// per lane become ~8 wide ones.
template <typename T, bool LOSS>
__global__ __launch_bounds__(256) void head_tail_fwd64_kernel(const float* __restrict__ head, int hs, const float* __restrict__ coord2d,
                                                              const float* __restrict__ extents, T* __restrict__ pnp, int pcs,
                                                              const float* __restrict__ gt_xyz, const float* __restrict__ mvis,
                                                              const float* __restrict__ mtr, const long long* __restrict__ gt_region,
                                                              double* acc, int N, int HW, int write_pad, int acc_rows) {
    const int q = threadIdx.x & 15;
    const long long M = (long long)N * HW;
    const long long g0 = ((long long)blockIdx.x * blockDim.x + threadIdx.x) >> 4;
    const long long ng = ((long long)gridDim.x * blockDim.x) >> 4;
    float a[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    for (long long m = g0; m < M; m += ng) {
        const int n = (int)(m / HW), pix = (int)(m - (long long)n * HW);
        const float* h = head + m * hs;
        // EVERY load of the iteration goes out here, by all 16 lanes of the pixel (same address: one request): issued where they are used --
        // behind the softmax, inside the `q == 0` / `q == 14` branches -- the loss inputs cost a second memory round trip per iteration
        // (train variant 65 us against 26 us for the eval variant, r4)
        float r[4], h03[4];
        load4<float>(h + 4 + 4 * q, r);                       // classes 4q .. 4q+3
        load4<float>(h, h03);                                 // mask, x, y, z
        const float h68 = h[68];                              // class 64
        const float c2x = coord2d[((size_t)n * 2 + 0) * HW + pix], c2y = coord2d[((size_t)n * 2 + 1) * HW + pix];
        const float ex[3] = {extents[n * 3 + 0], extents[n * 3 + 1], extents[n * 3 + 2]};
        float mv = 0.f, mt = 0.f, gx[3] = {0.f, 0.f, 0.f};
        long long gr = 0;
        if constexpr (LOSS) {
            mv = mvis[m];
            mt = mtr[m];
            gr = gt_region[m];
#pragma unroll
            for (int c = 0; c < 3; ++c) gx[c] = gt_xyz[((size_t)n * 3 + c) * HW + pix];
        }
        T* o = tail64_store<T>(pnp, m, pcs, q, r, h03, h68, c2x, c2y, ex);
        if (write_pad) {
            const float z[4] = {0.f, 0.f, 0.f, 0.f};
            for (int c = 72 + 4 * q; c < pcs; c += 64) store4<T>(o + c, z);
        }
        if constexpr (LOSS) tail64_loss(a, q, r, h03, h68, mv, mt, gr, gx);
    }
    if constexpr (LOSS) loss_sums_store(a, acc, acc_rows);
}

// ------------------------------------------------------------------------------------------ map losses fwd
__global__ __launch_bounds__(256) void map_loss_fwd_kernel(const float* __restrict__ head, int hs,
                                                           const float* __restrict__ gt_xyz,
                                                           const float* __restrict__ mvis, const float* __restrict__ mtr,
                                                           const long long* __restrict__ gt_region, int N, int HW, int nreg,
                                                           double* acc, int acc_rows) {
    const int q = threadIdx.x & 15;
    const long long M = (long long)N * HW;
    const long long g0 = ((long long)blockIdx.x * blockDim.x + threadIdx.x) >> 4;
    const long long ng = ((long long)gridDim.x * blockDim.x) >> 4;
    const int ncls = nreg + 1;
    float a[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};  // accumulators of lane q == 0 of each pixel group
    for (long long m = g0; m < M; m += ng) {
        const int n = (int)(m / HW), pix = (int)(m - (long long)n * HW);
        const float* h = head + m * hs;
        const float mv = mvis[m];
        // CE over nreg+1 classes of logits region*mv; lane q <-> classes q + 16 j
        const int tgt = (int)(gt_region[m] * (long long)mv);
        float z[5], mx = -INFINITY, zt = 0.f;
#pragma unroll
        for (int j = 0; j < 5; ++j) {
            const int k = q + 16 * j;
            z[j] = (k < ncls) ? h[4 + k] * mv : -INFINITY;
            mx = fmaxf(mx, z[j]);
            if (k == tgt) zt = z[j];
        }
        mx = row16_max(mx);
        float e = 0.f;
#pragma unroll
        for (int j = 0; j < 5; ++j)
            if (q + 16 * j < ncls) e += expf(z[j] - mx);
        const float se = row16_sum(e);
        zt = row16_sum(zt);
        if (q == 0) {
            a[4] += (logf(se) + mx) - zt;
            a[5] += mv;
            a[3] += fabsf(h[0] - mtr[m]);
#pragma unroll
            for (int c = 0; c < 3; ++c) a[c] += fabsf(h[1 + c] * mv - gt_xyz[((size_t)n * 3 + c) * HW + pix] * mv);
        }
    }
    loss_sums_store(a, acc, acc_rows);
}

// the five map losses (xyz, mask, region cross entropy) from the totals tot[0..5] of the loss sums
__device__ __forceinline__ void map_losses(const double* tot, double npix, float* out) {
    const double den = tot[5] < 1.0 ? 1.0 : tot[5];
    out[0] = (float)(tot[0] / den);
    out[1] = (float)(tot[1] / den);
    out[2] = (float)(tot[2] / den);
    out[3] = (float)(tot[3] / npix);
    out[4] = (float)(tot[4] / den);
}

// partial rows acc[8 + 8 r + k] (r < nrows, written by the loss kernels in GDRN_ACC_ROWS mode) -> totals acc[0..7] in a fixed order, then the
// five map losses.  1024 threads: thread t sums column t & 7 over rows (t >> 3) + 128 i with all (<= 32) loads of a batch in flight
// together (256 threads walking their rows one load at a time took 17 us for 4096 rows), 128 such sums per column are added in order.
__global__ __launch_bounds__(1024) void map_loss_finalize_rows_kernel(double* acc, int nrows, double npix, float* losses, const float* pose_rows, int N,
                                                                      const float* w, float* weighted) {
    __shared__ double part[128][8], part2[8][8];
    __shared__ double tot[8];
    const int k = threadIdx.x & 7, r0 = threadIdx.x >> 3;
    double v = 0.0;
    for (int rb = 0; rb < nrows; rb += 128 * 32) {
        double x[32];
#pragma unroll
        for (int i = 0; i < 32; ++i) {
            const int r = rb + r0 + 128 * i;
            x[i] = (r < nrows) ? acc[8 + (size_t)r * 8 + k] : 0.0;
        }
#pragma unroll
        for (int i = 0; i < 32; ++i) v += x[i];
    }
    part[r0][k] = (k < 6) ? v : 0.0;
    __syncthreads();
    if (threadIdx.x < 64) {   // column t & 7, eight lanes per column: 16 rows each, then a fixed-order 8-way add through the LDS
        const int c = threadIdx.x & 7, g = threadIdx.x >> 3;
        double t = 0.0;
#pragma unroll
        for (int i = 0; i < 16; ++i) t += part[g * 16 + i][c];
        part2[g][c] = t;
    }
    __syncthreads();
    if (threadIdx.x < 8) {
        double t = 0.0;
#pragma unroll
        for (int i = 0; i < 8; ++i) t += part2[i][threadIdx.x];
        tot[threadIdx.x] = t;
        acc[threadIdx.x] = t;
    }
    __syncthreads();
    __shared__ float lv[8];
    if (threadIdx.x == 0) {
        map_losses(tot, npix, lv);
#pragma unroll
        for (int k = 0; k < 5; ++k) losses[k] = lv[k];
    } else if (threadIdx.x >= 64 && threadIdx.x < 67) {
        // (gdrn_loss_finalize) the three pose losses from gdrn_pose_loss's per-RoI rows, in RoI order (fp32, as the atomics added them -- in a fixed order)
        const int k = threadIdx.x - 64;
        float v = 0.f;
        if (pose_rows != nullptr) {
            for (int n = 0; n < N; ++n) v += pose_rows[n * 4 + k];
            losses[5 + k] = v;
        } else {
            v = losses[5 + k];
        }
        lv[5 + k] = v;
    }
    __syncthreads();
    if (weighted != nullptr && threadIdx.x < 8) weighted[threadIdx.x] = lv[threadIdx.x] * w[threadIdx.x];
}

__global__ void map_loss_finalize_kernel(const double* acc, double npix, float* losses) {
    if (threadIdx.x == 0) map_losses(acc, npix, losses);
}

// ------------------------------------------------------------------------------------------ head tail bwd
template <typename T>
__global__ __launch_bounds__(256) void head_tail_bwd_kernel(const float* __restrict__ head, int hs, const T* __restrict__ pnp,
                                                            const T* __restrict__ dpnp, int pcs,
                                                            const float* __restrict__ extents,
                                                            const float* __restrict__ gt_xyz, const float* __restrict__ mvis,
                                                            const float* __restrict__ mtr,
                                                            const long long* __restrict__ gt_region,
                                                            const double* __restrict__ acc, const float* __restrict__ gw,
                                                            T* __restrict__ dhead, int dcs, int N, int HW, int nreg, int write_pad) {
    const int q = threadIdx.x & 15;  // 16 lanes per pixel, lane q <-> classes q + 16 j
    const long long M = (long long)N * HW;
    const long long g0 = ((long long)blockIdx.x * blockDim.x + threadIdx.x) >> 4;
    const long long ng = ((long long)gridDim.x * blockDim.x) >> 4;
    const float inv_den = (float)(1.0 / (acc[5] < 1.0 ? 1.0 : acc[5]));
    const float inv_np = (float)(1.0 / (double)M);
    const float gx[3] = {gw[0], gw[1], gw[2]};
    const float gmask = gw[3], gce = gw[4];
    const int ncls = nreg + 1;
    for (long long m = g0; m < M; m += ng) {
        const int n = (int)(m / HW), pix = (int)(m - (long long)n * HW);
        const float* h = head + m * hs;
        const float mv = mvis[m];
        const int tgt = (int)(gt_region[m] * (long long)mv);
        // CE gradient: mv * (softmax(region*mv)_k - onehot_k) / den
        float z[5], mx = -INFINITY;
#pragma unroll
        for (int j = 0; j < 5; ++j) {
            const int k = q + 16 * j;
            z[j] = (k < ncls) ? h[4 + k] * mv : -INFINITY;
            mx = fmaxf(mx, z[j]);
        }
        mx = row16_max(mx);
        float e[5], se = 0.f;
#pragma unroll
        for (int j = 0; j < 5; ++j) {
            e[j] = (q + 16 * j < ncls) ? expf(z[j] - mx) : 0.f;
            se += e[j];
        }
        se = row16_sum(se);
        // attention softmax chain: region class k (>= 1) <- pnp channel 4 + k
        float sk[5], dk[5], dot = 0.f;
#pragma unroll
        for (int j = 0; j < 5; ++j) {
            const int k = q + 16 * j;
            const bool on = dpnp != nullptr && k >= 1 && k <= nreg;
            sk[j] = on ? ld1<T>(pnp + m * pcs + 4 + k) : 0.f;
            dk[j] = on ? ld1<T>(dpnp + m * pcs + 4 + k) : 0.f;
            dot += sk[j] * dk[j];
        }
        dot = row16_sum(dot);
        T* o = dhead + m * dcs;
        const float cs = gce * mv * inv_den;
#pragma unroll
        for (int j = 0; j < 5; ++j) {
            const int k = q + 16 * j;
            if (k < ncls) st1<T>(o + 4 + k, cs * (e[j] / se - (tgt == k ? 1.f : 0.f)) + sk[j] * (dk[j] - dot));
        }
        if (q == 0) {
            st1<T>(o + 0, gmask * inv_np * sgn(h[0] - mtr[m]));
        } else if (q < 4) {
            const int c = q - 1;
            const float gt = gt_xyz[((size_t)n * 3 + c) * HW + pix];
            float d = gx[c] * mv * inv_den * sgn(h[1 + c] * mv - gt * mv);
            if (dpnp != nullptr) d += ld1<T>(dpnp + m * pcs + c) * extents[n * 3 + c];
            st1<T>(o + q, d);
        }
        if (write_pad)
            for (int c = 4 + ncls + q; c < dcs; c += 16) st1<T>(o + c, 0.f);
    }
}

// ------------------------------------------------------------------------------------------ head tail bwd, nreg == 64
// same lane <-> class map as head_tail_fwd64_kernel: 16-byte logit loads, 4-channel loads of the softmax / its gradient, one
// 4-channel store per lane.  write_pad = 0: channels >= 72 of d_head are the caller's (zero-filled once).
template <typename T>
__global__ __launch_bounds__(256) void head_tail_bwd64_kernel(const float* __restrict__ head, int hs, const T* __restrict__ pnp,
                                                              const T* __restrict__ dpnp, int pcs, const float* __restrict__ extents,
                                                              const float* __restrict__ gt_xyz, const float* __restrict__ mvis,
                                                              const float* __restrict__ mtr, const long long* __restrict__ gt_region,
                                                              const double* __restrict__ acc, const float* __restrict__ gw,
                                                              T* __restrict__ dhead, int dcs, int N, int HW, int write_pad) {
    const int q = threadIdx.x & 15;
    const long long M = (long long)N * HW;
    const long long g0 = ((long long)blockIdx.x * blockDim.x + threadIdx.x) >> 4;
    const long long ng = ((long long)gridDim.x * blockDim.x) >> 4;
    const float inv_den = (float)(1.0 / (acc[5] < 1.0 ? 1.0 : acc[5]));
    const float inv_np = (float)(1.0 / (double)M);
    const float gx[3] = {gw[0], gw[1], gw[2]};
    const float gmask = gw[3], gce = gw[4];
    for (long long m = g0; m < M; m += ng) {
        const int n = (int)(m / HW), pix = (int)(m - (long long)n * HW);
        const float* h = head + m * hs;
        // every load of the iteration up front, by all 16 lanes of the pixel (see head_tail_fwd64_kernel): the ones that sat in the
        // `q == 14` / `q == 15` branches behind the softmax cost a second memory round trip per iteration
        const float mv = mvis[m];
        const int tgt = (int)(gt_region[m] * (long long)mv);
        float r[4], h03[4];
        load4<float>(h + 4 + 4 * q, r);
        load4<float>(h, h03);                                  // mask, x, y, z
        const float h68 = h[68];
        const float mt = mtr[m];
        float gt3[3], ex[3], d03[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int c = 0; c < 3; ++c) { gt3[c] = gt_xyz[((size_t)n * 3 + c) * HW + pix]; ex[c] = extents[n * 3 + c]; }
        float sk[4] = {0.f, 0.f, 0.f, 0.f}, dk[4] = {0.f, 0.f, 0.f, 0.f}, s64 = 0.f, d64 = 0.f;
        if (dpnp != nullptr) {   // attention softmax chain: region class k (>= 1) <- pnp channel 4 + k
            load4<T>(pnp + m * pcs + 4 + 4 * q, sk);
            load4<T>(dpnp + m * pcs + 4 + 4 * q, dk);
            load4<T>(dpnp + m * pcs, d03);                     // d/d(x, y, z scaled by the extents), channel 3 unused
            s64 = ld1<T>(pnp + m * pcs + 68);
            d64 = ld1<T>(dpnp + m * pcs + 68);
            if (q == 0) { sk[0] = 0.f; dk[0] = 0.f; }   // channel 4 is roi_coord_2d, not a class
            if (q != 15) { s64 = 0.f; d64 = 0.f; }
        }
        // CE gradient: mv * (softmax(region*mv)_k - onehot_k) / den over the 65 classes
        float z[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) z[j] = r[j] * mv;
        const float z64 = (q == 15) ? h68 * mv : -INFINITY;
        float mz = fmaxf(fmaxf(z[0], z[1]), fmaxf(fmaxf(z[2], z[3]), z64));
        mz = row16_max(mz);
        float e[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) e[j] = expf(z[j] - mz);
        const float e64 = (q == 15) ? expf(z64 - mz) : 0.f;
        const float inv = 1.f / row16_sum(e[0] + e[1] + e[2] + e[3] + e64);
        const float dot = row16_sum(sk[0] * dk[0] + sk[1] * dk[1] + sk[2] * dk[2] + sk[3] * dk[3] + s64 * d64);
        T* o = dhead + m * dcs;
        const float cs = gce * mv * inv_den;
        float v[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = cs * (e[j] * inv - (tgt == 4 * q + j ? 1.f : 0.f)) + sk[j] * (dk[j] - dot);
        store4<T>(o + 4 + 4 * q, v);
        if (q == 15) {
            const float w[4] = {cs * (e64 * inv - (tgt == 64 ? 1.f : 0.f)) + s64 * (d64 - dot), 0.f, 0.f, 0.f};
            store4<T>(o + 68, w);
        } else if (q == 14) {
            float w[4];
            w[0] = gmask * inv_np * sgn(h03[0] - mt);
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                float d = gx[c] * mv * inv_den * sgn(h03[1 + c] * mv - gt3[c] * mv);
                if (dpnp != nullptr) d += d03[c] * ex[c];
                w[1 + c] = d;
            }
            store4<T>(o, w);
        }
        if (write_pad) {
            const float zz[4] = {0.f, 0.f, 0.f, 0.f};
            for (int c = 72 + 4 * q; c < dcs; c += 64) store4<T>(o + c, zz);
        }
    }
}

// fast path of the head-tail kernels: 64 regions, rows of whole 4-element groups (16-byte head rows, 8-byte bf16 rows)
inline bool ht64_ok(int nreg, int hs, int pcs) { return nreg == 64 && hs >= 72 && (hs & 3) == 0 && pcs >= 72 && (pcs & 3) == 0; }

// The grids.  16 pixels per 256-thread workgroup and pass; every kernel walks its pixels with a grid stride, so the caps bound the launch, not the
// problem.  In GDRN_ACC_ROWS mode the kernel that carries the loss sums writes one partial row per workgroup: gdrn_head_tail_loss_rows sizes the
// caller's buffer with the SAME function the launch takes its grid from.
constexpr int HT_MAX_BLOCKS = 4096;         // head_tail_fwd*/bwd* (the value the kernels were tuned with; no derivation on record)
constexpr int MAP_LOSS_MAX_BLOCKS = 2048;   // map_loss_fwd_kernel (likewise)
inline int ht_blocks(long long M) { return (int)std::min<long long>((M + 15) / 16, HT_MAX_BLOCKS); }
inline int map_loss_blocks(long long M) { return (int)std::min<long long>((M + 15) / 16, MAP_LOSS_MAX_BLOCKS); }

template <bool LOSS>
int launch_ht_fwd(const float* head, int hs, const float* coord2d, const float* extents, void* pnp_in, int pcs, const float* gt_xyz,
                  const float* mv, const float* mt, const long long* greg, double* acc, int N, int HW, int nreg, int dtype, hipStream_t st) {
    const int write_pad = (dtype & GDRN_PREZEROED) ? 0 : 1, rows = (dtype & GDRN_ACC_ROWS) ? 1 : 0;
    const long long M = (long long)N * HW;
    const int blocks = ht_blocks(M);
    if (ht64_ok(nreg, hs, pcs)) {
        DISPATCH(dtype & 0xff,
                 GDRN_LAUNCH((head_tail_fwd64_kernel<float, LOSS>), dim3(blocks), dim3(256), 0, st, head, hs, coord2d, extents, (float*)pnp_in, pcs,
                             gt_xyz, mv, mt, greg, acc, N, HW, write_pad, rows),
                 GDRN_LAUNCH((head_tail_fwd64_kernel<bf16_t, LOSS>), dim3(blocks), dim3(256), 0, st, head, hs, coord2d, extents, (bf16_t*)pnp_in, pcs,
                             gt_xyz, mv, mt, greg, acc, N, HW, write_pad, rows));
    } else {
        DISPATCH(dtype & 0xff,
                 GDRN_LAUNCH(head_tail_fwd_kernel<float>, dim3(blocks), dim3(256), 0, st, head, hs, coord2d, extents, (float*)pnp_in, pcs, N, HW, nreg, write_pad),
                 GDRN_LAUNCH(head_tail_fwd_kernel<bf16_t>, dim3(blocks), dim3(256), 0, st, head, hs, coord2d, extents, (bf16_t*)pnp_in, pcs, N, HW, nreg, write_pad));
        if (LOSS)
            GDRN_LAUNCH(map_loss_fwd_kernel, dim3(map_loss_blocks(M)), dim3(256), 0, st, head, hs, gt_xyz, mv, mt, greg, N, HW, nreg, acc, rows);
    }
    GDRN_CHECK_LAUNCH();
    return GDRN_OK;
}

}  // namespace

#define ST reinterpret_cast<hipStream_t>(stream)

// partial rows gdrn_head_tail_loss_fwd writes behind acc[0..7] in GDRN_ACC_ROWS mode (= the workgroups of the kernel that carries the sums)
extern "C" int gdrn_head_tail_loss_rows(int N, int HW, int nreg, int hs, int pcs) {
    if (N <= 0 || HW <= 0 || nreg < 1 || nreg > 64) return GDRN_ERR_ARG;
    const long long M = (long long)N * HW;
    return ht64_ok(nreg, hs, pcs) ? ht_blocks(M) : map_loss_blocks(M);
}

extern "C" int gdrn_head_tail_fwd(const float* head, int hs, const float* coord2d, const float* extents, void* pnp_in, int pcs,
                                  int N, int HW, int nreg, int dtype, void* stream) {
    const int dt = dtype & 0xff;
    if (!head || !coord2d || !extents || !pnp_in || N <= 0 || HW <= 0 || nreg < 1 || nreg > 64 || hs < nreg + 5 ||
        pcs < nreg + 5 || (dt != GDRN_DT_F32 && dt != GDRN_DT_H16))
        return GDRN_ERR_ARG;
    return launch_ht_fwd<false>(head, hs, coord2d, extents, pnp_in, pcs, nullptr, nullptr, nullptr, nullptr, nullptr, N, HW, nreg, dtype, ST);
}

extern "C" int gdrn_head_tail_loss_fwd(const float* head, int hs, const float* coord2d, const float* extents, void* pnp_in, int pcs,
                                       const float* gt_xyz, const float* mask_visib, const float* mask_trunc, const long long* gt_region,
                                       double* acc, int N, int HW, int nreg, int dtype, void* stream) {
    const int dt = dtype & 0xff;
    if (!head || !coord2d || !extents || !pnp_in || !gt_xyz || !mask_visib || !mask_trunc || !gt_region || !acc || N <= 0 || HW <= 0 ||
        nreg < 1 || nreg > 64 || hs < nreg + 5 || pcs < nreg + 5 || (dt != GDRN_DT_F32 && dt != GDRN_DT_H16))
        return GDRN_ERR_ARG;
    if (!(dtype & GDRN_ACC_ROWS) && hipMemsetAsync(acc, 0, 8 * sizeof(double), ST) != hipSuccess) return GDRN_ERR_LAUNCH;
    return launch_ht_fwd<true>(head, hs, coord2d, extents, pnp_in, pcs, gt_xyz, mask_visib, mask_trunc, gt_region, acc, N, HW, nreg, dtype, ST);
}

extern "C" int gdrn_map_loss_fwd(const float* head, int hs, const float* gt_xyz, const float* mask_visib, const float* mask_trunc,
                                 const long long* gt_region, int N, int HW, int nreg, double* acc, void* stream) {
    if (!head || !gt_xyz || !mask_visib || !mask_trunc || !gt_region || !acc || N <= 0 || HW <= 0 || nreg < 1 || nreg > 64 || hs < nreg + 5)
        return GDRN_ERR_ARG;
    if (hipMemsetAsync(acc, 0, 8 * sizeof(double), ST) != hipSuccess) return GDRN_ERR_LAUNCH;
    GDRN_LAUNCH(map_loss_fwd_kernel, dim3(map_loss_blocks((long long)N * HW)), dim3(256), 0, ST, head, hs, gt_xyz, mask_visib, mask_trunc, gt_region,
                N, HW, nreg, acc, 0);
    GDRN_CHECK_LAUNCH();
    return GDRN_OK;
}

extern "C" int gdrn_map_loss_finalize(const double* acc, int N, int HW, float* losses, void* stream) {
    if (!acc || !losses) return GDRN_ERR_ARG;
    GDRN_LAUNCH(map_loss_finalize_kernel, dim3(1), dim3(64), 0, ST, acc, (double)N * (double)HW, losses);
    GDRN_CHECK_LAUNCH();
    return GDRN_OK;
}

extern "C" int gdrn_map_loss_finalize_rows(double* acc, int nrows, int N, int HW, float* losses, void* stream) {
    if (!acc || !losses || nrows <= 0 || N <= 0 || HW <= 0) return GDRN_ERR_ARG;
    GDRN_LAUNCH(map_loss_finalize_rows_kernel, dim3(1), dim3(1024), 0, ST, acc, nrows, (double)N * (double)HW, losses, (const float*)nullptr, N,
                (const float*)nullptr, (float*)nullptr);
    GDRN_CHECK_LAUNCH();
    return GDRN_OK;
}

// (ABI 5) ... the same launch also finishes the pose losses from gdrn_pose_loss's per-RoI rows (pose_rows [N][4], nullable: losses[5..7] are then
// already final) and writes weighted[k] = losses[k] * w[k], k < 8 (both nullable): the loss vector the train step returns, without a launch of its own
extern "C" int gdrn_loss_finalize(double* acc, int nrows, int N, int HW, const float* pose_rows, float* losses, const float* w, float* weighted,
                                  void* stream) {
    if (!acc || !losses || nrows <= 0 || N <= 0 || HW <= 0 || ((w != nullptr) != (weighted != nullptr))) return GDRN_ERR_ARG;
    GDRN_LAUNCH(map_loss_finalize_rows_kernel, dim3(1), dim3(1024), 0, ST, acc, nrows, (double)N * (double)HW, losses, pose_rows, N, w, weighted);
    GDRN_CHECK_LAUNCH();
    return GDRN_OK;
}

extern "C" int gdrn_head_tail_bwd(const float* head, int hs, const void* pnp_in, const void* d_pnp_in, int pcs,
                                  const float* extents, const float* gt_xyz, const float* mask_visib, const float* mask_trunc,
                                  const long long* gt_region, const double* acc, const float* gw, void* d_head, int dcs, int N,
                                  int HW, int nreg, int dtype, void* stream) {
    const int dt = dtype & 0xff, write_pad = (dtype & GDRN_PREZEROED) ? 0 : 1;
    if (!head || !extents || !gt_xyz || !mask_visib || !mask_trunc || !gt_region || !acc || !gw || !d_head || N <= 0 ||
        HW <= 0 || nreg < 1 || nreg > 64 || hs < nreg + 5 || dcs < nreg + 5 || (dt != GDRN_DT_F32 && dt != GDRN_DT_H16))
        return GDRN_ERR_ARG;   // (the kernels read h[4 + nreg])
    if (d_pnp_in != nullptr && (pnp_in == nullptr || pcs < nreg + 5)) return GDRN_ERR_ARG;   // (... and pnp[4 + nreg], d_pnp[4 + nreg])
    const int blocks = ht_blocks((long long)N * HW);
    if (ht64_ok(nreg, hs, dcs) && (d_pnp_in == nullptr || ht64_ok(nreg, hs, pcs)))
        DISPATCH(dt,
                 GDRN_LAUNCH(head_tail_bwd64_kernel<float>, dim3(blocks), dim3(256), 0, ST, head, hs, (const float*)pnp_in, (const float*)d_pnp_in, pcs,
                             extents, gt_xyz, mask_visib, mask_trunc, gt_region, acc, gw, (float*)d_head, dcs, N, HW, write_pad),
                 GDRN_LAUNCH(head_tail_bwd64_kernel<bf16_t>, dim3(blocks), dim3(256), 0, ST, head, hs, (const bf16_t*)pnp_in, (const bf16_t*)d_pnp_in,
                             pcs, extents, gt_xyz, mask_visib, mask_trunc, gt_region, acc, gw, (bf16_t*)d_head, dcs, N, HW, write_pad));
    else
        DISPATCH(dt,
                 GDRN_LAUNCH(head_tail_bwd_kernel<float>, dim3(blocks), dim3(256), 0, ST, head, hs, (const float*)pnp_in, (const float*)d_pnp_in, pcs,
                             extents, gt_xyz, mask_visib, mask_trunc, gt_region, acc, gw, (float*)d_head, dcs, N, HW, nreg, write_pad),
                 GDRN_LAUNCH(head_tail_bwd_kernel<bf16_t>, dim3(blocks), dim3(256), 0, ST, head, hs, (const bf16_t*)pnp_in, (const bf16_t*)d_pnp_in,
                             pcs, extents, gt_xyz, mask_visib, mask_trunc, gt_region, acc, gw, (bf16_t*)d_head, dcs, N, HW, nreg, write_pad));
    GDRN_CHECK_LAUNCH();
    return GDRN_OK;
}
