// The two MFMA kernels around the head's 1x1 output conv -- nn.Conv2d(256, 69, 1) of cdpn_rot_head_region.py:127-135 -- of the GDR-Net RoI path for
// gfx950: the conv fused with the 64-region head tail (forward) and its data gradient fused with the BatchNorm-backward sums (backward).
#include "head_tail.h"

namespace {

// ------------------------------------------------------------------------------------------ 1x1 output conv + head tail, nreg == 64
// The head's last layer and the glue behind it (GDRN.py:156-169: slice, softmax over region[:, 1:], concat with roi_coord_2d, extent scaling) in ONE
// pass over the 256-channel activation (r5).  As two launches the fp32 logits (75 MB at bs = 64) are written by a generic 128 x 128 GEMM tile of
// which 59 columns are padding and read back by the tail (70 + 28 us).
// Here: the 69 x 256 weights sit in LDS in MFMA fragment order (5 fragments of 16 channels x 8 k-steps = 40 KB, shared by the four waves); a
// wave takes 16 pixels at a time, its B fragments (pixel r16, 8 input channels per k-group) straight from global memory, 40 MFMAs with the bias as
// the accumulator's initial value, then parks the 16 x 80 logit tile in its own 5 KB of LDS and re-reads it in the tail's lane map (16 lanes per
// pixel, four classes per lane): the softmax and the stores are tail64_store, as in head_tail_fwd64_kernel.  `head` (nullable) still receives the
// fp32 logits for callers that return the maps (cfg.TEST.USE_PNP, gdrn_correspondences).
constexpr int HCT_PITCH = 84;   // floats per pixel row of the wave's logit tile (80 + 4: consecutive pixels 16 bytes apart in the bank map)
// LOSS (train mode, r5): the same pass also accumulates the map losses as head_tail_fwd64_kernel<T, true> does (tail64_loss, GDRN.py:345-400; one
// partial row per workgroup, added in a fixed order by gdrn_map_loss_finalize_rows); `head` is then mandatory -- the backward pass reads the logits.
template <typename T, bool LOSS>
__global__ __launch_bounds__(256) void head_conv_tail64_kernel(const bf16_t* __restrict__ x, int x_cs, const bf16_t* __restrict__ w,
                                                               const float* __restrict__ bias, const float* __restrict__ coord2d,
                                                               const float* __restrict__ extents, float* __restrict__ head, int hs,
                                                               T* __restrict__ pnp, int pcs, int N, int HW, int ngroups,
                                                               const float* __restrict__ gt_xyz, const float* __restrict__ mvis,
                                                               const float* __restrict__ mtr, const long long* __restrict__ gt_region, double* acc) {
    __shared__ __attribute__((aligned(16))) uint4 wl[5 * 8 * 64];            // [fragment][k-step][lane]: one ds_read_b128 per A operand, conflict-free
    __shared__ __attribute__((aligned(16))) float tile[4][16 * HCT_PITCH];
    float a[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, g = lane >> 4, r16 = lane & 15;
    for (int i = threadIdx.x; i < 5 * 8 * 64; i += 256) {   // A operand: row = output channel 16f + (l & 15), k = 32 ks + 8 (l >> 4) .. + 7
        const int l = i & 63, ks = (i >> 6) & 7, f = i >> 9;
        const int row = 16 * f + (l & 15);
        wl[i] = row < 69 ? *reinterpret_cast<const uint4*>(w + (size_t)row * 256 + 32 * ks + 8 * (l >> 4)) : make_uint4(0, 0, 0, 0);
    }
    f32x4_t bv[5];   // bias of the lane's result channels 16f + 4g + j
#pragma unroll
    for (int f = 0; f < 5; ++f)
#pragma unroll
        for (int j = 0; j < 4; ++j) { const int c = 16 * f + 4 * g + j; bv[f][j] = c < 69 ? bias[c] : 0.f; }
    __syncthreads();
    float* tw = tile[wave];
    const int q = lane & 15, sub = lane >> 4;
    const int nw = gridDim.x * 4, gw = blockIdx.x * 4 + wave;
    uint4 xq[8], xn[8];
    auto xload = [&](int grp, uint4 (&dst)[8]) {
        const long long m = (long long)grp * 16 + r16;
        const bf16_t* px = x + (size_t)m * x_cs + 8 * g;
#pragma unroll
        for (int ks = 0; ks < 8; ++ks) dst[ks] = *reinterpret_cast<const uint4*>(px + 32 * ks);
    };
    if (gw < ngroups) xload(gw, xq);
    for (int grp = gw; grp < ngroups; grp += nw) {
        if (grp + nw < ngroups) xload(grp + nw, xn);   // the next pixel group's operand under this group's MFMAs and tail
        // (r6c) the per-pixel inputs of the tail's four passes (2-D coordinates, extents, and in train mode the loss targets) are requested HERE, in
        // front of the MFMAs, for all four passes at once: inside the passes every one of them was a memory round trip of its own
        const int n = (int)(((long long)grp * 16) / HW);   // (a 16-pixel group never straddles two RoIs: HW % 16 == 0, checked by the host)
        const float ex[3] = {extents[n * 3 + 0], extents[n * 3 + 1], extents[n * 3 + 2]};
        float pc2x[4], pc2y[4], pmv[4], pmt[4], pgx[4][3];
        long long pgr[4];
#pragma unroll
        for (int s4 = 0; s4 < 4; ++s4) {
            const long long m = (long long)grp * 16 + 4 * s4 + sub;
            const int pix = (int)(m - (long long)n * HW);
            pc2x[s4] = coord2d[((size_t)n * 2 + 0) * HW + pix];
            pc2y[s4] = coord2d[((size_t)n * 2 + 1) * HW + pix];
            pmv[s4] = 0.f; pmt[s4] = 0.f; pgr[s4] = 0;
            pgx[s4][0] = pgx[s4][1] = pgx[s4][2] = 0.f;
            if constexpr (LOSS) {
                pmv[s4] = mvis[m];
                pmt[s4] = mtr[m];
                pgr[s4] = gt_region[m];
#pragma unroll
                for (int c = 0; c < 3; ++c) pgx[s4][c] = gt_xyz[((size_t)n * 3 + c) * HW + pix];
            }
        }
        f32x4_t acc[5];
#pragma unroll
        for (int f = 0; f < 5; ++f) acc[f] = bv[f];
#pragma unroll
        for (int ks = 0; ks < 8; ++ks)
#pragma unroll
            for (int f = 0; f < 5; ++f)
                acc[f] = GDRN_MFMA16(__builtin_bit_cast(bf16x8_t, wl[(f * 8 + ks) * 64 + lane]), __builtin_bit_cast(bf16x8_t, xq[ks]), acc[f]);
        // D[i = 4g + j][col = r16] of fragment f = channel 16f + 4g + j of pixel r16 -> tile[pixel][channel]
#pragma unroll
        for (int f = 0; f < 5; ++f)
            *reinterpret_cast<float4*>(tw + r16 * HCT_PITCH + 16 * f + 4 * g) = make_float4(acc[f][0], acc[f][1], acc[f][2], acc[f][3]);
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // the tile is this wave's own: its LDS operations complete in order
        __builtin_amdgcn_wave_barrier();
#pragma unroll
        for (int s4 = 0; s4 < 4; ++s4) {   // the tail, four pixels per pass (16 lanes each), as head_tail_fwd64_kernel
            const int pl = 4 * s4 + sub;
            const long long m = (long long)grp * 16 + pl;
            const float* h = tw + pl * HCT_PITCH;
            float r[4], h03[4];
            load4<float>(h + 4 + 4 * q, r);
            load4<float>(h, h03);
            const float h68 = h[68];
            if (head != nullptr) {   // the fp32 logits, 72 floats per pixel: 16 lanes x 16 bytes + two more
                float* ho = head + m * hs;
                store4<float>(ho + 4 * q, *reinterpret_cast<const float(*)[4]>(h + 4 * q));
                if (q < 2) store4<float>(ho + 64 + 4 * q, *reinterpret_cast<const float(*)[4]>(h + 64 + 4 * q));
            }
            tail64_store<T>(pnp, m, pcs, q, r, h03, h68, pc2x[s4], pc2y[s4], ex);
            if constexpr (LOSS) tail64_loss(a, q, r, h03, h68, pmv[s4], pmt[s4], pgr[s4], pgx[s4]);
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // the tail's reads are done before the next group overwrites the tile
        __builtin_amdgcn_wave_barrier();
#pragma unroll
        for (int ks = 0; ks < 8; ++ks) xq[ks] = xn[ks];
    }
    if constexpr (LOSS) loss_sums_store(a, acc, true);   // always this workgroup's partial row [8 + blockIdx.x * 8 .. + 5]
}

// ------------------------------------------------------------------------------------------ 1x1 output conv: data gradient + BatchNorm-backward sums
// The data gradient of the head's nn.Conv2d(256, 69, 1) -- d_act[px][256] = d_logits[px][69] . W -- with the ReLU mask and the two BatchNorm-backward
// sums of the BatchNorm(+ReLU) in front of the conv in its epilogue (what gdrn_conv_gemm's bnb_* epilogue does for this launch; autograd,
// core/gdrn_modeling/engine.py:279).  On the generic 128 x 128 tile this is the step's least efficient launch (K = 69 of a 128-deep reduction, 83 TFLOP/s,
// 111 us for 335 MB).  Here (r5): W^T in LDS in fragment order (16 fragments of 16 channels x 3 k-steps of 32 = 48 KB); a wave takes 16 pixels at a
// time -- B fragments (pixel r16, 8 logit gradients per k-group) straight from global memory, 48 MFMAs -- and turns the 16 x 256 fp32 result through a
// wave-private LDS tile, 64 channels at a time, into the layout in which the tensors stream: a lane owns 8 consecutive channels of one pixel = one
// 16-byte load of the BatchNorm's raw input and one 16-byte store, eight lanes a pixel's 128-byte line.  A lane meets the same 32 channels for every
// pixel it handles, so the BatchNorm-backward sums are 64 lane-local accumulators, reduced once at the end: one partial row [2][256] per workgroup.
constexpr int HOD_PITCH = 68;   // floats per pixel of the wave's 64-channel result tile
template <typename T>
__global__ __launch_bounds__(256, 2) void head_out_dgrad64_kernel(const bf16_t* __restrict__ dy, int dy_cs, const bf16_t* __restrict__ wd, int wd_cs,
                                                               const bf16_t* __restrict__ raw, int raw_cs, const float* __restrict__ mean,
                                                               const float* __restrict__ invstd, const float* __restrict__ scale,
                                                               const float* __restrict__ shift, bf16_t* __restrict__ dx, int dx_cs,
                                                               float* __restrict__ rows, int ngroups) {
    __shared__ __attribute__((aligned(16))) uint4 wl[16 * 3 * 64];          // [fragment][k-step][lane]
    __shared__ __attribute__((aligned(16))) float tab[4][256];              // mean, 1/std, forward scale, forward shift per channel
    __shared__ __attribute__((aligned(16))) float tile[4][16 * HOD_PITCH];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, g = lane >> 4, r16 = lane & 15;
    for (int i = threadIdx.x; i < 16 * 3 * 64; i += 256) {   // A operand: row = input channel 16f + (l & 15), k = logit 32 ks + 8 (l >> 4) .. + 7
        const int l = i & 63, ks = (i >> 6) % 3, f = i / 192;
        wl[i] = *reinterpret_cast<const uint4*>(wd + (size_t)(16 * f + (l & 15)) * wd_cs + 32 * ks + 8 * (l >> 4));
    }
    for (int c = threadIdx.x; c < 256; c += 256) { tab[0][c] = mean[c]; tab[1][c] = invstd[c]; tab[2][c] = scale[c]; tab[3][c] = shift[c]; }
    __syncthreads();
    float* tw = tile[wave];
    const int oct = lane & 7, psub = lane >> 3;   // streaming layout: channel octet of the 64-channel quarter, pixel 0..7 (+ 8 in the second half)
    float t1[4][8], t2[4][8];
#pragma unroll
    for (int qd = 0; qd < 4; ++qd)
#pragma unroll
        for (int j = 0; j < 8; ++j) { t1[qd][j] = 0.f; t2[qd][j] = 0.f; }
    const int nw = gridDim.x * 4;
    for (int grp = blockIdx.x * 4 + wave; grp < ngroups; grp += nw) {
        const long long m0 = (long long)grp * 16;
        uint4 yq[3];
#pragma unroll
        for (int ks = 0; ks < 3; ++ks) yq[ks] = *reinterpret_cast<const uint4*>(dy + (size_t)(m0 + r16) * dy_cs + 32 * ks + 8 * g);
        uint4 rq[4][2];   // the raw BatchNorm input of the lane's (pixel, octet) pairs: all eight loads of the group go out before the MFMAs
#pragma unroll
        for (int qd = 0; qd < 4; ++qd)
#pragma unroll
            for (int hf = 0; hf < 2; ++hf)
                rq[qd][hf] = *reinterpret_cast<const uint4*>(raw + (size_t)(m0 + psub + 8 * hf) * raw_cs + 64 * qd + 8 * oct);
        f32x4_t acc[16];
#pragma unroll
        for (int f = 0; f < 16; ++f) acc[f] = f32x4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int ks = 0; ks < 3; ++ks)
#pragma unroll
            for (int f = 0; f < 16; ++f)
                acc[f] = GDRN_MFMA16(__builtin_bit_cast(bf16x8_t, wl[(f * 3 + ks) * 64 + lane]), __builtin_bit_cast(bf16x8_t, yq[ks]), acc[f]);
#pragma unroll
        for (int qd = 0; qd < 4; ++qd) {   // channels 64 qd .. 64 qd + 63
#pragma unroll
            for (int f4 = 0; f4 < 4; ++f4) {
                const f32x4_t v = acc[4 * qd + f4];
                *reinterpret_cast<float4*>(tw + r16 * HOD_PITCH + 16 * f4 + 4 * g) = make_float4(v[0], v[1], v[2], v[3]);
            }
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            __builtin_amdgcn_wave_barrier();
            const int c0 = 64 * qd + 8 * oct;
            float km[8], ki[8], kc[8], kh[8];
#pragma unroll
            for (int j4 = 0; j4 < 2; ++j4) {
                const float4 a0 = *reinterpret_cast<const float4*>(&tab[0][c0 + 4 * j4]), a1 = *reinterpret_cast<const float4*>(&tab[1][c0 + 4 * j4]);
                const float4 a2 = *reinterpret_cast<const float4*>(&tab[2][c0 + 4 * j4]), a3 = *reinterpret_cast<const float4*>(&tab[3][c0 + 4 * j4]);
                km[4 * j4] = a0.x; km[4 * j4 + 1] = a0.y; km[4 * j4 + 2] = a0.z; km[4 * j4 + 3] = a0.w;
                ki[4 * j4] = a1.x; ki[4 * j4 + 1] = a1.y; ki[4 * j4 + 2] = a1.z; ki[4 * j4 + 3] = a1.w;
                kc[4 * j4] = a2.x; kc[4 * j4 + 1] = a2.y; kc[4 * j4 + 2] = a2.z; kc[4 * j4 + 3] = a2.w;
                kh[4 * j4] = a3.x; kh[4 * j4 + 1] = a3.y; kh[4 * j4 + 2] = a3.z; kh[4 * j4 + 3] = a3.w;
            }
#pragma unroll
            for (int hf = 0; hf < 2; ++hf) {
                const int pl = psub + 8 * hf;
                float gq[8];
                {
                    const float4 u0 = *reinterpret_cast<const float4*>(tw + pl * HOD_PITCH + 8 * oct), u1 = *reinterpret_cast<const float4*>(tw + pl * HOD_PITCH + 8 * oct + 4);
                    gq[0] = u0.x; gq[1] = u0.y; gq[2] = u0.z; gq[3] = u0.w; gq[4] = u1.x; gq[5] = u1.y; gq[6] = u1.z; gq[7] = u1.w;
                }
                float xv[8];
                Vec16<bf16_t>::unpack(rq[qd][hf], xv);
                float ov[8];
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const bool keep = xv[j] * kc[j] + kh[j] > 0.f;
                    const float gv = keep ? gq[j] : 0.f;
                    ov[j] = gv;
                    t1[qd][j] += gv;
                    t2[qd][j] += gv * (xv[j] - km[j]) * ki[j];
                }
                *reinterpret_cast<uint4*>(dx + (size_t)(m0 + pl) * dx_cs + c0) = Vec16<bf16_t>::pack(ov);
            }
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // the tile's reads are done before the next quarter overwrites it
            __builtin_amdgcn_wave_barrier();
        }
    }
    // the lane's 32 channels (quarter qd, octet oct, j) summed over the eight lanes that share the octet (psub = lane >> 3), then over the four waves
    // in a fixed order: one partial row [2][256] per workgroup
    __syncthreads();   // (every wave is done with its tile; the tiles are reused as the reduction buffer: [wave][2][256] floats = 8 KB <= 4 x 4352 B)
    float* red = &tile[0][0];
#pragma unroll
    for (int qd = 0; qd < 4; ++qd)
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            float u1 = t1[qd][j], u2 = t2[qd][j];
#pragma unroll
            for (int o = 8; o < 64; o <<= 1) { u1 += __shfl_xor(u1, o, 64); u2 += __shfl_xor(u2, o, 64); }
            if (psub == 0) {
                red[(wave * 2 + 0) * 256 + 64 * qd + 8 * oct + j] = u1;
                red[(wave * 2 + 1) * 256 + 64 * qd + 8 * oct + j] = u2;
            }
        }
    __syncthreads();
    for (int i = threadIdx.x; i < 512; i += 256)
        rows[(size_t)blockIdx.x * 512 + i] = (red[i] + red[512 + i]) + (red[1024 + i] + red[1536 + i]);
}

// The grids: a wave takes 16-pixel groups with a grid stride, four waves per workgroup; each workgroup writes ONE partial row, so the `_rows` queries
// that size the callers' buffers and the launches take their grids from the same functions.
constexpr int HCT_MAX_BLOCKS = 1024;   // head_conv_tail64_kernel: two 62 KB workgroups per CU, two rounds
constexpr int HOD_MAX_BLOCKS = 512;    // head_out_dgrad64_kernel: two 69 KB workgroups per CU (its launch bounds), one round
inline int hct_blocks(long long M) { return (int)std::min<long long>((M / 16 + 3) / 4, HCT_MAX_BLOCKS); }
inline int hod_blocks(long long M) { return (int)std::min<long long>((M / 16 + 3) / 4, HOD_MAX_BLOCKS); }

#define ST reinterpret_cast<hipStream_t>(stream)

// eval (LOSS = false: the loss pointers are unused) and train mode of the fused conv + tail behind one shape check
template <bool LOSS>
int launch_hct(const void* x, int x_cs, const void* w, int w_rows, const float* bias, const float* coord2d, const float* extents, float* head, int hs,
               void* pnp_in, int pcs, const float* gt_xyz, const float* mask_visib, const float* mask_trunc, const long long* gt_region, double* acc,
               int N, int HW, int nreg, int dtype, void* stream) {
    const int dt = dtype & 0xff;
    if (!x || !w || !bias || !coord2d || !extents || !pnp_in || N <= 0 || HW <= 0) return GDRN_ERR_ARG;
    if (dt != GDRN_DT_H16 || nreg != 64 || w_rows < 69 || x_cs < 256 || (x_cs & 7) || pcs < 72 || (pcs & 3) || (head && (hs < 72 || (hs & 3)))) return GDRN_ERR_SHAPE;
    const long long M = (long long)N * HW;
    if ((HW & 15) || M * std::max(x_cs, pcs) >= (1ll << 31)) return GDRN_ERR_SHAPE;   // (a 16-pixel group belongs to ONE RoI)
    GDRN_LAUNCH((head_conv_tail64_kernel<bf16_t, LOSS>), dim3(hct_blocks(M)), dim3(256), 0, ST, reinterpret_cast<const bf16_t*>(x), x_cs,
                reinterpret_cast<const bf16_t*>(w), bias, coord2d, extents, head, hs, reinterpret_cast<bf16_t*>(pnp_in), pcs, N, HW, (int)(M / 16), gt_xyz,
                mask_visib, mask_trunc, gt_region, acc);
    GDRN_CHECK_LAUNCH();
    return GDRN_OK;
}

}  // namespace

// eval mode, nreg = 64: the head's 1x1 output conv (256 -> 69, weight rows [>= 69][256] in the 16-bit format, fp32 bias) + gdrn_head_tail_fwd in
// one launch; x: [N*HW][x_cs] 16-bit activations, head (nullable): fp32 logits [N*HW][hs >= 72], pnp_in: [N*HW][pcs >= 72] (pad channels the caller's)
extern "C" int gdrn_head_conv_tail_fwd(const void* x, int x_cs, const void* w, int w_rows, const float* bias, const float* coord2d,
                                       const float* extents, float* head, int hs, void* pnp_in, int pcs, int N, int HW, int nreg, int dtype,
                                       void* stream) {
    return launch_hct<false>(x, x_cs, w, w_rows, bias, coord2d, extents, head, hs, pnp_in, pcs, nullptr, nullptr, nullptr, nullptr, nullptr, N, HW, nreg,
                             dtype, stream);
}

// train mode: the same + the map-loss sums of gdrn_head_tail_loss_fwd as per-workgroup partial rows: acc = 8 + 8 * gdrn_head_conv_tail_loss_rows(N, HW)
// doubles, finished by gdrn_map_loss_finalize_rows; head (the fp32 logits) is mandatory -- gdrn_head_tail_bwd reads it
extern "C" int gdrn_head_conv_tail_loss_rows(int N, int HW) {
    const long long M = (long long)N * HW;
    if (N <= 0 || HW <= 0 || (M & 15)) return GDRN_ERR_ARG;
    return hct_blocks(M);
}

extern "C" int gdrn_head_conv_tail_loss_fwd(const void* x, int x_cs, const void* w, int w_rows, const float* bias, const float* coord2d,
                                            const float* extents, float* head, int hs, void* pnp_in, int pcs, const float* gt_xyz,
                                            const float* mask_visib, const float* mask_trunc, const long long* gt_region, double* acc, int N, int HW,
                                            int nreg, int dtype, void* stream) {
    if (!head || !gt_xyz || !mask_visib || !mask_trunc || !gt_region || !acc) return GDRN_ERR_ARG;
    return launch_hct<true>(x, x_cs, w, w_rows, bias, coord2d, extents, head, hs, pnp_in, pcs, gt_xyz, mask_visib, mask_trunc, gt_region, acc, N, HW, nreg,
                            dtype, stream);
}

// data gradient of the 1x1 output conv with the BatchNorm(+ReLU)-backward mask and sums of the layer in front of it: dy = d_logits [N*HW][dy_cs >= 96]
// (16-bit; channels >= 69 zero), wd = the data-gradient operand rows [256][wd_cs >= 96] (row ci = W[:, ci], columns >= 69 zero), raw = that BatchNorm's raw
// input [N*HW][raw_cs], mean / invstd / scale / shift its statistics and forward affine (mask = scale * raw + shift > 0), dx = the masked gradient
// [N*HW][dx_cs], rows = [gdrn_head_out_dgrad_rows(N, HW)][2][256] partial sums for gdrn_bn_bwd_coef
extern "C" int gdrn_head_out_dgrad_rows(int N, int HW) {
    const long long M = (long long)N * HW;
    if (N <= 0 || HW <= 0 || (M & 15)) return GDRN_ERR_ARG;
    return hod_blocks(M);
}

extern "C" int gdrn_head_out_dgrad(const void* dy, int dy_cs, const void* wd, int wd_cs, const void* raw, int raw_cs, const float* mean,
                                   const float* invstd, const float* scale, const float* shift, void* dx, int dx_cs, float* rows, int N, int HW,
                                   int dtype, void* stream) {
    const int dt = dtype & 0xff;
    if (!dy || !wd || !raw || !mean || !invstd || !scale || !shift || !dx || !rows || N <= 0 || HW <= 0) return GDRN_ERR_ARG;
    if (dt != GDRN_DT_H16 || dy_cs < 96 || wd_cs < 96 || raw_cs < 256 || dx_cs < 256 || ((dy_cs | wd_cs | raw_cs | dx_cs) & 7)) return GDRN_ERR_SHAPE;
    const long long M = (long long)N * HW;
    if ((M & 15) || M * std::max(std::max(dy_cs, raw_cs), dx_cs) >= (1ll << 31)) return GDRN_ERR_SHAPE;
    GDRN_LAUNCH(head_out_dgrad64_kernel<bf16_t>, dim3(hod_blocks(M)), dim3(256), 0, ST, reinterpret_cast<const bf16_t*>(dy), dy_cs,
                reinterpret_cast<const bf16_t*>(wd), wd_cs, reinterpret_cast<const bf16_t*>(raw), raw_cs, mean, invstd, scale, shift,
                reinterpret_cast<bf16_t*>(dx), dx_cs, rows, (int)(M / 16));
    GDRN_CHECK_LAUNCH();
    return GDRN_OK;
}
