// Patch-PnP's pose decode and pose losses of the GDR-Net RoI path for gfx950 -- forward and dL/dfc in one launch, no host synchronisation.
// Reference call sites: GDRN.py:401-471 (losses), rot_reps.py:34-49, pose_from_pred_centroid_z.py:52-227, core/utils/utils.py:39-94,208-236,
// pose_utils.py:323-370,430-482, pm_loss.py:82-114, lib/pysixd/misc.py:930-949, pose_error.py:400-425.
#include <hip/amd_detail/amd_hip_unsafe_atomics.h>

#include "common.h"

namespace {

// ------------------------------------------------------------------------------------------ pose decode
// Forward-mode dual number for the nine inputs (rot6d[6], t_[3]) of the train-mode decode.  (r6b) One partial per LANE: lane k < 9 of the
// workgroup carries d/d(input k), every lane computes the value part redundantly -- the nine partials of a quantity used to be a 9-loop on one
// thread (20 us of serial arithmetic per RoI in a launch nothing overlaps with).  Same operations per partial, same results bit for bit.
struct D9 {
    float v;
    float d[1];
};
constexpr int DNP = 1;
__device__ __forceinline__ D9 dconst(float c) { D9 r; r.v = c; for (int i = 0; i < DNP; ++i) r.d[i] = 0.f; return r; }
__device__ __forceinline__ D9 dvar(float v, int k, int mine) { D9 r = dconst(v); r.d[0] = (k == mine) ? 1.f : 0.f; return r; }
__device__ __forceinline__ D9 operator+(const D9& a, const D9& b) { D9 r; r.v = a.v + b.v; for (int i = 0; i < DNP; ++i) r.d[i] = a.d[i] + b.d[i]; return r; }
__device__ __forceinline__ D9 operator-(const D9& a, const D9& b) { D9 r; r.v = a.v - b.v; for (int i = 0; i < DNP; ++i) r.d[i] = a.d[i] - b.d[i]; return r; }
__device__ __forceinline__ D9 operator*(const D9& a, const D9& b) { D9 r; r.v = a.v * b.v; for (int i = 0; i < DNP; ++i) r.d[i] = a.d[i] * b.v + a.v * b.d[i]; return r; }
__device__ __forceinline__ D9 operator*(const D9& a, float s) { D9 r; r.v = a.v * s; for (int i = 0; i < DNP; ++i) r.d[i] = a.d[i] * s; return r; }
__device__ __forceinline__ D9 operator+(const D9& a, float s) { D9 r = a; r.v += s; return r; }
__device__ __forceinline__ D9 operator/(const D9& a, const D9& b) {
    D9 r; const float ib = 1.f / b.v; r.v = a.v * ib;
    for (int i = 0; i < DNP; ++i) r.d[i] = (a.d[i] - r.v * b.d[i]) * ib;
    return r;
}
__device__ __forceinline__ D9 dfun(const D9& a, float f, float df) { D9 r; r.v = f; for (int i = 0; i < DNP; ++i) r.d[i] = a.d[i] * df; return r; }
__device__ __forceinline__ D9 dsqrt(const D9& a) { const float s = sqrtf(a.v); return dfun(a, s, s > 0.f ? 0.5f / s : 0.f); }
__device__ __forceinline__ D9 dacos(const D9& a) { const float q = 1.f - a.v * a.v; return dfun(a, acosf(a.v), q > 0.f ? -1.f / sqrtf(q) : 0.f); }
__device__ __forceinline__ D9 dsin(const D9& a) { return dfun(a, sinf(a.v), cosf(a.v)); }
__device__ __forceinline__ D9 dcos(const D9& a) { return dfun(a, cosf(a.v), -sinf(a.v)); }

template <typename S>
__device__ __forceinline__ void cross3(const S* a, const S* b, S* o) {
    o[0] = a[1] * b[2] - a[2] * b[1];
    o[1] = a[2] * b[0] - a[0] * b[2];
    o[2] = a[0] * b[1] - a[1] * b[0];
}

// F.normalize(v, p=2, dim=1, eps=1e-12): v / max(||v||, eps)
__device__ __forceinline__ void normalize3(const D9* v, D9* o) {
    D9 n = dsqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
    if (n.v < 1e-12f) n = dconst(1e-12f);
    for (int i = 0; i < 3; ++i) o[i] = v[i] / n;
}

// train-mode decode (differentiable): R_ego[9] row-major, t[3]
__device__ void decode_train(const D9* in, const float* K, const float* ctr, const float* wh, float ratio, D9* R, D9* t) {
    const float eps = 1e-4f;
    D9 x[3], y[3], z[3], zr[3];
    normalize3(in, x);            // x = normalize(a1)
    cross3(x, in + 3, zr);        // z = normalize(x x a2)
    normalize3(zr, z);
    cross3(z, x, y);              // y = z x x ; R_allo = [x y z] as columns
    D9 cx = in[6] * wh[0] + ctr[0];
    D9 cy = in[7] * wh[1] + ctr[1];
    D9 zz = in[8] * ratio;
    t[2] = zz;
    // written as in the reference: z * (cx - px) / fx
    t[0] = (zz * (cx + (-K[2]))) / dconst(K[0]);
    t[1] = (zz * (cy + (-K[5]))) / dconst(K[4]);
    D9 nt = dsqrt(t[0] * t[0] + t[1] * t[1] + t[2] * t[2]) + eps;
    D9 ray[3] = {t[0] / nt, t[1] / nt, t[2] / nt};
    D9 angle = dacos(ray[2]);
    // axis = cross((0,0,1), ray) = (-ray_y, ray_x, 0)
    D9 ax[3] = {dconst(0.f) - ray[1], ray[0], dconst(0.f)};
    D9 na = dsqrt(ax[0] * ax[0] + ax[1] * ax[1] + ax[2] * ax[2]) + eps;
    D9 half = angle * 0.5f;
    D9 sh = dsin(half);
    D9 q[4] = {dcos(half), (ax[0] / na) * sh, (ax[1] / na) * sh, (ax[2] / na) * sh};
    D9 nq = dsqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
    D9 qw = q[0] / nq, qx = q[1] / nq, qy = q[2] / nq, qz = q[3] / nq;
    D9 X = qx * 2.f, Y = qy * 2.f, Z = qz * 2.f;
    D9 wX = qw * X, wY = qw * Y, wZ = qw * Z, xX = qx * X, xY = qx * Y, xZ = qx * Z, yY = qy * Y, yZ = qy * Z, zZ = qz * Z;
    D9 one = dconst(1.f);
    D9 Q[9] = {one - (yY + zZ), xY - wZ, xZ + wY, xY + wZ, one - (xX + zZ), yZ - wX, xZ - wY, yZ + wX, one - (xX + yY)};
    // R_allo[r][c]: column 0 = x, 1 = y, 2 = z
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) {
            const D9* col = (c == 0) ? x : ((c == 1) ? y : z);
            R[r * 3 + c] = Q[r * 3 + 0] * col[0] + Q[r * 3 + 1] * col[1] + Q[r * 3 + 2] * col[2];
        }
}

// test-mode decode (reference: numpy float64 loop, no eps, `if angle > 0`)
__device__ void decode_test(const float* in, const float* K, const float* ctr, const float* wh, float ratio, float* R, float* t) {
    // rot6d -> R_allo in fp32 exactly as train mode (torch ops), then fp64 allo->ego
    float x[3], y[3], z[3], zr[3];
    float n = fmaxf(sqrtf(in[0] * in[0] + in[1] * in[1] + in[2] * in[2]), 1e-12f);
    for (int i = 0; i < 3; ++i) x[i] = in[i] / n;
    cross3(x, in + 3, zr);
    n = fmaxf(sqrtf(zr[0] * zr[0] + zr[1] * zr[1] + zr[2] * zr[2]), 1e-12f);
    for (int i = 0; i < 3; ++i) z[i] = zr[i] / n;
    cross3(z, x, y);
    const float cx = in[6] * wh[0] + ctr[0], cy = in[7] * wh[1] + ctr[1], zz = in[8] * ratio;
    t[0] = zz * (cx - K[2]) / K[0];
    t[1] = zz * (cy - K[5]) / K[4];
    t[2] = zz;
    const float nt32 = sqrtf(t[0] * t[0] + t[1] * t[1] + t[2] * t[2]);  // np.linalg.norm on float32
    const float ray32[3] = {t[0] / nt32, t[1] / nt32, t[2] / nt32};
    double c = (double)ray32[2];
    c = c > 1.0 ? 1.0 : (c < -1.0 ? -1.0 : c);
    const double angle = acos(c);
    double Q[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
    if (angle > 0.0) {
        double ax = -(double)ray32[1], ay = (double)ray32[0], az = 0.0;
        const double na = sqrt(ax * ax + ay * ay + az * az);
        ax /= na; ay /= na; az /= na;
        const double cs = cos(angle), sn = sin(angle), C = 1.0 - cs;
        Q[0] = ax * ax * C + cs;      Q[1] = ax * ay * C - az * sn; Q[2] = ax * az * C + ay * sn;
        Q[3] = ay * ax * C + az * sn; Q[4] = ay * ay * C + cs;      Q[5] = ay * az * C - ax * sn;
        Q[6] = az * ax * C - ay * sn; Q[7] = az * ay * C + ax * sn; Q[8] = az * az * C + cs;
    }
    for (int r = 0; r < 3; ++r)
        for (int cc = 0; cc < 3; ++cc) {
            const float* col = (cc == 0) ? x : ((cc == 1) ? y : z);
            R[r * 3 + cc] = (float)(Q[r * 3 + 0] * (double)col[0] + Q[r * 3 + 1] * (double)col[1] + Q[r * 3 + 2] * (double)col[2]);
        }
}

__device__ double rot_err_deg(const double* A, const double* B) {  // pose_error.re: arccos((tr(A B^T)-1)/2)
    double tr = 0.0;
    for (int i = 0; i < 9; ++i) tr += A[i] * B[i];
    if (tr > 3.0) tr = 3.0;
    double c = 0.5 * (tr - 1.0);
    c = c > 1.0 ? 1.0 : (c < -1.0 ? -1.0 : c);
    return acos(c) * 57.29577951308232;
}

__global__ __launch_bounds__(256) void pose_loss_kernel(const gdrn_pose_params p) {
    __shared__ float sR[9], sG[9], sT[3], sW;
    __shared__ float red[10][4];
    __shared__ float sS[10];
    const int n = blockIdx.x, tid = threadIdx.x;
    __shared__ float fcs[12], red9[9][4];
    const float* in = p.fc + (size_t)n * p.fs;
    if (p.fc2_ws != nullptr) {
        // (ABI 5) the tail of Patch-PnP's fully connected stack in this launch (conv_pnp_net.py:152-160): fc2's split-K slabs -> bias + LeakyReLU
        // (gdrn_linear_splitk's finish pass) -> fc_r | fc_t (a 9 x 256 product per RoI) -> p.fc; then the decode below.  One workgroup per RoI,
        // thread c = fc2 channel c.  The three launches this replaces (finish, a one-workgroup GEMM, this kernel) were 20 us of latency.
        float v = 0.f;
        for (int sp = 0; sp < p.fc2_splits; ++sp) v += p.fc2_ws[((size_t)sp * p.N + n) * 256 + tid];
        v += p.fc2_bias[tid];
        v = v > 0.f ? v : 0.1f * v;
        const bf16_t hv = f2bf(v);
        reinterpret_cast<bf16_t*>(p.f2_out)[(size_t)n * 256 + tid] = hv;
        const float a = bf2f(hv);
        const bf16_t* wr = reinterpret_cast<const bf16_t*>(p.w_rt);
#pragma unroll
        for (int k = 0; k < 9; ++k) {
            const float s_ = wave_sum(a * bf2f(wr[k * 256 + tid]));
            if ((tid & 63) == 0) red9[k][tid >> 6] = s_;
        }
        __syncthreads();
        if (tid < 9) {
            const float o = ((red9[tid][0] + red9[tid][1]) + (red9[tid][2] + red9[tid][3])) + p.b_rt[tid];
            fcs[tid] = o;
            p.fc_w[(size_t)n * p.fs + tid] = o;
        }
        __syncthreads();
        in = fcs;
    }
    const float* K = p.cams + n * 9;
    const float* ctr = p.centers + n * 2;
    const float* wh = p.whs + n * 2;
    const float ratio = p.ratios[n];

    D9 Rd[9], td[3];
    if (p.train && tid < 9) {   // lane k: the value parts + the partial derivatives w.r.t. input k
        D9 v[9];
        for (int k = 0; k < 9; ++k) v[k] = dvar(in[k], k, tid);
        decode_train(v, K, ctr, wh, ratio, Rd, td);
    }
    if (tid == 0) {
        float Rf[9], tf[3];
        if (p.train) {
            for (int k = 0; k < 9; ++k) Rf[k] = Rd[k].v;
            for (int k = 0; k < 3; ++k) tf[k] = td[k].v;
        } else {
            decode_test(in, K, ctr, wh, ratio, Rf, tf);
        }
        for (int k = 0; k < 9; ++k) { sR[k] = Rf[k]; p.rot[n * 9 + k] = Rf[k]; }
        for (int k = 0; k < 3; ++k) { sT[k] = tf[k]; p.trans[n * 3 + k] = tf[k]; }
        if (p.gt_rot != nullptr) {
            // closest symmetric ground truth (pose_utils.py:430-482), errors in fp64
            double P[9], G0[9], best[9];
            for (int k = 0; k < 9; ++k) { P[k] = Rf[k]; G0[k] = p.gt_rot[n * 9 + k]; best[k] = G0[k]; }
            double best_err = rot_err_deg(P, G0);
            const double err0 = best_err;
            const int ns = (p.sym != nullptr && p.sym_count != nullptr) ? p.sym_count[n] : 0;
            for (int s = 0; s < ns; ++s) {
                const float* S = p.sym + ((size_t)n * p.Kmax + s) * 9;
                double C[9];
                for (int r = 0; r < 3; ++r)
                    for (int c = 0; c < 3; ++c) C[r * 3 + c] = G0[r * 3 + 0] * S[0 * 3 + c] + G0[r * 3 + 1] * S[1 * 3 + c] + G0[r * 3 + 2] * S[2 * 3 + c];
                const double e = rot_err_deg(P, C);
                if (e < best_err) { best_err = e; for (int k = 0; k < 9; ++k) best[k] = C[k]; }
            }
            for (int k = 0; k < 9; ++k) sG[k] = (float)best[k];
            if (p.vis != nullptr) {
                p.vis[n * 2 + 0] = (float)err0;
                float te = 0.f;
                if (p.gt_trans != nullptr)
                    for (int k = 0; k < 3; ++k) { const float d = p.gt_trans[n * 3 + k] - tf[k]; te += d * d; }
                p.vis[n * 2 + 1] = sqrtf(te);
            }
        }
        if (p.extents != nullptr) sW = 1.f / fmaxf(fmaxf(p.extents[n * 3], p.extents[n * 3 + 1]), p.extents[n * 3 + 2]);
    }
    __syncthreads();
    if (!p.train || p.gt_rot == nullptr || p.points == nullptr) return;

    // point-matching loss: sum_p sum_a |w (R p - Rgt p)_a| and S[a][b] = sum_p sign(.)_a w p_b
    float acc[10];
    for (int k = 0; k < 10; ++k) acc[k] = 0.f;
    const float w = sW;
    for (int i = tid; i < p.npts; i += 256) {
        const float* pt = p.points + ((size_t)n * p.npts + i) * 3;
        const float px = pt[0], py = pt[1], pz = pt[2];
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            // A prediction bit-equal to its target must give d == 0 exactly (|.| has gradient 0 there; sgn of a rounding residue is a full-magnitude
            // gradient with arbitrary signs).  So (1) e and g are the SAME operations in the same order: written as sums of products, the compiler
            // contracted a x + b y into fma(a, x, b y) for one and fma(b, y, a x) for the other; (2) w e and w g stay two rounded products, as in the
            // reference (pm_loss.py: w * est - w * tgt), instead of fma(w, e, -(w g)), which leaves the rounding residue of w g.
            const float e = fmaf(sR[a * 3 + 2], pz, fmaf(sR[a * 3 + 1], py, sR[a * 3] * px));
            const float g = fmaf(sG[a * 3 + 2], pz, fmaf(sG[a * 3 + 1], py, sG[a * 3] * px));
            float d;
            {
#pragma clang fp contract(off)
                const float we = w * e, wg = w * g;
                d = we - wg;
            }
            acc[0] += fabsf(d);
            const float s = sgn(d) * w;
            acc[1 + a * 3 + 0] += s * px;
            acc[1 + a * 3 + 1] += s * py;
            acc[1 + a * 3 + 2] += s * pz;
        }
    }
    for (int k = 0; k < 10; ++k) {
        const float v = wave_sum(acc[k]);
        if ((tid & 63) == 0) red[k][tid >> 6] = v;
    }
    __syncthreads();
    if (tid < 10) sS[tid] = red[tid][0] + red[tid][1] + red[tid][2] + red[tid][3];
    __syncthreads();
    const float inv = 1.f / ((float)p.N * (float)p.npts);  // 3 * mean over (N, npts, 3)
    const float* gtr = p.gt_trans_ratio + n * 3;
    if (tid == 0) {
        const float lc = fabsf(in[6] - gtr[0]) + fabsf(in[7] - gtr[1]);
        if (p.loss_rows != nullptr) {   // (ABI 5) one row per RoI, added up in RoI order by gdrn_loss_finalize: no memset, no atomics, run-to-run identical
            p.loss_rows[n * 4 + 0] = sS[0] * inv;
            p.loss_rows[n * 4 + 1] = lc / (2.f * p.N);
            p.loss_rows[n * 4 + 2] = fabsf(in[8] - gtr[2]) / (float)p.N;
        } else {
            unsafeAtomicAdd(&p.losses[0], sS[0] * inv);
            unsafeAtomicAdd(&p.losses[1], lc / (2.f * p.N));
            unsafeAtomicAdd(&p.losses[2], fabsf(in[8] - gtr[2]) / (float)p.N);
        }
    }
    // dL/dfc: lane k < 9 holds d(R_ego)/d(input k) and forms its own entry; entries 9 .. fs - 1 are zero
    if (tid < p.fs) {
        const int k = tid;
        float g = 0.f;
        if (k < 9) {
            for (int ab = 0; ab < 9; ++ab) g += sS[1 + ab] * Rd[ab].d[0];
        }
        const float u1 = (k == 6) ? sgn(in[6] - gtr[0]) / (2.f * p.N) : ((k == 7) ? sgn(in[7] - gtr[1]) / (2.f * p.N) : 0.f);   // d loss_centroid / d fc[k]
        const float u2 = (k == 8) ? sgn(in[8] - gtr[2]) / (float)p.N : 0.f;                                                      // d loss_z / d fc[k]
        if (p.dfc_comb != nullptr) {
            // (ABI 5) dL/dfc directly -- the three unit gradients weighted with dL/dloss_k (p.gw: known before the forward pass in the fused train
            // step) and stored at the storage width: the combine + cast launches in front of the backward pass disappear
            bf16_t* dc = reinterpret_cast<bf16_t*>(p.dfc_comb) + (size_t)n * p.fs;
            float d = 0.f;
            if (k < 9) {
                d = p.gw[0] * (g * inv);   // (combine3's order: w0 * d0 + w1 * d1 + w2 * d2)
                if (k == 6 || k == 7) d += p.gw[1] * u1;
                if (k == 8) d += p.gw[2] * u2;
            }
            dc[k] = f2bf(d);
        } else if (p.dfc != nullptr) {
            p.dfc[((size_t)0 * p.N + n) * p.fs + k] = (k < 9) ? g * inv : 0.f;
            p.dfc[((size_t)1 * p.N + n) * p.fs + k] = u1;
            p.dfc[((size_t)2 * p.N + n) * p.fs + k] = u2;
        }
    }
}

__global__ void combine3_kernel(const float* in, const float* w, float* out, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = w[0] * in[i] + w[1] * in[n + i] + w[2] * in[2 * n + i];
}

}  // namespace

#define ST reinterpret_cast<hipStream_t>(stream)

extern "C" int gdrn_pose_loss(const gdrn_pose_params* p, void* stream) {
    if (!p || !p->fc || !p->cams || !p->centers || !p->whs || !p->ratios || !p->rot || !p->trans || p->N <= 0 || p->fs < 9 || p->fs > 256)
        return GDRN_ERR_ARG;   // (fs <= 256: one thread per entry of a dL/dfc row)
    if (p->train && (!p->losses || !p->gt_rot || !p->gt_trans_ratio || !p->points || !p->extents || p->npts <= 0))
        return GDRN_ERR_ARG;
    if (p->fc2_ws && (!p->fc2_bias || !p->f2_out || !p->w_rt || !p->b_rt || !p->fc_w || p->fc2_splits <= 0)) return GDRN_ERR_ARG;
    if (p->dfc_comb && (!p->gw || !p->train)) return GDRN_ERR_ARG;
    if (p->sym && p->Kmax < 1) return GDRN_ERR_ARG;   // (the candidate rows are indexed n * Kmax + s)
    if (p->train && p->losses && !p->loss_rows && hipMemsetAsync(p->losses, 0, 3 * sizeof(float), ST) != hipSuccess) return GDRN_ERR_LAUNCH;
    GDRN_LAUNCH(pose_loss_kernel, dim3(p->N), dim3(256), 0, ST, *p);
    GDRN_CHECK_LAUNCH();
    return GDRN_OK;
}

extern "C" int gdrn_combine3(const float* in, const float* w, float* out, int n, void* stream) {
    if (!in || !w || !out || n <= 0) return GDRN_ERR_ARG;
    GDRN_LAUNCH(combine3_kernel, dim3(cdiv(n, 256)), dim3(256), 0, ST, in, w, out, n);
    GDRN_CHECK_LAUNCH();
    return GDRN_OK;
}
