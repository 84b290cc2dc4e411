// pointwise_fwd.hip -- point-wise (kernel-size-1) convolution with the PREVIOUS layer's BatchNorm +
// ReLU applied to its input on the fly, on the exact-fp32 MFMA, gfx950.
//
//   y[b, o, p] = sum_i W[o, i] * act_i(x[b, i, p])        x (B, Cin, P), y (B, Cout, P)
//   act_i(v)   = relu?(v * sc_i + sh_i),  sc_i = invstd_i * gamma_i,  sh_i = beta_i - mean_i * sc_i
//                (the arithmetic of bn_apply_kernel, csrc/bn_act.hip), or the identity
//
// This is one [BN -> ReLU -> Conv2d 1x1] step of the reference's shared MLPs (pointnet2_batch/
// pointnet2_modules.py:86-92, pointnet2_stack/pointnet2_modules.py:33-40, voxel_pool_modules.py:41-
// 52) without ever writing the activated tensor: the layer input is the previous layer's PRE-BN
// output.  The same kernel with W read transposed and the identity activation is the data gradient
// of the layer (dX = W^T dY).
//
// As a GEMM it is skinny -- Cout, Cin <= 64, up to 15.7 M columns at config c3 -- and HBM-bound
// (4*(Cin + Cout) bytes per column against 2*Cin*Cout flops: 5..16 flop/byte); the library runs these
// shapes at 1.2-1.6 TB/s.  Here:
//   * the B operand of v_mfma_f32_32x32x2_f32 (k = channel pair, n = column) is exactly the layout
//     of a row-major (channel, column) tensor, so x goes global -> registers -> MFMA with no LDS
//     staging: lane (l, h) loads a float4 = columns 4l..4l+3 of channel 2k+h (512 contiguous bytes
//     per half-wave), and component j of the float4 feeds the j-th of four interleaved 32-column
//     sub-tiles; the D registers of the four sub-tiles then hold columns 4l..4l+3 again, so y is
//     written with 16-byte stores;
//   * W (<= 32 KB) and the per-channel (sc, sh) sit in LDS, read conflict-free as the A operand;
//   * every wave owns whole 128-column tiles and software-pipelines them: the loads of the next
//     16-channel slab are in flight while the MFMAs of the current one run.
//
// GRAD operand mode (dX of the layer in front of a fused [BatchNorm -> ReLU -> max over nsample]): the operand is that
// max-pool layer's input gradient, which is a closed form of data already in memory (bn_max_bwd_apply_kernel, csrc/bn_act.hip)
//   dx[b,c,m,s] = k_c * ((s == arg[b,c,m] ? d[b,c,m] : 0) - m0_c - (x4[b,c,m,s] - mu_c) * is_c * m1_c)
// so the kernel reads the PRE-BN tensor x4 (B, C, M, ns) where it would read a dense dx, plus one arg byte and one d float per
// float4 (ns % 4 == 0: the four columns of a float4 lie in one group), and forms dx while feeding the MFMA, in the operation
// order of bn_max_bwd_apply_kernel: the products are bit for bit those of the dense route, and dx is never written or re-read.
//
// MAXPOOL epilogue (inference: the layer's output (B, Cout, M, ns) is followed by a running-statistics BatchNorm [+ ReLU] and the
// max over ns): at tile finish a lane holds four consecutive columns of a row, so with ns % 4 == 0 and 128 % ns == 0 a group is
// the four components of ns / 4 neighbouring lanes of one half-wave.  The epilogue forms relu?(fmaf(acc, scale_o, shift_o)),
// takes the NaN-propagating max over the components and over the group's lanes (xor shuffles inside the half-wave) and the
// group's first lane stores pooled[b, o, p / ns]: the (B, Cout, M, ns) tensor is never written.
#include <type_traits>

#include "common.hpp"
#include "payload.hpp"

namespace mgar {

constexpr int PF_COLS = 128;  // columns per wave tile
// channels per slab (2 per MFMA k-step): 16, or 8 for the 64-output-channel instance so that its 128 accumulator
// registers + two slab buffers stay under 256 VGPRs (2 waves per SIMD instead of 1)
// (4 for its GRAD instance, whose slabs also carry the groups' (d, arg): 8 spilled)
template <int OB, bool GRAD = false> struct PfSlab { static constexpr int KC = OB == 1 ? 16 : (GRAD ? 4 : 8); };

struct PfPool {                 // MAXPOOL epilogue: y = pooled (B, Cout, P / ns)
    const float *scale, *shift; // (Cout) eval-mode BatchNorm of the layer's output as an affine map
    int ns, relu;
};

struct PfGrad {                 // GRAD operand mode: x = x4 (B, Cin, M, ns), P = M * ns
    const unsigned char *arg;   // (B, Cin, M) arg-max slot of every group
    const float *d;             // (B, Cin, M) pooled gradient, already zeroed where the ReLU cut it (bn_max_bwd_partial_kernel)
    const float *coef;          // (Cin, 2) = {m0, m1} of the BatchNorm backward (bn_bwd_finalize_kernel)
    int M, ns;
};

template <typename T>
struct PfArgs {
    const T *x;                                 // payload: float or bf16_t (fp32 accumulation on the fp32 MFMA either way)
    const float *w;
    const float *mean, *invstd, *gamma, *beta;  // input activation (mean == nullptr: identity)
    T *y;
    int B, Cin, Cout, P;
    int w_rs, w_cs;  // W[o, i] = w[o * w_rs + i * w_cs]
    int relu;
    // optional (P % 128 == 0): per (output channel, 128-column tile) the tile's (mean, M2) of y, in the layout of
    // bn_partial_kernel with chunk = 128 -- stats[(o * ntiles + tile) * 2 + {0, 1}], tile = b * (P / 128) + tile of the
    // sample -- so that the BatchNorm that follows needs no pass over y for its statistics (csrc/bn_act.hip, bn_finalize_kernel)
    float *stats;
    PfGrad g;        // GRAD instances only (mean / invstd / gamma are then those of the max-pool layer's BatchNorm)
    PfPool mp;       // MAXPOOL instances only
};

// one slab of operand registers; the GRAD instances carry the group's (d, arg) next to every float4 and the float4's first slot
template <int KS, bool GRAD> struct PfBuf { float4 v[KS]; };
template <int KS> struct PfBuf<KS, true> { float4 v[KS]; float d[KS]; int a[KS]; int s0; };

template <int OB, typename T, bool STATS = false, bool GRAD = false, bool MAXPOOL = false>
__global__ __launch_bounds__(256, 2) void pointwise_fwd_kernel(PfArgs<T> a) {
    constexpr int PF_KC = PfSlab<OB, GRAD>::KC, KS = PF_KC / 2;
    constexpr int WLD = OB == 1 ? 32 : 96;  // LDS row stride of W: the two half-waves hit disjoint banks
    extern __shared__ float lds[];          // [nkc*16][WLD] weights, then [nkc*16][4] (sc, sh, mu, -); GRAD: (k, m0, mu, is), then [nkc*16] m1
                                            // MAXPOOL: then [OB*32][2] (scale, shift) of the output rows
    const int nkc = (a.Cin + PF_KC - 1) / PF_KC;
    float *wl = lds;
    float *act = lds + (size_t)nkc * PF_KC * WLD;
    float *gm1 = act + (size_t)nkc * PF_KC * 4;
    if constexpr (MAXPOOL) {
        for (int o = threadIdx.x; o < OB * 32; o += 256)
            *reinterpret_cast<float2 *>(gm1 + 2 * o) = o < a.Cout ? make_float2(a.mp.scale[o], a.mp.shift[o]) : make_float2(0.f, 0.f);
    }
    for (int e = threadIdx.x; e < nkc * PF_KC * WLD; e += 256) {
        const int ch = e / WLD, o = e - ch * WLD;
        wl[e] = (ch < a.Cin && o < a.Cout) ? a.w[(size_t)o * a.w_rs + (size_t)ch * a.w_cs] : 0.f;
    }
    if constexpr (GRAD) {
        for (int ch = threadIdx.x; ch < nkc * PF_KC; ch += 256) {
            float k = 0.f, m0 = 0.f, mu = 0.f, is = 0.f, m1 = 0.f;   // padding channels: the operand comes out as zero
            if (ch < a.Cin) {
                mu = a.mean[ch];
                is = a.invstd[ch];
                k = (a.gamma ? a.gamma[ch] : 1.f) * is;
                m0 = a.g.coef[2 * ch];
                m1 = a.g.coef[2 * ch + 1];
            }
            *reinterpret_cast<float4 *>(act + 4 * ch) = make_float4(k, m0, mu, is);
            gm1[ch] = m1;
        }
    } else
    for (int ch = threadIdx.x; ch < nkc * PF_KC; ch += 256) {
        float sc = 1.f, sh = 0.f, mu = 0.f;   // act(v) = (v - mu) * sc + sh: the arithmetic of bn_apply_kernel
        if (a.mean && ch < a.Cin) {
            sc = a.invstd[ch] * (a.gamma ? a.gamma[ch] : 1.f);
            sh = a.beta ? a.beta[ch] : 0.f;
            mu = a.mean[ch];
        }
        *reinterpret_cast<float4 *>(act + 4 * ch) = make_float4(sc, sh, mu, 0.f);
    }
    __syncthreads();

    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int l = lane & 31, h = lane >> 5;
    const int tiles_per_b = (a.P + PF_COLS - 1) / PF_COLS;
    const long long ntiles = (long long)a.B * tiles_per_b;
    const long long wave_id = (long long)blockIdx.x * 4 + wave, nwaves = (long long)gridDim.x * 4;
    if (wave_id >= ntiles) return;
    const long long my_tiles = (ntiles - wave_id + nwaves - 1) / nwaves;
    const long long steps = my_tiles * nkc;
    const bool has_act = a.mean != nullptr, relu = a.relu != 0;

    f32x16 acc[OB][4];
#pragma unroll
    for (int ob = 0; ob < OB; ++ob)
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[ob][j][r] = 0.f;

    // slab loads of step s (tile s / nkc of this wave, channel slab s % nkc)
    auto issue = [&](long long s, PfBuf<KS, GRAD> &sl) {
        float4 (&buf)[KS] = sl.v;
        const long long t = wave_id + (s / nkc) * nwaves;
        const int kc = (int)(s % nkc);
        const int b = (int)(t / tiles_per_b);
        const int p = (int)(t - (long long)b * tiles_per_b) * PF_COLS + 4 * l;
        const T *src = a.x + ((size_t)b * a.Cin + kc * PF_KC + h) * a.P + p;
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
            const int ch = kc * PF_KC + 2 * ks + h;
            buf[ks] = (ch < a.Cin && p < a.P) ? Payload<T>::ld4(src + (size_t)2 * ks * a.P)
                                              : make_float4(0.f, 0.f, 0.f, 0.f);
        }
        if constexpr (GRAD) {   // one 32-bit division per slab: every float4 of the slab lies in group m of its channel
            const int m = (int)((unsigned)p / (unsigned)a.g.ns);
            sl.s0 = p - m * a.g.ns;
            const size_t go = ((size_t)b * a.Cin + kc * PF_KC + h) * a.g.M + m;
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) {
                const bool ok = kc * PF_KC + 2 * ks + h < a.Cin && p < a.P;
                sl.d[ks] = ok ? a.g.d[go + (size_t)2 * ks * a.g.M] : 0.f;
                sl.a[ks] = ok ? (int)a.g.arg[go + (size_t)2 * ks * a.g.M] : 0;
            }
        }
    };
    auto compute = [&](long long s, PfBuf<KS, GRAD> &sl) {
        float4 (&buf)[KS] = sl.v;
        const int kc = (int)(s % nkc);
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
            const int ch = kc * PF_KC + 2 * ks + h;
            float4 v = buf[ks];
            if constexpr (GRAD) {   // bn_max_bwd_apply_kernel's expression, term for term (columns past P are never stored)
                const float4 ac = *reinterpret_cast<const float4 *>(act + 4 * ch);
                const float k = ac.x, m0 = ac.y, mu = ac.z, is = ac.w, m1 = gm1[ch];
                const float d = sl.d[ks];
                const int sa = sl.a[ks] - sl.s0;   // the arg-max slot relative to the float4's first column
                v.x = k * ((sa == 0 ? d : 0.f) - m0 - (v.x - mu) * is * m1);
                v.y = k * ((sa == 1 ? d : 0.f) - m0 - (v.y - mu) * is * m1);
                v.z = k * ((sa == 2 ? d : 0.f) - m0 - (v.z - mu) * is * m1);
                v.w = k * ((sa == 3 ? d : 0.f) - m0 - (v.w - mu) * is * m1);
            } else
            if (has_act) {
                const float4 ac = *reinterpret_cast<const float4 *>(act + 4 * ch);
                const float sc = ac.x, sh = ac.y, mu = ac.z;
                v.x = (v.x - mu) * sc + sh; v.y = (v.y - mu) * sc + sh; v.z = (v.z - mu) * sc + sh; v.w = (v.w - mu) * sc + sh;
                if (relu) { v.x = relu_nan(v.x); v.y = relu_nan(v.y); v.z = relu_nan(v.z); v.w = relu_nan(v.w); }
                if (ch >= a.Cin) v = make_float4(0.f, 0.f, 0.f, 0.f);   // padding channels stay zero (W is zero there too)
            }
#pragma unroll
            for (int ob = 0; ob < OB; ++ob) {
                const float wa = wl[ch * WLD + ob * 32 + l];
                acc[ob][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(wa, v.x, acc[ob][0], 0, 0, 0);
                acc[ob][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(wa, v.y, acc[ob][1], 0, 0, 0);
                acc[ob][2] = __builtin_amdgcn_mfma_f32_32x32x2f32(wa, v.z, acc[ob][2], 0, 0, 0);
                acc[ob][3] = __builtin_amdgcn_mfma_f32_32x32x2f32(wa, v.w, acc[ob][3], 0, 0, 0);
            }
        }
        if (kc == nkc - 1) {  // tile finished: D[row = (r&3) + 8*(r>>2) + 4*h][col = l] of sub-tile j = column 4l + j
            const long long t = wave_id + (s / nkc) * nwaves;
            const int b = (int)(t / tiles_per_b);
            const int p = (int)(t - (long long)b * tiles_per_b) * PF_COLS + 4 * l;
            if constexpr (MAXPOOL) {   // relu?(fmaf(acc, scale, shift)), max over the group, one store per group and row
                const int gl = a.mp.ns >> 2;                                  // lanes per group: 1, 2, 4, .., 32
                const int m = (int)((unsigned)p / (unsigned)a.mp.ns), M = a.P / a.mp.ns;
                const bool lead = (l & (gl - 1)) == 0 && p < a.P, orelu = a.mp.relu != 0;
#pragma unroll
                for (int ob = 0; ob < OB; ++ob)
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const int o = ob * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
                        const float2 ss = *reinterpret_cast<const float2 *>(gm1 + 2 * o);
                        float v0 = fmaf(acc[ob][0][r], ss.x, ss.y), v1 = fmaf(acc[ob][1][r], ss.x, ss.y);
                        float v2 = fmaf(acc[ob][2][r], ss.x, ss.y), v3 = fmaf(acc[ob][3][r], ss.x, ss.y);
                        if (orelu) { v0 = relu_nan(v0); v1 = relu_nan(v1); v2 = relu_nan(v2); v3 = relu_nan(v3); }
                        float best = max_nan(max_nan(max_nan(v0, v1), v2), v3);
#pragma unroll
                        for (int d = 1; d < 32; d <<= 1)
                            if (d < gl) best = max_nan(best, __shfl_xor(best, d, 32));
                        if (lead && o < a.Cout) Payload<T>::st(a.y + ((size_t)b * a.Cout + o) * M + m, best);
                        acc[ob][0][r] = 0.f; acc[ob][1][r] = 0.f; acc[ob][2][r] = 0.f; acc[ob][3][r] = 0.f;
                    }
                return;
            }
            if (STATS) {   // the 128 columns of a channel live in the 32 lanes of one half-wave x 4 sub-tiles: exact two-pass
#pragma unroll
                for (int ob = 0; ob < OB; ++ob)
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const float v0 = acc[ob][0][r], v1 = acc[ob][1][r], v2 = acc[ob][2][r], v3 = acc[ob][3][r];
                        float sum = (v0 + v1) + (v2 + v3);
#pragma unroll
                        for (int d = 1; d < 32; d <<= 1) sum += __shfl_xor(sum, d, 32);
                        const float mean = sum * (1.f / PF_COLS);
                        const float d0 = v0 - mean, d1 = v1 - mean, d2 = v2 - mean, d3 = v3 - mean;
                        float m2 = (d0 * d0 + d1 * d1) + (d2 * d2 + d3 * d3);
#pragma unroll
                        for (int d = 1; d < 32; d <<= 1) m2 += __shfl_xor(m2, d, 32);
                        const int o = ob * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
                        if (l == 0 && o < a.Cout)
                            *reinterpret_cast<float2 *>(a.stats + ((size_t)o * ntiles + t) * 2) = make_float2(mean, m2);
                    }
            }
#pragma unroll
            for (int ob = 0; ob < OB; ++ob)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int o = ob * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
                    if (o < a.Cout && p < a.P)
                        Payload<T>::st4(a.y + ((size_t)b * a.Cout + o) * a.P + p,
                                        make_float4(acc[ob][0][r], acc[ob][1][r], acc[ob][2][r], acc[ob][3][r]));
                    acc[ob][0][r] = 0.f; acc[ob][1][r] = 0.f; acc[ob][2][r] = 0.f; acc[ob][3][r] = 0.f;
                }
        }
    };

    PfBuf<KS, GRAD> buf0, buf1;
    issue(0, buf0);
    for (long long s = 0; s < steps; s += 2) {
        if (s + 1 < steps) issue(s + 1, buf1);
        compute(s, buf0);
        if (s + 1 < steps) {
            if (s + 2 < steps) issue(s + 2, buf0);
            compute(s + 1, buf1);
        }
    }
}

template <int OB, typename T, bool STATS = false, bool GRAD = false, bool MAXPOOL = false>
static void launch_pf(const PfArgs<T> &a, hipStream_t st) {
    constexpr int WLD = OB == 1 ? 32 : 96, PF_KC = PfSlab<OB, GRAD>::KC;
    const int nkc = (a.Cin + PF_KC - 1) / PF_KC;
    const int lds = (nkc * PF_KC * (WLD + 4 + (GRAD ? 1 : 0)) + (MAXPOOL ? OB * 64 : 0)) * (int)sizeof(float);
    static int attr_lds = 0;
    if (lds > 65536 && lds > attr_lds) {
        (void)hipFuncSetAttribute((const void *)pointwise_fwd_kernel<OB, T, STATS, GRAD, MAXPOOL>,
                                  hipFuncAttributeMaxDynamicSharedMemorySize, lds);
        attr_lds = lds;
    }
    const long long ntiles = (long long)a.B * ((a.P + PF_COLS - 1) / PF_COLS);
    long long wgs = (ntiles + 3) / 4;
    if (wgs > 2048) wgs = 2048;   // 8 workgroups per CU; waves stride over the tiles
    hipLaunchKernelGGL((pointwise_fwd_kernel<OB, T, STATS, GRAD, MAXPOOL>), dim3((unsigned)wgs), dim3(256), lds, st, a);
}

}  // namespace mgar

using namespace mgar;

template <typename T>
static int pointwise_conv_fwd_impl(const T *x, int B, int Cin, int P, const float *w, int w_row_stride, int w_col_stride, int Cout,
                                   const float *in_mean, const float *in_invstd, const float *in_gamma, const float *in_beta,
                                   int in_relu, T *y, void *stream, float *out_stats = nullptr) {
    MGAR_REQUIRE(B >= 0 && Cin >= 0 && Cout >= 0 && P >= 0, "pointwise_conv_fwd: negative size");
    if ((long long)B * P == 0 || Cout == 0) return MGAR_OK;
    MGAR_REQUIRE(x && w && y, "pointwise_conv_fwd: null pointer");
    MGAR_REQUIRE(in_mean == nullptr || in_invstd != nullptr, "pointwise_conv_fwd: in_mean without in_invstd");
    if (Cout > 64 || Cin > 256 || Cin == 0 || (P & 3) != 0) {
        set_error("pointwise_conv_fwd: needs 1 <= Cin <= 256, Cout <= 64 and P % 4 == 0 (use the library GEMM otherwise)");
        return MGAR_EUNSUPPORTED;
    }
    MGAR_REQUIRE(out_stats == nullptr || P % PF_COLS == 0, "pointwise_conv_fwd: output statistics need P % 128 == 0");
    PfArgs<T> a{x, w, in_mean, in_invstd, in_gamma, in_beta, y, B, Cin, Cout, P, w_row_stride, w_col_stride, in_relu, out_stats};
    hipStream_t st = (hipStream_t)stream;
    KtScope kt(KT_POINTWISE_FWD, st, (double)sizeof(T) * B * P * (Cin + Cout), 2.0 * (double)B * P * Cin * Cout);
    if (out_stats) {   // Cout <= 32 (checked by the entry point): the 64-channel instance has no registers left for it
        if constexpr (std::is_same<T, float>::value) launch_pf<1, float, true>(a, st);
    } else if (Cout <= 32) launch_pf<1, T>(a, st);
    else launch_pf<2, T>(a, st);
    return check_launch("pointwise_conv_fwd: launch failed");
}

MGAR_API int mgar_pointwise_conv_fwd(const float *x, int B, int Cin, int P, const float *w, int w_row_stride, int w_col_stride, int Cout,
                                     const float *in_mean, const float *in_invstd, const float *in_gamma, const float *in_beta,
                                     int in_relu, float *y, void *stream) {
    return pointwise_conv_fwd_impl<float>(x, B, Cin, P, w, w_row_stride, w_col_stride, Cout, in_mean, in_invstd, in_gamma, in_beta,
                                          in_relu, y, stream);
}
// bf16 payload (x, y address bf16 elements; W and the BatchNorm vectors stay fp32)
MGAR_API int mgar_pointwise_conv_fwd_bf16(const void *x, int B, int Cin, int P, const float *w, int w_row_stride, int w_col_stride,
                                          int Cout, const float *in_mean, const float *in_invstd, const float *in_gamma,
                                          const float *in_beta, int in_relu, void *y, void *stream) {
    return pointwise_conv_fwd_impl<bf16_t>((const bf16_t *)x, B, Cin, P, w, w_row_stride, w_col_stride, Cout, in_mean, in_invstd,
                                           in_gamma, in_beta, in_relu, (bf16_t *)y, stream);
}

// pointwise_conv_fwd that also leaves the BatchNorm statistics partials of its OUTPUT: out_stats (Cout, B * P / 128, 2) floats =
// per (channel, 128-column tile) the tile's mean and sum of squared deviations, the chunk format mgar_bn_stats_from_partials
// finalizes (chunk = 128).  P % 128 == 0, Cout <= 32.  fp32.  Saves the BatchNorm's own pass over y (4 * B * Cout * P bytes).
MGAR_API int mgar_pointwise_conv_fwd_stats(const float *x, int B, int Cin, int P, const float *w, int w_row_stride, int w_col_stride,
                                           int Cout, const float *in_mean, const float *in_invstd, const float *in_gamma,
                                           const float *in_beta, int in_relu, float *y, float *out_stats, void *stream) {
    MGAR_REQUIRE(out_stats, "pointwise_conv_fwd_stats: null pointer");
    if (Cout > 32) {
        set_error("pointwise_conv_fwd_stats: Cout <= 32 (run mgar_pointwise_conv_fwd and the BatchNorm's own statistics pass)");
        return MGAR_EUNSUPPORTED;
    }
    return pointwise_conv_fwd_impl<float>(x, B, Cin, P, w, w_row_stride, w_col_stride, Cout, in_mean, in_invstd, in_gamma, in_beta,
                                          in_relu, y, stream, out_stats);
}

// dX of the layer in front of a fused [BatchNorm -> ReLU -> max over nsample], with that max-pool layer's input gradient formed
// in the operand prologue instead of read from memory (GRAD mode above):
//   y[b, o, p] = sum_i w[o * w_row_stride + i * w_col_stride] * dx4[b, i, p]
//   dx4[b,i,m,s] = k_i * ((s == arg[b,i,m] ? dmask[b,i,m] : 0) - coef[2i] - (x4[b,i,m,s] - mean_i) * invstd_i * coef[2i+1]),  k_i = gamma_i invstd_i
// x4 (B, Cin, M, nsample) is the max-pool layer's PRE-BN input; coef and dmask come from mgar_bn_act_maxpool_bwd_reduce.
// Cin, Cout <= 64, nsample % 4 == 0 (MGAR_EUNSUPPORTED otherwise).  fp32.
MGAR_API int mgar_pointwise_conv_fwd_maxgrad(const float *x4, int B, int Cin, int M, int nsample, const float *w, int w_row_stride,
                                             int w_col_stride, int Cout, const float *mean, const float *invstd, const float *gamma,
                                             const float *coef, const unsigned char *arg, const float *dmask, float *y, void *stream) {
    MGAR_REQUIRE(B >= 0 && Cin >= 0 && Cout >= 0 && M >= 0 && nsample >= 1 && nsample <= 255, "pointwise_conv_fwd_maxgrad: bad sizes");
    MGAR_REQUIRE((long long)M * nsample <= 2147483647LL - PF_COLS, "pointwise_conv_fwd_maxgrad: M * nsample too large");
    if ((long long)B * M == 0 || Cout == 0) return MGAR_OK;
    MGAR_REQUIRE(x4 && w && y && mean && invstd && coef && arg && dmask, "pointwise_conv_fwd_maxgrad: null pointer");
    if (Cout > 64 || Cin > 64 || Cin == 0 || (nsample & 3) != 0) {
        set_error("pointwise_conv_fwd_maxgrad: needs 1 <= Cin <= 64, Cout <= 64 and nsample % 4 == 0 (write the gradient with "
                  "mgar_bn_act_maxpool_bwd otherwise)");
        return MGAR_EUNSUPPORTED;
    }
    const int P = M * nsample;
    PfArgs<float> a{x4, w, mean, invstd, gamma, nullptr, y, B, Cin, Cout, P, w_row_stride, w_col_stride, 0, nullptr, {arg, dmask, coef, M, nsample}};
    hipStream_t st = (hipStream_t)stream;
    KtScope kt(KT_POINTWISE_FWD, st, 4.0 * (double)B * P * (Cin + Cout) + 5.0 * (double)B * Cin * M, 2.0 * (double)B * P * Cin * Cout);
    if (Cout <= 32) launch_pf<1, float, false, true>(a, st);
    else launch_pf<2, float, false, true>(a, st);
    return check_launch("pointwise_conv_fwd_maxgrad: launch failed");
}

// Inference tail of a shared MLP: [BN -> ReLU ->] conv 1x1 -> running-statistics BatchNorm [-> ReLU] -> max over nsample in one
// launch (MAXPOOL epilogue above); the conv's output (B, Cout, M, nsample) is never written:
//   pooled[b, o, m] = max_s relu?(fmaf(sum_i w[o, i] act_i(x[b, i, m, s]), out_scale[o], out_shift[o]))
// NaN-propagating max and ReLU (csrc/common.hpp); a bf16 pooled value is rounded once, after the max.
template <typename T>
static int pointwise_conv_maxpool_eval_impl(const T *x, int B, int Cin, int M, int nsample, const float *w, int w_row_stride,
                                            int w_col_stride, int Cout, const float *in_mean, const float *in_invstd,
                                            const float *in_gamma, const float *in_beta, int in_relu, const float *out_scale,
                                            const float *out_shift, int out_relu, T *pooled, void *stream) {
    MGAR_REQUIRE(B >= 0 && Cin >= 0 && Cout >= 0 && M >= 0 && nsample >= 1, "pointwise_conv_maxpool_eval: bad sizes");
    MGAR_REQUIRE((long long)M * nsample <= 2147483647LL - PF_COLS, "pointwise_conv_maxpool_eval: M * nsample too large");
    if ((long long)B * M == 0 || Cout == 0) return MGAR_OK;
    MGAR_REQUIRE(x && w && pooled && out_scale && out_shift, "pointwise_conv_maxpool_eval: null pointer");
    MGAR_REQUIRE(in_mean == nullptr || in_invstd != nullptr, "pointwise_conv_maxpool_eval: in_mean without in_invstd");
    if (Cout > 64 || Cin > 256 || Cin == 0 || (nsample & 3) != 0 || nsample > PF_COLS || PF_COLS % nsample != 0) {
        set_error("pointwise_conv_maxpool_eval: needs 1 <= Cin <= 256, Cout <= 64 and nsample in {4, 8, 16, 32, 64, 128} (run "
                  "mgar_pointwise_conv_fwd and mgar_bn_act_maxpool_fwd otherwise)");
        return MGAR_EUNSUPPORTED;
    }
    const int P = M * nsample;
    PfArgs<T> a{x, w, in_mean, in_invstd, in_gamma, in_beta, pooled, B, Cin, Cout, P, w_row_stride, w_col_stride, in_relu, nullptr,
                {}, {out_scale, out_shift, nsample, out_relu}};
    hipStream_t st = (hipStream_t)stream;
    KtScope kt(KT_POINTWISE_FWD, st, (double)sizeof(T) * B * ((double)P * Cin + (double)M * Cout), 2.0 * (double)B * P * Cin * Cout);
    if (Cout <= 32) launch_pf<1, T, false, false, true>(a, st);
    else launch_pf<2, T, false, false, true>(a, st);
    return check_launch("pointwise_conv_maxpool_eval: launch failed");
}

MGAR_API int mgar_pointwise_conv_maxpool_eval_fwd(const float *x, int B, int Cin, int M, int nsample, const float *w, int w_row_stride,
                                                  int w_col_stride, int Cout, const float *in_mean, const float *in_invstd,
                                                  const float *in_gamma, const float *in_beta, int in_relu, const float *out_scale,
                                                  const float *out_shift, int out_relu, float *pooled, void *stream) {
    return pointwise_conv_maxpool_eval_impl<float>(x, B, Cin, M, nsample, w, w_row_stride, w_col_stride, Cout, in_mean, in_invstd,
                                                   in_gamma, in_beta, in_relu, out_scale, out_shift, out_relu, pooled, stream);
}
// bf16 payload: x and pooled address bf16 elements (called by name: no `_bf16` payload twin, see include/mgar_ops.h)
MGAR_API int mgar_pointwise_conv_maxpool_eval_bf16_fwd(const void *x, int B, int Cin, int M, int nsample, const float *w,
                                                       int w_row_stride, int w_col_stride, int Cout, const float *in_mean,
                                                       const float *in_invstd, const float *in_gamma, const float *in_beta,
                                                       int in_relu, const float *out_scale, const float *out_shift, int out_relu,
                                                       void *pooled, void *stream) {
    return pointwise_conv_maxpool_eval_impl<bf16_t>((const bf16_t *)x, B, Cin, M, nsample, w, w_row_stride, w_col_stride, Cout, in_mean,
                                                    in_invstd, in_gamma, in_beta, in_relu, out_scale, out_shift, out_relu,
                                                    (bf16_t *)pooled, stream);
}
