// pointwise_bf16.hip -- forward of the point-wise (kernel-size-1) convolution of the shared MLPs for bf16 payloads, with the
// previous layer's BatchNorm + ReLU applied to its input on the fly, on the bf16 MFMA of gfx950 (v_mfma_f32_32x32x16_bf16).
// The bf16 forward configurations run it where csrc/pointwise_fwd.hip would widen every element and multiply on the fp32 MFMA.
//
//   a[b,i,p] = bf16( act_i(float(x[b,i,p])) )     act_i(v) = relu_nan?(((v - mean_i) * sc_i) + beta_i), sc_i = invstd_i * gamma_i:
//                                                 the prologue of pointwise_fwd_kernel, every operation rounded to fp32 on its own;
//                                                 identity prologue: a = x, nothing is rounded
//   w~[o,i]  = bf16( w[o * w_rs + i * w_cs] )     fp32 master weight, round to nearest even
//   y[b,o,p] = bf16( sum_i w~[o,i] * a[b,i,p] )   the products are exact in the fp32 accumulator (16-channel k-steps ascending),
//                                                 rounded ONCE on store
// -- the contract of csrc/conv3d_bf16.hip, csrc/stem_conv.hip and csrc/sparse_conv_bf16.hip.  A NaN stays a NaN through the
// roundings (v_cvt_pk_bf16_f32) and through the ReLU (relu_nan, csrc/common.hpp).
//
// pointwise_fwd_kernel's "no LDS for x" layout carried over to the k = 16 instruction: W is the A operand, x the B operand.
//   * lane (l = lane & 31, h = lane >> 5) holds B[k = 8 h + j][column l], j = 0 .. 7.  It issues eight 8-byte loads, load j =
//     x[channel 16 s + 8 h + j][columns 4 l .. 4 l + 3] (256 contiguous bytes per half-wave and channel); element i of load j is
//     fragment element j of the i-th of four interleaved 32-column sub-tiles.  The prologue constants are per load (one channel);
//     the fragments are packed in registers (v_cvt_pk_bf16_f32, or 16-bit selects for the identity prologue);
//   * the D registers of the four sub-tiles hold columns 4 l .. 4 l + 3 of a row again: one 8-byte store per row;
//   * every workgroup rounds W to bf16 into LDS in fragment order -- [k-step][32-row block][lane] 16-byte vectors, a wave's
//     ds_read_b128 covers 1 KB contiguous -- next to the per-channel (sc, beta, mean): no pack kernel, no workspace;
//   * every wave owns whole 128-column tiles and software-pipelines them: the loads of the next k-step are in flight while the
//     MFMAs of the current one run.
// Channels beyond Cin are zero in BOTH operands: W~ is stored as zero there, x is not loaded (zero registers) and the padding
// entries of the prologue table are (1, 0, 0), which map that zero to zero.  Columns beyond P are never stored.
// No atomics, no cross-column state: a column's bits depend on that column of x, on W and on the BatchNorm vectors only -- not on
// B, on P, on the tile the column falls in or on the grid.
#include "common.hpp"
#include "payload.hpp"

namespace mgar {

constexpr int PB_COLS = 128;   // columns per wave tile: 4 interleaved sub-tiles of 32
constexpr int PB_KC = 16;      // channels per k-step (one MFMA per sub-tile and row block)

struct PbArgs {
    const uint16_t *x;                          // (B, Cin, P) bf16
    const float *w;
    const float *mean, *invstd, *gamma, *beta;  // ACT instances only
    uint16_t *y;                                // (B, Cout, P) bf16
    int B, Cin, Cout, P;
    int w_rs, w_cs;                             // W[o, i] = w[o * w_rs + i * w_cs]
    int relu;
};

// OB: 32-row blocks of the output (Cout <= 32 OB); ACT: the BatchNorm [+ ReLU] prologue.  grid: waves stride over the tiles.
template <int OB, bool ACT>
__global__ __launch_bounds__(256, 2) void pointwise_bf16_kernel(PbArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char pb_lds[];
    const int nks = (a.Cin + PB_KC - 1) / PB_KC;
    u32x4 *wl = reinterpret_cast<u32x4 *>(pb_lds);                                    // [nks][OB][64 lanes]
    float4 *act = reinterpret_cast<float4 *>(pb_lds + (size_t)nks * OB * 1024);       // [nks * 16] (sc, beta, mean, -)
    for (int e = threadIdx.x; e < nks * OB * 64; e += 256) {
        // vector e = A fragment of lane (l, h) for k-step s, row block ob: W~[32 ob + l][16 s + 8 h + j], j = 0 .. 7
        const int ln = e & 63, ob = (e >> 6) % OB, s = (e >> 6) / OB;
        const int o = ob * 32 + (ln & 31), ch0 = s * PB_KC + 8 * (ln >> 5);
        float wv[8];
#pragma unroll
        for (int j = 0; j < 8; ++j)
            wv[j] = (o < a.Cout && ch0 + j < a.Cin) ? a.w[(size_t)o * a.w_rs + (size_t)(ch0 + j) * a.w_cs] : 0.f;
        wl[e] = u32x4{pack_bf16x2(wv[0], wv[1]), pack_bf16x2(wv[2], wv[3]), pack_bf16x2(wv[4], wv[5]), pack_bf16x2(wv[6], wv[7])};
    }
    if constexpr (ACT) {
        for (int ch = threadIdx.x; ch < nks * PB_KC; ch += 256)
            act[ch] = bn_prologue_entry(ch, a.Cin, a.mean, a.invstd, a.gamma, a.beta);
    }
    __syncthreads();

    // the wave's position is wave-uniform: pinned to scalar registers, so tile, sample and k-step arithmetic runs on the scalar unit
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int l = lane & 31, h = lane >> 5;
    const int tiles_per_b = (a.P + PB_COLS - 1) / PB_COLS;
    const int ntiles = a.B * tiles_per_b;                       // <= 2^30 (checked by the entry point)
    const int wave_id = (int)blockIdx.x * 4 + wave, nwaves = (int)gridDim.x * 4;
    if (wave_id >= ntiles) return;
    const bool relu = a.relu != 0;
    const size_t lane_off = (size_t)8 * h * a.P + 4 * l;        // elements from (channel 16 s, first column of the tile)

    f32x16 acc[OB][4];
#pragma unroll
    for (int ob = 0; ob < OB; ++ob)
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[ob][i][r] = 0.f;

    struct Pos { int t, ks; };   // tile (b * tiles_per_b + tile of the sample), k-step
    auto advance = [&](Pos &q) {
        if (++q.ks == nks) { q.ks = 0; q.t += nwaves; }
    };
    // the eight loads of one step
    auto issue = [&](const Pos q, uint2 (&buf)[8]) {
        const int b = q.t / tiles_per_b;
        const int p0 = (q.t - b * tiles_per_b) * PB_COLS;
        // wave-uniform base + the lane's offset, then a wave-uniform step per load: nothing per (lane, load) is loop-invariant,
        // so the compiler keeps no table of 64-bit addresses in registers
        const uint16_t *src = a.x + ((size_t)b * a.Cin + q.ks * PB_KC) * a.P + p0 + lane_off;
        const int ch0 = q.ks * PB_KC + 8 * h;
        const bool pok = p0 + 4 * l < a.P;
#pragma unroll
        for (int j = 0; j < 8; ++j)
            buf[j] = (pok && ch0 + j < a.Cin) ? *reinterpret_cast<const uint2 *>(src + (size_t)j * a.P) : make_uint2(0u, 0u);
    };
    auto compute = [&](const Pos q, uint2 (&buf)[8]) {
        const int ks = q.ks;
        u32x4 bf[4];   // B fragments of the four sub-tiles: dword q = fragment elements 2 q (low half), 2 q + 1 (high half)
        if constexpr (ACT) {
            const float4 *ac = act + ks * PB_KC + 8 * h;
#pragma unroll
            for (int d = 0; d < 4; ++d) {
                float v[2][4];
#pragma unroll
                for (int e = 0; e < 2; ++e) {
                    const uint2 u = buf[2 * d + e];
                    const float4 c = ac[2 * d + e];
                    const float sc = c.x, sh = c.y, mu = c.z;
                    v[e][0] = (bf16_lo(u.x) - mu) * sc + sh; v[e][1] = (bf16_hi(u.x) - mu) * sc + sh;
                    v[e][2] = (bf16_lo(u.y) - mu) * sc + sh; v[e][3] = (bf16_hi(u.y) - mu) * sc + sh;
                    if (relu) {
#pragma unroll
                        for (int i = 0; i < 4; ++i) v[e][i] = relu_nan(v[e][i]);
                    }
                }
#pragma unroll
                for (int i = 0; i < 4; ++i) bf[i][d] = pack_bf16x2(v[0][i], v[1][i]);
            }
        } else {
            pack_b_fragments(buf, bf);
        }
#pragma unroll
        for (int ob = 0; ob < OB; ++ob) {
            const bf16x8 wa = __builtin_bit_cast(bf16x8, wl[(ks * OB + ob) * 64 + lane]);
#pragma unroll
            for (int i = 0; i < 4; ++i)
                acc[ob][i] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wa, __builtin_bit_cast(bf16x8, bf[i]), acc[ob][i], 0, 0, 0);
        }
        if (ks == nks - 1) {  // tile finished: D[row = (r & 3) + 8 (r >> 2) + 4 h][col = l] of sub-tile i = column 4 l + i
            const int b = q.t / tiles_per_b;
            const int p = (q.t - b * tiles_per_b) * PB_COLS + 4 * l;
            uint16_t *dst = a.y + ((size_t)b * a.Cout + 4 * h) * a.P + p;   // the lane's row 4 h; the rest of a row index is uniform
#pragma unroll
            for (int ob = 0; ob < OB; ++ob)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int ou = ob * 32 + (r & 3) + 8 * (r >> 2);
                    if (ou + 4 * h < a.Cout && p < a.P)
                        *reinterpret_cast<uint2 *>(dst + (size_t)ou * a.P) =
                            make_uint2(pack_bf16x2(acc[ob][0][r], acc[ob][1][r]), pack_bf16x2(acc[ob][2][r], acc[ob][3][r]));
                    acc[ob][0][r] = 0.f; acc[ob][1][r] = 0.f; acc[ob][2][r] = 0.f; acc[ob][3][r] = 0.f;
                }
        }
    };

    uint2 buf0[8], buf1[8];
    Pos ip{wave_id, 0}, cp{wave_id, 0};   // next step to load / to multiply: the loads run one step ahead
    issue(ip, buf0); advance(ip);
    while (cp.t < ntiles) {
        if (ip.t < ntiles) { issue(ip, buf1); advance(ip); }
        compute(cp, buf0); advance(cp);
        if (cp.t < ntiles) {
            if (ip.t < ntiles) { issue(ip, buf0); advance(ip); }
            compute(cp, buf1); advance(cp);
        }
    }
}

template <int OB, bool ACT>
static void launch_pb(const PbArgs &a, hipStream_t st) {
    const int nks = (a.Cin + PB_KC - 1) / PB_KC;
    const int lds = nks * (OB * 1024 + PB_KC * (int)sizeof(float4));   // <= 16 * (2048 + 256) = 36 KB
    const long long ntiles = (long long)a.B * ((a.P + PB_COLS - 1) / PB_COLS);
    long long wgs = (ntiles + 3) / 4;
    if (wgs > 2048) wgs = 2048;   // 8 workgroups per CU; waves stride over the tiles
    hipLaunchKernelGGL((pointwise_bf16_kernel<OB, ACT>), dim3((unsigned)wgs), dim3(256), lds, st, a);
}

}  // namespace mgar

using namespace mgar;

MGAR_API int mgar_pointwise_mfma_bf16_fwd(const void *x, int B, int Cin, int P, const float *w, int w_row_stride, int w_col_stride,
                                          int Cout, const float *in_mean, const float *in_invstd, const float *in_gamma,
                                          const float *in_beta, int in_relu, void *y, void *stream) {
    MGAR_REQUIRE(B >= 0 && Cin >= 0 && Cout >= 0 && P >= 0, "pointwise_mfma_bf16_fwd: negative size");
    if ((long long)B * P == 0) return MGAR_OK;
    if (Cout < 1 || Cout > 64 || Cin < 1 || Cin > 256 || (P & 3) != 0) {
        set_error("pointwise_mfma_bf16_fwd: needs 1 <= Cin <= 256, 1 <= Cout <= 64 and P % 4 == 0 (use mgar_pointwise_conv_fwd_bf16 "
                  "or the library GEMM otherwise)");
        return MGAR_EUNSUPPORTED;
    }
    MGAR_REQUIRE(P <= 2147483647 - PB_COLS && (long long)B * ((P + PB_COLS - 1) / PB_COLS) <= (1LL << 30),
                 "pointwise_mfma_bf16_fwd: more than 2^30 column tiles");
    MGAR_REQUIRE(x && w && y, "pointwise_mfma_bf16_fwd: null pointer");
    MGAR_REQUIRE(in_mean == nullptr || in_invstd != nullptr, "pointwise_mfma_bf16_fwd: in_mean without in_invstd");
    MGAR_REQUIRE(((uintptr_t)x & 7) == 0 && ((uintptr_t)y & 7) == 0, "pointwise_mfma_bf16_fwd: x and y must be 8-byte aligned");
    PbArgs a{(const uint16_t *)x, w, in_mean, in_invstd, in_gamma, in_beta, (uint16_t *)y, B, Cin, Cout, P, w_row_stride, w_col_stride,
             in_relu};
    hipStream_t st = (hipStream_t)stream;
    KtScope kt(KT_POINTWISE_BF16, st, 2.0 * (double)B * P * (Cin + Cout), 2.0 * (double)B * P * Cin * Cout);
    if (Cout <= 32) {
        if (in_mean) launch_pb<1, true>(a, st); else launch_pb<1, false>(a, st);
    } else {
        if (in_mean) launch_pb<2, true>(a, st); else launch_pb<2, false>(a, st);
    }
    return check_launch("pointwise_mfma_bf16_fwd: launch failed");
}
