// sparse_conv_bf16.hip -- forward gather-GEMM of the sparse 3-D convolution for bf16 feature rows, on the bf16 MFMA of gfx950
// (v_mfma_f32_32x32x16_bf16).  The bf16 forward configurations run the Voxel R-CNN trunk (VoxelBackBone8x after conv_input) on it
// where the fp32 step runs spconv_os_kernel of csrc/sparse_conv.hip; rulebooks, hash tables and indices are shared with that file.
//
//   out[o] = bf16( sum_k in[nbr[o, k]] . bf16(w[k']) ),   k' = K - 1 - k if flip_k else k
// Products of bf16 operands are exact in the fp32 accumulator, so a row is the fp32 sum of its exact products (offsets ascending,
// 16-channel k-steps ascending inside an offset), rounded ONCE to bf16 on store (round to nearest even) -- the contract of
// csrc/conv3d_bf16.hip and csrc/stem_conv.hip.  An absent neighbour (nbr == -1) contributes nothing.
//
// spconv_os_kernel transposed to the bf16 instruction: a wave owns 32 output rows for the whole kernel, D[row][c_out].
//   * A operand straight from global memory: lane (r = lane & 31, h = lane >> 5) holds A[row r][k = 8 h + j], so for k-step s it
//     needs channels 16 s + 8 h .. + 7 of the gathered row of output row r: ONE 16-byte load, no LDS round trip;
//   * the rows of offset k + 1 (and the table entry of k + 2) are in flight while offset k multiplies;
//   * W is converted to bf16 once per call by spconv_bf16_pack_kernel into [offset][k-step][column block][half 2][column 32][ci 8]:
//     a lane's B fragment (B[k = 8 h + j][col r]) is one 16-byte vector at index lane of its (k-step, column block), a wave's
//     ds_read_b128 covers 1 KB contiguous.  W_k goes through a double-buffered LDS tile filled by all four waves, one barrier per
//     offset; the tile is C_in / 16 x ceil(C_out / 32) KB, at most 32 KB: two fit the 64 KB of static LDS;
//   * an offset under which none of the wave's 64 lanes has a neighbour issues no MFMA (it would add zeros: same bits).
// No atomics, no cross-row state: a row's bits depend on its table row, the rows it names and W only -- not on its position in the
// launch, on No, or on the other rows of its wave.
#include "common.hpp"
#include "payload.hpp"

namespace mgar {

constexpr int SB_MAXC = 128;      // C_in, C_out <= 128
constexpr int SB_MAXK = 343;      // kernel offsets (7 x 7 x 7)
constexpr int SB_ROWS = 128;      // output rows per workgroup: 4 waves x 32

// w (K, Cin, Cout) fp32 -> wp [k][s = Cin / 16][cb = ceil(Cout / 32)][h 2][col 32][j 8] bf16 (round to nearest even), element
// = w[k'][16 s + 8 h + j][32 cb + col]; columns beyond Cout are zero.  The mirrored offset order of flip_k is resolved here.
__global__ __launch_bounds__(256) void spconv_bf16_pack_kernel(const float *__restrict__ w, int K, int Cin, int Cout, int flip_k,
                                                               long long total, uint16_t *__restrict__ wp) {
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= total) return;
    const int j = (int)(e & 7), col = (int)(e >> 3) & 31, h = (int)(e >> 8) & 1;
    long long rest = e >> 9;
    const int ncb = (Cout + 31) / 32, ns = Cin / 16;
    const int cb = (int)(rest % ncb); rest /= ncb;
    const int s = (int)(rest % ns);
    const int k = (int)(rest / ns);
    const int ci = 16 * s + 8 * h + j, co = 32 * cb + col;
    float v = 0.f;
    if (co < Cout) v = w[((long long)(flip_k ? K - 1 - k : k) * Cin + ci) * Cout + co];
    wp[e] = (uint16_t)(pack_bf16x2(v, 0.f) & 0xffffu);
}

// NSP: k-steps the registers are sized for (C_in / 16 rounded up to 1, 2, 4, 8; the steps that exist, ns, are a launch argument);
// NCB: 32-column blocks of the output.  grid ceil(No / 128).
// AFF: an eval-mode BatchNorm [+ ReLU] in the store -- v = fma(acc, scale[c], shift[c]) in fp32, relu ? max(v, +0) with a NaN
// passed through : v, and THEN the one rounding to bf16.  The lane's NCB scale / shift values (columns 32 a + l) are loaded once,
// after the last offset, when the gathered-row registers are dead.
template <int NSP, int NCB, bool AFF>
__global__ __launch_bounds__(256) void spconv_bf16_kernel(int No, int K, int Cin, int Cout, const uint16_t *__restrict__ in,
                                                          const int *__restrict__ nbr, const u32x4 *__restrict__ wp,
                                                          const float *__restrict__ scale, const float *__restrict__ shift, int relu,
                                                          uint16_t *__restrict__ out) {
    constexpr int WPT = (NSP * NCB * 64 + 255) / 256;          // 16-byte vectors of W_k each thread stages
    __shared__ __attribute__((aligned(16))) u32x4 Wl[2][NSP * NCB * 64];
    const int ns = Cin / 16;
    const int tile = ns * NCB * 64;                            // vectors of one packed W_k (<= NSP * NCB * 64)
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int l = lane & 31, h = lane >> 5;
    const long long row = (long long)blockIdx.x * SB_ROWS + wave * 32 + l;
    const bool rok = row < No;
    const int *__restrict__ nrow = nbr + (size_t)(rok ? row : 0) * K;
    f32x16 acc[NCB];
#pragma unroll
    for (int a = 0; a < NCB; ++a)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[a][r] = 0.f;
    u32x4 areg0[NSP], areg1[NSP];                              // the gathered rows of the current / next offset
    u32x4 wreg[WPT];
    auto load_w = [&](int k) {
        const u32x4 *ws = wp + (size_t)k * tile;
#pragma unroll
        for (int q = 0; q < WPT; ++q) {
            const int e = q * 256 + threadIdx.x;
            if (e < tile) wreg[q] = ws[e];
        }
    };
    auto store_w = [&](int buf) {
#pragma unroll
        for (int q = 0; q < WPT; ++q) {
            const int e = q * 256 + threadIdx.x;
            if (e < tile) Wl[buf][e] = wreg[q];
        }
    };
    auto load_a = [&](u32x4 (&dst)[NSP], int j) {
        if (j >= 0) {
            const u32x4 *src = reinterpret_cast<const u32x4 *>(in + (size_t)j * Cin + 8 * h);    // 16-byte aligned: Cin % 16 == 0
#pragma unroll
            for (int s = 0; s < NSP; ++s)
                if (s < ns) dst[s] = src[2 * s];
        } else {
#pragma unroll
            for (int s = 0; s < NSP; ++s) dst[s] = u32x4{0u, 0u, 0u, 0u};
        }
    };
    int j_cur = -1, j_next = -1;
    // one offset: rows of offset k are in `cur`, W_k in Wl[buf]; fetch offset k + 1 into `nxt` / the other W buffer meanwhile
    auto step = [&](int k, int buf, u32x4 (&cur)[NSP], u32x4 (&nxt)[NSP]) {
        const int j1 = j_next;
        if (k + 1 < K) {
            load_w(k + 1);                                     // in flight during the MFMAs below
            j_next = (rok && k + 2 < K) ? nrow[k + 2] : -1;
            load_a(nxt, j1);
        }
        if (__builtin_amdgcn_ballot_w64(j_cur >= 0) != 0ull) { // wave-uniform
            const u32x4 *Wk = Wl[buf] + lane;
#pragma unroll
            for (int s = 0; s < NSP; ++s) {
                if (s < ns) {
                    const bf16x8 av = __builtin_bit_cast(bf16x8, cur[s]);
#pragma unroll
                    for (int a = 0; a < NCB; ++a)
                        acc[a] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(av, __builtin_bit_cast(bf16x8, Wk[(s * NCB + a) * 64]), acc[a],
                                                                         0, 0, 0);
                }
            }
        }
        j_cur = j1;
        if (k + 1 < K) store_w(buf ^ 1);
        __syncthreads();                                       // W_{k+1} visible; W_k's buffer is free for offset k + 2
    };
    // prologue: W_0 -> LDS, rows of offset 0 -> registers, table entry of offset 1
    load_w(0);
    j_cur = rok ? nrow[0] : -1;
    j_next = (rok && K > 1) ? nrow[1] : -1;
    load_a(areg0, j_cur);
    store_w(0);
    __syncthreads();
    for (int k = 0; k < K; k += 2) {
        step(k, 0, areg0, areg1);
        if (k + 1 < K) step(k + 1, 1, areg1, areg0);
    }
    // store: register r of a lane is (row = (r & 3) + 8 (r >> 2) + 4 h, column 32 a + l); one rounding, fp32 -> bf16
    const long long obase = (long long)blockIdx.x * SB_ROWS + wave * 32;
    float sc[NCB], sh[NCB];
    if constexpr (AFF) {
#pragma unroll
        for (int a = 0; a < NCB; ++a) {
            const int co = a * 32 + l;
            sc[a] = co < Cout ? scale[co] : 1.f;
            sh[a] = co < Cout ? shift[co] : 0.f;
        }
    }
#pragma unroll
    for (int a = 0; a < NCB; ++a) {
        const int co = a * 32 + l;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const long long orow = obase + (r & 3) + 8 * (r >> 2) + 4 * h;
            float v = acc[a][r];
            if constexpr (AFF) {
                v = __builtin_fmaf(v, sc[a], sh[a]);
                if (relu) v = v > 0.f ? v : (v != v ? v : 0.f);
            }
            if (orow < No && co < Cout) out[(size_t)orow * Cout + co] = (uint16_t)(pack_bf16x2(v, 0.f) & 0xffffu);
        }
    }
}

static bool sb_plan_ok(int K, int Cin, int Cout) {
    return K >= 1 && K <= SB_MAXK && Cin >= 16 && Cin <= SB_MAXC && Cin % 16 == 0 && Cout >= 1 && Cout <= SB_MAXC;
}

}  // namespace mgar

using namespace mgar;

// bytes of the packed-weight scratch mgar_spconv_bf16_fwd needs (rewritten on every call): K * (Cin / 16) * ceil(Cout / 32) KB --
// per offset, k-step and 32-column block 64 lanes x 16 bytes.  0 for a plan the kernel does not take.
MGAR_API long long mgar_spconv_bf16_workspace_bytes(int K, int Cin, int Cout) {
    if (!sb_plan_ok(K, Cin, Cout)) return 0;
    return (long long)K * (Cin / 16) * ceil_div(Cout, 32) * 1024;
}

// The two forward entry points below share one launcher (arguments already checked).  AFF = false: the plain store; AFF = true:
// the affine [+ ReLU] store.  Same packing pass, same plans, same timer row.
template <bool AFF>
static int spconv_bf16_launch(int No, int K, int Cin, int Cout, const void *in, const int *nbr, const float *w, int flip_k,
                              const float *scale, const float *shift, int relu, void *w_packed, void *out, void *stream) {
    hipStream_t st = (hipStream_t)stream;
    const int ns = Cin / 16, ncb = ceil_div(Cout, 32);
    const long long wtotal = (long long)K * ns * ncb * 512;     // bf16 elements
    hipLaunchKernelGGL(spconv_bf16_pack_kernel, dim3(ceil_div(wtotal, 256)), dim3(256), 0, st, w, K, Cin, Cout, flip_k ? 1 : 0, wtotal,
                       (uint16_t *)w_packed);
    const int nsp = ns <= 1 ? 1 : (ns <= 2 ? 2 : (ns <= 4 ? 4 : 8));
    const dim3 grid(ceil_div(No, SB_ROWS));
    const uint16_t *ip = (const uint16_t *)in;
    const u32x4 *wv = (const u32x4 *)w_packed;
    uint16_t *op = (uint16_t *)out;
    {
        // table (No, K) read, out written at 2 B per element, the fp32 master weight read once; the gathered input rows and the
        // flops depend on the number of pairs, which the caller credits (mgar_ktimer_add_bytes / _flops)
        KtScope kt(KT_SPCONV_BF16, st, 4.0 * No * (double)K + 2.0 * No * (double)Cout + 4.0 * (double)K * Cin * Cout);
#define SB_CASE(NS, NB)                                                                                                      \
        if (nsp == NS && ncb == NB)                                                                                              \
            hipLaunchKernelGGL((spconv_bf16_kernel<NS, NB, AFF>), grid, dim3(256), 0, st, No, K, Cin, Cout, ip, nbr, wv, scale, shift,  \
                               relu, op)
#define SB_ROW(NS) SB_CASE(NS, 1); SB_CASE(NS, 2); SB_CASE(NS, 3); SB_CASE(NS, 4)
        SB_ROW(1); SB_ROW(2); SB_ROW(4); SB_ROW(8);
#undef SB_ROW
#undef SB_CASE
    }
    return check_launch("spconv_bf16_fwd: launch failed");
}

// in (Ni, Cin) bf16 rows, nbr (No, K) int32 (-1 = no neighbour), w (K, Cin, Cout) fp32 -> out (No, Cout) bf16, fully written.
// Cin % 16 == 0, 16 <= Cin <= 128, Cout <= 128, K <= 343: anything else is MGAR_EUNSUPPORTED and the caller keeps the fp32 kernel.
MGAR_API int mgar_spconv_bf16_fwd(int No, int K, int Cin, int Cout, const void *in, const int *nbr, const float *w, int flip_k,
                                  void *w_packed, void *out, void *stream) {
    MGAR_REQUIRE(No >= 0 && K >= 1 && K <= SB_MAXK && Cin >= 1 && Cout >= 1, "spconv_bf16_fwd: bad sizes");
    if (!sb_plan_ok(K, Cin, Cout)) {
        set_error("spconv_bf16_fwd: C_in a multiple of 16 in [16, 128], C_out <= 128");
        return MGAR_EUNSUPPORTED;
    }
    if (No == 0) return MGAR_OK;
    MGAR_REQUIRE(in && nbr && w && w_packed && out, "spconv_bf16_fwd: null pointer");
    MGAR_REQUIRE(((uintptr_t)in & 15) == 0 && ((uintptr_t)w_packed & 15) == 0 && ((uintptr_t)out & 1) == 0,
                 "spconv_bf16_fwd: in and w_packed must be 16-byte aligned");
    return spconv_bf16_launch<false>(No, K, Cin, Cout, in, nbr, w, flip_k, nullptr, nullptr, 0, w_packed, out, stream);
}

// mgar_spconv_bf16_fwd with an eval-mode BatchNorm [+ ReLU] folded into the store: out = bf16(act(fma(acc, scale[c], shift[c]))),
// acc the fp32 accumulator that entry point would have rounded; ONE rounding.  scale, shift (Cout) fp32, both required.  Same
// plans, workspace and refusals.
MGAR_API int mgar_spconv_bf16_fwd_affine(int No, int K, int Cin, int Cout, const void *in, const int *nbr, const float *w, int flip_k,
                                         const float *scale, const float *shift, int relu, void *w_packed, void *out, void *stream) {
    MGAR_REQUIRE(No >= 0 && K >= 1 && K <= SB_MAXK && Cin >= 1 && Cout >= 1, "spconv_bf16_fwd_affine: bad sizes");
    if (!sb_plan_ok(K, Cin, Cout)) {
        set_error("spconv_bf16_fwd_affine: C_in a multiple of 16 in [16, 128], C_out <= 128");
        return MGAR_EUNSUPPORTED;
    }
    if (No == 0) return MGAR_OK;
    MGAR_REQUIRE(in && nbr && w && scale && shift && w_packed && out, "spconv_bf16_fwd_affine: null pointer");
    MGAR_REQUIRE(((uintptr_t)in & 15) == 0 && ((uintptr_t)w_packed & 15) == 0 && ((uintptr_t)out & 1) == 0,
                 "spconv_bf16_fwd_affine: in and w_packed must be 16-byte aligned");
    return spconv_bf16_launch<true>(No, K, Cin, Cout, in, nbr, w, flip_k, scale, shift, relu ? 1 : 0, w_packed, out, stream);
}
