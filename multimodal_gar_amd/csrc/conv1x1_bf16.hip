// conv1x1_bf16.hip -- the 1x1x1 units of Inception-I3D for bf16 payloads on the bf16 MFMA of gfx950 (v_mfma_f32_32x32x16_bf16):
// per sample the product Y[n] (Cout, P) = W (Cout, Cin) . X[n] (Cin, P), P = T * H * W, on the NCDHW tensor as it lies.
//
//   w~[o,i]    = bf16( w[o * Cin + i] )                   fp32 master weight, round to nearest even
//   acc[n,o,p] = sum_i w~[o,i] * x[n,i,p]                 exact products in the fp32 accumulator, 16-channel k-steps ascending
//   plain:  y = bf16(acc)
//   affine: v = fmaf(acc, scale[o], shift[o]);  y = bf16(relu ? relu_nan(v) : v)          ONE rounding of the payload
// -- the contract of csrc/pointwise_bf16.hip and csrc/conv3d_bf16.hip.  A NaN stays a NaN through the ReLU and the rounding.
// y[n,o,p] lies at y + n * y_batch_stride + o * P + p: a unit can write its channels of an Inception module's output.
//
// The operand layout of pointwise_bf16_kernel: W is the A operand, x the B operand; lane (l = lane & 31, h = lane >> 5) issues
// eight 8-byte loads per k-step (channel 16 s + 8 h + j, columns 4 l .. 4 l + 3 of a 128-column tile), packs four B fragments in
// registers (no LDS for x) and stores one 8-byte vector per row.  What is new:
//   * Cout up to 512 = 16 row blocks of 32.  A wave holds OB <= 2 of them (128 accumulator registers); G waves of ONE workgroup
//     share a column tile, wave g of the group owning row blocks g, g + G, ..: every Cout block of a column tile runs in the same
//     workgroup at the same time, so the x tile comes from HBM once (the G - 1 re-reads hit the CU's L1 / the XCD's L2).
//     A workgroup of NW waves works on NW / G tiles at a time.
//   * the K loop: W no longer fits in LDS whole.  The workgroup rounds W into LDS in chunks of KCH = 64 / (G OB) k-steps (64 KB:
//     two workgroups per CU) in fragment order -- [k-step][row block][lane] 16-byte vectors -- between two barriers.  Where the
//     whole of W is one chunk (every unit of Mixed_3b / 3c and Conv3d_2b_1x1) it is written once per workgroup and no barrier
//     sits in the tile loop.  No pack kernel, no workspace.
// Channels beyond Cin and rows beyond Cout are zero in W~, and zero in x too: the load of such a channel (or of a lane without a
// column) goes to a clamped address inside x and its result is replaced by zeros.  Columns beyond P and rows beyond Cout are
// never stored.  No atomics, no cross-column state: a column's bits depend on that column of x, on w and on
// scale / shift only -- not on N, P, y_batch_stride, the tile or the grid.
#include "common.hpp"
#include "payload.hpp"

namespace mgar {

typedef float __attribute__((ext_vector_type(16))) c1_f32x16;
typedef __bf16 __attribute__((ext_vector_type(8))) c1_bf16x8;
typedef unsigned int __attribute__((ext_vector_type(4))) c1_u32x4;

constexpr int C1_COLS = 128;        // columns per tile: 4 interleaved sub-tiles of 32
constexpr int C1_KC = 16;           // channels per k-step
constexpr int C1_LDS_VECS = 64;     // 1 KB (row block, k-step) slabs of W~ in LDS: 64 KB
constexpr int C1_FILL = 4;          // W vectors a thread has in flight while a chunk is filled

struct C1Args {
    const uint16_t *x;              // (N, Cin, P) bf16
    const float *w;                 // (Cout, Cin) fp32
    const float *scale, *shift;     // (Cout), AFF only
    uint16_t *y;
    long long ybs;                  // elements between samples of y
    int N, Cin, Cout, P;
    int relu;
};

// OB row blocks per wave, G waves per column tile, NW waves per workgroup, AFF: the eval-mode BatchNorm [+ ReLU] in the store.
template <int OB, int G, int NW, bool AFF>
__global__ __launch_bounds__(NW * 64, NW == 4 ? 2 : 1) void conv1x1_bf16_kernel(C1Args a) {
    constexpr int NRB = OB * G, KCH = C1_LDS_VECS / NRB, TPW = NW / G, NT = NW * 64;
    extern __shared__ __attribute__((aligned(16))) unsigned char c1_lds[];
    c1_u32x4 *wl = reinterpret_cast<c1_u32x4 *>(c1_lds);                 // [k-step of the chunk][NRB][64 lanes]
    const int nks = (a.Cin + C1_KC - 1) / C1_KC;
    const bool one_chunk = nks <= KCH;
    const bool wvec = (a.Cin & 3) == 0 && ((uintptr_t)a.w & 15) == 0;

    // k-steps [s0, s0 + cnt) of W, rounded, in fragment order.  C1_FILL vectors per thread at a time: their 2 C1_FILL loads are in
    // flight together (one vector per trip is a chain of L2 latencies, 16 trips per 64 KB chunk)
    auto fill = [&](const int s0) {
        const int total = min(KCH, nks - s0) * NRB * 64;
        for (int e0 = threadIdx.x; e0 < total; e0 += NT * C1_FILL) {
            float4 lo[C1_FILL], hi[C1_FILL];
#pragma unroll
            for (int u = 0; u < C1_FILL; ++u) {
                // vector e = A fragment of lane (l, h) for k-step s, row block rb: W~[32 rb + l][16 s + 8 h + j], j = 0 .. 7
                const int e = e0 + u * NT, ln = e & 63, rb = (e >> 6) % NRB, s = s0 + (e >> 6) / NRB;
                const int o = rb * 32 + (ln & 31), ch0 = s * C1_KC + 8 * (ln >> 5);
                const float *src = a.w + (size_t)o * a.Cin + ch0;
                lo[u] = hi[u] = make_float4(0.f, 0.f, 0.f, 0.f);
                if (e < total && o < a.Cout) {
                    if (wvec && ch0 + 8 <= a.Cin) {
                        lo[u] = *reinterpret_cast<const float4 *>(src);
                        hi[u] = *reinterpret_cast<const float4 *>(src + 4);
                    } else {
                        if (ch0 + 0 < a.Cin) lo[u].x = src[0];
                        if (ch0 + 1 < a.Cin) lo[u].y = src[1];
                        if (ch0 + 2 < a.Cin) lo[u].z = src[2];
                        if (ch0 + 3 < a.Cin) lo[u].w = src[3];
                        if (ch0 + 4 < a.Cin) hi[u].x = src[4];
                        if (ch0 + 5 < a.Cin) hi[u].y = src[5];
                        if (ch0 + 6 < a.Cin) hi[u].z = src[6];
                        if (ch0 + 7 < a.Cin) hi[u].w = src[7];
                    }
                }
            }
#pragma unroll
            for (int u = 0; u < C1_FILL; ++u)
                if (e0 + u * NT < total)
                    wl[e0 + u * NT] = c1_u32x4{pack_bf16x2(lo[u].x, lo[u].y), pack_bf16x2(lo[u].z, lo[u].w), pack_bf16x2(hi[u].x, hi[u].y),
                                               pack_bf16x2(hi[u].z, hi[u].w)};
        }
    };

    // the wave's position is wave-uniform: pinned to scalar registers
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int l = lane & 31, h = lane >> 5;
    const int g = wave % G, slot = wave / G;                    // row blocks g + G ob of tile slot `slot` of the workgroup's tile group
    const int tiles_per_n = (a.P + C1_COLS - 1) / C1_COLS;
    const int ntiles = a.N * tiles_per_n;                       // <= 2^30 (checked by the entry point)
    const int ngroups = (ntiles + TPW - 1) / TPW;               // a workgroup takes TPW tiles at a time; every wave of it makes
    const int gstep = (int)gridDim.x;                           // the same number of steps (the barriers of fill are uniform)

    c1_f32x16 acc[OB][4];
#pragma unroll
    for (int ob = 0; ob < OB; ++ob)
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[ob][i][r] = 0.f;

    struct Pos { int tg, ks; };   // tile group, k-step
    auto advance = [&](Pos &q) {
        if (++q.ks == nks) { q.ks = 0; q.tg += gstep; }
    };
    // Straight-line loads: a load in a branch of its own makes the compiler wait for every load in flight at the join, and the
    // pipeline below is gone.  A lane without a column (beyond P, or a tile beyond the last) reads column 0 of sample 0, a channel
    // beyond Cin reads channel Cin - 1 -- always inside x -- and compute() replaces what came back by zeros.
    auto issue = [&](const Pos q, uint2 (&buf)[8]) {
        const int t = q.tg * TPW + slot;
        const int n = t / tiles_per_n;
        const int p0 = (t - n * tiles_per_n) * C1_COLS;
        const bool pok = t < ntiles && p0 + 4 * l < a.P;
        const uint16_t *src = pok ? a.x + (size_t)n * a.Cin * a.P + p0 + 4 * l : a.x;
        const int ch0 = q.ks * C1_KC + 8 * h;
#pragma unroll
        for (int j = 0; j < 8; ++j)
            buf[j] = *reinterpret_cast<const uint2 *>(src + (size_t)min(ch0 + j, a.Cin - 1) * a.P);
    };
    auto compute = [&](const Pos q, uint2 (&buf)[8]) {
        const int ks = q.ks, kl = ks % KCH;
        if (kl == 0 && !one_chunk) {     // workgroup-uniform: the next chunk of W~ replaces the one every wave has finished with
            __syncthreads();
            fill(ks);
            __syncthreads();
        }
        {
            const int t = q.tg * TPW + slot;
            const int n = t / tiles_per_n;
            const bool pok = t < ntiles && (t - n * tiles_per_n) * C1_COLS + 4 * l < a.P;
            const int ch0 = ks * C1_KC + 8 * h;
#pragma unroll
            for (int j = 0; j < 8; ++j)
                if (!(pok && ch0 + j < a.Cin)) buf[j] = make_uint2(0u, 0u);
        }
        c1_u32x4 bf[4];   // B fragments of the four sub-tiles: dword d = fragment elements 2 d (low half), 2 d + 1 (high half)
#pragma unroll
        for (int d = 0; d < 4; ++d) {
            const uint2 u0 = buf[2 * d], u1 = buf[2 * d + 1];
            bf[0][d] = (u0.x & 0xffffu) | (u1.x << 16);
            bf[1][d] = (u0.x >> 16) | (u1.x & 0xffff0000u);
            bf[2][d] = (u0.y & 0xffffu) | (u1.y << 16);
            bf[3][d] = (u0.y >> 16) | (u1.y & 0xffff0000u);
        }
#pragma unroll
        for (int ob = 0; ob < OB; ++ob) {
            const int rb = g + G * ob;
            if (rb * 32 < a.Cout) {      // wave-uniform: a row block beyond Cout multiplies nothing
                const c1_bf16x8 wa = __builtin_bit_cast(c1_bf16x8, wl[(kl * NRB + rb) * 64 + lane]);
#pragma unroll
                for (int i = 0; i < 4; ++i)
                    acc[ob][i] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wa, __builtin_bit_cast(c1_bf16x8, bf[i]), acc[ob][i], 0, 0, 0);
            }
        }
        if (ks == nks - 1) {  // tile finished: D[row = (r & 3) + 8 (r >> 2) + 4 h][col = l] of sub-tile i = column 4 l + i
            const int t = q.tg * TPW + slot;
            const int n = t / tiles_per_n;
            const int p = (t - n * tiles_per_n) * C1_COLS + 4 * l;
            const bool pok = t < ntiles && p < a.P;
            uint16_t *dst = a.y + (size_t)n * a.ybs + (size_t)(4 * h) * a.P + p;
            [[maybe_unused]] const float lim = a.relu ? 0.f : -__builtin_inff();
            // the lane's first row, 32 g + 4 h: every row of the epilogue is this plus a compile-time constant, so one address per
            // vector serves all 16 OB loads (an address per row would be hoisted out of the tile loop: 64 registers)
            [[maybe_unused]] const float *scp = a.scale + (g * 32 + 4 * h), *shp = a.shift + (g * 32 + 4 * h);
#pragma unroll
            for (int ob = 0; ob < OB; ++ob)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int oc = G * ob * 32 + (r & 3) + 8 * (r >> 2), ou = g * 32 + oc;
                    if (pok && ou + 4 * h < a.Cout) {
                        float v0 = acc[ob][0][r], v1 = acc[ob][1][r], v2 = acc[ob][2][r], v3 = acc[ob][3][r];
                        if constexpr (AFF) {
                            const float sc = scp[oc], sh = shp[oc];
                            v0 = __builtin_fmaf(v0, sc, sh); v1 = __builtin_fmaf(v1, sc, sh);
                            v2 = __builtin_fmaf(v2, sc, sh); v3 = __builtin_fmaf(v3, sc, sh);
                            // relu_nan with the floor lim = 0 (ReLU) or -inf (none): !(v <= lim) ? v : lim keeps a NaN, -0 gives +0
                            v0 = !(v0 <= lim) ? v0 : lim; v1 = !(v1 <= lim) ? v1 : lim;
                            v2 = !(v2 <= lim) ? v2 : lim; v3 = !(v3 <= lim) ? v3 : lim;
                        }
                        *reinterpret_cast<uint2 *>(dst + (size_t)ou * a.P) = make_uint2(pack_bf16x2(v0, v1), pack_bf16x2(v2, v3));
                    }
                    acc[ob][0][r] = 0.f; acc[ob][1][r] = 0.f; acc[ob][2][r] = 0.f; acc[ob][3][r] = 0.f;
                }
        }
    };

    // next step to load / to multiply: the loads run NBUF - 1 steps ahead (a workgroup with few tiles -- one clip at the
    // 14 400-column units -- is a chain of Cin / 16 load latencies otherwise); the first of them are in flight while W is filled
    constexpr int NBUF = OB == 1 ? 6 : 3;                 // (four would spill next to 128 accumulator registers)
    uint2 buf[NBUF][8];
    Pos ip{(int)blockIdx.x, 0}, cp{(int)blockIdx.x, 0};
    if (cp.tg >= ngroups) return;                         // (the whole workgroup)
#pragma unroll
    for (int i = 0; i < NBUF - 1; ++i)
        if (ip.tg < ngroups) { issue(ip, buf[i]); advance(ip); }
    if (one_chunk) {
        fill(0);
        __syncthreads();
    }
    while (cp.tg < ngroups) {
#pragma unroll
        for (int i = 0; i < NBUF; ++i)
            if (cp.tg < ngroups) {
                if (ip.tg < ngroups) { issue(ip, buf[(i + NBUF - 1) % NBUF]); advance(ip); }
                compute(cp, buf[i]); advance(cp);
            }
    }
}

template <int OB, int G, int NW, bool AFF>
static void launch_c1(const C1Args &a, hipStream_t st) {
    constexpr int NRB = OB * G, KCH = C1_LDS_VECS / NRB, TPW = NW / G;
    const int nks = (a.Cin + C1_KC - 1) / C1_KC;
    const int lds = (nks < KCH ? nks : KCH) * NRB * 1024;      // <= 64 KB
    const long long ntiles = (long long)a.N * ((a.P + C1_COLS - 1) / C1_COLS);
    long long wgs = (ntiles + TPW - 1) / TPW;
    if (wgs > 1024) wgs = 1024;   // 4 workgroups per CU; they stride over the tile groups
    hipLaunchKernelGGL((conv1x1_bf16_kernel<OB, G, NW, AFF>), dim3((unsigned)wgs), dim3(NW * 64), lds, st, a);
}

template <bool AFF>
static int c1_forward(const char *name_unsupported, const char *name_launch, const void *x, int N, int Cin, int P, const float *w,
                      int Cout, const float *scale, const float *shift, int relu, void *y, long long ybs, void *stream) {
    MGAR_REQUIRE(N >= 0 && Cin >= 0 && Cout >= 0 && P >= 0, "conv1x1_bf16_fwd: negative size");
    if ((long long)N * P == 0) return MGAR_OK;
    if (Cin < 1 || Cin > 1024 || Cout < 1 || Cout > 512 || (P & 3) != 0 || ((uintptr_t)x & 7) != 0 || ((uintptr_t)y & 7) != 0 ||
        (ybs & 3) != 0) {
        set_error(name_unsupported);
        return MGAR_EUNSUPPORTED;
    }
    MGAR_REQUIRE(P <= 2147483647 - C1_COLS && (long long)N * ((P + C1_COLS - 1) / C1_COLS) <= (1LL << 30),
                 "conv1x1_bf16_fwd: more than 2^30 column tiles");
    MGAR_REQUIRE(x && w && y && (!AFF || (scale && shift)), "conv1x1_bf16_fwd: null pointer");
    MGAR_REQUIRE(ybs >= (long long)Cout * P, "conv1x1_bf16_fwd: y_batch_stride smaller than Cout * P");
    C1Args a{(const uint16_t *)x, w, scale, shift, (uint16_t *)y, ybs, N, Cin, Cout, P, relu};
    hipStream_t st = (hipStream_t)stream;
    KtScope kt(KT_CONV1X1_BF16, st, 2.0 * (double)N * P * (Cin + Cout), 2.0 * (double)N * P * Cin * Cout);
    if (Cout <= 32) launch_c1<1, 1, 4, AFF>(a, st);
    else if (Cout <= 64) launch_c1<2, 1, 4, AFF>(a, st);
    else if (Cout <= 128) launch_c1<2, 2, 4, AFF>(a, st);
    else if (Cout <= 256) launch_c1<2, 4, 4, AFF>(a, st);
    else launch_c1<2, 8, 8, AFF>(a, st);
    return check_launch(name_launch);
}

}  // namespace mgar

using namespace mgar;

MGAR_API int mgar_conv1x1_bf16_fwd(const void *x, int N, int Cin, int P, const float *w, int Cout, void *y, long long y_batch_stride,
                                   void *stream) {
    return c1_forward<false>("conv1x1_bf16_fwd: needs 1 <= Cin <= 1024, 1 <= Cout <= 512, P % 4 == 0, x and y 8-byte aligned and "
                             "y_batch_stride % 4 == 0 (use the library GEMM or convolution otherwise)",
                             "conv1x1_bf16_fwd: launch failed", x, N, Cin, P, w, Cout, nullptr, nullptr, 0, y, y_batch_stride, stream);
}

MGAR_API int mgar_conv1x1_bf16_fwd_affine(const void *x, int N, int Cin, int P, const float *w, int Cout, const float *scale,
                                          const float *shift, int relu, void *y, long long y_batch_stride, void *stream) {
    return c1_forward<true>("conv1x1_bf16_fwd_affine: needs 1 <= Cin <= 1024, 1 <= Cout <= 512, P % 4 == 0, x and y 8-byte aligned "
                            "and y_batch_stride % 4 == 0 (use the library GEMM or convolution + mgar_bn_act_fwd otherwise)",
                            "conv1x1_bf16_fwd_affine: launch failed", x, N, Cin, P, w, Cout, scale, shift, relu, y, y_batch_stride,
                            stream);
}
