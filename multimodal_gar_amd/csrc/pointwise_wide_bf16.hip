// pointwise_wide_bf16.hip -- the point-wise product Y[b] (Cout, P) = W (Cout, Cin) . X[b] (Cin, P) for bf16 payloads on the bf16
// MFMA of gfx950 (v_mfma_f32_32x32x16_bf16) beyond the 64 channels of csrc/pointwise_bf16.hip: ONE kernel template behind
//   mgar_pointwise_wide_bf16_fwd, mgar_pointwise_wide_maxpool_bf16_fwd   the WIDE layers of the shared MLPs (SA levels 2-4, the FP
//                                       modules and FP projections of PointNet++): the previous layer's BatchNorm [+ ReLU] applied
//                                       to the input on the fly, optionally the NEXT BatchNorm [+ ReLU] [+ max over nsample] in the store
//   mgar_conv1x1_bf16_fwd[_affine]      the 1x1x1 units of Inception-I3D on the NCDHW tensor as it lies (P = T * H * W), eval-mode
//                                       BatchNorm [+ ReLU] in the store; identity prologue, w_ld = Cin
// The contract (that of csrc/pointwise_bf16.hip and csrc/conv3d_bf16.hip):
//
//   a[b,i,p] = bf16( act_i(float(x[b,i,p])) )     act_i(v) = relu_nan?(((v - mean_i) * sc_i) + beta_i), sc_i = invstd_i * gamma_i,
//                                                 every operation rounded to fp32 on its own; identity prologue: a = x
//   w~[o,i]  = bf16( w[o * w_ld + i] )            fp32 master weight, round to nearest even
//   acc      = sum_i w~[o,i] * a[b,i,p]           exact products in the fp32 accumulator, 16-channel k-steps ascending
//   plain :  y[b,o,p] = bf16(acc)
//   affine:  y[b,o,p] = bf16(relu_nan?(fmaf(acc, scale_o, shift_o)))                               ONE rounding of the payload
//   pooled:  y[b,o,m] = bf16(max_{s < ns} relu_nan?(fmaf(acc[b,o,m*ns+s], scale_o, shift_o)))      x (B, Cin, M, ns), max_nan
// A NaN stays a NaN through the ReLU, the max and the rounding.  Unpooled, y[b,o,p] lies at y + b * y_batch_stride + o * P + p: a
// unit can write its channels of an Inception module's output.
//
// Structure: the operand layout of pointwise_bf16_kernel -- W is the A operand, x the B operand straight from global memory
// (no LDS for x): lane (l = lane & 31, h = lane >> 5) issues eight 8-byte loads per k-step (channel 16 s + 8 h + j, columns
// 4 l .. 4 l + 3 of a 128-column tile), packs four B fragments in registers and stores one 8-byte vector per row.  Beyond it:
//   * Cout up to 512 = 16 row blocks of 32.  A wave holds OB <= 2 of them (128 accumulator registers); G waves of ONE workgroup
//     share a column tile, wave g of the group owning row blocks g, g + G, ..: every Cout block of a column tile runs in the same
//     workgroup at the same time, so the x tile comes from HBM once (the G - 1 re-reads hit the CU's L1 / the XCD's L2).
//     A workgroup of NW waves works on NW / G tiles at a time.
//   * the K loop: W does not fit in LDS whole.  The workgroup rounds W into LDS in chunks of KCH = 64 / (G OB) k-steps (64 KB: two
//     workgroups per CU) in fragment order -- [k-step][row block][lane] 16-byte vectors -- between two barriers.  Where the whole
//     of W is one chunk (every unit of Mixed_3b / 3c and Conv3d_2b_1x1) it is written once per workgroup and no barrier sits in
//     the tile loop.  No pack kernel, no workspace.  Tiles are software-pipelined NBUF - 1 steps ahead.
//   * the prologue (ACT) works per load = per channel on a table (sc, beta, mean) in LDS; the table is filled WITH the W chunk and
//     covers that chunk's channels only, and ACT instances cap KCH at 32: at most 512 x 16 B = 8 KB next to the 64 KB of W, so
//     two workgroups still share a CU (a table for all 1024 channels would make it 80 KB each: 160 KB, the whole CU).  The cap
//     binds only where G OB = 1 (Cout <= 32); an identity-prologue instance has no table and keeps up to 64 k-steps in one chunk
//     there -- the k-steps ascend either way, so the chunking never shows in the bits.
//   * the pooled store (MAXPOOL epilogue of csrc/pointwise_fwd.hip): a lane holds columns 4 l .. 4 l + 3 of a row, a group of ns
//     columns is ns / 4 neighbouring lanes of one half-wave (tiles start at multiples of 128, ns divides 128), so the reduction
//     is a max within the lane and log2(ns / 4) cross-lane steps per row; the group's first lane stores.
// Channels beyond Cin and rows beyond Cout are zero in W~; the load of such a channel (or of a lane without a column) goes to
// a clamped address inside x and its result never reaches the MFMA: identity instances zero the loaded bits, ACT instances
// select zero after the prologue.  Columns beyond P and rows beyond Cout are never stored.  No atomics, no cross-column state:
// a column's bits (pooled: a group's) depend on that column (group) of x, on w and on the vectors only -- not on B, P,
// y_batch_stride, the tile or the grid.  Accumulators are zeroed after every epilogue.
#include "common.hpp"
#include "payload.hpp"

namespace mgar {

constexpr int PW_COLS = 128;        // columns per tile: 4 interleaved sub-tiles of 32
constexpr int PW_KC = 16;           // channels per k-step
constexpr int PW_LDS_VECS = 64;     // 1 KB (row block, k-step) slabs of W~ in LDS: 64 KB
constexpr int PW_MAX_KCH = 32;      // k-steps per chunk at most where there is a prologue table: a chunk's table stays within 8 KB
constexpr int PW_FILL = 4;          // W vectors a thread has in flight while a chunk is filled

enum PwEpilogue { EPI_PLAIN, EPI_AFFINE, EPI_POOLED };

// k-steps of W~ a chunk holds for NRB row blocks
constexpr int pw_kch(int NRB, bool ACT) { return ACT && PW_LDS_VECS / NRB > PW_MAX_KCH ? PW_MAX_KCH : PW_LDS_VECS / NRB; }

// What the identity-prologue plain / affine instances read comes first, laid out as the I3D kernel's own argument block was.
struct PwArgs {
    const uint16_t *x;                          // (B, Cin, P) bf16
    const float *w;                             // rows w_ld floats apart
    const float *scale, *shift;                 // (Cout), EPI_AFFINE and EPI_POOLED only
    uint16_t *y;
    long long ybs;                              // elements between samples of y
    int B, Cin, Cout, P;
    int out_relu, w_ld;
    const float *mean, *invstd, *gamma, *beta;  // (Cin), ACT instances only
    int in_relu, ns;
};

// OB row blocks per wave, G waves per column tile, NW waves per workgroup; ACT: the BatchNorm [+ ReLU] prologue; EPI: the store.
template <int OB, int G, int NW, bool ACT, PwEpilogue EPI>
__global__ __launch_bounds__(NW * 64, NW == 4 ? 2 : 1) void pointwise_wide_bf16_kernel(PwArgs a) {
    constexpr int NRB = OB * G, KCH = pw_kch(NRB, ACT), TPW = NW / G, NT = NW * 64;
    extern __shared__ __attribute__((aligned(16))) unsigned char pw_lds[];
    const int nks = (a.Cin + PW_KC - 1) / PW_KC;
    u32x4 *wl = reinterpret_cast<u32x4 *>(pw_lds);                       // [k-step of the chunk][NRB][64 lanes]
    [[maybe_unused]] float4 *act = reinterpret_cast<float4 *>(pw_lds + (size_t)min(KCH, nks) * NRB * 1024);   // [16 per k-step of the chunk]
    const bool one_chunk = nks <= KCH;
    const bool wvec = (a.w_ld & 3) == 0 && ((uintptr_t)a.w & 15) == 0;

    // k-steps [s0, s0 + cnt) of W, rounded, in fragment order, and the prologue constants of their channels.  PW_FILL vectors
    // per thread at a time: their 2 PW_FILL loads are in flight together (one vector per trip is a chain of L2 latencies, 16
    // trips per 64 KB chunk)
    auto fill = [&](const int s0) {
        const int cnt = min(KCH, nks - s0);
        const int total = cnt * NRB * 64;
        for (int e0 = threadIdx.x; e0 < total; e0 += NT * PW_FILL) {
            float4 lo[PW_FILL], hi[PW_FILL];
#pragma unroll
            for (int u = 0; u < PW_FILL; ++u) {
                // vector e = A fragment of lane (l, h) for k-step s, row block rb: W~[32 rb + l][16 s + 8 h + j], j = 0 .. 7
                const int e = e0 + u * NT, ln = e & 63, rb = (e >> 6) % NRB, s = s0 + (e >> 6) / NRB;
                const int o = rb * 32 + (ln & 31), ch0 = s * PW_KC + 8 * (ln >> 5);
                const float *src = a.w + (size_t)o * a.w_ld + ch0;
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
            for (int u = 0; u < PW_FILL; ++u)
                if (e0 + u * NT < total)
                    wl[e0 + u * NT] = u32x4{pack_bf16x2(lo[u].x, lo[u].y), pack_bf16x2(lo[u].z, lo[u].w), pack_bf16x2(hi[u].x, hi[u].y),
                                            pack_bf16x2(hi[u].z, hi[u].w)};
        }
        if constexpr (ACT) {   // (padding channels: compute() selects zero for them)
            for (int c = threadIdx.x; c < cnt * PW_KC; c += NT)
                act[c] = bn_prologue_entry(s0 * PW_KC + c, a.Cin, a.mean, a.invstd, a.gamma, a.beta);
        }
    };

    // the wave's position is wave-uniform: pinned to scalar registers
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int l = lane & 31, h = lane >> 5;
    const int g = wave % G, slot = wave / G;                    // row blocks g + G ob of tile slot `slot` of the workgroup's tile group
    const int tiles_per_b = (a.P + PW_COLS - 1) / PW_COLS;
    const int ntiles = a.B * tiles_per_b;                       // <= 2^30 (checked by the entry point)
    const int ngroups = (ntiles + TPW - 1) / TPW;               // a workgroup takes TPW tiles at a time; every wave of it makes
    const int gstep = (int)gridDim.x;                           // the same number of steps (the barriers of fill are uniform)

    f32x16 acc[OB][4];
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
        const int b = t / tiles_per_b;
        const int p0 = (t - b * tiles_per_b) * PW_COLS;
        const bool pok = t < ntiles && p0 + 4 * l < a.P;
        const uint16_t *src = pok ? a.x + (size_t)b * a.Cin * a.P + p0 + 4 * l : a.x;
        const int ch0 = q.ks * PW_KC + 8 * h;
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
        u32x4 bf[4];   // B fragments of the four sub-tiles: dword d = fragment elements 2 d (low half), 2 d + 1 (high half)
        {
            const int t = q.tg * TPW + slot;
            const int b = t / tiles_per_b;
            const bool pok = t < ntiles && (t - b * tiles_per_b) * PW_COLS + 4 * l < a.P;
            const int ch0 = ks * PW_KC + 8 * h;
            if constexpr (ACT) {
                const float4 *ac = act + kl * PW_KC + 8 * h;
                const bool relu = a.in_relu != 0;
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
                        if (!(pok && ch0 + 2 * d + e < a.Cin)) v[e][0] = v[e][1] = v[e][2] = v[e][3] = 0.f;
                    }
#pragma unroll
                    for (int i = 0; i < 4; ++i) bf[i][d] = pack_bf16x2(v[0][i], v[1][i]);
                }
            } else {
#pragma unroll
                for (int j = 0; j < 8; ++j)
                    if (!(pok && ch0 + j < a.Cin)) buf[j] = make_uint2(0u, 0u);
                pack_b_fragments(buf, bf);
            }
        }
#pragma unroll
        for (int ob = 0; ob < OB; ++ob) {
            const int rb = g + G * ob;
            if (rb * 32 < a.Cout) {      // wave-uniform: a row block beyond Cout multiplies nothing
                const bf16x8 wa = __builtin_bit_cast(bf16x8, wl[(kl * NRB + rb) * 64 + lane]);
#pragma unroll
                for (int i = 0; i < 4; ++i)
                    acc[ob][i] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wa, __builtin_bit_cast(bf16x8, bf[i]), acc[ob][i], 0, 0, 0);
            }
        }
        if (ks == nks - 1) {  // tile finished: D[row = (r & 3) + 8 (r >> 2) + 4 h][col = l] of sub-tile i = column 4 l + i
            const int t = q.tg * TPW + slot;
            const int b = t / tiles_per_b;
            const int p = (t - b * tiles_per_b) * PW_COLS + 4 * l;
            const bool pok = t < ntiles && p < a.P;
            // relu_nan with the floor lim = 0 (ReLU) or -inf (none): !(v <= lim) ? v : lim keeps a NaN, -0 gives +0
            [[maybe_unused]] const float lim = a.out_relu ? 0.f : -__builtin_inff();
            // the lane's first row, 32 g + 4 h: every row of the epilogue is this plus a compile-time constant, so one address per
            // vector serves all 16 OB loads (an address per row would be hoisted out of the tile loop: 64 registers)
            [[maybe_unused]] const float *scp = a.scale + (g * 32 + 4 * h), *shp = a.shift + (g * 32 + 4 * h);
            if constexpr (EPI == EPI_POOLED) {
                const int gl = a.ns >> 2;                                     // lanes per group: 1, 2, 4, .., 32
                const int M = a.P / a.ns, m = (int)((unsigned)p / (unsigned)a.ns);
                const bool lead = pok && (l & (gl - 1)) == 0;
                uint16_t *dst = a.y + ((size_t)b * a.Cout + 4 * h) * M + m;
#pragma unroll
                for (int ob = 0; ob < OB; ++ob)
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const int oc = G * ob * 32 + (r & 3) + 8 * (r >> 2), ou = g * 32 + oc;
                        const bool rok = ou + 4 * h < a.Cout;
                        float sc = 0.f, sh = 0.f;
                        if (rok) { sc = scp[oc]; sh = shp[oc]; }
                        float v0 = __builtin_fmaf(acc[ob][0][r], sc, sh), v1 = __builtin_fmaf(acc[ob][1][r], sc, sh);
                        float v2 = __builtin_fmaf(acc[ob][2][r], sc, sh), v3 = __builtin_fmaf(acc[ob][3][r], sc, sh);
                        v0 = !(v0 <= lim) ? v0 : lim; v1 = !(v1 <= lim) ? v1 : lim;
                        v2 = !(v2 <= lim) ? v2 : lim; v3 = !(v3 <= lim) ? v3 : lim;
                        float best = max_nan(max_nan(max_nan(v0, v1), v2), v3);
                        // every lane of the wave takes part; a group's lanes share pok and rok
                        // (a rolled loop: unrolled, the epilogue -- which the tile pipeline below repeats NBUF times -- grows past
                        // what the compiler unrolls in full, and the load buffers go to scratch)
#pragma unroll 1
                        for (int d = 1; d < gl; d <<= 1) best = max_nan(best, __shfl_xor(best, d, 32));
                        if (lead && rok) dst[(size_t)ou * M] = (uint16_t)(pack_bf16x2(best, 0.f) & 0xffffu);
                        acc[ob][0][r] = 0.f; acc[ob][1][r] = 0.f; acc[ob][2][r] = 0.f; acc[ob][3][r] = 0.f;
                    }
            } else {
                uint16_t *dst = a.y + (size_t)b * a.ybs + (size_t)(4 * h) * a.P + p;
#pragma unroll
                for (int ob = 0; ob < OB; ++ob)
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const int oc = G * ob * 32 + (r & 3) + 8 * (r >> 2), ou = g * 32 + oc;
                        if (pok && ou + 4 * h < a.Cout) {
                            float v0 = acc[ob][0][r], v1 = acc[ob][1][r], v2 = acc[ob][2][r], v3 = acc[ob][3][r];
                            if constexpr (EPI == EPI_AFFINE) {
                                const float sc = scp[oc], sh = shp[oc];
                                v0 = __builtin_fmaf(v0, sc, sh); v1 = __builtin_fmaf(v1, sc, sh);
                                v2 = __builtin_fmaf(v2, sc, sh); v3 = __builtin_fmaf(v3, sc, sh);
                                v0 = !(v0 <= lim) ? v0 : lim; v1 = !(v1 <= lim) ? v1 : lim;
                                v2 = !(v2 <= lim) ? v2 : lim; v3 = !(v3 <= lim) ? v3 : lim;
                            }
                            *reinterpret_cast<uint2 *>(dst + (size_t)ou * a.P) = make_uint2(pack_bf16x2(v0, v1), pack_bf16x2(v2, v3));
                        }
                        acc[ob][0][r] = 0.f; acc[ob][1][r] = 0.f; acc[ob][2][r] = 0.f; acc[ob][3][r] = 0.f;
                    }
            }
        }
    };

    // next step to load / to multiply: the loads run NBUF - 1 steps ahead (a workgroup with few tiles -- one clip at the
    // 14 400-column units of I3D -- is a chain of Cin / 16 load latencies otherwise); the first of them are in flight while W is
    // filled (OB = 2: four would spill next to 128 accumulator registers; OB = 1 with both the prologue and the pooled store: six
    // copies of the step are more than the compiler unrolls in full, and the buffers would go to scratch)
    constexpr int NBUF = OB == 1 ? (ACT && EPI == EPI_POOLED ? 4 : 6) : 3;
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

template <int OB, int G, int NW, bool ACT, PwEpilogue EPI>
static void launch_pw(const PwArgs &a, hipStream_t st) {
    constexpr int NRB = OB * G, KCH = pw_kch(NRB, ACT), TPW = NW / G;
    const int nks = (a.Cin + PW_KC - 1) / PW_KC;
    const int kch = nks < KCH ? nks : KCH;
    const int lds = kch * (NRB * 1024 + (ACT ? PW_KC * (int)sizeof(float4) : 0));      // <= 64 KB + 8 KB
    // above 64 KB the limit is raised on every such launch: the attribute belongs to the current device, and a flag kept per
    // process would leave a second GPU of the same process without it (a host-side call, no stream work)
    if (lds > 64 * 1024)
        (void)hipFuncSetAttribute((const void *)pointwise_wide_bf16_kernel<OB, G, NW, ACT, EPI>,
                                  hipFuncAttributeMaxDynamicSharedMemorySize, 72 * 1024);
    const long long ntiles = (long long)a.B * ((a.P + PW_COLS - 1) / PW_COLS);
    long long wgs = (ntiles + TPW - 1) / TPW;
    if (wgs > 1024) wgs = 1024;   // 4 workgroups per CU; they stride over the tile groups
    hipLaunchKernelGGL((pointwise_wide_bf16_kernel<OB, G, NW, ACT, EPI>), dim3((unsigned)wgs), dim3(NW * 64), lds, st, a);
}

template <bool ACT, PwEpilogue EPI>
static void launch_by_cout(const PwArgs &a, hipStream_t st) {
    if (a.Cout <= 32) launch_pw<1, 1, 4, ACT, EPI>(a, st);
    else if (a.Cout <= 64) launch_pw<2, 1, 4, ACT, EPI>(a, st);
    else if (a.Cout <= 128) launch_pw<2, 2, 4, ACT, EPI>(a, st);
    else if (a.Cout <= 256) launch_pw<2, 4, 4, ACT, EPI>(a, st);
    else launch_pw<2, 8, 8, ACT, EPI>(a, st);
}

// What an entry point brings to pw_forward besides its operands: the timer row, whether a NULL out_scale is an error, and the
// texts of its errors (set_error keeps the pointer, so whole literals); the MGAR_EINVAL texts are one set per family.
struct PwFamily {
    int kt;
    const char *negative, *tiles, *null, *ybs;
};
struct PwEntry {
    const PwFamily &family;
    bool needs_affine;
    const char *unsupported, *launch;
};
static const PwFamily kWide{KT_POINTWISE_WIDE_BF16, "pointwise_wide_bf16: negative size", "pointwise_wide_bf16: more than 2^30 column tiles",
                            "pointwise_wide_bf16: null pointer", "pointwise_wide_bf16_fwd: y_batch_stride smaller than Cout * P"};
static const PwFamily kConv1x1{KT_CONV1X1_BF16, "conv1x1_bf16_fwd: negative size", "conv1x1_bf16_fwd: more than 2^30 column tiles",
                               "conv1x1_bf16_fwd: null pointer", "conv1x1_bf16_fwd: y_batch_stride smaller than Cout * P"};
static const PwEntry kWideFwd{kWide, false,
                              "pointwise_wide_bf16_fwd: needs 1 <= Cin <= 1024, 1 <= Cout <= 512, P % 4 == 0, w_ld >= Cin, x and y 8-byte "
                              "aligned and y_batch_stride % 4 == 0 (use the library GEMM otherwise)",
                              "pointwise_wide_bf16_fwd: launch failed"};
static const PwEntry kWidePooled{kWide, false,
                                 "pointwise_wide_maxpool_bf16_fwd: needs 1 <= Cin <= 1024, 1 <= Cout <= 512, nsample in {4, 8, 16, 32, 64, "
                                 "128}, w_ld >= Cin, x and y 8-byte aligned (use mgar_pointwise_wide_bf16_fwd + mgar_bn_act_maxpool_fwd "
                                 "otherwise)",
                                 "pointwise_wide_maxpool_bf16_fwd: launch failed"};
static const PwEntry kConv1x1Plain{kConv1x1, false,
                                   "conv1x1_bf16_fwd: needs 1 <= Cin <= 1024, 1 <= Cout <= 512, P % 4 == 0, x and y 8-byte aligned and "
                                   "y_batch_stride % 4 == 0 (use the library GEMM or convolution otherwise)",
                                   "conv1x1_bf16_fwd: launch failed"};
static const PwEntry kConv1x1Affine{kConv1x1, true,
                                    "conv1x1_bf16_fwd_affine: needs 1 <= Cin <= 1024, 1 <= Cout <= 512, P % 4 == 0, x and y 8-byte aligned "
                                    "and y_batch_stride % 4 == 0 (use the library GEMM or convolution + mgar_bn_act_fwd otherwise)",
                                    "conv1x1_bf16_fwd_affine: launch failed"};

// P: columns per sample (pooled: M * ns); ns 0 = an unpooled entry.  The store is plain where out_scale is NULL.
static int pw_forward(const PwEntry &e, const void *x, int B, int Cin, long long P, int ns, const float *w, int w_ld, int Cout,
                      const float *in_mean, const float *in_invstd, const float *in_gamma, const float *in_beta, int in_relu,
                      const float *out_scale, const float *out_shift, int out_relu, void *y, long long ybs, void *stream) {
    const PwFamily &f = e.family;
    MGAR_REQUIRE(B >= 0 && Cin >= 0 && Cout >= 0 && P >= 0, f.negative);
    const bool pool = ns != 0;
    const bool ns_ok = !pool || ns == 4 || ns == 8 || ns == 16 || ns == 32 || ns == 64 || ns == 128;
    if (ns_ok && (long long)B * P == 0) return MGAR_OK;
    if (!ns_ok || Cin < 1 || Cin > 1024 || Cout < 1 || Cout > 512 || (P & 3) != 0 || ((uintptr_t)x & 7) != 0 || ((uintptr_t)y & 7) != 0 ||
        w_ld < Cin || (!pool && (ybs & 3) != 0)) {
        set_error(e.unsupported);
        return MGAR_EUNSUPPORTED;
    }
    MGAR_REQUIRE(P <= 2147483647 - PW_COLS && (long long)B * ((P + PW_COLS - 1) / PW_COLS) <= (1LL << 30), f.tiles);
    MGAR_REQUIRE(x && w && y && (!e.needs_affine || (out_scale && out_shift)), f.null);
    MGAR_REQUIRE(in_mean == nullptr || in_invstd != nullptr, "pointwise_wide_bf16: in_mean without in_invstd");
    MGAR_REQUIRE((out_scale == nullptr) == (out_shift == nullptr), "pointwise_wide_bf16: out_scale and out_shift go together");
    MGAR_REQUIRE(!pool || out_scale != nullptr, "pointwise_wide_maxpool_bf16_fwd: out_scale and out_shift are required");
    MGAR_REQUIRE(pool || ybs >= (long long)Cout * P, f.ybs);
    PwArgs a{(const uint16_t *)x, w, out_scale, out_shift, (uint16_t *)y, ybs, B, Cin, Cout, (int)P, out_relu, w_ld,
             in_mean, in_invstd, in_gamma, in_beta, in_relu, ns};
    hipStream_t st = (hipStream_t)stream;
    const double cols = (double)B * (double)P;
    KtScope kt(f.kt, st, pool ? 2.0 * cols * Cin + 2.0 * (cols / ns) * Cout : 2.0 * cols * (Cin + Cout), 2.0 * cols * Cin * Cout);
    if (pool) {
        if (in_mean) launch_by_cout<true, EPI_POOLED>(a, st); else launch_by_cout<false, EPI_POOLED>(a, st);
    } else if (out_scale) {
        if (in_mean) launch_by_cout<true, EPI_AFFINE>(a, st); else launch_by_cout<false, EPI_AFFINE>(a, st);
    } else {
        if (in_mean) launch_by_cout<true, EPI_PLAIN>(a, st); else launch_by_cout<false, EPI_PLAIN>(a, st);
    }
    return check_launch(e.launch);
}

}  // namespace mgar

using namespace mgar;

MGAR_API int mgar_pointwise_wide_bf16_fwd(const void *x, int B, int Cin, int P, const float *w, int w_ld, int Cout,
                                          const float *in_mean, const float *in_invstd, const float *in_gamma, const float *in_beta,
                                          int in_relu, const float *out_scale, const float *out_shift, int out_relu, void *y,
                                          long long y_batch_stride, void *stream) {
    return pw_forward(kWideFwd, x, B, Cin, P, 0, w, w_ld, Cout, in_mean, in_invstd, in_gamma, in_beta, in_relu, out_scale, out_shift,
                      out_relu, y, y_batch_stride, stream);
}

MGAR_API int mgar_pointwise_wide_maxpool_bf16_fwd(const void *x, int B, int Cin, int M, int ns, const float *w, int w_ld, int Cout,
                                                  const float *in_mean, const float *in_invstd, const float *in_gamma,
                                                  const float *in_beta, int in_relu, const float *out_scale, const float *out_shift,
                                                  int out_relu, void *y, void *stream) {
    MGAR_REQUIRE(M >= 0 && ns >= 0, "pointwise_wide_maxpool_bf16_fwd: negative size");
    // ns 0 is not a group width: -1 keeps it out of the unpooled path of pw_forward
    return pw_forward(kWidePooled, x, B, Cin, (long long)M * (ns ? ns : 1), ns ? ns : -1, w, w_ld, Cout, in_mean, in_invstd, in_gamma,
                      in_beta, in_relu, out_scale, out_shift, out_relu, y, 0, stream);
}

// The I3D entries: identity prologue, W dense (w_ld = Cin)
MGAR_API int mgar_conv1x1_bf16_fwd(const void *x, int N, int Cin, int P, const float *w, int Cout, void *y, long long y_batch_stride,
                                   void *stream) {
    const float *none = nullptr;
    return pw_forward(kConv1x1Plain, x, N, Cin, P, 0, w, Cin, Cout, none, none, none, none, 0, none, none, 0, y, y_batch_stride, stream);
}

MGAR_API int mgar_conv1x1_bf16_fwd_affine(const void *x, int N, int Cin, int P, const float *w, int Cout, const float *scale,
                                          const float *shift, int relu, void *y, long long y_batch_stride, void *stream) {
    const float *none = nullptr;
    return pw_forward(kConv1x1Affine, x, N, Cin, P, 0, w, Cin, Cout, none, none, none, none, 0, scale, shift, relu, y, y_batch_stride,
                      stream);
}
