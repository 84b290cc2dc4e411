// conv3d_bf16.hip -- the 3x3x3, stride-1, "same"-padded convolutions of Inception-I3D (Conv3d_2c_3x3 and the Branch_1 /
// Branch_2 ``Conv3d_0b_3x3`` units of every Mixed block) for bf16 payloads, on the bf16 MFMA of gfx950
// (v_mfma_f32_32x32x16_bf16), NCDHW in and out, padding inside the kernel.  The bf16 forward configurations (c2, c5) run it
// where the fp32 step runs csrc/conv3d_wino.hip.
//
// Reference: model/backbone.py:134-206 (Unit3D: dynamic "same" padding + nn.Conv3d(bias=False)); instances :311-312
// (Conv3d_2c_3x3, 64 -> 192) and :215-236 (InceptionModule b1b / b2b).
//
// A DIRECT convolution, not minimal filtering: products of bf16 operands are exact in the fp32 accumulator, so the result is
// the fp32 sum of the exact products, rounded once to bf16 on store (round to nearest even) -- the contract of the other
// bf16-MFMA kernels (csrc/stem_conv.hip).  A Winograd input transform would have to be rounded to bf16 before the MFMA.
//
// Implicit GEMM D[co][pixel]: the MFMA rows are 32 output channels, the columns 32 output pixels (a PW x BH patch, PW * BH = 32),
// k runs over items (8-channel group, tap); one instruction takes two items (lane l holds k = 8 (l >> 5) + j, j = 0..7: half-wave
// h = the item, j = the channel inside the group).  A channel group has 27 taps = 13 1/2 instructions: a 28th item with zero
// weights fills the 14th.  A wave owns 2 channel blocks x 2 pixel blocks (4 accumulators, 64 registers); the 4 waves of a
// workgroup stack their pixel blocks along H and share the filter block: tile = 64 channels x PW x (256 / PW) outputs.
//
// Per channel group the workgroup stages in LDS
//   * the 3 x (TH + 2) x (TW + 4) halo tile with the 8 channels of the group innermost (16 bytes per pixel): a lane's B fragment is
//     one ds_read_b128, and all 27 taps read the same staged tile at shifted addresses;
//   * the packed filter block [step 14][channel block 2][half 2][co 32][ci 8] (conv3d_bf16_pack_kernel): an A fragment is one
//     ds_read_b128, a wave's read 1 KB contiguous.
// 4 reads feed 4 MFMAs.  Both are double-buffered: the next group's global loads are issued before the current group's 56 MFMAs per
// wave and stored to the other buffer after them.  The tile is gathered from the 8 channel planes as aligned PAIRS of pixels
// (one 4-byte load = columns 2i, 2i + 1 of one channel; W is even) through a raw buffer resource over the 8 planes: the offset
// of a pair outside the volume is out of the resource's range and reads 0 -- the zero padding costs no select.
//
// No atomics, no cross-sample state: sample n's output does not depend on N, and two launches give the same bits.
// Workgroups are numbered so that the channel groups of one spatial tile and the tiles next to it run on the same XCD.
#include "common.hpp"
#include "payload.hpp"

namespace mgar {

constexpr int CB_CG = 64;                              // output channels per workgroup (2 MFMA row blocks)
constexpr int CB_CI = 8;                               // input channels per group (the k of one item)
constexpr int CB_STEPS = 14;                           // MFMA k-steps per group: 27 taps + one zero item
constexpr int CB_W_VEC = CB_STEPS * 2 * 2 * 32;        // 16-byte vectors of one packed filter block: [step][mb][half][co 32] = 1792
constexpr int CB_W_PER_THREAD = CB_W_VEC / 256;        // 7
constexpr unsigned CB_OUTSIDE = 0x80000000u;           // byte offset of a padding pair: beyond any resource this kernel makes

template <int PW>
struct CbGeom {
    static constexpr int BH = 32 / PW;                 // rows of a pixel block
    static constexpr int TW = PW, TH = 8 * BH;         // outputs per workgroup tile (w, h)
    static constexpr int IH = TH + 2;                  // halo rows
    static constexpr int IWP = TW + 4;                 // halo columns w0 - 2 .. w0 + TW + 1: whole aligned pairs
    static constexpr int HP = IWP / 2;                 // pairs per row
    static constexpr int SLOTS = 3 * IH * HP;          // pairs per channel
    static constexpr int ROUNDS = (SLOTS + 255) / 256;
    static constexpr int IN_VEC = 3 * IH * IWP + 2;    // 16-byte vectors per buffer; the last two take the stores of idle staging slots
    static constexpr int tap_off(int t) { return ((t / 9) * IH + (t / 3) % 3) * IWP + t % 3 + 1; }
};

struct CbArgs {
    int N, Cin, D, H, W, Cout, ncg, cg0, tiles_w, tiles_h, per_xcd;   // this launch: channel groups cg0 .. cg0 + ncg - 1
    long long total;
};

struct CbEpilogue {                                    // mgar_conv3d_k3_bf16_fwd_affine: scale, shift (Cout), the ReLU flag, elements between samples of y
    const float *scale, *shift;
    int relu;
    long long y_batch_stride;
};

// wp: [cg][c_in group][step 14][mb 2][half 2][co 32][ci 8] bf16 (conv3d_bf16_pack_kernel)
// NMB: 32-channel blocks per workgroup that exist (2; 1 for a tail group of <= 32 channels, launched separately)
// AFF: the store applies conv_affine to the fp32 accumulator BEFORE the one rounding, with the channel's scale / shift, and sample n
// starts at y + n * e.y_batch_stride (a channel slice of a wider tensor).  The store loop runs channel block by channel block and
// loads the block's 16 scale / shift values at the head of its pass (32 independent loads behind one wait, shared by both pixel
// blocks; not a load-to-store dependency per element); the plain instantiations keep their loop and read nothing of `e`.
template <int PW, int NMB, bool AFF>
__global__ __launch_bounds__(256) void conv3d_bf16_kernel(const uint16_t *__restrict__ x, const u32x4 *__restrict__ wp, CbArgs a,
                                                          CbEpilogue e, uint16_t *__restrict__ y) {
    typedef CbGeom<PW> G;
    __shared__ __attribute__((aligned(16))) u32x4 s_in[2][G::IN_VEC];
    __shared__ __attribute__((aligned(16))) u32x4 s_w[2][CB_W_VEC];

    // XCD-aware numbering: hardware workgroup b runs on XCD b % 8; logical ids are contiguous per XCD
    const long long logical = (long long)(blockIdx.x & 7) * a.per_xcd + (blockIdx.x >> 3);
    if (logical >= a.total) return;
    int rest = (int)logical;
    const int cg = a.cg0 + rest % a.ncg; rest /= a.ncg;
    const int bx = rest % a.tiles_w; rest /= a.tiles_w;
    const int by = rest % a.tiles_h; rest /= a.tiles_h;
    const int d = rest % a.D, n = rest / a.D;
    const int w0 = bx * G::TW, h0 = by * G::TH;

    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int l = lane & 31, half = lane >> 5;

    const int HW = a.H * a.W;
    const long long DHW = (long long)a.D * HW;
    const unsigned plane_bytes = (unsigned)(2 * DHW);
    // staging slots of this thread: one aligned pixel pair each, all 8 channels of the group.  Byte offset of the pair inside a
    // channel plane (CB_OUTSIDE: padding, or an idle slot) and its place in the LDS tile.
    unsigned off[G::ROUNDS];
    int pos[G::ROUNDS];
#pragma unroll
    for (int u = 0; u < G::ROUNDS; ++u) {
        const int e = threadIdx.x + u * 256;
        const int dz = e / (G::IH * G::HP), r1 = e - dz * (G::IH * G::HP);
        const int iy = r1 / G::HP, ip = r1 - iy * G::HP;
        const int dd = d - 1 + dz, hh = h0 - 1 + iy, ww = w0 - 2 + 2 * ip;
        const bool ok = e < G::SLOTS && dd >= 0 && dd < a.D && hh >= 0 && hh < a.H && ww >= 0 && ww < a.W;
        off[u] = ok ? 2u * (unsigned)(dd * HW + hh * a.W + ww) : CB_OUTSIDE;
        pos[u] = e < G::SLOTS ? (dz * G::IH + iy) * G::IWP + 2 * ip : G::IN_VEC - 2;
    }
    const uint16_t *xin = x + (long long)n * a.Cin * DHW;
    const int group_bytes = (int)(2 * CB_CI * DHW);
    const int ngroup = a.Cin / CB_CI;
    const u32x4 *wsrc = wp + (long long)cg * ngroup * CB_W_VEC;

    f32x16 acc[NMB][2];
#pragma unroll
    for (int mb = 0; mb < NMB; ++mb)
#pragma unroll
        for (int nb = 0; nb < 2; ++nb)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[mb][nb][r] = 0.f;

    unsigned pin[G::ROUNDS][CB_CI];                    // a pixel pair of one channel each (low half: the even column)
    u32x4 pw4[CB_W_PER_THREAD];
    auto fetch = [&](int g) {                          // global -> registers: channel group g; nothing here waits for a load
        const __amdgpu_buffer_rsrc_t src = uniform_buffer(xin + (long long)(CB_CI * g) * DHW, group_bytes);
#pragma unroll
        for (int u = 0; u < G::ROUNDS; ++u)
#pragma unroll
            for (int c = 0; c < CB_CI; ++c)
                pin[u][c] = (unsigned)__builtin_amdgcn_raw_buffer_load_b32(src, (int)(off[u] + (unsigned)c * plane_bytes), 0, 0);
        const u32x4 *ws = wsrc + (long long)g * CB_W_VEC;
#pragma unroll
        for (int u = 0; u < CB_W_PER_THREAD; ++u) pw4[u] = ws[threadIdx.x + u * 256];
    };
    auto stash = [&](int buf) {                        // registers -> LDS: the 8 channels of a pixel become its 16 bytes
#pragma unroll
        for (int u = 0; u < G::ROUNDS; ++u) {
            u32x4 p0, p1;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const unsigned c0 = pin[u][2 * k], c1 = pin[u][2 * k + 1];
                p0[k] = (c0 & 0xffffu) | (c1 << 16);
                p1[k] = (c0 >> 16) | (c1 & 0xffff0000u);
            }
            s_in[buf][pos[u]] = p0;
            s_in[buf][pos[u] + 1] = p1;
        }
#pragma unroll
        for (int u = 0; u < CB_W_PER_THREAD; ++u) s_w[buf][threadIdx.x + u * 256] = pw4[u];
    };

    fetch(0);
    stash(0);
    __syncthreads();
    // lane constants: output pixel (row, column) of pixel block 0 inside the tile; block 1 lies BH rows below
    const int prow = (2 * wave) * G::BH + l / PW, pcol = l % PW;
    const int b_lane = prow * G::IWP + pcol;
    const int a_lane = half * 32 + l;
    for (int g = 0; g < ngroup; ++g) {
        const int buf = g & 1;
        // the next group's global loads are in flight under the MFMAs below (the last iteration re-loads its own group: one
        // unconditional straight-line body)
        fetch(min(g + 1, ngroup - 1));
        __builtin_amdgcn_sched_barrier(0);
        const u32x4 *ti = s_in[buf] + b_lane;
        const u32x4 *tw = s_w[buf] + a_lane;
        // operands of k-step s + 1 are read from LDS before the MFMAs of k-step s are issued
        u32x4 fa[2][NMB], fb[2][2];
        auto read_operands = [&](int s, int slot) {
            // this half-wave's item: tap 2 s + half (item 27 has zero weights: it reads tap 26's pixels)
            const int t0 = G::tap_off(2 * s), t1 = G::tap_off(2 * s + 1 < 27 ? 2 * s + 1 : 26);
            const int o = half ? t1 : t0;
#pragma unroll
            for (int nb = 0; nb < 2; ++nb) fb[slot][nb] = ti[o + nb * G::BH * G::IWP];
#pragma unroll
            for (int mb = 0; mb < NMB; ++mb) fa[slot][mb] = tw[(s * 2 + mb) * 64];
        };
        read_operands(0, 0);
#pragma unroll
        for (int s = 0; s < CB_STEPS; ++s) {
            const int slot = s & 1;
            if (s + 1 < CB_STEPS) read_operands(s + 1, slot ^ 1);
#pragma unroll
            for (int mb = 0; mb < NMB; ++mb)
#pragma unroll
                for (int nb = 0; nb < 2; ++nb)
                    acc[mb][nb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, fa[slot][mb]),
                                                                          __builtin_bit_cast(bf16x8, fb[slot][nb]), acc[mb][nb], 0, 0, 0);
        }
        __builtin_amdgcn_sched_barrier(0);
        stash(buf ^ 1);                                // the other buffer: its last readers passed the barrier of group g - 1
        __syncthreads();
    }

    // store: register r of a lane is (co = 32 mb + (r & 3) + 8 (r >> 2) + 4 half, pixel l); one rounding, fp32 -> bf16
    const int wo = w0 + pcol;
    if constexpr (AFF) {
#pragma unroll
        for (int mb = 0; mb < NMB; ++mb) {
            float sc[16], sh[16];
#pragma unroll
            for (int r = 0; r < 16; ++r) {                 // (a channel beyond Cout reads the last one's: never stored)
                const int cc = min(cg * CB_CG + mb * 32 + (r & 3) + 8 * (r >> 2) + 4 * half, a.Cout - 1);
                sc[r] = e.scale[cc];
                sh[r] = e.shift[cc];
            }
#pragma unroll
            for (int nb = 0; nb < 2; ++nb) {
                const int ho = h0 + prow + nb * G::BH;
                if (ho >= a.H || wo >= a.W) continue;
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int co = cg * CB_CG + mb * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
                    if (co >= a.Cout) continue;
                    const float v = conv_affine(acc[mb][nb][r], sc[r], sh[r], e.relu);
                    y[(long long)n * e.y_batch_stride + ((long long)co * a.D + d) * HW + (long long)ho * a.W + wo] =
                        (uint16_t)(pack_bf16x2(v, 0.f) & 0xffffu);
                }
            }
        }
    } else {
#pragma unroll
        for (int nb = 0; nb < 2; ++nb) {
            const int ho = h0 + prow + nb * G::BH;
            if (ho >= a.H || wo >= a.W) continue;
#pragma unroll
            for (int mb = 0; mb < NMB; ++mb) {
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int co = cg * CB_CG + mb * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
                    if (co >= a.Cout) continue;
                    y[(((long long)n * a.Cout + co) * a.D + d) * HW + (long long)ho * a.W + wo] =
                        (uint16_t)(pack_bf16x2(acc[mb][nb][r], 0.f) & 0xffffu);
                }
            }
        }
    }
}

// w (Cout, Cin, 3, 3, 3) fp32 -> wp [cg][c_in group][step 14][mb 2][half 2][co 32][ci 8] bf16 (round to nearest even); item
// 2 step + half = 27 and channels beyond Cout are zero
__global__ void conv3d_bf16_pack_kernel(const float *__restrict__ w, int Cin, int Cout, long long total, uint16_t *__restrict__ wp) {
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= total) return;
    const int j = (int)(e & 7), col = (int)(e >> 3) & 31, half = (int)(e >> 8) & 1, mb = (int)(e >> 9) & 1;
    long long rest = e >> 10;
    const int s = (int)(rest % CB_STEPS); rest /= CB_STEPS;
    const int ngroup = Cin / CB_CI;
    const int g = (int)(rest % ngroup), cg = (int)(rest / ngroup);
    const int item = 2 * s + half, co = cg * CB_CG + mb * 32 + col, ci = g * CB_CI + j;
    float v = 0.f;
    if (item < 27 && co < Cout) v = w[((long long)co * Cin + ci) * 27 + item];
    wp[e] = (uint16_t)(pack_bf16x2(v, 0.f) & 0xffffu);
}

template <int PW, bool AFF>
static void cb_launch(const uint16_t *x, const u32x4 *wp, CbArgs a, CbEpilogue e, uint16_t *y, hipStream_t st) {
    typedef CbGeom<PW> G;
    a.tiles_w = ceil_div(a.W, G::TW);
    a.tiles_h = ceil_div(a.H, G::TH);
    const int groups = ceil_div(a.Cout, CB_CG);
    const int tail = (a.Cout % CB_CG != 0 && a.Cout % CB_CG <= 32) ? 1 : 0;      // a last group with one 32-channel block
    const long long tiles = (long long)a.tiles_w * a.tiles_h * a.D * a.N;
    if (groups - tail > 0) {
        a.cg0 = 0; a.ncg = groups - tail;
        a.total = tiles * a.ncg;
        a.per_xcd = (int)((a.total + 7) / 8);
        hipLaunchKernelGGL((conv3d_bf16_kernel<PW, 2, AFF>), dim3(a.per_xcd * 8), dim3(256), 0, st, x, wp, a, e, y);
    }
    if (tail) {
        a.cg0 = groups - 1; a.ncg = 1;
        a.total = tiles;
        a.per_xcd = (int)((a.total + 7) / 8);
        hipLaunchKernelGGL((conv3d_bf16_kernel<PW, 1, AFF>), dim3(a.per_xcd * 8), dim3(256), 0, st, x, wp, a, e, y);
    }
}

}  // namespace mgar

using namespace mgar;

// bytes of the packed-filter scratch mgar_conv3d_k3_bf16_fwd needs (rewritten on every call): 28 672 per (64 output channels,
// 8 input channels)
MGAR_API long long mgar_conv3d_k3_bf16_workspace_bytes(int Cin, int Cout) {
    if (Cin <= 0 || Cout <= 0) return 0;
    return (long long)ceil_div(Cout, CB_CG) * ceil_div(Cin, CB_CI) * CB_W_VEC * 16;
}

// The two entry points below: AFF = false, mgar_conv3d_k3_bf16_fwd (e unused); AFF = true, mgar_conv3d_k3_bf16_fwd_affine.  Same
// packing, same tile choice, same timer row.
template <bool AFF>
static int cb_forward(const char *who, const void *x, int N, int Cin, int D, int H, int W, const float *w, int Cout, void *w_packed,
                      CbEpilogue e, void *y, void *stream) {
    hipStream_t st = (hipStream_t)stream;
    CbArgs a{N, Cin, D, H, W, Cout, ceil_div(Cout, CB_CG), 0, 0, 0, 0, 0};
    const long long wtotal = (long long)a.ncg * (Cin / CB_CI) * CB_W_VEC * 8;    // bf16 elements
    hipLaunchKernelGGL(conv3d_bf16_pack_kernel, dim3(ceil_div(wtotal, 256)), dim3(256), 0, st, w, Cin, Cout, wtotal, (uint16_t *)w_packed);
    // the tile shape that wastes the fewest outputs (ties: the widest rows)
    auto padded = [&](int pw) { return (long long)ceil_div(W, pw) * pw * ceil_div(H, 256 / pw) * (256 / pw); };
    int best = 32;
    if (padded(16) < padded(best)) best = 16;
    if (padded(8) < padded(best)) best = 8;
    const double outs = (double)N * D * H * W;
    {
        // bytes: input + output once at 2 B per element; flops: the direct convolution's 2 * 27 * Cin * Cout per output
        KtScope kt(KT_CONV3D_BF16, st, 2.0 * outs * (Cin + Cout), 2.0 * 27.0 * outs * Cin * Cout);
        const uint16_t *xp = (const uint16_t *)x;
        const u32x4 *wv = (const u32x4 *)w_packed;
        uint16_t *yp = (uint16_t *)y;
        if (best == 32) cb_launch<32, AFF>(xp, wv, a, e, yp, st);
        else if (best == 16) cb_launch<16, AFF>(xp, wv, a, e, yp, st);
        else cb_launch<8, AFF>(xp, wv, a, e, yp, st);
    }
    return check_launch(who);
}

// x (N, Cin, D, H, W) bf16 NCDHW, w (Cout, Cin, 3, 3, 3) fp32 -> y (N, Cout, D, H, W) bf16: stride 1, zero padding 1 on every
// side.  Cin % 8 == 0 and even W (every I3D instance); anything else is MGAR_EINVAL and the caller keeps the library convolution.
MGAR_API int mgar_conv3d_k3_bf16_fwd(const void *x, int N, int Cin, int D, int H, int W, const float *w, int Cout, void *w_packed,
                                     void *y, void *stream) {
    MGAR_REQUIRE(N >= 0 && Cin > 0 && Cout > 0 && D > 0 && H > 0 && W > 0, "conv3d_k3_bf16_fwd: bad sizes");
    MGAR_REQUIRE(Cin % CB_CI == 0 && W % 2 == 0, "conv3d_k3_bf16_fwd: Cin must be a multiple of 8 and W even");
    if (N == 0) return MGAR_OK;
    MGAR_REQUIRE(x && w && w_packed && y, "conv3d_k3_bf16_fwd: null pointer");
    MGAR_REQUIRE(((uintptr_t)x & 3) == 0 && ((uintptr_t)y & 1) == 0 && ((uintptr_t)w_packed & 15) == 0,
                 "conv3d_k3_bf16_fwd: x must be 4-byte, w_packed 16-byte aligned");
    MGAR_REQUIRE((long long)2 * CB_CI * D * H * W < (1ll << 31), "conv3d_k3_bf16_fwd: volume too large for 32-bit tile offsets");
    MGAR_REQUIRE((long long)ceil_div(Cout, CB_CG) * ceil_div(W, 8) * ceil_div(H, 8) * D * N < (1ll << 30), "conv3d_k3_bf16_fwd: too many tiles");
    return cb_forward<false>("conv3d_k3_bf16_fwd: launch failed", x, N, Cin, D, H, W, w, Cout, w_packed, CbEpilogue{nullptr, nullptr, 0, 0}, y, stream);
}

// mgar_conv3d_k3_bf16_fwd with the eval-mode BatchNorm [+ ReLU] epilogue applied to the fp32 accumulator before the one rounding:
// y = bf16(conv_affine(acc, scale[co], shift[co], relu)).  scale, shift (Cout) fp32, both required; y_batch_stride in ELEMENTS
// (>= Cout * D * H * W, even) as in mgar_conv3d_k3_fwd_affine: y may be a channel slice of a wider contiguous NCDHW tensor.
MGAR_API int mgar_conv3d_k3_bf16_fwd_affine(const void *x, int N, int Cin, int D, int H, int W, const float *w, int Cout, void *w_packed,
                                            const float *scale, const float *shift, int relu, void *y, long long y_batch_stride,
                                            void *stream) {
    MGAR_REQUIRE(N >= 0 && Cin > 0 && Cout > 0 && D > 0 && H > 0 && W > 0, "conv3d_k3_bf16_fwd_affine: bad sizes");
    MGAR_REQUIRE(Cin % CB_CI == 0 && W % 2 == 0, "conv3d_k3_bf16_fwd_affine: Cin must be a multiple of 8 and W even");
    if (N == 0) return MGAR_OK;
    MGAR_REQUIRE(x && w && w_packed && scale && shift && y, "conv3d_k3_bf16_fwd_affine: null pointer");
    MGAR_REQUIRE(((uintptr_t)x & 3) == 0 && ((uintptr_t)y & 1) == 0 && ((uintptr_t)w_packed & 15) == 0,
                 "conv3d_k3_bf16_fwd_affine: x must be 4-byte, y 2-byte, w_packed 16-byte aligned");
    MGAR_REQUIRE(y_batch_stride % 2 == 0 && y_batch_stride >= (long long)Cout * D * H * W,
                 "conv3d_k3_bf16_fwd_affine: y_batch_stride must be even and at least Cout * D * H * W");
    MGAR_REQUIRE((long long)2 * CB_CI * D * H * W < (1ll << 31), "conv3d_k3_bf16_fwd_affine: volume too large for 32-bit tile offsets");
    MGAR_REQUIRE((long long)ceil_div(Cout, CB_CG) * ceil_div(W, 8) * ceil_div(H, 8) * D * N < (1ll << 30), "conv3d_k3_bf16_fwd_affine: too many tiles");
    return cb_forward<true>("conv3d_k3_bf16_fwd_affine: launch failed", x, N, Cin, D, H, W, w, Cout, w_packed,
                            CbEpilogue{scale, shift, relu ? 1 : 0, y_batch_stride}, y, stream);
}
