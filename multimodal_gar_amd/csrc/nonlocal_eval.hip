// nonlocal_eval.hip -- the eval-mode non-local block (NLBlockND, mode 'dot') as ONE kernel per call, BatchNorm folded.
//
// Per sample a, with x_a a (C, P) matrix (element (c, p) at x + a sx_n + c sx_c + p sx_p):
//     [T; Phi; G] = W_tpg x + b_tpg            (3 Ci, P)    phase 1, K = C
//     S = G Phi^T / P                          (Ci, Ci)     phase 2, K = P     'dot' has no softmax: the (P, P) matrix is never formed
//     Y = S T                                  (Ci, P)      phase 3, K = Ci
//     z = fma(W_z Y + b_z, scale, shift) + x   (C, P)       phase 4, K = Ci
// One workgroup of 8 waves per sample; T, Phi, G, S and Y live in LDS only; x is streamed once from HBM through a 32-channel
// LDS stage (phase 1) and read a second time, from cache, for the residual (phase 4).  No workspace, no atomics.
// Every product is v_mfma_f32_32x32x2_f32 (exact fp32, a k-ordered fmaf chain), tiles of 32 x 32 with zero-masked tails.  The k
// order of a tile is fixed by (C, Ci, P) alone, so a sample's bits depend on that sample and the parameters only.
#include "common.hpp"
#include "payload.hpp"

namespace mgar {

constexpr int NL_WAVES = 8, NL_THREADS = NL_WAVES * kWave;
constexpr int NL_KC = 32;          // channels of x per LDS stage
constexpr int NL_PRE = 16;         // staged elements per lane: NL_KC * 256 positions / NL_THREADS
constexpr int NL_MAX_TPW = 3;      // projection tiles whose accumulators one wave keeps over the K loop
constexpr int NL_MAX_LDS = 160 * 1024;

// Tiling and LDS layout of one (C, Ci, P); computed on the host, passed by value.  Pitches are odd: a fragment whose lanes walk
// rows reads conflict-free.
struct NlPlan {
    int MT, NT, ST, CT;   // 32-row tiles of 3 Ci, 32-column tiles of P, 32-row tiles of Ci and of C
    int PT, SP, XP;       // pitch of a T / Phi / G / Y row, of an S row, of a staged x row (floats)
    int nsplit;           // phase 2: parts the sum over P is cut into, one wave each (added in part order)
    int tpw;              // projection tiles per wave
    int lds_floats;
    int xvec, wvec, zvec; // 4-element loads of x rows (sx_c == 1) / of w_tpg rows / of w_z rows are aligned
};

static NlPlan nl_plan(int C, int Ci, int P) {
    NlPlan p{};
    p.MT = (3 * Ci + 31) / 32; p.NT = (P + 31) / 32; p.ST = (Ci + 31) / 32; p.CT = (C + 31) / 32;
    p.PT = P | 1; p.SP = Ci | 1; p.XP = p.NT * 32 + 1;
    const int t2 = p.ST * p.ST;
    p.nsplit = t2 >= NL_WAVES ? 1 : NL_WAVES / t2;
    p.tpw = (p.MT * p.NT + NL_WAVES - 1) / NL_WAVES;
    const int r2a = NL_KC * p.XP, r2b = p.nsplit * Ci * p.SP;
    p.lds_floats = 3 * Ci * p.PT + (r2a > r2b ? r2a : r2b);
    return p;
}

static bool nl_supported(int C, int Ci, int P) {
    if (C < 1 || Ci < 1 || P < 1 || C > 1024 || Ci > 128 || P > 256 || (long long)Ci * P > 4096) return false;
    const NlPlan p = nl_plan(C, Ci, P);
    return p.tpw <= NL_MAX_TPW && p.lds_floats * 4 <= NL_MAX_LDS;
}

// D[row][col = lane & 31] of a 32 x 32 accumulator: register r of lane half h holds this row
__device__ __forceinline__ int nl_row(int r, int h) { return (r & 3) + 8 * (r >> 2) + 4 * h; }

// W[row][k0 .. k0 + 3] of a row-major (M, K) matrix, zero outside it.  vec: K % 4 == 0 and W 16-byte aligned (k0 % 4 == 0 always).
__device__ __forceinline__ float4 nl_w4(const float *__restrict__ W, int row, int M, int k0, int K, bool vec) {
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (row < M && k0 < K) {
        const float *p = W + (size_t)row * K + k0;
        if (vec) {
            v = *reinterpret_cast<const float4 *>(p);
        } else {
            v.x = p[0];
            if (k0 + 1 < K) v.y = p[1];
            if (k0 + 2 < K) v.z = p[2];
            if (k0 + 3 < K) v.w = p[3];
        }
    }
    return v;
}

#define NL_MFMA(a, b, c) __builtin_amdgcn_mfma_f32_32x32x2f32((a), (b), (c), 0, 0, 0)

template <typename T, int TPW>
__global__ __launch_bounds__(NL_THREADS, TPW == 1 ? 4 : 2) void nonlocal_dot_eval_kernel(const T *__restrict__ x, long long sx_n, long long sx_c,
                                                                       long long sx_p, int C, int Ci, int P,
                                                                       const float *__restrict__ w_tpg, const float *__restrict__ b_tpg,
                                                                       const float *__restrict__ w_z, const float *__restrict__ b_z,
                                                                       const float *__restrict__ scale, const float *__restrict__ shift,
                                                                       T *__restrict__ z, NlPlan pl) {
    extern __shared__ __attribute__((aligned(16))) float nl_lds[];
    float *tpg = nl_lds;                       // rows [0, Ci) T, [Ci, 2 Ci) Phi then Y, [2 Ci, 3 Ci) G
    float *r2 = nl_lds + 3 * Ci * pl.PT;       // the x stage, then S (and its partial sums)
    const int tid = threadIdx.x, lane = tid & 63, li = lane & 31, lh = lane >> 5;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const T *xa = x + (long long)blockIdx.x * sx_n;
    const int PT = pl.PT, SP = pl.SP, XP = pl.XP, NT = pl.NT, M1 = 3 * Ci;

    // ---- phase 1: [T; Phi; G] = W_tpg x + b.  A fragments from global (a lane takes 4 consecutive k: lane half h of the q-th
    // 8-block of a stage holds k = 8 q + 4 h .. + 3), B from the staged x rows in the same k order.
    {
        f32x16 acc[TPW];
#pragma unroll
        for (int t = 0; t < TPW; ++t)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;
        const int n1 = pl.MT * NT;
        // Element i of a lane's share of a stage is channel k0 + dk (i & 3), position p0 + dp (i & 3) + 64 (i >> 2): in the rows layout
        // (sx_c == 1) consecutive lanes take consecutive channels, otherwise consecutive positions.  Channels >= C are staged as
        // zeros: 0 * stale LDS could be a NaN.
        const bool cfast = sx_c == 1;
        const int k0 = cfast ? li : wave, p0 = cfast ? lh + 2 * wave : lane, dk = cfast ? 0 : 8, dp = cfast ? 16 : 0;
        const long long step_a = dk * sx_c + dp * sx_p, step_b = 64 * sx_p;
        const T *xl = xa + k0 * sx_c + p0 * sx_p;
        float pre[NL_PRE];
        auto fetch = [&](int kc) {
            const T *xk = xl + kc * sx_c;
#pragma unroll
            for (int i = 0; i < NL_PRE; ++i) {
                const int k = k0 + dk * (i & 3), p = p0 + dp * (i & 3) + 64 * (i >> 2);
                pre[i] = (p < P && kc + k < C) ? Payload<T>::ld(xk + (i & 3) * step_a + (i >> 2) * step_b) : 0.f;
            }
        };
        fetch(0);
        for (int kc = 0; kc < C; kc += NL_KC) {
            float4 a[TPW][4];
#pragma unroll
            for (int t = 0; t < TPW; ++t) {
                const int tile = wave + t * NL_WAVES;
#pragma unroll
                for (int q = 0; q < 4; ++q)
                    a[t][q] = tile < n1 ? nl_w4(w_tpg, (tile / NT) * 32 + li, M1, kc + 8 * q + 4 * lh, C, pl.wvec != 0)
                                        : make_float4(0.f, 0.f, 0.f, 0.f);
            }
#pragma unroll
            for (int i = 0; i < NL_PRE; ++i) {
                const int k = k0 + dk * (i & 3), p = p0 + dp * (i & 3) + 64 * (i >> 2);
                if (p < P) r2[k * XP + p] = pre[i];
            }
            __syncthreads();
            if (kc + NL_KC < C) fetch(kc + NL_KC);      // in flight under this stage's MFMAs
#pragma unroll
            for (int t = 0; t < TPW; ++t) {
                const int tile = wave + t * NL_WAVES;
                if (tile < n1) {
                    const float *b = r2 + 4 * lh * XP + (tile % NT) * 32 + li;   // columns >= P hold stale values: their D columns are dropped
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        acc[t] = NL_MFMA(a[t][q].x, b[(8 * q + 0) * XP], acc[t]);
                        acc[t] = NL_MFMA(a[t][q].y, b[(8 * q + 1) * XP], acc[t]);
                        acc[t] = NL_MFMA(a[t][q].z, b[(8 * q + 2) * XP], acc[t]);
                        acc[t] = NL_MFMA(a[t][q].w, b[(8 * q + 3) * XP], acc[t]);
                    }
                }
            }
            __syncthreads();
        }
#pragma unroll
        for (int t = 0; t < TPW; ++t) {
            const int tile = wave + t * NL_WAVES;
            if (tile < n1) {
                const int col = (tile % NT) * 32 + li;
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int row = (tile / NT) * 32 + nl_row(r, lh);
                    if (row < M1 && col < P) tpg[row * PT + col] = acc[t][r] + b_tpg[row];
                }
            }
        }
    }
    __syncthreads();

    // ---- phase 2: S[j][i] = (sum_p G[j][p] Phi[i][p]) / P.  Fewer tiles than waves: the sum over p is cut into nsplit parts.
    {
        const int ST = pl.ST, nsplit = pl.nsplit, steps = (P + 1) / 2, seg = (steps + nsplit - 1) / nsplit;
        const float fp = (float)P;
        for (int u = wave; u < ST * ST * nsplit; u += NL_WAVES) {
            const int tile = u / nsplit, part = u - tile * nsplit;
            const int rj = (tile / ST) * 32 + li, ri = (tile % ST) * 32 + li;
            const float *ga = tpg + (2 * Ci + (rj < Ci ? rj : 0)) * PT, *pb = tpg + (Ci + (ri < Ci ? ri : 0)) * PT;
            f32x16 acc;
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[r] = 0.f;
            const int s1 = min(steps, (part + 1) * seg);
            for (int s = part * seg; s < s1; ++s) {
                const int p = 2 * s + lh;
                const float av = (rj < Ci && p < P) ? ga[p] : 0.f, bv = (ri < Ci && p < P) ? pb[p] : 0.f;
                acc = NL_MFMA(av, bv, acc);
            }
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int j = (tile / ST) * 32 + nl_row(r, lh);
                if (j < Ci && ri < Ci) r2[(part * Ci + j) * SP + ri] = nsplit == 1 ? acc[r] / fp : acc[r];
            }
        }
        __syncthreads();
        if (nsplit > 1) {
            for (int e = tid; e < Ci * Ci; e += NL_THREADS) {
                const int j = e / Ci, i = e - j * Ci;
                float s = r2[j * SP + i];
                for (int part = 1; part < nsplit; ++part) s += r2[(part * Ci + j) * SP + i];
                r2[j * SP + i] = s / fp;
            }
            __syncthreads();
        }
    }

    // ---- phase 3: Y = S T, written over Phi
    for (int tile = wave; tile < pl.ST * NT; tile += NL_WAVES) {
        const int rj = (tile / NT) * 32 + li, col = (tile % NT) * 32 + li;
        const float *sa = r2 + (rj < Ci ? rj : 0) * SP, *tb = tpg + (col < P ? col : 0);
        f32x16 acc;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = 0.f;
        for (int s = 0; s < (Ci + 1) / 2; ++s) {
            const int k = 2 * s + lh;
            const bool kin = k < Ci;
            const float av = (rj < Ci && kin) ? sa[k] : 0.f, bv = (col < P && kin) ? tb[k * PT] : 0.f;
            acc = NL_MFMA(av, bv, acc);
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int j = (tile / NT) * 32 + nl_row(r, lh);
            if (j < Ci && col < P) tpg[(Ci + j) * PT + col] = acc[r];
        }
    }
    __syncthreads();

    // ---- phase 4: z = fma(W_z Y + b_z, scale, shift) + x
    const float *yb = tpg + Ci * PT;
    T *za = z + (size_t)blockIdx.x * C * P;
    for (int tile = wave; tile < pl.CT * NT; tile += NL_WAVES) {
        const int c0 = (tile / NT) * 32, col = (tile % NT) * 32 + li;
        const float *b = yb + (col < P ? col : 0);
        f32x16 acc;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = 0.f;
        float4 a = nl_w4(w_z, c0 + li, C, 4 * lh, Ci, pl.zvec != 0);
        for (int kb = 0; kb < Ci; kb += 8) {
            const float4 an = nl_w4(w_z, c0 + li, C, kb + 8 + 4 * lh, Ci, pl.zvec != 0);   // zero past Ci
            const int k = kb + 4 * lh;
            const bool cin = col < P;
            acc = NL_MFMA(a.x, (cin && k + 0 < Ci) ? b[(k + 0) * PT] : 0.f, acc);
            acc = NL_MFMA(a.y, (cin && k + 1 < Ci) ? b[(k + 1) * PT] : 0.f, acc);
            acc = NL_MFMA(a.z, (cin && k + 2 < Ci) ? b[(k + 2) * PT] : 0.f, acc);
            acc = NL_MFMA(a.w, (cin && k + 3 < Ci) ? b[(k + 3) * PT] : 0.f, acc);
            a = an;
        }
        if (col >= P) continue;
        if (pl.xvec) {      // rows layout: the four channels of a register group are one aligned load
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int c = c0 + 8 * g + 4 * lh;
                if (c < C) {
                    const float4 xv = Payload<T>::ld4(xa + c + (long long)col * sx_p);
                    const float xr[4] = {xv.x, xv.y, xv.z, xv.w};
#pragma unroll
                    for (int i = 0; i < 4; ++i)
                        Payload<T>::st(za + (size_t)(c + i) * P + col,
                                       __builtin_fmaf(acc[4 * g + i] + b_z[c + i], scale[c + i], shift[c + i]) + xr[i]);
                }
            }
        } else {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int c = c0 + nl_row(r, lh);
                if (c < C)
                    Payload<T>::st(za + (size_t)c * P + col, __builtin_fmaf(acc[r] + b_z[c], scale[c], shift[c]) +
                                                                 Payload<T>::ld(xa + (long long)c * sx_c + (long long)col * sx_p));
            }
        }
    }
}

template <typename T, int TPW>
static void nl_launch(int n, const T *x, long long sx_n, long long sx_c, long long sx_p, int C, int Ci, int P, const float *w_tpg,
                      const float *b_tpg, const float *w_z, const float *b_z, const float *scale, const float *shift, T *z,
                      const NlPlan &pl, hipStream_t st) {
    static bool attr_set = false;
    if (!attr_set) {
        (void)hipFuncSetAttribute((const void *)nonlocal_dot_eval_kernel<T, TPW>, hipFuncAttributeMaxDynamicSharedMemorySize, NL_MAX_LDS);
        attr_set = true;
    }
    hipLaunchKernelGGL((nonlocal_dot_eval_kernel<T, TPW>), dim3(n), dim3(NL_THREADS), (size_t)pl.lds_floats * 4, st, x, sx_n, sx_c, sx_p, C,
                       Ci, P, w_tpg, b_tpg, w_z, b_z, scale, shift, z, pl);
}

template <typename T>
static int nl_eval_impl(const T *x, long long sx_n, long long sx_c, long long sx_p, int n, int C, int Ci, int P, const float *w_tpg,
                        const float *b_tpg, const float *w_z, const float *b_z, const float *scale, const float *shift, T *z,
                        void *stream) {
    MGAR_REQUIRE(n >= 0 && C >= 1 && Ci >= 1 && P >= 1 && sx_n >= 0 && sx_c >= 0 && sx_p >= 0,
                 "nonlocal_dot_eval_fwd: bad sizes (n >= 0; C, Ci, P >= 1; strides >= 0)");
    if (!nl_supported(C, Ci, P)) {
        set_error("nonlocal_dot_eval_fwd: needs C <= 1024, Ci <= 128, P <= 256, Ci * P <= 4096");
        return MGAR_EUNSUPPORTED;
    }
    if (n == 0) return MGAR_OK;
    MGAR_REQUIRE(x && w_tpg && b_tpg && w_z && b_z && scale && shift && z, "nonlocal_dot_eval_fwd: null pointer");
    NlPlan pl = nl_plan(C, Ci, P);
    const uintptr_t xalign = 4 * sizeof(T) - 1;
    pl.xvec = sx_c == 1 && C % 4 == 0 && sx_p % 4 == 0 && sx_n % 4 == 0 && ((uintptr_t)x & xalign) == 0;
    pl.wvec = C % 4 == 0 && ((uintptr_t)w_tpg & 15) == 0;
    pl.zvec = Ci % 4 == 0 && ((uintptr_t)w_z & 15) == 0;
    hipStream_t st = (hipStream_t)stream;
    // algebraic traffic: x once, z once, the parameters once
    KtScope kt(KT_NONLOCAL_EVAL, st, 2.0 * sizeof(T) * n * C * P + 4.0 * (4.0 * Ci * C + 3.0 * Ci + 3.0 * C),
               2.0 * n * (4.0 * Ci * C * P + 2.0 * Ci * Ci * P));
    switch (pl.tpw) {
        case 1: nl_launch<T, 1>(n, x, sx_n, sx_c, sx_p, C, Ci, P, w_tpg, b_tpg, w_z, b_z, scale, shift, z, pl, st); break;
        case 2: nl_launch<T, 2>(n, x, sx_n, sx_c, sx_p, C, Ci, P, w_tpg, b_tpg, w_z, b_z, scale, shift, z, pl, st); break;
        default: nl_launch<T, 3>(n, x, sx_n, sx_c, sx_p, C, Ci, P, w_tpg, b_tpg, w_z, b_z, scale, shift, z, pl, st); break;
    }
    return check_launch("nonlocal_dot_eval_fwd: launch failed");
}

}  // namespace mgar

using namespace mgar;

MGAR_API int mgar_nonlocal_dot_eval_supported(int C, int Ci, int P) { return nl_supported(C, Ci, P) ? 1 : 0; }

MGAR_API int mgar_nonlocal_dot_eval_fwd(const float *x, long long sx_n, long long sx_c, long long sx_p, int n, int C, int Ci, int P,
                                        const float *w_tpg, const float *b_tpg, const float *w_z, const float *b_z,
                                        const float *scale, const float *shift, float *z, void *stream) {
    return nl_eval_impl<float>(x, sx_n, sx_c, sx_p, n, C, Ci, P, w_tpg, b_tpg, w_z, b_z, scale, shift, z, stream);
}
MGAR_API int mgar_nonlocal_dot_eval_bf16_fwd(const void *x, long long sx_n, long long sx_c, long long sx_p, int n, int C, int Ci, int P,
                                             const float *w_tpg, const float *b_tpg, const float *w_z, const float *b_z,
                                             const float *scale, const float *shift, void *z, void *stream) {
    return nl_eval_impl<bf16_t>((const bf16_t *)x, sx_n, sx_c, sx_p, n, C, Ci, P, w_tpg, b_tpg, w_z, b_z, scale, shift, (bf16_t *)z,
                                stream);
}
