// scene_mha.hip -- per-scene multi-head attention core (fwd + bwd) over packed scene rows, for gfx950.
//
// The attention core of nn.MultiheadAttention(512, 8) as the reference calls it on one scene's (n, 512) rows
// (cross_attention_fusion, model/gat_model.py:30-38; FUSION 'catandAtt', :1426-1428): for every scene s and head h, with
// Q / K / V the head's 64 columns of the scene's rows,
//     Att = softmax(Q K^T * scale, dim=1),   out = Att V
// The in- and out-projections are dense GEMMs over all rows and stay on the library GEMM path.
//
// The DAFM kernels (dafm.hip) take ONE head of width D with contiguous rows; eight heads of 64 inside a 512- or 1536-wide
// row would need permute copies on both sides.  Here q, k, v are three pointers into fp32 rows of leading dimension `ld`
// (the three slices of one fused (rows, 3 * 64 * H) in-projection are passed as they are), head h being columns
// [64 h, 64 h + 64) from each pointer; out and the three gradients are (rows, 64 * H) contiguous; att and the backward's
// scratch gmat are (H, pairs), head h's plane packed like de of mgar_dafm_attn_fwd.
//
// grid (ceil(rows / 4), H), one WAVE per (query row, head):
//   lanes along j : logits s_ij = q_i . k_j (q_i's 64 values arrive as wave-uniform scalars, each lane streams its own
//                   k_j slice of 256 B), the row softmax as DPP reductions (wave_max / wave_sum);
//   lane = channel: out_i = sum_j att_ij v_j, dq, dk, dv.  head_dim equals the wave width, so every row read is one coalesced
//                   256-byte line and ALL lanes are active -- the readlane of a column register needs no care about
//                   inactive lanes here (dafm.hip's bcast_col note), the register is still picked on the scalar side.
// The wave's row index goes through readfirstlane: the compiler cannot prove threadIdx.x >> 6 uniform, and without the proof
// the address_space(4) reads below (q_i, gO_i, the columns of G and Att) compile to per-lane global loads of one address
// instead of scalar loads.
// No atomics: every sum has a fixed order, two runs give the same bits.
#include "common.hpp"

namespace mgar {

constexpr int MHA_HD = 64;                          // head width == wave width
constexpr int MHA_JPL = MGAR_DAFM_MAX_N / kWave;    // j's per lane (2)
typedef const float __attribute__((address_space(4))) *mha_cfloat_p;

__device__ __forceinline__ int mha_scene_of_row(int row, int S, const int *__restrict__ scene_off) {
    int lo = 0, hi = S - 1;  // largest s with scene_off[s] <= row
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (scene_off[mid] <= row) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// column j of a row held lanes-along-j (r[t] of lane l is column l + t * kWave), wave-uniform; j is wave-uniform
__device__ __forceinline__ float mha_bcast_col(const float (&r)[MHA_JPL], int j) {
    const int lo = __builtin_amdgcn_readlane(__builtin_bit_cast(int, r[0]), j & 63);
    const int hi = __builtin_amdgcn_readlane(__builtin_bit_cast(int, r[1]), j & 63);
    return __builtin_bit_cast(float, j < kWave ? lo : hi);
}

// sum_j w(j) * col[(r0 + j) * ld], j ascending, lane = channel (col already points at the lane's channel); w(j) is wave-uniform.
// The loads of four rows are issued together -- one dependent load per iteration would leave the loop latency-bound -- and the
// adds keep their order, so the unrolling does not change a bit.
template <class W>
__device__ __forceinline__ float mha_weighted_rows(const float *__restrict__ col, int ld, int r0, int n, W w) {
    float acc = 0.f;
    int j = 0;
    for (; j + 4 <= n; j += 4) {
        float x[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) x[u] = col[(size_t)(r0 + j + u) * ld];
#pragma unroll
        for (int u = 0; u < 4; ++u) acc += w(j + u) * x[u];
    }
    for (; j < n; ++j) acc += w(j) * col[(size_t)(r0 + j) * ld];
    return acc;
}

// dot[t] = x_i . y_j for j = lane + t * kWave < n: x_i (64 floats at a wave-uniform address) as scalars, y's rows at stride ld
__device__ __forceinline__ void mha_row_dots(const float *__restrict__ xi_, const float *__restrict__ y, int ld, int r0, int n,
                                             int lane, float (&dot)[MHA_JPL]) {
    mha_cfloat_p xi = (mha_cfloat_p)xi_;
#pragma unroll
    for (int t = 0; t < MHA_JPL; ++t) dot[t] = 0.f;
    for (int d0 = 0; d0 < MHA_HD; d0 += 16) {
        float xc[16];
#pragma unroll
        for (int u = 0; u < 16; ++u) xc[u] = xi[d0 + u];
#pragma unroll
        for (int t = 0; t < MHA_JPL; ++t) {
            const int j = lane + t * kWave;
            if (j < n) {
                const float4 *yj = reinterpret_cast<const float4 *>(y + (size_t)(r0 + j) * ld + d0);
#pragma unroll
                for (int u4 = 0; u4 < 4; ++u4) {
                    const float4 yy = yj[u4];
                    dot[t] += xc[u4 * 4 + 0] * yy.x + xc[u4 * 4 + 1] * yy.y + xc[u4 * 4 + 2] * yy.z + xc[u4 * 4 + 3] * yy.w;
                }
            }
        }
    }
}

__global__ __launch_bounds__(256) void scene_mha_fwd_kernel(int S, int total_rows, int pairs, const int *__restrict__ scene_off,
                                                            const int *__restrict__ de_off, const float *__restrict__ q,
                                                            const float *__restrict__ k, const float *__restrict__ v, int ld,
                                                            float scale, float *__restrict__ att, float *__restrict__ out) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);   // provably wave-uniform (see above)
    if (row >= total_rows) return;
    const int h = blockIdx.y, c0 = h * MHA_HD, ldo = gridDim.y * MHA_HD;
    const int s = mha_scene_of_row(row, S, scene_off);
    const int r0 = scene_off[s], n = scene_off[s + 1] - r0, i = row - r0;
    float *att_row = att + (size_t)h * pairs + de_off[s] + (size_t)i * n;

    float dot[MHA_JPL];
    mha_row_dots(q + (size_t)row * ld + c0, k + c0, ld, r0, n, lane, dot);
    float lg[MHA_JPL], lmax = -__builtin_inff();
#pragma unroll
    for (int t = 0; t < MHA_JPL; ++t) {
        lg[t] = (lane + t * kWave) < n ? dot[t] * scale : -__builtin_inff();
        lmax = fmaxf(lmax, lg[t]);
    }
    lmax = wave_max(lmax);
    float psum = 0.f, p[MHA_JPL];
#pragma unroll
    for (int t = 0; t < MHA_JPL; ++t) { p[t] = (lane + t * kWave) < n ? __expf(lg[t] - lmax) : 0.f; psum += p[t]; }
    psum = wave_sum(psum);
#pragma unroll
    for (int t = 0; t < MHA_JPL; ++t) {
        p[t] /= psum;
        if (lane + t * kWave < n) att_row[lane + t * kWave] = p[t];
    }

    // ---- out_i = sum_j att_ij v_j, lane = channel ----
    out[(size_t)row * ldo + c0 + lane] = mha_weighted_rows(v + c0 + lane, ld, r0, n, [&](int j) { return mha_bcast_col(p, j); });
}

// Backward, rows pass (one wave per (query row i, head)):
//   dAtt_ij = gO_i . v_j ;  dS_ij = att_ij (dAtt_ij - sum_j' att_ij' dAtt_ij') ;  G_ij = dS_ij * scale (written to gmat) ;
//   dq_i = sum_j G_ij k_j
__global__ __launch_bounds__(256) void scene_mha_bwd_rows_kernel(int S, int total_rows, int pairs,
                                                                 const int *__restrict__ scene_off,
                                                                 const int *__restrict__ de_off, const float *__restrict__ k,
                                                                 const float *__restrict__ v, int ld, float scale,
                                                                 const float *__restrict__ att,
                                                                 const float *__restrict__ grad_out, float *__restrict__ gmat,
                                                                 float *__restrict__ grad_q) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);   // provably wave-uniform (see above)
    if (row >= total_rows) return;
    const int h = blockIdx.y, c0 = h * MHA_HD, ldo = gridDim.y * MHA_HD;
    const int s = mha_scene_of_row(row, S, scene_off);
    const int r0 = scene_off[s], n = scene_off[s + 1] - r0, i = row - r0;
    const size_t mo = (size_t)h * pairs + de_off[s] + (size_t)i * n;

    float a[MHA_JPL], dot[MHA_JPL];
#pragma unroll
    for (int t = 0; t < MHA_JPL; ++t) a[t] = (lane + t * kWave) < n ? att[mo + lane + t * kWave] : 0.f;
    mha_row_dots(grad_out + (size_t)row * ldo + c0, v + c0, ld, r0, n, lane, dot);
    float rsum = 0.f;
#pragma unroll
    for (int t = 0; t < MHA_JPL; ++t) rsum += a[t] * dot[t];
    rsum = wave_sum(rsum);
    float g[MHA_JPL];
#pragma unroll
    for (int t = 0; t < MHA_JPL; ++t) {
        g[t] = a[t] * (dot[t] - rsum) * scale;
        if (lane + t * kWave < n) gmat[mo + lane + t * kWave] = g[t];
    }
    grad_q[(size_t)row * ldo + c0 + lane] = mha_weighted_rows(k + c0 + lane, ld, r0, n, [&](int j) { return mha_bcast_col(g, j); });
}

// Backward, columns pass (one wave per (key row j, head)):  dk_j = sum_i G_ij q_i ;  dv_j = sum_i att_ij gO_i
__global__ __launch_bounds__(256) void scene_mha_bwd_cols_kernel(int S, int total_rows, int pairs,
                                                                 const int *__restrict__ scene_off,
                                                                 const int *__restrict__ de_off, const float *__restrict__ q,
                                                                 int ld, const float *__restrict__ att,
                                                                 const float *__restrict__ grad_out,
                                                                 const float *__restrict__ gmat, float *__restrict__ grad_k,
                                                                 float *__restrict__ grad_v) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);   // provably wave-uniform (see above)
    if (row >= total_rows) return;
    const int h = blockIdx.y, c0 = h * MHA_HD, ldo = gridDim.y * MHA_HD;
    const int s = mha_scene_of_row(row, S, scene_off);
    const int r0 = scene_off[s], n = scene_off[s + 1] - r0, j = row - r0;
    mha_cfloat_p G = (mha_cfloat_p)(gmat + (size_t)h * pairs + de_off[s]);
    mha_cfloat_p A = (mha_cfloat_p)(att + (size_t)h * pairs + de_off[s]);
    grad_k[(size_t)row * ldo + c0 + lane] = mha_weighted_rows(q + c0 + lane, ld, r0, n, [&](int i) { return G[(size_t)i * n + j]; });
    grad_v[(size_t)row * ldo + c0 + lane] =
        mha_weighted_rows(grad_out + c0 + lane, ldo, r0, n, [&](int i) { return A[(size_t)i * n + j]; });
}

}  // namespace mgar

using namespace mgar;

// sizes first (negative / non-positive: EINVAL), then the shapes the kernels are built for (EUNSUPPORTED), all before any
// device call
#define MHA_CHECK_SHAPE(name)                                                                                              \
    MGAR_REQUIRE(S >= 0 && total_rows >= 0 && H > 0 && head_dim > 0 && ld > 0 && pairs >= 0, name ": bad sizes");          \
    if (head_dim != MHA_HD || ld % 4 != 0 || ld < H * MHA_HD) {                                                            \
        set_error(name ": head_dim must be 64, ld a multiple of 4 and at least 64 * H");                                   \
        return MGAR_EUNSUPPORTED;                                                                                          \
    }

MGAR_API int mgar_scene_mha_fwd(int S, int total_rows, int H, int head_dim, const int *scene_off, const int *de_off, int pairs,
                                const float *q, const float *k, const float *v, int ld, float scale, float *att, float *out,
                                void *stream) {
    MHA_CHECK_SHAPE("scene_mha_fwd");
    if (S == 0 || total_rows == 0) return MGAR_OK;
    MGAR_REQUIRE(scene_off && de_off && q && k && v && att && out, "scene_mha_fwd: null pointer");
    MGAR_REQUIRE((((uintptr_t)q | (uintptr_t)k | (uintptr_t)v) & 15) == 0, "scene_mha_fwd: q, k, v must be 16-byte aligned");
    // per head what mgar_dafm_attn_add_fwd counts at D = 64 without a prior: q, k, v read + out written, Att written;
    // QK^T and Att V
    const double D = (double)H * MHA_HD;
    KtScope kt(KT_DAFM_FWD, (hipStream_t)stream, 4.0 * (4.0 * total_rows * D + (double)H * pairs), 4.0 * (double)pairs * D);
    hipLaunchKernelGGL(scene_mha_fwd_kernel, dim3(ceil_div(total_rows, 4), H), dim3(256), 0, (hipStream_t)stream, S, total_rows,
                       pairs, scene_off, de_off, q, k, v, ld, scale, att, out);
    return check_launch("scene_mha_fwd: launch failed");
}

MGAR_API int mgar_scene_mha_bwd(int S, int total_rows, int H, int head_dim, const int *scene_off, const int *de_off, int pairs,
                                const float *q, const float *k, const float *v, int ld, float scale, const float *att,
                                const float *grad_out, float *gmat, float *grad_q, float *grad_k, float *grad_v, void *stream) {
    MHA_CHECK_SHAPE("scene_mha_bwd");
    if (S == 0 || total_rows == 0) return MGAR_OK;
    MGAR_REQUIRE(scene_off && de_off && q && k && v && att && grad_out && gmat && grad_q && grad_k && grad_v,
                 "scene_mha_bwd: null pointer");
    MGAR_REQUIRE((((uintptr_t)v | (uintptr_t)grad_out) & 15) == 0, "scene_mha_bwd: v and grad_out must be 16-byte aligned");
    // q, k, v, grad_out read + 3 gradients written, Att read + the (H, pairs) scratch written and read;
    // dAtt = gO V^T, dq = dS K, dk = dS^T Q, dv = Att^T gO
    const double D = (double)H * MHA_HD;
    KtScope kt(KT_DAFM_BWD, (hipStream_t)stream, 4.0 * (7.0 * total_rows * D + 3.0 * (double)H * pairs), 8.0 * (double)pairs * D);
    hipLaunchKernelGGL(scene_mha_bwd_rows_kernel, dim3(ceil_div(total_rows, 4), H), dim3(256), 0, (hipStream_t)stream, S,
                       total_rows, pairs, scene_off, de_off, k, v, ld, scale, att, grad_out, gmat, grad_q);
    hipLaunchKernelGGL(scene_mha_bwd_cols_kernel, dim3(ceil_div(total_rows, 4), H), dim3(256), 0, (hipStream_t)stream, S,
                       total_rows, pairs, scene_off, de_off, q, ld, att, grad_out, gmat, grad_k, grad_v);
    return check_launch("scene_mha_bwd: launch failed");
}
