// scene_ops.hip -- the three per-scene operations of the fusion net's ragged batched route, in segment form, for gfx950.
//
// All entries work on PACKED scene rows: the rows of every scene are stacked, scene s owns rows
// [scene_off[s], scene_off[s + 1]) and the dense (n_s, n_s) block at de_off[s] -- the layout of mgar_dafm_attn_* (dafm.hip).
//   scene_bn       training-mode BatchNorm1d of every scene by itself (GAR_Fusion_Net3._scene_bn, the reference's per-scene
//                  self.bn_rgb(R) / self.bn_lidar(L) of model/gat_model.py:1403-1406), forward and backward
//   pair_geometry  De (pairwise Euclidean distance of the 3-D box centres, evaluated in double) and Dg (generalized box IoU
//                  of the 2-D boxes) of every scene
//   gram           G_s = X_s X_s^T, forward and backward (the cosine-similarity matrix D_v once the rows are normalised)
// None of them moves enough bytes to matter (a 120-scene step reads a few MB); each replaces a Python loop over scenes or a
// pad-to-the-largest-scene batched op, so the point is the launch count.  No float atomics: every sum runs in a fixed order.
#include "common.hpp"

namespace mgar {

constexpr int SCENE_JPL = MGAR_DAFM_MAX_N / kWave;  // columns per lane of the pair kernels (2)
typedef const float __attribute__((address_space(4))) *scene_cfloat_p;

__device__ __forceinline__ int scene_of_packed_row(int row, int S, const int *__restrict__ scene_off) {
    int lo = 0, hi = S - 1;  // largest s with scene_off[s] <= row: empty scenes (equal offsets) are stepped over
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (scene_off[mid] <= row) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// see bcast_col of dafm.hip: the register is picked on the scalar side because the caller runs with part of the lanes off
__device__ __forceinline__ float scene_bcast_col(const float (&r)[SCENE_JPL], int j) {
    const int lo = __builtin_amdgcn_readlane(__builtin_bit_cast(int, r[0]), j & 63);
    const int hi = __builtin_amdgcn_readlane(__builtin_bit_cast(int, r[1]), j & 63);
    return __builtin_bit_cast(float, j < kWave ? lo : hi);
}

// ------------------------------------------------------------------------------------------------ scene BatchNorm
// grid (S, C / 64), one wave per block, lanes along channels: every row read is one coalesced 256-byte line and every
// (scene, channel) sum is a serial chain over the scene's rows in ascending order.
__global__ __launch_bounds__(64) void scene_bn_fwd_kernel(int C, const int *__restrict__ scene_off, const float *__restrict__ x,
                                                          const float *__restrict__ gamma, const float *__restrict__ beta,
                                                          float eps, float *__restrict__ y, float *__restrict__ save_mean,
                                                          float *__restrict__ save_invstd, float *__restrict__ save_var) {
    const int s = blockIdx.x, c = blockIdx.y * kWave + threadIdx.x;
    const int r0 = scene_off[s], n = scene_off[s + 1] - r0;
    const size_t sc = (size_t)s * C + c;
    if (n <= 0) {  // nothing to normalise; the saved statistics are still defined (the backward and the EMA skip the scene)
        save_mean[sc] = 0.f; save_invstd[sc] = 0.f; save_var[sc] = 0.f;
        return;
    }
    const float *xs = x + (size_t)r0 * C + c;
    float *ys = y + (size_t)r0 * C + c;
    const float b = beta[c];
    if (n == 1) {  // PyTorch raises here; defined as y = beta, no statistics
        save_mean[sc] = xs[0]; save_invstd[sc] = 0.f; save_var[sc] = 0.f;
        ys[0] = b;
        return;
    }
    float sum = 0.f;
    for (int r = 0; r < n; ++r) sum += xs[(size_t)r * C];
    const float mean = sum / (float)n;
    float m2 = 0.f;
    for (int r = 0; r < n; ++r) {
        const float d = xs[(size_t)r * C] - mean;
        m2 = __builtin_fmaf(d, d, m2);
    }
    const float var = m2 / (float)n;
    const float invstd = 1.0f / sqrtf(var + eps);
    const float a = invstd * gamma[c];
    for (int r = 0; r < n; ++r) ys[(size_t)r * C] = __builtin_fmaf(xs[(size_t)r * C] - mean, a, b);
    save_mean[sc] = mean; save_invstd[sc] = invstd; save_var[sc] = var;
}

// One thread per channel: the reference loop's EMA steps, one per scene of at least two rows, in ascending scene order.
__global__ __launch_bounds__(256) void scene_bn_running_kernel(int S, int C, const int *__restrict__ scene_off,
                                                               const float *__restrict__ save_mean,
                                                               const float *__restrict__ save_var, float momentum,
                                                               float *__restrict__ running_mean, float *__restrict__ running_var,
                                                               long long *__restrict__ num_batches_tracked) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= C) return;
    float rm = running_mean[c], rv = running_var[c];
    int steps = 0;
    for (int s = 0; s < S; ++s) {
        const int n = scene_off[s + 1] - scene_off[s];
        if (n < 2) continue;
        const float unbiased = save_var[(size_t)s * C + c] * ((float)n / (float)(n - 1));
        rm = (1.0f - momentum) * rm + momentum * save_mean[(size_t)s * C + c];
        rv = (1.0f - momentum) * rv + momentum * unbiased;
        ++steps;
    }
    running_mean[c] = rm; running_var[c] = rv;
    if (c == 0 && num_batches_tracked) *num_batches_tracked += steps;
}

// Backward, same launch shape.  With xhat = (x - mean) invstd, a = sum dy, b = sum dy xhat over the scene's rows:
//   dx = gamma invstd (dy - a / n - xhat b / n);   per-scene partials of dbeta (a) and dgamma (b) go to the workspace.
__global__ __launch_bounds__(64) void scene_bn_bwd_kernel(int S, int C, const int *__restrict__ scene_off,
                                                          const float *__restrict__ x, const float *__restrict__ dy,
                                                          const float *__restrict__ gamma, const float *__restrict__ save_mean,
                                                          const float *__restrict__ save_invstd, float *__restrict__ dx,
                                                          float *__restrict__ workspace) {
    const int s = blockIdx.x, c = blockIdx.y * kWave + threadIdx.x;
    const int r0 = scene_off[s], n = scene_off[s + 1] - r0;
    const size_t sc = (size_t)s * C + c;
    float *part_dgamma = workspace, *part_dbeta = workspace + (size_t)S * C;
    if (n <= 0) { part_dgamma[sc] = 0.f; part_dbeta[sc] = 0.f; return; }
    const float *xs = x + (size_t)r0 * C + c, *gs = dy + (size_t)r0 * C + c;
    float *ds = dx + (size_t)r0 * C + c;
    if (n == 1) {  // forward wrote y = beta: no path to x or gamma
        part_dgamma[sc] = 0.f; part_dbeta[sc] = gs[0];
        ds[0] = 0.f;
        return;
    }
    const float mean = save_mean[sc], invstd = save_invstd[sc];
    float a = 0.f, b = 0.f;
    for (int r = 0; r < n; ++r) {
        const float g = gs[(size_t)r * C];
        a += g;
        b = __builtin_fmaf(g, (xs[(size_t)r * C] - mean) * invstd, b);
    }
    part_dgamma[sc] = b; part_dbeta[sc] = a;
    const float am = a / (float)n, bm = b / (float)n, gi = gamma[c] * invstd;
    for (int r = 0; r < n; ++r) {
        const float xhat = (xs[(size_t)r * C] - mean) * invstd;
        ds[(size_t)r * C] = gi * ((gs[(size_t)r * C] - am) - xhat * bm);
    }
}

__global__ __launch_bounds__(256) void scene_bn_bwd_params_kernel(int S, int C, const float *__restrict__ workspace,
                                                                  float *__restrict__ dgamma, float *__restrict__ dbeta) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= C) return;
    float g = 0.f, b = 0.f;
    for (int s = 0; s < S; ++s) {  // ascending scene order
        g += workspace[(size_t)s * C + c];
        b += workspace[(size_t)(S + s) * C + c];
    }
    dgamma[c] = g; dbeta[c] = b;
}

// ------------------------------------------------------------------------------------------------ pair geometry
// grid: ceil(total_rows / 4) workgroups of 4 waves, one wave per row i, lanes along j (any n: the lanes stride over j).
__global__ __launch_bounds__(256) void scene_pair_geometry_kernel(int S, int total_rows, const int *__restrict__ scene_off,
                                                                  const int *__restrict__ de_off, const float *__restrict__ centres,
                                                                  const float *__restrict__ boxes, float *__restrict__ de,
                                                                  float *__restrict__ dg) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= total_rows) return;
    const int s = scene_of_packed_row(row, S, scene_off);
    const int r0 = scene_off[s], n = scene_off[s + 1] - r0, i = row - r0;
    const size_t mo = (size_t)de_off[s] + (size_t)i * n;
    const double xi = centres[(size_t)row * 3 + 0], yi = centres[(size_t)row * 3 + 1], zi = centres[(size_t)row * 3 + 2];
    const double sqi = xi * xi + yi * yi + zi * zi;
    for (int j = lane; j < n; j += kWave) {
        const float *cj = centres + (size_t)(r0 + j) * 3;
        const double xj = cj[0], yj = cj[1], zj = cj[2];
        const double sqj = xj * xj + yj * yj + zj * zj;
        const double dot = xi * xj + yi * yj + zi * zj;
        const double d2 = sqi + sqj - 2.0 * dot;
        de[mo + j] = j == i ? 0.f : (float)sqrt(d2 > 0.0 ? d2 : 0.0);
    }
    if (!boxes) return;
    const float4 bi = *reinterpret_cast<const float4 *>(boxes + (size_t)row * 4);
    const float area_i = (bi.z - bi.x) * (bi.w - bi.y);
    for (int j = lane; j < n; j += kWave) {
        const float4 bj = *reinterpret_cast<const float4 *>(boxes + (size_t)(r0 + j) * 4);
        const float area_j = (bj.z - bj.x) * (bj.w - bj.y);
        const float w = fmaxf(fminf(bi.z, bj.z) - fmaxf(bi.x, bj.x), 0.f), h = fmaxf(fminf(bi.w, bj.w) - fmaxf(bi.y, bj.y), 0.f);
        const float inter = w * h;
        const float uni = area_i + area_j - inter;
        const float wc = fmaxf(fmaxf(bi.z, bj.z) - fminf(bi.x, bj.x), 0.f), hc = fmaxf(fmaxf(bi.w, bj.w) - fminf(bi.y, bj.y), 0.f);
        const float areac = wc * hc;
        dg[mo + j] = inter / uni - (areac - uni) / areac;
    }
}

// ------------------------------------------------------------------------------------------------ Gram matrix
// One wave per row i, lanes along j: x_i arrives as wave-uniform scalars, each lane streams its own x_j row; every dot product is
// one fmaf chain over d ascending, so G_ij and G_ji are the same bits.
__global__ __launch_bounds__(256) void scene_gram_fwd_kernel(int S, int total_rows, int D, const int *__restrict__ scene_off,
                                                             const int *__restrict__ de_off, const float *__restrict__ x,
                                                             float *__restrict__ g) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= total_rows) return;
    const int s = scene_of_packed_row(row, S, scene_off);
    const int r0 = scene_off[s], n = scene_off[s + 1] - r0, i = row - r0;
    float dot[SCENE_JPL];
#pragma unroll
    for (int t = 0; t < SCENE_JPL; ++t) dot[t] = 0.f;
    scene_cfloat_p xi = (scene_cfloat_p)(x + (size_t)row * D);
    for (int d0 = 0; d0 < D; d0 += 16) {
        float xc[16];
#pragma unroll
        for (int u = 0; u < 16; ++u) xc[u] = xi[d0 + u];
#pragma unroll
        for (int t = 0; t < SCENE_JPL; ++t) {
            const int j = lane + t * kWave;
            if (j < n) {
                const float4 *xj = reinterpret_cast<const float4 *>(x + (size_t)(r0 + j) * D + d0);
#pragma unroll
                for (int u4 = 0; u4 < 4; ++u4) {
                    const float4 v = xj[u4];
                    dot[t] = __builtin_fmaf(xc[u4 * 4 + 0], v.x, dot[t]);
                    dot[t] = __builtin_fmaf(xc[u4 * 4 + 1], v.y, dot[t]);
                    dot[t] = __builtin_fmaf(xc[u4 * 4 + 2], v.z, dot[t]);
                    dot[t] = __builtin_fmaf(xc[u4 * 4 + 3], v.w, dot[t]);
                }
            }
        }
    }
    float *g_row = g + (size_t)de_off[s] + (size_t)i * n;
#pragma unroll
    for (int t = 0; t < SCENE_JPL; ++t)
        if (lane + t * kWave < n) g_row[lane + t * kWave] = dot[t];
}

// dX_i = sum_j (dG_ij + dG_ji) x_j: the weights lanes along j, then lanes along d with j ascending.
__global__ __launch_bounds__(256) void scene_gram_bwd_kernel(int S, int total_rows, int D, const int *__restrict__ scene_off,
                                                             const int *__restrict__ de_off, const float *__restrict__ x,
                                                             const float *__restrict__ grad_g, float *__restrict__ grad_x) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= total_rows) return;
    const int s = scene_of_packed_row(row, S, scene_off);
    const int r0 = scene_off[s], n = scene_off[s + 1] - r0, i = row - r0;
    const float *gs = grad_g + (size_t)de_off[s];
    float w[SCENE_JPL];
#pragma unroll
    for (int t = 0; t < SCENE_JPL; ++t) {
        const int j = lane + t * kWave;
        w[t] = j < n ? gs[(size_t)i * n + j] + gs[(size_t)j * n + i] : 0.f;
    }
    for (int d0 = lane * 4; d0 < D; d0 += 256) {
        float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
        for (int j = 0; j < n; ++j) {
            const float wj = scene_bcast_col(w, j);
            const float4 v = *reinterpret_cast<const float4 *>(x + (size_t)(r0 + j) * D + d0);
            acc.x = __builtin_fmaf(wj, v.x, acc.x); acc.y = __builtin_fmaf(wj, v.y, acc.y);
            acc.z = __builtin_fmaf(wj, v.z, acc.z); acc.w = __builtin_fmaf(wj, v.w, acc.w);
        }
        *reinterpret_cast<float4 *>(grad_x + (size_t)row * D + d0) = acc;
    }
}

}  // namespace mgar

using namespace mgar;

#define SCENE_LANES_64(cond, msg)      \
    do {                               \
        if (!(cond)) {                 \
            set_error(msg);            \
            return MGAR_EUNSUPPORTED;  \
        }                              \
    } while (0)

MGAR_API int mgar_scene_bn_fwd(int S, int total_rows, int C, const int *scene_off, const float *x, const float *gamma,
                               const float *beta, float eps, float momentum, float *running_mean, float *running_var,
                               long long *num_batches_tracked, float *y, float *save_mean, float *save_invstd,
                               float *save_var, void *stream) {
    MGAR_REQUIRE(S >= 0 && total_rows >= 0 && C > 0, "scene_bn_fwd: bad sizes");
    SCENE_LANES_64(C % 64 == 0, "scene_bn_fwd: C must be a multiple of 64");
    if (S == 0 || total_rows == 0) return MGAR_OK;
    MGAR_REQUIRE(scene_off && x && gamma && beta && y && save_mean && save_invstd && save_var, "scene_bn_fwd: null pointer");
    MGAR_REQUIRE((running_mean == nullptr) == (running_var == nullptr), "scene_bn_fwd: running_mean and running_var go together");
    hipLaunchKernelGGL(scene_bn_fwd_kernel, dim3(S, C / 64), dim3(64), 0, (hipStream_t)stream, C, scene_off, x, gamma, beta, eps,
                       y, save_mean, save_invstd, save_var);
    if (running_mean)
        hipLaunchKernelGGL(scene_bn_running_kernel, dim3(ceil_div(C, 256)), dim3(256), 0, (hipStream_t)stream, S, C, scene_off,
                           save_mean, save_var, momentum, running_mean, running_var, num_batches_tracked);
    return check_launch("scene_bn_fwd: launch failed");
}

MGAR_API int mgar_scene_bn_bwd(int S, int total_rows, int C, const int *scene_off, const float *x, const float *grad_y,
                               const float *gamma, const float *save_mean, const float *save_invstd, float *workspace,
                               float *grad_x, float *grad_gamma, float *grad_beta, void *stream) {
    MGAR_REQUIRE(S >= 0 && total_rows >= 0 && C > 0, "scene_bn_bwd: bad sizes");
    SCENE_LANES_64(C % 64 == 0, "scene_bn_bwd: C must be a multiple of 64");
    if (S == 0 || total_rows == 0) return MGAR_OK;  // nothing is written, grad_gamma / grad_beta included
    MGAR_REQUIRE(scene_off && x && grad_y && gamma && save_mean && save_invstd && workspace && grad_x && grad_gamma && grad_beta,
                 "scene_bn_bwd: null pointer");
    hipLaunchKernelGGL(scene_bn_bwd_kernel, dim3(S, C / 64), dim3(64), 0, (hipStream_t)stream, S, C, scene_off, x, grad_y, gamma,
                       save_mean, save_invstd, grad_x, workspace);
    hipLaunchKernelGGL(scene_bn_bwd_params_kernel, dim3(ceil_div(C, 256)), dim3(256), 0, (hipStream_t)stream, S, C, workspace,
                       grad_gamma, grad_beta);
    return check_launch("scene_bn_bwd: launch failed");
}

MGAR_API int mgar_scene_pair_geometry(int S, int total_rows, const int *scene_off, const int *de_off, const float *centres,
                                      const float *boxes, float *de, float *dg, void *stream) {
    MGAR_REQUIRE(S >= 0 && total_rows >= 0, "scene_pair_geometry: bad sizes");
    if (S == 0 || total_rows == 0) return MGAR_OK;
    MGAR_REQUIRE(scene_off && de_off && centres && de, "scene_pair_geometry: null pointer");
    MGAR_REQUIRE(!boxes || dg, "scene_pair_geometry: boxes without dg");
    hipLaunchKernelGGL(scene_pair_geometry_kernel, dim3(ceil_div(total_rows, 4)), dim3(256), 0, (hipStream_t)stream, S, total_rows,
                       scene_off, de_off, centres, boxes, de, dg);
    return check_launch("scene_pair_geometry: launch failed");
}

MGAR_API int mgar_scene_gram_fwd(int S, int total_rows, int D, const int *scene_off, const int *de_off, const float *x, float *g,
                                 void *stream) {
    MGAR_REQUIRE(S >= 0 && total_rows >= 0 && D > 0, "scene_gram_fwd: bad sizes");
    SCENE_LANES_64(D % 64 == 0, "scene_gram_fwd: D must be a multiple of 64");
    if (S == 0 || total_rows == 0) return MGAR_OK;
    MGAR_REQUIRE(scene_off && de_off && x && g, "scene_gram_fwd: null pointer");
    hipLaunchKernelGGL(scene_gram_fwd_kernel, dim3(ceil_div(total_rows, 4)), dim3(256), 0, (hipStream_t)stream, S, total_rows, D,
                       scene_off, de_off, x, g);
    return check_launch("scene_gram_fwd: launch failed");
}

MGAR_API int mgar_scene_gram_bwd(int S, int total_rows, int D, const int *scene_off, const int *de_off, const float *x,
                                 const float *grad_g, float *grad_x, void *stream) {
    MGAR_REQUIRE(S >= 0 && total_rows >= 0 && D > 0, "scene_gram_bwd: bad sizes");
    SCENE_LANES_64(D % 64 == 0, "scene_gram_bwd: D must be a multiple of 64");
    if (S == 0 || total_rows == 0) return MGAR_OK;
    MGAR_REQUIRE(scene_off && de_off && x && grad_g && grad_x, "scene_gram_bwd: null pointer");
    hipLaunchKernelGGL(scene_gram_bwd_kernel, dim3(ceil_div(total_rows, 4)), dim3(256), 0, (hipStream_t)stream, S, total_rows, D,
                       scene_off, de_off, x, grad_g, grad_x);
    return check_launch("scene_gram_bwd: launch failed");
}
