// scene_tail_eval.hip -- the eval-mode tail of the fusion net behind the fused rows, one workgroup per scene, for gfx950.
//
// What GAR_Fusion_Net3.forward_per_scene does in eval mode between `_fuse` and the heads, for packed scene rows laid out as
// scene_ops.py lays them out (scene s owns rows [scene_off[s], scene_off[s + 1]) and the (n, n) block of dg at de_off[s]):
//   Dv_ij  = <x_i, x_j> / (|x_i| |x_j|)                   one fmaf chain over d ascending per dot product and per |x_i|^2
//   a_ij   = D_embed([Dv_ij, Dg_ij]),  a_ii = 1           Linear(2,1) + Sigmoid, or Linear(2,H) + ReLU + Linear(H,1) + Sigmoid
//   A_list : the scene's whole (mnp, mnp) block, padding zeros included
//   gid_i  = smallest j with a_ij >= 0.5 (a NaN compares false; the diagonal is 1)   -> (S, mnp) int32, -1 in the padding
//   sg_i   = max over {k : gid_k == gid_i} of x_k, NaN propagating (compare-select; fmaxf would drop the NaN)
//   card   = [column maximum of the scene's rows (NaN propagating), sum of the (n, n) adjacency block]
// No atomics, no workspace.  Every sum runs in an order that depends on (n, D, hidden) alone: the dot products over d
// ascending, the hidden layer over its units ascending, the block sum as n row chains over j ascending added over i ascending.
// A scene is read and written by its own workgroup only, so its bits depend on that scene and the parameters alone and a
// NaN stays inside it.
// LDS (dynamic, sized by the batch's largest scene): the (n, n) adjacency (64 KiB at n = 128) and four n-vectors; the rows
// themselves stay in global memory / L2 (a full copy at n = 128, D = 512 would be 256 KB): the Gram phase streams x_j per lane
// and x_i as wave-uniform scalars, like scene_gram_fwd_kernel of scene_ops.hip.
#include "common.hpp"

namespace mgar {

constexpr int ST_THREADS = 1024;
constexpr int ST_WAVES = ST_THREADS / kWave;
constexpr int ST_MAX_N = MGAR_DAFM_MAX_N;
constexpr int ST_JPL = ST_MAX_N / kWave;   // columns per lane of the Gram phase (2)
constexpr int ST_MAX_HIDDEN = 8;
typedef const float __attribute__((address_space(4))) *st_cfloat_p;

// 66 692 bytes at 128 actors: inside the 160 KiB of a CU with room for a second workgroup
inline int st_lds_bytes(int cap) { return (cap * cap + 4 * cap + 4 * ST_MAX_HIDDEN + 1) * 4; }

// D_embed on one pair.  p: [w_v, w_g, b] (hidden == 0) or [W1 (H, 2) row-major, b1 (H), w2 (H), b2] (hidden == H).
__device__ __forceinline__ float st_embed(float dv, float dgv, const float *p, int hidden) {
    float z;
    if (hidden == 0) {
        z = __builtin_fmaf(p[1], dgv, __builtin_fmaf(p[0], dv, p[2]));
    } else {
        z = p[4 * hidden];
        for (int k = 0; k < hidden; ++k) {
            const float h = relu_nan(__builtin_fmaf(p[2 * k + 1], dgv, __builtin_fmaf(p[2 * k], dv, p[2 * hidden + k])));
            z = __builtin_fmaf(p[3 * hidden + k], h, z);
        }
    }
    return 1.0f / (1.0f + expf(-z));
}

__global__ __launch_bounds__(ST_THREADS) void scene_tail_eval_kernel(int D, int mnp, int hidden, int cap, const int *__restrict__ scene_off,
                                                                     const int *__restrict__ de_off, const float *__restrict__ x,
                                                                     const float *__restrict__ dg, const float *__restrict__ dembed,
                                                                     float *__restrict__ a_list, int *__restrict__ group_id,
                                                                     float *__restrict__ sg, float *__restrict__ card) {
    // dynamic LDS, sized by the launcher from the largest scene: cap * cap adjacency, then four cap-vectors and the parameters
    extern __shared__ __attribute__((aligned(16))) float st_lds[];
    float *s_a = st_lds;
    float *s_nrm = s_a + cap * cap;
    float *s_rowsum = s_nrm + cap;
    int *s_gid = reinterpret_cast<int *>(s_rowsum + cap);
    int *s_lead = s_gid + cap;
    float *s_par = reinterpret_cast<float *>(s_lead + cap);

    const int s = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r0 = scene_off[s];
    int n = scene_off[s + 1] - r0;
    n = n < 0 ? 0 : (n > cap ? cap : n);    // the host refuses such counts; this keeps every index inside LDS
    n = n > mnp ? mnp : n;
    const float *xs = x + (size_t)r0 * D;
    const int n_par = hidden == 0 ? 3 : 4 * hidden + 1;
    if (tid < n_par) s_par[tid] = dembed[tid];

    // |x_i|: one thread per row, fmaf chain over d ascending
    if (tid < n) {
        const float4 *xi = reinterpret_cast<const float4 *>(xs + (size_t)tid * D);
        float ss = 0.f;
        for (int d4 = 0; d4 < D / 4; ++d4) {
            const float4 v = xi[d4];
            ss = __builtin_fmaf(v.x, v.x, ss); ss = __builtin_fmaf(v.y, v.y, ss);
            ss = __builtin_fmaf(v.z, v.z, ss); ss = __builtin_fmaf(v.w, v.w, ss);
        }
        s_nrm[tid] = sqrtf(ss);
    }
    __syncthreads();

    // adjacency: one wave per row i, lanes along j
    const float *dgs = dg + (size_t)de_off[s];
    for (int i = wave; i < n; i += ST_WAVES) {
        float dot[ST_JPL];
#pragma unroll
        for (int t = 0; t < ST_JPL; ++t) dot[t] = 0.f;
        st_cfloat_p xi = (st_cfloat_p)(xs + (size_t)i * D);
        for (int d0 = 0; d0 < D; d0 += 16) {
            float xc[16];
#pragma unroll
            for (int u = 0; u < 16; ++u) xc[u] = xi[d0 + u];
#pragma unroll
            for (int t = 0; t < ST_JPL; ++t) {
                const int j = lane + t * kWave;
                if (j < n) {
                    const float4 *xj = reinterpret_cast<const float4 *>(xs + (size_t)j * D + d0);
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
        const float ni = s_nrm[i];
#pragma unroll
        for (int t = 0; t < ST_JPL; ++t) {
            const int j = lane + t * kWave;
            if (j < n) {
                const float dv = dot[t] / (ni * s_nrm[j]);
                s_a[i * n + j] = j == i ? 1.0f : st_embed(dv, dgs[(size_t)i * n + j], s_par, hidden);
            }
        }
    }
    __syncthreads();

    // the scene's whole padded block of A_list
    float *ab = a_list + (size_t)s * mnp * mnp;
    for (int e = tid; e < mnp * mnp; e += ST_THREADS) {
        const int i = e / mnp, j = e - i * mnp;
        ab[e] = (i < n && j < n) ? s_a[i * n + j] : 0.f;
    }
    // group ids and row sums: one thread per row, j ascending
    if (tid < n) {
        const float *row = s_a + tid * n;
        int g = tid;                                   // a_ii = 1 guarantees a hit at the latest there
        for (int j = 0; j < tid; ++j)
            if (row[j] >= 0.5f) { g = j; break; }
        s_gid[tid] = g;
        float rs = 0.f;
        for (int j = 0; j < n; ++j) rs += row[j];
        s_rowsum[tid] = rs;
    }
    for (int i = tid; i < mnp; i += ST_THREADS)
        if (i >= n) group_id[(size_t)s * mnp + i] = -1;
    __syncthreads();
    if (tid < n) {
        group_id[(size_t)s * mnp + tid] = s_gid[tid];
        int lead = -1;                                 // first member of the group labelled tid, if it has any
        for (int k = 0; k < n; ++k)
            if (s_gid[k] == tid) { lead = k; break; }
        s_lead[tid] = lead;
    }
    __syncthreads();

    // group max-pool: threads along float4 columns, row slices across the rest of the workgroup; the first member of a group
    // computes the pooled row, the others copy it afterwards
    const int cols = D / 4;
    const int slices = ST_THREADS / cols > 0 ? ST_THREADS / cols : 1;
    const int slice = tid / cols;
    float *sgs = sg + (size_t)r0 * D;
    for (int c0 = tid % cols; c0 < cols && slice < slices; c0 += (cols > ST_THREADS ? ST_THREADS : cols)) {
        for (int i = slice; i < n; i += slices) {
            const int g = s_gid[i];
            if (s_lead[g] != i) continue;
            float4 m = reinterpret_cast<const float4 *>(xs + (size_t)i * D)[c0];
            for (int k = i + 1; k < n; ++k) {
                if (s_gid[k] != g) continue;
                const float4 v = reinterpret_cast<const float4 *>(xs + (size_t)k * D)[c0];
                m.x = max_nan(m.x, v.x); m.y = max_nan(m.y, v.y); m.z = max_nan(m.z, v.z); m.w = max_nan(m.w, v.w);
            }
            reinterpret_cast<float4 *>(sgs + (size_t)i * D)[c0] = m;
        }
    }
    // card feature: column maxima over the scene's rows, k ascending; the block sum, i ascending
    float *cs = card + (size_t)s * (D + 1);
    for (int c = tid; c < D; c += ST_THREADS) {
        float m = n > 0 ? xs[c] : 0.f;
        for (int k = 1; k < n; ++k) m = max_nan(m, xs[(size_t)k * D + c]);
        cs[c] = m;
    }
    if (tid == 0) {
        float t = 0.f;
        for (int i = 0; i < n; ++i) t += s_rowsum[i];
        cs[D] = t;
    }
    __syncthreads();   // the leaders' pooled rows are visible to the workgroup
    for (int c0 = tid % cols; c0 < cols && slice < slices; c0 += (cols > ST_THREADS ? ST_THREADS : cols)) {
        for (int i = slice; i < n; i += slices) {
            const int l = s_lead[s_gid[i]];
            if (l == i) continue;
            reinterpret_cast<float4 *>(sgs + (size_t)i * D)[c0] = reinterpret_cast<const float4 *>(sgs + (size_t)l * D)[c0];
        }
    }
}

}  // namespace mgar

using namespace mgar;

MGAR_API int mgar_scene_tail_eval_fwd(int S, int total_rows, int D, int mnp, int n_min, int n_max, const int *scene_off,
                                      const int *de_off, const float *fused, const float *dg, const float *dembed, int hidden,
                                      float *a_list, int *group_id, float *sg, float *card, void *stream) {
    MGAR_REQUIRE(S >= 0 && total_rows >= 0 && D > 0 && mnp > 0, "scene_tail_eval_fwd: bad sizes");
    MGAR_REQUIRE(hidden >= 0, "scene_tail_eval_fwd: negative hidden width");
    if (D % 64 != 0) {
        set_error("scene_tail_eval_fwd: D must be a multiple of 64");
        return MGAR_EUNSUPPORTED;
    }
    if (hidden > ST_MAX_HIDDEN) {
        set_error("scene_tail_eval_fwd: D_embed hidden width above 8");
        return MGAR_EUNSUPPORTED;
    }
    if (S == 0) return MGAR_OK;
    if (n_min < 2 || n_max > MGAR_DAFM_MAX_N || n_max > mnp || n_min > n_max) {
        set_error("scene_tail_eval_fwd: scene sizes must be 2..MGAR_DAFM_MAX_N and fit mnp");
        return MGAR_EUNSUPPORTED;
    }
    MGAR_REQUIRE(scene_off && de_off && fused && dg && dembed && a_list && group_id && sg && card,
                 "scene_tail_eval_fwd: null pointer");
    static bool attr_set = false;
    if (!attr_set) {
        (void)hipFuncSetAttribute((const void *)scene_tail_eval_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, st_lds_bytes(ST_MAX_N));
        attr_set = true;
    }
    hipLaunchKernelGGL(scene_tail_eval_kernel, dim3(S), dim3(ST_THREADS), st_lds_bytes(n_max), (hipStream_t)stream, D, mnp, hidden,
                       n_max, scene_off, de_off, fused, dg, dembed, a_list, group_id, sg, card);
    return check_launch("scene_tail_eval_fwd: launch failed");
}
