// sparse_conv.hip -- sparse 3-D convolution (submanifold and strided) for gfx950: voxel hash table, rulebook
// (neighbour tables) built on the device, gather-GEMM forward / data-gradient and weight-gradient kernels on the
// exact-fp32 MFMA.
//
// Replaces the third-party spconv 2.2.3 calls of the reference's Voxel R-CNN trunk
//   pcdet/models/backbones_3d/spconv_backbone.py:69-170  VoxelBackBone8x
//       spconv.SubMConv3d(C_in, C_out, 3, padding=1, bias=False, indice_key=...)            (submanifold)
//       spconv.SparseConv3d(C_in, C_out, k, stride=s, padding=p, bias=False, indice_key=...) (strided)
// and the dense (B, Z, Y, X) voxel -> row table of pcdet/utils/common_utils.py:235-252 (80 MB per sample at the shipped
// grid) as a lookup structure.  spconv is not vendored and its CUDA source is not in the reference tree; the
// arithmetic follows the published definition of the two layers (Graham et al. 2018):
//   out[o] = sum_k W_k . in[i]  over the kernel offsets k whose input site i = o * stride - pad + k is ACTIVE;
//   submanifold: output sites = input sites;  strided: output sites = every o with at least one active input.
//
// Data structures
//   * hash table: open addressing, linear probing, 64-bit keys ((b*Z + z)*Y + y)*X + x -> row id, capacity a power of two
//     >= 2N (load <= 0.5).  Built with one 64-bit atomicCAS per site.
//   * rulebook = neighbour table nbr (N_out, K) int32: row of the input site under kernel offset k, or -1.  The inverse
//     table (N_in, K): output row that input i reaches through offset k -- the data gradient is the same gather-GEMM over
//     it with W_k transposed.
// Kernels (all features row-major (rows, C), fp32; the MFMA is v_mfma_f32_32x32x2_f32: a k-ordered fp32 FMA chain):
//   * spconv_gather_gemm_kernel: a workgroup owns 64 output rows; per kernel offset it stages the gathered input rows
//     (64 x C_in, coalesced along the channels) and W_k (C_in x C_out) in LDS and accumulates 32x32 output blocks; offsets
//     no row of the tile uses are skipped (most of the 27 at LiDAR sparsity);
//   * spconv_dw_kernel: grid (site chunks, K); dW_k = A_k^T dOut accumulated in registers over the chunk, written as a
//     partial (summed by the caller in a fixed order: reproducible).
#include "common.hpp"
#include "voxel_hash.hpp"

namespace mgar {

typedef float __attribute__((ext_vector_type(16))) f32x16;

__global__ __launch_bounds__(256) void sph_build_kernel(int N, const int *__restrict__ coords, int Z, int Y, int X,
                                                        long long *__restrict__ tkeys, int *__restrict__ tvals, int mask) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= N) return;
    const long long key = sph_key(coords[i * 4], coords[i * 4 + 1], coords[i * 4 + 2], coords[i * 4 + 3], Z, Y, X);
    if (key == SPH_EMPTY) return;
    unsigned slot = (unsigned)sph_mix((unsigned long long)key) & (unsigned)mask;
    for (int probe = 0; probe <= mask; ++probe) {
        const long long old = (long long)atomicCAS((unsigned long long *)&tkeys[slot], (unsigned long long)SPH_EMPTY,
                                                   (unsigned long long)key);
        if (old == SPH_EMPTY || old == key) {
            atomicMin(&tvals[slot], i);               // values pre-filled with INT_MAX; duplicate coordinates: smallest row wins
            return;
        }
        slot = (slot + 1) & (unsigned)mask;
    }
}

__global__ __launch_bounds__(256) void sph_lookup_kernel(int M, const int *__restrict__ coords, int Z, int Y, int X,
                                                         const long long *__restrict__ tkeys, const int *__restrict__ tvals,
                                                         int mask, int *__restrict__ rows) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= M) return;
    const long long key = sph_key(coords[i * 4], coords[i * 4 + 1], coords[i * 4 + 2], coords[i * 4 + 3], Z, Y, X);
    rows[i] = key == SPH_EMPTY ? -1 : sph_find(tkeys, tvals, mask, key);
}

struct SpGeom {
    int kz, ky, kx, sz, sy, sx, pz, py, px;   // kernel, stride, padding (z, y, x)
    int Zi, Yi, Xi, Zo, Yo, Xo;               // spatial shapes of the input / output grids
};

// forward rulebook: nbr[o][k] = input row at o * stride - pad + k (table = hash of the INPUT sites)
__global__ __launch_bounds__(256) void sp_neighbors_kernel(long long total, int K, const int *__restrict__ out_coords, SpGeom g,
                                                           const long long *__restrict__ tkeys, const int *__restrict__ tvals,
                                                           int mask, int *__restrict__ nbr) {
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= total) return;
    const long long o = e / K;
    const int k = (int)(e - o * K);
    const int kx = k % g.kx, ky = (k / g.kx) % g.ky, kz = k / (g.kx * g.ky);
    const int *c = out_coords + o * 4;
    const long long key = sph_key(c[0], c[1] * g.sz - g.pz + kz, c[2] * g.sy - g.py + ky, c[3] * g.sx - g.px + kx, g.Zi, g.Yi, g.Xi);
    nbr[e] = key == SPH_EMPTY ? -1 : sph_find(tkeys, tvals, mask, key);
}

// inverse rulebook: inv[i][k] = output row o with o * stride - pad + k == i (table = hash of the OUTPUT sites)
__global__ __launch_bounds__(256) void sp_neighbors_inverse_kernel(long long total, int K, const int *__restrict__ in_coords, SpGeom g,
                                                                   const long long *__restrict__ tkeys,
                                                                   const int *__restrict__ tvals, int mask, int *__restrict__ inv) {
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= total) return;
    const long long i = e / K;
    const int k = (int)(e - i * K);
    const int kx = k % g.kx, ky = (k / g.kx) % g.ky, kz = k / (g.kx * g.ky);
    const int *c = in_coords + i * 4;
    const int nz = c[1] + g.pz - kz, ny = c[2] + g.py - ky, nx = c[3] + g.px - kx;
    int r = -1;
    if (nz >= 0 && ny >= 0 && nx >= 0 && nz % g.sz == 0 && ny % g.sy == 0 && nx % g.sx == 0) {
        const long long key = sph_key(c[0], nz / g.sz, ny / g.sy, nx / g.sx, g.Zo, g.Yo, g.Xo);
        if (key != SPH_EMPTY) r = sph_find(tkeys, tvals, mask, key);
    }
    inv[e] = r;
}

// candidate output sites of a strided convolution: keys[i * K + k] = linear (b, z, y, x) key in the OUTPUT grid of the site that
// input i reaches through offset k, or -1 (not integral / outside the grid).  The caller keeps the non-negative keys and makes
// them unique (one sort): ascending (b, z, y, x) order of the output sites.
__global__ __launch_bounds__(256) void sp_output_keys_kernel(long long total, int K, const int *__restrict__ in_coords, SpGeom g,
                                                             long long *__restrict__ keys) {
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= total) return;
    const long long i = e / K;
    const int k = (int)(e - i * K);
    const int kx = k % g.kx, ky = (k / g.kx) % g.ky, kz = k / (g.kx * g.ky);
    const int *c = in_coords + i * 4;
    const int nz = c[1] + g.pz - kz, ny = c[2] + g.py - ky, nx = c[3] + g.px - kx;
    long long key = SPH_EMPTY;
    if (nz >= 0 && ny >= 0 && nx >= 0 && nz % g.sz == 0 && ny % g.sy == 0 && nx % g.sx == 0)
        key = sph_key(c[0], nz / g.sz, ny / g.sy, nx / g.sx, g.Zo, g.Yo, g.Xo);
    keys[e] = key;
}

// ---- gather-GEMM: out[o, :] = sum_k in[nbr[o, k], :] . W[k]  (W (K, Cin, Cout) row-major) ------------------------------
constexpr int SC_ROWS = 64;       // output rows per workgroup
constexpr int SC_MAXC = 128;      // C_in, C_out <= 128

// The eval-mode BatchNorm [+ ReLU] epilogue of the two forward kernels (AFF instantiations): v = fma(acc, scale[c], shift[c]), then
// relu ? max(v, +0) with a NaN passed through (torch.relu; csrc/bn_act.hip) : v.  A negative or -0 pre-activation gives +0.
__device__ __forceinline__ float sc_affine(float acc, float scale, float shift, int relu) {
    const float v = __builtin_fmaf(acc, scale, shift);
    return relu ? (v > 0.f ? v : (v != v ? v : 0.f)) : v;
}

// grid ceil(No / 64).  LDS: nbr tile [64][K] ints, A [64][Cin + 1], W [Cin][CoutP] (CoutP = C_out rounded up to 32)
// AFF: the store applies sc_affine with scale / shift (Cout) -- a lane needs them at its own column cb * 32 + l only.
template <bool AFF>
__global__ __launch_bounds__(256) void spconv_gather_gemm_kernel(int No, int K, int Cin, int Cout, const float *__restrict__ in,
                                                                 const int *__restrict__ nbr, const float *__restrict__ w,
                                                                 int flip_k, const float *__restrict__ scale,
                                                                 const float *__restrict__ shift, int relu, float *__restrict__ out) {
    extern __shared__ float lds[];
    const int CoutP = (Cout + 31) & ~31, CinP = (Cin + 1) & ~1, ALD = CinP + 1;
    int *nb = reinterpret_cast<int *>(lds);               // [SC_ROWS][K]
    float *A = lds + SC_ROWS * K;                          // [SC_ROWS][ALD]
    float *W = A + SC_ROWS * ALD;                          // [CinP][CoutP]
    __shared__ int used[343];                              // used[k] != 0: some row of this tile has a neighbour under offset k
    const int o0 = blockIdx.x * SC_ROWS;
    const int nrow = min(SC_ROWS, No - o0);
    for (int k = threadIdx.x; k < K; k += 256) used[k] = 0;
    __syncthreads();
    for (int e = threadIdx.x; e < SC_ROWS * K; e += 256) {
        const int r = e / K;
        const int j = r < nrow ? nbr[(size_t)(o0 + r) * K + (e - r * K)] : -1;
        nb[e] = j;
        if (j >= 0) used[e - r * K] = 1;                   // benign race: every writer stores 1
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int l = lane & 31, h = lane >> 5;
    const int sb = wave & 1;                               // which 32-row half of the tile this wave accumulates
    const int ncb = CoutP / 32;                            // 32-column blocks of the output; this wave: cb = wave>>1, +2, ...
    f32x16 acc[2];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[a][r] = 0.f;
    __syncthreads();
    for (int k = 0; k < K; ++k) {
        if (!used[k]) continue;                            // uniform over the workgroup (read-only after the barrier above)
        for (int e = threadIdx.x; e < SC_ROWS * CinP; e += 256) {          // gathered rows, lanes along the channels
            const int r = e / CinP, c = e - r * CinP;
            const int j = nb[r * K + k];
            A[r * ALD + c] = (j >= 0 && c < Cin) ? in[(size_t)j * Cin + c] : 0.f;
        }
        const float *wk = w + (size_t)(flip_k ? K - 1 - k : k) * Cin * Cout;
        for (int e = threadIdx.x; e < CinP * CoutP; e += 256) {
            const int ci = e / CoutP, co = e - ci * CoutP;
            W[e] = (ci < Cin && co < Cout) ? wk[(size_t)ci * Cout + co] : 0.f;
        }
        __syncthreads();
#pragma unroll
        for (int a = 0; a < 2; ++a) {                      // static accumulator indices: no scratch
            const int cb = (wave >> 1) + 2 * a;
            if (cb < ncb) {
                for (int s = 0; s < CinP / 2; ++s) {
                    const float av = A[(sb * 32 + l) * ALD + 2 * s + h];
                    const float bv = W[(2 * s + h) * CoutP + cb * 32 + l];
                    acc[a] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bv, acc[a], 0, 0, 0);
                }
            }
        }
        __syncthreads();
    }
#pragma unroll
    for (int a = 0; a < 2; ++a) {
        const int cb = (wave >> 1) + 2 * a;
        const int co = cb * 32 + l;
        if (cb < ncb) {
            float sc = 1.f, sh = 0.f;
            if constexpr (AFF) {
                if (co < Cout) { sc = scale[co]; sh = shift[co]; }
            }
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int row = sb * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;     // D[row][col = l]
                float v = acc[a][r];
                if constexpr (AFF) v = sc_affine(v, sc, sh, relu);
                if (row < nrow && co < Cout) out[(size_t)(o0 + row) * Cout + co] = v;
            }
        }
    }
}

// ---- output-stationary gather-GEMM with the gathered rows in REGISTERS (round 3) -------------------------------------------------
// spconv_gather_gemm_kernel stages every offset's 64 gathered rows AND W_k through LDS between two barriers, with nothing in
// flight while it multiplies: 5 ms per 64-channel layer at config c3 (21 TFLOP/s).  Here a wave owns 32 output rows for the whole
// kernel and the MFMA's A operand comes straight from global memory:
//   * v_mfma_f32_32x32x2_f32 sums over a k index whose ORDER is free as long as A and B agree.  With k = h * (C_in / 2) + s
//     (h = lane / 32, s = step) lane (l, h) needs elements [h * C_in / 2, (h + 1) * C_in / 2) of the gathered row of output row l:
//     one contiguous run -- C_in / 8 16-byte loads, no LDS round trip, no transposition;
//   * the rows of offset k + 1 (and the table entry of k + 2) are in flight while offset k is multiplied;
//   * W_k goes through a double-buffered LDS tile filled by all four waves (one barrier per offset); lanes read it with unit
//     stride along the output channel (conflict-free).
// Same sums in another order (rows with no neighbour contribute zeros), so results agree with the LDS kernel to fp32 rounding.
// CINP: C_in rounded up to {4, 16, 32, 64, 128}; NCB: 32-column blocks of the output (C_out <= 32 * NCB).
// AFF: the store applies sc_affine; the lane's NCB scale / shift values (columns 32 a + l) are loaded once, after the last offset,
// when the gathered-row registers are dead: the main loop and its register budget are those of the plain instantiation.
template <int CINP, int NCB, bool AFF>
__global__ __launch_bounds__(256) void spconv_os_kernel(int No, int K, int Cin, int Cout, const float *__restrict__ in,
                                                        const int *__restrict__ nbr, const float *__restrict__ w, int flip_k,
                                                        const float *__restrict__ scale, const float *__restrict__ shift, int relu,
                                                        float *__restrict__ out) {
    constexpr int CH = CINP / 2;                 // k steps per MFMA half = elements of its row a lane holds
    constexpr int COUTP = NCB * 32;
    constexpr int WPT = CINP * COUTP / 256;      // floats of W_k each thread stages (>= 1 for every instantiation)
    __shared__ float Wl[2][CINP * COUTP];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int l = lane & 31, h = lane >> 5;
    const int row = blockIdx.x * 128 + wave * 32 + l;
    const bool rok = row < No;
    const int *__restrict__ nrow = nbr + (size_t)(rok ? row : 0) * K;
    f32x16 acc[NCB];
#pragma unroll
    for (int a = 0; a < NCB; ++a)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[a][r] = 0.f;
    float areg0[CH], areg1[CH];                  // the gathered rows of the current / next offset (two named arrays: static register indices)
    float wreg[WPT];
    auto load_w = [&](int k) {
        const float *wk = w + (size_t)(flip_k ? K - 1 - k : k) * Cin * Cout;
#pragma unroll
        for (int q = 0; q < WPT; ++q) {
            const int e = q * 256 + threadIdx.x;
            const int ci = e / COUTP, co = e - ci * COUTP;
            wreg[q] = (ci < Cin && co < Cout) ? wk[(size_t)ci * Cout + co] : 0.f;
        }
    };
    auto store_w = [&](int buf) {
#pragma unroll
        for (int q = 0; q < WPT; ++q) Wl[buf][q * 256 + threadIdx.x] = wreg[q];
    };
    auto load_a = [&](float (&dst)[CH], int j) {
        if (j >= 0) {
            const float *src = in + (size_t)j * Cin + h * CH;
            if constexpr (CH % 4 == 0) {
                if (Cin == CINP) {
#pragma unroll
                    for (int q = 0; q < CH / 4; ++q) {
                        const float4 v = *reinterpret_cast<const float4 *>(src + 4 * q);
                        dst[4 * q + 0] = v.x; dst[4 * q + 1] = v.y; dst[4 * q + 2] = v.z; dst[4 * q + 3] = v.w;
                    }
                    return;
                }
            }
#pragma unroll
            for (int q = 0; q < CH; ++q) dst[q] = (h * CH + q < Cin) ? src[q] : 0.f;
        } else {
#pragma unroll
            for (int q = 0; q < CH; ++q) dst[q] = 0.f;
        }
    };
    int j_next = -1;
    // one offset: rows of offset k are in `cur`, W_k in Wl[buf]; fetch offset k + 1 into `nxt` / the other W buffer meanwhile
    auto step = [&](int k, int buf, float (&cur)[CH], float (&nxt)[CH]) {
        const int j1 = j_next;
        if (k + 1 < K) {
            load_w(k + 1);                                    // in flight during the MFMAs below
            j_next = (rok && k + 2 < K) ? nrow[k + 2] : -1;
            load_a(nxt, j1);
        }
        const float *Wk = Wl[buf];
#pragma unroll
        for (int s = 0; s < CH; ++s) {
            const float av = cur[s];
#pragma unroll
            for (int a = 0; a < NCB; ++a) {
                const float bv = Wk[(h * CH + s) * COUTP + a * 32 + l];
                acc[a] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bv, acc[a], 0, 0, 0);
            }
        }
        if (k + 1 < K) store_w(buf ^ 1);
        __syncthreads();                                      // W_{k+1} visible; W_k's buffer is free for offset k + 2
    };
    // prologue: W_0 -> LDS, rows of offset 0 -> registers, table entry of offset 1
    load_w(0);
    j_next = (rok && K > 1) ? nrow[1] : -1;
    load_a(areg0, rok ? nrow[0] : -1);
    store_w(0);
    __syncthreads();
    for (int k = 0; k < K; k += 2) {
        step(k, 0, areg0, areg1);
        if (k + 1 < K) step(k + 1, 1, areg1, areg0);
    }
    const int obase = blockIdx.x * 128 + wave * 32;
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
            const int orow = obase + (r & 3) + 8 * (r >> 2) + 4 * h;
            float v = acc[a][r];
            if constexpr (AFF) v = sc_affine(v, sc[a], sh[a], relu);
            if (orow < No && co < Cout) out[(size_t)orow * Cout + co] = v;
        }
    }
}

// ---- weight gradient: dW[k] (Cin, Cout) = sum_o in[nbr[o, k], :]^T dout[o, :] ----------------------------------------------
// grid (K, nchunk) -- the K workgroups of one row chunk are neighbours in launch order, so the chunk's dout rows and the input
// rows around it are fetched from HBM once and then served by L2 / MALL to the other offsets;
// partial[(chunk * K + k)][Cin][Cout]; chunk = SC_DW_CHUNK output rows
constexpr int SC_DW_CHUNK = 8192;

__global__ __launch_bounds__(256) void spconv_dw_kernel(int No, int K, int Cin, int Cout, const float *__restrict__ in,
                                                        const int *__restrict__ nbr, const float *__restrict__ dout,
                                                        float *__restrict__ partial) {
    extern __shared__ float lds[];
    const int CoutP = (Cout + 31) & ~31, CinP = (Cin + 31) & ~31;
    float *A = lds;                                   // [SC_ROWS][CinP + 1]   gathered input rows (zero where no neighbour)
    float *G = A + SC_ROWS * (CinP + 1);              // [SC_ROWS][CoutP + 1]  dout rows
    __shared__ int nbk[SC_ROWS];
    __shared__ int any_flag[2];                        // alternating between tiles: a reader of tile t never meets the reset of t + 1
    const int k = blockIdx.x, chunk = blockIdx.y;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int l = lane & 31, h = lane >> 5;
    const int nib = CinP / 32, ncb = CoutP / 32, nblk = nib * ncb;     // 32x32 blocks of dW_k; wave w owns blocks w, w+4, ...
    f32x16 acc[4];                                                      // nblk <= 16 -> at most 4 per wave
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[a][r] = 0.f;
    const int row0 = chunk * SC_DW_CHUNK, row1 = min(No, row0 + SC_DW_CHUNK);
    int par = 0;
    for (int t0 = row0; t0 < row1; t0 += SC_ROWS, par ^= 1) {
        const int nrow = min(SC_ROWS, row1 - t0);
        if (threadIdx.x == 0) any_flag[par] = 0;
        __syncthreads();
        if (threadIdx.x < SC_ROWS) {
            const int j = threadIdx.x < nrow ? nbr[(size_t)(t0 + threadIdx.x) * K + k] : -1;
            nbk[threadIdx.x] = j;
            if (j >= 0) any_flag[par] = 1;
        }
        __syncthreads();
        if (!any_flag[par]) continue;
        for (int e = threadIdx.x; e < SC_ROWS * CinP; e += 256) {
            const int r = e / CinP, c = e - r * CinP;
            const int j = nbk[r];
            A[r * (CinP + 1) + c] = (j >= 0 && c < Cin) ? in[(size_t)j * Cin + c] : 0.f;
        }
        for (int e = threadIdx.x; e < SC_ROWS * CoutP; e += 256) {
            const int r = e / CoutP, c = e - r * CoutP;
            G[r * (CoutP + 1) + c] = (r < nrow && c < Cout && nbk[r] >= 0) ? dout[(size_t)(t0 + r) * Cout + c] : 0.f;
        }
        __syncthreads();
#pragma unroll
        for (int a = 0; a < 4; ++a) {                    // static accumulator indices: no scratch
            const int blk = wave + 4 * a;
            if (blk < nblk) {
                const int ib = blk / ncb, cb = blk - ib * ncb;
#pragma unroll 4
                for (int s = 0; s < SC_ROWS / 2; ++s) {  // reduction over the 64 rows of the tile, 2 per MFMA
                    const float av = A[(2 * s + h) * (CinP + 1) + ib * 32 + l];      // A^T: row = ci, k = site
                    const float bv = G[(2 * s + h) * (CoutP + 1) + cb * 32 + l];
                    acc[a] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bv, acc[a], 0, 0, 0);
                }
            }
        }
        // the next tile's first barrier orders these LDS reads before its staging writes
    }
    float *dst = partial + ((size_t)chunk * K + k) * Cin * Cout;
#pragma unroll
    for (int a = 0; a < 4; ++a) {
        const int blk = wave + 4 * a;
        if (blk < nblk) {
            const int ib = blk / ncb, cb = blk - ib * ncb;
            const int co = cb * 32 + l;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int ci = ib * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
                if (ci < Cin && co < Cout) dst[(size_t)ci * Cout + co] = acc[a][r];
            }
        }
    }
}

// ---- weight gradient over PAIR LISTS ---------------------------------------------------------------------------------------
// The table form above spends most of its time on sites that have no neighbour under the offset at hand (LiDAR sparsity: ~7 of
// 27) and on a dependent chain per tile (table column -> gather -> LDS -> MFMA).  Here the caller compacts the table once per
// rulebook into, per offset k, the list of (input row, output row) pairs in ascending output order (both rows then ascend, so
// the two gathers are nearly sequential streams), cut into work items of at most SC_PAIR_CHUNK pairs of one offset.  A
// workgroup owns an item and software-pipelines 64-pair tiles: the indices of tile t + 2 and the rows of tile t + 1 are in
// flight while tile t is multiplied out of LDS.  dW_k = sum over the pairs of in[i]^T dout[o]; partial per item, summed per
// offset in item order by spconv_pairs_reduce_kernel (fixed order: reproducible).  C_in, C_out in {1, 2, 4, ..., 128}.
constexpr int SC_PAIR_CHUNK = 4096;
// SC_PREF: prefetch registers per operand = 64 rows * max(C_in, C_out) / 256 lanes (4, 8, 16 or 32)
template <int SC_PREF>
__global__ __launch_bounds__(256) void spconv_pairs_dw_kernel(int Cin, int Cout, const float *__restrict__ in,
                                                              const float *__restrict__ dout, const int *__restrict__ pair_i,
                                                              const int *__restrict__ pair_o, const int4 *__restrict__ items,
                                                              float *__restrict__ partial) {
    extern __shared__ float lds[];
    const int CoutP = (Cout + 31) & ~31, CinP = (Cin + 31) & ~31, ALD = CinP + 1, GLD = CoutP + 1;
    float *A = lds;                                   // [64][ALD]  gathered input rows
    float *G = A + SC_ROWS * ALD;                     // [64][GLD]  gathered dout rows
    __shared__ int idx_i[3][SC_ROWS], idx_o[3][SC_ROWS];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int l = lane & 31, h = lane >> 5;
    const int4 item = items[blockIdx.x];
    const int pb = item.y, pe = item.z;
    const int ntiles = (pe - pb + SC_ROWS - 1) / SC_ROWS;
    // element mapping of the staging passes (256 % C == 0): pass q covers rows q * rp + tid / C, column tid % C
    const int ca = tid % Cin, ra = tid / Cin, rpa = 256 / Cin, qa = (SC_ROWS + rpa - 1) / rpa;
    const int cg = tid % Cout, rg = tid / Cout, rpg = 256 / Cout, qg = (SC_ROWS + rpg - 1) / rpg;
    for (int e = tid; e < SC_ROWS * (ALD + GLD); e += 256) lds[e] = 0.f;      // the padding columns stay zero
    const int nib = CinP / 32, ncb = CoutP / 32, nblk = nib * ncb;
    f32x16 acc[4];
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[a][r] = 0.f;
    float a_reg[SC_PREF], g_reg[SC_PREF];
    int vi = -1, vo = -1;
    auto load_idx = [&](int t) {
        const int p = pb + t * SC_ROWS + tid;
        const bool ok = t < ntiles && tid < SC_ROWS && p < pe;
        vi = ok ? pair_i[p] : -1;
        vo = ok ? pair_o[p] : -1;
    };
    auto store_idx = [&](int slot) {
        if (tid < SC_ROWS) { idx_i[slot][tid] = vi; idx_o[slot][tid] = vo; }
    };
    auto gather = [&](int slot) {
#pragma unroll
        for (int q = 0; q < SC_PREF; ++q) {
            const int r = q * rpa + ra;
            const int j = (q < qa && r < SC_ROWS) ? idx_i[slot][r] : -1;
            a_reg[q] = j >= 0 ? in[(size_t)j * Cin + ca] : 0.f;
        }
#pragma unroll
        for (int q = 0; q < SC_PREF; ++q) {
            const int r = q * rpg + rg;
            const int j = (q < qg && r < SC_ROWS) ? idx_o[slot][r] : -1;
            g_reg[q] = j >= 0 ? dout[(size_t)j * Cout + cg] : 0.f;
        }
    };
    auto put = [&]() {
#pragma unroll
        for (int q = 0; q < SC_PREF; ++q) {
            const int r = q * rpa + ra;
            if (q < qa && r < SC_ROWS) A[r * ALD + ca] = a_reg[q];
        }
#pragma unroll
        for (int q = 0; q < SC_PREF; ++q) {
            const int r = q * rpg + rg;
            if (q < qg && r < SC_ROWS) G[r * GLD + cg] = g_reg[q];
        }
    };
    load_idx(0);
    store_idx(0);
    load_idx(1);
    __syncthreads();
    gather(0);
    store_idx(1);
    load_idx(2);
    for (int t = 0; t < ntiles; ++t) {
        __syncthreads();                              // the previous tile's MFMA reads are done; index slot (t + 1) % 3 is visible
        put();
        if (t + 1 < ntiles) gather((t + 1) % 3);      // in flight during this tile's MFMA
        store_idx((t + 2) % 3);
        load_idx(t + 3);
        __syncthreads();
#pragma unroll
        for (int a = 0; a < 4; ++a) {
            const int blk = wave + 4 * a;
            if (blk < nblk) {
                const int ib = blk / ncb, cb = blk - ib * ncb;
#pragma unroll 4
                for (int sidx = 0; sidx < SC_ROWS / 2; ++sidx) {
                    const float av = A[(2 * sidx + h) * ALD + ib * 32 + l];
                    const float bv = G[(2 * sidx + h) * GLD + cb * 32 + l];
                    acc[a] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bv, acc[a], 0, 0, 0);
                }
            }
        }
    }
    float *dst = partial + (size_t)blockIdx.x * Cin * Cout;
#pragma unroll
    for (int a = 0; a < 4; ++a) {
        const int blk = wave + 4 * a;
        if (blk < nblk) {
            const int ib = blk / ncb, cb = blk - ib * ncb;
            const int co = cb * 32 + l;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int ci = ib * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
                if (ci < Cin && co < Cout) dst[(size_t)ci * Cout + co] = acc[a][r];
            }
        }
    }
}

// ---- forward / data gradient over PAIR LISTS -----------------------------------------------------------------------------
// dst[pair_dst[p], :] += src[pair_src[p], :] . W   for the pairs of ONE kernel offset (W = W_k, C_src x C_dst, row-major).  Under
// one offset every destination row occurs at most once (o -> i = o * stride - pad + k is injective), so the update is a plain
// read-modify-write without atomics; the launcher runs the offsets one after the other on the stream, which also fixes the
// order of the sum over k.  Forward: src = input rows, dst = output rows; data gradient: src = dout rows, dst = input rows,
// W = W_k^T -- no inverse table.  A workgroup owns an item (<= SC_PAIR_CHUNK pairs): W stays in LDS for the whole item, 64-pair
// tiles are software-pipelined (rows of tile t + 1 and the old destination values of tile t in flight during the MFMA of t).
template <int SC_PREF>
__global__ __launch_bounds__(256) void spconv_pairs_gemm_kernel(int Cs, int Cd, const float *__restrict__ src,
                                                                const int *__restrict__ pair_src, const int *__restrict__ pair_dst,
                                                                const int4 *__restrict__ items, const float *__restrict__ w,
                                                                float *__restrict__ dst) {
    extern __shared__ float lds[];
    const int CdP = (Cd + 31) & ~31, CsP = (Cs + 1) & ~1, ALD = CsP + 1;
    float *A = lds;                                   // [64][ALD]   gathered source rows
    float *W = A + SC_ROWS * ALD;                     // [CsP][CdP]
    __shared__ int idx_s[3][SC_ROWS], idx_d[3][SC_ROWS];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int l = lane & 31, h = lane >> 5;
    const int4 item = items[blockIdx.x];
    const int pb = item.y, pe = item.z;
    const int ntiles = (pe - pb + SC_ROWS - 1) / SC_ROWS;
    const int ca = tid % Cs, ra = tid / Cs, rpa = 256 / Cs, qa = (SC_ROWS + rpa - 1) / rpa;
    for (int e = tid; e < SC_ROWS * ALD; e += 256) A[e] = 0.f;                // padding column(s) stay zero
    for (int e = tid; e < CsP * CdP; e += 256) {
        const int ci = e / CdP, co = e - ci * CdP;
        W[e] = (ci < Cs && co < Cd) ? w[(size_t)ci * Cd + co] : 0.f;
    }
    const int sb = wave & 1, ncb = CdP / 32;
    float a_reg[SC_PREF];
    int vs = -1, vd = -1;
    auto load_idx = [&](int t) {
        const int p = pb + t * SC_ROWS + tid;
        const bool ok = t < ntiles && tid < SC_ROWS && p < pe;
        vs = ok ? pair_src[p] : -1;
        vd = ok ? pair_dst[p] : -1;
    };
    auto store_idx = [&](int slot) {
        if (tid < SC_ROWS) { idx_s[slot][tid] = vs; idx_d[slot][tid] = vd; }
    };
    auto gather = [&](int slot) {
#pragma unroll
        for (int q = 0; q < SC_PREF; ++q) {
            const int r = q * rpa + ra;
            const int j = (q < qa && r < SC_ROWS) ? idx_s[slot][r] : -1;
            a_reg[q] = j >= 0 ? src[(size_t)j * Cs + ca] : 0.f;
        }
    };
    auto put = [&]() {
#pragma unroll
        for (int q = 0; q < SC_PREF; ++q) {
            const int r = q * rpa + ra;
            if (q < qa && r < SC_ROWS) A[r * ALD + ca] = a_reg[q];
        }
    };
    load_idx(0);
    store_idx(0);
    load_idx(1);
    __syncthreads();
    gather(0);
    store_idx(1);
    load_idx(2);
    for (int t = 0; t < ntiles; ++t) {
        __syncthreads();
        put();
        if (t + 1 < ntiles) gather((t + 1) % 3);
        store_idx((t + 2) % 3);
        load_idx(t + 3);
        __syncthreads();
        const int slot = t % 3;
#pragma unroll
        for (int a = 0; a < 2; ++a) {
            const int cb = (wave >> 1) + 2 * a;
            if (cb < ncb) {
                const int co = cb * 32 + l;
                float old[16];
                int row_of[16];
#pragma unroll
                for (int r = 0; r < 16; ++r) {                                 // the old destination values: in flight during the MFMA
                    const int j = idx_d[slot][sb * 32 + (r & 3) + 8 * (r >> 2) + 4 * h];
                    row_of[r] = j;
                    old[r] = (j >= 0 && co < Cd) ? dst[(size_t)j * Cd + co] : 0.f;
                }
                f32x16 acc;
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[r] = 0.f;
                for (int sidx = 0; sidx < CsP / 2; ++sidx) {
                    const float av = A[(sb * 32 + l) * ALD + 2 * sidx + h];
                    const float bv = W[(2 * sidx + h) * CdP + co];
                    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bv, acc, 0, 0, 0);
                }
#pragma unroll
                for (int r = 0; r < 16; ++r)
                    if (row_of[r] >= 0 && co < Cd) dst[(size_t)row_of[r] * Cd + co] = old[r] + acc[r];
            }
        }
    }
}

// dW[k][e] = sum of partial[item][e] over the items of offset k, in item order.  grid (ceil(Cin * Cout / 256), K)
__global__ __launch_bounds__(256) void spconv_pairs_reduce_kernel(int elems, const int *__restrict__ item_start,
                                                                  const float *__restrict__ partial, float *__restrict__ dw) {
    const int e = blockIdx.x * 256 + threadIdx.x, k = blockIdx.y;
    if (e >= elems) return;
    float s = 0.f;
    for (int it = item_start[k]; it < item_start[k + 1]; ++it) s = s + partial[(size_t)it * elems + e];
    dw[(size_t)k * elems + e] = s;
}

static bool sp_geom_ok(const int *g) {
    for (int i = 0; i < 6; ++i)
        if (g[i] < 1) return false;
    for (int i = 6; i < 9; ++i)
        if (g[i] < 0) return false;
    for (int i = 9; i < 15; ++i)
        if (g[i] < 1) return false;
    return true;
}

// ---- pair lists from the neighbour table, on the device (round 3) -------------------------------------------------------------
// nbr (No, K) -> for every offset k the (input row, output row) pairs with a neighbour, ascending output row, offsets one after
// another: pair_i / pair_o (P).  Three launches instead of the six torch passes (mask, transpose, sum, nonzero, two index
// gathers: ~10 ms per rulebook at 4 M sites):
//   sp_pairs_count_kernel  a workgroup owns SP_PB consecutive rows (its tile of the table staged in LDS): per offset, how many of them
//                          have a neighbour -> blk (K, nblk)
//   sp_pairs_scan_kernel   one workgroup per offset: exclusive scan over the row blocks (in place) + the offset's total
//   sp_pairs_fill_kernel   the same workgroups rank their rows per offset (ballot prefix inside a wave, the waves in order) and write
//                          the pairs at  offset_start[k] + blk[k][b] + rank  -- stable: ascending output row, deterministic.
constexpr int SP_PB = 512;    // rows per workgroup: 4 waves x 2 groups of 64 rows; the (SP_PB, K) tile of the table is staged in LDS
constexpr int SP_PG = SP_PB / 64;   // 64-row groups per workgroup (group g belongs to wave g / 2)

// the workgroup's (rows, K) tile of the neighbour table -> LDS with coalesced reads (the per-offset passes below read it with a
// stride of K words: conflict-free for odd K, and never from global memory)
__device__ __forceinline__ void sp_pairs_stage(int No, int K, int row0, const int *__restrict__ nbr, int *__restrict__ tile) {
    const long long base = (long long)row0 * K;
    const int n = min(SP_PB, No - row0) * K;
    for (int e = threadIdx.x; e < SP_PB * K; e += 256) tile[e] = e < n ? nbr[base + e] : -1;
}

// gcnt[g * K + k] = rows of 64-row group g with a neighbour under offset k
__device__ __forceinline__ void sp_pairs_group_counts(int K, const int *__restrict__ tile, int *__restrict__ gcnt) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int gg = 0; gg < 2; ++gg) {
        const int g = wave * 2 + gg;
        const int *r = tile + (g * 64 + lane) * K;
        for (int k = 0; k < K; ++k) {
            const unsigned long long m = __builtin_amdgcn_ballot_w64(r[k] >= 0);
            if (lane == 0) gcnt[g * K + k] = __builtin_popcountll(m);
        }
    }
}

__global__ __launch_bounds__(256) void sp_pairs_count_kernel(int No, int K, const int *__restrict__ nbr, int *__restrict__ blk) {
    extern __shared__ int lds_i[];   // tile [SP_PB][K], gcnt [SP_PG][K]
    int *tile = lds_i, *gcnt = lds_i + SP_PB * K;
    const int b = blockIdx.x, nblk = gridDim.x;
    sp_pairs_stage(No, K, b * SP_PB, nbr, tile);
    __syncthreads();
    sp_pairs_group_counts(K, tile, gcnt);
    __syncthreads();
    for (int k = threadIdx.x; k < K; k += 256) {
        int t = 0;
#pragma unroll
        for (int g = 0; g < SP_PG; ++g) t += gcnt[g * K + k];
        blk[(size_t)k * nblk + b] = t;
    }
}

__global__ __launch_bounds__(1024) void sp_pairs_scan_kernel(int nblk, int *__restrict__ blk, int *__restrict__ total) {
    __shared__ int part[1024];
    const int k = blockIdx.x, t = threadIdx.x;
    int *row = blk + (size_t)k * nblk;
    const int per = (nblk + 1023) / 1024;
    const int b0 = t * per, b1 = min(b0 + per, nblk);
    int s = 0;
    for (int b = b0; b < b1; ++b) s += row[b];
    part[t] = s;
    __syncthreads();
    for (int off = 1; off < 1024; off <<= 1) {
        const int add = t >= off ? part[t - off] : 0;
        __syncthreads();
        part[t] += add;
        __syncthreads();
    }
    int run = part[t] - s;
    for (int b = b0; b < b1; ++b) { const int c = row[b]; row[b] = run; run += c; }
    if (t == 1023) total[k] = part[1023];
}

__global__ __launch_bounds__(256) void sp_pairs_fill_kernel(int No, int K, const int *__restrict__ nbr, const int *__restrict__ blk,
                                                            const long long *__restrict__ offset_start, int *__restrict__ pair_i,
                                                            int *__restrict__ pair_o) {
    extern __shared__ int lds_i[];   // tile [SP_PB][K], gcnt [SP_PG][K]
    int *tile = lds_i, *gcnt = lds_i + SP_PB * K;
    const int b = blockIdx.x, nblk = gridDim.x;
    const int row0 = b * SP_PB;
    sp_pairs_stage(No, K, row0, nbr, tile);
    __syncthreads();
    sp_pairs_group_counts(K, tile, gcnt);
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int gg = 0; gg < 2; ++gg) {
        const int g = wave * 2 + gg;
        const int row = row0 + g * 64 + lane;
        const int *r = tile + (g * 64 + lane) * K;
        for (int k = 0; k < K; ++k) {
            const int v = r[k];
            const unsigned long long m = __builtin_amdgcn_ballot_w64(v >= 0);
            if (m == 0ull) continue;                     // wave-uniform
            int before = 0;
            for (int q = 0; q < g; ++q) before += gcnt[q * K + k];   // the groups in front of this one (ascending rows)
            if (v >= 0) {
                const long long pos = offset_start[k] + blk[(size_t)k * nblk + b] + before + __builtin_popcountll(m & ((1ull << lane) - 1ull));
                pair_i[pos] = v;
                pair_o[pos] = row;
            }
        }
    }
}

}  // namespace mgar

using namespace mgar;

static int g_spconv_os = 1;
// A/B switch (tests, profiles): 1 = register-gather kernel where it applies (default), 0 = always the LDS kernel
MGAR_API int mgar_spconv_set_register_gather(int on) { g_spconv_os = on ? 1 : 0; return MGAR_OK; }

// Hash table over the voxel coordinates coords (N, 4) int32 [b, z, y, x] of a (Z, Y, X) grid.  table_keys (capacity) int64
// must be pre-filled with -1 and table_vals (capacity) int32 with INT_MAX by the caller; capacity a power of two >= 2 N.
MGAR_API int mgar_voxel_hash_build(int N, const int *coords, int Z, int Y, int X, long long *table_keys, int *table_vals,
                                   int capacity, void *stream) {
    MGAR_REQUIRE(N >= 0 && Z > 0 && Y > 0 && X > 0 && capacity > 0 && (capacity & (capacity - 1)) == 0 && capacity >= 2 * N,
                 "voxel_hash_build: capacity must be a power of two >= 2 N");
    if (N == 0) return MGAR_OK;
    MGAR_REQUIRE(coords && table_keys && table_vals, "voxel_hash_build: null pointer");
    KtScope kt(KT_SPCONV_INDEX, (hipStream_t)stream, 16.0 * N + 12.0 * N);   // coords read, one (key, value) slot written per site
    hipLaunchKernelGGL(sph_build_kernel, dim3(ceil_div(N, 256)), dim3(256), 0, (hipStream_t)stream, N, coords, Z, Y, X, table_keys,
                       table_vals, capacity - 1);
    return check_launch("voxel_hash_build: launch failed");
}

// rows[i] = row id stored for coords[i] (M, 4), or -1 (the sparse replacement of indexing the dense (B, Z, Y, X) table of
// pcdet/utils/common_utils.py:244-252)
MGAR_API int mgar_voxel_hash_lookup(int M, const int *coords, int Z, int Y, int X, const long long *table_keys, const int *table_vals,
                                    int capacity, int *rows, void *stream) {
    MGAR_REQUIRE(M >= 0 && Z > 0 && Y > 0 && X > 0 && capacity > 0 && (capacity & (capacity - 1)) == 0, "voxel_hash_lookup: bad sizes");
    if (M == 0) return MGAR_OK;
    MGAR_REQUIRE(coords && table_keys && table_vals && rows, "voxel_hash_lookup: null pointer");
    KtScope kt(KT_SPCONV_INDEX, (hipStream_t)stream, 16.0 * M + 12.0 * M + 4.0 * M);   // coords, one probed slot, one row id
    hipLaunchKernelGGL(sph_lookup_kernel, dim3(ceil_div(M, 256)), dim3(256), 0, (hipStream_t)stream, M, coords, Z, Y, X, table_keys,
                       table_vals, capacity - 1, rows);
    return check_launch("voxel_hash_lookup: launch failed");
}

// Rulebook of one sparse convolution.  geom: 15 HOST ints {kz,ky,kx, sz,sy,sx, pz,py,px, Zi,Yi,Xi, Zo,Yo,Xo}.
//   inverse = 0: site_coords = OUTPUT sites (No, 4), table = hash of the INPUT sites -> nbr (No, K): input row under offset k
//   inverse = 1: site_coords = INPUT sites (Ni, 4), table = hash of the OUTPUT sites -> nbr (Ni, K): output row reached through k
// K = kz * ky * kx, offsets ordered z-major (k = (kz * KY + ky) * KX + kx, the order of spconv's (O, kd, kh, kw, I) weight).
MGAR_API int mgar_spconv_rulebook(int n_sites, const int *site_coords, const int *geom, const long long *table_keys,
                                  const int *table_vals, int capacity, int inverse, int *nbr, void *stream) {
    MGAR_REQUIRE(n_sites >= 0 && geom && sp_geom_ok(geom) && capacity > 0 && (capacity & (capacity - 1)) == 0, "spconv_rulebook: bad geometry");
    if (n_sites == 0) return MGAR_OK;
    MGAR_REQUIRE(site_coords && table_keys && table_vals && nbr, "spconv_rulebook: null pointer");
    SpGeom g{geom[0], geom[1], geom[2], geom[3], geom[4], geom[5], geom[6], geom[7], geom[8], geom[9], geom[10], geom[11], geom[12],
             geom[13], geom[14]};
    const int K = g.kz * g.ky * g.kx;
    const long long total = (long long)n_sites * K;
    MGAR_REQUIRE(total / 256 < 2147483647LL, "spconv_rulebook: too many (site, offset) pairs");
    KtScope kt(KT_SPCONV_INDEX, (hipStream_t)stream, 16.0 * n_sites + (double)total * (12.0 + 4.0));   // one probe + one table entry per (site, offset)
    if (inverse)
        hipLaunchKernelGGL(sp_neighbors_inverse_kernel, dim3(ceil_div(total, 256)), dim3(256), 0, (hipStream_t)stream, total, K, site_coords,
                           g, table_keys, table_vals, capacity - 1, nbr);
    else
        hipLaunchKernelGGL(sp_neighbors_kernel, dim3(ceil_div(total, 256)), dim3(256), 0, (hipStream_t)stream, total, K, site_coords, g,
                           table_keys, table_vals, capacity - 1, nbr);
    return check_launch("spconv_rulebook: launch failed");
}

// keys (n_in, K) int64: see sp_output_keys_kernel.  geom as in mgar_spconv_rulebook.
MGAR_API int mgar_spconv_output_keys(int n_in, const int *in_coords, const int *geom, long long *keys, void *stream) {
    MGAR_REQUIRE(n_in >= 0 && geom && sp_geom_ok(geom), "spconv_output_keys: bad geometry");
    if (n_in == 0) return MGAR_OK;
    MGAR_REQUIRE(in_coords && keys, "spconv_output_keys: null pointer");
    SpGeom g{geom[0], geom[1], geom[2], geom[3], geom[4], geom[5], geom[6], geom[7], geom[8], geom[9], geom[10], geom[11], geom[12],
             geom[13], geom[14]};
    const int K = g.kz * g.ky * g.kx;
    const long long total = (long long)n_in * K;
    MGAR_REQUIRE(total / 256 < 2147483647LL, "spconv_output_keys: too many (site, offset) pairs");
    KtScope kt(KT_SPCONV_INDEX, (hipStream_t)stream, 16.0 * n_in + 8.0 * (double)total);
    hipLaunchKernelGGL(sp_output_keys_kernel, dim3(ceil_div(total, 256)), dim3(256), 0, (hipStream_t)stream, total, K, in_coords, g, keys);
    return check_launch("spconv_output_keys: launch failed");
}

// The two forward entry points below share one launcher.  AFF = false: the plain store (mgar_spconv_gather_gemm, scale / shift
// unused); AFF = true: the sc_affine store (mgar_spconv_gather_gemm_affine).  Same plans, same kernel choice, same timer row.
template <bool AFF>
static int spconv_gather_gemm_launch(int No, int K, int Cin, int Cout, const float *in, const int *nbr, const float *w, int flip_k,
                                     const float *scale, const float *shift, int relu, float *out, void *stream) {
    {
        // register-gather kernel (spconv_os_kernel) for the channel counts of VoxelBackBone8x; anything else: the LDS kernel below
        const int cinp = Cin <= 4 ? 4 : (Cin <= 16 ? 16 : (Cin <= 32 ? 32 : (Cin <= 64 ? 64 : 128)));
        const int ncb = (Cout + 31) / 32;
        const bool aligned = (Cin == cinp ? (reinterpret_cast<uintptr_t>(in) & 15) == 0 : true);
        hipStream_t st = (hipStream_t)stream;
        const dim3 grid(ceil_div(No, 128));
#define SP_OS(CI, NB)                                                                                                        \
        do {                                                                                                                     \
            KtScope kt(KT_SPCONV_GEMM, st, 4.0 * No * ((double)K + Cout) + 4.0 * (double)K * Cin * Cout);                        \
            hipLaunchKernelGGL((spconv_os_kernel<CI, NB, AFF>), grid, dim3(256), 0, st, No, K, Cin, Cout, in, nbr, w, flip_k,     \
                               scale, shift, relu, out);                                                                         \
            return check_launch("spconv_gather_gemm: launch failed");                                                            \
        } while (0)
        if (g_spconv_os && aligned && cinp * ncb * 32 >= 256 && cinp * ncb * 32 * 8 <= 64 * 1024) {
            if (cinp == 16 && ncb == 1) SP_OS(16, 1);
            if (cinp == 32 && ncb == 1) SP_OS(32, 1);
            if (cinp == 32 && ncb == 2) SP_OS(32, 2);
            if (cinp == 64 && ncb == 1) SP_OS(64, 1);
            if (cinp == 64 && ncb == 2) SP_OS(64, 2);
            if (cinp == 128 && ncb == 2) SP_OS(128, 2);
            if (cinp == 16 && ncb == 2) SP_OS(16, 2);
        }
#undef SP_OS
    }
    const int CoutP = (Cout + 31) & ~31, CinP = (Cin + 1) & ~1;
    const size_t lds = ((size_t)SC_ROWS * K + (size_t)SC_ROWS * (CinP + 1) + (size_t)CinP * CoutP) * sizeof(float);
    MGAR_REQUIRE(lds <= 160 * 1024, "spconv_gather_gemm: tile does not fit LDS");
    static size_t attr_lds = 0;                          // one per instantiation of this template = one per kernel
    if (lds > 65536 && lds > attr_lds) {
        (void)hipFuncSetAttribute((const void *)spconv_gather_gemm_kernel<AFF>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        attr_lds = lds;
    }
    // table (No, K) read, out written; the gathered input rows and the flops depend on the number of pairs, which the caller
    // credits (mgar_ktimer_add_bytes / _flops)
    KtScope kt(KT_SPCONV_GEMM, (hipStream_t)stream, 4.0 * No * ((double)K + Cout) + 4.0 * (double)K * Cin * Cout);
    hipLaunchKernelGGL(spconv_gather_gemm_kernel<AFF>, dim3(ceil_div(No, SC_ROWS)), dim3(256), lds, (hipStream_t)stream, No, K, Cin, Cout,
                       in, nbr, w, flip_k, scale, shift, relu, out);
    return check_launch("spconv_gather_gemm: launch failed");
}

// out (No, Cout) = sum_k in[nbr[:, k]] . w[k]   with w (K, Cin, Cout) row-major; rows with nbr == -1 contribute nothing.
// flip_k != 0 reads w[K - 1 - k] (data gradient of a submanifold convolution: its inverse rulebook is the forward one
// with the offsets mirrored).  out is fully written.  Cin, Cout <= 128.
MGAR_API int mgar_spconv_gather_gemm(int No, int K, int Cin, int Cout, const float *in, const int *nbr, const float *w, int flip_k,
                                     float *out, void *stream) {
    MGAR_REQUIRE(No >= 0 && K >= 1 && K <= 343 && Cin >= 1 && Cout >= 1, "spconv_gather_gemm: bad sizes");
    if (Cin > SC_MAXC || Cout > SC_MAXC) {
        set_error("spconv_gather_gemm: C_in, C_out <= 128");
        return MGAR_EUNSUPPORTED;
    }
    if (No == 0) return MGAR_OK;
    MGAR_REQUIRE(in && nbr && w && out, "spconv_gather_gemm: null pointer");
    return spconv_gather_gemm_launch<false>(No, K, Cin, Cout, in, nbr, w, flip_k, nullptr, nullptr, 0, out, stream);
}

// mgar_spconv_gather_gemm with an eval-mode BatchNorm [+ ReLU] folded into the store: with acc the fp32 value that entry point
// would have stored (same sum, same order), out = sc_affine(acc, scale[c], shift[c], relu).  scale, shift (Cout) fp32, both
// required.  Same plans, kernels (mgar_spconv_set_register_gather) and refusals.
MGAR_API int mgar_spconv_gather_gemm_affine(int No, int K, int Cin, int Cout, const float *in, const int *nbr, const float *w,
                                            int flip_k, const float *scale, const float *shift, int relu, float *out, void *stream) {
    MGAR_REQUIRE(No >= 0 && K >= 1 && K <= 343 && Cin >= 1 && Cout >= 1, "spconv_gather_gemm_affine: bad sizes");
    if (Cin > SC_MAXC || Cout > SC_MAXC) {
        set_error("spconv_gather_gemm_affine: C_in, C_out <= 128");
        return MGAR_EUNSUPPORTED;
    }
    if (No == 0) return MGAR_OK;
    MGAR_REQUIRE(in && nbr && w && scale && shift && out, "spconv_gather_gemm_affine: null pointer");
    return spconv_gather_gemm_launch<true>(No, K, Cin, Cout, in, nbr, w, flip_k, scale, shift, relu ? 1 : 0, out, stream);
}

// weight gradient: partial (nchunk, K, Cin, Cout) with nchunk = mgar_spconv_dw_chunks(No); dW = partial.sum(0) (caller).
MGAR_API int mgar_spconv_dw_chunks(int No) { return No < 0 ? MGAR_EINVAL : (No + SC_DW_CHUNK - 1) / SC_DW_CHUNK; }
MGAR_API int mgar_spconv_dw(int No, int K, int Cin, int Cout, const float *in, const int *nbr, const float *dout, float *partial,
                            void *stream) {
    MGAR_REQUIRE(No >= 0 && K >= 1 && K <= 65535 && Cin >= 1 && Cout >= 1 && (No + SC_DW_CHUNK - 1) / SC_DW_CHUNK <= 65535, "spconv_dw: bad sizes");
    if (Cin > SC_MAXC || Cout > SC_MAXC) {
        set_error("spconv_dw: C_in, C_out <= 128");
        return MGAR_EUNSUPPORTED;
    }
    if (No == 0) return MGAR_OK;
    MGAR_REQUIRE(in && nbr && dout && partial, "spconv_dw: null pointer");
    const int CoutP = (Cout + 31) & ~31, CinP = (Cin + 31) & ~31;
    const size_t lds = ((size_t)SC_ROWS * (CinP + 1) + (size_t)SC_ROWS * (CoutP + 1)) * sizeof(float);
    static size_t attr_lds = 0;
    if (lds > 65536 && lds > attr_lds) {
        (void)hipFuncSetAttribute((const void *)spconv_dw_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        attr_lds = lds;
    }
    KtScope kt(KT_SPCONV_DW, (hipStream_t)stream, 4.0 * No * ((double)K + Cout) + 4.0 * (double)K * Cin * Cout);
    hipLaunchKernelGGL(spconv_dw_kernel, dim3(K, (No + SC_DW_CHUNK - 1) / SC_DW_CHUNK), dim3(256), lds, (hipStream_t)stream, No, K, Cin,
                       Cout, in, nbr, dout, partial);
    return check_launch("spconv_dw: launch failed");
}

// Weight gradient over pair lists (see spconv_pairs_dw_kernel).  pair_i / pair_o (P): input / output row of every (offset, site)
// pair, grouped by offset, ascending output row inside an offset; items (n_items, 4) int32 {k, first pair, end pair, 0}, at most
// mgar_spconv_pair_chunk() pairs each, grouped by offset in ascending order; item_start (K + 1): first item of every offset.
// partial (n_items, Cin, Cout) scratch; dw (K, Cin, Cout) fully written.  C_in, C_out powers of two <= 128
// (MGAR_EUNSUPPORTED otherwise: use mgar_spconv_dw).
MGAR_API int mgar_spconv_pair_chunk(void) { return SC_PAIR_CHUNK; }
MGAR_API int mgar_spconv_pairs_dw(int n_items, int K, int Cin, int Cout, const float *in, const float *dout, const int *pair_i,
                                  const int *pair_o, const int *items, const int *item_start, float *partial, float *dw, void *stream) {
    MGAR_REQUIRE(n_items >= 0 && K >= 1 && K <= 65535 && Cin >= 1 && Cout >= 1, "spconv_pairs_dw: bad sizes");
    if (Cin > SC_MAXC || Cout > SC_MAXC || (Cin & (Cin - 1)) || (Cout & (Cout - 1))) {
        set_error("spconv_pairs_dw: C_in, C_out must be powers of two <= 128");
        return MGAR_EUNSUPPORTED;
    }
    MGAR_REQUIRE(item_start && dw && (n_items == 0 || (in && dout && pair_i && pair_o && items && partial)), "spconv_pairs_dw: null pointer");
    hipStream_t st = (hipStream_t)stream;
    KtScope kt(KT_SPCONV_DW, st, 4.0 * (double)K * Cin * Cout);   // + 8 B of indices and both rows per pair: credited by the caller
    if (n_items > 0) {
        const int CoutP = (Cout + 31) & ~31, CinP = (Cin + 31) & ~31;
        const size_t lds = (size_t)SC_ROWS * (CinP + 1 + CoutP + 1) * sizeof(float);
        const int cmax = Cin > Cout ? Cin : Cout;
        const int4 *it4 = reinterpret_cast<const int4 *>(items);
        if (cmax <= 16) hipLaunchKernelGGL(spconv_pairs_dw_kernel<4>, dim3(n_items), dim3(256), lds, st, Cin, Cout, in, dout, pair_i, pair_o, it4, partial);
        else if (cmax <= 32) hipLaunchKernelGGL(spconv_pairs_dw_kernel<8>, dim3(n_items), dim3(256), lds, st, Cin, Cout, in, dout, pair_i, pair_o, it4, partial);
        else if (cmax <= 64) hipLaunchKernelGGL(spconv_pairs_dw_kernel<16>, dim3(n_items), dim3(256), lds, st, Cin, Cout, in, dout, pair_i, pair_o, it4, partial);
        else {
            static bool attr_set = false;
            if (!attr_set) {
                (void)hipFuncSetAttribute((const void *)spconv_pairs_dw_kernel<32>, hipFuncAttributeMaxDynamicSharedMemorySize, 80 * 1024);
                attr_set = true;
            }
            hipLaunchKernelGGL(spconv_pairs_dw_kernel<32>, dim3(n_items), dim3(256), lds, st, Cin, Cout, in, dout, pair_i, pair_o, it4, partial);
        }
    }
    hipLaunchKernelGGL(spconv_pairs_reduce_kernel, dim3(ceil_div(Cin * Cout, 256), K), dim3(256), 0, st, Cin * Cout, item_start, partial, dw);
    return check_launch("spconv_pairs_dw: launch failed");
}

// Forward / data gradient over pair lists (see spconv_pairs_gemm_kernel): for k = 0 .. K-1 in order,
//   dst[pair_dst[p], :] += src[pair_src[p], :] . w[k]   over the pairs of offset k.
// dst (n_dst, Cd) must be ZERO-FILLED by the caller; w (K, Cs, Cd) row-major; items / pair lists as for mgar_spconv_pairs_dw,
// item_start_host: the (K + 1) item offsets as a HOST array.  Forward: src = in, pair_src = pair_i, pair_dst = pair_o, w = W;
// data gradient: src = dout, pair_src = pair_o, pair_dst = pair_i, w = W_k^T.  C_s a power of two <= 128, C_d <= 128.
MGAR_API int mgar_spconv_pairs_gemm(int K, int Cs, int Cd, const float *src, const int *pair_src, const int *pair_dst, const int *items,
                                    const int *item_start_host, const float *w, float *dst, void *stream) {
    MGAR_REQUIRE(K >= 1 && K <= 65535 && Cs >= 1 && Cd >= 1 && item_start_host, "spconv_pairs_gemm: bad arguments");
    if (Cs > SC_MAXC || Cd > SC_MAXC || (Cs & (Cs - 1))) {
        set_error("spconv_pairs_gemm: C_src must be a power of two, both <= 128");
        return MGAR_EUNSUPPORTED;
    }
    if (item_start_host[K] == 0) return MGAR_OK;
    MGAR_REQUIRE(src && pair_src && pair_dst && items && w && dst, "spconv_pairs_gemm: null pointer");
    hipStream_t st = (hipStream_t)stream;
    const int CdP = (Cd + 31) & ~31, CsP = (Cs + 1) & ~1;
    const size_t lds = ((size_t)SC_ROWS * (CsP + 1) + (size_t)CsP * CdP) * sizeof(float);
    static size_t attr_lds[4] = {0, 0, 0, 0};
    const int variant = Cs <= 16 ? 0 : (Cs <= 32 ? 1 : (Cs <= 64 ? 2 : 3));
    if (lds > 65536 && lds > attr_lds[variant]) {
        const void *fn = variant == 0 ? (const void *)spconv_pairs_gemm_kernel<4>
                         : variant == 1 ? (const void *)spconv_pairs_gemm_kernel<8>
                         : variant == 2 ? (const void *)spconv_pairs_gemm_kernel<16> : (const void *)spconv_pairs_gemm_kernel<32>;
        (void)hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        attr_lds[variant] = lds;
    }
    KtScope kt(KT_SPCONV_GEMM, st, 4.0 * (double)K * Cs * Cd);   // all offsets of the layer = one row of the table; pairs credited by the caller
    for (int k = 0; k < K; ++k) {
        const int n = item_start_host[k + 1] - item_start_host[k];
        if (n <= 0) continue;
        const int4 *it = reinterpret_cast<const int4 *>(items) + item_start_host[k];
        const float *wk = w + (size_t)k * Cs * Cd;
        if (variant == 0) hipLaunchKernelGGL(spconv_pairs_gemm_kernel<4>, dim3(n), dim3(256), lds, st, Cs, Cd, src, pair_src, pair_dst, it, wk, dst);
        else if (variant == 1) hipLaunchKernelGGL(spconv_pairs_gemm_kernel<8>, dim3(n), dim3(256), lds, st, Cs, Cd, src, pair_src, pair_dst, it, wk, dst);
        else if (variant == 2) hipLaunchKernelGGL(spconv_pairs_gemm_kernel<16>, dim3(n), dim3(256), lds, st, Cs, Cd, src, pair_src, pair_dst, it, wk, dst);
        else hipLaunchKernelGGL(spconv_pairs_gemm_kernel<32>, dim3(n), dim3(256), lds, st, Cs, Cd, src, pair_src, pair_dst, it, wk, dst);
    }
    return check_launch("spconv_pairs_gemm: launch failed");
}

// Pair lists of a rulebook on the device.  Step 1: mgar_spconv_pairs_count fills blk (K, nblk) int32 with the per-row-block counts,
// scanned per offset, and total (K) int32; nblk = mgar_spconv_pairs_blocks(No).  The caller reads `total` (the one host
// synchronisation of a rulebook), forms offset_start (K) int64 = exclusive sums of total, allocates pair_i / pair_o (sum of total) and
// calls step 2, mgar_spconv_pairs_fill: pairs of offset k at [offset_start[k], offset_start[k] + total[k]), ascending output row.
MGAR_API int mgar_spconv_pairs_blocks(int No) { return No < 0 ? MGAR_EINVAL : (No + SP_PB - 1) / SP_PB; }
MGAR_API int mgar_spconv_pairs_count(int No, int K, const int *nbr, int *blk, int *total, void *stream) {
    MGAR_REQUIRE(No >= 0 && K >= 1 && K <= 4096, "spconv_pairs_count: bad sizes");
    MGAR_REQUIRE(total, "spconv_pairs_count: null pointer");
    hipStream_t st = (hipStream_t)stream;
    if (No == 0) { (void)hipMemsetAsync(total, 0, sizeof(int) * K, st); return MGAR_OK; }
    MGAR_REQUIRE(nbr && blk, "spconv_pairs_count: null pointer");
    const int nblk = (No + SP_PB - 1) / SP_PB;
    KtScope kt(KT_SPCONV_INDEX, st, 4.0 * (double)No * K);
    const size_t lds = (size_t)(SP_PB + SP_PG) * K * sizeof(int);
    MGAR_REQUIRE(lds <= 160 * 1024, "spconv_pairs_count: K too large for the LDS tile");
    if (lds > 65536) (void)hipFuncSetAttribute((const void *)sp_pairs_count_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    hipLaunchKernelGGL(sp_pairs_count_kernel, dim3(nblk), dim3(256), lds, st, No, K, nbr, blk);
    hipLaunchKernelGGL(sp_pairs_scan_kernel, dim3(K), dim3(1024), 0, st, nblk, blk, total);
    return check_launch("spconv_pairs_count: launch failed");
}
MGAR_API int mgar_spconv_pairs_fill(int No, int K, const int *nbr, const int *blk, const long long *offset_start, int *pair_i, int *pair_o,
                                    void *stream) {
    MGAR_REQUIRE(No >= 0 && K >= 1 && K <= 4096, "spconv_pairs_fill: bad sizes");
    if (No == 0) return MGAR_OK;
    MGAR_REQUIRE(nbr && blk && offset_start && pair_i && pair_o, "spconv_pairs_fill: null pointer");
    hipStream_t st = (hipStream_t)stream;
    const int nblk = (No + SP_PB - 1) / SP_PB;
    KtScope kt(KT_SPCONV_INDEX, st, 4.0 * (double)No * K + 8.0 * (double)No * K / 3.0);
    const size_t lds = (size_t)(SP_PB + SP_PG) * K * sizeof(int);
    MGAR_REQUIRE(lds <= 160 * 1024, "spconv_pairs_fill: K too large for the LDS tile");
    if (lds > 65536) (void)hipFuncSetAttribute((const void *)sp_pairs_fill_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    hipLaunchKernelGGL(sp_pairs_fill_kernel, dim3(nblk), dim3(256), lds, st, No, K, nbr, blk, offset_start, pair_i, pair_o);
    return check_launch("spconv_pairs_fill: launch failed");
}
