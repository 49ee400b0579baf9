// Shared device parts of the sparse implicit-GEMM kernels (sparse_conv.hip only): accumulators and the MFMA C/D
// mapping, the fused epilogue, the row-mask walk, W staging through registers, the register-A gather and its MFMA stage.
// Everything is __forceinline__ and works on the caller's arrays by reference.  The compiler does not give a kernel the same code
// as its own copy gave (§3.33 lists the register differences); sc_implicit_gemm_rega_kernel therefore uses only part of this file.
#pragma once

typedef float f32x16 __attribute__((ext_vector_type(16)));
#define IG_ROWS 128          // rows per workgroup (4 waves x 32)
#define IG_MAX_C 128

template <int NT>
__device__ __forceinline__ void ig_zero(f32x16 (&acc)[NT]) {
#pragma unroll
    for (int q = 0; q < NT; ++q)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[q][r] = 0.f;
}

// C/D layout of the 32x32 MFMA: accumulator register r of lane l holds column l & 31 of this row of the 32-row tile at row0
__device__ __forceinline__ int ig_cd_row(int row0, int r, int ak) { return row0 + (r & 3) + 8 * (r >> 2) + 4 * ak; }

// Fused epilogue of one 32-row tile starting at row0: out = act(acc (+ bias) (+ residual)); sorted tables scatter rows through
// out_row (NULL: table order).  Output row indices and residual values are requested eight rows at a time before any is used
// (clamped, unconditional loads: no wait per element).  n_out >= 1 (checked by the launcher).
template <int NT>
__device__ __forceinline__ void ig_epilogue(const f32x16 (&acc)[NT], int row0, int ar, int ak, int n_out, int Cout, const float *__restrict__ bias,
                                            const float *__restrict__ residual, int relu, float *__restrict__ out,
                                            const int *__restrict__ out_row) {
    const int last = n_out - 1;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        int orow[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int row = min(ig_cd_row(row0, h * 8 + j, ak), last);
            orow[j] = out_row ? out_row[row] : row;
        }
#pragma unroll
        for (int q = 0; q < NT; ++q) {
            const int col = q * 32 + ar;
            const int cc = min(col, Cout - 1);
            const float bv = bias ? bias[cc] : 0.f;
            float res[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) res[j] = 0.f;
            if (residual) {
#pragma unroll
                for (int j = 0; j < 8; ++j) res[j] = residual[(size_t)orow[j] * Cout + cc];
            }
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int r = h * 8 + j;
                if (ig_cd_row(row0, r, ak) < n_out && col < Cout) {
                    const float v = acc[q][r] + bv + res[j];
                    out[(size_t)orow[j] * Cout + col] = relu ? fmaxf(v, 0.f) : v;
                }
            }
        }
    }
}

// ---- the mask walk.  Mask-sorted tables (row_mask != NULL, K <= 32): rows arrive grouped by their neighbour-offset bit mask, so
// the 32 rows of a wave tile (and the 128 of the workgroup) mostly share one mask: offsets no row of the WORKGROUP uses are skipped
// outright (no W staging, no barriers) and a wave's MFMAs run only for offsets its own rows use.  The helpers take the mask to
// walk: the workgroup's (pipe, register-A, two-row-tile, packed), the wave's (wave-private) or a row tile's (two-row-tile use test).
__device__ __forceinline__ unsigned ig_tile_mask(const int *__restrict__ row_mask, int myrow, int trow, int n_out) {
    unsigned m = (myrow < n_out) ? (unsigned)row_mask[trow] : 0u;          // OR over the wave's rows
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) m |= (unsigned)__shfl_xor((int)m, d, 64);
    return m;
}

__device__ __forceinline__ unsigned ig_wg_mask(unsigned (&s_wmask)[4], unsigned m, int l, int wv) {
    if (l == 0) s_wmask[wv] = m;
    __syncthreads();
    return s_wmask[0] | s_wmask[1] | s_wmask[2] | s_wmask[3];
}

// next offset > k some row behind `mask` uses (K when none); unsorted tables visit every offset
__device__ __forceinline__ int ig_next_k(unsigned mask, int k, int K, bool sorted) {
    if (!sorted) return k + 1;
    const unsigned rest = (k + 1 < 32) ? (mask >> (k + 1)) : 0u;
    return rest ? k + 1 + __builtin_ctz(rest) : K;
}

// does a tile use offset k: its mask bit, or (unsorted) any lane with a neighbour
__device__ __forceinline__ bool ig_uses(unsigned mask, int k, int src, bool sorted) {
    return sorted ? ((mask >> k) & 1u) != 0u : __ballot(src >= 0) != 0ull;
}

// table entry of lane-row myrow (table row trow: the permutation entry for mask-sorted execution) at offset k, -1 past the ends.
// Entries are requested one offset ahead of the gathers that use them (two ahead of the MFMAs), so no wave waits for a table
// load with nothing else in flight.
__device__ __forceinline__ int ig_load_src(const int *__restrict__ nbr, int myrow, int trow, int n_out, int k, int K) {
    return (myrow < n_out && k < K) ? nbr[(size_t)trow * K + k] : -1;
}

// ---- W staging through registers: the float4 pieces of the Cin x Cout slice that starts at weight row wrow, zero padded to CW
// columns, distributed over STRIDE threads (256: a workgroup, 64: a wave; t = the thread's index among them).
template <int Cin, int CW, int STRIDE>
__device__ __forceinline__ void ig_fetch_w(float4 (&wr)[(Cin * (CW / 4) + STRIDE - 1) / STRIDE], const float *__restrict__ Wt, size_t wrow,
                                           int Cout, int t) {
    constexpr int CW4 = CW / 4, NW = (Cin * CW4 + STRIDE - 1) / STRIDE;
    const int Co4 = Cout >> 2;
#pragma unroll
    for (int q = 0; q < NW; ++q) {
        const int e = q * STRIDE + t, ci = e / CW4, q4 = e - ci * CW4;
        wr[q] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (e < Cin * CW4 && q4 < Co4) wr[q] = reinterpret_cast<const float4 *>(Wt + (wrow + ci) * Cout)[q4];
    }
}

template <int Cin, int CW, int STRIDE>
__device__ __forceinline__ void ig_store_w(float *s_w, const float4 (&wr)[(Cin * (CW / 4) + STRIDE - 1) / STRIDE], int t) {
    constexpr int CW4 = CW / 4, NW = (Cin * CW4 + STRIDE - 1) / STRIDE;
    float4 *dst = reinterpret_cast<float4 *>(s_w);
#pragma unroll
    for (int q = 0; q < NW; ++q) {
        const int e = q * STRIDE + t;
        if (e < Cin * CW4) dst[e] = wr[q];
    }
}

// ---- register-A gather.  The MFMA's A operand wants lane (row r = lane & 31, half ak = lane >> 5) to supply channel (step, ak) of
// row r.  Any fixed assignment of channels to (step, half) gives the same products summed in a fixed order, so half ak of row r
// simply OWNS the 16-byte pieces ak, ak + 2, ak + 4, ... of the row's stage (channels [ch0, ch0 + 8 NG)).  (r03 gave it the
// contiguous half [ak * Cin/2, (ak + 1) * Cin/2): one gather instruction then touched every 64-byte sector of a row with a single
// 16-byte piece and each sector was requested by four different instructions; interleaved, the two halves of a row read
// neighbouring pieces in the same instruction and a sector is requested twice.)
// (The register-A kernel, which honours SC_PROBE, keeps its own gather and staging lambdas: DESIGN §3.33.)
template <int NG>
__device__ __forceinline__ void ig_fetch_a(float4 (&g)[NG], const float *__restrict__ in, int CinT, int ch0, int src, int ak, bool any) {
    const float4 *rowp = reinterpret_cast<const float4 *>(in + (size_t)max(src, 0) * CinT + ch0) + ak;
#pragma unroll
    for (int u = 0; u < NG; ++u) {
        g[u] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (any && src >= 0) g[u] = rowp[2 * u];
    }
}

// one stage of MFMAs on the gathered pieces: B is read one float per step from the stage's W in LDS, Wb = W + 4 ak CW + ar
template <int NT, int NG>
__device__ __forceinline__ void ig_mma_stage(f32x16 (&acc)[NT], const float4 (&ga)[NG], const float *Wb) {
    constexpr int CW = NT * 32;
#pragma unroll
    for (int u = 0; u < NG; ++u) {
        const float av[4] = {ga[u].x, ga[u].y, ga[u].z, ga[u].w};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
#pragma unroll
            for (int q = 0; q < NT; ++q)
                acc[q] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[j], Wb[(u * 8 + j) * CW + q * 32], acc[q], 0, 0, 0);
        }
    }
}
