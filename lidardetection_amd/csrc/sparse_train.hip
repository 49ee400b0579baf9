// Training glue of the sparse half: the backward of HeightCompression in one pass.
//   reference: pcdet/models/backbones_2d/map_to_bev/height_compression.py:21-24 (spconv's .dense(), then the (N, C * D, H, W) view)
//
// lidar_sparse_to_bev_nhwc (pillar.hip) writes out[b][y][x][c * D + z] = features[row at (b, z, y, x)][c].  Its gradient is the same
// copy read the other way: d_features[row][c] = grad_out[b][y][x][c * D + z], a pure gather over the rows: no atomics, no workspace,
// every output element written exactly once.  A row whose coordinates scatter_index_kernel (pillar.hip) does not enter into the
// forward's map never reaches the BEV map, so its gradient is exactly zero; the test below is that kernel's, with nx = W,
// hrows = H and ny = D * H.
// One thread = one row's 4 consecutive channels: the pixel's 4 * D consecutive gradient floats (channel c * D + z is strided by D in
// the source) are read as D 16-byte loads and the 4 values at level z picked from them, the forward's register shuffle in reverse.
#include "common.h"

template <int D, bool VEC>
__global__ __launch_bounds__(256) void bev_nhwc_bwd_kernel(const float *__restrict__ g, long long g_ld, int g_off,
                                                           const int *__restrict__ idx, int n, int C4, int B, int H, int W,
                                                           float *__restrict__ df) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long long)n * C4) return;
    const int row = (int)(i / C4);
    const int c4 = (int)(i - (long long)row * C4);
    const int4 c = reinterpret_cast<const int4 *>(idx)[row];
    const int b = c.x, z = c.y, y = c.z, x = c.w;
    const long long cell = ((long long)z * H + y) * W + x;
    float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
    if (b >= 0 && b < B && x >= 0 && x < W && y >= 0 && y < H && cell >= 0 && cell < (long long)W * D * H) {
        // the cell test leaves 0 <= z < D: z * H + y < D * H with 0 <= y < H
        const float *src = g + (((long long)b * H + y) * W + x) * g_ld + g_off + (long long)c4 * (4 * D);
        float v[4 * D];
        if constexpr (VEC) {
#pragma unroll
            for (int d = 0; d < D; ++d) {
                const float4 t = reinterpret_cast<const float4 *>(src)[d];
                v[4 * d + 0] = t.x; v[4 * d + 1] = t.y; v[4 * d + 2] = t.z; v[4 * d + 3] = t.w;
            }
        } else {
#pragma unroll
            for (int k = 0; k < 4 * D; ++k) v[k] = src[k];
        }
        // v[k * D + z], k = 0..3, with constant register indices (a runtime index would send v to scratch)
#pragma unroll
        for (int d = 0; d < D; ++d)
            if (d == z) o = make_float4(v[0 * D + d], v[1 * D + d], v[2 * D + d], v[3 * D + d]);
    }
    reinterpret_cast<float4 *>(df)[(size_t)row * C4 + c4] = o;
}

LIDAR_EXPORT int lidar_sparse_to_bev_nhwc_backward(const float *grad_out, int g_ld, int g_off, const int *indices, int n, int channels,
                                                   int batch, int D, int H, int W, float *d_features, void *stream) {
    if (!grad_out || !indices || !d_features || batch <= 0 || D <= 0 || D > 4 || H <= 0 || W <= 0 || n < 0) return LIDAR_ERR_ARG;
    if (channels <= 0 || (channels & 3)) return LIDAR_ERR_ARG;
    if (g_off < 0 || (long long)g_off + (long long)channels * D > (long long)g_ld) return LIDAR_ERR_ARG;
    if (((uintptr_t)indices & 15) || ((uintptr_t)d_features & 15) || ((uintptr_t)grad_out & 3)) return LIDAR_ERR_ARG;
    if (n == 0) return LIDAR_OK;
    const int C4 = channels / 4;
    const long long blocks = ((long long)n * C4 + 255) / 256;
    if (blocks > 0x7fffffffll) return LIDAR_ERR_ARG;
    hipStream_t s = (hipStream_t)stream;
    // 16-byte loads when every pixel's slice starts on a 16-byte boundary
    const bool vec = (((uintptr_t)grad_out & 15) == 0) && g_ld % 4 == 0 && g_off % 4 == 0;
#define BWD_CASE(DD, VV)                                                                                                              \
    hipLaunchKernelGGL((bev_nhwc_bwd_kernel<DD, VV>), dim3((unsigned)blocks), dim3(256), 0, s, grad_out, (long long)g_ld, g_off,      \
                       indices, n, C4, batch, H, W, d_features)
    if (vec) {
        if (D == 1) BWD_CASE(1, true); else if (D == 2) BWD_CASE(2, true); else if (D == 3) BWD_CASE(3, true); else BWD_CASE(4, true);
    } else {
        if (D == 1) BWD_CASE(1, false); else if (D == 2) BWD_CASE(2, false); else if (D == 3) BWD_CASE(3, false); else BWD_CASE(4, false);
    }
#undef BWD_CASE
    return lidar_check_launch("lidar_sparse_to_bev_nhwc_backward");
}
