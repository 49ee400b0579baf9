// Shared host/device helpers for the gfx950 kernels.  wave = 64 lanes everywhere.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include "../../include/lidar_hip.h"   // the ABI: every LIDAR_EXPORT definition is compiled against its declaration; LIDAR_* codes, limits

#define LIDAR_EXPORT extern "C" __attribute__((visibility("default")))

static inline int lidar_check_launch(const char *what) {
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        fprintf(stderr, "[lidar_hip] %s: %s\n", what, hipGetErrorString(e));
        return LIDAR_ERR_LAUNCH;
    }
    return LIDAR_OK;
}

static inline int divup(long long a, long long b) { return (int)((a + b - 1) / b); }
static inline size_t align_up(size_t x, size_t a) { return (x + a - 1) / a * a; }

// Carves a workspace into 256-byte aligned pieces.  base == nullptr only measures: take() returns nullptr; off is the size so far.
struct WsCarve {
    char *base;
    size_t off = 0;
    char *take(size_t bytes) {
        const size_t o = off;
        off = align_up(off + bytes, 256);
        return base ? base + o : nullptr;
    }
};

// ---------------------------------------------------------------- device helpers
__device__ __forceinline__ int lane_id() { return (int)(threadIdx.x & 63); }

__device__ __forceinline__ unsigned long long lanemask_lt() {
    return (1ull << lane_id()) - 1ull;
}

// inclusive wave scan (sum) of an int over 64 lanes
__device__ __forceinline__ int wave_incl_scan(int v) {
    const int l = lane_id();
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        int t = __shfl_up(v, d, 64);
        if (l >= d) v += t;
    }
    return v;
}

// wave sum by an xor butterfly, 32 -> 1: every lane ends with the same value, and the order of the additions is fixed
__device__ __forceinline__ int wave_sum(int v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}

// The ordered sum of a workgroup of WAVES waves (no float atomics: two runs are bit-equal): each of a thread's NF floats and NI ints
// goes through wave_sum, lane 0 of every wave stores into the caller's LDS record, and after a barrier thread 0 adds waves 1, 2, ...
// in index order onto its own wave's sums.  The totals are left with thread 0 only.  Thread 0 starts from wave 0's sum, not from
// 0.0f + it: the two differ only for a wave sum of -0.0f, which this start keeps as the exact sum of its terms.  A thread value
// that was itself accumulated from 0.0f is never -0.0f (x + y is -0.0f only when both are), and then neither is any wave sum.
template <int WAVES, int NF, int NI>
struct BlockSumLds {
    float f[WAVES][NF];
    int i[WAVES][NI];
};

template <int WAVES, int NF, int NI>
__device__ __forceinline__ void block_sum(float (&f)[NF], int (&i)[NI], BlockSumLds<WAVES, NF, NI> &s) {
    const int wave = (int)(threadIdx.x >> 6);
#pragma unroll
    for (int q = 0; q < NF; ++q) f[q] = wave_sum(f[q]);
#pragma unroll
    for (int q = 0; q < NI; ++q) i[q] = wave_sum(i[q]);
    if (lane_id() == 0) {
#pragma unroll
        for (int q = 0; q < NF; ++q) s.f[wave][q] = f[q];
#pragma unroll
        for (int q = 0; q < NI; ++q) s.i[wave][q] = i[q];
    }
    __syncthreads();
    if (threadIdx.x == 0)
        for (int k = 1; k < WAVES; ++k) {
#pragma unroll
            for (int q = 0; q < NF; ++q) f[q] += s.f[k][q];
#pragma unroll
            for (int q = 0; q < NI; ++q) i[q] += s.i[k][q];
        }
}
