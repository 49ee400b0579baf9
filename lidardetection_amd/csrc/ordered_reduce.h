// The second step of every "fp64 partial sums per block, reduced in a fixed order" scheme of the train-mode kernels (bn_train_dev.h:
// the BatchNorm statistics; csrc/pfn_train.hip: PillarVFE's moments and gradient sums).  One definition, so every such sum is added
// in the same order: no float atomics, two runs are bit-equal.  The kernel is static: each including file owns its copy.
#pragma once
#include "common.h"

// rows of `part` ([entries][nparts]) -> tot[entry]; one block per entry, fixed summation order
static __global__ __launch_bounds__(256) void ordered_reduce_kernel(const double *__restrict__ part, int nparts, double *__restrict__ tot) {
    __shared__ double s[256];
    const double *row = part + (size_t)blockIdx.x * nparts;
    double a = 0.0;
    for (int b = threadIdx.x; b < nparts; b += 256) a += row[b];
    s[threadIdx.x] = a;
    __syncthreads();
    for (int h = 128; h > 0; h >>= 1) {
        if ((int)threadIdx.x < h) s[threadIdx.x] += s[threadIdx.x + h];
        __syncthreads();
    }
    if (threadIdx.x == 0) tot[blockIdx.x] = s[0];
}
