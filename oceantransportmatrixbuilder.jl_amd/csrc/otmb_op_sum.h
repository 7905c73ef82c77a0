// otmb_op_sum.h -- the ONE reduction tree of the operator's iterative layers (the solver, otmb_solve.hip; the periodic state,
// otmb_periodic.hip).  The determinism contract of include/otmb.h rests on every sum of a workgroup taking this order:
//     a wave of 64 lanes: xor shuffles at distances 32, 16, 8, 4, 2, 1 (every lane ends with the wave's sum);
//     a workgroup of 256 lanes: the four waves' sums added in wave order, ((w0 + w1) + w2) + w3; thread 0 holds the sums;
//     red: 4 * NV doubles of LDS, NV the number of values a lane brings.
// Device code only; force-inlined, so a kernel's machine code does not depend on which file states the tree.
#pragma once
#include "otmb_common.h"

__device__ __forceinline__ double op_wave_sum(double x) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) x = x + __shfl_xor(x, d);
    return x;
}
// 256 threads, NV values each: thread 0 gets the sums (waves in order).  red: 4 * NV doubles of LDS.
template <int NV>
__device__ __forceinline__ void op_block_sum(double (&x)[NV], double *red) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
    for (int q = 0; q < NV; ++q) {
        const double s = op_wave_sum(x[q]);
        if (lane == 0) red[w * NV + q] = s;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int q = 0; q < NV; ++q) x[q] = ((red[q] + red[NV + q]) + red[2 * NV + q]) + red[3 * NV + q];
    }
}
// a workgroup's sums q[0..NV) to its place in the partials: quantity j of the launch at part[j * np + workgroup]
template <int NV>
__device__ __forceinline__ void op_put(double *__restrict__ part, i64 np, const double (&q)[NV]) {
#pragma unroll
    for (int j = 0; j < NV; ++j) part[(i64)j * np + blockIdx.x] = q[j];
}
