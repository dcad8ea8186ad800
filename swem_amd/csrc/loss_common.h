// What the loss kernels of train.hip and lovasz.hip share.
#pragma once
#include "common.h"

namespace {

constexpr int LOSS_MAXC = 8;  // objects + background per clip (reference trains with MAX_NUM_OBJS = 2)

__device__ __forceinline__ double block_sum(double v, double *sh) {
  const int tid = threadIdx.x;
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o);
  __syncthreads();
  if ((tid & 63) == 0) sh[tid >> 6] = v;
  __syncthreads();
  double t = 0.0;
  if (tid == 0)
    for (int i = 0; i < (int)(blockDim.x >> 6); ++i) t += sh[i];
  return t;  // valid in thread 0
}

}  // namespace
