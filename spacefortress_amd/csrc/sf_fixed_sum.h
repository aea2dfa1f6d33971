// sf_fixed_sum.h -- the float64 sum in a FIXED order that sf_ppo_loss (sfmi_ppo.h) and sf_advantages (sfmi_minibatch.h) document:
// a fixed shuffle tree within the wave (lane l takes lane l ^ 32, then ^ 16, ... ^ 1), the four waves of a 256-lane block in
// index order, the blocks in index order.  No float atomic anywhere: equal inputs give equal bits.
//
//   sf_wave_tree_sum        the tree; every lane ends with the wave's sum.  No lane may have left in front of it.
//   sf_block_partials<NV>   NV sums at once: the tree, the waves through LDS, lanes 0 .. NV-1 store the block's NV partial
//                           sums at partials[block * NV + j].  Holds a barrier: every lane of the block calls it.
//   sf_blocks_in_order<NV>  the blocks' partials added up in index order, staged through LDS SF_SUM_CHUNK blocks at a time;
//                           lanes 0 .. NV-1 return the NV totals (the other lanes 0).  Holds barriers, as above.
#pragma once
#include <hip/hip_runtime.h>

#define SF_SUM_BLOCK 256
#define SF_SUM_CHUNK 1024

__device__ __forceinline__ double sf_wave_tree_sum(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = v + __shfl_xor(v, off);
  return v;
}

// part: __shared__ double [4][NV]
template <int NV>
__device__ __forceinline__ void sf_block_partials(double (&v)[NV], double (*part)[NV], double* __restrict__ partials) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {  // (NV trees side by side: the shuffles of one hide under the adds of the others)
#pragma unroll
    for (int j = 0; j < NV; j++) v[j] = v[j] + __shfl_xor(v[j], off);
  }
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int j = 0; j < NV; j++) part[wave][j] = v[j];
  }
  __syncthreads();
  if (threadIdx.x < NV) {
    const int j = threadIdx.x;
    double t = part[0][j];
    t = t + part[1][j];
    t = t + part[2][j];
    t = t + part[3][j];
    partials[(size_t)blockIdx.x * NV + j] = t;
  }
}

// buf: __shared__ double [SF_SUM_CHUNK * NV]
template <int NV>
__device__ __forceinline__ double sf_blocks_in_order(const double* __restrict__ partials, int nblocks, double* buf) {
  const int tid = threadIdx.x;
  double acc = 0.0;
  for (int base = 0; base < nblocks; base += SF_SUM_CHUNK) {
    const int blocks = nblocks - base < SF_SUM_CHUNK ? nblocks - base : SF_SUM_CHUNK;
    for (int j = tid; j < blocks * NV; j += SF_SUM_BLOCK) buf[j] = partials[(size_t)base * NV + j];
    __syncthreads();
    if (tid < NV)
      for (int b = 0; b < blocks; b++) acc = acc + buf[b * NV + tid];  // the blocks in index order
    __syncthreads();
  }
  return acc;
}
