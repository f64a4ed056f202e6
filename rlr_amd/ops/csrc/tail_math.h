// Per-output arithmetic of the small "tail" kernels of a CNN step (pool,
// dropout, tiny GEMMs, cross entropy), factored out so that the unfused
// kernels (elementwise.hip, gemm_f32.hip) and the fused ones
// (fused_tail.hip) evaluate the SAME expressions in the SAME order: the
// fused paths are bitwise-equal to the sequences they replace by
// construction.  Every value that a kernel boundary used to round by a
// store is still a separately rounded float here: no function takes a
// product it could contract into a following add.
#pragma once
#include "common.h"

// ------------------------------------------------------------- maxpool 2x2
// strict '>' in the order 00, 01, 10, 11: the first maximum wins
__device__ __forceinline__ void pool2x2_select(float v00, float v01,
                                               float v10, float v11,
                                               float& m, uint8_t& a) {
  m = v00; a = 0;
  if (v01 > m) { m = v01; a = 1; }
  if (v10 > m) { m = v10; a = 2; }
  if (v11 > m) { m = v11; a = 3; }
}

// gradient of one input cell `a` of a window whose argmax is `am`
__device__ __forceinline__ float pool_bwd_pick(uint8_t am, uint8_t a,
                                               float dy) {
  return am == a ? dy : 0.f;
}
// upstream relu mask through the pooled value (window max of post-relu x)
__device__ __forceinline__ float relu_gate(float y, float g) {
  return y > 0.f ? g : 0.f;
}

// ---------------------------------------------------------------- dropout
__device__ __forceinline__ float dropout_scale(float p) {
  return 1.0f / (1.0f - p);
}
__device__ __forceinline__ bool dropout_keep(uint32_t r, float p) {
  return u32_to_uniform(r) >= p;
}
// keep flag of the flat element k: word k%4 of the draw for group k/4
__device__ __forceinline__ bool dropout_keep_at(uint64_t seed,
                                                uint64_t offset, long k,
                                                float p) {
  Philox4 r = philox4(seed, offset, (uint32_t)(k / 4));
  int j = (int)(k & 3);
  uint32_t v = j == 0 ? r.x : j == 1 ? r.y : j == 2 ? r.z : r.w;
  return dropout_keep(v, p);
}
__device__ __forceinline__ float dropout_apply(bool keep, float x,
                                               float scale) {
  return keep ? x * scale : 0.f;
}
// dropout backward fused with the relu mask of the layer below
__device__ __forceinline__ float dropout_relu_gate(float y, bool keep,
                                                   float dy, float scale) {
  return (y > 0.f && keep) ? dy * scale : 0.f;
}

// ------------------------------------------------------------- small dots
// thread form (gemm_small_k): K in order over 4 rotating fmaf accumulators
template <typename FA, typename FB>
__device__ __forceinline__ float dot_rot4(int K, FA a, FB b) {
  float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
  int k = 0;
  for (; k + 3 < K; k += 4) {
    a0 = fmaf(a(k + 0), b(k + 0), a0);
    a1 = fmaf(a(k + 1), b(k + 1), a1);
    a2 = fmaf(a(k + 2), b(k + 2), a2);
    a3 = fmaf(a(k + 3), b(k + 3), a3);
  }
  for (; k < K; ++k) a0 = fmaf(a(k), b(k), a0);
  return (a0 + a1) + (a2 + a3);
}

// wave form (gemm_small_wave_k): lane-strided K ...
template <typename FA, typename FB>
__device__ __forceinline__ float dot_wave_partial(int K, int lane, FA a,
                                                  FB b) {
  float acc = 0.f;
  for (int k = lane; k < K; k += kWave) acc = fmaf(a(k), b(k), acc);
  return acc;
}
// ... then a shuffle-down tree; lane 0 holds the sum
__device__ __forceinline__ float wave_tree_down(float acc) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off, kWave);
  return acc;
}

// the colsum role: lane-strided rows of column n, then the same tree
__device__ __forceinline__ float colsum_wave(const float* __restrict__ dY,
                                             int M, int N, int n, int lane) {
  float acc = 0.f;
  for (int m = lane; m < M; m += kWave) acc += dY[(long)m * N + n];
  return wave_tree_down(acc);
}

// ----------------------------------------------------------- cross entropy
// One wave per row, lane c holds logit c (C <= 64); v must be -3.4e38f on
// the lanes with in == false.
__device__ __forceinline__ void ce_row_softmax(float v, bool in, float& sm,
                                               float& m, float& sum) {
  m = v;
#pragma unroll
  for (int off = 32; off > 0; off >>= 1)
    m = fmaxf(m, __shfl_xor(m, off, kWave));
  float e = in ? __expf(v - m) : 0.f;
  sum = e;
#pragma unroll
  for (int off = 32; off > 0; off >>= 1)
    sum += __shfl_xor(sum, off, kWave);
  sm = e / sum;
}
__device__ __forceinline__ float ce_row_loss(float sum, float m, float lt) {
  return logf(sum) + m - lt;
}
// dlogit = dloss * (softmax - onehot) / B
__device__ __forceinline__ float ce_grad(float g, float sm, bool is_label,
                                         int B) {
  float v = sm - (is_label ? 1.f : 0.f);
  return g * v / B;
}
// ce_reduce_k: thread-strided sums, a kBlock-wide LDS tree, then / B.
// Whole block (blockDim.x == kBlock) must call; thread 0 gets the mean.
__device__ __forceinline__ float ce_mean_block(
    const float* __restrict__ row_loss, int B, float* sh) {
  float acc = 0.f;
  for (int i = threadIdx.x; i < B; i += blockDim.x) acc += row_loss[i];
  sh[threadIdx.x] = acc;
  __syncthreads();
  for (int off = kBlock / 2; off > 0; off >>= 1) {
    if (threadIdx.x < off) sh[threadIdx.x] += sh[threadIdx.x + off];
    __syncthreads();
  }
  return sh[0] / B;
}
