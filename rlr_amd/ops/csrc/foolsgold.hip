// FoolsGold (Fung, Yoon, Beschastnikh, "The Limitations of Federated
// Learning in Sybil Settings", RAID 2020): the two server kernels that are
// not the Gram matrix (pairdist.hip, launch_gram_rows).
//
// rows_add_k: the history update H[rows[k]][j] += U[k][j], one fp64 add per
// element, for K distinct rows of the (A, n) history.  A streaming kernel of
// rowclip.hip's shape: block b owns row b / chunks of U and the chunk
// b % chunks of its columns, thread t takes columns c0 + t, c0 + t + 256, ...
// with kFgUnroll loads of U and of H in flight (8-byte accesses: a row is
// only 8-byte aligned when n is odd).  The rows are distinct, so no element
// is touched twice: no atomics, and the result is index_add_'s bit for bit.
//
// The weights, steps 2-7 of the rule (PARITY.md), from the Gram matrix G of
// the sampled history rows, in three launches on the stream:
//   fg_cosine_k  block i: cs[i][j] = den > 0 ? G[i][j] / den : 0 with
//                den = sqrt(G[i][i] * G[j][j]), cs[i][i] = 0, and the row
//                maximum v[i] (the zero diagonal takes part) -> alpha[i]
//   fg_pardon_k  block i: over j != i, c = cs[i][j], and where v[i] < v[j]
//                c = (c * v[i]) / v[j]; wv[i] = clamp(1 - max(0, max_j c), 0, 1)
//                -> cs[i][i].  cs itself stays the matrix of step 2; block i
//                alone touches cs[i][i], and v is only read.
//   fg_alpha_k   one block: m = max_i wv[i]; wv /= m when m > 0; a weight of
//                exactly 1.0 becomes 0.99; alpha = clamp(kappa (ln(wv /
//                (1 - wv)) + 0.5), 0, 1), wv = 0 giving -inf and so 0; the
//                diagonal of cs goes back to 0.
// Every reduction is a maximum, so nothing depends on the thread order; no
// atomics, no host synchronisation, no workspace.
#include "common.h"
#include "launchers.h"

#include <math.h>

constexpr int kFoolsgoldMaxK = 512;   // = pairdist_max_k(): G comes from it
constexpr int kFgBlock = 256;
constexpr int kFgUnroll = 4;                    // loads of U and of H each
constexpr int kFgTile = kFgBlock * kFgUnroll;   // columns
constexpr int kFgBlocks = 4096;                 // as rowclip.hip's stage 1

static inline long fg_tiles(long n) { return (n + kFgTile - 1) / kFgTile; }
static inline long fg_tiles_per_chunk(int K, long n) {
  long tiles = fg_tiles(n);
  long want = (kFgBlocks + K - 1) / K;          // chunks per row, >= 1
  if (want > tiles) want = tiles;
  return (tiles + want - 1) / want;
}

__global__ __launch_bounds__(kFgBlock) void rows_add_k(
    double* __restrict__ H, const long* __restrict__ rows,
    const double* __restrict__ U, long n, int chunks, long cols_per_chunk) {
  const int tid = threadIdx.x;
  const int k = blockIdx.x / chunks;
  const int chunk = blockIdx.x % chunks;
  const long c0 = (long)chunk * cols_per_chunk;
  const long c1 = c0 + cols_per_chunk < n ? c0 + cols_per_chunk : n;
  const double* src = U + (long)k * n;
  double* dst = H + rows[k] * n;

  long j = c0 + tid;
  for (; j + (long)(kFgUnroll - 1) * kFgBlock < c1;
       j += (long)kFgUnroll * kFgBlock) {
    double u[kFgUnroll], h[kFgUnroll];
#pragma unroll
    for (int i = 0; i < kFgUnroll; ++i) {
      u[i] = src[j + (long)i * kFgBlock];
      h[i] = dst[j + (long)i * kFgBlock];
    }
#pragma unroll
    for (int i = 0; i < kFgUnroll; ++i)
      dst[j + (long)i * kFgBlock] = h[i] + u[i];
  }
  for (; j < c1; j += kFgBlock) dst[j] = dst[j] + src[j];
}

// maximum over the block of kFgBlock threads; every thread gets it
__device__ __forceinline__ double fg_block_max(double v, double* wave_max) {
  v = fmax(v, __shfl_xor(v, 32));
  v = fmax(v, __shfl_xor(v, 16));
  v = fmax(v, __shfl_xor(v, 8));
  v = fmax(v, __shfl_xor(v, 4));
  v = fmax(v, __shfl_xor(v, 2));
  v = fmax(v, __shfl_xor(v, 1));
  const int tid = threadIdx.x;
  if ((tid & (kWave - 1)) == 0) wave_max[tid / kWave] = v;
  __syncthreads();
  double m = wave_max[0];
#pragma unroll
  for (int w = 1; w < kFgBlock / kWave; ++w) m = fmax(m, wave_max[w]);
  return m;
}

__global__ __launch_bounds__(kFgBlock) void fg_cosine_k(
    const double* __restrict__ G, int K, double* __restrict__ cs,
    double* __restrict__ v) {
  __shared__ double wave_max[kFgBlock / kWave];
  const int i = blockIdx.x;
  const double gii = G[(long)i * K + i];
  double mx = 0.0;                      // the diagonal's 0
  for (int j = threadIdx.x; j < K; j += kFgBlock) {
    const double den = sqrt(gii * G[(long)j * K + j]);
    const double c = (j != i && den > 0.0) ? G[(long)i * K + j] / den : 0.0;
    cs[(long)i * K + j] = c;
    mx = fmax(mx, c);
  }
  mx = fg_block_max(mx, wave_max);
  if (threadIdx.x == 0) v[i] = mx;
}

// cs is read off the diagonal and written on it: no __restrict__
__global__ __launch_bounds__(kFgBlock) void fg_pardon_k(
    double* cs, const double* __restrict__ v, int K) {
  __shared__ double wave_max[kFgBlock / kWave];
  const int i = blockIdx.x;
  const double vi = v[i];
  double mx = 0.0;                      // the diagonal's 0
  for (int j = threadIdx.x; j < K; j += kFgBlock) {
    if (j == i) continue;
    double c = cs[(long)i * K + j];
    const double vj = v[j];
    if (vi < vj) c = (c * vi) / vj;
    mx = fmax(mx, c);
  }
  mx = fg_block_max(mx, wave_max);
  if (threadIdx.x == 0)
    cs[(long)i * K + i] = fmin(fmax(1.0 - mx, 0.0), 1.0);
}

__global__ __launch_bounds__(kFgBlock) void fg_alpha_k(
    double* __restrict__ cs, int K, double kappa,
    double* __restrict__ alpha) {
  __shared__ double wave_max[kFgBlock / kWave];
  double mx = 0.0;                      // wv >= 0
  for (int i = threadIdx.x; i < K; i += kFgBlock)
    mx = fmax(mx, cs[(long)i * K + i]);
  const double m = fg_block_max(mx, wave_max);
  for (int i = threadIdx.x; i < K; i += kFgBlock) {
    double wv = cs[(long)i * K + i];
    if (m > 0.0) wv = wv / m;
    if (wv == 1.0) wv = 0.99;
    const double a = kappa * (log(wv / (1.0 - wv)) + 0.5);
    alpha[i] = fmin(fmax(a, 0.0), 1.0);
    cs[(long)i * K + i] = 0.0;
  }
}

extern "C" {
int foolsgold_max_k() { return kFoolsgoldMaxK; }

void launch_rows_add(double* H, const long* rows, const double* U, int K,
                     long n, void* s) {
  const long per = fg_tiles_per_chunk(K, n);
  const int chunks = (int)((fg_tiles(n) + per - 1) / per);
  rows_add_k<<<(unsigned)((long)K * chunks), kFgBlock, 0, (hipStream_t)s>>>(
      H, rows, U, n, chunks, per * kFgTile);
}

void launch_foolsgold_weights(const double* G, int K, double kappa,
                              double* cs, double* alpha, void* s) {
  hipStream_t st = (hipStream_t)s;
  fg_cosine_k<<<K, kFgBlock, 0, st>>>(G, K, cs, alpha);
  fg_pardon_k<<<K, kFgBlock, 0, st>>>(cs, alpha, K);
  fg_alpha_k<<<1, kFgBlock, 0, st>>>(cs, K, kappa, alpha);
}
}
