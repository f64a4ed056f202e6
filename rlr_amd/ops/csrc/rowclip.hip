// Server-side update-norm clipping (Sun et al., "Can You Really Backdoor
// Federated Learning?"; the clipping half of DP-FedAvg) of the rows of the
// stacked (K, n) fp64 update matrix, for any K >= 1:
//     sq[k]   = sum_j U[k][j]^2
//     norm[k] = sqrt(sq[k])
//     tau     = bound                                 (fixed mode)
//     tau     = mult * lower median of norm[0..K-1]   (median mode: the
//               ((K-1)/2)-th smallest, as agg_comed takes it)
//     s[k]    = norm[k] > tau ? tau / norm[k] : 1.0
//     U[k][j] = s[k] * U[k][j]                        in place
// Three stages on the stream, no host synchronisation, no atomics.
//
// Stage 1 (rownorm_partial_k): block b owns row b / chunks and the chunk
// b % chunks of its columns, so neighbouring blocks stream neighbouring
// memory.  Thread t takes columns c0 + t, c0 + t + 256, ... of the chunk and
// adds their squares into ONE register in ascending order; a wave reads 512
// contiguous bytes per load with 8-byte loads, since a row is only 8-byte
// aligned when n is odd, and kRcUnroll loads are in flight per thread to
// cover the HBM latency (8 B read per FMA: the kernel is bandwidth-bound).
// The 64 lanes of a wave meet in a fixed xor tree (32, 16, 8, 4, 2, 1), the
// four waves through LDS, added in wave order, and thread 0 writes
// ws[chunk][k].  No LDS tile of K rows, so no limit on K.
// The chunking comes from (K, n) alone - rownorm_chunks(): whole tiles of
// kRcTile columns, about kRcBlocks blocks over all rows (twice the eight
// blocks of 256 threads that each of the 256 CUs holds, so the last blocks
// to finish are half a round at most), fewer when there are fewer tiles.
//
// Stage 2 (rowclip_factors_k): ONE block.  Thread t takes rows t, t + 1024,
// ...; sq[k] is the sum of its partials in ASCENDING chunk order (the loads
// of neighbouring threads are contiguous).  In median mode the norms then
// pass through LDS in slabs and every row counts the rows that sort before
// it (smaller, or equal with a lower index): the row whose count is
// (K - 1) / 2 holds the median.  K^2 comparisons in one block: K is a few
// thousand at most, and this is not worth more.
//
// Stage 3 (rowscale_k): the blocks of stage 1; a block whose row has
// s[k] == 1.0 returns before it touches memory (uniform over the block), so
// an unclipped row costs no traffic and keeps its bits.
//
// norm, s and tau are pure functions of (U, bound or mult, mode): the same
// bits run to run and at every world size.
#include "common.h"
#include "launchers.h"

#include <math.h>

constexpr int kRcBlock = 256;
constexpr int kRcUnroll = 8;                    // loads in flight per thread
constexpr int kRcTile = kRcBlock * kRcUnroll;   // columns
constexpr int kRcBlocks = 4096;                 // 2 x (256 CUs x 8 blocks)
constexpr int kRcFactorBlock = 1024;
constexpr int kRcAhead = 16;                    // partial loads in flight
constexpr int kRcSlab = 4096;                   // norms per LDS slab, 32 KiB

static inline long rc_tiles(long n) { return (n + kRcTile - 1) / kRcTile; }
static inline long rc_tiles_per_chunk(int K, long n) {
  long tiles = rc_tiles(n);
  long want = (kRcBlocks + K - 1) / K;          // chunks per row, >= 1
  if (want > tiles) want = tiles;
  return (tiles + want - 1) / want;
}

__global__ __launch_bounds__(kRcBlock) void rownorm_partial_k(
    const double* __restrict__ U, int K, long n, int chunks,
    long cols_per_chunk, double* __restrict__ ws) {
  __shared__ double wave_sum[kRcBlock / kWave];
  const int tid = threadIdx.x;
  const int k = blockIdx.x / chunks;
  const int chunk = blockIdx.x % chunks;
  const long c0 = (long)chunk * cols_per_chunk;
  const long c1 = c0 + cols_per_chunk < n ? c0 + cols_per_chunk : n;
  const double* row = U + (long)k * n;

  double acc = 0.0;
  long j = c0 + tid;
  // whole tiles: kRcUnroll independent loads, then the adds in column order
  for (; j + (long)(kRcUnroll - 1) * kRcBlock < c1;
       j += (long)kRcUnroll * kRcBlock) {
    double u[kRcUnroll];
#pragma unroll
    for (int i = 0; i < kRcUnroll; ++i) u[i] = row[j + (long)i * kRcBlock];
#pragma unroll
    for (int i = 0; i < kRcUnroll; ++i) acc = fma(u[i], u[i], acc);
  }
  for (; j < c1; j += kRcBlock) {
    const double u = row[j];
    acc = fma(u, u, acc);
  }

  acc += __shfl_xor(acc, 32);
  acc += __shfl_xor(acc, 16);
  acc += __shfl_xor(acc, 8);
  acc += __shfl_xor(acc, 4);
  acc += __shfl_xor(acc, 2);
  acc += __shfl_xor(acc, 1);
  if ((tid & (kWave - 1)) == 0) wave_sum[tid / kWave] = acc;
  __syncthreads();
  if (tid == 0) {
    double v = wave_sum[0];
#pragma unroll
    for (int w = 1; w < kRcBlock / kWave; ++w) v += wave_sum[w];
    ws[(long)chunk * K + k] = v;
  }
}

// One block.  norm[k] = sqrt(partials of k in ascending chunk order); with
// scale not null also tau and s (file header).  norm is read back by the
// whole block after a barrier, hence no __restrict__ on it.
__global__ __launch_bounds__(kRcFactorBlock) void rowclip_factors_k(
    const double* __restrict__ ws, int chunks, int K, double value,
    int median_mode, double* norm, double* __restrict__ scale,
    double* __restrict__ tau_out) {
  __shared__ double slab[kRcSlab];
  __shared__ double med;
  const int tid = threadIdx.x;
  for (int k = tid; k < K; k += kRcFactorBlock) {
    // the loads run ahead of the chain of adds kRcAhead at a time: with few
    // rows this block is one wave waiting on each load in turn
    double sq = 0.0;
    int c = 0;
    for (; c + kRcAhead <= chunks; c += kRcAhead) {
      double p[kRcAhead];
#pragma unroll
      for (int i = 0; i < kRcAhead; ++i) p[i] = ws[(long)(c + i) * K + k];
#pragma unroll
      for (int i = 0; i < kRcAhead; ++i) sq += p[i];
    }
    for (; c < chunks; ++c) sq += ws[(long)c * K + k];
    norm[k] = sqrt(sq);
  }
  if (!scale) return;

  double tau = value;
  if (median_mode) {
    if (tid == 0) med = 0.0;
    __syncthreads();                    // norm[] and med are in place
    const int want = (K - 1) / 2;
    // the trip counts are uniform over the block: barriers inside
    for (int k0 = 0; k0 < K; k0 += kRcFactorBlock) {
      const int k = k0 + tid;
      const double mine = k < K ? norm[k] : 0.0;
      int before = 0;
      for (int j0 = 0; j0 < K; j0 += kRcSlab) {
        const int cnt = j0 + kRcSlab < K ? kRcSlab : K - j0;
        for (int i = tid; i < cnt; i += kRcFactorBlock)
          slab[i] = norm[j0 + i];
        __syncthreads();
        if (k < K) {
          for (int i = 0; i < cnt; ++i) {
            const double other = slab[i];
            before += (other < mine || (other == mine && j0 + i < k)) ? 1 : 0;
          }
        }
        __syncthreads();                // the slab is overwritten next
      }
      if (k < K && before == want) med = mine;   // exactly one row
    }
    __syncthreads();
    tau = value * med;
  }
  if (tid == 0) *tau_out = tau;
  for (int k = tid; k < K; k += kRcFactorBlock) {
    const double nk = norm[k];
    scale[k] = nk > tau ? tau / nk : 1.0;
  }
}

__global__ __launch_bounds__(kRcBlock) void rowscale_k(
    double* __restrict__ U, const double* __restrict__ scale, int K, long n,
    int chunks, long cols_per_chunk) {
  const int tid = threadIdx.x;
  const int k = blockIdx.x / chunks;
  const int chunk = blockIdx.x % chunks;
  const double s = scale[k];
  if (s == 1.0) return;                 // uniform over the block
  const long c0 = (long)chunk * cols_per_chunk;
  const long c1 = c0 + cols_per_chunk < n ? c0 + cols_per_chunk : n;
  double* row = U + (long)k * n;

  long j = c0 + tid;
  for (; j + (long)(kRcUnroll - 1) * kRcBlock < c1;
       j += (long)kRcUnroll * kRcBlock) {
    double u[kRcUnroll];
#pragma unroll
    for (int i = 0; i < kRcUnroll; ++i) u[i] = row[j + (long)i * kRcBlock];
#pragma unroll
    for (int i = 0; i < kRcUnroll; ++i) row[j + (long)i * kRcBlock] = s * u[i];
  }
  for (; j < c1; j += kRcBlock) row[j] = s * row[j];
}

static void rc_partials(const double* U, int K, long n, double* ws,
                        hipStream_t st) {
  const int chunks = rownorm_chunks(K, n);
  rownorm_partial_k<<<(unsigned)((long)K * chunks), kRcBlock, 0, st>>>(
      U, K, n, chunks, rc_tiles_per_chunk(K, n) * kRcTile, ws);
}

extern "C" {
int rownorm_chunks(int K, long n) {
  long per = rc_tiles_per_chunk(K, n);
  return (int)((rc_tiles(n) + per - 1) / per);
}

long rownorm_ws_doubles(int K, long n) {
  return (long)rownorm_chunks(K, n) * K;
}

void launch_rownorm_partials(const double* U, int K, long n, double* ws,
                             void* s) {
  rc_partials(U, K, n, ws, (hipStream_t)s);
}

void launch_row_norms(const double* U, int K, long n, double* ws,
                      double* norm, void* s) {
  hipStream_t st = (hipStream_t)s;
  rc_partials(U, K, n, ws, st);
  rowclip_factors_k<<<1, kRcFactorBlock, 0, st>>>(
      ws, rownorm_chunks(K, n), K, 0.0, 0, norm, nullptr, nullptr);
}

void launch_rowclip(double* U, int K, long n, double value, int median_mode,
                    double* ws, double* norm, double* scale, double* tau,
                    void* s) {
  hipStream_t st = (hipStream_t)s;
  const int chunks = rownorm_chunks(K, n);
  rc_partials(U, K, n, ws, st);
  rowclip_factors_k<<<1, kRcFactorBlock, 0, st>>>(ws, chunks, K, value,
                                                  median_mode, norm, scale,
                                                  tau);
  rowscale_k<<<(unsigned)((long)K * chunks), kRcBlock, 0, st>>>(
      U, scale, K, n, chunks, rc_tiles_per_chunk(K, n) * kRcTile);
}
}
