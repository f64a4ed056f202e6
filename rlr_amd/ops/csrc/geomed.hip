// Geometric median (RFA; Pillutla et al., "Robust Aggregation for Federated
// Learning") of the rows of the stacked (K, n) fp64 update matrix by
// smoothed Weiszfeld iterations:
//     s     = a[0] + a[1] + ... + a[K-1]          sequential in k
//     z_j   = (sum_k a[k] U[k][j]) * (1 / s)      sequential in k from 0
//     d2[k] = sum_j (U[k][j] - z_j)^2
//     a[k]  = 1 / max(nu, sqrt(d2[k]))
// The final weighted mean with w = a is the fused avg kernel
// (aggregation.hip); this file is the iteration's other half, the K
// distances to the current weighted mean — one streaming pass over U.
//
// Stage 1 (geomed_sqdist_k): a block owns one CHUNK of columns and walks it
// in tiles held resident in LDS as [k][cols], cols = 32 << lgCB a multiple
// of 32, so U is read from HBM once per iteration.  Thread t serves column
// t % 32 of a 32-column block: the 32 lanes of a half-wave always touch ONE
// 256 B run of one tile row = one full bank row, so every ds_read_b64 /
// ds_write_b64 lane group is conflict-free (cdna_hip_programming.md §2
// 'Bank structure'), and the same half-wave reads 256 contiguous bytes of a
// row of U (rows are only 8-byte aligned for odd n, hence 8-byte loads).
// Columns past n are staged as zeros: their z is 0 and they add (0 - 0)^2.
//   load   : half-wave g takes the 256 B runs g, g + G, ... of the tile (G
//            half-waves per block), at most kGmRuns = 16 per lane, into
//            registers; the NEXT tile's loads are issued as soon as this
//            tile sits in LDS and land behind phases A and B.
//   phase A: one lane per column forms z_j sequentially over k from the tile
//   phase B: half-wave g takes rows g, g + G, ... (at most 16); a lane adds
//            (u - z_j)^2 over its columns in ascending order into one
//            register per row, across ALL tiles of the chunk in ascending
//            order.
//   end    : per row the 32 lanes meet in a fixed xor tree (16, 8, 4, 2, 1)
//            and lane 0 writes the partial to ws[chunk][k].
// Every register array is indexed by unrolled loop counters only (§5.4:
// runtime-indexed local arrays spill); that is what bounds runs and rows per
// half-wave at 16 and so fixes the shapes:
//   K <= 128: 256 threads (G = 8), cols = the largest of {256, 128, 64, 32}
//             with K * cols / 32 <= 128 runs — a tile of at most 32 KiB, so
//             four or more blocks fit the 160 KiB LDS of a CU;
//   K >  128: 1024 threads (G = 32), cols = 32 — a tile of 33 .. 128 KiB;
//             two blocks per CU up to K = 309, one above.
// The chunking comes from (K, n) alone — geomed_chunks(): 512 chunks where
// two blocks fit a CU and 256 where one does, fewer when there are fewer
// tiles, every chunk a whole number of tiles.
//
// Stage 2 (geomed_reweight_k): ONE block.  The partials pass through LDS in
// slabs of whole chunks (a coalesced copy by all threads), then thread k
// adds its column of the slab sequentially, so d2[k] is the sum of its
// partials in ASCENDING chunk order.  It writes d2[k] and, in the loop,
// a[k]; thread 0 then forms 1 / s for the next iteration sequentially in k.
// No atomics anywhere: d2 and a are pure functions of (U, a, nu) — the same
// bits run to run and at every world size.
//
// The host loop enqueues iters x (stage 1, stage 2) on the stream; weights,
// distances and 1 / s stay on the device and nothing waits on the host.
#include "common.h"
#include "launchers.h"

constexpr int kGeomedMaxK = 512;          // = orderstat_max_k()
constexpr int kGmGroup = 32;              // lanes per row run (256 B)
constexpr int kGmRuns = 16;               // runs, and rows, per half-wave
constexpr int kGmSmallK = 128;            // up to here: 256 threads
constexpr int kGmSmallBlock = 256;
constexpr int kGmLargeBlock = 1024;
constexpr int kGmMaxLgCB = 3;             // at most 256 columns per tile
constexpr long kGmLdsBytes = 160 * 1024;
constexpr int kGmChunksTwo = 512;         // two or more blocks per CU
constexpr int kGmChunksOne = 256;         // one block per CU
constexpr int kGmReduceBlock = 512;
constexpr int kGmSlabDoubles = 8192;      // 64 KiB of partials per slab
constexpr int kGmWsTail = 8;              // 1 / s lives behind the partials

static_assert(kGeomedMaxK <= kGmLargeBlock / kGmGroup * kGmRuns,
              "rows per half-wave");

static inline int gm_threads(int K) {
  return K <= kGmSmallK ? kGmSmallBlock : kGmLargeBlock;
}
// log2 of the 32-column blocks per tile
static inline int gm_lg_cb(int K) {
  if (K > kGmSmallK) return 0;
  const int runs = kGmSmallBlock / kGmGroup * kGmRuns;
  int lg = 0;
  while (lg < kGmMaxLgCB && (K << (lg + 1)) <= runs) ++lg;
  return lg;
}
// tile [K][cols], z [cols], a [K]
static inline long gm_lds_bytes(int K) {
  long cols = kGmGroup << gm_lg_cb(K);
  return ((long)K * cols + cols + K) * 8;
}
static inline long gm_tiles(int K, long n) {
  long cols = kGmGroup << gm_lg_cb(K);
  return (n + cols - 1) / cols;
}
static inline long gm_tiles_per_chunk(int K, long n) {
  long tiles = gm_tiles(K, n);
  long want = 2 * gm_lds_bytes(K) <= kGmLdsBytes ? kGmChunksTwo : kGmChunksOne;
  if (want > tiles) want = tiles;
  return (tiles + want - 1) / want;
}

// 1 / (a[0] + a[1] + ... + a[K-1]), added sequentially: the ONE place the
// weight sum is formed, so the loop and a single step agree bit for bit.
__device__ inline double gm_inv_sum(const double* a, int K) {
  double s = 0.0;
  for (int k = 0; k < K; ++k) s += a[k];
  return 1.0 / s;
}

template <int LGCB, int THREADS>
__global__ __launch_bounds__(THREADS) void geomed_sqdist_k(
    const double* __restrict__ U, const double* __restrict__ a,
    const double* __restrict__ inv_s_p, int K, long n, long tiles,
    long tiles_per_chunk, double* __restrict__ ws) {
  constexpr int COLS = kGmGroup << LGCB;
  constexpr int CB = 1 << LGCB;                 // 32-column blocks per tile
  constexpr int G = THREADS / kGmGroup;         // half-waves per block
  constexpr int RSTEP = G / CB;                 // rows between a lane's runs
  static_assert(G % CB == 0, "a lane keeps its column block");
  extern __shared__ double smem[];
  double* tile = smem;                          // [K][COLS]
  double* z = tile + (long)K * COLS;            // [COLS]
  double* sa = z + COLS;                        // [K]
  const int tid = threadIdx.x;
  const int c = tid & (kGmGroup - 1);
  const int g = tid / kGmGroup;

  for (int k = tid; k < K; k += THREADS) sa[k] = a[k];
  const double inv_s = *inv_s_p;

  const long t0 = (long)blockIdx.x * tiles_per_chunk;
  const long t1 = t0 + tiles_per_chunk < tiles ? t0 + tiles_per_chunk : tiles;

  // half-wave g loads run g, g + G, ...: row (g >> LGCB) + RSTEP * i, always
  // column block g & (CB - 1).  Rows per lane <= kGmRuns.
  const int row0 = g >> LGCB;
  const int cofs = ((g & (CB - 1)) << 5) + c;   // column within the tile
  double* lds_run = tile + row0 * COLS + cofs;
  double r[kGmRuns];
  auto gload = [&](long t) {
    const long col = t * COLS + cofs;
    // the row stride is made opaque so that the 16 row addresses are formed
    // afresh per tile: kept across the tile loop they cost 32 registers
    long stride = (long)RSTEP * n;
    asm volatile("" : "+s"(stride));
    const double* src = U + (long)row0 * n + col;
#pragma unroll
    for (int i = 0; i < kGmRuns; ++i)
      r[i] = (row0 + RSTEP * i < K && col < n) ? src[i * stride] : 0.0;
  };

  double p[kGmRuns];                            // row g + G * i of d2
#pragma unroll
  for (int i = 0; i < kGmRuns; ++i) p[i] = 0.0;

  gload(t0);
  // the trip count is uniform over the block: barriers inside
  for (long t = t0; t < t1; ++t) {
#pragma unroll
    for (int i = 0; i < kGmRuns; ++i)
      if (row0 + RSTEP * i < K) lds_run[i * RSTEP * COLS] = r[i];
    __syncthreads();
    if (t + 1 < t1) gload(t + 1);

    // phase A: z_j, sequentially over k; the tile reads run ahead of the
    // chain of multiply-adds four at a time
    if (tid < COLS) {
      double s = 0.0;
      int k = 0;
      for (; k + 4 <= K; k += 4) {
        double u[4], w[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          u[i] = tile[(k + i) * COLS + tid];
          w[i] = sa[k + i];
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) s += w[i] * u[i];
      }
      for (; k < K; ++k) s += sa[k] * tile[k * COLS + tid];
      z[tid] = s * inv_s;
    }
    __syncthreads();

    // phase B: rows g, g + G, ... of this half-wave
#pragma unroll
    for (int b = 0; b < CB; ++b) {
      const double zb = z[b * kGmGroup + c];
#pragma unroll
      for (int i = 0; i < kGmRuns; ++i) {
        if (g + G * i < K) {
          const double d = tile[(g + G * i) * COLS + b * kGmGroup + c] - zb;
          p[i] += d * d;
        }
      }
    }
    __syncthreads();  // tile and z are overwritten by the next iteration
  }

#pragma unroll
  for (int i = 0; i < kGmRuns; ++i) {
    const int k = g + G * i;                    // uniform over the half-wave
    double v = p[i];
    v += __shfl_xor(v, 16);
    v += __shfl_xor(v, 8);
    v += __shfl_xor(v, 4);
    v += __shfl_xor(v, 2);
    v += __shfl_xor(v, 1);
    if (c == 0 && k < K) ws[(long)blockIdx.x * K + k] = v;
  }
}

// One block.  d2[k] = partials of k in ascending chunk order; a_out (when
// not null) = 1 / max(nu, sqrt(d2)) and *inv_s = 1 / sum a_out.
__global__ __launch_bounds__(kGmReduceBlock) void geomed_reweight_k(
    const double* __restrict__ ws, int chunks, int K, double nu,
    double* __restrict__ d2, double* __restrict__ a_out,
    double* __restrict__ inv_s) {
  __shared__ double slab[kGmSlabDoubles];
  const int tid = threadIdx.x;
  const int rows = kGmSlabDoubles / K;          // chunks per slab, >= 16
  double sum = 0.0;                             // K <= 512: one row per thread
  for (int c0 = 0; c0 < chunks; c0 += rows) {
    const int r1 = c0 + rows < chunks ? rows : chunks - c0;
    const int cnt = r1 * K;
    for (int i = tid; i < cnt; i += kGmReduceBlock)
      slab[i] = ws[(long)c0 * K + i];
    __syncthreads();
    if (tid < K)
      for (int r = 0; r < r1; ++r) sum += slab[r * K + tid];
    __syncthreads();
  }
  if (tid < K) {
    d2[tid] = sum;
    if (a_out) {
      const double w = 1.0 / fmax(nu, sqrt(sum));
      a_out[tid] = w;
      slab[tid] = w;
    }
  }
  __syncthreads();
  if (a_out && tid == 0) *inv_s = gm_inv_sum(slab, K);
}

// a = 1, d2 = 0, *inv_s = 1 / K (formed as the sequential sum of the ones)
__global__ __launch_bounds__(kGmReduceBlock) void geomed_init_k(
    int K, double* __restrict__ a, double* __restrict__ d2,
    double* __restrict__ inv_s) {
  __shared__ double ones[kGeomedMaxK];
  const int tid = threadIdx.x;
  if (tid < K) {
    a[tid] = 1.0;
    d2[tid] = 0.0;
    ones[tid] = 1.0;
  }
  __syncthreads();
  if (tid == 0) *inv_s = gm_inv_sum(ones, K);
}

// *inv_s = 1 / sum a for a caller-given weight vector
__global__ void geomed_invsum_k(const double* __restrict__ a, int K,
                                double* __restrict__ inv_s) {
  if (threadIdx.x == 0 && blockIdx.x == 0) *inv_s = gm_inv_sum(a, K);
}

template <int LGCB, int THREADS>
static void gm_sqdist_t(const double* U, const double* a,
                        const double* inv_s, int K, long n, double* ws,
                        hipStream_t st) {
  const size_t lds = (size_t)gm_lds_bytes(K);
  if (lds > 64 * 1024) {
    HIP_CHECK(hipFuncSetAttribute(
        (const void*)geomed_sqdist_k<LGCB, THREADS>,
        hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  }
  geomed_sqdist_k<LGCB, THREADS><<<geomed_chunks(K, n), THREADS, lds, st>>>(
      U, a, inv_s, K, n, gm_tiles(K, n), gm_tiles_per_chunk(K, n), ws);
}

static void gm_sqdist(const double* U, const double* a, const double* inv_s,
                      int K, long n, double* ws, hipStream_t st) {
  if (K > kGmSmallK) {
    gm_sqdist_t<0, kGmLargeBlock>(U, a, inv_s, K, n, ws, st);
    return;
  }
  switch (gm_lg_cb(K)) {
    case 0: gm_sqdist_t<0, kGmSmallBlock>(U, a, inv_s, K, n, ws, st); break;
    case 1: gm_sqdist_t<1, kGmSmallBlock>(U, a, inv_s, K, n, ws, st); break;
    case 2: gm_sqdist_t<2, kGmSmallBlock>(U, a, inv_s, K, n, ws, st); break;
    default: gm_sqdist_t<3, kGmSmallBlock>(U, a, inv_s, K, n, ws, st); break;
  }
}

extern "C" {
int geomed_max_k() { return kGeomedMaxK; }

int geomed_chunks(int K, long n) {
  long per = gm_tiles_per_chunk(K, n);
  return (int)((gm_tiles(K, n) + per - 1) / per);
}

long geomed_ws_doubles(int K, long n) {
  return (long)geomed_chunks(K, n) * K + kGmWsTail;
}

void launch_geomed_sqdist(const double* U, const double* a, int K, long n,
                          double* ws, double* d2, void* s) {
  hipStream_t st = (hipStream_t)s;
  const int chunks = geomed_chunks(K, n);
  double* inv_s = ws + (long)chunks * K;
  geomed_invsum_k<<<1, kWave, 0, st>>>(a, K, inv_s);
  gm_sqdist(U, a, inv_s, K, n, ws, st);
  geomed_reweight_k<<<1, kGmReduceBlock, 0, st>>>(ws, chunks, K, 0.0, d2,
                                                  nullptr, nullptr);
}

void launch_geomed_weights(const double* U, int K, long n, int iters,
                           double nu, double* ws, double* a, double* d2,
                           void* s) {
  hipStream_t st = (hipStream_t)s;
  const int chunks = geomed_chunks(K, n);
  double* inv_s = ws + (long)chunks * K;
  geomed_init_k<<<1, kGmReduceBlock, 0, st>>>(K, a, d2, inv_s);
  for (int r = 0; r < iters; ++r) {
    gm_sqdist(U, a, inv_s, K, n, ws, st);
    geomed_reweight_k<<<1, kGmReduceBlock, 0, st>>>(ws, chunks, K, nu, d2, a,
                                                    inv_s);
  }
}
}
