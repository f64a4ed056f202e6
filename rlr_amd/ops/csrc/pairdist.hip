// Pairwise squared L2 distances between the rows of the stacked (K, n) fp64
// update matrix, D[i][j] = ||U_i - U_j||^2 — what Krum / Multi-Krum
// (Blanchard et al., 2017) scores agents by.
//
// Gram form on the fp64 matrix cores: G = U U^T on upper-triangle tiles,
// then D[i][j] = (G_ii + G_jj) - 2 G_ij, clamped at 0, mirrored, with the
// diagonal written as 0.
//
// Stage 1 (pairdist_partial_k): a block owns (tile pair, chunk of columns).
// A tile is kPdTile = 64 rows of U; the tile pairs (ti <= tj) cover the
// upper triangle of G.  The block walks its chunk kPdKC = 32 columns at a
// time: 256 threads stage the two 64 x 32 slabs through LDS (a half-wave
// reads 256 contiguous bytes of one row of U, so global reads stay
// coalesced along n; rows of U are only 8-byte aligned for odd n, hence
// 8-byte loads) with the next slab prefetched into registers behind the
// MFMAs.  Rows >= K and columns past the chunk are staged as zeros, which
// add nothing to G: that is the whole tail path.
// LDS rows are padded to kPdStride = 34 doubles: the 32 lanes of a half-wave
// read rows 0..15 x k in {0,1}, i.e. banks 4*row + {0..3} — all 64 banks
// once (cdna_hip_programming.md §2 'Bank structure').
// Each of the 4 waves owns a 32 x 32 quarter = 2 x 2 tiles of
// v_mfma_f64_16x16x4_f64.  Operands: lane l holds A[row l&15][k l>>4] and
// B[k l>>4][col l&15]; here B = (the other tile)^T, so both come from LDS as
// slab[l&15][l>>4].  The f64 C/D map is col = lane&15,
// row = (lane>>4) + 4*reg — NOT the f32 one (cdna_hip_programming.md §3).
// MFMA tiles whose rows or columns lie wholly at or past K, and tiles below
// the diagonal of a diagonal pair, are skipped (wave-uniform).
// The block writes the needed MFMA tiles of its 64 x 64 partial to
// ws[chunk][pair][64][64]; the rest of a slab is never written nor read.
//
// K <= kPdSmallK = 16 (pairdist_partial16_k): U is ONE MFMA tile tall, so a
// 64-row slab would be mostly zeros and would keep too few bytes in flight
// to cover HBM latency.  The slab is 16 rows x 128 columns instead (up to
// 8 loads in flight per thread), A = B = the one fragment, and the 4 waves
// split the slab's 128 columns; their accumulators meet in LDS and are
// added in wave order, so the block writes one 16 x 16 partial.
//
// Stage 2 (pairdist_reduce_k) sums the partials of every needed element of
// G in a fixed order — no atomics, so the result is a pure function of
// (U, K, n): the chunks are cut into kPdSegs = 16 contiguous segments, one
// thread adds a segment sequentially in chunk order, and the 16 segment
// sums are added in segment order.  (One thread walking all chunks of an
// element is a chain of ~1000 dependent-latency loads when a single tile
// pair is split 1000 ways: measured 2.7 ms at K = 40 against 0.1 ms.)
// Stage 3 (pairdist_finish_k): one block per tile pair forms
// (G_ii + G_jj) - 2 G_ij and writes D[i][j] and D[j][i] from the one value.
// G lives in the workspace behind the partials.
//
// launch_gram_rows is stages 1 and 2 over the rows rows[0..K) of a taller
// matrix H (FoolsGold's per-agent history) and a finish that writes G itself,
// mirrored from the one reduced value (pairdist_gram_finish_k): the partial
// kernels are templated on the row map, so the distance path compiles
// without it.  A pure function of (H, rows).
//
// The chunking depends on (K, n) only: pairdist_chunks().  chunks * pairs
// <= kPdTargetBlocks = 1024 = four resident blocks per CU (128 VGPRs,
// 34 KiB LDS), all in flight at once and none left over for a ragged second
// round.  Workspace bound: at most 1024 + 36 slabs of 32 KiB < 34 MiB
// (<= 64 MiB) for every K <= 512 and every n.
#include "common.h"
#include "launchers.h"

constexpr int kPairdistMaxK = 512;    // = orderstat_max_k(): D feeds the sort
constexpr int kPdTile = 64;           // rows of U per tile
constexpr int kPdKC = 32;             // columns per LDS slab (256 B rows)
constexpr int kPdStride = kPdKC + 2;  // padded LDS row, doubles
constexpr int kPdSlab = kPdTile * kPdTile;   // doubles per partial
constexpr int kPdTargetBlocks = 1024; // four resident blocks per CU
constexpr long kPdMinChunk = 512;     // columns; amortises the partial write
constexpr int kPdSmallK = 16;         // one MFMA tile of rows: small kernel
constexpr int kPdSmallKC = 128;       // its columns per LDS slab
constexpr int kPdSmallStride = kPdSmallKC + 2;
constexpr int kPdSegs = 16;           // chunk segments of the reduction

typedef double pd_f64x4 __attribute__((ext_vector_type(4)));

static inline int pd_tiles(int K) { return (K + kPdTile - 1) / kPdTile; }
static inline int pd_pairs(int K) {
  int T = pd_tiles(K);
  return T * (T + 1) / 2;
}
// rows (= columns) of one partial slab
static inline int pd_slab_side(int K) {
  return K <= kPdSmallK ? kPdSmallK : kPdTile;
}
// columns per chunk: a multiple of the LDS slab depth
static inline long pd_chunk_len(int K, long n) {
  const int kc = K <= kPdSmallK ? kPdSmallKC : kPdKC;
  long want = kPdTargetBlocks / pd_pairs(K);
  long most = (n + kPdMinChunk - 1) / kPdMinChunk;
  if (want > most) want = most;
  if (want < 1) want = 1;
  long len = (n + want - 1) / want;
  return (len + kc - 1) / kc * kc;
}

// row-major index of tile pair (ti <= tj) in the upper triangle of T x T
__host__ __device__ inline int pd_pair_index(int ti, int tj, int T) {
  return ti * T - ti * (ti - 1) / 2 + (tj - ti);
}
__device__ inline void pd_pair_decode(int p, int T, int& ti, int& tj) {
  ti = 0;
  while (p >= T - ti) {
    p -= T - ti;
    ++ti;
  }
  tj = ti + p;
}

// kMap: row r of the operand is row rows[r] of U (launch_gram_rows); without
// it rows is unused and the kernel is the one launch_pairwise_sqdist always
// had.  The mapped row offsets of both tiles are staged in LDS once: a slab
// load reads them back as a broadcast.
template <bool kMap>
__global__ __launch_bounds__(256) void pairdist_partial_k(
    const double* __restrict__ U, const long* __restrict__ rows, int K,
    long n, int T, int pairs, long chunk_len, double* __restrict__ ws) {
  __shared__ double sA[kPdTile * kPdStride];
  __shared__ double sB[kPdTile * kPdStride];
  __shared__ long sRow[kMap ? 2 * kPdTile : 1];
  const int p = blockIdx.x % pairs;
  const long c = blockIdx.x / pairs;
  int ti, tj;
  pd_pair_decode(p, T, ti, tj);
  const bool diag = ti == tj;
  const long col0 = c * chunk_len;
  const long col1 = (col0 + chunk_len < n) ? col0 + chunk_len : n;

  const int tid = threadIdx.x;
  const int lc = tid & (kPdKC - 1);     // column of the slab
  const int lr = tid >> 5;              // first of 8 rows, step 8
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int wr = wave >> 1, wc = wave & 1;
  const int fr = lane & 15;             // operand row within the MFMA tile
  const int fk = lane >> 4;             // operand k within the MFMA step

  // MFMA tile (a, b) of this wave is needed when it holds a live (i <= j)
  bool need[2][2];
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b) {
      const int ra = wr * 2 + a, cb = wc * 2 + b;
      need[a][b] = ti * kPdTile + ra * 16 < K && tj * kPdTile + cb * 16 < K &&
                   !(diag && ra > cb);
    }

  if constexpr (kMap) {
    if (tid < 2 * kPdTile) {
      const int r = (tid < kPdTile ? ti : tj) * kPdTile + (tid & (kPdTile - 1));
      sRow[tid] = r < K ? rows[r] * n : 0;
    }
    __syncthreads();
  }

  double ga[8], gb[8];
  auto gload = [&](long cb) {
    const long col = cb + lc;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int row = lr + 8 * i;
      const int ia = ti * kPdTile + row, ib = tj * kPdTile + row;
      if constexpr (kMap) {
        ga[i] = (ia < K && col < col1) ? U[sRow[row] + col] : 0.0;
        gb[i] = (!diag && ib < K && col < col1)
                    ? U[sRow[kPdTile + row] + col] : 0.0;
      } else {
        ga[i] = (ia < K && col < col1) ? U[(long)ia * n + col] : 0.0;
        gb[i] = (!diag && ib < K && col < col1) ? U[(long)ib * n + col] : 0.0;
      }
    }
  };

  pd_f64x4 acc[2][2];
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b) acc[a][b] = pd_f64x4{0.0, 0.0, 0.0, 0.0};

  const double* sBp = diag ? sA : sB;
  gload(col0);
  // the trip count is uniform over the block: barriers inside
  for (long cb = col0; cb < col1; cb += kPdKC) {
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      sA[(lr + 8 * i) * kPdStride + lc] = ga[i];
      if (!diag) sB[(lr + 8 * i) * kPdStride + lc] = gb[i];
    }
    __syncthreads();
    if (cb + kPdKC < col1) gload(cb + kPdKC);
#pragma unroll
    for (int ks = 0; ks < kPdKC / 4; ++ks) {
      const int k = ks * 4 + fk;
      double fa[2], fb[2];
#pragma unroll
      for (int a = 0; a < 2; ++a) {
        fa[a] = sA[(wr * 32 + a * 16 + fr) * kPdStride + k];
        fb[a] = sBp[(wc * 32 + a * 16 + fr) * kPdStride + k];
      }
#pragma unroll
      for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b)
          if (need[a][b])
            acc[a][b] = __builtin_amdgcn_mfma_f64_16x16x4f64(
                fa[a], fb[b], acc[a][b], 0, 0, 0);
    }
    __syncthreads();   // slabs are overwritten by the next iteration
  }

  // f64 C/D map: col = lane & 15, row = (lane >> 4) + 4 * reg
  double* out = ws + (c * pairs + p) * (long)kPdSlab;
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b) {
      if (!need[a][b]) continue;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = wr * 32 + a * 16 + fk + 4 * r;
        const int col = wc * 32 + b * 16 + fr;
        out[row * kPdTile + col] = acc[a][b][r];
      }
    }
}

// K <= 16: one 16-row tile, chunk c -> ws[c][16][16]
template <bool kMap>
__global__ __launch_bounds__(256) void pairdist_partial16_k(
    const double* __restrict__ U, const long* __restrict__ rows, int K,
    long n, long chunk_len, double* __restrict__ ws) {
  __shared__ double sA[kPdSmallK * kPdSmallStride];
  __shared__ double red[4 * kPdSmallK * kPdSmallK];
  const long c = blockIdx.x;
  const long col0 = c * chunk_len;
  const long col1 = (col0 + chunk_len < n) ? col0 + chunk_len : n;

  const int tid = threadIdx.x;
  const int lc = tid & (kPdSmallKC - 1);  // column of the slab
  const int lr = tid >> 7;                // first of 8 rows, step 2
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int fr = lane & 15;
  const int fk = lane >> 4;

  // kMap: the 8 rows this thread loads, as offsets into U
  long off[8];
  if constexpr (kMap) {
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int row = lr + 2 * i;
      off[i] = row < K ? rows[row] * n : 0;
    }
  }

  double ga[8];
  auto gload = [&](long cb) {
    const long col = cb + lc;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int row = lr + 2 * i;
      if constexpr (kMap)
        ga[i] = (row < K && col < col1) ? U[off[i] + col] : 0.0;
      else
        ga[i] = (row < K && col < col1) ? U[(long)row * n + col] : 0.0;
    }
  };

  // two accumulators: consecutive MFMAs do not wait on each other
  pd_f64x4 acc0 = {0.0, 0.0, 0.0, 0.0}, acc1 = {0.0, 0.0, 0.0, 0.0};
  gload(col0);
  for (long cb = col0; cb < col1; cb += kPdSmallKC) {
#pragma unroll
    for (int i = 0; i < 8; ++i)
      sA[(lr + 2 * i) * kPdSmallStride + lc] = ga[i];
    __syncthreads();
    if (cb + kPdSmallKC < col1) gload(cb + kPdSmallKC);
    // this wave's quarter of the slab: columns [32 wave, 32 wave + 32)
#pragma unroll
    for (int ks = 0; ks < 8; ks += 2) {
      const double f0 = sA[fr * kPdSmallStride + wave * 32 + ks * 4 + fk];
      const double f1 = sA[fr * kPdSmallStride + wave * 32 + ks * 4 + 4 + fk];
      acc0 = __builtin_amdgcn_mfma_f64_16x16x4f64(f0, f0, acc0, 0, 0, 0);
      acc1 = __builtin_amdgcn_mfma_f64_16x16x4f64(f1, f1, acc1, 0, 0, 0);
    }
    __syncthreads();
  }

  // f64 C/D map: col = lane & 15, row = (lane >> 4) + 4 * reg
#pragma unroll
  for (int r = 0; r < 4; ++r)
    red[wave * 256 + (fk + 4 * r) * kPdSmallK + fr] = acc0[r] + acc1[r];
  __syncthreads();
  ws[c * 256 + tid] = ((red[tid] + red[256 + tid]) + red[512 + tid])
                      + red[768 + tid];
}

// side = rows of a slab: 64, or 16 from the small kernel (T = pairs = 1).
// Block = 16 consecutive elements of one slab row x kPdSegs segments.
__global__ __launch_bounds__(256) void pairdist_reduce_k(
    const double* __restrict__ ws, int K, int T, int pairs, int chunks,
    int side, double* __restrict__ G) {
  __shared__ double part[kPdSegs][16];
  const long slab = (long)side * side;
  const int groups = (int)(slab / 16);
  const int p = blockIdx.x / groups;
  const int x = threadIdx.x & 15, seg = threadIdx.x >> 4;
  const int e = (blockIdx.x % groups) * 16 + x;
  int ti, tj;
  pd_pair_decode(p, T, ti, tj);
  const int li = e / side, lj = e % side;
  // exactly the elements stage 1 wrote that stage 3 reads
  const bool live = ti * side + li < K && tj * side + lj < K &&
                    !(ti == tj && li > lj);
  const int per = (chunks + kPdSegs - 1) / kPdSegs;
  const int c0 = seg * per;
  const int c1 = c0 + per < chunks ? c0 + per : chunks;
  double g = 0.0;
  if (live) {
    const double* src = ws + (long)p * slab + e;
#pragma unroll 8
    for (int c = c0; c < c1; ++c) g += src[(long)c * pairs * slab];
  }
  part[seg][x] = g;
  __syncthreads();
  if (seg == 0 && live) {
    double t = part[0][x];
#pragma unroll
    for (int s = 1; s < kPdSegs; ++s) t += part[s][x];
    G[(long)p * slab + e] = t;
  }
}

// D from G: one block per tile pair, G one slab per pair
__global__ __launch_bounds__(256) void pairdist_finish_k(
    const double* __restrict__ G, int K, int T, int side,
    double* __restrict__ D) {
  __shared__ double gd[2 * kPdTile];    // G_ii of tile ti, G_jj of tile tj
  const int p = blockIdx.x;
  const long slab = (long)side * side;
  int ti, tj;
  pd_pair_decode(p, T, ti, tj);
  const int tid = threadIdx.x;
  if (tid < 2 * side) {
    const int t = tid < side ? ti : tj;
    const int l = tid % side;
    gd[tid] = t * side + l < K          // rows >= K are never written
                  ? G[(long)pd_pair_index(t, t, T) * slab + l * side + l]
                  : 0.0;
  }
  __syncthreads();
  for (int e = tid; e < (int)slab; e += 256) {
    const int li = e / side, lj = e % side;
    const int i = ti * side + li, j = tj * side + lj;
    if (i >= K || j >= K) continue;
    if (ti == tj && li >= lj) {
      if (li == lj) D[(long)i * K + i] = 0.0;
      continue;                         // (j, i) is written by its mirror
    }
    const double g = G[(long)p * slab + e];
    const double d = fmax((gd[li] + gd[side + lj]) - 2.0 * g, 0.0);
    D[(long)i * K + j] = d;
    D[(long)j * K + i] = d;
  }
}

// The Gram matrix itself from the reduced slabs: one block per tile pair
// writes Gm[i][j] and Gm[j][i] from the one reduced value, and the diagonal
// from the diagonal pair.
__global__ __launch_bounds__(256) void pairdist_gram_finish_k(
    const double* __restrict__ G, int K, int T, int side,
    double* __restrict__ Gm) {
  const int p = blockIdx.x;
  const long slab = (long)side * side;
  int ti, tj;
  pd_pair_decode(p, T, ti, tj);
  for (int e = threadIdx.x; e < (int)slab; e += 256) {
    const int li = e / side, lj = e % side;
    const int i = ti * side + li, j = tj * side + lj;
    if (i >= K || j >= K) continue;
    if (ti == tj && li > lj) continue;  // (i, j) is written by its mirror
    const double g = G[(long)p * slab + e];
    Gm[(long)i * K + j] = g;
    if (i != j) Gm[(long)j * K + i] = g;
  }
}

// stages 1 and 2; returns the reduced slabs, which live behind the partials
template <bool kMap>
static double* pd_gram_slabs(const double* U, const long* rows, int K, long n,
                             double* ws, hipStream_t st) {
  const int T = pd_tiles(K), pairs = pd_pairs(K);
  const int chunks = pairdist_chunks(K, n);
  if (K <= kPdSmallK)
    pairdist_partial16_k<kMap><<<chunks, 256, 0, st>>>(
        U, rows, K, n, pd_chunk_len(K, n), ws);
  else
    pairdist_partial_k<kMap><<<chunks * pairs, 256, 0, st>>>(
        U, rows, K, n, T, pairs, pd_chunk_len(K, n), ws);
  const int side = pd_slab_side(K);
  double* G = ws + (long)chunks * pairs * side * side;
  pairdist_reduce_k<<<pairs * (side * side / 16), 256, 0, st>>>(
      ws, K, T, pairs, chunks, side, G);
  return G;
}

extern "C" {
int pairdist_max_k() { return kPairdistMaxK; }

int pairdist_chunks(int K, long n) {
  long len = pd_chunk_len(K, n);
  return (int)((n + len - 1) / len);
}

long pairdist_ws_doubles(int K, long n) {
  const long side = pd_slab_side(K);
  // the partials, then G
  return ((long)pairdist_chunks(K, n) + 1) * pd_pairs(K) * side * side;
}

void launch_pairwise_sqdist(const double* U, int K, long n, double* ws,
                            double* D, void* s) {
  hipStream_t st = (hipStream_t)s;
  const double* G = pd_gram_slabs<false>(U, nullptr, K, n, ws, st);
  pairdist_finish_k<<<pd_pairs(K), 256, 0, st>>>(G, K, pd_tiles(K),
                                                 pd_slab_side(K), D);
}

void launch_gram_rows(const double* H, const long* rows, int K, long n,
                      double* ws, double* Gm, void* s) {
  hipStream_t st = (hipStream_t)s;
  const double* G = pd_gram_slabs<true>(H, rows, K, n, ws, st);
  pairdist_gram_finish_k<<<pd_pairs(K), 256, 0, st>>>(G, K, pd_tiles(K),
                                                      pd_slab_side(K), Gm);
}
}
