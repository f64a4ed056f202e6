// MFMA fp32 GEMM for gfx950 (SURVEY.md §2b K6 — Linear fwd/bwd; also the
// inner engine shape for the conv kernels).
//
// C[M,N] = A[M,K] x B[K,N], all row-major, exact fp32 numerics via
// v_mfma_f32_16x16x4_f32 (f32-in/f32-acc MFMA at the 157 TF f32 vector
// rate — cdna_hip_programming.md §3 "FP32-input MFMA"; there is no
// xf32/TF32 on gfx950 and this is bitwise an fmaf chain).
//
// Structure: 256-thread block = 4 waves (2x2), block tile BM=128 x BN=64,
// K-step BK=32, double-buffered LDS:
//   A_lds[2][BM][BK+2]  — +2 pad makes the b32 fragment read (lane groups
//                         {m0..m0+15} x k, bank = (2m+k) mod 32) conflict-
//                         free across the two 16-lane halves of a group
//   B_lds[2][BK][BN+16] — +16 pad shifts consecutive k rows by 16 banks
// Deterministic split-K for small-M*N / large-K shapes (fc1: M=256, N=128,
// K=9216 — 4 output tiles would leave 252 CUs idle): gridDim.z K-chunks
// write fp32 partial slabs, a fixed-order reduce kernel (fused bias+relu)
// combines them.  No atomics anywhere: bitwise run-to-run reproducible.
#include "common.h"
#include "launchers.h"
#include "tail_math.h"

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int BM = 128, BN = 64, BK = 32;
constexpr int LDA_S = BK + 2;   // A_lds row stride (floats)
constexpr int LDB_S = BN + 16;  // B_lds row stride (floats)

// Staging guards handle M/N/K edges by zero-fill; VEC selects float4 global
// loads (requires 16B-aligned rows: ld % 4 == 0).
// AT: A is stored transposed [K][M] (lda = its row length = M direction);
// BT: B is stored transposed [N][K] (e.g. a torch Linear weight (out,in)
// consumed directly — no separate transpose pass).
template <bool VEC, bool AT = false, bool BT = false>
__global__ __launch_bounds__(256)
void gemm_f32_k(const float* __restrict__ A, const float* __restrict__ B,
                float* __restrict__ C, const float* __restrict__ bias,
                int M, int N, int K, int lda, int ldb, int ldc,
                long k_per_chunk, int relu, int direct_out) {
  __shared__ float A_lds[2][BM * LDA_S];
  __shared__ float B_lds[2][BK * LDB_S];

  const int m_blk = blockIdx.x * BM;
  const int n_blk = blockIdx.y * BN;
  const long k_lo = (long)blockIdx.z * k_per_chunk;
  const long k_hi = min((long)K, k_lo + k_per_chunk);

  const int t = threadIdx.x;
  const int wave = t >> 6, lane = t & 63;
  const int wr = wave >> 1, wc = wave & 1;       // 2x2 wave grid
  const int l15 = lane & 15, l4 = lane >> 4;     // fragment coords

  f32x4 acc[4][2];
#pragma unroll
  for (int mi = 0; mi < 4; ++mi)
#pragma unroll
    for (int ni = 0; ni < 2; ++ni) acc[mi][ni] = {0.f, 0.f, 0.f, 0.f};

  // staging coordinates (per thread, fixed across k-tiles)
  const int am = t >> 3;            // 0..31 (+32 per round, 4 rounds)
  const int ak = (t & 7) * 4;       // 0,4,..,28
  const int bk = t >> 4;            // 0..15 (+16 per round, 2 rounds)
  const int bn = (t & 15) * 4;      // 0,4,..,60

  // async-STAGE split (guide T14/G15): global loads go to registers a
  // K-tile early; the LDS write lands after the barrier, under the MFMAs.
  // AT/BT staging loads along the transposed storage rows (still float4
  // coalesced) and scatter-writes the LDS image transposed.
  float4 ra[4], rb[2];
  // transposed-staging thread coordinates
  const int tak = t >> 3;           // AT: k index, 0..31
  const int tam = (t & 7) * 4;      // AT: m base, +32 per round (4 rounds)
  const int tbn = t >> 3;           // BT: n index base, +32 per round (2)
  const int tbk = (t & 7) * 4;      // BT: k base
  auto stage_load = [&](long k0) {
    if (AT) {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        long gk = k0 + tak;
        long gm = m_blk + tam + j * 32;
        float v0 = 0.f, v1 = 0.f, v2 = 0.f, v3 = 0.f;
        if (gk < k_hi) {
          long base = gk * (long)lda + gm;
          if (VEC && gm + 3 < M) {
            const float4 q = *(const float4*)(A + base);
            v0 = q.x; v1 = q.y; v2 = q.z; v3 = q.w;
          } else {
            if (gm + 0 < M) v0 = A[base + 0];
            if (gm + 1 < M) v1 = A[base + 1];
            if (gm + 2 < M) v2 = A[base + 2];
            if (gm + 3 < M) v3 = A[base + 3];
          }
        }
        ra[j] = {v0, v1, v2, v3};
      }
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        int m = am + j * 32;
        long gm = m_blk + m;
        float v0 = 0.f, v1 = 0.f, v2 = 0.f, v3 = 0.f;
        if (gm < M) {
          long base = gm * (long)lda + k0 + ak;
          if (VEC && k0 + ak + 3 < k_hi) {
            const float4 q = *(const float4*)(A + base);
            v0 = q.x; v1 = q.y; v2 = q.z; v3 = q.w;
          } else {
            if (k0 + ak + 0 < k_hi) v0 = A[base + 0];
            if (k0 + ak + 1 < k_hi) v1 = A[base + 1];
            if (k0 + ak + 2 < k_hi) v2 = A[base + 2];
            if (k0 + ak + 3 < k_hi) v3 = A[base + 3];
          }
        }
        ra[j] = {v0, v1, v2, v3};
      }
    }
    if (BT) {
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        long gn = n_blk + tbn + j * 32;
        long gk = k0 + tbk;
        float v0 = 0.f, v1 = 0.f, v2 = 0.f, v3 = 0.f;
        if (gn < N) {
          long base = gn * (long)ldb + gk;
          if (VEC && gk + 3 < k_hi) {
            const float4 q = *(const float4*)(B + base);
            v0 = q.x; v1 = q.y; v2 = q.z; v3 = q.w;
          } else {
            if (gk + 0 < k_hi) v0 = B[base + 0];
            if (gk + 1 < k_hi) v1 = B[base + 1];
            if (gk + 2 < k_hi) v2 = B[base + 2];
            if (gk + 3 < k_hi) v3 = B[base + 3];
          }
        }
        rb[j] = {v0, v1, v2, v3};
      }
    } else {
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        long gk = k0 + bk + j * 16;
        float v0 = 0.f, v1 = 0.f, v2 = 0.f, v3 = 0.f;
        if (gk < k_hi) {
          long base = gk * (long)ldb + n_blk + bn;
          if (VEC && n_blk + bn + 3 < N) {
            const float4 q = *(const float4*)(B + base);
            v0 = q.x; v1 = q.y; v2 = q.z; v3 = q.w;
          } else {
            if (n_blk + bn + 0 < N) v0 = B[base + 0];
            if (n_blk + bn + 1 < N) v1 = B[base + 1];
            if (n_blk + bn + 2 < N) v2 = B[base + 2];
            if (n_blk + bn + 3 < N) v3 = B[base + 3];
          }
        }
        rb[j] = {v0, v1, v2, v3};
      }
    }
  };
  auto stage_write = [&](int buf) {
    if (AT) {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float v[4] = {ra[j].x, ra[j].y, ra[j].z, ra[j].w};
#pragma unroll
        for (int e = 0; e < 4; ++e)
          A_lds[buf][(tam + j * 32 + e) * LDA_S + tak] = v[e];
      }
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        float* dst = &A_lds[buf][(am + j * 32) * LDA_S + ak];
        ((float2*)dst)[0] = {ra[j].x, ra[j].y};
        ((float2*)dst)[1] = {ra[j].z, ra[j].w};
      }
    }
    if (BT) {
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const float v[4] = {rb[j].x, rb[j].y, rb[j].z, rb[j].w};
#pragma unroll
        for (int e = 0; e < 4; ++e)
          B_lds[buf][(tbk + e) * LDB_S + tbn + j * 32] = v[e];
      }
    } else {
#pragma unroll
      for (int j = 0; j < 2; ++j)
        *(float4*)&B_lds[buf][(bk + j * 16) * LDB_S + bn] = rb[j];
    }
  };

  stage_load(k_lo);
  stage_write(0);
  if (k_lo + BK < k_hi) stage_load(k_lo + BK);
  __syncthreads();

  int buf = 0;
  for (long k0 = k_lo; k0 < k_hi; k0 += BK) {
    if (k0 + BK < k_hi) {
      stage_write(buf ^ 1);
      if (k0 + 2 * BK < k_hi) stage_load(k0 + 2 * BK);
    }
    const float* Abuf = A_lds[buf];
    const float* Bbuf = B_lds[buf];
#pragma unroll
    for (int kk = 0; kk < BK / 4; ++kk) {
      float a_frag[4], b_frag[2];
#pragma unroll
      for (int mi = 0; mi < 4; ++mi)
        a_frag[mi] = Abuf[(wr * 64 + mi * 16 + l15) * LDA_S + kk * 4 + l4];
#pragma unroll
      for (int ni = 0; ni < 2; ++ni)
        b_frag[ni] = Bbuf[(kk * 4 + l4) * LDB_S + wc * 32 + ni * 16 + l15];
#pragma unroll
      for (int mi = 0; mi < 4; ++mi)
#pragma unroll
        for (int ni = 0; ni < 2; ++ni)
          acc[mi][ni] = __builtin_amdgcn_mfma_f32_16x16x4f32(
              a_frag[mi], b_frag[ni], acc[mi][ni], 0, 0, 0);
    }
    __syncthreads();
    buf ^= 1;
  }

  // epilogue: C/D mapping col = lane&15, row = (lane>>4)*4 + reg
#pragma unroll
  for (int mi = 0; mi < 4; ++mi) {
#pragma unroll
    for (int ni = 0; ni < 2; ++ni) {
      int col = n_blk + wc * 32 + ni * 16 + l15;
      if (col >= N) continue;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        int row = m_blk + wr * 64 + mi * 16 + l4 * 4 + r;
        if (row >= M) continue;
        float v = acc[mi][ni][r];
        if (direct_out) {
          if (bias) v += bias[col];
          if (relu) v = fmaxf(v, 0.f);
          C[(long)row * ldc + col] = v;
        } else {
          // split-K partial slab: [z][M][N] dense
          C[((long)blockIdx.z * M + row) * N + col] = v;
        }
      }
    }
  }
}

// ---------------------------------------------------------------------------
// Short-K form: a chunk of at most T K-tiles (fc1: 4 or 5 per block).  The
// pipeline above keeps one K-tile in flight, which suits the conv-sized K
// loops; with 3..5 tiles it exposes nearly every memory latency and there is
// no second block on the CU to hide them.  Here every global load of the
// chunk is issued before the first LDS write, into a register ring of one
// float4 set per tile; the same double-buffered LDS ring then consumes the
// sets in order, and the compiler's counted s_waitcnt vmcnt(n) makes tile i
// wait for tile i's loads only.  Same tile, wave grid, LDS image, chunking
// and k order as gemm_f32_k, so C and every slab carry the same bits.
//
// For the counted waits to survive code generation the loads must be
// unconditional and the tile count a compile-time constant: a load under a
// branch merges to vmcnt(0) at the join.  So (a) the body is instantiated
// per tile count NT and the kernel picks one by the block-uniform count, and
// (b) an out-of-range float4 is loaded from the matrix base instead (always
// mapped) and zeroed by a select at LDS-write time.  Only a float4 that
// straddles the edge (ld % 4 == 0 but the extent is not) takes a branch,
// which re-loads it element-wise as gemm_f32_k does.
// ---------------------------------------------------------------------------
constexpr int kShortKMaxTiles = 5;

// One float4 slot: elements v0..v0+3 of row `row` of P, valid while
// row_ok && v < lim.  sk_load issues the load, sk_mask (at LDS-write time)
// zero-fills what the guards exclude.
__device__ __forceinline__ float4 sk_load(const float* __restrict__ P,
                                          long row, long ld, long v0,
                                          bool row_ok, long lim) {
  const bool full = row_ok && v0 + 3 < lim;
  float4 q = *(const float4*)(P + (full ? row * ld + v0 : 0));
  if (row_ok && !full && v0 < lim) {
    const float* r = P + row * ld + v0;
    q.x = r[0];
    q.y = v0 + 1 < lim ? r[1] : 0.f;
    q.z = v0 + 2 < lim ? r[2] : 0.f;
    q.w = 0.f;
  }
  return q;
}

__device__ __forceinline__ float4 sk_mask(float4 q, bool row_ok, long v0,
                                          long lim) {
  const bool keep = row_ok && v0 < lim;
  return {keep ? q.x : 0.f, keep ? q.y : 0.f, keep ? q.z : 0.f,
          keep ? q.w : 0.f};
}

// The chunk [k_lo, k_hi) of exactly NT K-tiles, accumulated into acc.
template <int NT, bool AT, bool BT>
__device__ __forceinline__ void shortk_chunk(
    const float* __restrict__ A, const float* __restrict__ B, int M, int N,
    int lda, int ldb, int m_blk, int n_blk, long k_lo, long k_hi,
    float (&A_lds)[2][BM * LDA_S], float (&B_lds)[2][BK * LDB_S],
    f32x4 (&acc)[4][2]) {
  const int t = threadIdx.x;
  const int wave = t >> 6, lane = t & 63;
  const int wr = wave >> 1, wc = wave & 1;
  const int l15 = lane & 15, l4 = lane >> 4;
  // staging coordinates of gemm_f32_k: A slot j is row a_r + 32 j (NN) or
  // m base a_v + 32 j (AT); B slot j is k row b_r + 16 j (NN) or n row
  // b_r + 32 j (BT)
  const int a_r = t >> 3, a_v = (t & 7) * 4;
  const int b_r = BT ? t >> 3 : t >> 4;
  const int b_v = BT ? (t & 7) * 4 : (t & 15) * 4;

  float4 ra[NT][4], rb[NT][2];
#pragma unroll
  for (int i = 0; i < NT; ++i) {
    const long k0 = k_lo + i * BK;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (AT)
        ra[i][j] = sk_load(A, k0 + a_r, lda, m_blk + a_v + j * 32,
                           k0 + a_r < k_hi, M);
      else
        ra[i][j] = sk_load(A, m_blk + a_r + j * 32, lda, k0 + a_v,
                           m_blk + a_r + j * 32 < M, k_hi);
    }
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      if (BT)
        rb[i][j] = sk_load(B, n_blk + b_r + j * 32, ldb, k0 + b_v,
                           n_blk + b_r + j * 32 < N, k_hi);
      else
        rb[i][j] = sk_load(B, k0 + b_r + j * 16, ldb, n_blk + b_v,
                           k0 + b_r + j * 16 < k_hi, N);
    }
  }

#pragma unroll
  for (int i = 0; i <= NT; ++i) {
    // first half of tile i - 1's MFMAs, the LDS write of tile i, the second
    // half: the wait for tile i's loads sits under tile i - 1's MFMAs
#pragma unroll
    for (int half = 0; half < 2; ++half) {
      if (i > 0) {
        const float* Abuf = A_lds[(i - 1) & 1];
        const float* Bbuf = B_lds[(i - 1) & 1];
#pragma unroll
        for (int kk = half * (BK / 8); kk < (half + 1) * (BK / 8); ++kk) {
          float a_frag[4], b_frag[2];
#pragma unroll
          for (int mi = 0; mi < 4; ++mi)
            a_frag[mi] =
                Abuf[(wr * 64 + mi * 16 + l15) * LDA_S + kk * 4 + l4];
#pragma unroll
          for (int ni = 0; ni < 2; ++ni)
            b_frag[ni] =
                Bbuf[(kk * 4 + l4) * LDB_S + wc * 32 + ni * 16 + l15];
#pragma unroll
          for (int mi = 0; mi < 4; ++mi)
#pragma unroll
            for (int ni = 0; ni < 2; ++ni)
              acc[mi][ni] = __builtin_amdgcn_mfma_f32_16x16x4f32(
                  a_frag[mi], b_frag[ni], acc[mi][ni], 0, 0, 0);
        }
      }
      if (half == 0 && i < NT) {
        const long k0 = k_lo + i * BK;
        float* Aw = A_lds[i & 1];
        float* Bw = B_lds[i & 1];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          if (AT) {
            const float4 q = sk_mask(ra[i][j], k0 + a_r < k_hi,
                                     m_blk + a_v + j * 32, M);
            const float v[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
            for (int e = 0; e < 4; ++e)
              Aw[(a_v + j * 32 + e) * LDA_S + a_r] = v[e];
          } else {
            const float4 q = sk_mask(ra[i][j], m_blk + a_r + j * 32 < M,
                                     k0 + a_v, k_hi);
            float* dst = &Aw[(a_r + j * 32) * LDA_S + a_v];
            ((float2*)dst)[0] = {q.x, q.y};
            ((float2*)dst)[1] = {q.z, q.w};
          }
        }
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          if (BT) {
            const float4 q = sk_mask(rb[i][j], n_blk + b_r + j * 32 < N,
                                     k0 + b_v, k_hi);
            const float v[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
            for (int e = 0; e < 4; ++e)
              Bw[(b_v + e) * LDB_S + b_r + j * 32] = v[e];
          } else {
            const float4 q = sk_mask(rb[i][j], k0 + b_r + j * 16 < k_hi,
                                     n_blk + b_v, N);
            *(float4*)&Bw[(b_r + j * 16) * LDB_S + b_v] = q;
          }
        }
      }
    }
    // tile i is in LDS for everyone; everyone is done reading tile i - 1
    if (i < NT) __syncthreads();
  }
}

// picks the instantiation of the block's tile count: nt in [0, NT]
template <int NT, bool AT, bool BT, typename... Args>
__device__ __forceinline__ void shortk_dispatch(int nt, Args&&... args) {
  if (nt == NT) {
    shortk_chunk<NT, AT, BT>(args...);
  } else if constexpr (NT > 1) {
    shortk_dispatch<NT - 1, AT, BT>(nt, args...);
  }
}

// Requires lda % 4 == 0 && ldb % 4 == 0 (gemm_f32_k's VEC) and
// k_per_chunk <= T * BK; arguments, grid, slab layout and epilogue are
// gemm_f32_k's.
template <int T, bool AT, bool BT>
__global__ __launch_bounds__(256)
void gemm_f32_shortk_k(const float* __restrict__ A,
                       const float* __restrict__ B, float* __restrict__ C,
                       const float* __restrict__ bias, int M, int N, int K,
                       int lda, int ldb, int ldc, long k_per_chunk, int relu,
                       int direct_out) {
  __shared__ float A_lds[2][BM * LDA_S];
  __shared__ float B_lds[2][BK * LDB_S];

  const int m_blk = blockIdx.x * BM;
  const int n_blk = blockIdx.y * BN;
  const long k_lo = (long)blockIdx.z * k_per_chunk;
  const long k_hi = min((long)K, k_lo + k_per_chunk);
  // block-uniform: a shorter last chunk and the empty chunks of a deep
  // split (which still write their zero slab) run a smaller instantiation
  const int nt = k_hi > k_lo ? (int)((k_hi - k_lo + BK - 1) / BK) : 0;

  f32x4 acc[4][2];
#pragma unroll
  for (int mi = 0; mi < 4; ++mi)
#pragma unroll
    for (int ni = 0; ni < 2; ++ni) acc[mi][ni] = {0.f, 0.f, 0.f, 0.f};

  shortk_dispatch<T, AT, BT>(nt, A, B, M, N, lda, ldb, m_blk, n_blk, k_lo,
                             k_hi, A_lds, B_lds, acc);

  const int t = threadIdx.x;
  const int lane = t & 63, wave = t >> 6;
  const int wr = wave >> 1, wc = wave & 1;
  const int l15 = lane & 15, l4 = lane >> 4;
  // the output: C itself or this chunk's slab, [M][ldo]
  const int ldo = direct_out ? ldc : N;
  float* __restrict__ O = direct_out ? C : C + (long)blockIdx.z * M * N;
  // epilogue: C/D mapping col = lane&15, row = (lane>>4)*4 + reg
#pragma unroll
  for (int mi = 0; mi < 4; ++mi) {
#pragma unroll
    for (int ni = 0; ni < 2; ++ni) {
      int col = n_blk + wc * 32 + ni * 16 + l15;
      if (col >= N) continue;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        int row = m_blk + wr * 64 + mi * 16 + l4 * 4 + r;
        if (row >= M) continue;
        float v = acc[mi][ni][r];
        if (direct_out) {
          if (bias) v += bias[col];
          if (relu) v = fmaxf(v, 0.f);
        }
        O[(long)row * ldo + col] = v;
      }
    }
  }
}

// fixed-order split-K reduce + bias + relu.  Two geometries:
//  * small outputs / large SK: one WAVE per output, lanes over z + shuffle
//    tree (the serial-z loop was pure L2-latency, 60 us for 288 outputs)
//  * large outputs: thread per output with 4-way z ILP
__global__ void splitk_reduce_wave_k(const float* __restrict__ ws,
                                     float* __restrict__ C,
                                     const float* __restrict__ bias, int M,
                                     int N, int ldc, int SK, int relu) {
  long n_out = (long)M * N;
  long i = blockIdx.x * (long)(blockDim.x / kWave) + threadIdx.x / kWave;
  int lane = threadIdx.x % kWave;
  if (i >= n_out) return;
  float acc = 0.f;
  for (int z = lane; z < SK; z += kWave) acc += ws[(long)z * n_out + i];
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off, kWave);
  if (lane == 0) {
    int col = i % N;
    if (bias) acc += bias[col];
    if (relu) acc = fmaxf(acc, 0.f);
    C[(i / N) * (long)ldc + col] = acc;
  }
}

// (the thread-per-output form and the stage-1 fold of a deep split are
// roles: bodies in step_roles.h, makers below)

// Direct small GEMM: for tiny outputs (the 10/128-wide fc2 shapes) the
// MFMA tile machinery + split-K reduce is pure overhead — a grid-stride
// dot-product kernel does the whole thing in one short launch.  K summed
// in order with 4 rotating accumulators (deterministic).
__global__ void gemm_small_k(const float* __restrict__ A,
                             const float* __restrict__ B,
                             float* __restrict__ C,
                             const float* __restrict__ bias, int M, int N,
                             int K, int lda, int ldb, int ldc, int relu,
                             int layout) {
  long n_out = (long)M * N;
  long stride = (long)gridDim.x * blockDim.x;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n_out;
       i += stride) {
    int n = (int)(i % N);
    int m = (int)(i / N);
    const float* a = layout == 1 ? A + m : A + (long)m * lda;
    const long astep = layout == 1 ? lda : 1;
    const float* b = layout == 2 ? B + (long)n * ldb : B + n;
    const long bstep = layout == 2 ? 1 : ldb;
    float acc = dot_rot4(K, [&](int k) { return a[k * astep]; },
                         [&](int k) { return b[k * bstep]; });
    if (bias) acc += bias[n];
    if (relu) acc = fmaxf(acc, 0.f);
    C[(long)m * ldc + n] = acc;
  }
}

// wave-per-output form of the small GEMM: lanes stride K with a shuffle
// tree (deterministic).  The thread-per-output form is latency-starved
// when outputs are few and K is real (fc2 fwd/dw: 15.4 us avg measured —
// 1-10 waves on a 256-CU chip).
__global__ void gemm_small_wave_k(const float* __restrict__ A,
                                  const float* __restrict__ B,
                                  float* __restrict__ C,
                                  const float* __restrict__ bias, int M,
                                  int N, int K, int lda, int ldb, int ldc,
                                  int relu, int layout) {
  long out = blockIdx.x * (long)(blockDim.x / kWave) + threadIdx.x / kWave;
  int lane = threadIdx.x % kWave;
  if (out >= (long)M * N) return;
  int n = (int)(out % N);
  int m = (int)(out / N);
  const float* a = layout == 1 ? A + m : A + (long)m * lda;
  const long astep = layout == 1 ? lda : 1;
  const float* b = layout == 2 ? B + (long)n * ldb : B + n;
  const long bstep = layout == 2 ? 1 : ldb;
  float acc = dot_wave_partial(K, lane, [&](int k) { return a[k * astep]; },
                               [&](int k) { return b[k * bstep]; });
  acc = wave_tree_down(acc);
  if (lane == 0) {
    if (bias) acc += bias[n];
    if (relu) acc = fmaxf(acc, 0.f);
    C[(long)m * ldc + n] = acc;
  }
}

extern "C" {

// Heuristic split-K: fill the chip (256 CUs) when the tile grid is
// small.  The block target is env-tunable for sweeps
// (RLR_GEMM_SK_TARGET); the sweep at the fc1 shapes read 5.43 / 5.35 /
// 5.23 rounds/s at targets 256 / 512 / 1024 — deeper splits pay more in
// slab+reduce traffic than the overlapped prologue returns.
int gemm_f32_splitk(int M, int N, int K) {
  static long target = -1;
  if (target < 0) {
    const char* e = getenv("RLR_GEMM_SK_TARGET");
    target = e ? atol(e) : 256;
  }
  long tiles = ((M + BM - 1) / BM) * (long)((N + BN - 1) / BN);
  if (tiles >= 192 || K <= 2 * BK) return 1;
  long want = (target + tiles - 1) / tiles;
  long max_chunks = (K + BK - 1) / BK;
  long sk = want < max_chunks ? want : max_chunks;
  return (int)(sk < 1 ? 1 : (sk > 192 ? 192 : sk));
}

// Split-K workspace of launch_gemm_f32_main and launch_gemm_bf16 (both
// combine through splitk_reduce_roles): SK slabs of M*N partials, then the
// stage-1 slabs of a deep split.  No workspace for SK == 1.
long gemm_splitk_ws_floats(int M, int N, int SK) {
  if (SK == 1) return 0;
  return (long)(SK + splitk_stage1_slabs(SK)) * M * N;
}

// launch_gemm_f32_main's tiny-problem branch: one direct kernel, no tiles
static bool gemm_f32_tiny(int M, int N, int K) {
  return (long)M * N * K <= 8'000'000 && (long)M * N <= 65536;
}

// The K-tiles per chunk when launch_gemm_f32_main runs the short-K form,
// else 0: the call takes the tile path, both row strides allow float4
// loads, and a full chunk holds 3..kShortKMaxTiles K-tiles.  (A two-tile
// chunk has at most one latency to lose in gemm_f32_k.)  Host arithmetic
// only; RLR_AMD_NO_GEMM_SHORTK is the launcher's business, not this
// function's.
int gemm_f32_shortk_tiles(int M, int N, int K, int SK, int lda, int ldb) {
  if (gemm_f32_tiny(M, N, K)) return 0;
  if (lda % 4 != 0 || ldb % 4 != 0) return 0;
  long k_per_chunk = SK == 1 ? (long)K
                             : ((((long)K + SK - 1) / SK + BK - 1) / BK) * BK;
  if (k_per_chunk <= 2 * BK || k_per_chunk > kShortKMaxTiles * BK) return 0;
  return (int)((k_per_chunk + BK - 1) / BK);
}

// the short-K launches of launch_gemm_f32_main, same arguments
static void launch_gemm_f32_shortk(const float* A, const float* B, float* out,
                                   const float* bias, int M, int N, int K,
                                   int lda, int ldb, int ldc, dim3 grid,
                                   long k_per_chunk, int relu, int direct_out,
                                   int layout, hipStream_t st) {
  constexpr int T = kShortKMaxTiles;
  if (layout == 1)
    gemm_f32_shortk_k<T, true, false><<<grid, 256, 0, st>>>(
        A, B, out, bias, M, N, K, lda, ldb, ldc, k_per_chunk, relu,
        direct_out);
  else if (layout == 2)
    gemm_f32_shortk_k<T, false, true><<<grid, 256, 0, st>>>(
        A, B, out, bias, M, N, K, lda, ldb, ldc, k_per_chunk, relu,
        direct_out);
  else
    gemm_f32_shortk_k<T, false, false><<<grid, 256, 0, st>>>(
        A, B, out, bias, M, N, K, lda, ldb, ldc, k_per_chunk, relu,
        direct_out);
}

// ws: null unless SK>1, then gemm_splitk_ws_floats(M, N, SK) floats.
// layout: 0 = NN, 1 = A transposed ([K][M]), 2 = B transposed ([N][K]).
// A chunk of 3..5 K-tiles with float4-able strides runs the short-K form
// (gemm_f32_shortk_tiles) unless RLR_AMD_NO_GEMM_SHORTK=1, which is read on
// every call and sends everything to gemm_f32_k.
// The main kernel only.  Returns 1 when it left SK partial slabs in ws that
// launch_splitk_reduce (or the roles of splitk_reduce_roles) must still
// fold into C, 0 when C is complete.
int launch_gemm_f32_main(const float* A, const float* B, float* C,
                         const float* bias, float* ws, int M, int N, int K,
                         int lda, int ldb, int ldc, int SK, int relu,
                         int layout, void* s) {
  hipStream_t st = (hipStream_t)s;
  // tiny problems: one direct kernel beats tile GEMM + split-K reduce;
  // with a real K give every output a wave (lane-strided K + shuffle)
  if (gemm_f32_tiny(M, N, K)) {
    if (K >= 32) {
      int wpb = kBlock / kWave;
      gemm_small_wave_k<<<((long)M * N + wpb - 1) / wpb, kBlock, 0, st>>>(
          A, B, C, bias, M, N, K, lda, ldb, ldc, relu, layout);
    } else {
      gemm_small_k<<<grid_for((long)M * N), kBlock, 0, st>>>(
          A, B, C, bias, M, N, K, lda, ldb, ldc, relu, layout);
    }
    return 0;
  }
  dim3 grid((M + BM - 1) / BM, (N + BN - 1) / BN, SK);
  long k_per_chunk = SK == 1 ? (long)K
                             : ((((long)K + SK - 1) / SK + BK - 1) / BK) * BK;
  bool vec = (lda % 4 == 0) && (ldb % 4 == 0);
  float* out = SK == 1 ? C : ws;
  const char* no_shortk = getenv("RLR_AMD_NO_GEMM_SHORTK");
  if (!(no_shortk && no_shortk[0] == '1') &&
      gemm_f32_shortk_tiles(M, N, K, SK, lda, ldb)) {
    launch_gemm_f32_shortk(A, B, out, bias, M, N, K, lda, ldb, ldc, grid,
                           k_per_chunk, relu, SK == 1, layout, st);
    return SK > 1;
  }
  if (layout == 1) {
    if (vec)
      gemm_f32_k<true, true, false><<<grid, 256, 0, st>>>(
          A, B, out, bias, M, N, K, lda, ldb, ldc, k_per_chunk, relu,
          SK == 1);
    else
      gemm_f32_k<false, true, false><<<grid, 256, 0, st>>>(
          A, B, out, bias, M, N, K, lda, ldb, ldc, k_per_chunk, relu,
          SK == 1);
  } else if (layout == 2) {
    if (vec)
      gemm_f32_k<true, false, true><<<grid, 256, 0, st>>>(
          A, B, out, bias, M, N, K, lda, ldb, ldc, k_per_chunk, relu,
          SK == 1);
    else
      gemm_f32_k<false, false, true><<<grid, 256, 0, st>>>(
          A, B, out, bias, M, N, K, lda, ldb, ldc, k_per_chunk, relu,
          SK == 1);
  } else if (vec)
    gemm_f32_k<true><<<grid, 256, 0, st>>>(A, B, out, bias, M, N, K, lda,
                                           ldb, ldc, k_per_chunk, relu,
                                           SK == 1);
  else
    gemm_f32_k<false><<<grid, 256, 0, st>>>(A, B, out, bias, M, N, K, lda,
                                            ldb, ldc, k_per_chunk, relu,
                                            SK == 1);
  return SK > 1;
}

// stage-1 partial for deep split-K: each (output, 16-slab chunk) gets its
// own thread — the single-stage thread-per-output form is parallelism-
// starved when n_out is small and SK deep (e.g. 64 slabs x 32k outputs)
StepRole splitk_partial_role(const float* ws, float* out, long n_out, int S,
                             int zstride) {
  int chunks = (S + zstride - 1) / zstride;
  StepRole r{};
  r.kind = kRoleSplitkPartial;
  r.gx = grid_for(n_out * chunks);
  r.gy = 1;
  r.count = r.gx;
  r.splitk_partial.ws = ws;
  r.splitk_partial.out = out;
  r.splitk_partial.n_out = n_out;
  r.splitk_partial.S = S;
  r.splitk_partial.zstride = zstride;
  return r;
}

static StepRole splitk_reduce_role(const float* ws, float* C,
                                   const float* bias, int M, int N, int ldc,
                                   int SK, int relu) {
  StepRole r{};
  r.kind = kRoleSplitkReduce;
  r.gx = grid_for((long)M * N);
  r.gy = 1;
  r.count = r.gx;
  r.splitk_reduce.ws = ws;
  r.splitk_reduce.C = C;
  r.splitk_reduce.bias = bias;
  r.splitk_reduce.M = M;
  r.splitk_reduce.N = N;
  r.splitk_reduce.ldc = ldc;
  r.splitk_reduce.SK = SK;
  r.splitk_reduce.relu = relu;
  return r;
}

// The split-K combine as roles: returns the number of levels, 2 (*l1
// folds, *l2 finishes), 1 (*l1 is the thread-form reduce) or 0: the wave
// form has no role, launch_splitk_reduce runs it.  ws holds
// gemm_splitk_ws_floats(M, N, SK) floats: the stage-1 scratch is the
// splitk_stage1_slabs(SK) slabs after the SK partials.
int splitk_reduce_roles(const float* ws, float* C, const float* bias, int M,
                        int N, int ldc, int SK, int relu, StepRole* l1,
                        StepRole* l2) {
  long n_out = (long)M * N;
  if (SK > kSplitKFold && n_out <= 262144) {
    int chunks = splitk_stage1_slabs(SK);
    float* ws2 = const_cast<float*>(ws) + (long)SK * n_out;
    *l1 = splitk_partial_role(ws, ws2, n_out, SK, kSplitKFold);
    *l2 = splitk_reduce_role(ws2, C, bias, M, N, ldc, chunks, relu);
    return 2;
  }
  if (n_out <= 8192 && SK >= 16) return 0;
  *l1 = splitk_reduce_role(ws, C, bias, M, N, ldc, SK, relu);
  return 1;
}

// column sum: db[n] = sum_m dY[m][n] (bias gradient), one wave per column
StepRole colsum_role(const float* dY, float* db, int M, int N) {
  int wpb = kBlock / kWave;
  StepRole r{};
  r.kind = kRoleColsum;
  r.gx = (N + wpb - 1) / wpb;
  r.gy = 1;
  r.count = r.gx;
  r.colsum.dY = dY;
  r.colsum.db = db;
  r.colsum.M = M;
  r.colsum.N = N;
  return r;
}

// the combine now: its roles in order, or the wave form
void launch_splitk_reduce(const float* ws, float* C, const float* bias,
                          int M, int N, int ldc, int SK, int relu, void* s) {
  StepRole a, b;
  int levels = splitk_reduce_roles(ws, C, bias, M, N, ldc, SK, relu, &a, &b);
  if (levels == 0) {
    long n_out = (long)M * N;
    int wpb = kBlock / kWave;
    splitk_reduce_wave_k<<<(n_out + wpb - 1) / wpb, kBlock, 0,
                           (hipStream_t)s>>>(ws, C, bias, M, N, ldc, SK,
                                             relu);
    return;
  }
  launch_step_role(&a, s);
  if (levels == 2) launch_step_role(&b, s);
}
}
