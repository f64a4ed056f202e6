// Bodies of the small fold / permute / copy kernels of a training step:
// one role_run overload per kind, a __device__ function of the kind's
// argument struct (launchers.h), the block index (bx, by) inside the role's
// grid, the grid's width gx and, for the two bodies that reduce through
// LDS, kBlock floats of it.  step_role_run at the end is the one dispatch
// from a StepRole to its body.  Both kernels of step_batch.hip, the one that
// runs a role alone and the one that runs up to 16 in one launch, go through
// it: this is the tail_math.h rule one level up, a batched role and the
// same role alone are bitwise equal because they are the same code.  Every
// body expects blockDim.x == kBlock.
//
// A body reads its scalars from the struct by name and takes its pointers
// as the __restrict__ parameters of a lambda it calls at once: the compiler
// honours __restrict__ on parameters only, and without it the grid-stride
// loops lose their unrolling (the weight permutes drop from 36 to 21 VGPRs,
// step_batch_k from 6471 to 4107 instructions).
#pragma once
#include "common.h"
#include "launchers.h"
#include "tail_math.h"

// ------------------------------------------------------------ role lookup
// The role that owns flat block b: the first entry whose [first, first +
// count) holds it.  An entry with count == 0 owns nothing.  -1: no owner.
__host__ __device__ inline int step_role_of(const StepRole* roles, int n,
                                            int b) {
  for (int r = 0; r < n; ++r)
    if (b >= roles[r].first && b - roles[r].first < roles[r].count) return r;
  return -1;
}

// ------------------------------------------------------- conv bias grads
// db[ko] = column sum of dy [M][KO] in two stages.  thread -> (slice = tid
// / K_blk, ko = tid % K_blk): all four waves of a block work even when
// Kout < 256.
__device__ __forceinline__ void role_run(const ConvDbStage1Args& a, int bx,
                                         int by, int, float*) {
  const long M = a.M;
  const int Kout = a.Kout, chunks = a.chunks, K_blk = a.K_blk;
  [&](const float* __restrict__ dy, float* __restrict__ partials) {
    int sub_per = blockDim.x / K_blk;
    int ko = by * K_blk + threadIdx.x % K_blk;
    int chunk = bx * sub_per + threadIdx.x / K_blk;
    if (ko >= Kout || chunk >= chunks) return;
    long per = (M + chunks - 1) / chunks;
    long lo = (long)chunk * per, hi = min(M, lo + per);
    float acc = 0.f;
#pragma unroll 4
    for (long m = lo; m < hi; ++m) acc += dy[m * Kout + ko];
    partials[(long)chunk * Kout + ko] = acc;
  }(a.dy, a.partials);
}

// one BLOCK per ko: 256 threads stride the chunks, LDS tree combine.
// sh: kBlock floats of LDS.
__device__ __forceinline__ void role_run(const ConvDbStage2Args& a, int bx,
                                         int, int, float* sh) {
  const int Kout = a.Kout, chunks = a.chunks;
  [&](const float* __restrict__ partials, float* __restrict__ db) {
    int ko = bx;
    float acc = 0.f;
    for (int c = threadIdx.x; c < chunks; c += blockDim.x)
      acc += partials[(long)c * Kout + ko];
    sh[threadIdx.x] = acc;
    __syncthreads();
    for (int off = kBlock / 2; off > 0; off >>= 1) {
      if (threadIdx.x < off) sh[threadIdx.x] += sh[threadIdx.x + off];
      __syncthreads();
    }
    if (threadIdx.x == 0) db[ko] = sh[0];
  }(a.partials, a.db);
}

// ---------------------------------------------------------- split-K folds
// stage-1 partial for deep split-K: each (output, zstride-slab chunk) gets
// its own thread
__device__ __forceinline__ void role_run(const SplitkPartialArgs& a, int bx,
                                         int, int gx, float*) {
  const long n_out = a.n_out;
  const int S = a.S, zstride = a.zstride;
  [&](const float* __restrict__ ws, float* __restrict__ out) {
    long stride = (long)gx * blockDim.x;
    long total = n_out * ((S + zstride - 1) / zstride);
    for (long v = (long)bx * blockDim.x + threadIdx.x; v < total; v += stride) {
      long i = v % n_out;
      int chunk = (int)(v / n_out);
      int z0 = chunk * zstride, z1 = min(S, z0 + zstride);
      float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
      int z = z0;
      for (; z + 3 < z1; z += 4) {
        a0 += ws[(long)z * n_out + i];
        a1 += ws[(long)(z + 1) * n_out + i];
        a2 += ws[(long)(z + 2) * n_out + i];
        a3 += ws[(long)(z + 3) * n_out + i];
      }
      for (; z < z1; ++z) a0 += ws[(long)z * n_out + i];
      out[(long)chunk * n_out + i] = (a0 + a1) + (a2 + a3);
    }
  }(a.ws, a.out);
}

// fixed-order split-K reduce + bias + relu, thread per output, 4-way z ILP
__device__ __forceinline__ void role_run(const SplitkReduceArgs& a, int bx,
                                         int, int gx, float*) {
  const int M = a.M, N = a.N, ldc = a.ldc, SK = a.SK, relu = a.relu;
  [&](const float* __restrict__ ws, float* __restrict__ C,
      const float* __restrict__ bias) {
    long n_out = (long)M * N;
    long stride = (long)gx * blockDim.x;
    for (long i = (long)bx * blockDim.x + threadIdx.x; i < n_out;
         i += stride) {
      float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
      int z = 0;
      for (; z + 3 < SK; z += 4) {
        a0 += ws[(long)z * n_out + i];
        a1 += ws[(long)(z + 1) * n_out + i];
        a2 += ws[(long)(z + 2) * n_out + i];
        a3 += ws[(long)(z + 3) * n_out + i];
      }
      for (; z < SK; ++z) a0 += ws[(long)z * n_out + i];
      float acc = (a0 + a1) + (a2 + a3);
      int col = i % N;
      if (bias) acc += bias[col];
      if (relu) acc = fmaxf(acc, 0.f);
      C[(i / N) * (long)ldc + col] = acc;
    }
  }(a.ws, a.C, a.bias);
}

// fused split-K combine + dw permute: sums the SK rsc-ordered slabs and
// writes straight into the torch (ko,(c,r,s)) layout
__device__ __forceinline__ void role_run(const SplitkReduceDwpermArgs& a,
                                         int bx, int, int gx, float*) {
  const int Kout = a.Kout, C = a.C, RS = a.RS, SK = a.SK;
  [&](const float* __restrict__ ws, float* __restrict__ dw) {
    long n_out = (long)Kout * C * RS;
    long stride = (long)gx * blockDim.x;
    int CRS = C * RS;
    for (long i = (long)bx * blockDim.x + threadIdx.x; i < n_out;
         i += stride) {
      float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
      int z = 0;
      for (; z + 3 < SK; z += 4) {
        a0 += ws[(long)z * n_out + i];
        a1 += ws[(long)(z + 1) * n_out + i];
        a2 += ws[(long)(z + 2) * n_out + i];
        a3 += ws[(long)(z + 3) * n_out + i];
      }
      for (; z < SK; ++z) a0 += ws[(long)z * n_out + i];
      float acc = (a0 + a1) + (a2 + a3);
      int col = i % CRS;  // (r,s,c) flat: rs*C + c
      long ko = i / CRS;
      int c = col % C;
      int rs = col / C;
      dw[(ko * C + c) * RS + rs] = acc;
    }
  }(a.ws, a.dw);
}

// combine the small-conv bwd-weight chunk partials (fixed order, wave per
// pair) + permute (r,s,c)->(c,r,s)
__device__ __forceinline__ void role_run(const ConvSmallBwdwReduceArgs& a,
                                         int bx, int, int, float*) {
  const int KO = a.KO, C = a.C, RS = a.RS, chunks = a.chunks;
  [&](const float* __restrict__ partials, float* __restrict__ dw) {
    int pairs = KO * C * RS;
    int p = bx * (blockDim.x / kWave) + threadIdx.x / kWave;
    int lane = threadIdx.x % kWave;
    if (p >= pairs) return;
    float acc = 0.f;
    for (int ch = lane; ch < chunks; ch += kWave)
      acc += partials[(long)ch * pairs + p];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off, kWave);
    if (lane == 0) {
      int crs = p % (C * RS);   // (r,s,c)
      int ko = p / (C * RS);
      int c = crs % C;
      int rs = crs / C;
      dw[(ko * C + c) * RS + rs] = acc;
    }
  }(a.partials, a.dw);
}

// column sum: db[n] = sum_m dY[m][n], one wave per column
__device__ __forceinline__ void role_run(const ColsumArgs& a, int bx, int,
                                         int, float*) {
  const int M = a.M, N = a.N;
  [&](const float* __restrict__ dY, float* __restrict__ db) {
    int n = bx * (blockDim.x / kWave) + threadIdx.x / kWave;
    int lane = threadIdx.x % kWave;
    if (n >= N) return;
    float acc = colsum_wave(dY, M, N, n, lane);
    if (lane == 0) db[n] = acc;
  }(a.dY, a.db);
}

// ------------------------------------------------------ classifier head B
// The three reductions over the batch; a block takes its part from its
// index.  dW: GEMM (M=C, N=H, K=B) with A = dlogits consumed transposed;
// db: column sums of dlogits; loss: mean of the rows.  sh: kBlock floats.
__device__ __forceinline__ void role_run(const FcHeadReduceArgs& a, int blk,
                                         int, int, float* sh) {
  const int B = a.B, H = a.H, C = a.C;
  const int dw_blocks = a.dw_blocks, db_blocks = a.db_blocks;
  const int dw_wave = a.dw_wave;
  [&](const float* __restrict__ gl, const float* __restrict__ d2,
      const float* __restrict__ row_loss, float* __restrict__ dw,
      float* __restrict__ db, float* __restrict__ loss) {
    const int wave = threadIdx.x / kWave, lane = threadIdx.x % kWave;
    const long n_out = (long)C * H;
    if (blk < dw_blocks) {
      long out = dw_wave ? blk * (long)(kBlock / kWave) + wave
                         : blk * (long)kBlock + threadIdx.x;
      if (out >= n_out) return;
      int n = (int)(out % H);
      int m = (int)(out / H);
      const float* a = gl + m;
      const float* bp = d2 + n;
      if (dw_wave) {
        float acc = dot_wave_partial(
            B, lane, [&](int k) { return a[(long)k * C]; },
            [&](int k) { return bp[(long)k * H]; });
        acc = wave_tree_down(acc);
        if (lane == 0) dw[(long)m * H + n] = acc;
      } else {
        dw[(long)m * H + n] =
            dot_rot4(B, [&](int k) { return a[(long)k * C]; },
                     [&](int k) { return bp[(long)k * H]; });
      }
    } else if (blk < dw_blocks + db_blocks) {
      int n = (blk - dw_blocks) * (kBlock / kWave) + wave;
      if (n >= C) return;
      float acc = colsum_wave(gl, B, C, n, lane);
      if (lane == 0) db[n] = acc;
    } else {
      float mean = ce_mean_block(row_loss, B, sh);
      if (threadIdx.x == 0) loss[0] = mean;
    }
  }(a.gl, a.d2, a.row_loss, a.dw, a.db, a.loss);
}

// -------------------------------------------------------- weight permutes
// w (Kout,C,R,S) -> out[((rs)*C + c)*Kout + ko] (KIND kRoleWpermRscKo) or
// out[((rs)*Kout + ko)*C + c] (kRoleWpermRskoC)
template <int KIND>
__device__ __forceinline__ void role_run_wperm(const WpermArgs& a, int bx,
                                               int gx) {
  const int Kout = a.Kout, C = a.C, RS = a.RS;
  [&](const float* __restrict__ w, float* __restrict__ out) {
    long n = (long)Kout * C * RS;
    long stride = (long)gx * blockDim.x;
    for (long i = (long)bx * blockDim.x + threadIdx.x; i < n; i += stride) {
      int rs = i % RS;
      int c = (i / RS) % C;
      long ko = i / ((long)RS * C);
      if (KIND == kRoleWpermRscKo)
        out[((long)rs * C + c) * Kout + ko] = w[i];
      else
        out[((long)rs * Kout + ko) * C + c] = w[i];
    }
  }(a.w, a.out);
}

// ------------------------------------------------------------- step feed
// dst row r = src row sel[r]; rows are row_words 32-bit words (a float
// image, or the two halves of an int64 label).  vec: row_words % 4 == 0
// and both bases 16-byte aligned, so a row moves as uint4.  Precondition:
// 0 <= sel[r] < src_rows.  An index outside that range is never
// dereferenced: its row is filled with all-one bits (NaN images, label -1)
// so that the mistake shows downstream instead of reading out of bounds.
__device__ __forceinline__ void role_run(const GatherRowsArgs& a, int bx,
                                         int, int gx, float*) {
  const long rows = a.rows;
  const int row_words = a.row_words, vec = a.vec, src_rows = a.src_rows;
  [&](const uint32_t* __restrict__ src, const long* __restrict__ sel,
      uint32_t* __restrict__ dst) {
    long stride = (long)gx * blockDim.x;
    if (vec) {
      int rw4 = row_words / 4;
      long total = rows * rw4;
      const uint4* s4 = (const uint4*)src;
      uint4* d4 = (uint4*)dst;
      for (long i = (long)bx * blockDim.x + threadIdx.x; i < total;
           i += stride) {
        long r = i / rw4;
        int j = (int)(i - r * rw4);
        long sr = sel[r];
        uint4 v = make_uint4(~0u, ~0u, ~0u, ~0u);
        if (sr >= 0 && sr < src_rows) v = s4[sr * rw4 + j];
        d4[i] = v;
      }
      return;
    }
    long total = rows * row_words;
    for (long i = (long)bx * blockDim.x + threadIdx.x; i < total;
         i += stride) {
      long r = i / row_words;
      int j = (int)(i - r * row_words);
      long sr = sel[r];
      dst[i] = (sr >= 0 && sr < src_rows) ? src[sr * row_words + j] : ~0u;
    }
  }(a.src, a.sel, a.dst);
}

// one thread: *p += delta (the dropout base offset of the next step)
__device__ __forceinline__ void role_run(const AddU64Args& a, int, int, int,
                                         float*) {
  if (threadIdx.x == 0) *a.p = *a.p + a.delta;
}

// --------------------------------------------------------------- dispatch
// Block (bx, by) of role r's grid, as kind `kind`: r.kind in the batched
// kernel, a compile-time constant in the kernel that runs one role alone, so
// that only that body is compiled into it.  The one place a role's arguments
// are read.  sh: kBlock floats of LDS for the kinds with
// step_role_uses_lds, unused (and may be null) for the others.
constexpr bool step_role_uses_lds(int kind) {
  return kind == kRoleConvDbStage2 || kind == kRoleFcHeadReduce;
}

__device__ __forceinline__ void step_role_run(int kind, const StepRole& r,
                                              int bx, int by, float* sh) {
  switch (kind) {
    case kRoleConvDbStage1:
      return role_run(r.conv_db_stage1, bx, by, r.gx, sh);
    case kRoleConvDbStage2:
      return role_run(r.conv_db_stage2, bx, by, r.gx, sh);
    case kRoleSplitkPartial:
      return role_run(r.splitk_partial, bx, by, r.gx, sh);
    case kRoleSplitkReduce:
      return role_run(r.splitk_reduce, bx, by, r.gx, sh);
    case kRoleSplitkReduceDwperm:
      return role_run(r.splitk_reduce_dwperm, bx, by, r.gx, sh);
    case kRoleConvSmallBwdwReduce:
      return role_run(r.conv_small_bwdw_reduce, bx, by, r.gx, sh);
    case kRoleColsum:
      return role_run(r.colsum, bx, by, r.gx, sh);
    case kRoleFcHeadReduce:
      return role_run(r.fc_head_reduce, bx, by, r.gx, sh);
    case kRoleWpermRscKo:
      return role_run_wperm<kRoleWpermRscKo>(r.wperm, bx, r.gx);
    case kRoleWpermRskoC:
      return role_run_wperm<kRoleWpermRskoC>(r.wperm, bx, r.gx);
    case kRoleGatherRows:
      return role_run(r.gather_rows, bx, by, r.gx, sh);
    case kRoleAddU64:
      return role_run(r.add_u64, bx, by, r.gx, sh);
    default:
      return;
  }
}
