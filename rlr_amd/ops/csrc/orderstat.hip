// Per-coordinate order statistics of the stacked (K, n) fp64 update matrix:
// coordinate median at any K up to kOrderstatMaxK and the coordinate-wise
// trimmed mean (Yin et al., 2018), optionally fused with the RLR sign vote
// and the fp32 parameter apply.
//
// One block owns a tile of kTile = 32 columns laid out [k][kTile] in LDS and
// sorts every column ascending with a bitonic network padded to P = pow2 >= K
// with +inf.  L lanes cooperate on a column (small K: L = 1 and the block
// carries several tiles); thread t serves column t % 32, so the 32 lanes of
// a half-wave always touch ONE LDS row of 32 x 8 B = 256 B = one full bank
// row: every ds_read_b64 / ds_write_b64 lane group is conflict-free
// (cdna_hip_programming.md §2 'Bank structure').
//
// The network runs in PASSES of up to four steps: a lane takes 2^NB rows
// whose indices differ only in NB consecutive bits into registers, runs the
// NB compare-exchange steps that pair exactly those rows, and writes them
// back — one LDS round trip and one barrier per pass instead of per step
// (12 passes instead of 45 steps at P = 512).  The first pass sorts runs of
// 16 entirely in registers.  Every index is a function of (pass, lane)
// only and every register index is a compile-time constant (§5.4:
// runtime-indexed local arrays spill), so all lanes execute the same
// sequence with no divergence.
//
// After the sort lane 0 of each column reads off
//     agg = (s[lo] + s[lo+1] + ... + s[hi-1]) * inv_cnt
// accumulated SEQUENTIALLY in ascending order in fp64.  That order is part
// of the contract: it makes the result independent of agent order and
// bitwise reproducible on the CPU (torch.sort + a row loop).  Median =
// (lo, hi) = ((K-1)/2, (K-1)/2 + 1) with inv_cnt = 1 (exact selection, the
// lower middle for even K = torch.median); trimmed mean with b dropped per
// side = (b, K - b).
//
// The RLR vote comes from the resident tile: each lane counts the signs of
// the rows it loads, the L partial counts meet in LDS.  Sums of +-1 are
// exact in any order, so lr is bitwise rlr_vote_k's.
//
// bulyan_k below is the sibling for Bulyan's second stage: the same network
// over a device-chosen subset of the rows and a per-column window around
// the subset's median instead of the fixed span.
#include "common.h"
#include "launchers.h"

constexpr int kTile = 32;             // columns per block tile (256 B rows)
constexpr int kOrderstatMaxK = 512;   // P*kTile*8 B = 128 KiB of 160 KiB LDS
constexpr int kOrderstatMaxLanes = 32;
constexpr int kPassBits = 4;          // 2^4 rows = 32 VGPRs per lane per pass

// ------------------------------------------------------- sorting network
// A pass runs the steps with partner distance 2^(sh+nb-1) .. 2^sh of the
// merge of size kk; the head pass (sh = 0) runs ALL merges 2 .. kk = 2^nb,
// i.e. sorts runs of 2^nb rows entirely in registers.
struct NetPass {
  int kk, sh, nb;
  bool head;
};

// Pass schedule of the bitonic network over P = 2^lg rows.  Start from a
// zeroed NetPass; returns false when the network is complete.
//   pass 0:  merges kk = 2 .. 2^min(lg,4), all inside one register group
//   then per merge kk = 2^b: its b steps from the top, four bits at a time
__host__ __device__ inline bool net_next(int lg, NetPass& t) {
  if (t.nb == 0) {
    if (lg == 0) return false;
    t.nb = lg < kPassBits ? lg : kPassBits;
    t.sh = 0;
    t.kk = 1 << t.nb;
    t.head = true;
    return true;
  }
  t.head = false;
  int top = t.sh;               // bits [0, sh) of the current merge remain
  if (top == 0) {               // merge finished: next size
    t.kk <<= 1;
    if (t.kk > (1 << lg)) return false;
    top = 31 - __builtin_clz(t.kk);
  }
  t.nb = top < kPassBits ? top : kPassBits;
  t.sh = top - t.nb;
  return true;
}

// min to a, max to b (or the reverse): two fp64 instructions, no selects.
// Equal values stay equal, so for finite input this permutes the values.
__host__ __device__ __forceinline__ void cmpex(double& a, double& b,
                                               bool up) {
  double x = fmin(a, b);
  double y = fmax(a, b);
  a = up ? x : y;
  b = up ? y : x;
}

// Lane j of L runs pass t on column c of the [P][kTile] tile s.  A group
// that the network sorts descending is taken into the registers in
// REVERSED order, so the direction of every compare-exchange is known at
// compile time: ascending in register order, except inside the head pass's
// smaller merges, where it alternates with the register index.
template <int NB, bool HEAD>
__host__ __device__ __forceinline__ void net_pass(double* s, int c, int j,
                                                  int L, int P,
                                                  const NetPass& t) {
  constexpr int R = 1 << NB;
  const int sh = t.sh;
  for (int g = j; g < (P >> NB); g += L) {
    // spread g around the NB group bits: [high | group bits | low sh bits]
    const int base = ((g >> sh) << (sh + NB)) | (g & ((1 << sh) - 1));
    const int flip = (base & t.kk) ? R - 1 : 0;
    double r[R];
#pragma unroll
    for (int m = 0; m < R; ++m)
      r[m] = s[(base | ((m ^ flip) << sh)) * kTile + c];
#pragma unroll
    for (int lk = HEAD ? 1 : NB; lk <= NB; ++lk) {   // merge of 2^lk rows
#pragma unroll
      for (int b = lk - 1; b >= 0; --b) {
#pragma unroll
        for (int m = 0; m < R; ++m) {
          if ((m & (1 << b)) == 0)
            cmpex(r[m], r[m | (1 << b)], lk == NB || ((m >> lk) & 1) == 0);
        }
      }
    }
#pragma unroll
    for (int m = 0; m < R; ++m)
      s[(base | ((m ^ flip) << sh)) * kTile + c] = r[m];
  }
}

__host__ __device__ __forceinline__ void net_pass_n(double* s, int c, int j,
                                                    int L, int P,
                                                    const NetPass& t) {
  if (t.head) {
    switch (t.nb) {
      case 1: net_pass<1, true>(s, c, j, L, P, t); break;
      case 2: net_pass<2, true>(s, c, j, L, P, t); break;
      case 3: net_pass<3, true>(s, c, j, L, P, t); break;
      default: net_pass<4, true>(s, c, j, L, P, t); break;
    }
  } else {
    switch (t.nb) {
      case 1: net_pass<1, false>(s, c, j, L, P, t); break;
      case 2: net_pass<2, false>(s, c, j, L, P, t); break;
      case 3: net_pass<3, false>(s, c, j, L, P, t); break;
      default: net_pass<4, false>(s, c, j, L, P, t); break;
    }
  }
}

// ----------------------------------------------------------------- kernel
// Block = TB column tiles x L lanes per column x kTile columns.
// MODE 0: write agg (and lr when lr_out != nullptr).
// MODE 1: fused apply, params <- float32(params + lr * agg).
template <int MODE>
__global__ void orderstat_k(const double* __restrict__ U, int K, int lgP,
                            int L, int TB, long n, int lo, int hi,
                            double inv_cnt, int mode_rlr, double thresh,
                            double slr, double* __restrict__ out,
                            float* __restrict__ params,
                            double* __restrict__ lr_out) {
  extern __shared__ double smem[];
  const int P = 1 << lgP;
  const int c = threadIdx.x % kTile;
  const int j = (threadIdx.x / kTile) % L;
  const int sub = threadIdx.x / (kTile * L);
  double* s = smem + (long)sub * P * kTile;            // [TB][P][kTile]
  int* part = (int*)(smem + (long)TB * P * kTile)      // [TB][L][kTile]
              + sub * L * kTile;                       // partial votes
  const bool vote = (MODE == 1) ? (mode_rlr != 0) : (lr_out != nullptr);
  const long tiles = (n + kTile - 1) / kTile;

  // the trip count is uniform over the block: barriers inside
  for (long t0 = (long)blockIdx.x * TB; t0 < tiles;
       t0 += (long)gridDim.x * TB) {
    const long col = (t0 + sub) * kTile + c;
    const bool live = col < n;

    // coalesced tile load (a half-wave reads 256 contiguous bytes of a row)
    int v = 0;
    for (int k = j; k < P; k += L) {
      double u = INFINITY;
      if (k < K && live) {
        u = U[(long)k * n + col];
        v += (u > 0.0) ? 1 : (u < 0.0 ? -1 : 0);
      }
      s[k * kTile + c] = u;
    }
    if (vote) part[j * kTile + c] = v;
    __syncthreads();

    NetPass t = {0, 0, 0, false};
    while (net_next(lgP, t)) {
      net_pass_n(s, c, j, L, P, t);
      __syncthreads();
    }

    if (j == 0 && live) {
      double acc = 0.0;
      for (int r = lo; r < hi; ++r) acc += s[r * kTile + c];
      double agg = acc * inv_cnt;
      double lr = slr;
      if (vote) {
        int vs = 0;
        for (int l = 0; l < L; ++l) vs += part[l * kTile + c];
        lr = (fabs((double)vs) >= thresh) ? slr : -slr;
      }
      if (lr_out) lr_out[col] = lr;
      if (MODE == 0) {
        out[col] = agg;
      } else {
        params[col] = (float)((double)params[col] + lr * agg);
      }
    }
    __syncthreads();  // tile is overwritten by the next iteration's load
  }
}

template <int MODE>
static void launch_orderstat(const double* U, int K, long n, int lo, int hi,
                             double inv_cnt, int mode_rlr, double thresh,
                             double slr, double* out, float* params,
                             double* lr_out, hipStream_t st) {
  int lgP = 0;
  while ((1 << lgP) < K) ++lgP;
  int P = 1 << lgP;
  // one register group of 2^kPassBits rows per lane and pass where P allows;
  // small P: several tiles per block keep the block at 256 threads
  int L = P >> kPassBits;
  if (L < 1) L = 1;
  if (L > kOrderstatMaxLanes) L = kOrderstatMaxLanes;
  int TB = kBlock / (kTile * L);
  if (TB < 1) TB = 1;
  size_t lds = (size_t)TB * P * kTile * sizeof(double)
               + (size_t)TB * L * kTile * sizeof(int);
  if (lds > 64 * 1024) {
    HIP_CHECK(hipFuncSetAttribute(
        (const void*)orderstat_k<MODE>,
        hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  }
  long tiles = (n + kTile - 1) / kTile;
  orderstat_k<MODE><<<grid_for((tiles + TB - 1) / TB, 1), TB * L * kTile, lds,
                      st>>>(U, K, lgP, L, TB, n, lo, hi, inv_cnt, mode_rlr,
                            thresh, slr, out, params, lr_out);
}

// ------------------------------------------------------------- Bulyan
// Stage 2 of Bulyan (El Mhamdi et al., 2018) on the same network: the tile
// holds only the theta SELECTED rows, row i < theta of the tile being row
// perm[i] of U (perm: K distinct row indices, selected first), padded to
// P = pow2 >= theta with +inf.  The rows perm[theta..K) are read in the same
// load loop for their sign alone, so every element of U still comes from
// HBM once and the vote is over all K rows.  perm is staged in LDS once per
// block.  After the sort lane 0 of each column grows a window of beta
// values around the lower median s[m], m = (theta - 1) / 2, always taking
// the nearer neighbour and the LEFT one on a tie,
//     dl = med - s[l-1]  (+inf at l == 0)
//     dr = s[r+1] - med  (+inf at r == theta - 1)
//     dl <= dr ? --l : ++r                         beta - 1 times
// and reads off agg = (s[l] + ... + s[r]) * inv_beta, sequentially in
// ascending order.  Subtractions, comparisons, ordered adds and one
// multiply: bitwise the CPU rule.  (Lane 0 finds the window's left end by
// bisection over the same differences instead of stepping; see there.)  A perm entry outside [0, K) (the binding
// cannot see the values) is never dereferenced: its row reads as padding.
constexpr int kBulyanMaxK = 512;      // tile 128 KiB + votes 4 KiB + perm 2 KiB

template <int MODE>
__global__ void bulyan_k(const double* __restrict__ U,
                         const int* __restrict__ perm, int K, int theta,
                         int beta, int lgP, int L, int TB, long n,
                         double inv_beta, int mode_rlr, double thresh,
                         double slr, double* __restrict__ out,
                         float* __restrict__ params,
                         double* __restrict__ lr_out) {
  extern __shared__ double smem[];
  const int P = 1 << lgP;
  const int c = threadIdx.x % kTile;
  const int j = (threadIdx.x / kTile) % L;
  const int sub = threadIdx.x / (kTile * L);
  double* s = smem + (long)sub * P * kTile;            // [TB][P][kTile]
  int* part = (int*)(smem + (long)TB * P * kTile)      // [TB][L][kTile]
              + sub * L * kTile;                       // partial votes
  int* prm = (int*)(smem + (long)TB * P * kTile)       // [K], block-wide
             + TB * L * kTile;
  const bool vote = (MODE == 1) ? (mode_rlr != 0) : (lr_out != nullptr);
  const long tiles = (n + kTile - 1) / kTile;
  const int rows = K > P ? K : P;       // load trips: tile rows and sign rows

  for (int k = threadIdx.x; k < K; k += blockDim.x) prm[k] = perm[k];
  __syncthreads();

  // the trip count is uniform over the block: barriers inside
  for (long t0 = (long)blockIdx.x * TB; t0 < tiles;
       t0 += (long)gridDim.x * TB) {
    const long col = (t0 + sub) * kTile + c;
    const bool live = col < n;

    // coalesced tile load (a half-wave reads 256 contiguous bytes of a row)
    int v = 0;
    for (int k = j; k < rows; k += L) {
      double u = INFINITY;
      if (k < K && live) {
        const int row = prm[k];
        if ((unsigned)row < (unsigned)K) {
          const double x = U[(long)row * n + col];
          v += (x > 0.0) ? 1 : (x < 0.0 ? -1 : 0);
          if (k < theta) u = x;
        }
      }
      if (k < P) s[k * kTile + c] = u;
    }
    if (vote) part[j * kTile + c] = v;
    __syncthreads();

    NetPass t = {0, 0, 0, false};
    while (net_next(lgP, t)) {
      net_pass_n(s, c, j, L, P, t);
      __syncthreads();
    }

    if (j == 0 && live) {
      const int m = (theta - 1) / 2;
      const double med = s[m * kTile + c];
      // The window's beta - 1 steps merge the two ascending sequences
      // dl(a) = med - s[m-a] and dr(b) = s[m+b] - med (rounded differences
      // of a sorted column stay ordered), left first on a tie.  The a-th
      // left value is among the first beta - 1 merged iff fewer than
      // beta - a right values are strictly nearer, i.e. iff
      // dl(a) <= dr(beta - a); that is monotone in a, so the number of
      // left steps is found by bisection: ~log2(beta) dependent LDS reads
      // instead of beta - 1.  [lo, hi] keeps both ends inside the theta
      // rows whatever the data.
      int lo = beta - 1 - (theta - 1 - m);
      if (lo < 0) lo = 0;
      int hi = beta - 1 < m ? beta - 1 : m;
      while (lo < hi) {
        const int a = (lo + hi + 1) >> 1;     // lo < a <= hi <= m
        const double dl = med - s[(m - a) * kTile + c];
        const double dr = s[(m + beta - a) * kTile + c] - med;  // <= theta-1
        if (dl <= dr) lo = a; else hi = a - 1;
      }
      const int l = m - lo, r = l + beta - 1;
      double acc = 0.0;
      for (int i = l; i <= r; ++i) acc += s[i * kTile + c];
      double agg = acc * inv_beta;
      double lr = slr;
      if (vote) {
        int vs = 0;
        for (int q = 0; q < L; ++q) vs += part[q * kTile + c];
        lr = (fabs((double)vs) >= thresh) ? slr : -slr;
      }
      if (lr_out) lr_out[col] = lr;
      if (MODE == 0) {
        out[col] = agg;
      } else {
        params[col] = (float)((double)params[col] + lr * agg);
      }
    }
    __syncthreads();  // tile is overwritten by the next iteration's load
  }
}

// Block shapes as launch_orderstat's, sized by theta: the tile holds theta
// rows, whatever K is.
template <int MODE>
static void launch_bulyan(const double* U, const int* perm, int K, int theta,
                          int beta, long n, int mode_rlr, double thresh,
                          double slr, double* out, float* params,
                          double* lr_out, hipStream_t st) {
  int lgP = 0;
  while ((1 << lgP) < theta) ++lgP;
  int P = 1 << lgP;
  int L = P >> kPassBits;
  if (L < 1) L = 1;
  if (L > kOrderstatMaxLanes) L = kOrderstatMaxLanes;
  int TB = kBlock / (kTile * L);
  if (TB < 1) TB = 1;
  size_t lds = (size_t)TB * P * kTile * sizeof(double)
               + (size_t)TB * L * kTile * sizeof(int)
               + (size_t)K * sizeof(int);
  if (lds > 64 * 1024) {
    HIP_CHECK(hipFuncSetAttribute(
        (const void*)bulyan_k<MODE>,
        hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  }
  long tiles = (n + kTile - 1) / kTile;
  bulyan_k<MODE><<<grid_for((tiles + TB - 1) / TB, 1), TB * L * kTile, lds,
                   st>>>(U, perm, K, theta, beta, lgP, L, TB, n,
                         1.0 / (double)beta, mode_rlr, thresh, slr, out,
                         params, lr_out);
}

extern "C" {
int orderstat_max_k() { return kOrderstatMaxK; }

void launch_agg_orderstat(const double* U, int K, long n, int lo, int hi,
                          double inv_cnt, double* out,
                          double* lr_out /*nullable*/, double thresh,
                          double slr, void* s) {
  launch_orderstat<0>(U, K, n, lo, hi, inv_cnt, 0, thresh, slr, out, nullptr,
                      lr_out, (hipStream_t)s);
}

void launch_orderstat_rlr_apply(const double* U, int K, long n, int lo,
                                int hi, double inv_cnt, int mode_rlr,
                                double thresh, double slr, float* params,
                                double* lr_out /*nullable*/, void* s) {
  launch_orderstat<1>(U, K, n, lo, hi, inv_cnt, mode_rlr, thresh, slr,
                      nullptr, params, lr_out, (hipStream_t)s);
}

int bulyan_max_k() { return kBulyanMaxK; }

void launch_bulyan_trim(const double* U, const int* perm, int K, int theta,
                        int beta, long n, double* out,
                        double* lr_out /*nullable*/, double thresh,
                        double slr, void* s) {
  launch_bulyan<0>(U, perm, K, theta, beta, n, 0, thresh, slr, out, nullptr,
                   lr_out, (hipStream_t)s);
}

void launch_bulyan_rlr_apply(const double* U, const int* perm, int K,
                             int theta, int beta, long n, int mode_rlr,
                             double thresh, double slr, float* params,
                             double* lr_out /*nullable*/, void* s) {
  launch_bulyan<1>(U, perm, K, theta, beta, n, mode_rlr, thresh, slr,
                   nullptr, params, lr_out, (hipStream_t)s);
}
}
