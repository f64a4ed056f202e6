// The launcher ABI: every function that crosses a translation-unit
// boundary, declared once.  bindings.cpp (torch side) and every kernel
// .hip include this, so the compiler checks each definition against the
// declaration its callers see.  Plain C++: no HIP, no torch; streams are
// void*, bf16 is raw unsigned short.  The *_ws_floats / *_scratch_floats /
// *_ws_slabs / *_ws_doubles functions are host arithmetic only: the size of
// the workspace the launcher below them indexes.
#pragma once
#include <cstdint>

// A role: one small fold / permute / copy kernel of a training step, as
// data.  `kind` names its body (step_roles.h); the union member of that name
// holds the body's arguments, named and typed as the body reads them.  The
// body runs as the blocks of a (gx, gy) grid, count == gx * gy: alone
// (launch_step_role), or as blocks [first, first + count) of a batched
// launch, which assigns `first`.  The role makers below fill the rest.
struct ConvDbStage1Args {
  const float* dy; float* partials; long M; int Kout, chunks, K_blk;
};
struct ConvDbStage2Args { const float* partials; float* db; int Kout, chunks; };
struct SplitkPartialArgs {
  const float* ws; float* out; long n_out; int S, zstride;
};
struct SplitkReduceArgs {
  const float* ws; float* C; const float* bias; int M, N, ldc, SK, relu;
};
struct SplitkReduceDwpermArgs {
  const float* ws; float* dw; int Kout, C, RS, SK;
};
struct ConvSmallBwdwReduceArgs {
  const float* partials; float* dw; int KO, C, RS, chunks;
};
struct ColsumArgs { const float* dY; float* db; int M, N; };
struct FcHeadReduceArgs {
  const float *gl, *d2, *row_loss; float *dw, *db, *loss;
  int B, H, C, dw_blocks, db_blocks, dw_wave;
};
struct WpermArgs { const float* w; float* out; int Kout, C, RS; };
struct GatherRowsArgs {
  const uint32_t* src; const long* sel; uint32_t* dst; long rows;
  int row_words, vec, src_rows;
};
struct AddU64Args { unsigned long long* p; unsigned long long delta; };
enum StepRoleKind {
  kRoleConvDbStage1 = 0,
  kRoleConvDbStage2,
  kRoleSplitkPartial,
  kRoleSplitkReduce,
  kRoleSplitkReduceDwperm,
  kRoleConvSmallBwdwReduce,
  kRoleColsum,
  kRoleFcHeadReduce,
  kRoleWpermRscKo,
  kRoleWpermRskoC,
  kRoleGatherRows,
  kRoleAddU64,
  kStepRoleKinds,
};
struct StepRole {
  int kind;
  int first;
  int count;
  int gx, gy;
  union {
    ConvDbStage1Args conv_db_stage1;
    ConvDbStage2Args conv_db_stage2;
    SplitkPartialArgs splitk_partial;
    SplitkReduceArgs splitk_reduce;
    SplitkReduceDwpermArgs splitk_reduce_dwperm;
    ConvSmallBwdwReduceArgs conv_small_bwdw_reduce;
    ColsumArgs colsum;
    FcHeadReduceArgs fc_head_reduce;
    WpermArgs wperm;  // both wperm kinds
    GatherRowsArgs gather_rows;
    AddU64Args add_u64;
  };
};
static_assert(sizeof(StepRole) <= 104, "16 of them are kernel arguments");
constexpr int kStepMaxRoles = 16;

// How the x-resident fp32 conv forward cuts one image: `tiles` blocks of
// mi * 32 output pixels (mi MFMA row-tiles per wave), each holding lds_rows
// input rows in lds_bytes of LDS.  tile_rows is the tile in output rows, 0
// where it is not a whole number of them.
struct ConvFwdResPlan {
  int tile_rows, tiles, mi, lds_rows;
  long lds_bytes;
};

extern "C" {
// step_batch.hip.  launch_step_role runs one role now, launch_step_batch up
// to kStepMaxRoles in one launch; both skip roles with count == 0 and return
// 0, or -1 (nothing launched) for an unknown kind or too many roles.
// step_batch_plan (host only): first[r] = blocks before r; returns the total.
int launch_step_role(const StepRole* r, void* s);
int step_batch_max_roles();
int step_batch_plan(const int* counts, int n, int* first);
int step_batch_lookup(const int* counts, int n, int block, int* vblock);
int launch_step_batch(const StepRole* roles, int n, void* s);
StepRole step_role_gather_rows(const void* src, const long* sel, void* dst,
                               long rows, int row_words, int src_rows);
StepRole step_role_add_u64(unsigned long long* p, unsigned long long delta);
// elementwise.hip
void launch_relu_fwd(const float* x, float* y, long n, void* s);
void launch_relu_bwd(const float* y, const float* dy, float* dx, long n,
                     void* s);
void launch_add_relu(const float* a, const float* b, float* y, long n,
                     void* s);
void launch_add_relu_bwd(float* a, const float* b, const float* y, long n,
                         void* s);
void launch_add_relu_bwd_bf16(unsigned short* a, const unsigned short* b,
                              const unsigned short* y, long n, void* s);
void launch_add_inplace(float* a, const float* b, long n, void* s);
void launch_add_inplace_bf16(unsigned short* a, const unsigned short* b,
                             long n, void* s);
void launch_maxpool2x2_fwd(const float* x, float* y, uint8_t* idx, long B,
                           int H, int W, int OH, int OW, int C, void* s);
void launch_maxpool2x2_bwd(const float* dy, const uint8_t* idx, float* dx,
                           long B, int H, int W, int OH, int OW, int C,
                           void* s);
void launch_maxpool2x2_bwd_relu(const float* dy, const uint8_t* idx,
                                const float* relu_pooled, float* dx, long B,
                                int H, int W, int OH, int OW, int C,
                                void* s);
void launch_maxpool2x2_fwd_bf16(const unsigned short* x, unsigned short* y,
                                uint8_t* idx, long B, int H, int W, int OH,
                                int OW, int C, void* s);
void launch_maxpool2x2_bwd_bf16(const unsigned short* dy,
                                const uint8_t* idx, unsigned short* dx,
                                long B, int H, int W, int OH, int OW, int C,
                                void* s);
void launch_gap_fwd(const float* x, float* y, long B, int HW, int C,
                    void* s);
void launch_gap_bwd(const float* dy, float* dx, long B, int HW, int C,
                    void* s);
void launch_gap_bwd_relu(const float* dy, const float* y, float* dx, long B,
                         int HW, int C, void* s);
void launch_dropout_fwd(const float* x, float* y, uint8_t* mask, long n,
                        float p, uint64_t seed, uint64_t offset, void* s);
void launch_dropout_fwd_dev(const float* x, float* y, uint8_t* mask, long n,
                            float p, const unsigned long long* state,
                            int site, void* s);
void launch_dropout_bwd(const float* dy, const uint8_t* mask, float* dx,
                        long n, float p, void* s);
void launch_dropout_relu_bwd(const float* dy, const uint8_t* mask,
                             const float* y, float* dx, long n, float p,
                             void* s);
void launch_ce_fwd(const float* logits, const long* labels, float* softmax,
                   float* row_loss, float* loss_out, int B, int C, void* s);
void launch_ce_bwd(const float* softmax, const long* labels,
                   const float* dloss, float* dlogits, int B, int C,
                   void* s);
void launch_eval_update(const float* logits, const long* labels, float* conf,
                        double* loss_sum, int B, int C, int num_classes,
                        void* s);
void launch_nhwc_flatten(const float* in, float* out, long B, int C, int H,
                         int W, void* s);
void launch_nhwc_unflatten(const float* in, float* out, long B, int C,
                           int H, int W, void* s);
// elementwise.hip, bf16
void launch_relu_fwd_bf16(const unsigned short* x, unsigned short* y,
                          long n, void* s);
void launch_relu_bwd_bf16(const unsigned short* y, const unsigned short* dy,
                          unsigned short* dx, long n, void* s);
void launch_add_relu_bf16(const unsigned short* a, const unsigned short* b,
                          unsigned short* y, long n, void* s);
void launch_dropout_fwd_dev_bf16(const unsigned short* x, unsigned short* y,
                                 uint8_t* mask, long n, float p,
                                 const unsigned long long* state, int site,
                                 void* s);
void launch_dropout_bwd_bf16(const unsigned short* dy, const uint8_t* mask,
                             unsigned short* dx, long n, float p, void* s);
void launch_gap_fwd_bf16(const unsigned short* x, unsigned short* y, long B,
                         int HW, int C, void* s);
void launch_gap_bwd_bf16(const unsigned short* dy, unsigned short* dx,
                         long B, int HW, int C, void* s);
void launch_gap_bwd_relu_bf16(const unsigned short* dy,
                              const unsigned short* y, unsigned short* dx,
                              long B, int HW, int C, void* s);
void launch_nhwc_flatten_bf16(const unsigned short* in, unsigned short* out,
                              long B, int C, int H, int W, void* s);
void launch_nhwc_unflatten_bf16(const unsigned short* in,
                                unsigned short* out, long B, int C, int H,
                                int W, void* s);
// fused_tail.hip (fp32).  The seam between the conv trunk and the first
// fc layer: x (B,H,W,C) NHWC -> pooled / idx (B,H/2,W/2,C) NHWC and the
// dropped flat-CHW rows d / mask (B, C*(H/2)*(W/2)), and its backward.
// Both need pool_seam_fused_ok(C, H, W): C % 4 == 0 and the pooled image
// fits the kernels' static LDS tile.
int pool_seam_fused_ok(int C, int H, int W);
void launch_pool_flatten_dropout_fwd(const float* x, float* pooled,
                                     uint8_t* idx, float* d, uint8_t* mask,
                                     long B, int H, int W, int C, float p,
                                     const unsigned long long* state,
                                     int site, void* s);
// the same kernel from an already pooled image (B,OH,OW,C), as
// launch_conv_pool_fwd leaves it: writes d / mask only; needs
// pool_seam_fused_ok(C, 2 * OH, 2 * OW)
void launch_flatten_dropout_fwd(const float* pooled, float* d, uint8_t* mask,
                                long B, int OH, int OW, int C, float p,
                                const unsigned long long* state, int site,
                                void* s);
void launch_dropout_unflatten_pool_bwd_relu(const float* g,
                                            const uint8_t* mask,
                                            const uint8_t* idx,
                                            const float* pooled, float* dx,
                                            long B, int H, int W, int C,
                                            float p, void* s);
// The classifier head on h1 (B,H), w (C,H), bias (C): dropout, fc, CE
// forward and backward: stage A (per row) launched, stage B (over the batch)
// a role over the ws (fc_head_ws_floats(B, H, C) floats) that A filled.
// fc_head_fused_ok(B, H, C): C <= 64 and the three fc GEMMs all take
// launch_gemm_f32_main's tiny-problem branch.
int fc_head_fused_ok(int B, int H, int C);
long fc_head_ws_floats(int B, int H, int C);
void launch_fc_head_rows(const float* h1, const float* w, const float* bias,
                         const long* labels, const float* dloss, float* ws,
                         float* g_h1, int B, int H, int C, float p,
                         const unsigned long long* state, int site,
                         void* s);
StepRole fc_head_reduce_role(const float* ws, float* dw, float* db,
                             float* loss, int B, int H, int C);
// flatopt.hip
long flat_norm_scratch_floats();
void launch_clipped_sgd(float* p, const float* g, float* v, float* scratch,
                        float lr, float mu, float max_norm, long n, void* s);
void launch_pgd_project(float* p, const float* t0, float* scratch, float clip,
                        long n, void* s);
void launch_delta64(const float* p, const double* t0, double* out, long n,
                    void* s);
void launch_gather_grads(const float* const* srcs, const long* offs,
                         const long* lens, int count, float* flat, void* s);
// aggregation.hip
void launch_fused_avg_rlr_apply(const double* U, const double* w, int K,
                                long n, double inv_wsum, int mode_rlr,
                                double thresh, double slr, float* params,
                                double* lr_out, double noise_std,
                                uint64_t seed, uint64_t offset, void* s);
void launch_rlr_vote(const double* U, int K, long n, double thresh,
                     double slr, double* lr, void* s);
void launch_agg_avg(const double* U, const double* w, int K, long n,
                    double inv_wsum, double* out, void* s);
void launch_agg_sign(const double* U, int K, long n, double* out, void* s);
void launch_agg_comed(const double* U, int K, long n, double* out, void* s);
void launch_apply_update(float* params, const double* agg, const double* lr,
                         double slr, long n, void* s);
// orderstat.hip (lr_out is nullable)
int orderstat_max_k();
void launch_agg_orderstat(const double* U, int K, long n, int lo, int hi,
                          double inv_cnt, double* out, double* lr_out,
                          double thresh, double slr, void* s);
void launch_orderstat_rlr_apply(const double* U, int K, long n, int lo,
                                int hi, double inv_cnt, int mode_rlr,
                                double thresh, double slr, float* params,
                                double* lr_out, void* s);
// Bulyan's trimmed mean around the median of the rows perm[0..theta) of U,
// vote over all K rows; perm: K distinct row indices on the device,
// 1 <= beta <= theta <= K <= bulyan_max_k() (lr_out is nullable)
int bulyan_max_k();
void launch_bulyan_trim(const double* U, const int* perm, int K, int theta,
                        int beta, long n, double* out, double* lr_out,
                        double thresh, double slr, void* s);
void launch_bulyan_rlr_apply(const double* U, const int* perm, int K,
                             int theta, int beta, long n, int mode_rlr,
                             double thresh, double slr, float* params,
                             double* lr_out, void* s);
// pairdist.hip: D (K, K) = squared L2 distances between the rows of U
// (K, n), 1 <= K <= pairdist_max_k().  Stage 1 splits n into
// pairdist_chunks(K, n) chunks (a pure function of K and n) and writes one
// 64 x 64 slab per (chunk, upper-triangle pair of 64-row tiles) to ws, or
// one 16 x 16 slab per chunk when K <= 16, and the reduced slabs behind
// them; chunks * pairs <= 1024 and pairs <= 36, so ws is at most 1060 slabs
// of 32 KiB < 34 MiB (bound: <= 64 MiB) for every K <= 512 and every n.
int pairdist_max_k();
int pairdist_chunks(int K, long n);
long pairdist_ws_doubles(int K, long n);
void launch_pairwise_sqdist(const double* U, int K, long n, double* ws,
                            double* D, void* s);
// The same stages 1 and 2 over the rows rows[0..K) of H (any number of rows,
// n columns): G (K, K), G[i][j] = <H[rows[i]], H[rows[j]]>, exactly
// symmetric.  rows: K int64 on the device, every entry a valid row of H (the
// caller checks; the kernel dereferences them as given).  Same chunking and
// workspace as launch_pairwise_sqdist.
void launch_gram_rows(const double* H, const long* rows, int K, long n,
                      double* ws, double* G, void* s);
// foolsgold.hip.  launch_rows_add: H[rows[k]][j] += U[k][j] for the K
// DISTINCT valid rows rows[0..K) of H (int64 on the device), any K >= 1.
// launch_foolsgold_weights: FoolsGold's weights from the Gram matrix G (K, K)
// of the sampled history rows, 1 <= K <= foolsgold_max_k(): cs (K, K) the
// cosine matrix with a zero diagonal (before pardoning), alpha (K) the
// learning-rate weights in [0, 1].  Three small launches, no host
// synchronisation, no workspace: alpha and the diagonal of cs carry the row
// maxima between the launches.
int foolsgold_max_k();
void launch_rows_add(double* H, const long* rows, const double* U, int K,
                     long n, void* s);
void launch_foolsgold_weights(const double* G, int K, double kappa,
                              double* cs, double* alpha, void* s);
// geomed.hip: smoothed Weiszfeld iterations for the geometric median of the
// rows of U (K, n), 1 <= K <= geomed_max_k().  Stage 1 splits n into
// geomed_chunks(K, n) <= 512 chunks (a pure function of K and n) and writes
// one partial squared distance per (chunk, k) to ws[chunk][K]; 1 / sum a
// lives behind the partials.  launch_geomed_sqdist: d2[k] = ||U_k - z||^2
// for the weighted mean z under a caller-given a (K).
// launch_geomed_weights: a = ones, then iters x (distances, a = 1 / max(nu,
// sqrt(d2))) with no host synchronisation; d2 = the last distances (zeros
// for iters == 0).
int geomed_max_k();
int geomed_chunks(int K, long n);
long geomed_ws_doubles(int K, long n);
void launch_geomed_sqdist(const double* U, const double* a, int K, long n,
                          double* ws, double* d2, void* s);
void launch_geomed_weights(const double* U, int K, long n, int iters,
                           double nu, double* ws, double* a, double* d2,
                           void* s);
// rowclip.hip: L2 norms of the rows of U (K, n) and the server-side clip
// U[k] *= s[k], s[k] = norm[k] > tau ? tau / norm[k] : 1, for any K >= 1.
// Stage 1 splits n into rownorm_chunks(K, n) chunks (a pure function of K
// and n) and writes one partial sum of squares per (chunk, k) to
// ws[chunk][K].  launch_rownorm_partials is stage 1 alone, launch_row_norms
// adds the one-block reduction to norm (K).  launch_rowclip: tau = value
// (median_mode == 0) or value * the lower median of the norms; writes norm
// (K), scale (K) and *tau, then scales U in place; no host synchronisation.
int rownorm_chunks(int K, long n);
long rownorm_ws_doubles(int K, long n);
void launch_rownorm_partials(const double* U, int K, long n, double* ws,
                             void* s);
void launch_row_norms(const double* U, int K, long n, double* ws,
                      double* norm, void* s);
void launch_rowclip(double* U, int K, long n, double value, int median_mode,
                    double* ws, double* norm, double* scale, double* tau,
                    void* s);
// gemm_f32.hip
int gemm_f32_splitk(int M, int N, int K);
long gemm_splitk_ws_floats(int M, int N, int SK);
// K-tiles per chunk (3..5) when launch_gemm_f32_main runs the short-K form
// of the tile kernel for this call at split depth SK, else 0
int gemm_f32_shortk_tiles(int M, int N, int K, int SK, int lda, int ldb);
// the GEMM without its split-K combine: returns 1 when ws holds SK partial
// slabs that still have to be folded into C, 0 when C is complete
int launch_gemm_f32_main(const float* A, const float* B, float* C,
                         const float* bias, float* ws, int M, int N, int K,
                         int lda, int ldb, int ldc, int SK, int relu,
                         int layout, void* s);
// the split-K combine as roles: the number of levels filled, 0 for the wave
// form, which has no role.  launch_splitk_reduce: the combine now, any form.
int splitk_reduce_roles(const float* ws, float* C, const float* bias, int M,
                        int N, int ldc, int SK, int relu, StepRole* l1,
                        StepRole* l2);
void launch_splitk_reduce(const float* ws, float* C, const float* bias,
                          int M, int N, int ldc, int SK, int relu, void* s);
StepRole splitk_partial_role(const float* ws, float* out, long n_out, int S,
                             int zstride);
StepRole colsum_role(const float* dY, float* db, int M, int N);
// gemm_bf16.hip
void launch_gemm_bf16(const unsigned short* A, const unsigned short* B,
                      float* C, const float* bias, unsigned short* C16,
                      float* ws, int M, int N, int K, int lda, int ldb,
                      int ldc, int SK, int relu, void* s);
// conv_f32.hip
void launch_conv_fwd(const float* x, const float* wt, const float* bias,
                     float* y, int Nb, int C, int H, int W, int Kout, int R,
                     int S, int OH, int OW, int stride, int pad, int relu,
                     void* s);
// The resident forward's tile plan (host only, a pure function of the
// shape): a tile of whole output rows with no padded MFMA row, 192 pixels
// at most, where one exists within the LDS that keeps 3 blocks on a CU;
// 128 pixels wherever they fall otherwise.
ConvFwdResPlan conv_fwd_res_plan(int C, int H, int W, int OH, int OW, int R);
// conv + bias + relu + maxpool2x2 in the resident forward's epilogue:
// pooled / idx (Nb, OH/2, OW/2, Kout) NHWC as launch_maxpool2x2_fwd writes
// them; the conv output itself is never stored.  conv_pool_fused_ok: the
// resident path applies, OH and OW are even and the planned tile is a whole
// even number of output rows.
int conv_pool_fused_ok(int C, int H, int W, int Kout, int R, int S,
                       int stride, int pad);
void launch_conv_pool_fwd(const float* x, const float* wt, const float* bias,
                          float* pooled, uint8_t* idx, int Nb, int C, int H,
                          int W, int Kout, int R, int S, void* s);
void launch_conv_bwd_data_relu(const float* dy, const float* wp,
                               float* dx, const float* relu_y, int Nb,
                               int C, int H, int W, int Kout, int R, int S,
                               int OH, int OW, int stride, int pad,
                               void* s);
int conv_bwd_weight_splitk(int Kout, int Ncrs, long Kdim);
long conv_bwd_weight_ws_floats(int Kout, int Ncrs, int SK);
// launch_conv_bwd_weight = main kernels + the combine roles (1 or 2 levels)
// over ws; a small layer's ws: conv_small_bwdw_chunks(Nb*OH*OW) chunk slabs
int conv_small_bwdw_chunks(long Kdim);
void launch_conv_bwd_weight(const float* dy, const float* x, float* dw,
                            float* ws, int SK, int Nb, int C, int H, int W,
                            int Kout, int R, int S, int OH, int OW,
                            int stride, int pad, void* s);
void launch_conv_bwd_weight_main(const float* dy, const float* x, float* ws,
                                 int SK, int Nb, int C, int H, int W,
                                 int Kout, int R, int S, int OH, int OW,
                                 int stride, int pad, void* s);
int conv_bwd_weight_combine_roles(float* ws, float* dw, int SK, int Nb,
                                  int C, int Kout, int R, int S, int OH,
                                  int OW, StepRole* l1, StepRole* l2);
int splitk_reduce_dwperm_roles(const float* ws, float* dw, int Kout, int C,
                               int RS, int SK, StepRole* l1, StepRole* l2);
void conv_db_roles(const float* dy, float* db, float* partials, int Nb,
                   int Kout, int OHW, StepRole* l1, StepRole* l2);
StepRole wperm_role(int kind, const float* w, float* out, int Kout, int C,
                    int RS);
int conv_db_chunks(long M, int Kout);
long conv_db_ws_floats(int Kout);
long conv_dwperm_ws_floats(int Kout, int Ncrs, int SK);
// conv_bf16.hip
int conv_bwd_weight_bf16_splitk(int Kout, int Ncrs, long Kdim);
void launch_conv_fwd_bf16(const unsigned short* x, const unsigned short* wt,
                          const float* bias, unsigned short* y, int Nb,
                          int C, int H, int W, int Kout, int R, int S,
                          int OH, int OW, int stride, int pad, int relu,
                          void* s);
void launch_conv_bwd_data_bf16_relu(const unsigned short* dy,
                                    const unsigned short* wp,
                                    unsigned short* dx,
                                    const unsigned short* relu_y, int Nb,
                                    int C, int H, int W, int Kout, int R,
                                    int S, int OH, int OW, int stride,
                                    int pad, void* s);
void launch_conv_bwd_weight_bf16(const unsigned short* dy,
                                 const unsigned short* x, float* dw,
                                 float* ws, int SK, int Nb, int C, int H,
                                 int W, int Kout, int R, int S, int OH,
                                 int OW, int stride, int pad, void* s);
void launch_wperm_rsc_ko_bf16(const float* w, unsigned short* out, int Kout,
                              int C, int RS, void* s);
void launch_wperm_rsko_c_bf16(const float* w, unsigned short* out, int Kout,
                              int C, int RS, void* s);
void launch_conv_db_bf16(const unsigned short* dy, float* db,
                         float* partials, int Nb, int Kout, int OHW,
                         void* s);
// conv_bwdw_tap.hip
int conv_bwdw_tap_ok(int C, int H, int W, int Kout, int R, int S,
                     int stride, int pad);
int conv_bwdw_tap_s2_ok(int C, int H, int W, int Kout, int R, int S,
                        int stride, int pad);
int conv_bwdw_tap_ws_slabs(int Nb, int C, int Kout, int* S_out, int* G_out,
                           int* chunks_out);
void launch_conv_bwdw_tap_bf16(const unsigned short* dy,
                               const unsigned short* x, float* dw,
                               float* ws, int Nb, int C, int H, int W,
                               int Kout, void* st);
void launch_conv_bwdw_tap_s2_bf16(const unsigned short* dy,
                                  const unsigned short* x, float* dw,
                                  float* ws, int Nb, int C, int H, int W,
                                  int Kout, void* st);
int conv_tap_fwd_ok(int Cin, int H, int W, int Cout, int R, int S,
                    int stride, int pad);
void launch_conv_tap_fwd_bf16(const unsigned short* x,
                              const unsigned short* wt, const float* bias,
                              unsigned short* y,
                              const unsigned short* relu_y, int Nb,
                              int Cin, int H, int W, int Cout, int relu,
                              int flip, void* st);
int conv_tap_fwd_w4_ok(int Cin, int H, int W, int Cout, int R, int S,
                       int stride, int pad);
void launch_conv_tap_fwd_w4_bf16(const unsigned short* x,
                                 const unsigned short* wt,
                                 const float* bias, unsigned short* y,
                                 const unsigned short* relu_y, int Nb,
                                 int Cin, int Cout, int relu, int flip,
                                 void* st);
int conv_tap_bwdd_s2_ok(int C, int H, int W, int KO, int R, int S,
                        int stride, int pad);
void launch_conv_tap_bwdd_s2_bf16(const unsigned short* dy,
                                  const unsigned short* wp,
                                  unsigned short* dx,
                                  const unsigned short* relu_y, int Nb,
                                  int KO, int H, int W, int C, void* st);
// batchnorm.hip
int bn_scratch_floats(int C);
void launch_bn_fwd(const float* x, const float* w, const float* b,
                   float* running_mean, float* running_var, float* save_mean,
                   float* save_rstd, float* y, float* scratch, int Nb,
                   int C, int HW, float momentum, float eps, int training,
                   int relu, void* s);
void launch_bn_fwd_bf16(const unsigned short* x, const float* w,
                        const float* b, float* running_mean,
                        float* running_var, float* save_mean,
                        float* save_rstd, unsigned short* y, float* scratch,
                        int Nb, int C, int HW, float momentum, float eps,
                        int training, int relu, void* s);
void launch_bn_bwd(const float* x, const float* dy, const float* w,
                   const float* save_mean, const float* save_rstd,
                   float* scratch, float* dx, float* dw, float* db, int Nb,
                   int C, int HW, int training, void* s);
void launch_bn_bwd_bf16(const unsigned short* x, const unsigned short* dy,
                        const float* w, const float* save_mean,
                        const float* save_rstd, float* scratch,
                        unsigned short* dx, float* dw, float* db, int Nb,
                        int C, int HW, int training, void* s);
// poison.hip
void launch_poison_set_u8(uint8_t* data, const long* idxs, int B,
                          const int* coords, int P, int H, int W, int C,
                          int value, void* s);
void launch_poison_set_f32(float* data, const long* idxs, int B,
                           const int* coords, int P, int H, int W,
                           float value, void* s);
void launch_poison_addwrap_u8(uint8_t* data, const long* idxs, int B,
                              const uint8_t* mask, int HW, void* s);
void launch_poison_subf(float* data, const long* idxs, int B,
                        const uint8_t* mask, int HW, void* s);
void launch_normalize_u8(const uint8_t* raw, float* out, long B, int H,
                         int W, int C, const float* mean, const float* stdv,
                         void* s);
// conv_bf16.hip (the variant sweep of tests/perf/bwdw_micro.hip)
void launch_conv_bwd_weight_bf16_ex(const unsigned short* dy,
                                    const unsigned short* x, float* dw,
                                    float* ws, int SK, int variant, int Nb,
                                    int C, int H, int W, int Kout, int R,
                                    int S, int OH, int OW, int stride,
                                    int pad, void* s);
}
