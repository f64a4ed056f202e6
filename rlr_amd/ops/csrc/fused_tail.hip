// Fused tail of the CNN training step (gfx950, fp32): the launch-latency
// bound kernels after the conv trunk, merged without changing one bit of
// the result.
//
//   pool_flatten_dropout_fwd_k        = maxpool2x2_fwd_k + batch_transpose_k
//                                       + dropout_fwd_dev_k
//   dropout_unflatten_pool_bwd_relu_k = dropout_bwd_k + batch_transpose_k
//                                       + maxpool2x2_bwd_gather4_k
//   fc_head_rows_k + fc_head_reduce   = dropout fwd, last-fc fwd, CE fwd,
//                                       loss mean, CE bwd, last-fc dx / dW /
//                                       db, dropout+relu bwd (9 launches)
//
// (fc_head_reduce is a role: its body is in step_roles.h.)
//
// Every output is computed by the tail_math.h function the unfused kernel
// calls, on the same operands in the same order; what a kernel boundary
// rounded to a float is still one float here.  No atomics, no grid sync.
#include "common.h"
#include "launchers.h"
#include "tail_math.h"

// ============================================================ the seam
// One block per image.  The pooled image lives in LDS as tile[hw][c] with
// a row of C + 1 floats: the NHWC side walks c (stride 1) and the flat CHW
// side walks hw (stride C + 1, odd), so both are spread over the banks.
constexpr int kSeamBlock = 512;
constexpr int kSeamTileFloats = 9600;  // 37.5 KiB: 144 x 65 (MNIST) fits

// The CHW side moves aligned groups of 4 flat elements per thread (one
// philox draw, float4 global access).  Their LDS addresses are 4 rows
// apart from lane to lane, which would hit 8 banks only; thread t
// therefore visits its 4 elements rotated by (t >> 3) & 3, which spreads
// 32 lanes over 32 banks.  rot_fwd gives w[s] = v[(s + r) & 3], rot_inv
// undoes it; both are selects, not indexed arrays (no scratch).
__device__ __forceinline__ void rot_fwd(float (&v)[4], int r) {
  float a = v[0], b = v[1], c = v[2], d = v[3];
  if (r & 1) { float t = a; a = b; b = c; c = d; d = t; }
  if (r & 2) { float t = a; a = c; c = t; t = b; b = d; d = t; }
  v[0] = a; v[1] = b; v[2] = c; v[3] = d;
}
__device__ __forceinline__ void rot_inv(float (&v)[4], int r) {
  float a = v[0], b = v[1], c = v[2], d = v[3];
  if (r & 1) { float t = d; d = c; c = b; b = a; a = t; }
  if (r & 2) { float t = a; a = c; c = t; t = b; b = d; d = t; }
  v[0] = a; v[1] = b; v[2] = c; v[3] = d;
}

// tile address of the flat per-image CHW element q0 + e (q0 = c0*OHW + hw0)
__device__ __forceinline__ int seam_tile_addr(int c0, int hw0, int e,
                                              int OHW, int S) {
  int c = c0, hw = hw0 + e;
  while (hw >= OHW) { hw -= OHW; ++c; }
  return hw * S + c;
}

// POOLED_IN: x is already the pooled image (conv_fwd_res_k's pooled
// epilogue wrote it, and idx): the first phase only copies it into the tile.
template <bool POOLED_IN>
__global__ __launch_bounds__(kSeamBlock)
void pool_flatten_dropout_fwd_k(const float* __restrict__ x,
                                float* __restrict__ pooled,
                                uint8_t* __restrict__ idx,
                                float* __restrict__ d,
                                uint8_t* __restrict__ mask, int H, int W,
                                int OH, int OW, int C, float p,
                                const unsigned long long* __restrict__ state,
                                int site) {
  __shared__ float tile[kSeamTileFloats];
  const long b = blockIdx.x;
  const int OHW = OH * OW, S = C + 1, c4n = C / 4;
  const int n4 = OHW * c4n;  // float4 items of one pooled image
  const int WC = W * C;
  const float* xb = x + b * (long)H * W * C;
  const long ob = b * (long)OHW * C;  // C % 4 == 0: a multiple of 4

  // NHWC side: 4 channels of one pooled pixel per thread
#pragma unroll 2
  for (int it = threadIdx.x; it < n4; it += kSeamBlock) {
    int ohw = it / c4n;
    int c = (it - ohw * c4n) * 4;
    float4 m;
    if (POOLED_IN) {
      m = *(const float4*)(x + ob + (long)it * 4);
    } else {
      int oh = ohw / OW, ow = ohw - oh * OW;
      const float* p0 = xb + ((long)(2 * oh) * W + 2 * ow) * C + c;
      float4 v00 = *(const float4*)p0;
      float4 v01 = *(const float4*)(p0 + C);
      float4 v10 = *(const float4*)(p0 + WC);
      float4 v11 = *(const float4*)(p0 + WC + C);
      uchar4 a;
      pool2x2_select(v00.x, v01.x, v10.x, v11.x, m.x, a.x);
      pool2x2_select(v00.y, v01.y, v10.y, v11.y, m.y, a.y);
      pool2x2_select(v00.z, v01.z, v10.z, v11.z, m.z, a.z);
      pool2x2_select(v00.w, v01.w, v10.w, v11.w, m.w, a.w);
      *(float4*)(pooled + ob + (long)it * 4) = m;
      *(uchar4*)(idx + ob + (long)it * 4) = a;
    }
    float* t = tile + ohw * S + c;
    t[0] = m.x; t[1] = m.y; t[2] = m.z; t[3] = m.w;
  }
  __syncthreads();

  // flat CHW side: dropout on the flat index ob + q, 4 elements per draw
  const uint64_t seed = state[0];
  const uint64_t offset = state[1] + site;
  const float scale = dropout_scale(p);
  const int rot = (threadIdx.x >> 3) & 3;
  const long gb = ob / 4;
  for (int g = threadIdx.x; g < n4; g += kSeamBlock) {
    Philox4 r = philox4(seed, offset, (uint32_t)(gb + g));
    int q0 = g * 4;
    int c0 = q0 / OHW, hw0 = q0 - c0 * OHW;
    float v[4];
#pragma unroll
    for (int s = 0; s < 4; ++s)
      v[s] = tile[seam_tile_addr(c0, hw0, (s + rot) & 3, OHW, S)];
    rot_inv(v, rot);
    bool k0 = dropout_keep(r.x, p), k1 = dropout_keep(r.y, p),
         k2 = dropout_keep(r.z, p), k3 = dropout_keep(r.w, p);
    float4 y;
    y.x = dropout_apply(k0, v[0], scale);
    y.y = dropout_apply(k1, v[1], scale);
    y.z = dropout_apply(k2, v[2], scale);
    y.w = dropout_apply(k3, v[3], scale);
    uchar4 mk;
    mk.x = k0; mk.y = k1; mk.z = k2; mk.w = k3;
    *(float4*)(d + ob + q0) = y;
    *(uchar4*)(mask + ob + q0) = mk;
  }
}

__global__ __launch_bounds__(kSeamBlock)
void dropout_unflatten_pool_bwd_relu_k(const float* __restrict__ g,
                                       const uint8_t* __restrict__ mask,
                                       const uint8_t* __restrict__ idx,
                                       const float* __restrict__ pooled,
                                       float* __restrict__ dx, int H, int W,
                                       int OH, int OW, int C, float p) {
  __shared__ float tile[kSeamTileFloats];
  const long b = blockIdx.x;
  const int OHW = OH * OW, S = C + 1, c4n = C / 4;
  const int n4 = OHW * c4n;
  const long ob = b * (long)OHW * C;
  const float scale = dropout_scale(p);
  const int rot = (threadIdx.x >> 3) & 3;

  // flat CHW side: dropout backward, transposed into the tile
#pragma unroll 2
  for (int grp = threadIdx.x; grp < n4; grp += kSeamBlock) {
    int q0 = grp * 4;
    float4 gv = *(const float4*)(g + ob + q0);
    uchar4 mk = *(const uchar4*)(mask + ob + q0);
    float v[4];
    v[0] = dropout_apply(mk.x, gv.x, scale);
    v[1] = dropout_apply(mk.y, gv.y, scale);
    v[2] = dropout_apply(mk.z, gv.z, scale);
    v[3] = dropout_apply(mk.w, gv.w, scale);
    rot_fwd(v, rot);
    int c0 = q0 / OHW, hw0 = q0 - c0 * OHW;
#pragma unroll
    for (int s = 0; s < 4; ++s)
      tile[seam_tile_addr(c0, hw0, (s + rot) & 3, OHW, S)] = v[s];
  }
  __syncthreads();

  // NHWC side: 4 channels of one INPUT pixel per thread, written once;
  // odd tail rows / columns lie outside every window and get zeros
  const int nin4 = H * W * c4n;
  float* dxb = dx + b * (long)H * W * C;
#pragma unroll 2
  for (int it = threadIdx.x; it < nin4; it += kSeamBlock) {
    int pos = it / c4n;
    int c = (it - pos * c4n) * 4;
    int ih = pos / W, iw = pos - ih * W;
    int oh = ih >> 1, ow = iw >> 1;
    float4 o = {0.f, 0.f, 0.f, 0.f};
    if (oh < OH && ow < OW) {
      int ohw = oh * OW + ow;
      long off = ob + (long)ohw * C + c;
      uchar4 ap = *(const uchar4*)(idx + off);
      float4 p4 = *(const float4*)(pooled + off);
      const float* t = tile + ohw * S + c;
      uint8_t a = ((ih & 1) << 1) | (iw & 1);
      o.x = relu_gate(p4.x, pool_bwd_pick(ap.x, a, t[0]));
      o.y = relu_gate(p4.y, pool_bwd_pick(ap.y, a, t[1]));
      o.z = relu_gate(p4.z, pool_bwd_pick(ap.z, a, t[2]));
      o.w = relu_gate(p4.w, pool_bwd_pick(ap.w, a, t[3]));
    }
    *(float4*)(dxb + (long)it * 4) = o;
  }
}

// ============================================================ the head
// Stage A: one wave per batch row.  Lane j + 64 t owns element j + 64 t of
// the row; lane c owns logit c (C <= 64).  The dropped activations go to
// the workspace for stage B; each lane re-reads only what it wrote itself.
__global__ __launch_bounds__(kBlock)
void fc_head_rows_k(const float* __restrict__ h1,
                    const float* __restrict__ w,
                    const float* __restrict__ bias,
                    const long* __restrict__ labels,
                    const float* __restrict__ dloss, float* d2,
                    float* __restrict__ gl, float* __restrict__ row_loss,
                    float* __restrict__ g_h1, int B, int H, int C, float p,
                    const unsigned long long* __restrict__ state, int site,
                    int fwd_wave, int dx_wave) {
  const int row = blockIdx.x * (kBlock / kWave) + threadIdx.x / kWave;
  const int lane = threadIdx.x % kWave;
  if (row >= B) return;  // wave-uniform
  const uint64_t seed = state[0];
  const uint64_t offset = state[1] + site;
  const float scale = dropout_scale(p);
  const float* hrow = h1 + (long)row * H;
  float* drow = d2 + (long)row * H;

  // 1. dropout on the flat index row*H + j
  float d_first = 0.f;
  for (int j = lane; j < H; j += kWave) {
    bool keep = dropout_keep_at(seed, offset, (long)row * H + j, p);
    float y = dropout_apply(keep, hrow[j], scale);
    drow[j] = y;
    if (j == lane) d_first = y;
  }

  // 2. logits: GEMM (M=B, N=C, K=H), w (C,H) consumed as B^T
  float v = -3.4e38f;
  if (fwd_wave) {
    // 4 classes at a time so the shuffle trees overlap
    for (int c0 = 0; c0 < C; c0 += 4) {
      float acc[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        int cu = min(c0 + u, C - 1);
        const float* wr = w + (long)cu * H;
        acc[u] = dot_wave_partial(H, lane, [&](int k) { return drow[k]; },
                                  [&](int k) { return wr[k]; });
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) acc[u] = wave_tree_down(acc[u]);
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        int cu = min(c0 + u, C - 1);
        float l = __shfl(acc[u], 0, kWave);
        l += bias[cu];
        if (lane == c0 + u && lane < C) v = l;
      }
    }
  } else {
    // H < 32: the whole dropped row sits in d_first of lanes 0..H-1
    int cc = min(lane, C - 1);
    const float* wr = w + (long)cc * H;
    float acc = dot_rot4(H, [&](int k) { return __shfl(d_first, k, kWave); },
                         [&](int k) { return wr[k]; });
    acc += bias[cc];
    if (lane < C) v = acc;
  }

  // 3. softmax + row loss, 4. dlogits
  float sm, m, sum;
  ce_row_softmax(v, lane < C, sm, m, sum);
  const long t = labels[row];
  float lt = __shfl(v, (int)t, kWave);
  if (lane == 0) row_loss[row] = ce_row_loss(sum, m, lt);
  float gv = 0.f;
  if (lane < C) {
    gv = ce_grad(dloss[0], sm, t == lane, B);
    gl[(long)row * C + lane] = gv;
  }

  // 5. dx: GEMM (M=B, N=H, K=C) NN, 6. dropout+relu backward
  for (int j0 = 0; j0 < H; j0 += kWave) {
    const int j = j0 + lane;
    const int jc = min(j, H - 1);
    float dxv = 0.f;
    if (!dx_wave) {
      dxv = dot_rot4(C, [&](int k) { return __shfl(gv, k, kWave); },
                     [&](int k) { return w[(long)k * H + jc]; });
    } else {
      // one wave-wide dot per output; lane jj keeps output j0 + jj
      for (int jj = 0; jj < kWave && j0 + jj < H; jj += 4) {
        float acc[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          int ju = min(j0 + jj + u, H - 1);
          acc[u] = dot_wave_partial(
              C, lane, [&](int) { return gv; },
              [&](int k) { return w[(long)k * H + ju]; });
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) acc[u] = wave_tree_down(acc[u]);
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          float r = __shfl(acc[u], 0, kWave);
          if (lane == jj + u) dxv = r;
        }
      }
    }
    if (j < H) {
      bool keep = dropout_keep_at(seed, offset, (long)row * H + j, p);
      g_h1[(long)row * H + j] = dropout_relu_gate(hrow[j], keep, dxv, scale);
    }
  }
}

// Stage B, the three reductions over the batch, is a role: body in
// step_roles.h, maker below (fc_head_reduce_role).

// launch_gemm_f32_main's tiny-problem branch and its thread / wave choice
static bool gemm_tiny(long M, long N, long K) {
  return M * N * K <= 8'000'000 && M * N <= 65536;
}

extern "C" {

int pool_seam_fused_ok(int C, int H, int W) {
  long OHW = (long)(H / 2) * (W / 2);
  return C > 0 && (C % 4) == 0 && OHW > 0 &&
         OHW * (C + 1) <= kSeamTileFloats;
}

void launch_pool_flatten_dropout_fwd(const float* x, float* pooled,
                                     uint8_t* idx, float* d, uint8_t* mask,
                                     long B, int H, int W, int C, float p,
                                     const unsigned long long* state,
                                     int site, void* s) {
  if (B <= 0) return;
  pool_flatten_dropout_fwd_k<false>
      <<<(unsigned)B, kSeamBlock, 0, (hipStream_t)s>>>(
          x, pooled, idx, d, mask, H, W, H / 2, W / 2, C, p, state, site);
}

void launch_flatten_dropout_fwd(const float* pooled, float* d, uint8_t* mask,
                                long B, int OH, int OW, int C, float p,
                                const unsigned long long* state, int site,
                                void* s) {
  if (B <= 0) return;
  pool_flatten_dropout_fwd_k<true>
      <<<(unsigned)B, kSeamBlock, 0, (hipStream_t)s>>>(
          pooled, nullptr, nullptr, d, mask, 2 * OH, 2 * OW, OH, OW, C, p,
          state, site);
}

void launch_dropout_unflatten_pool_bwd_relu(const float* g,
                                            const uint8_t* mask,
                                            const uint8_t* idx,
                                            const float* pooled, float* dx,
                                            long B, int H, int W, int C,
                                            float p, void* s) {
  if (B <= 0) return;
  dropout_unflatten_pool_bwd_relu_k<<<(unsigned)B, kSeamBlock, 0,
                                      (hipStream_t)s>>>(
      g, mask, idx, pooled, dx, H, W, H / 2, W / 2, C, p);
}

// fwd (M=B, N=C, K=H), dx (M=B, N=H, K=C), dW (M=C, N=H, K=B)
int fc_head_fused_ok(int B, int H, int C) {
  return B > 0 && H > 0 && C > 0 && C <= 64 && gemm_tiny(B, C, H) &&
         gemm_tiny(B, H, C) && gemm_tiny(C, H, B);
}

// dropped activations (B*H), dlogits (B*C), row losses (B)
long fc_head_ws_floats(int B, int H, int C) {
  return (long)B * H + (long)B * C + B;
}

// stage A: per-row work, into ws (dropped activations, dlogits, row
// losses) and g_h1
void launch_fc_head_rows(const float* h1, const float* w, const float* bias,
                         const long* labels, const float* dloss, float* ws,
                         float* g_h1, int B, int H, int C, float p,
                         const unsigned long long* state, int site,
                         void* s) {
  float* d2 = ws;
  float* gl = d2 + (long)B * H;
  float* row_loss = gl + (long)B * C;
  const int wpb = kBlock / kWave;
  fc_head_rows_k<<<(B + wpb - 1) / wpb, kBlock, 0, (hipStream_t)s>>>(
      h1, w, bias, labels, dloss, d2, gl, row_loss, g_h1, B, H, C, p, state,
      site, H >= 32, C >= 32);
}

// stage B as a role over the ws that stage A filled
StepRole fc_head_reduce_role(const float* ws, float* dw, float* db,
                             float* loss, int B, int H, int C) {
  const float* d2 = ws;
  const float* gl = d2 + (long)B * H;
  const float* row_loss = gl + (long)B * C;
  const int wpb = kBlock / kWave;
  const int dw_wave = B >= 32;
  const long n_out = (long)C * H;
  const int dw_blocks = (int)(dw_wave ? (n_out + wpb - 1) / wpb
                                      : (n_out + kBlock - 1) / kBlock);
  const int db_blocks = (C + wpb - 1) / wpb;
  StepRole r{};
  r.kind = kRoleFcHeadReduce;
  r.gx = dw_blocks + db_blocks + 1;
  r.gy = 1;
  r.count = r.gx;
  r.fc_head_reduce.gl = gl;
  r.fc_head_reduce.d2 = d2;
  r.fc_head_reduce.row_loss = row_loss;
  r.fc_head_reduce.dw = dw;
  r.fc_head_reduce.db = db;
  r.fc_head_reduce.loss = loss;
  r.fc_head_reduce.B = B;
  r.fc_head_reduce.H = H;
  r.fc_head_reduce.C = C;
  r.fc_head_reduce.dw_blocks = dw_blocks;
  r.fc_head_reduce.db_blocks = db_blocks;
  r.fc_head_reduce.dw_wave = dw_wave;
  return r;
}
}
