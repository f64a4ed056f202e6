// Torch bindings for the rlr_amd HIP kernels.  This TU is the only one
// that includes torch headers; the kernels are plain HIP compiled
// separately (no hipify, no CUDA shims anywhere).  The launchers and the
// functions that size their workspaces are declared in launchers.h.
#include <torch/extension.h>
#include <c10/hip/HIPStream.h>

#include <algorithm>
#include <cstdint>
#include <vector>

#include "launchers.h"

#define CHK(x) TORCH_CHECK(x, #x)
#define CHK_CUDA(t)                                                      \
  TORCH_CHECK((t).is_cuda() &&                                           \
                  ((t).is_contiguous() ||                                \
                   (t).is_contiguous(torch::MemoryFormat::ChannelsLast)),\
              #t " must be cuda + dense")

static void* stream_of(const torch::Tensor& t) {
  return (void*)c10::hip::getCurrentHIPStream(t.device().index()).stream();
}

// 4-D activations are channels_last (NHWC storage) on the HIP path.
// RLR_AMD_DEBUG_LAYOUT=1 prints every call that actually COPIES (a copy
// here means some producer broke the channels_last chain — hot-path bug).
static bool layout_debug() {
  static int v = -1;
  if (v < 0) {
    const char* e = getenv("RLR_AMD_DEBUG_LAYOUT");
    v = (e && e[0] == '1') ? 1 : 0;
  }
  return v == 1;
}
static torch::Tensor cl(torch::Tensor t, const char* site = "?") {
  if (layout_debug() && t.dim() == 4 &&
      !t.is_contiguous(torch::MemoryFormat::ChannelsLast))
    fprintf(stderr, "[layout] cl(%s) copy %ldx%ldx%ldx%ld dtype=%d\n",
            site, (long)t.size(0), (long)t.size(1), (long)t.size(2),
            (long)t.size(3), (int)t.scalar_type());
  return t.contiguous(torch::MemoryFormat::ChannelsLast);
}
static torch::Tensor empty_cl(std::vector<int64_t> sizes,
                              const torch::TensorOptions& opts) {
  return torch::empty(sizes,
                      opts.memory_format(torch::MemoryFormat::ChannelsLast));
}
// make t's storage order match ref's (flat elementwise kernels require it)
static torch::Tensor match_layout(const torch::Tensor& ref,
                                  torch::Tensor t) {
  if (ref.dim() == 4 &&
      ref.is_contiguous(torch::MemoryFormat::ChannelsLast) &&
      !ref.is_contiguous())
    return t.contiguous(torch::MemoryFormat::ChannelsLast);
  return t.contiguous();
}

namespace {

static bool is_bf16(const torch::Tensor& t) {
  return t.scalar_type() == torch::kBFloat16;
}
// bf16 storage as the launchers take it (raw ushort): read / write side
static const unsigned short* bfc(const torch::Tensor& t) {
  return (const unsigned short*)t.data_ptr();
}
static unsigned short* bfp(const torch::Tensor& t) {
  return (unsigned short*)t.data_ptr();
}

// ------------------------------------------------------------- step queue
// The small fold / permute / copy kernels of the fp32 entry points, as
// roles (step_batch.hip).  An entry point launches its main kernels and
// pushes its roles here, level 1 (a first stage, or a single-stage final)
// before level 2 (a second stage).  The deferred queue the manual tape
// hands in keeps them, and every tensor they touch, until flush() issues
// level 1 and then level 2 as role-batched launches; roles of one level
// never depend on each other.  The immediate queue an entry point makes for
// itself when it is handed none launches each role as it is pushed, on the
// stream of the tensors just held, and keeps nothing: the caching allocator
// already makes that safe, as for every other temporary here.
struct StepQueue {
  bool immediate;
  std::vector<StepRole> lv[2];
  std::vector<torch::Tensor> held;
  void* stream = nullptr;

  explicit StepQueue(bool immediate_ = false) : immediate(immediate_) {}

  void hold(const torch::Tensor& t) {
    if (!t.defined()) return;
    void* st = stream_of(t);
    TORCH_CHECK(stream == nullptr || stream == st,
                "StepQueue: roles of one flush must share a stream");
    stream = st;
    if (!immediate) held.push_back(t);
  }
  void push(int level, const StepRole& r) {
    if (!immediate) {
      lv[level].push_back(r);
      return;
    }
    TORCH_CHECK(launch_step_role(&r, stream) == 0, "StepQueue: bad role");
  }
  std::tuple<int64_t, int64_t> pending() const {
    return {(int64_t)lv[0].size(), (int64_t)lv[1].size()};
  }
  void flush() {
    for (auto& level : lv) {
      for (size_t i = 0; i < level.size(); i += kStepMaxRoles) {
        size_t n = std::min(level.size() - i, (size_t)kStepMaxRoles);
        TORCH_CHECK(launch_step_batch(level.data() + i, (int)n, stream) == 0,
                    "StepQueue: more roles than one launch takes");
      }
      level.clear();
    }
    held.clear();
    stream = nullptr;
  }

  static const float* f32c(const torch::Tensor& t) {
    TORCH_CHECK(t.is_cuda() && t.scalar_type() == torch::kFloat);
    return t.data_ptr<float>();
  }

  // db_out (Kout) = column sums of dy, channels_last (Nb, Kout, OH, OW)
  void conv_db(torch::Tensor dy, torch::Tensor db_out) {
    TORCH_CHECK(dy.dim() == 4 &&
                dy.is_contiguous(torch::MemoryFormat::ChannelsLast));
    int Nb = dy.size(0), Kout = dy.size(1), OHW = dy.size(2) * dy.size(3);
    TORCH_CHECK(db_out.is_contiguous() && db_out.numel() == Kout);
    auto parts = torch::empty({conv_db_ws_floats(Kout)}, dy.options());
    StepRole a, b;
    conv_db_roles(f32c(dy), (float*)f32c(db_out), parts.data_ptr<float>(), Nb,
                  Kout, OHW, &a, &b);
    hold(dy); hold(db_out); hold(parts);
    push(0, a);
    push(1, b);
  }
  // the split-K combine + dw permute over ws (conv_dwperm_ws_floats layout)
  void splitk_reduce_dwperm(torch::Tensor ws, torch::Tensor dw, int64_t Kout,
                            int64_t C, int64_t RS, int64_t SK,
                            int64_t ws_offset) {
    TORCH_CHECK(dw.is_contiguous() && dw.numel() == Kout * C * RS);
    StepRole a, b;
    int levels = splitk_reduce_dwperm_roles(
        f32c(ws) + ws_offset, (float*)f32c(dw), (int)Kout, (int)C, (int)RS,
        (int)SK, &a, &b);
    hold(ws); hold(dw);
    push(0, a);
    if (levels == 2) push(1, b);
  }
  // the split-K combine over ws; false (nothing pushed) for the wave form,
  // which has no role: the caller runs launch_splitk_reduce
  bool splitk_reduce(torch::Tensor ws, torch::Tensor C,
                     c10::optional<torch::Tensor> bias, int64_t M, int64_t N,
                     int64_t ldc, int64_t SK, bool relu) {
    StepRole a, b;
    int levels = splitk_reduce_roles(
        f32c(ws), (float*)f32c(C), bias ? f32c(*bias) : nullptr, (int)M,
        (int)N, (int)ldc, (int)SK, relu ? 1 : 0, &a, &b);
    if (levels == 0) return false;
    hold(ws); hold(C);
    if (bias) hold(*bias);
    push(0, a);
    if (levels == 2) push(1, b);
    return true;
  }
  void colsum(torch::Tensor dy, torch::Tensor db_out) {
    TORCH_CHECK(dy.dim() == 2 && dy.is_contiguous() &&
                db_out.is_contiguous() && db_out.numel() == dy.size(1));
    hold(dy); hold(db_out);
    push(0, colsum_role(f32c(dy), (float*)f32c(db_out), (int)dy.size(0),
                        (int)dy.size(1)));
  }
  // the combine of backward-weight over the ws its main kernels wrote
  void conv_bwd_weight_combine(torch::Tensor ws, torch::Tensor dw, int SK,
                               int Nb, int C, int Kout, int R, int S, int OH,
                               int OW) {
    StepRole a, b;
    int levels = conv_bwd_weight_combine_roles(
        (float*)f32c(ws), (float*)f32c(dw), SK, Nb, C, Kout, R, S, OH, OW,
        &a, &b);
    hold(ws); hold(dw);
    push(0, a);
    if (levels == 2) push(1, b);
  }
  // the small-conv chunk partials (chunks, KO*C*RS) -> dw, as
  // conv_bwd_weight_combine queues it for a layer with C*R*S <= 32
  void conv_small_bwdw_reduce(torch::Tensor partials, torch::Tensor dw,
                              int64_t Nb, int64_t C, int64_t Kout, int64_t R,
                              int64_t S, int64_t OH, int64_t OW) {
    TORCH_CHECK(C * R * S <= 32 && Kout <= 64);
    TORCH_CHECK(dw.is_contiguous() && dw.numel() == Kout * C * R * S);
    TORCH_CHECK(partials.numel() >=
                conv_small_bwdw_chunks(Nb * OH * OW) * Kout * C * R * S);
    conv_bwd_weight_combine(partials, dw, 1, (int)Nb, (int)C, (int)Kout,
                            (int)R, (int)S, (int)OH, (int)OW);
  }
  // kind 0: the forward's wt (C*R*S, Kout); kind 1: bwd-data's wp
  // (Kout*R*S, C)
  torch::Tensor wperm(torch::Tensor w, int64_t kind) {
    TORCH_CHECK(w.dim() == 4 && (kind == 0 || kind == 1));
    w = w.contiguous();
    int Kout = w.size(0), C = w.size(1), RS = w.size(2) * w.size(3);
    auto out = kind == 0 ? torch::empty({(long)C * RS, Kout}, w.options())
                         : torch::empty({(long)Kout * RS, C}, w.options());
    hold(w); hold(out);
    push(0, wperm_role((int)kind, f32c(w), out.data_ptr<float>(), Kout, C,
                       RS));
    return out;
  }
  // dst[r] = src[sel[r]] over dim 0; float or int64, rows dense and laid
  // out alike in src and dst.  sel must index [0, src.size(0)): unlike
  // index_select nothing asserts on the device; an index outside the range
  // is not read, its row comes out as all-one bits (NaN / -1).
  void gather_rows(torch::Tensor src, torch::Tensor sel, torch::Tensor dst) {
    TORCH_CHECK(src.is_cuda() && dst.is_cuda() && sel.is_cuda());
    TORCH_CHECK(sel.scalar_type() == torch::kInt64 && sel.is_contiguous());
    TORCH_CHECK(src.scalar_type() == dst.scalar_type() &&
                (src.scalar_type() == torch::kFloat ||
                 src.scalar_type() == torch::kInt64));
    TORCH_CHECK(src.dim() == dst.dim() && src.dim() >= 1 &&
                dst.size(0) == sel.numel());
    long row = src.dim() > 1 ? src.numel() / std::max<long>(src.size(0), 1)
                             : 1;
    TORCH_CHECK(src.is_non_overlapping_and_dense() &&
                dst.is_non_overlapping_and_dense());
    TORCH_CHECK(src.size(0) <= 1 || src.stride(0) == row);
    TORCH_CHECK(dst.size(0) <= 1 || dst.stride(0) == row);
    for (int d = 1; d < src.dim(); ++d)
      TORCH_CHECK(src.size(d) == dst.size(d) &&
                      (src.size(d) == 1 || src.stride(d) == dst.stride(d)),
                  "gather_rows: src and dst rows must be laid out alike");
    int words = (int)(row * (src.scalar_type() == torch::kInt64 ? 2 : 1));
    hold(src); hold(sel); hold(dst);
    TORCH_CHECK(src.size(0) <= INT32_MAX);
    push(0, step_role_gather_rows(src.data_ptr(), sel.data_ptr<int64_t>(),
                                  dst.data_ptr(), sel.numel(), words,
                                  (int)src.size(0)));
  }
  // level 2: state[index] += delta (the dropout base offset of the next
  // step, after every draw of this one)
  void add_u64(torch::Tensor state, int64_t index, int64_t delta) {
    TORCH_CHECK(state.is_cuda() && state.is_contiguous() &&
                (state.scalar_type() == torch::kInt64 ||
                 state.scalar_type() == torch::kUInt64) &&
                index >= 0 && index < state.numel());
    hold(state);
    push(1, step_role_add_u64((unsigned long long*)state.data_ptr() + index,
                              (unsigned long long)delta));
  }
};



// ------------------------------------------------------------ elementwise

torch::Tensor relu_fwd(torch::Tensor x) {
  CHK_CUDA(x);
  auto y = torch::empty_like(x);
  if (is_bf16(x))
    launch_relu_fwd_bf16(bfc(x), bfp(y), x.numel(), stream_of(x));
  else
    launch_relu_fwd(x.data_ptr<float>(), y.data_ptr<float>(), x.numel(),
                    stream_of(x));
  return y;
}

torch::Tensor relu_bwd(torch::Tensor y, torch::Tensor dy) {
  CHK_CUDA(y);
  dy = match_layout(y, dy);
  auto dx = torch::empty_like(y);
  if (is_bf16(y))
    launch_relu_bwd_bf16(bfc(y), bfc(dy), bfp(dx), y.numel(), stream_of(y));
  else
    launch_relu_bwd(y.data_ptr<float>(), dy.data_ptr<float>(),
                    dx.data_ptr<float>(), y.numel(), stream_of(y));
  return dx;
}

torch::Tensor add_relu_fwd(torch::Tensor a, torch::Tensor b) {
  CHK_CUDA(a);
  b = match_layout(a, b);
  auto y = torch::empty_like(a);
  if (is_bf16(a))
    launch_add_relu_bf16(bfc(a), bfc(b), bfp(y), a.numel(), stream_of(a));
  else
    launch_add_relu(a.data_ptr<float>(), b.data_ptr<float>(),
                    y.data_ptr<float>(), a.numel(), stream_of(a));
  return y;
}

std::tuple<torch::Tensor, torch::Tensor> maxpool2x2_fwd(torch::Tensor x) {
  TORCH_CHECK(x.is_cuda() && x.dim() == 4);
  x = cl(x, "mp_fwd.x");
  int Nb = x.size(0), C = x.size(1), H = x.size(2), W = x.size(3);
  int OH = H / 2, OW = W / 2;
  auto y = empty_cl({Nb, C, OH, OW}, x.options());
  auto idx = empty_cl({Nb, C, OH, OW}, x.options().dtype(torch::kUInt8));
  if (is_bf16(x))
    launch_maxpool2x2_fwd_bf16(bfc(x), bfp(y), idx.data_ptr<uint8_t>(), Nb,
                               H, W, OH, OW, C, stream_of(x));
  else
    launch_maxpool2x2_fwd(x.data_ptr<float>(), y.data_ptr<float>(),
                          idx.data_ptr<uint8_t>(), Nb, H, W, OH, OW, C,
                          stream_of(x));
  return {y, idx};
}

torch::Tensor maxpool2x2_bwd(torch::Tensor dy, torch::Tensor idx,
                             std::vector<int64_t> in_shape) {
  TORCH_CHECK(dy.is_cuda());
  dy = cl(dy, "mp_bwd.dy");
  int Nb = in_shape[0], C = in_shape[1], H = in_shape[2], W = in_shape[3];
  int OH = dy.size(2), OW = dy.size(3);
  auto dx = empty_cl({Nb, C, H, W}, dy.options());
  if (is_bf16(dy))
    launch_maxpool2x2_bwd_bf16(bfc(dy), idx.data_ptr<uint8_t>(), bfp(dx),
                               Nb, H, W, OH, OW, C, stream_of(dy));
  else
    launch_maxpool2x2_bwd(dy.data_ptr<float>(), idx.data_ptr<uint8_t>(),
                          dx.data_ptr<float>(), Nb, H, W, OH, OW, C,
                          stream_of(dy));
  return dx;
}

// masked join: a = (relu_y>0) ? a+b : 0 (manual tape — see
// add_relu_bwd_* kernels)
torch::Tensor add_relu_bwd_(torch::Tensor a, torch::Tensor b,
                            torch::Tensor relu_y) {
  CHK_CUDA(a);
  TORCH_CHECK(a.numel() == b.numel() && a.numel() == relu_y.numel());
  if (is_bf16(a))
    launch_add_relu_bwd_bf16(bfp(a), bfc(b), bfc(relu_y), a.numel(),
                             stream_of(a));
  else
    launch_add_relu_bwd(a.data_ptr<float>(), b.data_ptr<float>(),
                        relu_y.data_ptr<float>(), a.numel(), stream_of(a));
  return a;
}

// masked gap backward (manual tape)
torch::Tensor gap_bwd_relu(torch::Tensor dy, torch::Tensor relu_y,
                           std::vector<int64_t> in_shape) {
  CHK_CUDA(dy);
  int Nb = in_shape[0], C = in_shape[1];
  int HW = in_shape[2] * in_shape[3];
  auto dx = empty_cl(in_shape, relu_y.options());
  relu_y = cl(relu_y, "gap_bwd.relu");
  if (is_bf16(relu_y))
    launch_gap_bwd_relu_bf16(bfc(dy), bfc(relu_y), bfp(dx), Nb, HW, C,
                             stream_of(dy));
  else
    launch_gap_bwd_relu(dy.data_ptr<float>(), relu_y.data_ptr<float>(),
                        dx.data_ptr<float>(), Nb, HW, C, stream_of(dy));
  return dx;
}

// in-place elementwise add (residual gradient join in the manual tape)
torch::Tensor add_inplace(torch::Tensor a, torch::Tensor b) {
  CHK_CUDA(a);
  TORCH_CHECK(a.numel() == b.numel() && a.scalar_type() == b.scalar_type());
  if (is_bf16(a))
    launch_add_inplace_bf16(bfp(a), bfc(b), a.numel(), stream_of(a));
  else
    launch_add_inplace(a.data_ptr<float>(), b.data_ptr<float>(), a.numel(),
                       stream_of(a));
  return a;
}

// fused relu-mask maxpool backward (manual tape; C % 4 == 0)
torch::Tensor maxpool2x2_bwd_relu(torch::Tensor dy, torch::Tensor idx,
                                  torch::Tensor relu_pooled,
                                  std::vector<int64_t> in_shape) {
  TORCH_CHECK(dy.is_cuda() && !is_bf16(dy));
  dy = cl(dy, "mp_bwd.dy");
  relu_pooled = cl(relu_pooled, "mp_bwd.relu");
  int Nb = in_shape[0], C = in_shape[1], H = in_shape[2], W = in_shape[3];
  TORCH_CHECK((C % 4) == 0);
  int OH = dy.size(2), OW = dy.size(3);
  auto dx = empty_cl({Nb, C, H, W}, dy.options());
  launch_maxpool2x2_bwd_relu(dy.data_ptr<float>(), idx.data_ptr<uint8_t>(),
                             relu_pooled.data_ptr<float>(),
                             dx.data_ptr<float>(), Nb, H, W, OH, OW, C,
                             stream_of(dy));
  return dx;
}

std::tuple<torch::Tensor, torch::Tensor> dropout_fwd(torch::Tensor x,
                                                     double p, int64_t seed,
                                                     int64_t offset) {
  CHK_CUDA(x);
  auto y = torch::empty_like(x);
  auto mask = torch::empty(x.sizes(), x.options().dtype(torch::kUInt8));
  launch_dropout_fwd(x.data_ptr<float>(), y.data_ptr<float>(),
                     mask.data_ptr<uint8_t>(), x.numel(), (float)p,
                     (uint64_t)seed, (uint64_t)offset, stream_of(x));
  return {y, mask};
}

std::tuple<torch::Tensor, torch::Tensor> dropout_fwd_dev(torch::Tensor x,
                                                         double p,
                                                         torch::Tensor state,
                                                         int64_t site) {
  CHK_CUDA(x);
  CHK(state.scalar_type() == torch::kUInt64 ||
      state.scalar_type() == torch::kInt64);
  auto y = torch::empty_like(x);
  auto mask = torch::empty(x.sizes(), x.options().dtype(torch::kUInt8));
  if (is_bf16(x))
    launch_dropout_fwd_dev_bf16(
        bfc(x), bfp(y), mask.data_ptr<uint8_t>(), x.numel(), (float)p,
        (const unsigned long long*)state.data_ptr(), (int)site,
        stream_of(x));
  else
    launch_dropout_fwd_dev(
        x.data_ptr<float>(), y.data_ptr<float>(), mask.data_ptr<uint8_t>(),
        x.numel(), (float)p,
        (const unsigned long long*)state.data_ptr(), (int)site,
        stream_of(x));
  return {y, mask};
}

torch::Tensor dropout_bwd(torch::Tensor dy, torch::Tensor mask, double p) {
  CHK_CUDA(dy);
  auto dx = torch::empty_like(dy);
  if (is_bf16(dy))
    launch_dropout_bwd_bf16(bfc(dy), mask.data_ptr<uint8_t>(), bfp(dx),
                            dy.numel(), (float)p, stream_of(dy));
  else
    launch_dropout_bwd(dy.data_ptr<float>(), mask.data_ptr<uint8_t>(),
                       dx.data_ptr<float>(), dy.numel(), (float)p,
                       stream_of(dy));
  return dx;
}

// fused dropout+relu backward (manual tape): (y>0) * dropout_bwd(dy)
torch::Tensor dropout_relu_bwd(torch::Tensor dy, torch::Tensor mask,
                               torch::Tensor y, double p) {
  CHK_CUDA(dy);
  TORCH_CHECK(!is_bf16(dy));
  dy = dy.contiguous();
  auto dx = torch::empty_like(dy);
  launch_dropout_relu_bwd(dy.data_ptr<float>(), mask.data_ptr<uint8_t>(),
                          y.data_ptr<float>(), dx.data_ptr<float>(),
                          dy.numel(), (float)p, stream_of(dy));
  return dx;
}

torch::Tensor gap_fwd(torch::Tensor x) {
  TORCH_CHECK(x.is_cuda());
  x = cl(x, "mpB.x");
  int Nb = x.size(0), C = x.size(1), HW = x.size(2) * x.size(3);
  auto y = torch::empty({Nb, C}, x.options());
  if (is_bf16(x))
    launch_gap_fwd_bf16(bfc(x), bfp(y), Nb, HW, C, stream_of(x));
  else
    launch_gap_fwd(x.data_ptr<float>(), y.data_ptr<float>(), Nb, HW, C,
                   stream_of(x));
  return y;
}

torch::Tensor gap_bwd(torch::Tensor dy, std::vector<int64_t> in_shape) {
  TORCH_CHECK(dy.is_cuda());
  dy = dy.contiguous();
  int Nb = in_shape[0], C = in_shape[1], HW = in_shape[2] * in_shape[3];
  auto dx = empty_cl({Nb, C, in_shape[2], in_shape[3]}, dy.options());
  if (is_bf16(dy))
    launch_gap_bwd_bf16(bfc(dy), bfp(dx), Nb, HW, C, stream_of(dy));
  else
    launch_gap_bwd(dy.data_ptr<float>(), dx.data_ptr<float>(), Nb, HW, C,
                   stream_of(dy));
  return dx;
}

std::tuple<torch::Tensor, torch::Tensor> cross_entropy_fwd(
    torch::Tensor logits, torch::Tensor labels) {
  CHK_CUDA(logits);
  labels = labels.contiguous();
  int B = logits.size(0), C = logits.size(1);
  CHK(C <= 64);
  auto softmax = torch::empty_like(logits);
  auto row_loss = torch::empty({B}, logits.options());
  auto loss = torch::empty({}, logits.options());
  launch_ce_fwd(logits.data_ptr<float>(), labels.data_ptr<int64_t>(),
                softmax.data_ptr<float>(), row_loss.data_ptr<float>(),
                loss.data_ptr<float>(), B, C, stream_of(logits));
  return {loss, softmax};
}

torch::Tensor cross_entropy_bwd(torch::Tensor softmax, torch::Tensor labels,
                                torch::Tensor dloss) {
  CHK_CUDA(softmax);
  int B = softmax.size(0), C = softmax.size(1);
  auto dlogits = torch::empty_like(softmax);
  auto d = dloss.to(softmax.device()).contiguous();
  launch_ce_bwd(softmax.data_ptr<float>(), labels.data_ptr<int64_t>(),
                d.data_ptr<float>(), dlogits.data_ptr<float>(), B, C,
                stream_of(softmax));
  return dlogits;
}

void eval_update(torch::Tensor logits, torch::Tensor labels,
                 torch::Tensor conf, torch::Tensor loss_sum) {
  CHK_CUDA(logits);
  int B = logits.size(0), C = logits.size(1);
  int num_classes = (int)std::sqrt((double)conf.numel());
  launch_eval_update(logits.data_ptr<float>(), labels.data_ptr<int64_t>(),
                     conf.data_ptr<float>(), loss_sum.data_ptr<double>(), B,
                     C, num_classes, stream_of(logits));
}

// flatten: channels_last (B,C,H,W) -> (B, C*H*W) in CHW order
torch::Tensor nhwc_flatten(torch::Tensor x) {
  TORCH_CHECK(x.is_cuda() && x.dim() == 4);
  x = cl(x, "gap.x");
  long B = x.size(0);
  int C = x.size(1), H = x.size(2), W = x.size(3);
  auto out = torch::empty({B, (long)C * H * W}, x.options());
  if (is_bf16(x))
    launch_nhwc_flatten_bf16(bfc(x), bfp(out), B, C, H, W, stream_of(x));
  else
    launch_nhwc_flatten(x.data_ptr<float>(), out.data_ptr<float>(), B, C,
                        H, W, stream_of(x));
  return out;
}

torch::Tensor nhwc_unflatten(torch::Tensor g, int64_t C, int64_t H,
                             int64_t W) {
  TORCH_CHECK(g.is_cuda());
  g = g.contiguous();
  long B = g.size(0);
  auto out = empty_cl({B, C, H, W}, g.options());
  if (is_bf16(g))
    launch_nhwc_unflatten_bf16(bfc(g), bfp(out), B, (int)C, (int)H, (int)W,
                               stream_of(g));
  else
    launch_nhwc_unflatten(g.data_ptr<float>(), out.data_ptr<float>(), B,
                          (int)C, (int)H, (int)W, stream_of(g));
  return out;
}

// --------------------------------------------------------------- flatopt

void clipped_sgd_step(torch::Tensor p, torch::Tensor g, torch::Tensor v,
                      double lr, double mu, double max_norm) {
  CHK_CUDA(p);
  auto scratch = torch::empty({flat_norm_scratch_floats()}, p.options());
  launch_clipped_sgd(p.data_ptr<float>(), g.data_ptr<float>(),
                     v.data_ptr<float>(), scratch.data_ptr<float>(),
                     (float)lr, (float)mu, (float)max_norm, p.numel(),
                     stream_of(p));
}

void pgd_project(torch::Tensor p, torch::Tensor t0, double clip) {
  CHK_CUDA(p);
  auto scratch = torch::empty({flat_norm_scratch_floats()}, p.options());
  launch_pgd_project(p.data_ptr<float>(), t0.data_ptr<float>(),
                     scratch.data_ptr<float>(), (float)clip, p.numel(),
                     stream_of(p));
}

void gather_grads(torch::Tensor flat, std::vector<torch::Tensor> grads,
                  std::vector<int64_t> offsets) {
  CHK_CUDA(flat);
  CHK(grads.size() == offsets.size());
  // any .contiguous() temporaries must outlive ALL async launches below
  // (freeing them per-iteration would race the gather kernel when a grad
  // is non-contiguous)
  std::vector<torch::Tensor> held;
  held.reserve(grads.size());
  for (auto& g : grads) {
    TORCH_CHECK(g.scalar_type() == torch::kFloat);
    held.push_back(g.contiguous());
  }
  size_t i = 0;
  while (i < held.size()) {
    const float* srcs[16];
    long offs[16], lens[16];
    int cnt = 0;
    for (; cnt < 16 && i < held.size(); ++cnt, ++i) {
      srcs[cnt] = held[i].data_ptr<float>();
      offs[cnt] = offsets[i];
      lens[cnt] = held[i].numel();
    }
    launch_gather_grads(srcs, offs, lens, cnt, flat.data_ptr<float>(),
                        stream_of(flat));
  }
}

torch::Tensor delta64(torch::Tensor p, torch::Tensor t0) {
  CHK_CUDA(p);
  CHK(t0.scalar_type() == torch::kFloat64);
  auto out = torch::empty_like(t0);
  launch_delta64(p.data_ptr<float>(), t0.data_ptr<double>(),
                 out.data_ptr<double>(), p.numel(), stream_of(p));
  return out;
}

// ------------------------------------------------------------ aggregation

// The two argument checks every server entry point shares.  Each runs
// before any data_ptr and any launch: a kernel only ever sees pointers
// whose device, dtype and extent were checked here.
// A (K, n) update matrix: on device, 2-D, fp64, contiguous,
// 1 <= K <= max_k, n >= 1.
static void check_matrix(const torch::Tensor& U, int64_t max_k) {
  CHK(U.is_cuda());
  CHK(U.dim() == 2);
  CHK(U.scalar_type() == torch::kFloat64);
  CHK(U.is_contiguous());
  CHK(U.size(0) >= 1 && U.size(0) <= max_k);
  CHK(U.size(1) >= 1);
}
// A vector that belongs to `ref`: on ref's device, 1-D, contiguous, of
// exactly `len` elements; fp64 like the matrix unless the caller says fp32.
static void check_vector(const torch::Tensor& v, const torch::Tensor& ref,
                         int64_t len,
                         torch::ScalarType dtype = torch::kFloat64) {
  CHK(v.is_cuda() && v.device() == ref.device());
  CHK(v.scalar_type() == dtype);
  CHK(v.dim() == 1 && v.is_contiguous());
  CHK(v.numel() == len);
}

// the per-coordinate learning-rate output: n doubles, or empty (and a null
// pointer to the launcher) when the caller does not want it
static torch::Tensor lr_buf(bool want_lr, long n, const torch::Tensor& U) {
  return torch::empty({want_lr ? n : 0}, U.options());
}

// What a weighted mean divides by: the caller's divisor when it gives one
// (> 0), which needs no host read; sum(w), read back from the device, for
// the default 0.
static double mean_divisor(const torch::Tensor& w, double divisor) {
  CHK(divisor >= 0.0);
  return divisor > 0.0 ? divisor : w.sum().item<double>();
}

torch::Tensor fused_avg_rlr_apply(torch::Tensor U, torch::Tensor w,
                                  torch::Tensor params, bool rlr,
                                  double thresh, double slr,
                                  double noise_std, int64_t seed,
                                  int64_t offset, bool want_lr,
                                  double divisor) {
  check_matrix(U, INT32_MAX);
  check_vector(w, U, U.size(0));
  check_vector(params, U, U.size(1), torch::kFloat32);
  int K = U.size(0);
  long n = U.size(1);
  double wsum = mean_divisor(w, divisor);
  auto lr = lr_buf(want_lr, n, U);
  launch_fused_avg_rlr_apply(
      U.data_ptr<double>(), w.data_ptr<double>(), K, n, 1.0 / wsum,
      rlr ? 1 : 0, thresh, slr, params.data_ptr<float>(),
      want_lr ? lr.data_ptr<double>() : nullptr, noise_std, (uint64_t)seed,
      (uint64_t)offset, stream_of(U));
  return lr;
}

torch::Tensor rlr_vote(torch::Tensor U, double thresh, double slr) {
  check_matrix(U, INT32_MAX);
  int K = U.size(0);
  long n = U.size(1);
  auto lr = torch::empty({n}, U.options());
  launch_rlr_vote(U.data_ptr<double>(), K, n, thresh, slr,
                  lr.data_ptr<double>(), stream_of(U));
  return lr;
}

torch::Tensor agg_avg(torch::Tensor U, torch::Tensor w, double divisor) {
  check_matrix(U, INT32_MAX);
  check_vector(w, U, U.size(0));
  int K = U.size(0);
  long n = U.size(1);
  double wsum = mean_divisor(w, divisor);
  auto out = torch::empty({n}, U.options());
  launch_agg_avg(U.data_ptr<double>(), w.data_ptr<double>(), K, n,
                 1.0 / wsum, out.data_ptr<double>(), stream_of(U));
  return out;
}

torch::Tensor agg_sign(torch::Tensor U) {
  check_matrix(U, INT32_MAX);
  auto out = torch::empty({U.size(1)}, U.options());
  launch_agg_sign(U.data_ptr<double>(), U.size(0), U.size(1),
                  out.data_ptr<double>(), stream_of(U));
  return out;
}

torch::Tensor agg_comed(torch::Tensor U) {
  check_matrix(U, 64);
  auto out = torch::empty({U.size(1)}, U.options());
  launch_agg_comed(U.data_ptr<double>(), U.size(0), U.size(1),
                   out.data_ptr<double>(), stream_of(U));
  return out;
}

std::tuple<torch::Tensor, torch::Tensor> agg_orderstat(
    torch::Tensor U, int64_t lo, int64_t hi, bool want_lr, double thresh,
    double slr) {
  check_matrix(U, orderstat_max_k());
  CHK(0 <= lo && lo < hi && hi <= U.size(0));
  int K = U.size(0);
  long n = U.size(1);
  auto out = torch::empty({n}, U.options());
  auto lr = lr_buf(want_lr, n, U);
  launch_agg_orderstat(U.data_ptr<double>(), K, n, (int)lo, (int)hi,
                       1.0 / (double)(hi - lo), out.data_ptr<double>(),
                       want_lr ? lr.data_ptr<double>() : nullptr, thresh, slr,
                       stream_of(U));
  return {out, lr};
}

torch::Tensor orderstat_rlr_apply(torch::Tensor U, int64_t lo, int64_t hi,
                                  torch::Tensor params, bool rlr,
                                  double thresh, double slr, bool want_lr) {
  check_matrix(U, orderstat_max_k());
  CHK(0 <= lo && lo < hi && hi <= U.size(0));
  check_vector(params, U, U.size(1), torch::kFloat32);
  int K = U.size(0);
  long n = U.size(1);
  auto lr = lr_buf(want_lr, n, U);
  launch_orderstat_rlr_apply(U.data_ptr<double>(), K, n, (int)lo, (int)hi,
                             1.0 / (double)(hi - lo), rlr ? 1 : 0, thresh,
                             slr, params.data_ptr<float>(),
                             want_lr ? lr.data_ptr<double>() : nullptr,
                             stream_of(U));
  return lr;
}

// perm: K distinct row indices of U, the theta selected rows first.  Its
// values live on the device; the kernel never dereferences one outside
// [0, K).
static void check_bulyan(const torch::Tensor& U, const torch::Tensor& perm,
                         int64_t theta, int64_t beta) {
  check_matrix(U, bulyan_max_k());
  check_vector(perm, U, U.size(0), torch::kInt32);
  CHK(1 <= beta && beta <= theta && theta <= U.size(0));
}

std::tuple<torch::Tensor, torch::Tensor> bulyan_trim(
    torch::Tensor U, torch::Tensor perm, int64_t theta, int64_t beta,
    bool want_lr, double thresh, double slr) {
  check_bulyan(U, perm, theta, beta);
  int K = U.size(0);
  long n = U.size(1);
  auto out = torch::empty({n}, U.options());
  auto lr = lr_buf(want_lr, n, U);
  launch_bulyan_trim(U.data_ptr<double>(), perm.data_ptr<int>(), K,
                     (int)theta, (int)beta, n, out.data_ptr<double>(),
                     want_lr ? lr.data_ptr<double>() : nullptr, thresh, slr,
                     stream_of(U));
  return {out, lr};
}

torch::Tensor bulyan_rlr_apply(torch::Tensor U, torch::Tensor perm,
                               int64_t theta, int64_t beta,
                               torch::Tensor params, bool rlr, double thresh,
                               double slr, bool want_lr) {
  check_bulyan(U, perm, theta, beta);
  check_vector(params, U, U.size(1), torch::kFloat32);
  int K = U.size(0);
  long n = U.size(1);
  auto lr = lr_buf(want_lr, n, U);
  launch_bulyan_rlr_apply(U.data_ptr<double>(), perm.data_ptr<int>(), K,
                          (int)theta, (int)beta, n, rlr ? 1 : 0, thresh, slr,
                          params.data_ptr<float>(),
                          want_lr ? lr.data_ptr<double>() : nullptr,
                          stream_of(U));
  return lr;
}

torch::Tensor pairwise_sqdist(torch::Tensor U) {
  check_matrix(U, pairdist_max_k());
  int K = U.size(0);
  long n = U.size(1);
  auto ws = torch::empty({pairdist_ws_doubles(K, n)}, U.options());
  auto D = torch::empty({K, K}, U.options());
  launch_pairwise_sqdist(U.data_ptr<double>(), K, n, ws.data_ptr<double>(),
                         D.data_ptr<double>(), stream_of(U));
  return D;
}

// idx: K row indices of H as a CPU int64 vector.  Checked HERE, on the host,
// to be in range and distinct, and only then uploaded: the kernels
// dereference the device copy as given.
static torch::Tensor upload_rows(const torch::Tensor& H,
                                 const torch::Tensor& idx, int64_t max_k) {
  CHK(H.is_cuda());
  CHK(H.dim() == 2);
  CHK(H.scalar_type() == torch::kFloat64);
  CHK(H.is_contiguous());
  CHK(H.size(0) >= 1 && H.size(1) >= 1);
  CHK(!idx.is_cuda());
  CHK(idx.scalar_type() == torch::kInt64);
  CHK(idx.dim() == 1 && idx.is_contiguous());
  const int64_t K = idx.numel();
  CHK(K >= 1 && K <= max_k && K <= H.size(0));
  const int64_t* p = idx.data_ptr<int64_t>();
  std::vector<char> seen(H.size(0), 0);
  for (int64_t k = 0; k < K; ++k) {
    TORCH_CHECK(p[k] >= 0 && p[k] < H.size(0), "row index ", p[k],
                " is outside [0, ", H.size(0), ")");
    TORCH_CHECK(!seen[p[k]], "row index ", p[k], " appears twice");
    seen[p[k]] = 1;
  }
  return idx.to(H.device());
}

// H[idx[k]] += U[k] in place, for distinct rows idx of the (A, n) history
void rows_add_(torch::Tensor H, torch::Tensor idx, torch::Tensor U) {
  auto rows = upload_rows(H, idx, INT32_MAX);
  check_matrix(U, INT32_MAX);
  CHK(U.device() == H.device());
  CHK(U.size(0) == idx.numel() && U.size(1) == H.size(1));
  launch_rows_add(H.data_ptr<double>(), (const long*)rows.data_ptr<int64_t>(),
                  U.data_ptr<double>(), (int)U.size(0), U.size(1),
                  stream_of(H));
}

// G (K, K) = Gram matrix of the rows idx of H, exactly symmetric
torch::Tensor gram_rows(torch::Tensor H, torch::Tensor idx) {
  auto rows = upload_rows(H, idx, pairdist_max_k());
  int K = idx.numel();
  long n = H.size(1);
  auto ws = torch::empty({pairdist_ws_doubles(K, n)}, H.options());
  auto G = torch::empty({K, K}, H.options());
  launch_gram_rows(H.data_ptr<double>(), (const long*)rows.data_ptr<int64_t>(),
                   K, n, ws.data_ptr<double>(), G.data_ptr<double>(),
                   stream_of(H));
  return G;
}

// FoolsGold's (alpha, cs) from the Gram matrix of the sampled history rows:
// cs the cosine matrix before pardoning, alpha the weights in [0, 1]
std::tuple<torch::Tensor, torch::Tensor> foolsgold_weights(torch::Tensor G,
                                                           double kappa) {
  check_matrix(G, foolsgold_max_k());
  CHK(G.size(0) == G.size(1));
  CHK(kappa > 0.0);
  int K = G.size(0);
  auto cs = torch::empty({K, K}, G.options());
  auto alpha = torch::empty({K}, G.options());
  launch_foolsgold_weights(G.data_ptr<double>(), K, kappa,
                           cs.data_ptr<double>(), alpha.data_ptr<double>(),
                           stream_of(G));
  return {alpha, cs};
}

// d2[k] = ||U_k - z||^2, z the weighted mean of the rows under a (K fp64)
torch::Tensor geomed_sqdist(torch::Tensor U, torch::Tensor a) {
  check_matrix(U, geomed_max_k());
  check_vector(a, U, U.size(0));
  int K = U.size(0);
  long n = U.size(1);
  auto ws = torch::empty({geomed_ws_doubles(K, n)}, U.options());
  auto d2 = torch::empty({K}, U.options());
  launch_geomed_sqdist(U.data_ptr<double>(), a.data_ptr<double>(), K, n,
                       ws.data_ptr<double>(), d2.data_ptr<double>(),
                       stream_of(U));
  return d2;
}

// (a, d2) after `iters` Weiszfeld updates from a = ones
std::tuple<torch::Tensor, torch::Tensor> geomed_weights(torch::Tensor U,
                                                        int64_t iters,
                                                        double nu) {
  check_matrix(U, geomed_max_k());
  CHK(iters >= 0);
  CHK(nu > 0.0);
  int K = U.size(0);
  long n = U.size(1);
  auto ws = torch::empty({geomed_ws_doubles(K, n)}, U.options());
  auto a = torch::empty({K}, U.options());
  auto d2 = torch::empty({K}, U.options());
  launch_geomed_weights(U.data_ptr<double>(), K, n, (int)iters, nu,
                        ws.data_ptr<double>(), a.data_ptr<double>(),
                        d2.data_ptr<double>(), stream_of(U));
  return {a, d2};
}

// the caller's workspace (at least rownorm_ws_doubles(K, n) doubles), or a
// fresh one of exactly that size
static torch::Tensor rowclip_ws(const torch::Tensor& U,
                                const c10::optional<torch::Tensor>& ws) {
  const long need = rownorm_ws_doubles((int)U.size(0), U.size(1));
  if (!ws.has_value()) return torch::empty({need}, U.options());
  const torch::Tensor& w = *ws;
  CHK(w.is_cuda() && w.device() == U.device());
  CHK(w.scalar_type() == torch::kFloat64);
  CHK(w.dim() == 1 && w.is_contiguous());
  CHK(w.numel() >= need);
  return w;
}

// stage 1 alone: the (chunks, K) partial sums of squares.  The row-norm
// entry points put no limit of their own on K.
torch::Tensor rownorm_partials(torch::Tensor U) {
  check_matrix(U, INT32_MAX);
  int K = U.size(0);
  long n = U.size(1);
  auto ws = torch::empty({(long)rownorm_chunks(K, n), (long)K}, U.options());
  launch_rownorm_partials(U.data_ptr<double>(), K, n, ws.data_ptr<double>(),
                          stream_of(U));
  return ws;
}

// norm[k] = ||U_k||_2
torch::Tensor row_norms(torch::Tensor U, c10::optional<torch::Tensor> ws) {
  check_matrix(U, INT32_MAX);
  int K = U.size(0);
  long n = U.size(1);
  auto w = rowclip_ws(U, ws);
  auto norm = torch::empty({K}, U.options());
  launch_row_norms(U.data_ptr<double>(), K, n, w.data_ptr<double>(),
                   norm.data_ptr<double>(), stream_of(U));
  return norm;
}

// U[k] *= s[k] in place; (s, norm, tau).  tau = value, or value * the lower
// median of the norms in median mode
std::tuple<torch::Tensor, torch::Tensor, torch::Tensor> rowclip_(
    torch::Tensor U, double value, bool median_mode,
    c10::optional<torch::Tensor> ws) {
  check_matrix(U, INT32_MAX);
  CHK(value >= 0.0);
  int K = U.size(0);
  long n = U.size(1);
  auto w = rowclip_ws(U, ws);
  auto norm = torch::empty({K}, U.options());
  auto scale = torch::empty({K}, U.options());
  auto tau = torch::empty({}, U.options());
  launch_rowclip(U.data_ptr<double>(), K, n, value, median_mode ? 1 : 0,
                 w.data_ptr<double>(), norm.data_ptr<double>(),
                 scale.data_ptr<double>(), tau.data_ptr<double>(),
                 stream_of(U));
  return {scale, norm, tau};
}

// lr is the per-coordinate rate, or empty (of any dtype) for the constant slr
void apply_update(torch::Tensor params, torch::Tensor agg, torch::Tensor lr,
                  double slr) {
  CHK(params.is_cuda());
  check_vector(params, params, params.numel(), torch::kFloat32);
  check_vector(agg, params, params.numel());
  if (lr.numel()) check_vector(lr, params, params.numel());
  launch_apply_update(params.data_ptr<float>(), agg.data_ptr<double>(),
                      lr.numel() ? lr.data_ptr<double>() : nullptr, slr,
                      params.numel(), stream_of(params));
}

// ------------------------------------------------------------ gemm/linear

// The fp32 GEMM driver with explicit operand layout: C (M,N) = op(A)
// op(B) (+bias, relu).  C is the caller-owned contiguous output when
// given (manual tape: a flat-grad view), freshly allocated otherwise.
static torch::Tensor gemm_f32(const torch::Tensor& A, const torch::Tensor& B,
                              c10::optional<torch::Tensor> bias, bool relu,
                              int M, int N, int K, int lda, int ldb,
                              int layout,
                              torch::Tensor C = torch::Tensor(),
                              StepQueue* q = nullptr) {
  if (!C.defined()) C = torch::empty({M, N}, A.options());
  int SK = gemm_f32_splitk(M, N, K);
  torch::Tensor ws;  // split-K slabs; none for SK == 1
  if (SK > 1)
    ws = torch::empty({gemm_splitk_ws_floats(M, N, SK)}, A.options());
  const float* bp = bias ? bias->data_ptr<float>() : nullptr;
  float* wsp = SK > 1 ? ws.data_ptr<float>() : nullptr;
  StepQueue now(true);
  StepQueue& sq = q ? *q : now;
  // main kernel now; the split-K combine goes to the queue when its form
  // has a role
  if (launch_gemm_f32_main(A.data_ptr<float>(), B.data_ptr<float>(),
                           C.data_ptr<float>(), bp, wsp, M, N, K, lda, ldb,
                           N, SK, relu ? 1 : 0, layout, stream_of(A)) &&
      !sq.splitk_reduce(ws, C, bias, M, N, N, SK, relu))
    launch_splitk_reduce(wsp, C.data_ptr<float>(), bp, M, N, N, SK,
                         relu ? 1 : 0, stream_of(A));
  return C;
}

torch::Tensor gemm(torch::Tensor A, torch::Tensor B,
                   c10::optional<torch::Tensor> bias, bool relu) {
  CHK_CUDA(A);
  CHK_CUDA(B);
  int M = A.size(0), K = A.size(1), N = B.size(1);
  CHK(B.size(0) == K);
  return gemm_f32(A, B, bias, relu, M, N, K, K, N, 0);
}

// bf16 GEMM: A (M,K) bf16, B (K,N) bf16 -> C fp32 (or bf16 if out_bf16)
torch::Tensor gemm_bf16(torch::Tensor A, torch::Tensor B,
                        c10::optional<torch::Tensor> bias, bool relu,
                        bool out_bf16) {
  TORCH_CHECK(A.is_cuda() && A.is_contiguous() && B.is_contiguous());
  TORCH_CHECK(A.scalar_type() == torch::kBFloat16 &&
              B.scalar_type() == torch::kBFloat16);
  int M = A.size(0), K = A.size(1), N = B.size(1);
  CHK(B.size(0) == K);
  int SK = gemm_f32_splitk(M, N, K);
  torch::Tensor ws;
  float* wsp = nullptr;
  if (SK > 1) {
    ws = torch::empty({gemm_splitk_ws_floats(M, N, SK)},
                      A.options().dtype(torch::kFloat));
    wsp = ws.data_ptr<float>();
  }
  const float* bp = bias ? bias->data_ptr<float>() : nullptr;
  torch::Tensor C;
  if (out_bf16 && SK == 1) {
    C = torch::empty({M, N}, A.options());
    launch_gemm_bf16(bfc(A), bfc(B), nullptr, bp, bfp(C), wsp, M, N, K, K,
                     N, N, SK, relu ? 1 : 0, stream_of(A));
  } else {
    C = torch::empty({M, N}, A.options().dtype(torch::kFloat));
    launch_gemm_bf16(bfc(A), bfc(B), C.data_ptr<float>(), bp, nullptr, wsp,
                     M, N, K, K, N, N, SK, relu ? 1 : 0, stream_of(A));
    if (out_bf16) C = C.to(torch::kBFloat16);
  }
  return C;
}


torch::Tensor linear_fwd(torch::Tensor x, torch::Tensor w,
                         c10::optional<torch::Tensor> b, bool relu) {
  // y = x @ w^T (+b); w is (out, in) — transpose once, then plain GEMM
  if (is_bf16(x)) {
    auto wt16 = w.t().contiguous().to(torch::kBFloat16);
    return gemm_bf16(x.contiguous(), wt16, b, relu, /*out_bf16=*/true);
  }
  // w (out,in) consumed directly as B^T (layout 2) — no transpose pass
  x = x.contiguous();
  w = w.contiguous();
  int M = x.size(0), K = x.size(1), N = w.size(0);
  return gemm_f32(x, w, b, relu, M, N, K, K, K, 2);
}

// manual-tape variant, fp32 only: dw/db written into caller-owned views
// (see conv2d_bwd_into below for the rationale).  dx = dY (M,out) @ W
// (out,in): plain NN, skipped (undefined) unless need_dx; dw = dY^T @ X:
// A = dY consumed transposed (layout 1); db = column sums of dY.
torch::Tensor linear_bwd_into(torch::Tensor x, torch::Tensor w,
                              torch::Tensor dy, torch::Tensor dw_out,
                              c10::optional<torch::Tensor> db_out,
                              bool need_dx, StepQueue* q = nullptr) {
  TORCH_CHECK(x.is_cuda() && !is_bf16(x));
  dy = dy.contiguous();
  x = x.contiguous();
  w = w.contiguous();
  int bM = x.size(0), in = x.size(1), out = w.size(0);
  TORCH_CHECK(dw_out.is_contiguous() && dw_out.numel() == (long)out * in);
  torch::Tensor dx;
  if (need_dx)
    dx = gemm_f32(dy, w, c10::nullopt, false, bM, in, out, out, in, 0);
  gemm_f32(dy, x, c10::nullopt, false, out, in, bM, out, in, 1, dw_out, q);
  if (db_out) {
    StepQueue now(true);
    (q ? *q : now).colsum(dy, *db_out);
  }
  return dx;
}

std::tuple<torch::Tensor, torch::Tensor, torch::Tensor> linear_bwd(
    torch::Tensor x, torch::Tensor w, torch::Tensor dy) {
  if (is_bf16(x)) {
    dy = dy.contiguous();
    auto w16 = w.to(torch::kBFloat16).contiguous();
    auto dx = gemm_bf16(dy, w16, c10::nullopt, false, /*out_bf16=*/true);
    auto dyt = dy.t().contiguous();
    auto dw = gemm_bf16(dyt, x.contiguous(), c10::nullopt, false, false);
    auto db = dy.to(torch::kFloat).sum(0);
    return {dx, dw, db};
  }
  auto dw = torch::empty({w.size(0), w.size(1)}, dy.options());
  auto db = torch::empty({w.size(0)}, dy.options());
  auto dx = linear_bwd_into(x, w, dy, dw, db, true, nullptr);
  return {dx, dw, db};
}

// ------------------------------------------------------------ fused tail
// (manual tape, fp32; see fused_tail.hip).  Each binding runs the unfused
// sequence it replaces when its predicate is false, so the result never
// depends on which path ran.

static const unsigned long long* dropout_state(const torch::Tensor& state) {
  CHK(state.scalar_type() == torch::kUInt64 ||
      state.scalar_type() == torch::kInt64);
  return (const unsigned long long*)state.data_ptr();
}

// maxpool2x2 + flatten (CHW order) + dropout of a channels_last a:
// -> (pooled, idx, d, mask)
std::tuple<torch::Tensor, torch::Tensor, torch::Tensor, torch::Tensor>
pool_flatten_dropout_fwd(torch::Tensor a, double p, torch::Tensor state,
                         int64_t site) {
  TORCH_CHECK(a.is_cuda() && a.dim() == 4 && !is_bf16(a));
  int Nb = a.size(0), C = a.size(1), H = a.size(2), W = a.size(3);
  if (!pool_seam_fused_ok(C, H, W)) {
    auto [pooled, idx] = maxpool2x2_fwd(a);
    auto [d, mask] = dropout_fwd_dev(nhwc_flatten(pooled), p, state, site);
    return {pooled, idx, d, mask};
  }
  a = cl(a, "seam_fwd.a");
  int OH = H / 2, OW = W / 2;
  auto pooled = empty_cl({Nb, C, OH, OW}, a.options());
  auto idx = empty_cl({Nb, C, OH, OW}, a.options().dtype(torch::kUInt8));
  auto d = torch::empty({Nb, (int64_t)C * OH * OW}, a.options());
  auto mask = torch::empty({Nb, (int64_t)C * OH * OW},
                           a.options().dtype(torch::kUInt8));
  launch_pool_flatten_dropout_fwd(
      a.data_ptr<float>(), pooled.data_ptr<float>(), idx.data_ptr<uint8_t>(),
      d.data_ptr<float>(), mask.data_ptr<uint8_t>(), Nb, H, W, C, (float)p,
      dropout_state(state), (int)site, stream_of(a));
  return {pooled, idx, d, mask};
}

// flatten (CHW order) + dropout of an already pooled channels_last image
// (conv2d_pool_fwd's): -> (d, mask), what pool_flatten_dropout_fwd returns
// for them
std::tuple<torch::Tensor, torch::Tensor> flatten_dropout_fwd(
    torch::Tensor pooled, double p, torch::Tensor state, int64_t site) {
  TORCH_CHECK(pooled.is_cuda() && pooled.dim() == 4 && !is_bf16(pooled));
  int Nb = pooled.size(0), C = pooled.size(1), OH = pooled.size(2),
      OW = pooled.size(3);
  if (!pool_seam_fused_ok(C, 2 * OH, 2 * OW))
    return dropout_fwd_dev(nhwc_flatten(pooled), p, state, site);
  pooled = cl(pooled, "seam_fwd.pooled");
  auto d = torch::empty({Nb, (int64_t)C * OH * OW}, pooled.options());
  auto mask = torch::empty({Nb, (int64_t)C * OH * OW},
                           pooled.options().dtype(torch::kUInt8));
  launch_flatten_dropout_fwd(pooled.data_ptr<float>(), d.data_ptr<float>(),
                             mask.data_ptr<uint8_t>(), Nb, OH, OW, C,
                             (float)p, dropout_state(state), (int)site,
                             stream_of(pooled));
  return {d, mask};
}

// dropout backward + unflatten + maxpool backward with the relu mask of
// the pooled values: g (B, C*OH*OW) -> dx, channels_last of x_shape
torch::Tensor dropout_unflatten_pool_bwd_relu(torch::Tensor g,
                                              torch::Tensor mask,
                                              torch::Tensor idx,
                                              torch::Tensor pooled, double p,
                                              std::vector<int64_t> x_shape) {
  TORCH_CHECK(g.is_cuda() && !is_bf16(g) && x_shape.size() == 4);
  int Nb = x_shape[0], C = x_shape[1], H = x_shape[2], W = x_shape[3];
  int OH = pooled.size(2), OW = pooled.size(3);
  TORCH_CHECK(OH == H / 2 && OW == W / 2 && pooled.size(1) == C &&
              g.numel() == (int64_t)Nb * C * OH * OW &&
              mask.numel() == g.numel() && idx.numel() == g.numel());
  if (!pool_seam_fused_ok(C, H, W)) {
    auto gu = nhwc_unflatten(dropout_bwd(g, mask, p), C, OH, OW);
    if ((C % 4) == 0) return maxpool2x2_bwd_relu(gu, idx, pooled, x_shape);
    // the relu-mask gather needs C % 4 == 0: mask through the pooled values
    // first (a select either way, so the order does not matter bitwise)
    return maxpool2x2_bwd(relu_bwd(pooled, gu), idx, x_shape);
  }
  g = g.contiguous();
  mask = mask.contiguous();
  idx = cl(idx, "seam_bwd.idx");
  pooled = cl(pooled, "seam_bwd.pooled");
  auto dx = empty_cl({Nb, C, H, W}, g.options());
  launch_dropout_unflatten_pool_bwd_relu(
      g.data_ptr<float>(), mask.data_ptr<uint8_t>(), idx.data_ptr<uint8_t>(),
      pooled.data_ptr<float>(), dx.data_ptr<float>(), Nb, H, W, C, (float)p,
      stream_of(g));
  return dx;
}

// The classifier head of a step: dropout(h1) -> fc -> mean CE, and back to
// the gradient of h1 (pre-dropout, relu-masked).  dw / db are written into
// the caller's flat-grad views.  -> (loss, g_h1)
std::tuple<torch::Tensor, torch::Tensor> fc_head_step(
    torch::Tensor h1, torch::Tensor w, torch::Tensor b, torch::Tensor labels,
    torch::Tensor dloss, double p, torch::Tensor state, int64_t site,
    torch::Tensor dw_out, torch::Tensor db_out, StepQueue* q = nullptr) {
  TORCH_CHECK(h1.is_cuda() && h1.dim() == 2 && !is_bf16(h1));
  int B = h1.size(0), H = h1.size(1), C = w.size(0);
  TORCH_CHECK(w.size(1) == H && b.numel() == C && labels.numel() == B);
  TORCH_CHECK(dw_out.is_contiguous() && dw_out.numel() == (int64_t)C * H &&
              db_out.is_contiguous() && db_out.numel() == C);
  if (!fc_head_fused_ok(B, H, C)) {
    auto [d2, m2] = dropout_fwd_dev(h1, p, state, site);
    auto out = linear_fwd(d2, w, b, false);
    auto [loss, softmax] = cross_entropy_fwd(out, labels);
    auto g = cross_entropy_bwd(softmax, labels, dloss);
    g = linear_bwd_into(d2, w, g, dw_out, db_out, true, q);
    return {loss, dropout_relu_bwd(g, m2, h1, p)};
  }
  h1 = h1.contiguous();
  w = w.contiguous();
  b = b.contiguous();
  labels = labels.contiguous();
  auto dl = dloss.to(h1.device()).contiguous();
  auto ws = torch::empty({fc_head_ws_floats(B, H, C)}, h1.options());
  auto g_h1 = torch::empty_like(h1);
  auto loss = torch::empty({}, h1.options());
  // stage A now, stage B as a level-1 role
  launch_fc_head_rows(h1.data_ptr<float>(), w.data_ptr<float>(),
                      b.data_ptr<float>(), labels.data_ptr<int64_t>(),
                      dl.data_ptr<float>(), ws.data_ptr<float>(),
                      g_h1.data_ptr<float>(), B, H, C, (float)p,
                      dropout_state(state), (int)site, stream_of(h1));
  StepQueue now(true);
  StepQueue& sq = q ? *q : now;
  sq.hold(ws); sq.hold(dw_out); sq.hold(db_out); sq.hold(loss);
  sq.push(0, fc_head_reduce_role(ws.data_ptr<float>(),
                                 dw_out.data_ptr<float>(),
                                 db_out.data_ptr<float>(),
                                 loss.data_ptr<float>(), B, H, C));
  return {loss, g_h1};
}

// ------------------------------------------------------------------ conv

torch::Tensor conv2d_fwd(torch::Tensor x, torch::Tensor w,
                         c10::optional<torch::Tensor> b, int64_t stride,
                         int64_t pad, bool relu,
                         c10::optional<torch::Tensor> wt_in = c10::nullopt) {
  TORCH_CHECK(x.is_cuda() && w.is_cuda());
  // wt_in: the fp32 forward's permuted weights (StepQueue::wperm kind 0),
  // made once per step by the caller instead of per call here
  TORCH_CHECK(!wt_in || !is_bf16(x), "pre-permuted weights are fp32-only");
  x = cl(x, "conv_fwd.x");
  w = w.contiguous();
  int Nb = x.size(0), C = x.size(1), H = x.size(2), W = x.size(3);
  int Kout = w.size(0), R = w.size(2), S = w.size(3);
  int OH = (H + 2 * pad - R) / stride + 1;
  int OW = (W + 2 * pad - S) / stride + 1;
  const float* bp = b ? b->data_ptr<float>() : nullptr;
  if (is_bf16(x)) {
    if ((C % 32) == 0) {
      auto wt = torch::empty({(long)C * R * S, Kout},
                             w.options().dtype(torch::kBFloat16));
      launch_wperm_rsc_ko_bf16(w.data_ptr<float>(), bfp(wt), Kout, C, R * S,
                               stream_of(x));
      auto y = empty_cl({Nb, Kout, OH, OW}, x.options());
      if (conv_tap_fwd_w4_ok(C, H, W, Kout, R, S, (int)stride, (int)pad))
        launch_conv_tap_fwd_w4_bf16(bfc(x), bfc(wt), bp, bfp(y),
                                    nullptr, Nb, C, Kout, relu ? 1 : 0, 0,
                                    stream_of(x));
      else if (conv_tap_fwd_ok(C, H, W, Kout, R, S, (int)stride, (int)pad))
        launch_conv_tap_fwd_bf16(bfc(x), bfc(wt), bp, bfp(y),
                                 nullptr, Nb, C, H, W, Kout, relu ? 1 : 0, 0,
                                 stream_of(x));
      else
        launch_conv_fwd_bf16(bfc(x), bfc(wt), bp, bfp(y), Nb, C, H,
                             W, Kout, R, S, OH, OW, (int)stride, (int)pad,
                             relu ? 1 : 0, stream_of(x));
      return y;
    }
    // first-layer fallback (C=1,3): fp32 kernels, bf16 in/out casts
    auto y32 = conv2d_fwd(x.to(torch::kFloat), w, b, stride, pad, relu,
                          c10::nullopt);
    return y32.to(torch::kBFloat16);
  }
  torch::Tensor wt;
  if (wt_in) {
    wt = *wt_in;
    TORCH_CHECK(wt.is_cuda() && wt.is_contiguous() &&
                wt.scalar_type() == torch::kFloat &&
                wt.numel() == w.numel());
  } else {
    wt = StepQueue(true).wperm(w, 0);
  }
  auto y = empty_cl({Nb, Kout, OH, OW}, x.options());
  launch_conv_fwd(x.data_ptr<float>(), wt.data_ptr<float>(), bp,
                  y.data_ptr<float>(), Nb, C, H, W, Kout, R, S, OH, OW,
                  (int)stride, (int)pad, relu ? 1 : 0, stream_of(x));
  return y;
}

// conv + bias + relu + maxpool2x2 (fp32): -> (pooled, idx), what
// maxpool2x2_fwd(conv2d_fwd(..., relu=true)) returns.  One kernel where
// conv_pool_fused_ok, the two launches otherwise.
std::tuple<torch::Tensor, torch::Tensor> conv2d_pool_fwd(
    torch::Tensor x, torch::Tensor w, c10::optional<torch::Tensor> b,
    int64_t stride, int64_t pad,
    c10::optional<torch::Tensor> wt_in = c10::nullopt) {
  TORCH_CHECK(x.is_cuda() && w.is_cuda() && x.dim() == 4 && w.dim() == 4);
  int Nb = x.size(0), C = x.size(1), H = x.size(2), W = x.size(3);
  int Kout = w.size(0), R = w.size(2), S = w.size(3);
  if (is_bf16(x) ||
      !conv_pool_fused_ok(C, H, W, Kout, R, S, (int)stride, (int)pad))
    return maxpool2x2_fwd(conv2d_fwd(x, w, b, stride, pad, true, wt_in));
  x = cl(x, "conv_pool_fwd.x");
  w = w.contiguous();
  TORCH_CHECK(w.size(1) == C && (!b || b->numel() == Kout));
  const float* bp = b ? b->data_ptr<float>() : nullptr;
  torch::Tensor wt;
  if (wt_in) {
    wt = *wt_in;
    TORCH_CHECK(wt.is_cuda() && wt.is_contiguous() &&
                wt.scalar_type() == torch::kFloat &&
                wt.numel() == w.numel());
  } else {
    wt = StepQueue(true).wperm(w, 0);
  }
  int PH = (H - R + 1) / 2, PW = (W - S + 1) / 2;
  auto pooled = empty_cl({Nb, Kout, PH, PW}, x.options());
  auto idx = empty_cl({Nb, Kout, PH, PW}, x.options().dtype(torch::kUInt8));
  launch_conv_pool_fwd(x.data_ptr<float>(), wt.data_ptr<float>(), bp,
                       pooled.data_ptr<float>(), idx.data_ptr<uint8_t>(), Nb,
                       C, H, W, Kout, R, S, stream_of(x));
  return {pooled, idx};
}


// bf16 dw dispatch: tap-accumulator kernel for the 3x3 p1 ResNet shapes
// (single-pass streaming; s1 and s2 forms share the launch plan and the
// workspace), implicit-GEMM split-K otherwise
static void bf16_dw(const torch::Tensor& dy, const torch::Tensor& x,
                    torch::Tensor& dw_target, const torch::Tensor& w,
                    int Nb, int C, int H, int W, int Kout, int R, int S,
                    int stride, int pad, void* st) {
  auto f32 = w.options().dtype(torch::kFloat);
  bool tap_s1 = conv_bwdw_tap_ok(C, H, W, Kout, R, S, stride, pad);
  if (tap_s1 || conv_bwdw_tap_s2_ok(C, H, W, Kout, R, S, stride, pad)) {
    int SL = conv_bwdw_tap_ws_slabs(Nb, C, Kout, nullptr, nullptr, nullptr);
    auto ws = torch::empty({(long)SL * Kout * C * 9}, f32);
    auto launch = tap_s1 ? launch_conv_bwdw_tap_bf16
                         : launch_conv_bwdw_tap_s2_bf16;
    launch(bfc(dy), bfc(x), dw_target.data_ptr<float>(),
           ws.data_ptr<float>(), Nb, C, H, W, Kout, st);
    return;
  }
  int Ncrs = C * R * S;
  int OH = dy.size(2), OW = dy.size(3);
  long Kd = (long)Nb * OH * OW;
  int SK = conv_bwd_weight_bf16_splitk(Kout, Ncrs, Kd);
  auto ws = torch::empty({conv_dwperm_ws_floats(Kout, Ncrs, SK)}, f32);
  launch_conv_bwd_weight_bf16(bfc(dy), bfc(x), dw_target.data_ptr<float>(),
                              ws.data_ptr<float>(), SK, Nb, C, H, W, Kout,
                              R, S, OH, OW, stride, pad, st);
}

// The one conv backward, fp32 and bf16: returns dx (undefined unless
// need_dx, masked by relu_y > 0 when relu_y is given), writes dw into
// dw_out and, when db_out is given, the bias gradient into it.  Thin bf16
// layers (the first conv: C = 1, 3) run the fp32 kernels on casts.
static torch::Tensor conv_bwd_core(torch::Tensor x, torch::Tensor w,
                                   torch::Tensor dy, int64_t stride,
                                   int64_t pad, bool need_dx,
                                   torch::Tensor dw_out,
                                   c10::optional<torch::Tensor> db_out,
                                   c10::optional<torch::Tensor> relu_y,
                                   c10::optional<torch::Tensor> wp_in =
                                       c10::nullopt,
                                   StepQueue* q = nullptr) {
  // wp_in (fp32): bwd-data's permuted weights, made once per step by the
  // caller (StepQueue::wperm kind 1).  q (fp32): the dw combine and the
  // bias-gradient fold wait on the queue instead of running here.
  StepQueue now(true);
  StepQueue& sq = q ? *q : now;
  TORCH_CHECK((!wp_in && !q) || !is_bf16(x),
              "pre-permuted weights and the step queue are fp32-only");
  x = cl(x, "conv_bwd.x");
  w = w.contiguous();
  dy = cl(dy, "conv_bwd.dy");
  int Nb = x.size(0), C = x.size(1), H = x.size(2), W = x.size(3);
  int Kout = w.size(0), R = w.size(2), S = w.size(3);
  int OH = dy.size(2), OW = dy.size(3);
  int st_ = (int)stride, pd = (int)pad;
  auto st = stream_of(x);
  const bool bf = is_bf16(x);
  if (bf && !((Kout % 32) == 0 && (C % 8) == 0)) {
    auto dx32 = conv_bwd_core(
        x.to(torch::kFloat), w, dy.to(torch::kFloat), stride, pad, need_dx,
        dw_out, db_out,
        relu_y ? c10::optional<torch::Tensor>(relu_y->to(torch::kFloat))
               : c10::nullopt);
    return dx32.defined() ? dx32.to(torch::kBFloat16) : dx32;
  }

  torch::Tensor dx;
  if (need_dx) {
    torch::Tensor wp;
    if (wp_in) {
      wp = *wp_in;
      TORCH_CHECK(wp.is_cuda() && wp.is_contiguous() &&
                  wp.scalar_type() == torch::kFloat &&
                  wp.numel() == w.numel());
    } else if (bf) {
      wp = torch::empty({(long)Kout * R * S, C},
                        w.options().dtype(torch::kBFloat16));
      launch_wperm_rsko_c_bf16(w.data_ptr<float>(), bfp(wp), Kout, C, R * S,
                               st);
    } else {
      wp = now.wperm(w, 1);  // bwd-data below reads it: never deferred
    }
    dx = empty_cl({Nb, C, H, W}, x.options());
    torch::Tensor ryt;
    if (relu_y) ryt = cl(*relu_y, "conv_bwd.relu_y");
    if (!bf) {
      launch_conv_bwd_data_relu(
          dy.data_ptr<float>(), wp.data_ptr<float>(), dx.data_ptr<float>(),
          relu_y ? ryt.data_ptr<float>() : nullptr, Nb, C, H, W, Kout, R, S,
          OH, OW, st_, pd, st);
    } else {
      const unsigned short* ry = relu_y ? bfc(ryt) : nullptr;
      if (conv_tap_fwd_w4_ok(Kout, H, W, C, R, S, st_, pd))
        launch_conv_tap_fwd_w4_bf16(bfc(dy), bfc(wp), nullptr, bfp(dx), ry,
                                    Nb, Kout, C, 0, 1, st);
      else if (conv_tap_fwd_ok(Kout, H, W, C, R, S, st_, pd))
        // bwd-data == the same correlation over dy with flipped taps
        launch_conv_tap_fwd_bf16(bfc(dy), bfc(wp), nullptr, bfp(dx), ry, Nb,
                                 Kout, H, W, C, 0, 1, st);
      else if (conv_tap_bwdd_s2_ok(C, H, W, Kout, R, S, st_, pd))
        launch_conv_tap_bwdd_s2_bf16(bfc(dy), bfc(wp), bfp(dx), ry, Nb, Kout,
                                     H, W, C, st);
      else
        launch_conv_bwd_data_bf16_relu(bfc(dy), bfc(wp), bfp(dx), ry, Nb, C,
                                       H, W, Kout, R, S, OH, OW, st_, pd,
                                       st);
    }
  }

  if (bf) {
    bf16_dw(dy, x, dw_out, w, Nb, C, H, W, Kout, R, S, st_, pd, st);
  } else {
    int Ncrs = C * R * S;
    long Kdim = (long)Nb * OH * OW;
    int SK = conv_bwd_weight_splitk(Kout, Ncrs, Kdim);
    auto ws = torch::empty({conv_bwd_weight_ws_floats(Kout, Ncrs, SK)},
                           w.options());
    launch_conv_bwd_weight_main(dy.data_ptr<float>(), x.data_ptr<float>(),
                                ws.data_ptr<float>(), SK, Nb, C, H, W, Kout,
                                R, S, OH, OW, st_, pd, st);
    sq.conv_bwd_weight_combine(ws, dw_out, SK, Nb, C, Kout, R, S, OH, OW);
  }

  if (db_out) {
    TORCH_CHECK(db_out->is_contiguous() && db_out->numel() == Kout);
    if (bf) {
      auto parts = torch::empty({conv_db_ws_floats(Kout)}, w.options());
      launch_conv_db_bf16(bfc(dy), db_out->data_ptr<float>(),
                          parts.data_ptr<float>(), Nb, Kout, OH * OW, st);
    } else {
      sq.conv_db(dy, *db_out);
    }
  }
  return dx;
}

std::tuple<torch::Tensor, torch::Tensor, torch::Tensor> conv2d_bwd(
    torch::Tensor x, torch::Tensor w, torch::Tensor dy, int64_t stride,
    int64_t pad, bool has_b, bool need_dx) {
  TORCH_CHECK(x.is_cuda());
  w = w.contiguous();
  auto dw = torch::empty_like(w);
  torch::Tensor db;
  if (has_b) db = torch::empty({w.size(0)}, w.options());
  auto dx = conv_bwd_core(
      x, w, dy, stride, pad, need_dx, dw,
      has_b ? c10::optional<torch::Tensor>(db) : c10::nullopt, c10::nullopt);
  return {dx, dw, db};
}

// ---- manual-tape backward: grads land DIRECTLY in caller-owned views ----
// Used by engine.ManualTape (the hand-rolled training step): with the
// weight/bias gradients written straight into their flat_grads slices,
// autograd's per-param accumulate-add and the zero-grad fill disappear.
// Assignment into the view is bitwise-identical to autograd's
// accumulate-into-zeroed-grad.  fp32 only.

torch::Tensor conv2d_bwd_into(torch::Tensor x, torch::Tensor w,
                              torch::Tensor dy, int64_t stride, int64_t pad,
                              bool need_dx, torch::Tensor dw_out,
                              c10::optional<torch::Tensor> db_out,
                              c10::optional<torch::Tensor> relu_y,
                              c10::optional<torch::Tensor> wp = c10::nullopt,
                              StepQueue* q = nullptr) {
  TORCH_CHECK(x.is_cuda() && !is_bf16(x));
  TORCH_CHECK(dw_out.is_contiguous() && dw_out.numel() == w.numel());
  return conv_bwd_core(x, w, dy, stride, pad, need_dx, dw_out, db_out,
                       relu_y, wp, q);
}

// bf16/fp32 conv backward with dw written into a caller-owned view and
// no bias (the ResNet tape: conv layers are bias-free).
torch::Tensor conv2d_bwd_wdx_into(torch::Tensor x, torch::Tensor w,
                                  torch::Tensor dy, int64_t stride,
                                  int64_t pad, bool need_dx,
                                  torch::Tensor dw_out,
                                  c10::optional<torch::Tensor> relu_y) {
  TORCH_CHECK(x.is_cuda());
  TORCH_CHECK(dw_out.is_contiguous() && dw_out.numel() == w.numel());
  return conv_bwd_core(x, w, dy, stride, pad, need_dx, dw_out, c10::nullopt,
                       relu_y);
}

// ------------------------------------------------------------- batchnorm

std::tuple<torch::Tensor, torch::Tensor, torch::Tensor> batchnorm_fwd(
    torch::Tensor x, torch::Tensor w, torch::Tensor b,
    torch::Tensor running_mean, torch::Tensor running_var, double momentum,
    double eps, bool training, bool relu) {
  TORCH_CHECK(x.is_cuda());
  x = cl(x, "bn_fwd.x");
  int Nb = x.size(0), C = x.size(1), HW = x.size(2) * x.size(3);
  auto y = empty_cl({x.size(0), x.size(1), x.size(2), x.size(3)},
                    x.options());
  auto save_mean = torch::empty({C}, x.options().dtype(torch::kFloat));
  auto save_rstd = torch::empty({C}, x.options().dtype(torch::kFloat));
  auto scratch = torch::empty({(long)bn_scratch_floats(C)},
                              x.options().dtype(torch::kFloat));
  if (is_bf16(x))
    launch_bn_fwd_bf16(bfc(x), w.data_ptr<float>(), b.data_ptr<float>(),
                       running_mean.data_ptr<float>(),
                       running_var.data_ptr<float>(),
                       save_mean.data_ptr<float>(),
                       save_rstd.data_ptr<float>(), bfp(y),
                       scratch.data_ptr<float>(), Nb, C, HW,
                       (float)momentum, (float)eps, training ? 1 : 0,
                       relu ? 1 : 0, stream_of(x));
  else
    launch_bn_fwd(x.data_ptr<float>(), w.data_ptr<float>(),
                  b.data_ptr<float>(), running_mean.data_ptr<float>(),
                  running_var.data_ptr<float>(),
                  save_mean.data_ptr<float>(), save_rstd.data_ptr<float>(),
                  y.data_ptr<float>(), scratch.data_ptr<float>(), Nb, C,
                  HW, (float)momentum, (float)eps, training ? 1 : 0,
                  relu ? 1 : 0, stream_of(x));
  return {y, save_mean, save_rstd};
}

// dw/db written into caller-owned tensors (manual tape: flat-grad views)
torch::Tensor batchnorm_bwd_into(torch::Tensor x, torch::Tensor w,
                                 torch::Tensor save_mean,
                                 torch::Tensor save_rstd, torch::Tensor dy,
                                 torch::Tensor dw_out, torch::Tensor db_out) {
  TORCH_CHECK(x.is_cuda());
  x = cl(x, "bn_bwd.x");
  dy = cl(dy, "bn_bwd.dy");
  int Nb = x.size(0), C = x.size(1), HW = x.size(2) * x.size(3);
  TORCH_CHECK(dw_out.is_contiguous() && dw_out.numel() == C);
  TORCH_CHECK(db_out.is_contiguous() && db_out.numel() == C);
  auto dx = empty_cl({x.size(0), x.size(1), x.size(2), x.size(3)},
                     x.options());
  auto scratch = torch::empty({(long)bn_scratch_floats(C)},
                              x.options().dtype(torch::kFloat));
  if (is_bf16(x))
    launch_bn_bwd_bf16(bfc(x), bfc(dy), w.data_ptr<float>(),
                       save_mean.data_ptr<float>(),
                       save_rstd.data_ptr<float>(),
                       scratch.data_ptr<float>(), bfp(dx),
                       dw_out.data_ptr<float>(), db_out.data_ptr<float>(),
                       Nb, C, HW, 1, stream_of(x));
  else
    launch_bn_bwd(x.data_ptr<float>(), dy.data_ptr<float>(),
                  w.data_ptr<float>(), save_mean.data_ptr<float>(),
                  save_rstd.data_ptr<float>(), scratch.data_ptr<float>(),
                  dx.data_ptr<float>(), dw_out.data_ptr<float>(),
                  db_out.data_ptr<float>(), Nb, C, HW, 1, stream_of(x));
  return dx;
}

std::tuple<torch::Tensor, torch::Tensor, torch::Tensor> batchnorm_bwd(
    torch::Tensor x, torch::Tensor w, torch::Tensor save_mean,
    torch::Tensor save_rstd, torch::Tensor dy) {
  auto f32 = x.options().dtype(torch::kFloat);
  auto dw = torch::empty({x.size(1)}, f32);
  auto db = torch::empty({x.size(1)}, f32);
  auto dx = batchnorm_bwd_into(x, w, save_mean, save_rstd, dy, dw, db);
  return {dx, dw, db};
}

// ---------------------------------------------------------------- poison

void poison_set_u8(torch::Tensor data, torch::Tensor idxs,
                   torch::Tensor coords, int64_t value) {
  CHK_CUDA(data);
  int H = data.size(1), W = data.size(2);
  int C = data.dim() == 4 ? data.size(3) : 1;
  launch_poison_set_u8(data.data_ptr<uint8_t>(), idxs.data_ptr<int64_t>(),
                       idxs.numel(), coords.data_ptr<int>(),
                       coords.size(0), H, W, C, (int)value, stream_of(data));
}

void poison_set_f32(torch::Tensor data, torch::Tensor idxs,
                    torch::Tensor coords, double value) {
  CHK_CUDA(data);
  // (B,1,H,W) float
  int H = data.size(2), W = data.size(3);
  launch_poison_set_f32(data.data_ptr<float>(), idxs.data_ptr<int64_t>(),
                        idxs.numel(), coords.data_ptr<int>(),
                        coords.size(0), H, W, (float)value, stream_of(data));
}

void poison_addwrap_u8(torch::Tensor data, torch::Tensor idxs,
                       torch::Tensor mask) {
  CHK_CUDA(data);
  launch_poison_addwrap_u8(data.data_ptr<uint8_t>(),
                           idxs.data_ptr<int64_t>(), idxs.numel(),
                           mask.data_ptr<uint8_t>(),
                           data.size(1) * data.size(2), stream_of(data));
}

void poison_subf(torch::Tensor data, torch::Tensor idxs,
                 torch::Tensor mask) {
  CHK_CUDA(data);
  long HW = data.numel() / data.size(0);
  launch_poison_subf(data.data_ptr<float>(), idxs.data_ptr<int64_t>(),
                     idxs.numel(), mask.data_ptr<uint8_t>(), (int)HW,
                     stream_of(data));
}

torch::Tensor normalize_u8(torch::Tensor raw, torch::Tensor mean,
                           torch::Tensor stdv) {
  TORCH_CHECK(raw.is_cuda() && raw.is_contiguous());
  long B = raw.size(0);
  int H = raw.size(1), W = raw.size(2);
  int C = raw.dim() == 4 ? raw.size(3) : 1;
  // raw is HWC; output storage is NHWC = channels_last of (B,C,H,W)
  auto out = empty_cl({B, C, H, W}, raw.options().dtype(torch::kFloat32));
  launch_normalize_u8(raw.data_ptr<uint8_t>(), out.data_ptr<float>(), B, H,
                      W, C, mean.data_ptr<float>(), stdv.data_ptr<float>(),
                      stream_of(raw));
  return out;
}

// ------------------------------------------------------------ step batch

// One launch for every conv weight permute of a step: (weight, kind) pairs,
// kind 0 = the forward's wt, 1 = bwd-data's wp (StepQueue::wperm).  Valid
// until the weights next change (the optimizer kernels at the step's end).
std::vector<torch::Tensor> prep_conv_weights(
    std::vector<std::pair<torch::Tensor, int64_t>> items) {
  StepQueue q;
  std::vector<torch::Tensor> out;
  out.reserve(items.size());
  for (auto& it : items) out.push_back(q.wperm(it.first, it.second));
  q.flush();
  return out;
}

// The step's feed in one launch: out_x = X[sel], out_y = Y[sel] (dim 0);
// sel must index the rows of X and Y (StepQueue::gather_rows).
void feed_gather(torch::Tensor X, torch::Tensor Y, torch::Tensor sel,
                 torch::Tensor out_x, torch::Tensor out_y) {
  StepQueue q;
  q.gather_rows(X, sel, out_x);
  q.gather_rows(Y, sel, out_y);
  q.flush();
}

// Each role alone, one binding each, so a test can hold a role in a batch
// against the same role run by itself: the output allocated here, the
// StepQueue method of the same name on an immediate queue.
torch::Tensor conv_db(torch::Tensor dy) {
  TORCH_CHECK(dy.is_cuda() && dy.dim() == 4 && !is_bf16(dy));
  dy = cl(dy, "conv_db.dy");
  auto db = torch::empty({dy.size(1)}, dy.options());
  StepQueue(true).conv_db(dy, db);
  return db;
}

torch::Tensor splitk_reduce_dwperm(torch::Tensor ws, int64_t Kout, int64_t C,
                                   int64_t RS, int64_t SK) {
  CHK_CUDA(ws);
  TORCH_CHECK(ws.numel() >= conv_dwperm_ws_floats(Kout, C * RS, SK));
  auto dw = torch::empty({Kout * C * RS}, ws.options());
  StepQueue(true).splitk_reduce_dwperm(ws, dw, Kout, C, RS, SK, 0);
  return dw;
}

torch::Tensor splitk_reduce(torch::Tensor ws, int64_t M, int64_t N,
                            int64_t SK) {
  CHK_CUDA(ws);
  TORCH_CHECK(ws.numel() >= gemm_splitk_ws_floats(M, N, SK));
  auto C = torch::empty({M, N}, ws.options());
  if (!StepQueue(true).splitk_reduce(ws, C, c10::nullopt, M, N, N, SK, false))
    launch_splitk_reduce(ws.data_ptr<float>(), C.data_ptr<float>(), nullptr,
                         (int)M, (int)N, (int)N, (int)SK, 0, stream_of(ws));
  return C;
}

// chunk partials of a (C*R*S <= 32) layer's backward-weight -> dw
torch::Tensor conv_small_bwdw_reduce(torch::Tensor partials, int64_t Nb,
                                     int64_t C, int64_t Kout, int64_t R,
                                     int64_t S, int64_t OH, int64_t OW) {
  CHK_CUDA(partials);
  auto dw = torch::empty({Kout * C * R * S}, partials.options());
  StepQueue(true).conv_small_bwdw_reduce(partials, dw, Nb, C, Kout, R, S, OH,
                                         OW);
  return dw;
}

torch::Tensor colsum(torch::Tensor dy) {
  CHK_CUDA(dy);
  TORCH_CHECK(dy.dim() == 2);
  auto db = torch::empty({dy.size(1)}, dy.options());
  StepQueue(true).colsum(dy, db);
  return db;
}

torch::Tensor wperm(torch::Tensor w, int64_t kind) {
  TORCH_CHECK(w.is_cuda());
  return StepQueue(true).wperm(w, kind);
}

// (first block of each role, total blocks) of a batched launch
std::tuple<std::vector<int64_t>, int64_t> step_batch_plan_py(
    std::vector<int64_t> counts) {
  std::vector<int> c(counts.begin(), counts.end()), f(counts.size());
  int total = step_batch_plan(c.data(), (int)c.size(), f.data());
  return {std::vector<int64_t>(f.begin(), f.end()), (int64_t)total};
}

// (role, block inside the role) that flat block `block` runs; role -1: none
std::tuple<int64_t, int64_t> step_batch_lookup_py(std::vector<int64_t> counts,
                                                  int64_t block) {
  std::vector<int> c(counts.begin(), counts.end());
  int v = -1;
  int r = step_batch_lookup(c.data(), (int)c.size(), (int)block, &v);
  return {(int64_t)r, (int64_t)(r < 0 ? -1 : v)};
}

}  // namespace

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
  m.def("relu_fwd", &relu_fwd);
  m.def("relu_bwd", &relu_bwd);
  m.def("add_relu_fwd", &add_relu_fwd);
  m.def("maxpool2x2_fwd", &maxpool2x2_fwd);
  m.def("maxpool2x2_bwd", &maxpool2x2_bwd);
  m.def("dropout_fwd", &dropout_fwd);
  m.def("dropout_fwd_dev", &dropout_fwd_dev);
  m.def("dropout_bwd", &dropout_bwd);
  m.def("gap_fwd", &gap_fwd);
  m.def("gap_bwd", &gap_bwd);
  m.def("cross_entropy_fwd", &cross_entropy_fwd);
  m.def("cross_entropy_bwd", &cross_entropy_bwd);
  m.def("eval_update", &eval_update);
  m.def("clipped_sgd_step", &clipped_sgd_step);
  m.def("pgd_project", &pgd_project);
  m.def("delta64", &delta64);
  m.def("gather_grads", &gather_grads);
  m.def("fused_avg_rlr_apply", &fused_avg_rlr_apply, py::arg("U"),
        py::arg("w"), py::arg("params"), py::arg("rlr"), py::arg("thresh"),
        py::arg("slr"), py::arg("noise_std"), py::arg("seed"),
        py::arg("offset"), py::arg("want_lr"), py::arg("divisor") = 0.0);
  m.def("rlr_vote", &rlr_vote);
  m.def("agg_avg", &agg_avg, py::arg("U"), py::arg("w"),
        py::arg("divisor") = 0.0);
  m.def("agg_sign", &agg_sign);
  m.def("agg_comed", &agg_comed);
  m.def("apply_update", &apply_update);
  m.def("agg_orderstat", &agg_orderstat);
  m.def("orderstat_rlr_apply", &orderstat_rlr_apply);
  m.def("orderstat_max_k", &orderstat_max_k);
  m.def("bulyan_trim", &bulyan_trim);
  m.def("bulyan_rlr_apply", &bulyan_rlr_apply);
  m.def("bulyan_max_k", &bulyan_max_k);
  m.def("pairwise_sqdist", &pairwise_sqdist);
  m.def("pairdist_max_k", &pairdist_max_k);
  m.def("pairdist_chunks", &pairdist_chunks);
  m.def("pairdist_ws_doubles", &pairdist_ws_doubles);
  m.def("rows_add_", &rows_add_);
  m.def("gram_rows", &gram_rows);
  m.def("foolsgold_weights", &foolsgold_weights);
  m.def("foolsgold_max_k", &foolsgold_max_k);
  m.def("geomed_sqdist", &geomed_sqdist);
  m.def("geomed_weights", &geomed_weights);
  m.def("geomed_max_k", &geomed_max_k);
  m.def("geomed_chunks", &geomed_chunks);
  m.def("geomed_ws_doubles", &geomed_ws_doubles);
  m.def("rownorm_partials", &rownorm_partials);
  m.def("row_norms", &row_norms, py::arg("U"), py::arg("ws") = py::none());
  m.def("rowclip_", &rowclip_, py::arg("U"), py::arg("value"),
        py::arg("median_mode"), py::arg("ws") = py::none());
  m.def("rownorm_chunks", &rownorm_chunks);
  m.def("rownorm_ws_doubles", &rownorm_ws_doubles);
  m.def("gemm", &gemm);
  m.def("gemm_bf16", &gemm_bf16);
  m.def("nhwc_flatten", &nhwc_flatten);
  m.def("nhwc_unflatten", &nhwc_unflatten);
  m.def("linear_fwd", &linear_fwd);
  m.def("linear_bwd", &linear_bwd);
  m.def("conv2d_fwd", &conv2d_fwd, py::arg("x"), py::arg("w"), py::arg("b"),
        py::arg("stride"), py::arg("pad"), py::arg("relu"),
        py::arg("wt") = py::none());
  m.def("conv2d_pool_fwd", &conv2d_pool_fwd, py::arg("x"), py::arg("w"),
        py::arg("b"), py::arg("stride"), py::arg("pad"),
        py::arg("wt") = py::none());
  m.def("conv_pool_fused_ok", &conv_pool_fused_ok);
  // -> (tile_rows, tiles, mi, lds_rows, lds_bytes)
  m.def("conv_fwd_res_plan", [](int C, int H, int W, int OH, int OW, int R) {
    ConvFwdResPlan p = conv_fwd_res_plan(C, H, W, OH, OW, R);
    return std::make_tuple(p.tile_rows, p.tiles, p.mi, p.lds_rows,
                           p.lds_bytes);
  });
  m.def("conv2d_bwd", &conv2d_bwd);
  m.def("conv2d_bwd_into", &conv2d_bwd_into, py::arg("x"), py::arg("w"),
        py::arg("dy"), py::arg("stride"), py::arg("pad"), py::arg("need_dx"),
        py::arg("dw_out"), py::arg("db_out"), py::arg("relu_y"),
        py::arg("wp") = py::none(), py::arg("queue") = py::none());
  m.def("linear_bwd_into", &linear_bwd_into, py::arg("x"), py::arg("w"),
        py::arg("dy"), py::arg("dw_out"), py::arg("db_out"),
        py::arg("need_dx"), py::arg("queue") = py::none());
  m.def("dropout_relu_bwd", &dropout_relu_bwd);
  m.def("batchnorm_bwd_into", &batchnorm_bwd_into);
  m.def("conv2d_bwd_wdx_into", &conv2d_bwd_wdx_into);
  // host arithmetic only, exported so a test without a GPU can pin it:
  // the split-K pickers and the workspace size (in floats) each op
  // allocates for its launcher
  m.def("gemm_f32_splitk", &gemm_f32_splitk);
  m.def("gemm_f32_shortk_tiles", &gemm_f32_shortk_tiles);
  m.def("conv_bwd_weight_splitk", &conv_bwd_weight_splitk);
  m.def("conv_bwd_weight_bf16_splitk", &conv_bwd_weight_bf16_splitk);
  m.def("conv_db_chunks", &conv_db_chunks);
  m.def("gemm_splitk_ws_floats", &gemm_splitk_ws_floats);
  m.def("conv_bwd_weight_ws_floats", &conv_bwd_weight_ws_floats);
  m.def("conv_dwperm_ws_floats", &conv_dwperm_ws_floats);
  m.def("conv_db_ws_floats", &conv_db_ws_floats);
  m.def("flat_norm_scratch_floats", &flat_norm_scratch_floats);
  // (S, G, chunks, slabs): the tap bwd-weight launch plan and the
  // workspace slabs bf16_dw allocates for it
  m.def("conv_bwdw_tap_ws_slabs", [](int64_t Nb, int64_t C, int64_t Kout) {
    int S, G, chunks;
    int slabs = conv_bwdw_tap_ws_slabs((int)Nb, (int)C, (int)Kout, &S, &G,
                                       &chunks);
    return std::make_tuple(S, G, chunks, slabs);
  });
  // the tap-family dispatch predicates, (C, H, W, Kout, R, S, stride,
  // pad) in the argument order the call sites above use — exported so a
  // test can pin which kernel a shape reaches
  m.def("conv_tap_fwd_ok", [](int a, int b, int c, int d, int e, int f,
                              int g, int h) {
    return conv_tap_fwd_ok(a, b, c, d, e, f, g, h) != 0;
  });
  m.def("conv_tap_fwd_w4_ok", [](int a, int b, int c, int d, int e, int f,
                                 int g, int h) {
    return conv_tap_fwd_w4_ok(a, b, c, d, e, f, g, h) != 0;
  });
  m.def("conv_tap_bwdd_s2_ok", [](int a, int b, int c, int d, int e, int f,
                                  int g, int h) {
    return conv_tap_bwdd_s2_ok(a, b, c, d, e, f, g, h) != 0;
  });
  m.def("conv_bwdw_tap_ok", [](int a, int b, int c, int d, int e, int f,
                               int g, int h) {
    return conv_bwdw_tap_ok(a, b, c, d, e, f, g, h) != 0;
  });
  m.def("conv_bwdw_tap_s2_ok", [](int a, int b, int c, int d, int e, int f,
                                  int g, int h) {
    return conv_bwdw_tap_s2_ok(a, b, c, d, e, f, g, h) != 0;
  });
  m.def("pool_flatten_dropout_fwd", &pool_flatten_dropout_fwd);
  m.def("flatten_dropout_fwd", &flatten_dropout_fwd);
  m.def("dropout_unflatten_pool_bwd_relu", &dropout_unflatten_pool_bwd_relu);
  m.def("fc_head_step", &fc_head_step, py::arg("h1"), py::arg("w"),
        py::arg("b"), py::arg("labels"), py::arg("dloss"), py::arg("p"),
        py::arg("state"), py::arg("site"), py::arg("dw_out"),
        py::arg("db_out"), py::arg("queue") = py::none());
  // step batching (step_batch.hip): the queue of deferred roles, the two
  // one-launch helpers built on it, each role alone and the launch plan
  // (host arithmetic only)
  py::class_<StepQueue>(m, "StepQueue")
      .def(py::init<>())
      .def("flush", &StepQueue::flush)
      .def("pending", &StepQueue::pending)
      .def("conv_db", &StepQueue::conv_db)
      .def("splitk_reduce_dwperm", &StepQueue::splitk_reduce_dwperm,
           py::arg("ws"), py::arg("dw"), py::arg("Kout"), py::arg("C"),
           py::arg("RS"), py::arg("SK"), py::arg("ws_offset") = 0)
      .def("splitk_reduce", &StepQueue::splitk_reduce)
      .def("colsum", &StepQueue::colsum)
      .def("conv_small_bwdw_reduce", &StepQueue::conv_small_bwdw_reduce)
      .def("wperm", &StepQueue::wperm)
      .def("gather_rows", &StepQueue::gather_rows)
      .def("add_u64", &StepQueue::add_u64);
  m.def("prep_conv_weights", &prep_conv_weights);
  m.def("feed_gather", &feed_gather);
  m.def("conv_db", &conv_db);
  m.def("splitk_reduce_dwperm", &splitk_reduce_dwperm);
  m.def("splitk_reduce", &splitk_reduce);
  m.def("conv_small_bwdw_reduce", &conv_small_bwdw_reduce);
  m.def("colsum", &colsum);
  m.def("wperm", &wperm);
  m.def("step_batch_max_roles", &step_batch_max_roles);
  m.def("step_batch_plan", &step_batch_plan_py);
  m.def("step_batch_lookup", &step_batch_lookup_py);
  m.def("pool_seam_fused_ok", &pool_seam_fused_ok);
  m.def("fc_head_fused_ok", &fc_head_fused_ok);
  m.def("fc_head_ws_floats", &fc_head_ws_floats);
  m.def("add_", &add_inplace);
  m.def("add_relu_bwd_", &add_relu_bwd_);
  m.def("gap_bwd_relu", &gap_bwd_relu);
  m.def("maxpool2x2_bwd_relu", &maxpool2x2_bwd_relu);
  m.def("batchnorm_fwd", &batchnorm_fwd);
  m.def("batchnorm_bwd", &batchnorm_bwd);
  m.def("poison_set_u8", &poison_set_u8);
  m.def("poison_set_f32", &poison_set_f32);
  m.def("poison_addwrap_u8", &poison_addwrap_u8);
  m.def("poison_subf", &poison_subf);
  m.def("normalize_u8", &normalize_u8);
}
