// Torch bindings for the libai_amd gfx950 kernel library.
//
// Compiled by g++ (torch headers only); the kernels themselves live in
// csrc/kernels/*.hip, compiled by hipcc for gfx950 and linked in.  The split
// keeps torch headers out of hipcc (seconds-per-kernel compiles) and keeps the
// device code pure HIP.
#include <algorithm>
#include <torch/extension.h>
#include <c10/hip/HIPStream.h>
#include <hip/hip_runtime_api.h>

#include <tuple>
#include <vector>

// the extern "C" launchers of csrc/kernels/*.hip
#include "kernels/launchers.h"

namespace {

hipStream_t cur_stream() { return c10::hip::getCurrentHIPStream().stream(); }

void check_launch(const char* name) {
  hipError_t err = hipGetLastError();
  TORCH_CHECK(err == hipSuccess, name, " launch failed: ", hipGetErrorString(err));
}

bool is_bf16(const torch::Tensor& t) {
  TORCH_CHECK(t.scalar_type() == torch::kBFloat16 || t.scalar_type() == torch::kFloat32,
              "libai_amd kernels support bf16/f32, got ", t.scalar_type());
  return t.scalar_type() == torch::kBFloat16;
}

// the bias kernels index rows in whole 16-byte vectors: a width that is not a
// multiple of the vector width would read the wrong elements and leave the
// tail columns unwritten (the Python wrappers route such widths elsewhere)
void check_bias_width(const char* op, int W, int V) {
  TORCH_CHECK(W % V == 0 && W >= V, op, ": width ", W,
              " must be a positive multiple of the vector width ", V);
}

#define CHECK_IN(t)                                               \
  TORCH_CHECK(t.is_cuda(), #t " must be on device");              \
  TORCH_CHECK(t.is_contiguous(), #t " must be contiguous");

}  // namespace

// hipBLASLt epilogue-fused GEMMs (csrc/gemm_lt.cpp)
std::tuple<torch::Tensor, torch::Tensor> lt_gelu_aux_bias(torch::Tensor x,
                                                          torch::Tensor w,
                                                          torch::Tensor bias);
std::tuple<torch::Tensor, torch::Tensor> lt_dgelu_bgrad(torch::Tensor dy,
                                                        torch::Tensor w2,
                                                        torch::Tensor aux);
bool lt_epilogues_available();

// ---------------------------------------------------------------------------
// LayerNorm / RMSNorm
// ---------------------------------------------------------------------------
std::tuple<torch::Tensor, torch::Tensor, torch::Tensor> ln_fwd(
    torch::Tensor x, torch::Tensor gamma, c10::optional<torch::Tensor> beta, bool rms,
    double eps) {
  CHECK_IN(x);
  CHECK_IN(gamma);
  const int H = (int)gamma.numel();
  const int64_t R = x.numel() / H;
  auto y = torch::empty_like(x);
  auto opts = x.options().dtype(torch::kFloat32);
  auto mean = rms ? torch::empty({0}, opts) : torch::empty({R}, opts);
  auto rstd = torch::empty({R}, opts);
  const void* bptr = nullptr;
  if (beta.has_value()) {
    CHECK_IN(beta.value());
    bptr = beta->data_ptr();
  }
  auto fn = is_bf16(x) ? ln_fwd_bf16 : ln_fwd_f32;
  fn(x.data_ptr(), gamma.data_ptr(), bptr, y.data_ptr(),
     rms ? nullptr : mean.data_ptr<float>(), rstd.data_ptr<float>(), R, H, (float)eps,
     rms, cur_stream());
  check_launch("ln_fwd");
  return {y, mean, rstd};
}

// `dres` is the gradient arriving on the residual branch of x (the norm op's
// pass-through output): the result is bf16(bf16(dx_ln) + dres), what a
// separate add would give.  On the wave path one kernel writes dx and one
// [P, K*H] partial buffer (kernels/res_norm.hip); `single_pass = false`
// keeps the dx + wgrad_partial kernel pair there (tests and A/B runs), and
// wide or ragged rows always take the pair.
std::tuple<torch::Tensor, torch::Tensor, torch::Tensor> ln_bwd(
    torch::Tensor dy, torch::Tensor x, torch::Tensor gamma, torch::Tensor mean,
    torch::Tensor rstd, bool rms, bool need_dbeta, c10::optional<torch::Tensor> dres,
    bool single_pass) {
  CHECK_IN(dy);
  CHECK_IN(x);
  const int H = (int)gamma.numel();
  const int64_t R = x.numel() / H;
  auto dx = torch::empty_like(x);
  if (dres.has_value()) {
    CHECK_IN(dres.value());
    TORCH_CHECK(dres->numel() == x.numel() && dres->scalar_type() == x.scalar_type(),
                "ln_bwd: dres must match x");
  }
  if (single_pass && R > 0 && norm_wave_path(H, is_bf16(x) ? 8 : 4)) {
    const int maxP = norm_bwd_fused_blocks(R);
    const int64_t K = need_dbeta ? 2 : 1;
    auto partial =
        torch::empty({(int64_t)maxP, K * H}, x.options().dtype(torch::kFloat32));
    auto fn = is_bf16(x) ? ln_bwd_fused_bf16 : ln_bwd_fused_f32;
    const int P = fn(dy.data_ptr(), x.data_ptr(), gamma.data_ptr(),
       rms ? nullptr : mean.data_ptr<float>(), rstd.data_ptr<float>(),
       dres.has_value() ? dres->data_ptr() : nullptr, dx.data_ptr(),
       partial.data_ptr<float>(), need_dbeta, R, H, maxP, rms, cur_stream());
    check_launch("ln_bwd_fused");
    auto folded = partial.narrow(0, 0, P).sum(0);  // one reduction for every gradient
    auto dg = folded.narrow(0, 0, H).to(gamma.scalar_type());
    auto dbt = need_dbeta ? folded.narrow(0, H, H).to(gamma.scalar_type())
                          : torch::Tensor();
    return {dx, dg, dbt};
  }
  auto dgamma = torch::empty_like(gamma);
  auto dbeta = need_dbeta ? torch::empty_like(gamma) : torch::Tensor();
  const int64_t gxw = std::max<int64_t>(1, (H / 8 + 255) / 256);
  const int P = (int)std::min<int64_t>(std::max<int64_t>(1, 1024 / gxw),
                                       std::max<int64_t>(1, R / 4));
  auto partial = torch::empty({(need_dbeta ? 2L : 1L) * P, (int64_t)H},
                              x.options().dtype(torch::kFloat32));
  float* pgamma = partial.data_ptr<float>();
  float* pbeta = need_dbeta ? pgamma + (int64_t)P * H : nullptr;
  auto fdx = is_bf16(x) ? ln_bwd_dx_bf16 : ln_bwd_dx_f32;
  auto fw = is_bf16(x) ? ln_bwd_wgrad_bf16 : ln_bwd_wgrad_f32;
  const float* meanp = rms ? nullptr : mean.data_ptr<float>();
  fdx(dy.data_ptr(), x.data_ptr(), gamma.data_ptr(), meanp, rstd.data_ptr<float>(),
      dx.data_ptr(), R, H, rms, cur_stream());
  fw(dy.data_ptr(), x.data_ptr(), meanp, rstd.data_ptr<float>(), pgamma, pbeta,
     dgamma.data_ptr(), need_dbeta ? dbeta.data_ptr() : nullptr, R, H, P, rms,
     cur_stream());
  check_launch("ln_bwd");
  // fold the [P, H] fp32 partials with torch's reduction (the hand-rolled
  // fold was grid-starved at large P)
  dgamma.copy_(partial.narrow(0, 0, P).sum(0));
  if (need_dbeta) dbeta.copy_(partial.narrow(0, P, P).sum(0));
  if (dres.has_value()) dx.add_(dres->view_as(dx));
  return {dx, dgamma, dbeta};
}

// ---------------------------------------------------------------------------
// Training form of bias + dropout + residual + norm (kernels/res_norm.hip):
// h = (x + bias) * keep + res, y = norm(h); bf16, wave path only.
// ---------------------------------------------------------------------------
std::vector<torch::Tensor> res_drop_norm_fwd(
    torch::Tensor x, c10::optional<torch::Tensor> bias, torch::Tensor res,
    torch::Tensor gamma, c10::optional<torch::Tensor> beta, double eps, bool rms,
    double p, int64_t seed) {
  CHECK_IN(x);
  CHECK_IN(res);
  CHECK_IN(gamma);
  TORCH_CHECK(x.scalar_type() == torch::kBFloat16, "res_drop_norm_fwd: bf16 only");
  const int H = (int)x.size(-1);
  TORCH_CHECK(norm_wave_path(H, 8), "res_drop_norm_fwd: width ", H,
              " is outside the wave path");
  TORCH_CHECK(res.numel() == x.numel() && res.scalar_type() == x.scalar_type() &&
                  gamma.numel() == H && gamma.scalar_type() == x.scalar_type(),
              "res_drop_norm_fwd: res / gamma must match x");
  const void* bp = nullptr;
  const void* btp = nullptr;
  if (bias.has_value()) {
    CHECK_IN(bias.value());
    TORCH_CHECK(bias->numel() == H && bias->scalar_type() == x.scalar_type());
    bp = bias->data_ptr();
  }
  if (beta.has_value()) {
    CHECK_IN(beta.value());
    TORCH_CHECK(beta->numel() == H && beta->scalar_type() == x.scalar_type());
    btp = beta->data_ptr();
  }
  const int64_t R = x.numel() / H;
  auto h = torch::empty_like(x);
  auto y = torch::empty_like(x);
  auto opts = x.options().dtype(torch::kFloat32);
  auto mean = rms ? torch::empty({0}, opts) : torch::empty({R}, opts);
  auto rstd = torch::empty({R}, opts);
  if (R > 0) {
    res_drop_ln_fwd_bf16(x.data_ptr(), bp, res.data_ptr(), gamma.data_ptr(), btp,
                         h.data_ptr(), y.data_ptr(),
                         rms ? nullptr : mean.data_ptr<float>(), rstd.data_ptr<float>(),
                         R, H, (float)eps, rms, (float)p, (uint64_t)seed, cur_stream());
    check_launch("res_drop_norm_fwd");
  }
  return {h, y, mean, rstd};
}

// returns {dh, dx, dgamma, dbeta, dbias}: dh is the residual gradient
// bf16(bf16(dx_ln) + dres), dx = bf16(dh * keep) the gradient of the GEMM
// output (the same tensor as dh when p == 0)
std::vector<torch::Tensor> res_drop_norm_bwd(
    torch::Tensor dy, torch::Tensor h, torch::Tensor gamma, torch::Tensor mean,
    torch::Tensor rstd, c10::optional<torch::Tensor> dres, bool rms, bool need_dbeta,
    bool want_dbias, double p, int64_t seed) {
  CHECK_IN(dy);
  CHECK_IN(h);
  CHECK_IN(gamma);
  TORCH_CHECK(h.scalar_type() == torch::kBFloat16, "res_drop_norm_bwd: bf16 only");
  const int H = (int)h.size(-1);
  TORCH_CHECK(norm_wave_path(H, 8) && gamma.numel() == H,
              "res_drop_norm_bwd: width ", H, " is outside the wave path");
  TORCH_CHECK(dy.numel() == h.numel() && dy.scalar_type() == h.scalar_type(),
              "res_drop_norm_bwd: dy must match h");
  if (dres.has_value()) {
    CHECK_IN(dres.value());
    TORCH_CHECK(dres->numel() == h.numel() && dres->scalar_type() == h.scalar_type(),
                "res_drop_norm_bwd: dres must match h");
  }
  const int64_t R = h.numel() / H;
  TORCH_CHECK(R > 0, "res_drop_norm_bwd: empty input");
  TORCH_CHECK(rstd.numel() == R && (rms || mean.numel() == R));
  auto dh = torch::empty_like(h);
  auto dx = p > 0 ? torch::empty_like(h) : dh;
  const int maxP = norm_bwd_fused_blocks(R);
  const int64_t K = 1 + (need_dbeta ? 1 : 0) + (want_dbias ? 1 : 0);
  auto partial =
      torch::empty({(int64_t)maxP, K * H}, h.options().dtype(torch::kFloat32));
  const int P = res_drop_ln_bwd_bf16(dy.data_ptr(), h.data_ptr(), gamma.data_ptr(),
                       rms ? nullptr : mean.data_ptr<float>(), rstd.data_ptr<float>(),
                       dres.has_value() ? dres->data_ptr() : nullptr, dh.data_ptr(),
                       dx.data_ptr(), partial.data_ptr<float>(), need_dbeta, want_dbias,
                       R, H, maxP, rms, (float)p, (uint64_t)seed, cur_stream());
  check_launch("res_drop_norm_bwd");
  auto folded = partial.narrow(0, 0, P).sum(0);
  auto dg = folded.narrow(0, 0, H).to(h.scalar_type());
  auto dbt = need_dbeta ? folded.narrow(0, H, H).to(h.scalar_type()) : torch::Tensor();
  auto dbs = want_dbias ? folded.narrow(0, (need_dbeta ? 2 : 1) * (int64_t)H, H)
                              .to(h.scalar_type())
                        : torch::Tensor();
  return {dh, dx, dg, dbt, dbs};
}

// ---------------------------------------------------------------------------
// fused bias ops
// ---------------------------------------------------------------------------
torch::Tensor bias_gelu_fwd(torch::Tensor x, c10::optional<torch::Tensor> b) {
  CHECK_IN(x);
  auto y = torch::empty_like(x);
  const int W = b.has_value() ? (int)b->numel() : (int)x.size(-1);
  check_bias_width("bias_gelu_fwd", W, is_bf16(x) ? 8 : 4);
  auto fn = is_bf16(x) ? bias_gelu_fwd_bf16 : bias_gelu_fwd_f32;
  fn(x.data_ptr(), b.has_value() ? b->data_ptr() : nullptr, y.data_ptr(), x.numel(), W,
     cur_stream());
  check_launch("bias_gelu_fwd");
  return y;
}

std::tuple<torch::Tensor, c10::optional<torch::Tensor>> bias_gelu_bwd(
    torch::Tensor x, c10::optional<torch::Tensor> b, torch::Tensor dy,
    bool want_dbias) {
  CHECK_IN(x);
  CHECK_IN(dy);
  auto dx = torch::empty_like(x);
  const int W = b.has_value() ? (int)b->numel() : (int)x.size(-1);
  const int V = is_bf16(x) ? 8 : 4;
  check_bias_width("bias_gelu_bwd", W, V);
  float* pp = nullptr;
  torch::Tensor partial;
  int P = 0;
  if (want_dbias) {
    P = bias_col_grid_rows(x.numel(), W, V);
    partial = torch::empty({P, W}, x.options().dtype(torch::kFloat32));
    pp = partial.data_ptr<float>();
  }
  auto fn = is_bf16(x) ? bias_gelu_bwd_bf16 : bias_gelu_bwd_f32;
  fn(x.data_ptr(), b.has_value() ? b->data_ptr() : nullptr, dy.data_ptr(), dx.data_ptr(),
     pp, x.numel(), W, cur_stream());
  check_launch("bias_gelu_bwd");
  if (pp != nullptr)
    return {dx, partial.sum(0).to(x.scalar_type())};
  return {dx, c10::nullopt};
}

torch::Tensor colsum(torch::Tensor x, int64_t W) {
  CHECK_IN(x);
  const int64_t R = x.numel() / W;
  const int64_t gxw = std::max<int64_t>(1, (W / 8 + 255) / 256);
  const int P = (int)std::min<int64_t>(std::max<int64_t>(1, 1024 / gxw),
                                       std::max<int64_t>(1, R / 4));
  auto partial = torch::empty({P, W}, x.options().dtype(torch::kFloat32));
  auto out = torch::empty({W}, x.options());
  auto fn = is_bf16(x) ? colsum_bf16 : colsum_f32;
  fn(x.data_ptr(), partial.data_ptr<float>(), out.data_ptr(), R, (int)W, P,
     cur_stream());
  check_launch("colsum");
  out.copy_(partial.sum(0));
  return out;
}

torch::Tensor bias_dropout_res_fwd(torch::Tensor x, c10::optional<torch::Tensor> b,
                                   c10::optional<torch::Tensor> res, double p,
                                   int64_t seed) {
  CHECK_IN(x);
  auto y = torch::empty_like(x);
  const int W = b.has_value() ? (int)b->numel() : (int)x.size(-1);
  check_bias_width("bias_dropout_res_fwd", W, is_bf16(x) ? 8 : 4);
  auto fn = is_bf16(x) ? bias_dropout_res_fwd_bf16 : bias_dropout_res_fwd_f32;
  fn(x.data_ptr(), b.has_value() ? b->data_ptr() : nullptr,
     res.has_value() ? res->data_ptr() : nullptr, y.data_ptr(), x.numel(), W, (float)p,
     (uint64_t)seed, cur_stream());
  check_launch("bias_dropout_res_fwd");
  return y;
}

std::tuple<torch::Tensor, c10::optional<torch::Tensor>> bias_dropout_res_bwd(
    torch::Tensor dy, double p, int64_t seed, bool want_dbias) {
  CHECK_IN(dy);
  auto dx = torch::empty_like(dy);
  const int W = (int)dy.size(-1);
  const int V = is_bf16(dy) ? 8 : 4;
  check_bias_width("bias_dropout_res_bwd", W, V);
  float* pp = nullptr;
  torch::Tensor partial;
  if (want_dbias) {
    int P = bias_col_grid_rows(dy.numel(), W, V);
    partial = torch::empty({P, W}, dy.options().dtype(torch::kFloat32));
    pp = partial.data_ptr<float>();
  }
  auto fn = is_bf16(dy) ? bias_dropout_res_bwd_bf16 : bias_dropout_res_bwd_f32;
  fn(dy.data_ptr(), dx.data_ptr(), pp, dy.numel(), W, (float)p,
     (uint64_t)seed, cur_stream());
  check_launch("bias_dropout_res_bwd");
  if (pp != nullptr)
    return {dx, partial.sum(0).to(dy.scalar_type())};
  return {dx, c10::nullopt};
}

// ---------------------------------------------------------------------------
// fused scale+mask+softmax(+dropout)
// ---------------------------------------------------------------------------
torch::Tensor softmax_fwd(torch::Tensor s, c10::optional<torch::Tensor> pad_mask,
                          double scale, double p, int64_t seed, bool causal) {
  CHECK_IN(s);
  TORCH_CHECK(s.dim() == 4, "softmax_fwd expects [B, NH, SQ, SK]");
  auto out = torch::empty_like(s);
  const uint8_t* mp = nullptr;
  if (pad_mask.has_value()) {
    CHECK_IN(pad_mask.value());
    TORCH_CHECK(pad_mask->scalar_type() == torch::kUInt8 ||
                pad_mask->scalar_type() == torch::kBool);
    mp = (const uint8_t*)pad_mask->data_ptr();
  }
  auto fn = is_bf16(s) ? softmax_fwd_bf16 : softmax_fwd_f32;
  fn(s.data_ptr(), mp, out.data_ptr(), s.size(0), (int)s.size(1), (int)s.size(2),
     (int)s.size(3), (float)scale, (float)p, (uint64_t)seed, causal, cur_stream());
  check_launch("softmax_fwd");
  return out;
}

torch::Tensor softmax_bwd(torch::Tensor s, torch::Tensor dout,
                          c10::optional<torch::Tensor> pad_mask, double scale, double p,
                          int64_t seed, bool causal) {
  CHECK_IN(s);
  CHECK_IN(dout);
  auto ds = torch::empty_like(s);
  const uint8_t* mp = nullptr;
  if (pad_mask.has_value()) mp = (const uint8_t*)pad_mask->data_ptr();
  auto fn = is_bf16(s) ? softmax_bwd_bf16 : softmax_bwd_f32;
  fn(s.data_ptr(), dout.data_ptr(), mp, ds.data_ptr(), s.size(0), (int)s.size(1),
     (int)s.size(2), (int)s.size(3), (float)scale, (float)p, (uint64_t)seed, causal,
     cur_stream());
  check_launch("softmax_bwd");
  return ds;
}

// ---------------------------------------------------------------------------
// vocab-parallel cross entropy
// ---------------------------------------------------------------------------
std::tuple<torch::Tensor, torch::Tensor, torch::Tensor> ce_fwd(torch::Tensor logits,
                                                               torch::Tensor targets,
                                                               int64_t vocab_start,
                                                               int64_t ignore_index) {
  CHECK_IN(logits);
  CHECK_IN(targets);
  TORCH_CHECK(logits.dim() == 2, "ce_fwd expects [R, V_local]");
  const int64_t R = logits.size(0), Vl = logits.size(1);
  auto opts = logits.options().dtype(torch::kFloat32);
  auto lmax = torch::empty({R}, opts);
  auto lsumexp = torch::empty({R}, opts);
  auto tlogit = torch::empty({R}, opts);
  auto fn = is_bf16(logits) ? ce_fwd_bf16 : ce_fwd_f32;
  fn(logits.data_ptr(), targets.data_ptr<int64_t>(), lmax.data_ptr<float>(),
     lsumexp.data_ptr<float>(), tlogit.data_ptr<float>(), R, Vl, vocab_start,
     ignore_index, cur_stream());
  check_launch("ce_fwd");
  return {lmax, lsumexp, tlogit};
}

torch::Tensor ce_bwd(torch::Tensor logits, torch::Tensor targets, torch::Tensor gmax,
                     torch::Tensor gsumexp, torch::Tensor gscale, int64_t vocab_start,
                     int64_t ignore_index) {
  CHECK_IN(logits);
  auto dlogits = torch::empty_like(logits);
  auto fn = is_bf16(logits) ? ce_bwd_bf16 : ce_bwd_f32;
  fn(logits.data_ptr(), targets.data_ptr<int64_t>(), gmax.data_ptr<float>(),
     gsumexp.data_ptr<float>(), gscale.data_ptr<float>(), dlogits.data_ptr(),
     logits.size(0), logits.size(1), vocab_start, ignore_index, cur_stream());
  check_launch("ce_bwd");
  return dlogits;
}



// ---------------------------------------------------------------------------
// split-K weight-gradient GEMM: dW[N, K] = dY^T @ X (K1 bwd dW)
// ---------------------------------------------------------------------------
torch::Tensor gemm_dw(torch::Tensor dy, torch::Tensor x, int64_t splits) {
  CHECK_IN(dy);
  CHECK_IN(x);
  TORCH_CHECK(dy.scalar_type() == torch::kBFloat16 &&
              x.scalar_type() == torch::kBFloat16, "gemm_dw is bf16-only");
  const int64_t N = dy.size(-1), K = x.size(-1);
  const int64_t M = dy.numel() / N;
  TORCH_CHECK(x.numel() / K == M, "dY/X row mismatch");
  TORCH_CHECK(N % 128 == 0 && K % 128 == 0, "N and K must be 128-aligned");
  if (splits <= 0) {  // heuristic: >=512 workgroups to fill 8 XCDs
    const int64_t tiles = (N / 128) * (K / 128);
    splits = std::max<int64_t>(1, std::min<int64_t>(16, 512 / tiles));
  }
  auto ws = torch::empty({splits, N, K},
                         dy.options().dtype(torch::kFloat32));
  auto out = torch::empty({N, K}, dy.options());
  gemm_dw_bf16(dy.data_ptr(), x.data_ptr(), ws.data_ptr<float>(),
               out.data_ptr(), 1, M, N, K, splits, cur_stream());
  check_launch("gemm_dw");
  return out;
}


// ---------------------------------------------------------------------------
// argument checks shared by flash_fwd, flash_bwd and flash_decode
// ---------------------------------------------------------------------------
using OptTensor = c10::optional<torch::Tensor>;

// optional per-sequence valid key counts: int32 [B]
static const int* kv_len_ptr(const OptTensor& kv_len, int64_t B, bool contiguous) {
  if (!kv_len.has_value()) return nullptr;
  TORCH_CHECK(kv_len->scalar_type() == torch::kInt32 && kv_len->is_cuda() &&
                  (!contiguous || kv_len->is_contiguous()) && kv_len->numel() == B,
              "kv_len must be ", contiguous ? "a contiguous " : "an ",
              "int32 cuda tensor of size B");
  return kv_len->data_ptr<int>();
}

// The kernel variant arguments.  At most one of the four is set: the variants
// do not combine.
struct VariantPtrs {
  const float* alibi_slopes = nullptr;  // fp32 [H], one per QUERY head
  int window = 0;  // query i sees key j iff j <= i and i - j < window; 0 = off
  const float* rel_bias = nullptr;  // T5 table, fp32 [H, Sq + Sk - 1], one row per
                                    // QUERY head, entry kv - q + Sq - 1
  // packed documents, int32 [B, Sq] each: doc_start[b][i] the first token of
  // the document holding token i, doc_end[b][i] one past its last
  const int* doc_start = nullptr;
  const int* doc_end = nullptr;
};

// Every dtype, shape, device and exclusion check of the variant arguments, in
// one place and one order.  The window comes back clamped to the key count
// (the same mask).  flash_decode passes the alibi / window subset.
static VariantPtrs variant_ptrs(const char* op, const torch::Tensor& q, int64_t B,
                                int64_t H, int64_t Sq, int64_t Sk, bool causal,
                                const OptTensor& alibi_slopes, int64_t window,
                                const OptTensor& rel_bias = c10::nullopt,
                                const OptTensor& doc_start = c10::nullopt,
                                const OptTensor& doc_end = c10::nullopt,
                                int64_t q_offset = 0) {
  VariantPtrs p;
  // query offset (flash_fwd only): query row i sits at key position
  // q_offset + i.  0 is off and keeps the top-left alignment for Sq != Sk.
  TORCH_CHECK(q_offset >= 0, op, ": q_offset must be >= 0");
  if (q_offset > 0) {
    TORCH_CHECK(causal, op, ": q_offset requires causal attention");
    TORCH_CHECK(q_offset + Sq <= Sk, op, ": q_offset + Sq must not exceed Sk");
    TORCH_CHECK(!rel_bias.has_value(), op,
                ": q_offset cannot be combined with rel_bias");
    TORCH_CHECK(!doc_start.has_value() && !doc_end.has_value(), op,
                ": q_offset cannot be combined with document bounds");
  }
  auto on_q_device = [&](const torch::Tensor& t, torch::ScalarType dtype) {
    return t.scalar_type() == dtype && t.is_cuda() &&
           t.get_device() == q.get_device() && t.is_contiguous();
  };
  const bool has_alibi = alibi_slopes.has_value();
  if (has_alibi) {
    TORCH_CHECK(on_q_device(*alibi_slopes, torch::kFloat32) &&
                    alibi_slopes->numel() == H,
                "alibi_slopes must be a contiguous fp32 tensor of size H (query "
                "heads) on q's device");
    p.alibi_slopes = alibi_slopes->data_ptr<float>();
  }
  TORCH_CHECK(window >= 0, op, ": window must be >= 0 (0 = off)");
  if (window != 0) {
    TORCH_CHECK(causal, op, ": a sliding window requires causal attention");
    TORCH_CHECK(!has_alibi, op,
                ": a sliding window cannot be combined with alibi_slopes");
    // with an offset every query position lies inside the keys (checked above)
    TORCH_CHECK(q_offset > 0 || Sq == Sk, op, ": a sliding window needs Sq == Sk");
    p.window = (int)std::min<int64_t>(window, std::max<int64_t>(Sk, 1));
  }
  if (rel_bias.has_value()) {
    TORCH_CHECK(!has_alibi, op, ": rel_bias cannot be combined with alibi_slopes");
    TORCH_CHECK(window == 0, op,
                ": rel_bias cannot be combined with a sliding window");
    TORCH_CHECK(on_q_device(*rel_bias, torch::kFloat32) && rel_bias->dim() == 2 &&
                    rel_bias->size(0) == H && rel_bias->size(1) == Sq + Sk - 1,
                op, ": rel_bias must be a contiguous fp32 tensor of shape "
                "[H, Sq + Sk - 1] (query heads) on q's device");
    p.rel_bias = rel_bias->data_ptr<float>();
  }
  TORCH_CHECK(doc_start.has_value() == doc_end.has_value(), op,
              ": doc_start and doc_end must be given together");
  if (doc_start.has_value()) {
    TORCH_CHECK(causal, op, ": document bounds require causal attention");
    TORCH_CHECK(Sq == Sk, op, ": document bounds need Sq == Sk");
    TORCH_CHECK(!has_alibi, op,
                ": document bounds cannot be combined with alibi_slopes");
    TORCH_CHECK(window == 0, op,
                ": document bounds cannot be combined with a sliding window");
    TORCH_CHECK(!rel_bias.has_value(), op,
                ": document bounds cannot be combined with rel_bias");
    for (const torch::Tensor* t : {&doc_start.value(), &doc_end.value()})
      TORCH_CHECK(on_q_device(*t, torch::kInt32) && t->dim() == 2 &&
                      t->size(0) == B && t->size(1) == Sq,
                  op, ": doc_start / doc_end must be contiguous int32 tensors of "
                  "shape [B, Sq] on q's device");
    p.doc_start = doc_start->data_ptr<int>();
    p.doc_end = doc_end->data_ptr<int>();
  }
  return p;
}

// pointer and (batch, seq, head) element strides of a [B, S, H, D] tensor
static StridedBSHD strided(const torch::Tensor& t) {
  return {t.data_ptr(), t.stride(0), t.stride(1), t.stride(2)};
}

// ---------------------------------------------------------------------------
// fused single-query decode attention (K16 serving path)
// ---------------------------------------------------------------------------
torch::Tensor flash_decode(torch::Tensor q, torch::Tensor k, torch::Tensor v,
                           double scale, c10::optional<torch::Tensor> kv_len,
                           c10::optional<torch::Tensor> alibi_slopes,
                           int64_t window) {
  // q: [B, H, 1, D]; k/v: [B, Hkv, Skv, D] (the decode KV-cache layout)
  TORCH_CHECK(q.dim() == 4 && q.size(2) == 1, "flash_decode: q must be [B,H,1,D]");
  TORCH_CHECK(q.scalar_type() == torch::kBFloat16, "flash_decode is bf16-only");
  TORCH_CHECK(q.stride(3) == 1 && k.stride(3) == 1 && v.stride(3) == 1);
  const int B = (int)q.size(0), H = (int)q.size(1), D = (int)q.size(3);
  const int Skv = (int)k.size(2), Hkv = (int)k.size(1);
  TORCH_CHECK(D == 64 || D == 128, "head dim must be 64 or 128");
  TORCH_CHECK(H % Hkv == 0 && (int)v.size(1) == Hkv);
  const int* kvl = kv_len_ptr(kv_len, B, /*contiguous=*/false);
  // decode is causal by construction: the query is the last cached key, so it
  // stands at row Skv - 1 of a square problem
  const VariantPtrs var =
      variant_ptrs("flash_decode", q, B, H, Skv, Skv, true, alibi_slopes, window);
  const float* slopes = var.alibi_slopes;
  const int win = var.window;
  auto o = torch::empty({B, H, 1, D}, q.options());
  const int S = flash_decode_num_splits(B, H, Skv);
  if (S > 1) {
    // split-KV (flash-decoding): B*H WGs underfill 256 CUs at serving
    // batch sizes; fixed 512-key splits keep outputs bitwise-independent
    // of the cache capacity (see kernels/flash_decode.hip)
    auto fopt = q.options().dtype(torch::kFloat32);
    auto pm = torch::empty({(int64_t)B * H * S}, fopt);
    auto pl = torch::empty({(int64_t)B * H * S}, fopt);
    auto pa = torch::empty({(int64_t)B * H * S * D}, fopt);
    flash_decode_split_bf16(
        q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(),
        pm.data_ptr<float>(), pl.data_ptr<float>(), pa.data_ptr<float>(), kvl,
        q.stride(0), q.stride(1), k.stride(0), k.stride(2), k.stride(1),
        v.stride(0), v.stride(2), v.stride(1), o.stride(0), o.stride(1), B, H,
        S, Skv, D, (float)scale, H / Hkv, slopes, win, cur_stream());
  } else {
    flash_decode_bf16(q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(),
                      kvl, q.stride(0), q.stride(1), k.stride(0), k.stride(2),
                      k.stride(1), v.stride(0), v.stride(2), v.stride(1),
                      o.stride(0), o.stride(1), B, H, Skv, D, (float)scale,
                      H / Hkv, slopes, win, cur_stream());
  }
  check_launch("flash_decode");
  return o;
}

// ---------------------------------------------------------------------------
// embedding gather/scatter (K10)
// ---------------------------------------------------------------------------
torch::Tensor embedding_fwd(torch::Tensor ids, torch::Tensor w, int64_t vocab_start) {
  CHECK_IN(ids);
  CHECK_IN(w);
  TORCH_CHECK(ids.scalar_type() == torch::kInt64, "ids must be int64");
  const int64_t H = w.size(1);
  TORCH_CHECK((H * w.element_size()) % 16 == 0, "hidden dim must be 16B-aligned");
  auto sizes = ids.sizes().vec();
  sizes.push_back(H);
  auto out = torch::empty(sizes, w.options());
  const int64_t N = ids.numel();
  if (is_bf16(w))
    embedding_fwd_bf16(ids.data_ptr<int64_t>(), w.data_ptr(), out.data_ptr(), N, H,
                       vocab_start, w.size(0), cur_stream());
  else
    embedding_fwd_f32(ids.data_ptr<int64_t>(), w.data_ptr(), out.data_ptr(), N, H,
                      vocab_start, w.size(0), cur_stream());
  check_launch("embedding_fwd");
  return out;
}

torch::Tensor embedding_bwd(torch::Tensor ids, torch::Tensor dout,
                            int64_t vocab_local, int64_t vocab_start,
                            int64_t padding_idx, torch::ScalarType grad_dtype) {
  CHECK_IN(ids);
  auto douts = dout.contiguous();
  const int64_t H = douts.size(-1);
  const int64_t N = ids.numel();
  auto ws = torch::zeros({vocab_local, H},
                         douts.options().dtype(torch::kFloat32));
  const int64_t padding_row =
      (padding_idx >= 0) ? padding_idx - vocab_start : -1;
  if (is_bf16(douts))
    embedding_bwd_bf16(ids.data_ptr<int64_t>(), douts.data_ptr(),
                       ws.data_ptr<float>(), N, H, vocab_start, vocab_local,
                       padding_row, cur_stream());
  else
    embedding_bwd_f32(ids.data_ptr<int64_t>(), douts.data_ptr(),
                      ws.data_ptr<float>(), N, H, vocab_start, vocab_local,
                      padding_row, cur_stream());
  check_launch("embedding_bwd");
  return grad_dtype == torch::kFloat32 ? ws : ws.to(grad_dtype);
}

// ---------------------------------------------------------------------------
// flash attention
// ---------------------------------------------------------------------------
// the launch arguments the forward and the backward share, each stride next
// to the tensor it came from
static FlashFwdArgs flash_args(const torch::Tensor& q, const torch::Tensor& k,
                               const torch::Tensor& v, const torch::Tensor& o,
                               const torch::Tensor& lse, const int* kv_len,
                               double scale, double p_drop, int64_t seed, bool causal,
                               const VariantPtrs& var) {
  FlashFwdArgs a{};
  a.q = strided(q);
  a.k = strided(k);
  a.v = strided(v);
  a.o = strided(o);
  a.lse = lse.data_ptr<float>();
  a.kv_len = kv_len;
  a.B = (int)q.size(0);
  a.H = (int)q.size(2);
  a.Sq = (int)q.size(1);
  a.Sk = (int)k.size(1);
  a.D = (int)q.size(3);
  a.kv_group = (int)(q.size(2) / k.size(2));
  a.scale = (float)scale;
  a.p_drop = (float)p_drop;
  a.seed = (uint64_t)seed;
  a.causal = causal ? 1 : 0;
  a.alibi_slopes = var.alibi_slopes;
  a.window = var.window;
  a.rel_bias = var.rel_bias;
  a.doc_start = var.doc_start;
  return a;
}

std::tuple<torch::Tensor, torch::Tensor> flash_fwd(torch::Tensor q, torch::Tensor k,
                                                   torch::Tensor v, double scale,
                                                   double p_drop, int64_t seed,
                                                   bool causal,
                                                   c10::optional<torch::Tensor> kv_len,
                                                   c10::optional<torch::Tensor> alibi_slopes,
                                                   int64_t window,
                                                   c10::optional<torch::Tensor> rel_bias,
                                                   c10::optional<torch::Tensor> doc_start,
                                                   c10::optional<torch::Tensor> doc_end,
                                                   int64_t q_offset) {
  const int* kvl = kv_len_ptr(kv_len, q.size(0), /*contiguous=*/true);
  // q/k/v: [B, S, H, D] (strided views into a fused qkv buffer are fine; the
  // last dim must be contiguous and 16B-aligned)
  TORCH_CHECK(q.dim() == 4 && k.dim() == 4 && v.dim() == 4);
  TORCH_CHECK(q.scalar_type() == torch::kBFloat16, "flash_fwd is bf16-only");
  TORCH_CHECK(q.stride(3) == 1 && k.stride(3) == 1 && v.stride(3) == 1);
  const int B = (int)q.size(0), Sq = (int)q.size(1), H = (int)q.size(2),
            D = (int)q.size(3);
  const int Sk = (int)k.size(1), Hkv = (int)k.size(2);
  TORCH_CHECK(D == 64 || D == 128, "head dim must be 64 or 128");
  // the dropout hash keys on Sk / 4 and the backward stages keys in runs of
  // 8; a forward without dropout bounds every staged key row by Sk, so a
  // ragged key count (a cache of 117 keys) is fine there
  TORCH_CHECK(p_drop == 0.0 || Sk % 8 == 0,
              "Sk must be a multiple of 8 (with dropout)");
  TORCH_CHECK(Hkv > 0 && H % Hkv == 0 && (int)v.size(2) == Hkv,
              "GQA head counts: H divisible by Hkv, v matches k");
  TORCH_CHECK(q_offset == 0 || p_drop == 0.0,
              "flash_fwd: q_offset cannot be combined with dropout");
  const VariantPtrs var = variant_ptrs("flash_fwd", q, B, H, Sq, Sk, causal,
                                       alibi_slopes, window, rel_bias, doc_start,
                                       doc_end, q_offset);
  auto o = torch::empty({B, Sq, H, D}, q.options());
  auto lse = torch::empty({B, H, Sq}, q.options().dtype(torch::kFloat32));
  FlashFwdArgs a =
      flash_args(q, k, v, o, lse, kvl, scale, p_drop, seed, causal, var);
  a.q_off = (int)q_offset;
  flash_fwd_bf16(a, cur_stream());
  check_launch("flash_fwd");
  return {o, lse};
}

// Returns (dq, dk, dv), or (dq, dk, dv, d_rel_bias) when a relative-position
// table is given (fp32, the table's shape, summed over the batch).
py::tuple flash_bwd(
    torch::Tensor q, torch::Tensor k, torch::Tensor v, torch::Tensor o,
    torch::Tensor dout, torch::Tensor lse, double scale, double p_drop, int64_t seed,
    bool causal, c10::optional<torch::Tensor> dqkv,
    c10::optional<torch::Tensor> kv_len,
    c10::optional<torch::Tensor> alibi_slopes, int64_t window,
    c10::optional<torch::Tensor> rel_bias, c10::optional<torch::Tensor> doc_start,
    c10::optional<torch::Tensor> doc_end, c10::optional<torch::Tensor> dkv) {
  const int* kvl = kv_len_ptr(kv_len, q.size(0), /*contiguous=*/true);
  const int B = (int)q.size(0), Sq = (int)q.size(1), H = (int)q.size(2),
            D = (int)q.size(3);
  const int Sk = (int)k.size(1), Hkv = (int)k.size(2);
  // the forward waives this without dropout; the backward kernels do not
  TORCH_CHECK(Sk % 8 == 0, "flash_bwd: Sk must be a multiple of 8");
  const VariantPtrs var = variant_ptrs("flash_bwd", q, B, H, Sq, Sk, causal,
                                       alibi_slopes, window, rel_bias, doc_start,
                                       doc_end);
  // the dQ kernel accumulates into it with atomics: zero-filled here
  torch::Tensor d_relb;
  if (var.rel_bias != nullptr) d_relb = torch::zeros_like(rel_bias.value());
  TORCH_CHECK(dout.is_contiguous() && o.is_contiguous());
  torch::Tensor dq, dk, dv;
  if (dqkv.has_value()) {
    // [B, S, H, 3, D] fused grad buffer: write q/k/v grads in place
    TORCH_CHECK(H / Hkv == 1, "packed dqkv implies MHA");
    auto g = dqkv.value();
    dq = g.select(3, 0);
    dk = g.select(3, 1);
    dv = g.select(3, 2);
    TORCH_CHECK(!dkv.has_value(), "flash_bwd: dqkv and dkv exclude each other");
  } else if (dkv.has_value()) {
    // [B, Sk, Hkv, 2, D] fused grad buffer of a packed key/value projection
    // (cross-attention): write the k/v grads in place
    auto g = dkv.value();
    TORCH_CHECK(g.dim() == 5 && g.size(0) == B && g.size(1) == Sk &&
                    g.size(2) == Hkv && g.size(3) == 2 && g.size(4) == D &&
                    g.stride(4) == 1 && g.scalar_type() == q.scalar_type() &&
                    g.is_cuda() && g.get_device() == q.get_device(),
                "flash_bwd: dkv must be [B, Sk, Hkv, 2, D] of q's dtype and device");
    dq = torch::empty_like(q, q.options());
    dk = g.select(3, 0);
    dv = g.select(3, 1);
  } else {
    dq = torch::empty_like(q, q.options());
    dk = torch::empty({B, Sk, Hkv, D}, q.options());
    dv = torch::empty({B, Sk, Hkv, D}, q.options());
  }
  auto drow = torch::empty({B, H, Sq}, q.options().dtype(torch::kFloat32));
  FlashBwdArgs a{};
  static_cast<FlashFwdArgs&>(a) =
      flash_args(q, k, v, o, lse, kvl, scale, p_drop, seed, causal, var);
  a.dout = strided(dout);
  a.dq = strided(dq);
  a.dk = strided(dk);
  a.dv = strided(dv);
  a.drow_ws = drow.data_ptr<float>();
  a.d_rel_bias = var.rel_bias != nullptr ? d_relb.data_ptr<float>() : nullptr;
  a.doc_end = var.doc_end;
  flash_bwd_bf16(a, cur_stream());
  check_launch("flash_bwd");
  if (var.rel_bias != nullptr) return py::make_tuple(dq, dk, dv, d_relb);
  return py::make_tuple(dq, dk, dv);
}

void attn_dropout_apply(torch::Tensor x, int64_t Sq, int64_t Sk, double p,
                        int64_t seed) {
  CHECK_IN(x);
  int64_t BH = x.numel() / (Sq * Sk);
  auto fn = is_bf16(x) ? attn_dropout_apply_bf16 : attn_dropout_apply_f32;
  fn(x.data_ptr(), BH, Sq, Sk, (float)p, (uint64_t)seed, cur_stream());
  check_launch("attn_dropout_apply");
}


// ---------------------------------------------------------------------------
// RoPE / SwiGLU
// ---------------------------------------------------------------------------
torch::Tensor rope(torch::Tensor x, torch::Tensor cos_t, torch::Tensor sin_t,
                   int64_t pos0, bool bwd, c10::optional<torch::Tensor> pos_ids) {
  // x: [B, S, NH, HS] (strided view ok, last dim contiguous)
  TORCH_CHECK(x.dim() == 4 && x.stride(3) == 1);
  // optional per-token table rows (packed documents): int32 [B, S]; the kernel
  // clamps them into the table
  const int* pid = nullptr;
  if (pos_ids.has_value()) {
    TORCH_CHECK(pos_ids->scalar_type() == torch::kInt32 && pos_ids->is_cuda() &&
                    pos_ids->get_device() == x.get_device() &&
                    pos_ids->is_contiguous() && pos_ids->dim() == 2 &&
                    pos_ids->size(0) == x.size(0) && pos_ids->size(1) == x.size(1),
                "rope: pos_ids must be a contiguous int32 tensor of shape [B, S] "
                "on x's device");
    TORCH_CHECK(cos_t.size(0) > 0 && sin_t.size(0) == cos_t.size(0));
    pid = pos_ids->data_ptr<int>();
  }
  auto out = torch::empty(x.sizes(), x.options());
  const int B = (int)x.size(0), S = (int)x.size(1), NH = (int)x.size(2),
            HS = (int)x.size(3);
  auto fn = bwd ? (is_bf16(x) ? rope_bwd_bf16 : rope_bwd_f32)
                : (is_bf16(x) ? rope_fwd_bf16 : rope_fwd_f32);
  fn(x.data_ptr(), out.data_ptr(), cos_t.data_ptr<float>(), sin_t.data_ptr<float>(),
     x.stride(0), x.stride(1), x.stride(2), out.stride(0), out.stride(1),
     out.stride(2), B, S, NH, HS, (int)pos0, pid, (int)cos_t.size(0), cur_stream());
  check_launch("rope");
  return out;
}

// Fused decode-step RoPE + KV insert (hipGraph-captured serving; see
// kernels/rope_swiglu.hip).  q/k/v are [B, 1, H, HD] strided views; pos is a
// DEVICE int64 [1] tensor; ck/cv are the [B, KVH, max_len, HD] static caches.
// Returns rotated q in [B, NH, 1, HD] (flash_decode input layout).
torch::Tensor rope_kv_insert(torch::Tensor q, torch::Tensor k, torch::Tensor v,
                             torch::Tensor ck, torch::Tensor cv,
                             torch::Tensor cos_t, torch::Tensor sin_t,
                             torch::Tensor pos, bool rotate) {
  TORCH_CHECK(q.dim() == 4 && q.size(1) == 1 && q.stride(3) == 1);
  TORCH_CHECK(k.dim() == 4 && k.size(1) == 1 && k.stride(3) == 1);
  TORCH_CHECK(v.dim() == 4 && v.size(1) == 1 && v.stride(3) == 1);
  TORCH_CHECK(ck.is_contiguous() && cv.is_contiguous());
  TORCH_CHECK(pos.scalar_type() == torch::kInt64 && pos.is_cuda());
  TORCH_CHECK(pos.numel() == 1 || pos.numel() == q.size(0),
              "pos must be scalar or per-batch");
  TORCH_CHECK(pos.is_contiguous());
  TORCH_CHECK(is_bf16(q) && is_bf16(ck), "rope_kv_insert is bf16-only");
  const int B = (int)q.size(0), NH = (int)q.size(2), HD = (int)q.size(3);
  const int KVH = (int)k.size(2);
  TORCH_CHECK(ck.size(0) == B && ck.size(1) == KVH && ck.size(3) == HD);
  auto qo = torch::empty({B, NH, 1, HD}, q.options());
  rope_kv_insert_bf16(q.data_ptr(), k.data_ptr(), v.data_ptr(), qo.data_ptr(),
                      ck.data_ptr(), cv.data_ptr(), cos_t.data_ptr<float>(),
                      sin_t.data_ptr<float>(),
                      (const long long*)pos.data_ptr<int64_t>(), B, NH, KVH,
                      HD, ck.size(2), q.stride(0), q.stride(2), k.stride(0),
                      k.stride(2), v.stride(0), v.stride(2), rotate ? 1 : 0,
                      pos.numel() > 1 ? 1 : 0, cur_stream());
  check_launch("rope_kv_insert");
  return qo;
}

// Single-pass delayed-scaling quantize: bf16 -> fp8 e4m3 with the GIVEN
// scale; amax of the input accumulates into `amax` (caller derives the
// next scale).  kernels/quant_fp8.hip.
// Fused residual-add + norm (decode/eval forward only):
// h = x (+bias) + res, y = norm(h).  Wave-per-row, H <= 2048 * vec.
std::vector<torch::Tensor> res_norm_fwd(torch::Tensor x,
                                        c10::optional<torch::Tensor> bias,
                                        torch::Tensor res, torch::Tensor gamma,
                                        c10::optional<torch::Tensor> beta,
                                        double eps, bool rms) {
  CHECK_IN(x);
  CHECK_IN(res);
  TORCH_CHECK(is_bf16(x), "res_norm_fwd: bf16 only");
  const int H = (int)x.size(-1);
  TORCH_CHECK(H % 8 == 0 && H / 8 <= 256, "H must be vec8 and <= 2048");
  const int64_t R = x.numel() / H;
  auto h = torch::empty_like(x);
  auto y = torch::empty_like(x);
  const void* bp = bias.has_value() ? bias->contiguous().data_ptr() : nullptr;
  const void* btp = beta.has_value() ? beta->contiguous().data_ptr() : nullptr;
  res_ln_fwd_bf16(x.data_ptr(), bp, res.contiguous().data_ptr(),
                  gamma.contiguous().data_ptr(), btp, h.data_ptr(),
                  y.data_ptr(), R, H, (float)eps, rms, cur_stream());
  check_launch("res_norm_fwd");
  return {h, y};
}

torch::Tensor quant_fp8(torch::Tensor x, torch::Tensor scale,
                        torch::Tensor amax) {
  CHECK_IN(x);
  TORCH_CHECK(is_bf16(x), "quant_fp8: bf16 input only");
  TORCH_CHECK(scale.scalar_type() == torch::kFloat32 && scale.is_cuda());
  TORCH_CHECK(amax.scalar_type() == torch::kFloat32 && amax.is_cuda());
  auto out = torch::empty(x.sizes(),
                          x.options().dtype(torch::kFloat8_e4m3fn));
  quant_fp8_bf16(x.data_ptr(), out.data_ptr(), scale.data_ptr<float>(),
                 amax.data_ptr<float>(), x.numel(), cur_stream());
  check_launch("quant_fp8");
  return out;
}

torch::Tensor swiglu_fwd(torch::Tensor x) {
  CHECK_IN(x);
  const int64_t F = x.size(-1) / 2;
  auto sizes = x.sizes().vec();
  sizes.back() = F;
  auto y = torch::empty(sizes, x.options());
  auto fn = is_bf16(x) ? swiglu_fwd_bf16 : swiglu_fwd_f32;
  fn(x.data_ptr(), y.data_ptr(), x.numel() / (2 * F), (int)F, cur_stream());
  check_launch("swiglu_fwd");
  return y;
}

torch::Tensor swiglu_bwd(torch::Tensor x, torch::Tensor dy) {
  CHECK_IN(x);
  CHECK_IN(dy);
  const int64_t F = x.size(-1) / 2;
  auto dx = torch::empty_like(x);
  auto fn = is_bf16(x) ? swiglu_bwd_bf16 : swiglu_bwd_f32;
  fn(x.data_ptr(), dy.data_ptr(), dx.data_ptr(), x.numel() / (2 * F), (int)F,
     cur_stream());
  check_launch("swiglu_bwd");
  return dx;
}

// ---------------------------------------------------------------------------
// fused AdamW
// ---------------------------------------------------------------------------
void adamw_step(torch::Tensor chunks, bool bf16_params, double lr, double beta1,
                double beta2, double eps, double wd, double bc1, double bc2,
                double grad_scale) {
  CHECK_IN(chunks);
  TORCH_CHECK(chunks.scalar_type() == torch::kInt64 && chunks.size(1) == 6);
  auto fn = bf16_params ? adamw_step_bf16 : adamw_step_f32;
  fn(chunks.data_ptr(), (int)chunks.size(0), (float)lr, (float)beta1, (float)beta2,
     (float)eps, (float)wd, (float)bc1, (float)bc2, (float)grad_scale, cur_stream());
  check_launch("adamw_step");
}

void l2norm_sq(torch::Tensor chunks, bool bf16_grads, torch::Tensor out) {
  CHECK_IN(chunks);
  TORCH_CHECK(chunks.scalar_type() == torch::kInt64 && chunks.size(1) == 2);
  auto fn = bf16_grads ? l2norm_sq_bf16 : l2norm_sq_f32;
  fn(chunks.data_ptr(), (int)chunks.size(0), out.data_ptr<float>(), cur_stream());
  check_launch("l2norm_sq");
}

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
  m.def("ln_fwd", &ln_fwd);
  m.def("ln_bwd", &ln_bwd, py::arg("dy"), py::arg("x"), py::arg("gamma"),
        py::arg("mean"), py::arg("rstd"), py::arg("rms"), py::arg("need_dbeta"),
        py::arg("dres") = py::none(), py::arg("single_pass") = true);
  m.def("res_drop_norm_fwd", &res_drop_norm_fwd);
  m.def("res_drop_norm_bwd", &res_drop_norm_bwd);
  m.def("bias_gelu_fwd", &bias_gelu_fwd);
  m.def("bias_gelu_bwd", &bias_gelu_bwd);
  m.def("colsum", &colsum);
  m.def("bias_dropout_res_fwd", &bias_dropout_res_fwd);
  m.def("bias_dropout_res_bwd", &bias_dropout_res_bwd);
  m.def("softmax_fwd", &softmax_fwd);
  m.def("softmax_bwd", &softmax_bwd);
  m.def("lt_gelu_aux_bias", &lt_gelu_aux_bias);
  m.def("lt_dgelu_bgrad", &lt_dgelu_bgrad);
  m.def("lt_epilogues_available", &lt_epilogues_available);
  m.def("gemm_dw", &gemm_dw);
  m.def("flash_decode", &flash_decode, py::arg("q"), py::arg("k"), py::arg("v"),
        py::arg("scale"), py::arg("kv_len"),
        py::arg("alibi_slopes") = py::none(), py::arg("window") = 0);
  m.def("embedding_fwd", &embedding_fwd);
  m.def("embedding_bwd", &embedding_bwd);
  m.def("flash_fwd", &flash_fwd, py::arg("q"), py::arg("k"), py::arg("v"),
        py::arg("scale"), py::arg("p_drop"), py::arg("seed"), py::arg("causal"),
        py::arg("kv_len"), py::arg("alibi_slopes") = py::none(), py::arg("window") = 0,
        py::arg("rel_bias") = py::none(), py::arg("doc_start") = py::none(),
        py::arg("doc_end") = py::none(), py::arg("q_offset") = 0);
  m.def("flash_bwd", &flash_bwd, py::arg("q"), py::arg("k"), py::arg("v"),
        py::arg("o"), py::arg("dout"), py::arg("lse"), py::arg("scale"),
        py::arg("p_drop"), py::arg("seed"), py::arg("causal"), py::arg("dqkv"),
        py::arg("kv_len"), py::arg("alibi_slopes") = py::none(), py::arg("window") = 0,
        py::arg("rel_bias") = py::none(), py::arg("doc_start") = py::none(),
        py::arg("doc_end") = py::none(), py::arg("dkv") = py::none());
  m.def("attn_dropout_apply", &attn_dropout_apply);
  m.def("ce_fwd", &ce_fwd);
  m.def("ce_bwd", &ce_bwd);
  m.def("rope", &rope, py::arg("x"), py::arg("cos_t"), py::arg("sin_t"),
        py::arg("pos0"), py::arg("bwd"), py::arg("pos_ids") = py::none());
  m.def("rope_kv_insert", &rope_kv_insert);
  m.def("quant_fp8", &quant_fp8);
  m.def("res_norm_fwd", &res_norm_fwd);
  m.def("swiglu_fwd", &swiglu_fwd);
  m.def("swiglu_bwd", &swiglu_bwd);
  m.def("adamw_step", &adamw_step);
  m.def("l2norm_sq", &l2norm_sq);
  m.def("adamw_chunk_elems", &adamw_chunk_elems);
}
