// The C ABI between csrc/bindings.cpp (g++, torch headers) and the launchers
// defined in csrc/kernels/*.hip (hipcc).  Pure C/C++, no torch.
//
// Every .hip file and bindings.cpp include this header, so the compiler holds
// each definition and each call against one declaration: with C linkage a
// second declaration of a name with other parameters is a hard error, where a
// hand-copied prototype would have linked without a diagnostic.
#pragma once
#include <hip/hip_runtime_api.h>
#include <stdint.h>

// ---------------------------------------------------------------------------
// flash attention (flash_attn.hip): arguments by name
// ---------------------------------------------------------------------------
// a [B, S, H, D] bf16 tensor with a contiguous last dim; strides in elements
struct StridedBSHD {
  void* ptr;
  int64_t sb, ss, sh;
};

// At most one of alibi_slopes / window / rel_bias / doc_start is set (the
// binding rejects combinations); it selects the kernel variant.
struct FlashFwdArgs {
  StridedBSHD q, k, v, o;
  float* lse;         // [B, H, Sq]: written by the forward, read by the backward
  const int* kv_len;  // [B] valid key counts, or null
  int B, H, Sq, Sk, D;
  int kv_group;  // query heads per kv head (GQA)
  float scale, p_drop;
  uint64_t seed;
  int causal;
  const float* alibi_slopes;  // [H], or null
  int window;                 // sliding window, 0 = off
  const float* rel_bias;      // [H, Sq + Sk - 1], or null
  const int* doc_start;       // [B, Sq], or null
  int q_off;  // forward only: query row i sits at key position q_off + i (0 = off)
};

struct FlashBwdArgs : FlashFwdArgs {
  StridedBSHD dout, dq, dk, dv;  // dout shares o's layout
  float* drow_ws;                // [B, H, Sq] workspace: rowsum(dO * O)
  float* d_rel_bias;             // rel_bias's shape, zero-filled; null without rel_bias
  const int* doc_end;            // [B, Sq]; set together with doc_start
};

// NAME_bf16 and NAME_f32 with one parameter list (the .hip files define the
// pairs from one macro body too)
#define BF16_F32(RET, NAME, ...) \
  RET NAME##_bf16(__VA_ARGS__);  \
  RET NAME##_f32(__VA_ARGS__)

extern "C" {

void flash_fwd_bf16(const FlashFwdArgs& args, hipStream_t stream);
void flash_bwd_bf16(const FlashBwdArgs& args, hipStream_t stream);
BF16_F32(void, attn_dropout_apply, void* x, int64_t BH, int64_t Sq, int64_t Sk, float p,
         uint64_t seed, hipStream_t stream);

// flash_decode.hip: q/o [B, H, 1, D], k/v [B, Hkv, Skv, D] (the cache layout)
void flash_decode_bf16(const void* q, const void* k, const void* v, void* o,
                       const int* kv_len, int64_t q_sb, int64_t q_sh, int64_t k_sb,
                       int64_t k_ss, int64_t k_sh, int64_t v_sb, int64_t v_ss,
                       int64_t v_sh, int64_t o_sb, int64_t o_sh, int B, int H,
                       int Skv, int D, float scale, int kv_group,
                       const float* alibi_slopes, int window, hipStream_t stream);
int flash_decode_num_splits(int B, int H, int Skv);
void flash_decode_split_bf16(const void* q, const void* k, const void* v, void* o,
                             float* part_m, float* part_l, float* part_acc,
                             const int* kv_len, int64_t q_sb, int64_t q_sh,
                             int64_t k_sb, int64_t k_ss, int64_t k_sh, int64_t v_sb,
                             int64_t v_ss, int64_t v_sh, int64_t o_sb, int64_t o_sh,
                             int B, int H, int S, int Skv, int D, float scale,
                             int kv_group, const float* alibi_slopes, int window,
                             hipStream_t stream);

// layer_norm.hip
BF16_F32(void, ln_fwd, const void* x, const void* gamma, const void* beta, void* y,
         float* mean, float* rstd, int64_t R, int H, float eps, bool rms,
         hipStream_t stream);
BF16_F32(void, ln_bwd_dx, const void* dy, const void* x, const void* gamma,
         const float* mean, const float* rstd, void* dx, int64_t R, int H, bool rms,
         hipStream_t stream);
BF16_F32(void, ln_bwd_wgrad, const void* dy, const void* x, const float* mean,
         const float* rstd, float* pgamma, float* pbeta, void* dgamma, void* dbeta,
         int64_t R, int H, int P, bool rms, hipStream_t stream);
void res_ln_fwd_bf16(const void* x, const void* bias, const void* res,
                     const void* gamma, const void* beta, void* h, void* y, int64_t R,
                     int H, float eps, bool rms, hipStream_t stream);

// res_norm.hip
bool norm_wave_path(int H, int vec);
int norm_bwd_fused_blocks(int64_t R);
BF16_F32(int, ln_bwd_fused, const void* dy, const void* x, const void* gamma,
         const float* mean, const float* rstd, const void* dres, void* dx,
         float* partial, bool wbeta, int64_t R, int H, int P, bool rms,
         hipStream_t stream);
void res_drop_ln_fwd_bf16(const void* x, const void* bias, const void* res,
                          const void* gamma, const void* beta, void* h, void* y,
                          float* mean, float* rstd, int64_t R, int H, float eps,
                          bool rms, float p, uint64_t seed, hipStream_t stream);
int res_drop_ln_bwd_bf16(const void* dy, const void* h, const void* gamma,
                         const float* mean, const float* rstd, const void* dres,
                         void* dh, void* dxd, float* partial, bool wbeta, bool wbias,
                         int64_t R, int H, int P, bool rms, float p, uint64_t seed,
                         hipStream_t stream);

// fused_bias.hip
int bias_col_grid_rows(int64_t n, int W, int V);
BF16_F32(void, bias_gelu_fwd, const void* x, const void* b, void* y, int64_t n, int W,
         hipStream_t stream);
BF16_F32(void, bias_gelu_bwd, const void* x, const void* b, const void* dy, void* dx,
         float* db_partial, int64_t n, int W, hipStream_t stream);
BF16_F32(void, bias_dropout_res_fwd, const void* x, const void* b, const void* res,
         void* y, int64_t n, int W, float p, uint64_t seed, hipStream_t stream);
BF16_F32(void, bias_dropout_res_bwd, const void* dy, void* dx, float* db_partial,
         int64_t n, int W, float p, uint64_t seed, hipStream_t stream);
BF16_F32(void, colsum, const void* in, float* partial, void* out, int64_t R, int W,
         int P, hipStream_t stream);

// softmax.hip
BF16_F32(void, softmax_fwd, const void* s, const uint8_t* pad_mask, void* out,
         int64_t B, int NH, int SQ, int SK, float scale, float p, uint64_t seed,
         bool causal, hipStream_t stream);
BF16_F32(void, softmax_bwd, const void* s, const void* dout, const uint8_t* pad_mask,
         void* ds, int64_t B, int NH, int SQ, int SK, float scale, float p,
         uint64_t seed, bool causal, hipStream_t stream);

// cross_entropy.hip
BF16_F32(void, ce_fwd, const void* logits, const int64_t* targets, float* lmax,
         float* lsumexp, float* tlogit, int64_t R, int64_t Vl, int64_t vocab_start,
         int64_t ignore_index, hipStream_t stream);
BF16_F32(void, ce_bwd, const void* logits, const int64_t* targets, const float* gmax,
         const float* gsumexp, const float* gscale, void* dlogits, int64_t R,
         int64_t Vl, int64_t vocab_start, int64_t ignore_index, hipStream_t stream);

// embedding.hip
BF16_F32(void, embedding_fwd, const int64_t* ids, const void* w, void* out, int64_t N,
         int64_t H, int64_t vocab_start, int64_t vocab_local, hipStream_t stream);
BF16_F32(void, embedding_bwd, const int64_t* ids, const void* dout, float* ws,
         int64_t N, int64_t H, int64_t vocab_start, int64_t vocab_local,
         int64_t padding_row, hipStream_t stream);

// gemm_dw.hip
void gemm_dw_bf16(const void* dy, const void* x, float* ws, void* out,
                  int out_is_bf16, int64_t M, int64_t N, int64_t K, int64_t splits,
                  hipStream_t stream);

// rope_swiglu.hip: x/out [B, S, NH, HS] with element strides (sb, ss, sh) and
// (ob, os, oh)
BF16_F32(void, rope_fwd, const void* x, void* out, const float* cos_t,
         const float* sin_t, int64_t sb, int64_t ss, int64_t sh, int64_t ob, int64_t os,
         int64_t oh, int B, int S, int NH, int HS, int pos0, const int* pos_ids,
         int n_pos, hipStream_t stream);
BF16_F32(void, rope_bwd, const void* dy, void* dx, const float* cos_t,
         const float* sin_t, int64_t sb, int64_t ss, int64_t sh, int64_t ob, int64_t os,
         int64_t oh, int B, int S, int NH, int HS, int pos0, const int* pos_ids,
         int n_pos, hipStream_t stream);
void rope_kv_insert_bf16(const void* q, const void* k, const void* v, void* qo,
                         void* ck, void* cv, const float* cos_t, const float* sin_t,
                         const long long* pos_p, int B, int NH, int KVH, int HD,
                         int64_t max_len, int64_t q_sb, int64_t q_sh, int64_t k_sb,
                         int64_t k_sh, int64_t v_sb, int64_t v_sh, int rotate,
                         int per_batch_pos, hipStream_t stream);
BF16_F32(void, swiglu_fwd, const void* x, void* y, int64_t rows, int F,
         hipStream_t stream);
BF16_F32(void, swiglu_bwd, const void* x, const void* dy, void* dx, int64_t rows, int F,
         hipStream_t stream);

// quant_fp8.hip
void quant_fp8_bf16(const void* x, void* out, const float* scale, float* amax,
                    int64_t n, hipStream_t stream);

// adamw.hip
int adamw_chunk_elems();
BF16_F32(void, adamw_step, const void* chunks, int nchunks, float lr, float beta1,
         float beta2, float eps, float wd, float bc1, float bc2, float grad_scale,
         hipStream_t stream);
BF16_F32(void, l2norm_sq, const void* chunks, int nchunks, float* out,
         hipStream_t stream);

}  // extern "C"

#undef BF16_F32
