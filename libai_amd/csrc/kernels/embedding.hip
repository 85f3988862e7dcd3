// Embedding gather forward + fused scatter-add backward for gfx950 (K10).
//
// Replaces torch's F.embedding pair on the hot path (reference site:
// libai/layers/embedding.py:85,164 — flow._C.gather + implicit scatter-add
// backward).  The round-1 profile showed torch's embedding backward as
// at::native::reduce_kernel (3.5 ms) + vectorized_elementwise (4.9 ms) on
// GPT-2 345M — ~4% of the step for what is a ~50 MB scatter.
//
// Forward additionally folds the vocab-parallel OOV handling in-kernel
// (ids outside [vocab_start, vocab_start+vocab_local) produce zero rows),
// replacing the python-side sub/clamp/compare/mask-mul chain.
//
// Backward: fp32 atomic scatter into a workspace (dout rows hit distinct
// table rows mostly; fp32 global atomic add is native on CDNA4 and the
// accumulation is HIGHER precision than bf16 in-place adds), followed by a
// torch-side cast into the bf16 grad view.
#include "common.h"
#include "launchers.h"

namespace {

template <class E>
__global__ void embedding_fwd_kernel(const int64_t* __restrict__ ids,
                                     const typename E::T* __restrict__ w,
                                     typename E::T* __restrict__ out, int64_t N,
                                     int64_t H, int64_t vocab_start,
                                     int64_t vocab_local) {
  constexpr int V = E::VEC;
  const int64_t chunks_per_row = H / V;
  const int64_t total = N * chunks_per_row;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total;
       i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t n = i / chunks_per_row;
    const int64_t c = i % chunks_per_row;
    const int64_t row = ids[n] - vocab_start;
    typename E::VecT val{};
    if (row >= 0 && row < vocab_local)
      val = *(const typename E::VecT*)(w + row * H + c * V);
    *(typename E::VecT*)(out + n * H + c * V) = val;
  }
}

template <class E>
__global__ void embedding_bwd_kernel(const int64_t* __restrict__ ids,
                                     const typename E::T* __restrict__ dout,
                                     float* __restrict__ ws, int64_t N, int64_t H,
                                     int64_t vocab_start, int64_t vocab_local,
                                     int64_t padding_row) {
  constexpr int V = E::VEC;
  const int64_t chunks_per_row = H / V;
  const int64_t total = N * chunks_per_row;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total;
       i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t n = i / chunks_per_row;
    const int64_t c = i % chunks_per_row;
    const int64_t row = ids[n] - vocab_start;
    if (row < 0 || row >= vocab_local || row == padding_row) continue;
    typename E::VecT g = *(const typename E::VecT*)(dout + n * H + c * V);
    float* dst = ws + row * H + c * V;
#pragma unroll
    for (int j = 0; j < V; ++j) atomicAdd(dst + j, E::to_f(g[j]));
  }
}

inline uint32_t grid_for(int64_t work) {
  int64_t g = (work + 255) / 256;
  // >> 256 workgroups to fill 8 XCDs; cap so the grid-stride loop amortizes
  if (g > 16384) g = 16384;
  return (uint32_t)(g < 1 ? 1 : g);
}

}  // namespace

#define EMB_LAUNCHERS(SUFF, ETYPE)                                                   \
  extern "C" void embedding_fwd_##SUFF(const int64_t* ids, const void* w, void* out, \
                                       int64_t N, int64_t H, int64_t vocab_start,    \
                                       int64_t vocab_local, hipStream_t stream) {    \
    embedding_fwd_kernel<ETYPE>                                                      \
        <<<dim3(grid_for(N * H / ETYPE::VEC)), dim3(256), 0, stream>>>(              \
            ids, (const ETYPE::T*)w, (ETYPE::T*)out, N, H, vocab_start,              \
            vocab_local);                                                            \
  }                                                                                  \
  extern "C" void embedding_bwd_##SUFF(                                              \
      const int64_t* ids, const void* dout, float* ws, int64_t N, int64_t H,         \
      int64_t vocab_start, int64_t vocab_local, int64_t padding_row,                 \
      hipStream_t stream) {                                                          \
    embedding_bwd_kernel<ETYPE>                                                      \
        <<<dim3(grid_for(N * H / ETYPE::VEC)), dim3(256), 0, stream>>>(              \
            ids, (const ETYPE::T*)dout, ws, N, H, vocab_start, vocab_local,          \
            padding_row);                                                            \
  }

EMB_LAUNCHERS(bf16, BF16Elem)
EMB_LAUNCHERS(f32, F32Elem)
