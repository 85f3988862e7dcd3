// Multi-tensor fused AdamW + grad-norm kernels for gfx950.
//
// Replaces the reference's fused model-update path (OneFlow
// allow_fuse_model_update_ops + param-group clip_grad, reference:
// libai/models/utils/graph_base.py:74-76, libai/optim/build.py:86-88).
//
// The host packs per-chunk descriptors (pointers as int64, chunk length) into
// one device buffer; a single launch updates every parameter chunk.  bf16
// training keeps fp32 master weights: the kernel updates the master and
// rewrites the bf16 model copy in the same pass.  Gradient clipping is a
// multi-tensor squared-L2 kernel + a host-side scalar, applied in the update
// via grad_scale (one pass over grads total).
#include "common.h"
#include "launchers.h"

namespace {

constexpr int CHUNK = 1 << 16;  // elems per chunk (bf16: 128 KiB)

struct AdamChunkDesc {
  // int64 fields so Python can build the buffer as a [N, 6] int64 tensor
  int64_t param;   // bf16 model weights (0 if fp32-native)
  int64_t master;  // fp32 master weights (= param storage when fp32-native)
  int64_t grad;    // gradient (same dtype as param flag of the launcher)
  int64_t m;       // fp32 exp_avg
  int64_t v;       // fp32 exp_avg_sq
  int64_t n;       // number of elements in this chunk
};

struct AdamHyper {
  float lr, beta1, beta2, eps, wd, inv_bc1, inv_bc2, grad_scale;
  float omb1, omb2;  // 1 - beta1, 1 - beta2
};

// One parameter element.  Shared by the vector and the scalar loop, with the
// contractions written out, so that where a parameter sits in its bucket
// (which decides the loop) cannot decide a bit.  The two moment updates are
// contracted the other way round in the two instantiations: that is what the
// compiler made of `beta * m + (1 - beta) * g` in the scalar kernel this one
// replaces, read from that kernel's ISA, so that optimizer states written by
// it should continue bit for bit.  No fixture pins that: the tests compare
// the two loops of this kernel with each other, not with the old one.
template <class E>
__device__ __forceinline__ void adamw_elem(float g, float& p, float& m, float& v,
                                           const AdamHyper& h) {
#pragma clang fp contract(off)
  const float gv = g * h.grad_scale;
  const float t = h.omb2 * gv;
  if constexpr (std::is_same<E, BF16Elem>::value) {
    m = fmaf(h.beta1, m, h.omb1 * gv);
    v = fmaf(h.beta2, v, gv * t);
  } else {
    m = fmaf(h.omb1, gv, h.beta1 * m);
    v = fmaf(gv, t, h.beta2 * v);
  }
  const float mhat = m * h.inv_bc1;
  const float vhat = v * h.inv_bc2;
  p = fmaf(-h.lr, fmaf(h.wd, p, mhat / (sqrtf(vhat) + h.eps)), p);
}

constexpr int AVEC = 8;  // elements per thread and iteration of the vector loops

template <class E>
__global__ void adamw_kernel(const AdamChunkDesc* __restrict__ chunks, float lr,
                             float beta1, float beta2, float eps, float wd,
                             float bc1, float bc2,  // 1-b1^t, 1-b2^t
                             float grad_scale) {
  using VecT = typename E::VecT;
  constexpr int GV = AVEC / E::VEC;  // 16-byte vectors of E per AVEC elements
  const AdamChunkDesc c = chunks[blockIdx.x];
  const int64_t n = c.n;
  typename E::T* p16 = (typename E::T*)c.param;
  float* master = (float*)c.master;
  const typename E::T* g = (const typename E::T*)c.grad;
  float* m = (float*)c.m;
  float* v = (float*)c.v;
  const AdamHyper h = {lr,          beta1,       beta2,      eps,
                       wd,          1.0f / bc1,  1.0f / bc2, grad_scale,
                       1.0f - beta1, 1.0f - beta2};

  // Parameters are views into flat buckets at any element offset: the
  // 16-byte path serves a chunk only if all five of its pointers allow it
  // (uniform over the block, which serves one chunk).  A null param
  // (fp32-native) counts as aligned.
  const bool aligned = ((c.param | c.master | c.grad | c.m | c.v) & 15) == 0;
  const int64_t nvec = aligned ? n - n % AVEC : 0;

  for (int64_t i = (int64_t)threadIdx.x * AVEC; i < nvec;
       i += (int64_t)blockDim.x * AVEC) {
    // all loads of the iteration first: 112 (bf16) / 128 bytes per lane in flight
    VecT vg[GV];
    f32x4 vp[2], vm[2], vv[2];
#pragma unroll
    for (int k = 0; k < GV; ++k) vg[k] = ((const VecT*)(g + i))[k];
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      vp[k] = ((const f32x4*)(master + i))[k];
      vm[k] = ((const f32x4*)(m + i))[k];
      vv[k] = ((const f32x4*)(v + i))[k];
    }
    VecT o[GV];
#pragma unroll
    for (int j = 0; j < AVEC; ++j) {
      float pv = vp[j / 4][j % 4], mv = vm[j / 4][j % 4], sv = vv[j / 4][j % 4];
      adamw_elem<E>(E::to_f(vg[j / E::VEC][j % E::VEC]), pv, mv, sv, h);
      vp[j / 4][j % 4] = pv;
      vm[j / 4][j % 4] = mv;
      vv[j / 4][j % 4] = sv;
      o[j / E::VEC][j % E::VEC] = E::from_f(pv);
    }
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      ((f32x4*)(m + i))[k] = vm[k];
      ((f32x4*)(v + i))[k] = vv[k];
      ((f32x4*)(master + i))[k] = vp[k];
    }
    if (p16) {
#pragma unroll
      for (int k = 0; k < GV; ++k) ((VecT*)(p16 + i))[k] = o[k];
    }
  }

  // unaligned chunks, and the tail shorter than a vector
  for (int64_t i = nvec + threadIdx.x; i < n; i += blockDim.x) {
    float pv = master[i], mv = m[i], sv = v[i];
    adamw_elem<E>(E::to_f(g[i]), pv, mv, sv, h);
    m[i] = mv;
    v[i] = sv;
    master[i] = pv;
    if (p16) p16[i] = E::from_f(pv);
  }
}

struct NormChunkDesc {
  int64_t ptr;
  int64_t n;
};

template <class E>
__global__ void l2norm_sq_kernel(const NormChunkDesc* __restrict__ chunks,
                                 float* __restrict__ out) {
  __shared__ float red[16];
  const NormChunkDesc c = chunks[blockIdx.x];
  const typename E::T* x = (const typename E::T*)c.ptr;
  using VecT = typename E::VecT;
  constexpr int V = E::VEC;
  float s = 0.f;
  // 16-byte loads where the chunk's pointer allows them (see adamw_kernel);
  // the loads of the unrolled iterations do not depend on each other
  const int64_t nvec = (c.ptr & 15) == 0 ? c.n - c.n % V : 0;
#pragma unroll 4
  for (int64_t i = (int64_t)threadIdx.x * V; i < nvec; i += (int64_t)blockDim.x * V) {
    const VecT vx = *(const VecT*)(x + i);
#pragma unroll
    for (int j = 0; j < V; ++j) {
      float v = E::to_f(vx[j]);
      s += v * v;
    }
  }
  for (int64_t i = nvec + threadIdx.x; i < c.n; i += blockDim.x) {
    float v = E::to_f(x[i]);
    s += v * v;
  }
  s = block_reduce(s, red, SumOp(), 0.f);
  if (threadIdx.x == 0) atomicAdd(out, s);
}

}  // namespace

extern "C" int adamw_chunk_elems() { return CHUNK; }

#define ADAMW_LAUNCHERS(SUFF, ETYPE)                                                   \
  extern "C" void adamw_step_##SUFF(const void* chunks, int nchunks, float lr,         \
                                    float beta1, float beta2, float eps, float wd,     \
                                    float bc1, float bc2, float grad_scale,            \
                                    hipStream_t stream) {                              \
    adamw_kernel<ETYPE><<<dim3(nchunks), dim3(256), 0, stream>>>(                      \
        (const AdamChunkDesc*)chunks, lr, beta1, beta2, eps, wd, bc1, bc2,             \
        grad_scale);                                                                   \
  }                                                                                    \
  extern "C" void l2norm_sq_##SUFF(const void* chunks, int nchunks, float* out,        \
                                   hipStream_t stream) {                               \
    l2norm_sq_kernel<ETYPE><<<dim3(nchunks), dim3(256), 0, stream>>>(                  \
        (const NormChunkDesc*)chunks, out);                                            \
  }

ADAMW_LAUNCHERS(bf16, BF16Elem)
ADAMW_LAUNCHERS(f32, F32Elem)
