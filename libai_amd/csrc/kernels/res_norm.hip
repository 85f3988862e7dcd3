// Training kernels for the pre-LN residual chain on gfx950 (wave path:
// H % VEC == 0 and at most 4 vectors per lane, i.e. H <= 2048 bf16).
//
//   res_drop_norm_fwd_wave_kernel   h = (x + bias) * keep + res,  y = norm(h)
//   norm_bwd_fused_wave_kernel      dx of the norm (+ the gradient arriving on
//                                   the residual branch), the dropout backward
//                                   of that sum, and the dgamma / dbeta / dbias
//                                   partials -- all in ONE pass over dy and x
//
// Every element is computed with the expressions of the kernels they stand
// in for (norm_fwd_wave / norm_bwd_dx_wave in layer_norm.hip,
// bias_dropout_res in fused_bias.hip), so h, y, dx and the residual gradient
// are bit-identical to the separate kernels plus torch's add.  The weight
// gradients differ in summation order only: a lane accumulates its own
// columns in fp32 registers across the rows of its wave, the waves of a block
// fold through LDS in wave order, and each block writes one partial row
// (no float atomics: the result is the same from run to run).
#include "common.h"
#include "launchers.h"

// Bit-identity with the separate kernels needs the same roundings, and which
// products hipcc contracts into an fma there depends on the code around
// them.  So nothing is contracted implicitly in this file; the fmas the
// separate kernels' ISA has (checked with `hipcc -S`: norm_fwd_wave and
// norm_bwd_dx_wave in layer_norm.hip, bias_dropout_res in fused_bias.hip)
// are written out with __builtin_fmaf, everything else is a rounded product
// followed by a rounded sum.
#pragma clang fp contract(off)

namespace {

// 4 keep factors (scale or 0) per hash draw, as in bias_dropout_res_kernel:
// draw index = flat element index / 4, byte j of the draw decides element j
template <int V>
__device__ __forceinline__ void drop_keep(float (&keep)[V], uint64_t seed,
                                          uint64_t vec_idx, uint32_t thr8,
                                          float scale) {
#pragma unroll
  for (int q = 0; q < V / 4; ++q) {
    const uint32_t h = rnd_hash(seed, vec_idx * (V / 4) + q);
#pragma unroll
    for (int j = 0; j < 4; ++j)
      keep[q * 4 + j] = (((h >> (j * 8)) & 0xFFu) >= thr8) ? scale : 0.f;
  }
}

// One wave per row.  BIAS / DROP are compile-time so the element loop has no
// branch; stats are taken on the STORED (rounded) h, which is what a separate
// norm kernel would read back.
template <class E, bool RMS, int NV, bool DROP, bool BIAS>
__global__ void res_drop_norm_fwd_wave_kernel(
    const typename E::T* __restrict__ x, const typename E::T* __restrict__ bias,
    const typename E::T* __restrict__ res, const typename E::T* __restrict__ gamma,
    const typename E::T* __restrict__ beta, typename E::T* __restrict__ h,
    typename E::T* __restrict__ y, float* __restrict__ mean_out,
    float* __restrict__ rstd_out, int H, float eps, int64_t R, float p,
    uint64_t seed) {
  using T = typename E::T;
  using VecT = typename E::VecT;
  constexpr int V = E::VEC;
  const int wave = threadIdx.x >> 6;
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * (blockDim.x >> 6) + wave;
  if (row >= R) return;
  const T* xr = x + row * (int64_t)H;
  const T* rr = res + row * (int64_t)H;
  T* hr = h + row * (int64_t)H;
  T* yr = y + row * (int64_t)H;
  const int nvec = H / V;
  const float scale = 1.0f / (1.0f - p);
  const uint32_t thr8 = drop_threshold_u8(p);

  VecT vh[NV];
  float sum = 0.f, sumsq = 0.f;
#pragma unroll
  for (int n = 0; n < NV; ++n) {
    const int i = lane + n * 64;
    if (i < nvec) {
      VecT vx = ((const VecT*)xr)[i];
      VecT vr = ((const VecT*)rr)[i];
      VecT vb;
      if (BIAS) vb = ((const VecT*)bias)[i];
      float keep[V];
      if (DROP) drop_keep<V>(keep, seed, (uint64_t)(row * nvec + i), thr8, scale);
#pragma unroll
      for (int j = 0; j < V; ++j) {
        // ((x + bias) * keep) + res, the association of bias_dropout_res
        // (which adds 0.f for a missing bias; kept, it turns -0 into +0)
        const float v = E::to_f(vx[j]) + (BIAS ? E::to_f(vb[j]) : 0.f);
        vh[n][j] = E::from_f(DROP ? __builtin_fmaf(v, keep[j], E::to_f(vr[j]))
                                  : v + E::to_f(vr[j]));
        const float g = E::to_f(vh[n][j]);
        sum += g;
        sumsq += g * g;  // product rounded, as in norm_fwd_wave_kernel
      }
      ((VecT*)hr)[i] = vh[n];
    }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    sum += __shfl_xor(sum, off, 64);
    sumsq += __shfl_xor(sumsq, off, 64);
  }
  const float mean = RMS ? 0.f : sum / H;
  const float rstd =
      rsqrtf((RMS ? sumsq / H : __builtin_fmaf(-mean, mean, sumsq / H)) + eps);
  if (lane == 0) {
    if (!RMS) mean_out[row] = mean;
    rstd_out[row] = rstd;
  }
#pragma unroll
  for (int n = 0; n < NV; ++n) {
    const int i = lane + n * 64;
    if (i < nvec) {
      VecT g = ((const VecT*)gamma)[i];
      VecT o;
      if (!RMS && beta != nullptr) {
        VecT b = ((const VecT*)beta)[i];
#pragma unroll
        for (int j = 0; j < V; ++j)
          o[j] = E::from_f(__builtin_fmaf((E::to_f(vh[n][j]) - mean) * rstd,
                                          E::to_f(g[j]), E::to_f(b[j])));
      } else {
#pragma unroll
        for (int j = 0; j < V; ++j)
          o[j] = E::from_f((E::to_f(vh[n][j]) - mean) * rstd * E::to_f(g[j]));
      }
      ((VecT*)yr)[i] = o;
    }
  }
}

// Single-pass norm backward.  Waves stride over the rows; a row's dy, x and
// gamma stay in registers between the two row sums and the dx pass.
//   dh  = bf16(dx_ln)                      (DRES = false)
//       = bf16(bf16(dx_ln) + dres)         (DRES: round, add in fp32, round --
//                                           what a separate kernel followed by
//                                           torch's add gives)
//   dxd = bf16(dh * keep)                  (DROP: gradient of the GEMM output)
// Partials, one row of K * H floats per block: dgamma | dbeta (if wbeta) |
// dbias (DBIAS: column sums of dh * keep, or of dh when there is no dropout).
template <class E, bool RMS, int NV, bool DRES, bool DROP, bool DBIAS>
__global__ void __launch_bounds__(256) norm_bwd_fused_wave_kernel(
    const typename E::T* __restrict__ dy, const typename E::T* __restrict__ x,
    const typename E::T* __restrict__ gamma, const float* __restrict__ mean_in,
    const float* __restrict__ rstd_in, const typename E::T* __restrict__ dres,
    typename E::T* __restrict__ dh, typename E::T* __restrict__ dxd,
    float* __restrict__ partial, bool wbeta, int H, int64_t R, float p,
    uint64_t seed) {
  using T = typename E::T;
  using VecT = typename E::VecT;
  constexpr int V = E::VEC;
  constexpr int HV = V / 4;  // float4 pieces per vector
  extern __shared__ __attribute__((aligned(16))) float red[];
  f32x4* red4 = (f32x4*)red;

  const int wave = threadIdx.x >> 6;
  const int lane = threadIdx.x & 63;
  const int nw = blockDim.x >> 6;
  const int nvec = H / V;
  const float scale = 1.0f / (1.0f - p);
  const uint32_t thr8 = drop_threshold_u8(p);

  VecT vg[NV];
  float dg[NV][V], db[NV][V], dbi[DBIAS ? NV : 1][V];
#pragma unroll
  for (int n = 0; n < NV; ++n) {
    const int i = lane + n * 64;
    if (i < nvec) vg[n] = ((const VecT*)gamma)[i];
#pragma unroll
    for (int j = 0; j < V; ++j) {
      dg[n][j] = 0.f;
      db[n][j] = 0.f;
      if (DBIAS) dbi[n][j] = 0.f;
    }
  }

  for (int64_t row = (int64_t)blockIdx.x * nw + wave; row < R;
       row += (int64_t)gridDim.x * nw) {
    const T* dyr = dy + row * (int64_t)H;
    const T* xr = x + row * (int64_t)H;
    const float mean = RMS ? 0.f : mean_in[row];
    const float rstd = rstd_in[row];

    VecT vdy[NV], vx[NV], vdr[DRES ? NV : 1];
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int n = 0; n < NV; ++n) {
      const int i = lane + n * 64;
      if (i < nvec) {
        vdy[n] = ((const VecT*)dyr)[i];
        vx[n] = ((const VecT*)xr)[i];
        if (DRES) vdr[n] = ((const VecT*)(dres + row * (int64_t)H))[i];
#pragma unroll
        for (int j = 0; j < V; ++j) {
          const float dyg = E::to_f(vdy[n][j]) * E::to_f(vg[n][j]);
          const float xhat = (E::to_f(vx[n][j]) - mean) * rstd;
          s1 += dyg;
          s2 += dyg * xhat;
        }
      }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      s1 += __shfl_xor(s1, off, 64);
      s2 += __shfl_xor(s2, off, 64);
    }
    s1 /= H;
    s2 /= H;
#pragma unroll
    for (int n = 0; n < NV; ++n) {
      const int i = lane + n * 64;
      if (i < nvec) {
        float keep[V];
        if (DROP) drop_keep<V>(keep, seed, (uint64_t)(row * nvec + i), thr8, scale);
        VecT o, od;
#pragma unroll
        for (int j = 0; j < V; ++j) {
          const float dyv = E::to_f(vdy[n][j]);
          const float xhat = (E::to_f(vx[n][j]) - mean) * rstd;
          // LN: fma(-xhat, s2, fma(dy, g, -s1));  RMS: fma(dy, g, -(xhat * s2)),
          // except that the one fp32 RMS instantiation with 2 vectors per
          // lane of norm_bwd_dx_wave_kernel was compiled to the other
          // contraction, fma(-xhat, s2, dy * g): followed here, so that
          // every variant keeps the bits it always produced
          constexpr bool kRmsFmaOnS2 = sizeof(T) == 4 && NV == 2;
          const float gj = E::to_f(vg[n][j]);
          const float u =
              !RMS ? __builtin_fmaf(-xhat, s2, __builtin_fmaf(dyv, gj, -s1))
              : kRmsFmaOnS2 ? __builtin_fmaf(-xhat, s2, dyv * gj)
                            : __builtin_fmaf(dyv, gj, -(xhat * s2));
          o[j] = E::from_f(rstd * u);
          if (DRES) o[j] = E::from_f(E::to_f(o[j]) + E::to_f(vdr[n][j]));
          dg[n][j] += dyv * (E::to_f(vx[n][j]) - mean) * rstd;
          db[n][j] += dyv;
          if (DROP) {
            const float g = E::to_f(o[j]) * keep[j];
            od[j] = E::from_f(g);
            if (DBIAS) dbi[n][j] += g;
          } else if (DBIAS) {
            dbi[n][j] += E::to_f(o[j]);
          }
        }
        ((VecT*)(dh + row * (int64_t)H))[i] = o;
        if (DROP) ((VecT*)(dxd + row * (int64_t)H))[i] = od;
      }
    }
  }

  // fold the block's waves in wave order; slot layout [k][n][piece][lane]
  // keeps every LDS access 16 bytes wide and lane-contiguous
  const int kbeta = 1, kbias = wbeta ? 2 : 1;
  for (int w = 0; w < nw; ++w) {
    if (wave == w) {
#pragma unroll
      for (int n = 0; n < NV; ++n) {
#pragma unroll
        for (int q = 0; q < HV; ++q) {
          const int s0 = (n * HV + q) * 64 + lane;
          const int sb = ((kbeta * NV + n) * HV + q) * 64 + lane;
          const int sx = ((kbias * NV + n) * HV + q) * 64 + lane;
          f32x4 a = {dg[n][q * 4], dg[n][q * 4 + 1], dg[n][q * 4 + 2],
                     dg[n][q * 4 + 3]};
          if (w > 0) a = red4[s0] + a;
          red4[s0] = a;
          if (wbeta) {
            f32x4 b = {db[n][q * 4], db[n][q * 4 + 1], db[n][q * 4 + 2],
                       db[n][q * 4 + 3]};
            if (w > 0) b = red4[sb] + b;
            red4[sb] = b;
          }
          if (DBIAS) {
            f32x4 c = {dbi[n][q * 4], dbi[n][q * 4 + 1], dbi[n][q * 4 + 2],
                       dbi[n][q * 4 + 3]};
            if (w > 0) c = red4[sx] + c;
            red4[sx] = c;
          }
        }
      }
    }
    __syncthreads();
  }
  const int K = 1 + (wbeta ? 1 : 0) + (DBIAS ? 1 : 0);
  const int H4 = H / 4;
  f32x4* prow = (f32x4*)(partial + (int64_t)blockIdx.x * K * H);
  for (int c = threadIdx.x; c < K * H4; c += blockDim.x) {
    const int k = c / H4, c4 = c - k * H4;
    const int i = c4 / HV, q = c4 - i * HV;
    prow[c] = red4[((k * NV + (i >> 6)) * HV + q) * 64 + (i & 63)];
  }
}

constexpr int kBwdThreads = 256;     // 4 waves
constexpr int kBwdMaxBlocks = 1024;  // bounds the [P, K*H] partial buffer

// Starts as many blocks as the chip holds at once for this instantiation
// (so that the row loops all run in one round), at most `maxP`; returns the
// number started = the number of partial rows written.
template <class E, bool RMS, int NV, bool DRES, bool DROP, bool DBIAS>
int launch_bwd_inst(const void* dy, const void* x, const void* gamma,
                    const float* mean, const float* rstd, const void* dres,
                    void* dh, void* dxd, float* partial, bool wbeta, int64_t R,
                    int H, int maxP, float p, uint64_t seed, hipStream_t stream) {
  using T = typename E::T;
  auto kern = norm_bwd_fused_wave_kernel<E, RMS, NV, DRES, DROP, DBIAS>;
  const size_t lds = (size_t)3 * NV * E::VEC * 64 * sizeof(float);
  static int resident = 0;
  if (resident == 0) {
    int dev = 0, cus = 0, per = 0;
    if (hipGetDevice(&dev) != hipSuccess ||
        hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) !=
            hipSuccess ||
        hipOccupancyMaxActiveBlocksPerMultiprocessor(&per, kern, kBwdThreads, lds) !=
            hipSuccess)
      cus = per = 0;
    resident = cus * per > 0 ? cus * per : kBwdMaxBlocks;
  }
  const int P = resident < maxP ? resident : maxP;
  kern<<<dim3(P), dim3(kBwdThreads), lds, stream>>>(
      (const T*)dy, (const T*)x, (const T*)gamma, mean, rstd, (const T*)dres, (T*)dh,
      (T*)dxd, partial, wbeta, H, R, p, seed);
  return P;
}

template <class E, bool RMS, int NV, bool DROP, bool DBIAS>
int launch_bwd_dres(const void* dy, const void* x, const void* gamma,
                     const float* mean, const float* rstd, const void* dres,
                     void* dh, void* dxd, float* partial, bool wbeta, int64_t R,
                     int H, int P, float p, uint64_t seed, hipStream_t stream) {
  if (dres != nullptr)
    return launch_bwd_inst<E, RMS, NV, true, DROP, DBIAS>(
        dy, x, gamma, mean, rstd, dres, dh, dxd, partial, wbeta, R, H, P, p, seed,
        stream);
  return launch_bwd_inst<E, RMS, NV, false, DROP, DBIAS>(
      dy, x, gamma, mean, rstd, dres, dh, dxd, partial, wbeta, R, H, P, p, seed,
      stream);
}

template <class E, bool DROP, bool DBIAS>
int launch_bwd(const void* dy, const void* x, const void* gamma, const float* mean,
                const float* rstd, const void* dres, void* dh, void* dxd,
                float* partial, bool wbeta, int64_t R, int H, int P, bool rms,
                float p, uint64_t seed, hipStream_t stream) {
  const int nvl = CDIV(H / E::VEC, 64);
#define BWD_NV(RMS_, NV_)                                                     \
  return launch_bwd_dres<E, RMS_, NV_, DROP, DBIAS>(dy, x, gamma, mean, rstd, \
                                                    dres, dh, dxd, partial,   \
                                                    wbeta, R, H, P, p, seed,  \
                                                    stream)
#define BWD_RMS(RMS_)  \
  if (nvl <= 1)        \
    BWD_NV(RMS_, 1);   \
  else if (nvl == 2)   \
    BWD_NV(RMS_, 2);   \
  else                 \
    BWD_NV(RMS_, 4)
  if (rms) {
    BWD_RMS(true);
  } else {
    BWD_RMS(false);
  }
#undef BWD_RMS
#undef BWD_NV
}

template <class E, bool RMS, bool DROP, bool BIAS>
void launch_fwd(const void* x, const void* bias, const void* res, const void* gamma,
                const void* beta, void* h, void* y, float* mean, float* rstd,
                int64_t R, int H, float eps, float p, uint64_t seed,
                hipStream_t stream) {
  using T = typename E::T;
  const int nvl = CDIV(H / E::VEC, 64);
  dim3 g((uint32_t)CDIV(R, 4));
#define FWD_NV(NV_)                                                              \
  res_drop_norm_fwd_wave_kernel<E, RMS, NV_, DROP, BIAS>                         \
      <<<g, dim3(256), 0, stream>>>((const T*)x, (const T*)bias, (const T*)res,  \
                                    (const T*)gamma, (const T*)beta, (T*)h,      \
                                    (T*)y, mean, rstd, H, eps, R, p, seed)
  if (nvl <= 1)
    FWD_NV(1);
  else if (nvl == 2)
    FWD_NV(2);
  else
    FWD_NV(4);
#undef FWD_NV
}

}  // namespace

// the wave path: whole 16-byte vectors, at most 4 of them per lane
extern "C" bool norm_wave_path(int H, int vec) {
  return H >= vec && H % vec == 0 && CDIV(H / vec, 64) <= 4;
}

// upper bound on the blocks (= partial rows) of the single-pass backward for
// R rows; the launchers return how many they started
extern "C" int norm_bwd_fused_blocks(int64_t R) {
  const int64_t g = CDIV(R, (int64_t)(kBwdThreads / 64));
  return (int)(g < kBwdMaxBlocks ? (g < 1 ? 1 : g) : kBwdMaxBlocks);
}

// single-pass norm backward (no dropout, no bias): partial is [P, K * H]
#define NORM_BWD_FUSED(SUFF, ETYPE)                                              \
  extern "C" int ln_bwd_fused_##SUFF(                                            \
      const void* dy, const void* x, const void* gamma, const float* mean,       \
      const float* rstd, const void* dres, void* dx, float* partial, bool wbeta, \
      int64_t R, int H, int P, bool rms, hipStream_t stream) {                   \
    return launch_bwd<ETYPE, false, false>(dy, x, gamma, mean, rstd, dres, dx,   \
                                           nullptr, partial, wbeta, R, H, P,     \
                                           rms, 0.f, 0, stream);                 \
  }

NORM_BWD_FUSED(bf16, BF16Elem)
NORM_BWD_FUSED(f32, F32Elem)

extern "C" void res_drop_ln_fwd_bf16(const void* x, const void* bias, const void* res,
                                     const void* gamma, const void* beta, void* h,
                                     void* y, float* mean, float* rstd, int64_t R,
                                     int H, float eps, bool rms, float p,
                                     uint64_t seed, hipStream_t stream) {
#define FWD_ARGS x, bias, res, gamma, beta, h, y, mean, rstd, R, H, eps, p, seed, stream
#define FWD_SEL(RMS_)                                      \
  if (p > 0.f) {                                           \
    if (bias)                                              \
      launch_fwd<BF16Elem, RMS_, true, true>(FWD_ARGS);    \
    else                                                   \
      launch_fwd<BF16Elem, RMS_, true, false>(FWD_ARGS);   \
  } else {                                                 \
    if (bias)                                              \
      launch_fwd<BF16Elem, RMS_, false, true>(FWD_ARGS);   \
    else                                                   \
      launch_fwd<BF16Elem, RMS_, false, false>(FWD_ARGS);  \
  }
  if (rms) {
    FWD_SEL(true)
  } else {
    FWD_SEL(false)
  }
#undef FWD_SEL
#undef FWD_ARGS
}

// backward of the fused op: dh (residual gradient), dxd (gradient of the
// GEMM output; only written when p > 0, otherwise it IS dh) and the partials
extern "C" int res_drop_ln_bwd_bf16(const void* dy, const void* h, const void* gamma,
                                     const float* mean, const float* rstd,
                                     const void* dres, void* dh, void* dxd,
                                     float* partial, bool wbeta, bool wbias,
                                     int64_t R, int H, int P, bool rms, float p,
                                     uint64_t seed, hipStream_t stream) {
#define BWD_ARGS \
  dy, h, gamma, mean, rstd, dres, dh, dxd, partial, wbeta, R, H, P, rms, p, seed, stream
  if (p > 0.f) {
    if (wbias) return launch_bwd<BF16Elem, true, true>(BWD_ARGS);
    return launch_bwd<BF16Elem, true, false>(BWD_ARGS);
  }
  if (wbias) return launch_bwd<BF16Elem, false, true>(BWD_ARGS);
  return launch_bwd<BF16Elem, false, false>(BWD_ARGS);
#undef BWD_ARGS
}
