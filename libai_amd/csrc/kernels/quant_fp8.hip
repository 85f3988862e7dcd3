// Single-pass bf16 -> fp8(e4m3, OCP) quantize with delayed scaling
// (transformer-engine idiom): write out[i] = sat(x[i] / scale) using the
// PREVIOUS step's scale (device pointer), and accumulate this tensor's
// amax (one atomic per block) so the host-side wrapper derives the NEXT
// scale without a separate amax pass.  This replaces the 3-pass python
// quantize (amax read + scale-mul + cast = ~0.23 ms at the qkv activation
// shape, more than the fp8 GEMM saves) with one ~19 us read+write pass.
//
// Capability context: the fp8 forward-GEMM option (libai_amd/ops/fp8.py);
// reference has no fp8 path (fp16 AMP only, libai graph_base.py:54-61).
#include <hip/hip_fp8.h>

#include "common.h"
#include "launchers.h"

namespace {

typedef uint8_t u8x8 __attribute__((ext_vector_type(8)));

// atomicMax on non-negative floats via int reinterpretation (IEEE order)
__device__ __forceinline__ void atomic_max_pos(float* addr, float v) {
  atomicMax(reinterpret_cast<int*>(addr), __float_as_int(v));
}

__global__ void quant_fp8_kernel(const uint16_t* __restrict__ x,
                                 uint8_t* __restrict__ out,
                                 const float* __restrict__ scale,
                                 float* __restrict__ amax, int64_t n) {
  const float inv = 1.0f / scale[0];
  float local = 0.0f;
  // 8 elements per thread per trip: one b128 load, one b64 store
  const int64_t stride = (int64_t)gridDim.x * blockDim.x * 8;
  for (int64_t base = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) * 8;
       base < n; base += stride) {
    if (base + 8 <= n) {
      u16x8 xv = *reinterpret_cast<const u16x8*>(x + base);
      uint32_t o[2];
#pragma unroll
      for (int q = 0; q < 2; ++q) {
        float v0 = bf2f(xv[4 * q + 0]), v1 = bf2f(xv[4 * q + 1]);
        float v2 = bf2f(xv[4 * q + 2]), v3 = bf2f(xv[4 * q + 3]);
        local = fmaxf(local, fmaxf(fmaxf(fabsf(v0), fabsf(v1)),
                                   fmaxf(fabsf(v2), fabsf(v3))));
        // native packed cvt (v_cvt_pk_fp8_f32): 2 elems/instruction.
        // The instruction does NOT saturate (overflow -> NaN), so clamp to
        // +-448 first (measured: unclamped cvt NaN'd the training test)
        auto sat = [&](float v) { return fminf(fmaxf(v * inv, -448.f), 448.f); };
        uint32_t r = 0;
        r = __builtin_amdgcn_cvt_pk_fp8_f32(sat(v0), sat(v1), r, false);
        r = __builtin_amdgcn_cvt_pk_fp8_f32(sat(v2), sat(v3), r, true);
        o[q] = r;
      }
      *reinterpret_cast<uint64_t*>(out + base) =
          ((uint64_t)o[1] << 32) | o[0];
    } else {
      for (int64_t i = base; i < n; ++i) {
        float v = bf2f(x[i]);
        local = fmaxf(local, fabsf(v));
        out[i] = (uint8_t)__hip_cvt_float_to_fp8(v * inv, __HIP_SATFINITE,
                                                 __HIP_E4M3);
      }
    }
  }
  // wave-then-LDS reduce, one atomic per block
  __shared__ float red[4];
  for (int off = 32; off; off >>= 1)
    local = fmaxf(local, __shfl_down(local, off, 64));
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) red[wave] = local;
  __syncthreads();
  if (threadIdx.x == 0) {
    float m = red[0];
    for (int w = 1; w < (int)(blockDim.x >> 6); ++w) m = fmaxf(m, red[w]);
    atomic_max_pos(amax, m);
  }
}

}  // namespace

extern "C" void quant_fp8_bf16(const void* x, void* out, const float* scale,
                               float* amax, int64_t n, hipStream_t stream) {
  const int64_t blocks64 = CDIV(n, 256 * 8);
  const int blocks = (int)(blocks64 < 4096 ? blocks64 : 4096);
  quant_fp8_kernel<<<dim3(blocks), 256, 0, stream>>>(
      (const uint16_t*)x, (uint8_t*)out, scale, amax, n);
}
