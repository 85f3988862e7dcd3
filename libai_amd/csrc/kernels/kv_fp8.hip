// FP8 (OCP e4m3) KV cache for the captured decode step on gfx950: the
// quantizing insert, the prefill row quantizer and a GQA-packed MFMA decode
// kernel (docs/kernels.md "FP8 KV cache").
//
// Cache format: k8 / v8 [B, KVH, MAX, HD] one byte per element, plus one fp32
// scale per (token, KV head) row, k_scale / v_scale [B, KVH, MAX]:
//   scale = amax(row) / 448 (1.0 for an all-zero row)
//   byte  = e4m3_rne(clamp(x / scale, +-448))
// where the row is the bf16-rounded row the bf16 cache would hold.  The clamp
// comes before the convert: v_cvt_pk_fp8_f32 does not saturate (quant_fp8.hip).
//
// Decode: one workgroup per (batch, KV head, 512-key split) serves all G <= 8
// query heads of the KV head from ONE pass over its keys.  Each wave walks
// 32-key tiles of the split:
//   S[key][g] = K . Q^T   v_mfma_f32_32x32x16_bf16, keys as rows, the query
//                         heads as columns (columns g >= G are zero and never
//                         stored).  A lane's A fragment is 8 contiguous d of
//                         one key = 8 contiguous cache bytes, so K goes from
//                         global memory to registers and never through LDS.
//                         The contraction index is permuted (lane half `hi`
//                         takes d in [hi * D/2, hi * D/2 + D/2), MFMA step c
//                         its 8 values from c * 8), the same on K and on the Q
//                         fragments, so each lane's K loads are 16 bytes wide.
//   e4m3 -> fp32 -> bf16  packed converts in registers, both exact.
//   softmax               online, fp32, exp2 domain, m and l per column; the
//                         per-key k_scale * softmax_scale multiplies the fp32
//                         score, p * v_scale is repacked to bf16 for PV.
//   O^T[d][g] += V^T . P  V rows are converted to bf16 and staged through a
//                         wave-private LDS image read back transposed with
//                         ds_read_b64_tr_b16 (the flash forward's tr image).
// The four wave states merge through LDS, the splits by flash_decode_fp8_merge
// in index order.  Split boundaries are the fixed multiples of 512, a null
// split is an exact no-op under the merge: outputs do not depend on the cache
// capacity.
//
// Multi-token steps (flash_chunk_fp8): the same walk with the 32 columns packed
// token-major, column = t_local * G + g, 32 / G tokens of one sequence per
// workgroup.  A lane owns one column and so one position: the causal and the
// window bound are per lane, the key walk runs on the column tile's bounds.
#include "common.h"
#include "launchers.h"

namespace {

typedef __bf16 bf16_t;
typedef __bf16 bf16x8_t __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x4_t __attribute__((ext_vector_type(4)));
typedef float f32x16_t __attribute__((ext_vector_type(16)));
typedef float f32x2_t __attribute__((ext_vector_type(2)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

constexpr float E4M3_MAX = 448.f;

__device__ __forceinline__ float row_scale(float amax) {
  return amax > 0.f ? amax / E4M3_MAX : 1.0f;
}

// x / scale, clamped to the e4m3 range (the packed convert does not saturate)
__device__ __forceinline__ float sat_div(float x, float scale) {
  return fminf(fmaxf(x / scale, -E4M3_MAX), E4M3_MAX);
}

// ---------------------------------------------------------------------------
// rope_kv_insert_fp8: the captured-step insert.  Row mapping, positions and
// the q rows exactly as rope_kv_insert_kernel (rope_swiglu.hip); a K or V row
// is rotated / copied, rounded to bf16, its amax reduced over the wave, and
// stored as HD bytes plus one scale.  A lane holds up to two elements of the
// row: j and HD/2 + j when rotating, lane and 64 + lane otherwise.  A step of T
// tokens (q, k, v [B, T, heads, HD]) is one wave per (b, t, head) row at
// position pos[b] + t, each row skipped on its own when it falls outside the
// cache; qo is [B, NH, T, HD].
// ---------------------------------------------------------------------------
template <bool ROT>
__global__ void rope_kv_insert_fp8_kernel(
    const uint16_t* __restrict__ q, const uint16_t* __restrict__ k,
    const uint16_t* __restrict__ v, uint16_t* __restrict__ qo,
    uint8_t* __restrict__ k8, uint8_t* __restrict__ v8,
    float* __restrict__ k_scale, float* __restrict__ v_scale,
    const float* __restrict__ cos_t, const float* __restrict__ sin_t,
    const long long* __restrict__ pos_p, int B, int T, int NH, int KVH, int HD,
    int64_t max_len, int64_t q_sb, int64_t q_st, int64_t q_sh, int64_t k_sb,
    int64_t k_st, int64_t k_sh, int64_t v_sb, int64_t v_st, int64_t v_sh,
    int per_batch_pos) {
  const int half = HD / 2;
  const int rows_per_b = NH + 2 * KVH;
  const int wave = (int)((blockIdx.x * (int64_t)blockDim.x + threadIdx.x) >> 6);
  const int lane = threadIdx.x & 63;
  if (wave >= B * T * rows_per_b) return;
  const int bt = wave / rows_per_b;
  const int r = wave % rows_per_b;
  const int b = bt / T, t = bt % T;
  const int64_t pos = pos_p[per_batch_pos ? b : 0] + t;
  if (pos < 0 || pos >= max_len) return;
  const float* cp = cos_t + pos * half;
  const float* sp = sin_t + pos * half;
  if (r < NH) {  // q head: rotate (or copy) -> qo[b, r, t, :]
    const uint16_t* xp = q + b * q_sb + t * q_st + r * q_sh;
    uint16_t* op = qo + (((int64_t)b * NH + r) * T + t) * HD;
    if constexpr (ROT) {
      for (int j = lane; j < half; j += 64) {
        float a = bf2f(xp[j]), bb = bf2f(xp[half + j]);
        op[j] = f2bf(a * cp[j] - bb * sp[j]);
        op[half + j] = f2bf(bb * cp[j] + a * sp[j]);
      }
    } else {
      for (int j = lane; j < HD; j += 64) op[j] = xp[j];
    }
    return;
  }
  const bool is_k = r < NH + KVH;  // wave-uniform
  const int h = is_k ? r - NH : r - NH - KVH;
  const uint16_t* xp = is_k ? k + b * k_sb + t * k_st + h * k_sh
                            : v + b * v_sb + t * v_st + h * v_sh;
  float x0 = 0.f, x1 = 0.f;
  int j1;
  bool has0, has1;
  if (ROT && is_k) {
    j1 = half + lane;
    has0 = has1 = lane < half;
    if (has0) {
      float a = bf2f(xp[lane]), bb = bf2f(xp[j1]);
      x0 = bf2f(f2bf(a * cp[lane] - bb * sp[lane]));
      x1 = bf2f(f2bf(bb * cp[lane] + a * sp[lane]));
    }
  } else {
    j1 = 64 + lane;
    has0 = lane < HD;
    has1 = j1 < HD;
    if (has0) x0 = bf2f(xp[lane]);
    if (has1) x1 = bf2f(xp[j1]);
  }
  const float scale = row_scale(wave_reduce_max(fmaxf(fabsf(x0), fabsf(x1))));
  const uint32_t pk = (uint32_t)__builtin_amdgcn_cvt_pk_fp8_f32(
      sat_div(x0, scale), sat_div(x1, scale), 0, false);
  const int64_t row = ((int64_t)b * KVH + h) * max_len + pos;
  uint8_t* op = (is_k ? k8 : v8) + row * HD;
  if (has0) op[lane] = (uint8_t)(pk & 0xFF);
  if (has1) op[j1] = (uint8_t)((pk >> 8) & 0xFF);
  if (lane == 0) (is_k ? k_scale : v_scale)[row] = scale;
}

// ---------------------------------------------------------------------------
// kv_quantize_rows: the prefill copy.  src [B, KVH, L, HD] bf16 with element
// strides (last dim contiguous) -> rows [0, L) of dst [B, KVH, MAX, HD] and
// scale [B, KVH, MAX].  One wave per row, one 16-byte load and one 8-byte
// store per active lane.
// ---------------------------------------------------------------------------
__global__ void kv_quantize_rows_kernel(const uint16_t* __restrict__ src,
                                        uint8_t* __restrict__ dst,
                                        float* __restrict__ scale_out,
                                        int64_t s_sb, int64_t s_sh, int64_t s_sl,
                                        int B, int KVH, int L, int HD,
                                        int64_t max_len) {
  const int64_t wave = (blockIdx.x * (int64_t)blockDim.x + threadIdx.x) >> 6;
  const int lane = threadIdx.x & 63;
  if (wave >= (int64_t)B * KVH * L) return;
  const int l = (int)(wave % L);
  const int bh = (int)(wave / L);
  const int b = bh / KVH, h = bh % KVH;
  const bool active = lane < HD / 8;
  float x[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) x[j] = 0.f;
  if (active) {
    const u16x8 xv = *(const u16x8*)(src + b * s_sb + h * s_sh + l * s_sl + lane * 8);
#pragma unroll
    for (int j = 0; j < 8; ++j) x[j] = bf2f(xv[j]);
  }
  float amax = 0.f;
#pragma unroll
  for (int j = 0; j < 8; ++j) amax = fmaxf(amax, fabsf(x[j]));
  const float scale = row_scale(wave_reduce_max(amax));
  uint32_t w[2];
#pragma unroll
  for (int p = 0; p < 2; ++p) {
    uint32_t r = 0;
    r = __builtin_amdgcn_cvt_pk_fp8_f32(sat_div(x[4 * p], scale),
                                        sat_div(x[4 * p + 1], scale), r, false);
    r = __builtin_amdgcn_cvt_pk_fp8_f32(sat_div(x[4 * p + 2], scale),
                                        sat_div(x[4 * p + 3], scale), r, true);
    w[p] = r;
  }
  const int64_t row = (int64_t)bh * max_len + l;
  if (active)
    *(uint64_t*)(dst + row * HD + lane * 8) = ((uint64_t)w[1] << 32) | w[0];
  if (lane == 0) scale_out[row] = scale;
}

// ---------------------------------------------------------------------------
// flash_decode_fp8
// ---------------------------------------------------------------------------
constexpr int SPLIT_KEYS = 512;
constexpr int TK = 32;  // keys per wave tile (the MFMA's rows)
constexpr int MAX_GROUP = 8;

__device__ __forceinline__ uint32_t pack_bf16x2(float lo, float hi) {
  union {
    uint32_t u;
    bf16_t h[2];
  } r;
  r.h[0] = (bf16_t)lo;
  r.h[1] = (bf16_t)hi;
  return r.u;
}

// 8 e4m3 bytes (two words, memory order) -> bf16x8; both converts are exact
__device__ __forceinline__ bf16x8_t fp8x8_to_bf16(uint32_t w0, uint32_t w1) {
  const f32x2_t a = __builtin_amdgcn_cvt_pk_f32_fp8((int)w0, false);
  const f32x2_t b = __builtin_amdgcn_cvt_pk_f32_fp8((int)w0, true);
  const f32x2_t c = __builtin_amdgcn_cvt_pk_f32_fp8((int)w1, false);
  const f32x2_t d = __builtin_amdgcn_cvt_pk_f32_fp8((int)w1, true);
  const uint32_t words[4] = {pack_bf16x2(a[0], a[1]), pack_bf16x2(b[0], b[1]),
                             pack_bf16x2(c[0], c[1]), pack_bf16x2(d[0], d[1])};
  bf16x8_t out;
  memcpy(&out, words, 16);
  return out;
}

// D-layout regs (8 consecutive: rows {0..3}+4hi and {8..11}+4hi of a 16-row
// chunk) -> one contiguous-k bf16x8 fragment (as in flash_attn.hip)
__device__ __forceinline__ bf16x8_t repack_chunk(const float* sv8) {
  uint32_t x0 = pack_bf16x2(sv8[0], sv8[1]);
  uint32_t z0 = pack_bf16x2(sv8[2], sv8[3]);
  uint32_t y0 = pack_bf16x2(sv8[4], sv8[5]);
  uint32_t w0 = pack_bf16x2(sv8[6], sv8[7]);
  auto rx = __builtin_amdgcn_permlane32_swap(x0, y0, false, false);
  auto rz = __builtin_amdgcn_permlane32_swap(z0, w0, false, false);
  uint32_t words[4] = {(uint32_t)rx[0], (uint32_t)rz[0], (uint32_t)rx[1],
                       (uint32_t)rz[1]};
  bf16x8_t out;
  memcpy(&out, words, 16);
  return out;
}

// tr image of a [32][D] bf16 tile, [r/4][d/16][4][16]-blocked: write the 16B
// chunk (row, 8 cols at d0)
template <int D>
__device__ __forceinline__ void tr_img_write(bf16_t* lds, int row, int d0,
                                             bf16x8_t val) {
  int idx = (((row >> 2) * (D / 16) + (d0 >> 4)) * 64) + (row & 3) * 16 + (d0 & 15);
  *(bf16x8_t*)(lds + idx) = val;
}

// transposed fragment: lane gets [rbase + hi*8 + j][dt*32 + l31] for j=0..7
template <int D>
__device__ __forceinline__ bf16x8_t tr_img_frag(const bf16_t* lds, int rbase, int dt,
                                                int lane) {
  const int hi = lane >> 5;
  const int l31 = lane & 31;
  const int r0 = rbase + hi * 8;
  const int d0 = dt * 32 + (l31 & ~15);
  const bf16_t* p0 =
      lds + (((r0 >> 2) * (D / 16) + (d0 >> 4)) * 64) + (lane & 15) * 4;
  const bf16_t* p1 =
      lds + ((((r0 + 4) >> 2) * (D / 16) + (d0 >> 4)) * 64) + (lane & 15) * 4;
  bf16x4_t a = __builtin_amdgcn_ds_read_tr16_b64_v4bf16(
      (__attribute__((address_space(3))) bf16x4_t*)p0);
  bf16x4_t b = __builtin_amdgcn_ds_read_tr16_b64_v4bf16(
      (__attribute__((address_space(3))) bf16x4_t*)p1);
  bf16x8_t out;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    out[j] = a[j];
    out[4 + j] = b[j];
  }
  return out;
}

// orders a wave's own LDS stores before its following LDS reads for the
// compiler; the hardware runs one wave's LDS operations in order
__device__ __forceinline__ void wave_lds_fence() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// part_* are indexed by (b, query head, split): [B, H, S] and [B, H, S, D].
// m is kept in the exp2 domain (scale_log2 = softmax_scale * log2(e)).
template <int D>
__global__ __launch_bounds__(256, 2) void flash_decode_fp8_kernel(
    const bf16_t* __restrict__ q, const uint8_t* __restrict__ k8,
    const uint8_t* __restrict__ v8, const float* __restrict__ k_scale,
    const float* __restrict__ v_scale, float* __restrict__ part_m,
    float* __restrict__ part_l, float* __restrict__ part_acc,
    const int* __restrict__ kv_len, int64_t q_sb, int64_t q_sh, int H, int KVH,
    int G, int S, int Skv, float scale_log2, int window) {
  constexpr int KC = D / 16;    // MFMA steps of the score contraction
  constexpr int DT = D / 32;    // 32-row tiles of O^T
  constexpr int HALF = D / 2;   // row bytes per lane half
  constexpr int NV = HALF / 16; // 16-byte loads per lane and row
  const int tid = threadIdx.x;
  const int wave = tid >> 6;
  const int lane = tid & 63;
  const int l31 = lane & 31, hi = lane >> 5;

  const int split = blockIdx.x % S;
  const int bk = blockIdx.x / S;
  const int b = bk / KVH, hk = bk % KVH;
  const int skv = min((kv_len != nullptr) ? kv_len[b] : Skv, Skv);
  const int lo = split * SPLIT_KEYS;
  const int hi_key = min(lo + SPLIT_KEYS, skv);
  const int win_lo = window > 0 ? max(0, skv - window) : 0;  // first visible key
  const int64_t p_base = ((int64_t)b * H + (int64_t)hk * G) * S + split;  // g = 0

  // null split: exact no-op under the merge
  if (lo >= skv || lo + SPLIT_KEYS <= win_lo) {
    for (int i = tid; i < G * D; i += 256) {
      const int g = i / D, d = i % D;
      const int64_t pidx = p_base + (int64_t)g * S;
      part_acc[pidx * D + d] = 0.f;
      if (d == 0) {
        part_m[pidx] = -3.0e38f;
        part_l[pidx] = 0.f;
      }
    }
    return;
  }

  __shared__ __attribute__((aligned(16))) bf16_t v_lds[4][TK * D];
  __shared__ __attribute__((aligned(16))) float sc_lds[4][2 * TK];
  __shared__ float mrg_m[4][MAX_GROUP], mrg_l[4][MAX_GROUP];
  bf16_t* const v_img = v_lds[wave];
  float* const sc_w = sc_lds[wave];

  // Q as the B operand: column l31 = query head g, zero for g >= G
  bf16x8_t qfrag[KC];
  {
    const bool live = l31 < G;
    const bf16_t* qp = q + b * q_sb + ((int64_t)hk * G + (live ? l31 : 0)) * q_sh +
                       hi * HALF;
#pragma unroll
    for (int c = 0; c < KC; ++c) {
      bf16x8_t z{};
      qfrag[c] = live ? *(const bf16x8_t*)(qp + c * 8) : z;
    }
  }

  const int64_t row0 = ((int64_t)b * KVH + hk) * Skv;
  const uint8_t* kp = k8 + row0 * D + hi * HALF;
  const uint8_t* vp = v8 + row0 * D + hi * HALF;
  const float* scp = (hi ? v_scale : k_scale) + row0;

  float m_run = -3.0e38f, l_run = 0.f;
  f32x16_t oacc[DT];
#pragma unroll
  for (int t = 0; t < DT; ++t) oacc[t] = f32x16_t{};

  // a tile's raw bytes: this lane's half of key row l31 of K and of V (rows
  // past the split's last key repeat that key: finite data, masked below), and
  // one scale per lane (lanes 0..31 k_scale, 32..63 v_scale of key l31)
  auto load_tile = [&](int key0, u32x4* kr, u32x4* vr, float& sc) {
    const int key = key0 + l31;
    const int64_t row = min(key, hi_key - 1);
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      kr[i] = *(const u32x4*)(kp + row * D + i * 16);
      vr[i] = *(const u32x4*)(vp + row * D + i * 16);
    }
    sc = scp[row];
    if (key >= hi_key) sc = 0.f;
  };

  // wave w walks tiles w, w + 4, ... of the split; with a window it starts at
  // its first tile that does not end below win_lo
  int t0 = wave;
  if (window > 0) {
    const int c = max(0, win_lo - lo) / TK;
    t0 = c + ((wave - c) & 3);
  }
  int key0 = lo + t0 * TK;
  u32x4 kn[NV], vn[NV];
  float scn = 0.f;
  if (key0 < hi_key) load_tile(key0, kn, vn, scn);

  for (; key0 < hi_key; key0 += 4 * TK) {
    u32x4 kc[NV], vc[NV];
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      kc[i] = kn[i];
      vc[i] = vn[i];
    }
    const float scc = scn;
    if (key0 + 4 * TK < hi_key) load_tile(key0 + 4 * TK, kn, vn, scn);

    // S[key][g] = K . Q^T
    f32x16_t s{};
#pragma unroll
    for (int c = 0; c < KC; ++c) {
      const bf16x8_t ka =
          fp8x8_to_bf16(kc[c >> 1][(c & 1) * 2], kc[c >> 1][(c & 1) * 2 + 1]);
      s = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ka, qfrag[c], s, 0, 0, 0);
    }

    // V -> bf16 -> the wave's tr image; the scales -> LDS, so that a lane can
    // pick the 16 keys of its score registers
#pragma unroll
    for (int c = 0; c < KC; ++c)
      tr_img_write<D>(v_img, l31, hi * HALF + c * 8,
                      fp8x8_to_bf16(vc[c >> 1][(c & 1) * 2],
                                    vc[c >> 1][(c & 1) * 2 + 1]));
    sc_w[lane] = scc;
    wave_lds_fence();

    // register r of the D layout is key key0 + (r&3) + 8*(r>>2) + 4*hi
    float sv[16], vs[16];
    float pmax = -3.0e38f;
#pragma unroll
    for (int r4 = 0; r4 < 4; ++r4) {
      const f32x4 ks4 = *(const f32x4*)(sc_w + 8 * r4 + 4 * hi);
      const f32x4 vs4 = *(const f32x4*)(sc_w + TK + 8 * r4 + 4 * hi);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int r = r4 * 4 + j;
        const int key = key0 + 8 * r4 + 4 * hi + j;
        float a = s[r] * (ks4[j] * scale_log2);
        if (key >= hi_key || key < win_lo) a = -3.0e38f;
        sv[r] = a;
        vs[r] = vs4[j];
        pmax = fmaxf(pmax, a);
      }
    }
    pmax = fmaxf(pmax, __shfl_xor(pmax, 32));

    const float m_new = fmaxf(m_run, pmax);
    const float alpha =
        (m_run <= -3.0e38f) ? 0.f : __builtin_amdgcn_exp2f(m_run - m_new);
    m_run = m_new;
    float lsum = 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const float e =
          (sv[r] <= -3.0e38f) ? 0.f : __builtin_amdgcn_exp2f(sv[r] - m_new);
      lsum += e;
      sv[r] = e * vs[r];  // V's dequantisation rides on P
    }
    lsum += __shfl_xor(lsum, 32);
    l_run = l_run * alpha + lsum;
#pragma unroll
    for (int t = 0; t < DT; ++t)
#pragma unroll
      for (int r = 0; r < 16; ++r) oacc[t][r] *= alpha;

    // O^T[d][g] += V^T . P
#pragma unroll
    for (int c16 = 0; c16 < 2; ++c16) {
      const bf16x8_t pfrag = repack_chunk(&sv[c16 * 8]);
#pragma unroll
      for (int dt = 0; dt < DT; ++dt) {
        const bf16x8_t vfrag = tr_img_frag<D>(v_img, c16 * 16, dt, lane);
        oacc[dt] =
            __builtin_amdgcn_mfma_f32_32x32x16_bf16(vfrag, pfrag, oacc[dt], 0, 0, 0);
      }
    }
    wave_lds_fence();
  }

  // merge the 4 wave states in wave order; the [4][G][D] fp32 image reuses the
  // V images (4 * 8 * D * 4 bytes <= 4 * TK * D * 2 bytes)
  float* const mrg_acc = (float*)&v_lds[0][0];
  __syncthreads();
  if (l31 < G) {
#pragma unroll
    for (int dt = 0; dt < DT; ++dt)
#pragma unroll
      for (int r = 0; r < 16; ++r)
        mrg_acc[(wave * MAX_GROUP + l31) * D + dt * 32 + (r & 3) + 8 * (r >> 2) +
                4 * hi] = oacc[dt][r];
    if (hi == 0) {
      mrg_m[wave][l31] = m_run;
      mrg_l[wave][l31] = l_run;
    }
  }
  __syncthreads();
  for (int i = tid; i < G * D; i += 256) {
    const int g = i / D, d = i % D;
    float M = -3.0e38f;
#pragma unroll
    for (int w = 0; w < 4; ++w) M = fmaxf(M, mrg_m[w][g]);
    float L = 0.f, out = 0.f;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
      const float mw = mrg_m[w][g];
      const float a = (mw <= -3.0e38f) ? 0.f : __builtin_amdgcn_exp2f(mw - M);
      L += mrg_l[w][g] * a;
      out += a * mrg_acc[(w * MAX_GROUP + g) * D + d];
    }
    const int64_t pidx = p_base + (int64_t)g * S;
    part_acc[pidx * D + d] = out;
    if (d == 0) {
      part_m[pidx] = M;
      part_l[pidx] = L;
    }
  }
}

// ---------------------------------------------------------------------------
// flash_chunk_fp8: a step of T <= 32 tokens per sequence.  q [B, H, T, D]; token
// t of batch b sits at position p = kv_len[b] - T + t (kv_len is the length
// after the step's insert) and sees key j iff j <= p and, with a window W,
// p - j < W.  Rows with p < 0 give zeros.
//
// One workgroup per (batch, KV head, column tile, 512-key split).  The score
// MFMA's 32 columns are packed token-major: column c = t_local * G + g, a tile
// holds TPT = 32 / G tokens, columns >= TPT * G (and tokens >= T) are dead.  A
// lane owns column l31 and so one position: its causal bound p and its window
// bound are per lane.  The key walk is flash_decode_fp8's on tile-uniform
// bounds, the tile's highest position and its lowest window start; loads clamp
// to the tile's last key, so nothing past kv_len[b] - 1 is read.
//
// A column's state does not depend on which call computes it: the splits, the
// w, w + 4, ... tile walk, the per-key expressions and the two merges are those
// of flash_decode_fp8, and a tile that is fully masked for a column leaves its
// m, l and accumulators as they are (alpha = 1 or m = -3e38, every e = 0; the
// masked keys are real, finite cache rows, so their PV products are exact
// zeros).  Token t therefore carries the bits of a single-token call at
// kv_len - (T - 1 - t).
//
// part_* are indexed by (b, query head, token, split): [B, H, T, S] and
// [B, H, T, S, D], the rows flash_decode_fp8_merge folds.
// ---------------------------------------------------------------------------
constexpr int MRG_COLS = 16;  // columns per pass of the in-workgroup merge

template <int D>
__global__ __launch_bounds__(256, 2) void flash_chunk_fp8_kernel(
    const bf16_t* __restrict__ q, const uint8_t* __restrict__ k8,
    const uint8_t* __restrict__ v8, const float* __restrict__ k_scale,
    const float* __restrict__ v_scale, float* __restrict__ part_m,
    float* __restrict__ part_l, float* __restrict__ part_acc,
    const int* __restrict__ kv_len, int64_t q_sb, int64_t q_sh, int64_t q_st, int H,
    int KVH, int G, int T, int TPT, int CT, int S, int Skv, float scale_log2,
    int window) {
  constexpr int KC = D / 16;    // MFMA steps of the score contraction
  constexpr int DT = D / 32;    // 32-row tiles of O^T
  constexpr int HALF = D / 2;   // row bytes per lane half
  constexpr int NV = HALF / 16; // 16-byte loads per lane and row
  const int tid = threadIdx.x;
  const int wave = tid >> 6;
  const int lane = tid & 63;
  const int l31 = lane & 31, hi = lane >> 5;

  const int split = blockIdx.x % S;
  const int ct = (blockIdx.x / S) % CT;
  const int bk = blockIdx.x / (S * CT);
  const int b = bk / KVH, hk = bk % KVH;
  const int skv = min((kv_len != nullptr) ? kv_len[b] : Skv, Skv);
  // the column tile: tokens [t_lo, t_lo + nt) at positions [p_lo, p_hi]
  const int t_lo = ct * TPT;
  const int nt = min(TPT, T - t_lo);
  const int ncol = nt * G;
  const int p_lo = skv - T + t_lo, p_hi = p_lo + nt - 1;
  const int lo = split * SPLIT_KEYS;
  const int hi_key = min(lo + SPLIT_KEYS, p_hi + 1);  // one past the walk's last key
  const int win_lo = window > 0 ? max(0, p_lo + 1 - window) : 0;  // walk's first key

  // row of column c in the partials: (b, hk * G + c % G, t_lo + c / G, split)
  auto part_row = [&](int c) {
    const int tl = c / G, g = c - tl * G;
    return (((int64_t)b * H + hk * G + g) * T + t_lo + tl) * S + split;
  };

  // null for this column tile: exact no-op under the merge
  if (lo > p_hi || lo + SPLIT_KEYS <= win_lo) {
    for (int i = tid; i < ncol * D; i += 256) {
      const int d = i % D;
      const int64_t pidx = part_row(i / D);
      part_acc[pidx * D + d] = 0.f;
      if (d == 0) {
        part_m[pidx] = -3.0e38f;
        part_l[pidx] = 0.f;
      }
    }
    return;
  }

  __shared__ __attribute__((aligned(16))) bf16_t v_lds[4][TK * D];
  __shared__ __attribute__((aligned(16))) float sc_lds[4][2 * TK];
  __shared__ float mrg_m[4][TK], mrg_l[4][TK];
  bf16_t* const v_img = v_lds[wave];
  float* const sc_w = sc_lds[wave];

  // this lane's column: token tl of the tile, query head g; a dead column sits
  // at position -1, below every key
  const bool live = l31 < ncol;
  const int tl = live ? l31 / G : 0;
  const int g = live ? l31 - tl * G : 0;
  const int p = live ? p_lo + tl : -1;
  const int my_lo = window > 0 ? max(0, p + 1 - window) : 0;

  // Q as the B operand: column l31, zero for a dead column
  bf16x8_t qfrag[KC];
  {
    const bf16_t* qp = q + b * q_sb + ((int64_t)hk * G + g) * q_sh +
                       (int64_t)(t_lo + tl) * q_st + hi * HALF;
#pragma unroll
    for (int c = 0; c < KC; ++c) {
      bf16x8_t z{};
      qfrag[c] = live ? *(const bf16x8_t*)(qp + c * 8) : z;
    }
  }

  const int64_t row0 = ((int64_t)b * KVH + hk) * Skv;
  const uint8_t* kp = k8 + row0 * D + hi * HALF;
  const uint8_t* vp = v8 + row0 * D + hi * HALF;
  const float* scp = (hi ? v_scale : k_scale) + row0;

  float m_run = -3.0e38f, l_run = 0.f;
  f32x16_t oacc[DT];
#pragma unroll
  for (int t = 0; t < DT; ++t) oacc[t] = f32x16_t{};

  // as flash_decode_fp8: rows past the walk's last key repeat that key
  auto load_tile = [&](int key0, u32x4* kr, u32x4* vr, float& sc) {
    const int key = key0 + l31;
    const int64_t row = min(key, hi_key - 1);
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      kr[i] = *(const u32x4*)(kp + row * D + i * 16);
      vr[i] = *(const u32x4*)(vp + row * D + i * 16);
    }
    sc = scp[row];
    if (key >= hi_key) sc = 0.f;
  };

  // wave w walks tiles w, w + 4, ... of the split, from its first tile that
  // does not end below the lowest window start
  int t0 = wave;
  if (window > 0) {
    const int c = max(0, win_lo - lo) / TK;
    t0 = c + ((wave - c) & 3);
  }
  int key0 = lo + t0 * TK;
  u32x4 kn[NV], vn[NV];
  float scn = 0.f;
  if (key0 < hi_key) load_tile(key0, kn, vn, scn);

  for (; key0 < hi_key; key0 += 4 * TK) {
    u32x4 kc[NV], vc[NV];
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      kc[i] = kn[i];
      vc[i] = vn[i];
    }
    const float scc = scn;
    if (key0 + 4 * TK < hi_key) load_tile(key0 + 4 * TK, kn, vn, scn);

    // S[key][column] = K . Q^T
    f32x16_t s{};
#pragma unroll
    for (int c = 0; c < KC; ++c) {
      const bf16x8_t ka =
          fp8x8_to_bf16(kc[c >> 1][(c & 1) * 2], kc[c >> 1][(c & 1) * 2 + 1]);
      s = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ka, qfrag[c], s, 0, 0, 0);
    }

#pragma unroll
    for (int c = 0; c < KC; ++c)
      tr_img_write<D>(v_img, l31, hi * HALF + c * 8,
                      fp8x8_to_bf16(vc[c >> 1][(c & 1) * 2],
                                    vc[c >> 1][(c & 1) * 2 + 1]));
    sc_w[lane] = scc;
    wave_lds_fence();

    // register r of the D layout is key key0 + (r&3) + 8*(r>>2) + 4*hi; the
    // mask is this column's own: keys (p - W, p]
    float sv[16], vs[16];
    float pmax = -3.0e38f;
#pragma unroll
    for (int r4 = 0; r4 < 4; ++r4) {
      const f32x4 ks4 = *(const f32x4*)(sc_w + 8 * r4 + 4 * hi);
      const f32x4 vs4 = *(const f32x4*)(sc_w + TK + 8 * r4 + 4 * hi);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int r = r4 * 4 + j;
        const int key = key0 + 8 * r4 + 4 * hi + j;
        float a = s[r] * (ks4[j] * scale_log2);
        if (key > p || key < my_lo) a = -3.0e38f;
        sv[r] = a;
        vs[r] = vs4[j];
        pmax = fmaxf(pmax, a);
      }
    }
    pmax = fmaxf(pmax, __shfl_xor(pmax, 32));

    const float m_new = fmaxf(m_run, pmax);
    const float alpha =
        (m_run <= -3.0e38f) ? 0.f : __builtin_amdgcn_exp2f(m_run - m_new);
    m_run = m_new;
    float lsum = 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const float e =
          (sv[r] <= -3.0e38f) ? 0.f : __builtin_amdgcn_exp2f(sv[r] - m_new);
      lsum += e;
      sv[r] = e * vs[r];  // V's dequantisation rides on P
    }
    lsum += __shfl_xor(lsum, 32);
    l_run = l_run * alpha + lsum;
#pragma unroll
    for (int t = 0; t < DT; ++t)
#pragma unroll
      for (int r = 0; r < 16; ++r) oacc[t][r] *= alpha;

    // O^T[d][column] += V^T . P
#pragma unroll
    for (int c16 = 0; c16 < 2; ++c16) {
      const bf16x8_t pfrag = repack_chunk(&sv[c16 * 8]);
#pragma unroll
      for (int dt = 0; dt < DT; ++dt) {
        const bf16x8_t vfrag = tr_img_frag<D>(v_img, c16 * 16, dt, lane);
        oacc[dt] =
            __builtin_amdgcn_mfma_f32_32x32x16_bf16(vfrag, pfrag, oacc[dt], 0, 0, 0);
      }
    }
    wave_lds_fence();
  }

  // merge the 4 wave states in wave order, MRG_COLS columns per pass: the
  // [4][MRG_COLS][D] fp32 image is exactly the V images (4 * 16 * D * 4 bytes =
  // 4 * TK * D * 2 bytes), so the kernel holds no more LDS than the decode
  float* const mrg_acc = (float*)&v_lds[0][0];
  if (hi == 0) {
    mrg_m[wave][l31] = m_run;
    mrg_l[wave][l31] = l_run;
  }
  for (int c0 = 0; c0 < ncol; c0 += MRG_COLS) {  // ncol is workgroup-uniform
    __syncthreads();  // the V images, or the previous pass, have been read
    if (l31 >= c0 && l31 < c0 + MRG_COLS && live) {
#pragma unroll
      for (int dt = 0; dt < DT; ++dt)
#pragma unroll
        for (int r = 0; r < 16; ++r)
          mrg_acc[(wave * MRG_COLS + l31 - c0) * D + dt * 32 + (r & 3) +
                  8 * (r >> 2) + 4 * hi] = oacc[dt][r];
    }
    __syncthreads();
    const int nc = min(MRG_COLS, ncol - c0);
    for (int i = tid; i < nc * D; i += 256) {
      const int cl = i / D, d = i % D;
      const int c = c0 + cl;
      float M = -3.0e38f;
#pragma unroll
      for (int w = 0; w < 4; ++w) M = fmaxf(M, mrg_m[w][c]);
      float L = 0.f, out = 0.f;
#pragma unroll
      for (int w = 0; w < 4; ++w) {
        const float mw = mrg_m[w][c];
        const float a = (mw <= -3.0e38f) ? 0.f : __builtin_amdgcn_exp2f(mw - M);
        L += mrg_l[w][c] * a;
        out += a * mrg_acc[(w * MRG_COLS + cl) * D + d];
      }
      const int64_t pidx = part_row(c);
      part_acc[pidx * D + d] = out;
      if (d == 0) {
        part_m[pidx] = M;
        part_l[pidx] = L;
      }
    }
  }
}

// one wave per (batch, query head): fold the S split states in index order,
// normalize, write o [B, H, 1, D] (contiguous); per (batch, query head, token)
// row and o [B, H, T, D] behind flash_chunk_fp8
template <int D>
__global__ __launch_bounds__(64) void flash_decode_fp8_merge_kernel(
    const float* __restrict__ part_m, const float* __restrict__ part_l,
    const float* __restrict__ part_acc, uint16_t* __restrict__ o, int S) {
  constexpr int DPL = D / 64;
  const int64_t bh = blockIdx.x;
  const int lane = threadIdx.x;
  float M = -3.0e38f;
  for (int s = 0; s < S; ++s) M = fmaxf(M, part_m[bh * S + s]);
  float L = 0.f;
  float out[DPL];
#pragma unroll
  for (int t = 0; t < DPL; ++t) out[t] = 0.f;
  for (int s = 0; s < S; ++s) {
    const int64_t pidx = bh * S + s;
    const float m = part_m[pidx];
    const float a = (m <= -3.0e38f) ? 0.f : __builtin_amdgcn_exp2f(m - M);
    L += part_l[pidx] * a;
#pragma unroll
    for (int t = 0; t < DPL; ++t) out[t] += a * part_acc[pidx * D + t * 64 + lane];
  }
  const float inv = (L > 0.f) ? 1.0f / L : 0.f;
#pragma unroll
  for (int t = 0; t < DPL; ++t) o[bh * D + t * 64 + lane] = f2bf(out[t] * inv);
}

template <int D>
void launch_decode_fp8(const void* q, const void* k8, const void* v8,
                       const float* k_scale, const float* v_scale, void* o,
                       float* part_m, float* part_l, float* part_acc,
                       const int* kv_len, int64_t q_sb, int64_t q_sh, int B, int H,
                       int KVH, int S, int Skv, float scale, int window,
                       hipStream_t stream) {
  flash_decode_fp8_kernel<D><<<dim3(B * KVH * S), dim3(256), 0, stream>>>(
      (const bf16_t*)q, (const uint8_t*)k8, (const uint8_t*)v8, k_scale, v_scale,
      part_m, part_l, part_acc, kv_len, q_sb, q_sh, H, KVH, H / KVH, S, Skv,
      scale * 1.4426950408889634f, window);
  flash_decode_fp8_merge_kernel<D><<<dim3(B * H), dim3(64), 0, stream>>>(
      part_m, part_l, part_acc, (uint16_t*)o, S);
}

template <int D>
void launch_chunk_fp8(const void* q, const void* k8, const void* v8,
                      const float* k_scale, const float* v_scale, void* o,
                      float* part_m, float* part_l, float* part_acc,
                      const int* kv_len, int64_t q_sb, int64_t q_sh, int64_t q_st,
                      int B, int H, int KVH, int T, int S, int Skv, float scale,
                      int window, hipStream_t stream) {
  const int G = H / KVH;
  const int TPT = TK / G;        // tokens per column tile
  const int CT = CDIV(T, TPT);   // column tiles
  flash_chunk_fp8_kernel<D><<<dim3(B * KVH * CT * S), dim3(256), 0, stream>>>(
      (const bf16_t*)q, (const uint8_t*)k8, (const uint8_t*)v8, k_scale, v_scale,
      part_m, part_l, part_acc, kv_len, q_sb, q_sh, q_st, H, KVH, G, T, TPT, CT, S,
      Skv, scale * 1.4426950408889634f, window);
  flash_decode_fp8_merge_kernel<D><<<dim3(B * H * T), dim3(64), 0, stream>>>(
      part_m, part_l, part_acc, (uint16_t*)o, S);
}

}  // namespace

extern "C" void flash_chunk_fp8_bf16(
    const void* q, const void* k8, const void* v8, const float* k_scale,
    const float* v_scale, void* o, float* part_m, float* part_l, float* part_acc,
    const int* kv_len, int64_t q_sb, int64_t q_sh, int64_t q_st, int B, int H,
    int KVH, int T, int S, int Skv, int D, float scale, int window,
    hipStream_t stream) {
  if (D == 64)
    launch_chunk_fp8<64>(q, k8, v8, k_scale, v_scale, o, part_m, part_l, part_acc,
                         kv_len, q_sb, q_sh, q_st, B, H, KVH, T, S, Skv, scale,
                         window, stream);
  else if (D == 128)
    launch_chunk_fp8<128>(q, k8, v8, k_scale, v_scale, o, part_m, part_l, part_acc,
                          kv_len, q_sb, q_sh, q_st, B, H, KVH, T, S, Skv, scale,
                          window, stream);
}

extern "C" void rope_kv_insert_fp8(
    const void* q, const void* k, const void* v, void* qo, void* k8, void* v8,
    float* k_scale, float* v_scale, const float* cos_t, const float* sin_t,
    const long long* pos_p, int B, int T, int NH, int KVH, int HD, int64_t max_len,
    int64_t q_sb, int64_t q_st, int64_t q_sh, int64_t k_sb, int64_t k_st,
    int64_t k_sh, int64_t v_sb, int64_t v_st, int64_t v_sh, int rotate,
    int per_batch_pos, hipStream_t stream) {
  const int waves = B * T * (NH + 2 * KVH);
  const int blocks = CDIV(waves, 4);  // 4 waves (256 threads) per block
  auto launch = [&](auto kernel) {
    kernel<<<dim3(blocks), 256, 0, stream>>>(
        (const uint16_t*)q, (const uint16_t*)k, (const uint16_t*)v, (uint16_t*)qo,
        (uint8_t*)k8, (uint8_t*)v8, k_scale, v_scale, cos_t, sin_t, pos_p, B, T, NH,
        KVH, HD, max_len, q_sb, q_st, q_sh, k_sb, k_st, k_sh, v_sb, v_st, v_sh,
        per_batch_pos);
  };
  if (rotate) launch(rope_kv_insert_fp8_kernel<true>);
  else launch(rope_kv_insert_fp8_kernel<false>);
}

extern "C" void kv_quantize_rows_bf16(const void* src, void* dst, float* scale,
                                      int64_t s_sb, int64_t s_sh, int64_t s_sl,
                                      int B, int KVH, int L, int HD,
                                      int64_t max_len, hipStream_t stream) {
  const int64_t waves = (int64_t)B * KVH * L;
  if (waves == 0) return;
  kv_quantize_rows_kernel<<<dim3((uint32_t)CDIV(waves, 4)), 256, 0, stream>>>(
      (const uint16_t*)src, (uint8_t*)dst, scale, s_sb, s_sh, s_sl, B, KVH, L, HD,
      max_len);
}

extern "C" int flash_decode_fp8_num_splits(int Skv) {
  return Skv <= SPLIT_KEYS ? 1 : CDIV(Skv, SPLIT_KEYS);
}

extern "C" void flash_decode_fp8_bf16(
    const void* q, const void* k8, const void* v8, const float* k_scale,
    const float* v_scale, void* o, float* part_m, float* part_l, float* part_acc,
    const int* kv_len, int64_t q_sb, int64_t q_sh, int B, int H, int KVH, int S,
    int Skv, int D, float scale, int window, hipStream_t stream) {
  if (D == 64)
    launch_decode_fp8<64>(q, k8, v8, k_scale, v_scale, o, part_m, part_l, part_acc,
                          kv_len, q_sb, q_sh, B, H, KVH, S, Skv, scale, window,
                          stream);
  else if (D == 128)
    launch_decode_fp8<128>(q, k8, v8, k_scale, v_scale, o, part_m, part_l, part_acc,
                           kv_len, q_sb, q_sh, B, H, KVH, S, Skv, scale, window,
                           stream);
}
