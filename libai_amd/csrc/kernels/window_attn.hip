// Fused window attention for Swin (bf16, head size 32, 1 <= N <= 64 tokens per
// window, dense per-head bias plus an optional additive shift mask): forward
// and a single-kernel backward with the bias gradient.
//
//   score(w, h, i, j) = scale * q_i . k_j + bias[h][i][j] + mask[w % nW][i][j]
//   O = softmax_j(score) V
//
// The whole problem of one (window, head) fits one wavefront, so there is no
// tile loop, no online softmax and no second recompute kernel: a wave owns its
// windows from the loads to the stores, four independent waves share a
// workgroup, and each has a private 16 KB LDS region.  Waves only ever
// exchange data in the backward's final dbias fold.
//
// Machinery (the D = 32 forms of what flash_attn.hip keeps private):
//   * v_mfma_f32_32x32x16_bf16.  A-frag: lane owns row l&31 and holds
//     k = (l>>5)*8 + j; B-frag: lane owns column l&31, same k split; D-frag:
//     lane owns column l&31 and holds rows (r&3) + 8*(r>>2) + 4*(l>>5).
//   * row image: [rows][32] bf16, the four 16-byte chunks of a row XOR-ed with
//     (row>>2)&3, so the 16 lanes of one ds_read_b128 phase hit 16 bank groups.
//   * tr image: [r/4][d/16][4][16]-blocked bf16; ds_read_b64_tr_b16 hands a
//     lane column d and 8 consecutive rows (a fragment contracted over rows).
//   * D-layout fp32 -> contiguous-k bf16 fragment: pack + v_permlane32_swap.
//   * every product is "swapped" (S^T = K Q^T, O^T = V^T P^T, ...), so a lane
//     owns one QUERY column: softmax max/sum, lse and Drow are in-lane plus
//     one exchange with lane ^ 32.
//   * bias + mask of one 32-query block are staged by coalesced row loads into
//     an fp32 LDS image and read back as one ds_read_b128 per four keys; read
//     straight from HBM in the swapped layout, one load would touch 32 rows.
//
// Padding: keys >= N score the -3.0e38 sentinel; P and dS at padded keys and
// padded queries are exact zeros (bitwise AND, never a select of the
// expensive operand), and every global index is clamped into the tensor.
// Before that AND the score of a padded QUERY may be anything, a NaN
// included: its row of the bias + mask image is never staged and holds stale
// LDS.  The forward never stores those columns; the backward ANDs them away.
//
// Packed fp32 VALU forms are switched off for these kernels by a function
// attribute, as for the split-KV kernels of flash_attn.hip; a function with
// other target features is not inlined, so the kernels use builtins in place
// of the HIP header helpers (__shfl_xor, __syncthreads, min, max).
#include "common.h"
#include "launchers.h"

#include <atomic>

namespace {

typedef __bf16 bf16_t;
typedef __bf16 bf16x8_t __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x4_t __attribute__((ext_vector_type(4)));
typedef float f32x16_t __attribute__((ext_vector_type(16)));
typedef float f32x4_t __attribute__((ext_vector_type(4)));

#define WA_D 32             // head size
#define WA_WAVES 4          // independent waves per workgroup
#define WA_WAVE_LDS 16384   // bytes of LDS per wave, both kernels
#define WA_LOG2E 1.4426950408889634f
#define WA_LN2 0.6931471805599453f
#if defined(__HIP_DEVICE_COMPILE__)  // the host pass does not know the feature
#define WA_TARGET __attribute__((target("no-packed-fp32-ops")))
#else
#define WA_TARGET
#endif
#define WA_DEV __device__ __forceinline__ WA_TARGET

WA_DEV int imin(int a, int b) { return a < b ? a : b; }

// Orders the wave's LDS traffic for the compiler.  The hardware executes one
// wave's LDS instructions in order, so no instruction is needed; without the
// fences the compiler may move a lane's read over a write that only another
// lane's read depends on.
WA_DEV void wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

WA_DEV void block_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_s_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

// x of this lane and of lane ^ 32, in half order (the same pair on both)
WA_DEV void half_pair(float x, float& lo, float& up) {
  const uint32_t u = __builtin_bit_cast(uint32_t, x);
  auto r = __builtin_amdgcn_permlane32_swap(u, u, false, false);
  lo = __builtin_bit_cast(float, (uint32_t)r[0]);
  up = __builtin_bit_cast(float, (uint32_t)r[1]);
}
WA_DEV float pair_max(float x) {
  float lo, up;
  half_pair(x, lo, up);
  return __builtin_fmaxf(lo, up);
}
WA_DEV float pair_sum(float x) {
  float lo, up;
  half_pair(x, lo, up);
  return lo + up;
}

// x where m is all ones, an exact +0 (also for an inf or NaN x) where m is 0
WA_DEV float and_f32(float x, uint32_t m) {
  return __builtin_bit_cast(float, __builtin_bit_cast(uint32_t, x) & m);
}

WA_DEV uint32_t pack_bf16x2(float lo, float hi) {
  union {
    uint32_t u;
    bf16_t h[2];
  } r;
  r.h[0] = (bf16_t)lo;
  r.h[1] = (bf16_t)hi;
  return r.u;
}

// 8 consecutive D-layout regs (rows {0..3} + 4hi and {8..11} + 4hi of a 16-row
// chunk) -> the 8 contiguous rows 8hi .. 8hi+7 as bf16
WA_DEV bf16x8_t repack_chunk(const float* sv8) {
  uint32_t x0 = pack_bf16x2(sv8[0], sv8[1]);
  uint32_t z0 = pack_bf16x2(sv8[2], sv8[3]);
  uint32_t y0 = pack_bf16x2(sv8[4], sv8[5]);
  uint32_t w0 = pack_bf16x2(sv8[6], sv8[7]);
  auto rx = __builtin_amdgcn_permlane32_swap(x0, y0, false, false);
  auto rz = __builtin_amdgcn_permlane32_swap(z0, w0, false, false);
  uint32_t words[4] = {(uint32_t)rx[0], (uint32_t)rz[0], (uint32_t)rx[1],
                       (uint32_t)rz[1]};
  bf16x8_t out;
  __builtin_memcpy(&out, words, 16);
  return out;
}

// ---- LDS images -----------------------------------------------------------

// row image of [rows][32]: 16-byte chunk col8 of row `row`
WA_DEV int row_img_byte(int row, int col8) {
  return row * (WA_D * 2) + ((col8 ^ ((row >> 2) & 3)) << 4);
}
WA_DEV void row_img_write(bf16_t* lds, int row, int col8, bf16x8_t val) {
  *(bf16x8_t*)((char*)lds + row_img_byte(row, col8)) = val;
}
// A/B fragment: elements [row][c*16 + hi*8 .. +8]
WA_DEV bf16x8_t row_img_frag(const bf16_t* lds, int row, int c, int hi) {
  return *(const bf16x8_t*)((const char*)lds + row_img_byte(row, c * 2 + hi));
}

// tr image of [rows][W]: 16-byte chunk (row, 8 columns from d0)
template <int W>
WA_DEV void tr_img_write(bf16_t* lds, int row, int d0, bf16x8_t val) {
  const int idx = (((row >> 2) * (W / 16) + (d0 >> 4)) * 64) + (row & 3) * 16 + (d0 & 15);
  *(bf16x8_t*)(lds + idx) = val;
}
// transposed fragment: lane gets [rbase + hi*8 + j][dt*32 + l31], j = 0..7
template <int W>
WA_DEV bf16x8_t tr_img_frag(const bf16_t* lds, int rbase, int dt, int lane) {
  const int hi = lane >> 5;
  const int l31 = lane & 31;
  const int r0 = rbase + hi * 8;
  const int d0 = dt * 32 + (l31 & ~15);
  const bf16_t* p0 = lds + (((r0 >> 2) * (W / 16) + (d0 >> 4)) * 64) + (lane & 15) * 4;
  const bf16_t* p1 =
      lds + ((((r0 + 4) >> 2) * (W / 16) + (d0 >> 4)) * 64) + (lane & 15) * 4;
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

// bias + mask image of one 32-query block: fp32 [32][64], row r rotated by 4r
// floats (a lane's four consecutive keys stay one aligned 16-byte group, and
// the lanes of a read, one query row each, spread over the banks)
WA_DEV int bm_idx(int row, int key) { return row * 64 + ((key + 4 * row) & 63); }

// One coalesced row per step: lane = key.  Rows >= N of the block are not
// written (stale LDS: lanes of padded queries read it and their scores are
// discarded), keys >= N hold 0.
WA_DEV void stage_bm(float* img, const float* __restrict__ bias_h,
                     const float* __restrict__ mask_w, int q0, int N, int lane) {
  const int nrows = imin(32, N - q0);
  const int kc = imin(lane, N - 1);
  const uint32_t kvalid = lane < N ? 0xFFFFFFFFu : 0u;
#pragma unroll 4
  for (int r = 0; r < nrows; ++r) {
    const int e = (q0 + r) * N + kc;
    float v = bias_h[e];
    if (mask_w != nullptr) v += mask_w[e];
    img[bm_idx(r, lane)] = and_f32(v, kvalid);
  }
}

// the lane's four values of query row l31 at keys key0 .. key0+3 (key0 % 4 == 0)
WA_DEV f32x4_t bm_read(const float* img, int l31, int key0) {
  return *(const f32x4_t*)(img + bm_idx(l31, key0));
}

WA_DEV bf16x8_t load8(const bf16_t* p) { return *(const bf16x8_t*)p; }

// key (or d) row of D-layout register r in 32-row tile t
#define WA_DROW(t, r, hi) ((t)*32 + ((r)&3) + 8 * ((r) >> 2) + 4 * (hi))

// ===========================================================================
// forward: one wave per (window, head)
// ===========================================================================
// LDS of a wave: K row image [64][32] (4 KB), V tr image [64][32] (4 KB),
// bias + mask image [32][64] fp32 (8 KB).  NB = number of 32-row blocks of
// keys and of queries (1 for N <= 32, else 2).
template <int NB>
__global__ __launch_bounds__(256) WA_TARGET void window_attn_fwd_kernel(
    const WindowAttnArgs a) {
  __shared__ __align__(16) char lds_all[WA_WAVES * WA_WAVE_LDS];
  const int wave = threadIdx.x >> 6;
  const int lane = threadIdx.x & 63;
  const int l31 = lane & 31;
  const int hi = lane >> 5;
  const int N = a.N, H = a.H;

  const int64_t g = (int64_t)blockIdx.x * WA_WAVES + wave;  // (window, head)
  if (g >= (int64_t)a.B_ * H) return;  // no barrier anywhere: a wave may leave
  const int w = (int)(g / H), h = (int)(g % H);

  char* lds = lds_all + wave * WA_WAVE_LDS;
  bf16_t* k_img = (bf16_t*)lds;
  bf16_t* v_img = (bf16_t*)(lds + 4096);
  float* bm_img = (float*)(lds + 8192);

  const bf16_t* qp = (const bf16_t*)a.qkv + (int64_t)w * a.s_b + (int64_t)h * a.s_h;
  const bf16_t* kp = qp + a.s_3;
  const bf16_t* vp = qp + 2 * a.s_3;
  const float* bias_h = a.bias + (int64_t)h * N * N;
  const float* mask_w =
      a.mask != nullptr ? a.mask + (int64_t)(w % a.nW) * N * N : nullptr;

  // K row image and V tr image; rows >= N are zeros
#pragma unroll
  for (int i = 0; i < NB * 2; ++i) {
    const int flat = lane + 64 * i;
    const int row = flat >> 2, col8 = flat & 3;
    bf16x8_t kv{}, vv{};
    if (row < N) {
      kv = load8(kp + (int64_t)row * a.s_n + col8 * 8);
      vv = load8(vp + (int64_t)row * a.s_n + col8 * 8);
    }
    row_img_write(k_img, row, col8, kv);
    tr_img_write<WA_D>(v_img, row, col8 * 8, vv);
  }

  bf16_t* op = (bf16_t*)a.o;
  for (int qb = 0; qb < NB; ++qb) {
    const int q0 = qb * 32;
    const int query = q0 + l31;
    const int qc = imin(query, N - 1);
    bf16x8_t qfr[2];
#pragma unroll
    for (int c = 0; c < 2; ++c)
      qfr[c] = load8(qp + (int64_t)qc * a.s_n + c * 16 + hi * 8);

    wave_sync();
    stage_bm(bm_img, bias_h, mask_w, q0, N, lane);
    wave_sync();

    // S^T[key][query] = K x Q^T
    f32x16_t s[NB];
#pragma unroll
    for (int t = 0; t < NB; ++t) s[t] = f32x16_t{};
#pragma unroll
    for (int c = 0; c < 2; ++c)
#pragma unroll
      for (int t = 0; t < NB; ++t) {
        bf16x8_t ka = row_img_frag(k_img, t * 32 + l31, c, hi);
        s[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ka, qfr[c], s[t], 0, 0, 0);
      }

    // scores in fp32; single-pass softmax: the lane holds its query's whole row
    float sv[NB][16];
    float m = -3.0e38f;
#pragma unroll
    for (int t = 0; t < NB; ++t)
#pragma unroll
      for (int r4 = 0; r4 < 4; ++r4) {
        const int key0 = t * 32 + 8 * r4 + 4 * hi;
        const f32x4_t bm = bm_read(bm_img, l31, key0);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          float x = __builtin_fmaf(a.scale, s[t][r4 * 4 + j], bm[j]);
          if (key0 + j >= N) x = -3.0e38f;
          sv[t][r4 * 4 + j] = x;
          m = __builtin_fmaxf(m, x);
        }
      }
    m = pair_max(m);
    float l = 0.f;
#pragma unroll
    for (int t = 0; t < NB; ++t)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const uint32_t kvalid = WA_DROW(t, r, hi) < N ? 0xFFFFFFFFu : 0u;
        const float e =
            and_f32(__builtin_amdgcn_exp2f((sv[t][r] - m) * WA_LOG2E), kvalid);
        sv[t][r] = e;
        l += e;
      }
    l = pair_sum(l);

    // O^T[d][query] = V^T x P^T (P unnormalized, <= 1)
    f32x16_t o{};
#pragma unroll
    for (int t = 0; t < NB; ++t)
#pragma unroll
      for (int c16 = 0; c16 < 2; ++c16) {
        bf16x8_t pf = repack_chunk(&sv[t][c16 * 8]);
        bf16x8_t vf = tr_img_frag<WA_D>(v_img, t * 32 + c16 * 16, 0, lane);
        o = __builtin_amdgcn_mfma_f32_32x32x16_bf16(vf, pf, o, 0, 0, 0);
      }

    const float inv_l = 1.0f / l;  // key 0 is always valid: l >= 1
    float ov[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) ov[r] = o[r] * inv_l;
    // the repack exchanges with lane ^ 32: all lanes, before the guard
    bf16x8_t o0 = repack_chunk(&ov[0]), o1 = repack_chunk(&ov[8]);
    if (query < N) {
      bf16_t* orow = op + (((int64_t)w * N + query) * H + h) * WA_D + hi * 8;
      *(bf16x8_t*)orow = o0;
      *(bf16x8_t*)(orow + 16) = o1;
      if (hi == 0)
        a.lse[((int64_t)w * H + h) * N + query] =
            m + __builtin_amdgcn_logf(l) * WA_LN2;
    }
  }
}

// ===========================================================================
// backward: dQ, dK, dV and the dbias partial sums in one kernel
// ===========================================================================
// Grid (H, P): a wave stays on head h = blockIdx.x and walks the windows
// 4p + v, 4p + v + 4P, ... (p = blockIdx.y, v = its index in the workgroup).
// Per window, with P rebuilt from q, k, bias, mask and the saved lse:
//   Drow = rowsum(dO * O);  dV = P^T dO;  dP = dO V^T;  dS = P * (dP - Drow)
//   dQ = scale * dS K;  dK = scale * dS^T Q;  dbias[h] += dS
// In the swapped layout a lane's dS registers sit at the same (query, key) in
// every window, so dbias accumulates in NB * NB * 16 fp32 registers over the
// wave's whole walk.  At the end the four waves write their sums to LDS, the
// workgroup adds them in wave order and stores one [N, N] slice of the
// [P, H, N, N] partial buffer: no atomics, the same bits on every run.
//
// LDS of a wave (16 KB): K tr image [64][32] (4 KB); P and dS tr images
// [32 queries][64 keys] of the current query block (4 KB each; the bias +
// mask image occupies the same 8 KB before they are written); dO and Q tr
// images [32 queries][32] of the current query block (2 KB each).  The K and V
// row fragments (A operands of S^T and dP^T) come straight from HBM with
// clamped rows and stay in registers for both query blocks.
template <int NB>
__global__ __launch_bounds__(256) WA_TARGET void window_attn_bwd_kernel(
    const WindowAttnBwdArgs a) {
  __shared__ __align__(16) char lds_all[WA_WAVES * WA_WAVE_LDS];
  const int tid = threadIdx.x;
  const int wave = tid >> 6;
  const int lane = tid & 63;
  const int l31 = lane & 31;
  const int hi = lane >> 5;
  const int N = a.N, H = a.H;
  const int h = blockIdx.x, p = blockIdx.y, P = gridDim.y;

  char* lds = lds_all + wave * WA_WAVE_LDS;
  bf16_t* k_tr = (bf16_t*)lds;
  bf16_t* p_img = (bf16_t*)(lds + 4096);
  bf16_t* ds_img = (bf16_t*)(lds + 8192);
  float* bm_img = (float*)(lds + 4096);  // before p_img / ds_img are written
  bf16_t* do_tr = (bf16_t*)(lds + 12288);
  bf16_t* q_tr = (bf16_t*)(lds + 14336);

  const float* bias_h = a.bias + (int64_t)h * N * N;
  const int64_t row_o = (int64_t)H * WA_D;       // o / dout row stride
  const int64_t row_g = (int64_t)3 * H * WA_D;   // dqkv row stride

  float acc[NB][NB][16];
#pragma unroll
  for (int qb = 0; qb < NB; ++qb)
#pragma unroll
    for (int t = 0; t < NB; ++t)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[qb][t][r] = 0.f;

  for (int w = WA_WAVES * p + wave; w < a.B_; w += WA_WAVES * P) {
    const bf16_t* qp = (const bf16_t*)a.qkv + (int64_t)w * a.s_b + (int64_t)h * a.s_h;
    const bf16_t* kp = qp + a.s_3;
    const bf16_t* vp = qp + 2 * a.s_3;
    const bf16_t* op = (const bf16_t*)a.o + (int64_t)w * N * row_o + h * WA_D;
    const bf16_t* dop = (const bf16_t*)a.dout + (int64_t)w * N * row_o + h * WA_D;
    bf16_t* gq = (bf16_t*)a.dqkv + (int64_t)w * N * row_g + h * WA_D;
    bf16_t* gk = gq + (int64_t)H * WA_D;
    bf16_t* gv = gk + (int64_t)H * WA_D;
    const float* mask_w =
        a.mask != nullptr ? a.mask + (int64_t)(w % a.nW) * N * N : nullptr;
    const float* lse_w = a.lse + ((int64_t)w * H + h) * N;

    wave_sync();  // the previous window's image reads are done
#pragma unroll
    for (int i = 0; i < NB * 2; ++i) {
      const int flat = lane + 64 * i;
      const int row = flat >> 2, col8 = flat & 3;
      bf16x8_t kv{};
      if (row < N) kv = load8(kp + (int64_t)row * a.s_n + col8 * 8);
      tr_img_write<WA_D>(k_tr, row, col8 * 8, kv);
    }
    bf16x8_t kfr[NB][2], vfr[NB][2];
#pragma unroll
    for (int t = 0; t < NB; ++t) {
      const int kc = imin(t * 32 + l31, N - 1);
#pragma unroll
      for (int c = 0; c < 2; ++c) {
        kfr[t][c] = load8(kp + (int64_t)kc * a.s_n + c * 16 + hi * 8);
        vfr[t][c] = load8(vp + (int64_t)kc * a.s_n + c * 16 + hi * 8);
      }
    }

    f32x16_t dv[NB], dk[NB];  // dV^T, dK^T [d][key]: the lane owns a key
#pragma unroll
    for (int t = 0; t < NB; ++t) {
      dv[t] = f32x16_t{};
      dk[t] = f32x16_t{};
    }

#pragma unroll
    for (int qb = 0; qb < NB; ++qb) {
      const int q0 = qb * 32;
      const int query = q0 + l31;
      const int qc = imin(query, N - 1);
      const uint32_t qvalid = query < N ? 0xFFFFFFFFu : 0u;
      bf16x8_t qfr[2], dofr[2];
      float drow = 0.f;
#pragma unroll
      for (int c = 0; c < 2; ++c) {
        qfr[c] = load8(qp + (int64_t)qc * a.s_n + c * 16 + hi * 8);
        dofr[c] = load8(dop + (int64_t)qc * row_o + c * 16 + hi * 8);
        const bf16x8_t ofr = load8(op + (int64_t)qc * row_o + c * 16 + hi * 8);
#pragma unroll
        for (int j = 0; j < 8; ++j)
          drow = __builtin_fmaf((float)dofr[c][j], (float)ofr[j], drow);
      }
      drow = pair_sum(drow);
      const float lse_q = lse_w[qc];

      wave_sync();  // dV / dK of the previous block have read p_img / ds_img
      stage_bm(bm_img, bias_h, mask_w, q0, N, lane);
      wave_sync();

      // S^T = K x Q^T and dP^T = V x dO^T, [key][query]
      f32x16_t s[NB], dp[NB];
#pragma unroll
      for (int t = 0; t < NB; ++t) {
        s[t] = f32x16_t{};
        dp[t] = f32x16_t{};
      }
#pragma unroll
      for (int c = 0; c < 2; ++c)
#pragma unroll
        for (int t = 0; t < NB; ++t) {
          s[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kfr[t][c], qfr[c], s[t], 0, 0, 0);
          dp[t] =
              __builtin_amdgcn_mfma_f32_32x32x16_bf16(vfr[t][c], dofr[c], dp[t], 0, 0, 0);
        }

      float pv[NB][16], dsv[NB][16];
#pragma unroll
      for (int t = 0; t < NB; ++t)
#pragma unroll
        for (int r4 = 0; r4 < 4; ++r4) {
          const int key0 = t * 32 + 8 * r4 + 4 * hi;
          const f32x4_t bm = bm_read(bm_img, l31, key0);
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const int r = r4 * 4 + j;
            const uint32_t valid = key0 + j < N ? qvalid : 0u;
            const float x = __builtin_fmaf(a.scale, s[t][r], bm[j]);
            const float pe =
                and_f32(__builtin_amdgcn_exp2f((x - lse_q) * WA_LOG2E), valid);
            const float dse = and_f32(pe * (dp[t][r] - drow), valid);
            pv[t][r] = pe;
            dsv[t][r] = dse;
            acc[qb][t][r] += dse;
          }
        }
      wave_sync();  // the bias + mask image is read: its space becomes P / dS

      // P and dS as tr images (to be contracted over queries), dO and Q too;
      // dQ^T[d][query] = K^T x dS^T straight from the repacked fragments
      f32x16_t dq{};
#pragma unroll
      for (int t = 0; t < NB; ++t)
#pragma unroll
        for (int c16 = 0; c16 < 2; ++c16) {
          const bf16x8_t pf = repack_chunk(&pv[t][c16 * 8]);
          const bf16x8_t df = repack_chunk(&dsv[t][c16 * 8]);
          const int key0 = t * 32 + c16 * 16 + hi * 8;
          tr_img_write<64>(p_img, l31, key0, pf);
          tr_img_write<64>(ds_img, l31, key0, df);
          const bf16x8_t kf = tr_img_frag<WA_D>(k_tr, t * 32 + c16 * 16, 0, lane);
          dq = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kf, df, dq, 0, 0, 0);
        }
#pragma unroll
      for (int c = 0; c < 2; ++c) {
        tr_img_write<WA_D>(do_tr, l31, c * 16 + hi * 8, dofr[c]);
        tr_img_write<WA_D>(q_tr, l31, c * 16 + hi * 8, qfr[c]);
      }
      wave_sync();

      // dV^T[d][key] += dO^T x P, dK^T[d][key] += Q^T x dS over this block's
      // queries (padded queries: P and dS are zeros against clamped finite rows)
#pragma unroll
      for (int kq = 0; kq < 2; ++kq) {
        const bf16x8_t da = tr_img_frag<WA_D>(do_tr, kq * 16, 0, lane);
        const bf16x8_t qa = tr_img_frag<WA_D>(q_tr, kq * 16, 0, lane);
#pragma unroll
        for (int t = 0; t < NB; ++t) {
          const bf16x8_t pb = tr_img_frag<64>(p_img, kq * 16, t, lane);
          dv[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(da, pb, dv[t], 0, 0, 0);
          const bf16x8_t sb = tr_img_frag<64>(ds_img, kq * 16, t, lane);
          dk[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(qa, sb, dk[t], 0, 0, 0);
        }
      }

      float qv[16];
#pragma unroll
      for (int r = 0; r < 16; ++r) qv[r] = dq[r] * a.scale;
      const bf16x8_t g0 = repack_chunk(&qv[0]), g1 = repack_chunk(&qv[8]);
      if (query < N) {
        bf16_t* grow = gq + (int64_t)query * row_g + hi * 8;
        *(bf16x8_t*)grow = g0;
        *(bf16x8_t*)(grow + 16) = g1;
      }
    }

#pragma unroll
    for (int t = 0; t < NB; ++t) {
      float kvv[16], vvv[16];
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        kvv[r] = dk[t][r] * a.scale;
        vvv[r] = dv[t][r];
      }
      const bf16x8_t k0 = repack_chunk(&kvv[0]), k1 = repack_chunk(&kvv[8]);
      const bf16x8_t v0 = repack_chunk(&vvv[0]), v1 = repack_chunk(&vvv[8]);
      const int key = t * 32 + l31;
      if (key < N) {
        bf16_t* krow = gk + (int64_t)key * row_g + hi * 8;
        bf16_t* vrow = gv + (int64_t)key * row_g + hi * 8;
        *(bf16x8_t*)krow = k0;
        *(bf16x8_t*)(krow + 16) = k1;
        *(bf16x8_t*)vrow = v0;
        *(bf16x8_t*)(vrow + 16) = v1;
      }
    }
  }

  // dbias: each wave's sums as an fp32 [64][64] image in its own region (rows
  // rotated as in bm_idx): the wave's own earlier traffic there is ordered
  // in-wave, so the only workgroup barrier is the one before the other waves
  // read it.  Then the workgroup adds the four images in wave order.
  wave_sync();
  float* img = (float*)lds;
#pragma unroll
  for (int qb = 0; qb < NB; ++qb)
#pragma unroll
    for (int t = 0; t < NB; ++t)
#pragma unroll
      for (int r4 = 0; r4 < 4; ++r4) {
        f32x4_t v4;
#pragma unroll
        for (int j = 0; j < 4; ++j) v4[j] = acc[qb][t][r4 * 4 + j];
        *(f32x4_t*)(img + bm_idx(qb * 32 + l31, t * 32 + 8 * r4 + 4 * hi)) = v4;
      }
  block_sync();
  const float* i0 = (const float*)lds_all;
  float* out = a.dbias_partial + ((int64_t)p * H + h) * N * N;
  for (int e = tid; e < N * N; e += 256) {
    const int query = e / N, key = e - query * N;
    const int idx = bm_idx(query, key);
    out[e] = ((i0[idx] + i0[idx + WA_WAVE_LDS / 4]) + i0[idx + 2 * (WA_WAVE_LDS / 4)]) +
             i0[idx + 3 * (WA_WAVE_LDS / 4)];
  }
}

}  // namespace

// ===========================================================================
// launchers
// ===========================================================================
extern "C" void window_attn_fwd_bf16(const WindowAttnArgs& a, hipStream_t stream) {
  const int64_t pairs = (int64_t)a.B_ * a.H;
  const dim3 grid((unsigned)CDIV(pairs, WA_WAVES)), block(64 * WA_WAVES);
  if (a.N <= 32)
    hipLaunchKernelGGL(window_attn_fwd_kernel<1>, grid, block, 0, stream, a);
  else
    hipLaunchKernelGGL(window_attn_fwd_kernel<2>, grid, block, 0, stream, a);
}

// Slices of the dbias partial buffer = workgroups per head: enough to give
// every wave a window, and no more than the chip holds at once (more would
// only add partial slices to write and fold).  The capacity is that of the
// current device and of the instantiation N selects, asked once for each pair
// (devices past the table ask every time).  Any value gives the same dbias
// up to the order of the fold; the choice only costs or saves time.
static int window_attn_bwd_held(int N) {
  constexpr int MAX_DEV = 32;
  static std::atomic<int> cache[MAX_DEV][2];  // 0 = not asked yet
  const int nb = N <= 32 ? 0 : 1;
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return 256;
  const bool cached = dev >= 0 && dev < MAX_DEV;
  if (cached) {
    const int held = cache[dev][nb].load(std::memory_order_relaxed);
    if (held > 0) return held;
  }
  int cus = 0, per_cu = 0;
  const hipError_t occ =
      nb == 0 ? hipOccupancyMaxActiveBlocksPerMultiprocessor(
                    &per_cu, window_attn_bwd_kernel<1>, 64 * WA_WAVES, 0)
              : hipOccupancyMaxActiveBlocksPerMultiprocessor(
                    &per_cu, window_attn_bwd_kernel<2>, 64 * WA_WAVES, 0);
  if (occ != hipSuccess ||
      hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) !=
          hipSuccess)
    return 256;
  const int held = (cus > 0 ? cus : 256) * (per_cu > 0 ? per_cu : 1);
  if (cached) cache[dev][nb].store(held, std::memory_order_relaxed);
  return held;
}

extern "C" int window_attn_bwd_slices(int B_, int H, int N) {
  const int held = window_attn_bwd_held(N);
  const int need = CDIV(B_, WA_WAVES);
  const int fit = held / H > 0 ? held / H : 1;
  return need < fit ? need : fit;
}

extern "C" void window_attn_bwd_bf16(const WindowAttnBwdArgs& a, hipStream_t stream) {
  const dim3 grid((unsigned)a.H, (unsigned)a.P), block(64 * WA_WAVES);
  if (a.N <= 32)
    hipLaunchKernelGGL(window_attn_bwd_kernel<1>, grid, block, 0, stream, a);
  else
    hipLaunchKernelGGL(window_attn_bwd_kernel<2>, grid, block, 0, stream, a);
}
