// Fused flash-style scaled-dot-product attention for gfx950 (bf16, MFMA):
// forward + full backward.
//
// Replaces the reference's unfused QK^T -> fused_scale_tril_softmax -> PV
// chain (reference libai/layers/attention.py:211-253) with
// online-softmax kernels: the S x S score matrix never touches HBM in either
// direction.
//
// Shared machinery (fragment layouts verified empirically by
// csrc/tools/frag_probe.cpp on MI355X):
//   * v_mfma_f32_32x32x16_bf16 everywhere.  A-frag: lane i=l&31, k=(l>>5)*8+j.
//     B-frag: lane j=l&31, same k split.  D-frag: lane col j=l&31,
//     row=(r&3)+8*(r>>2)+4*(l>>5).
//   * row images: [ROWS][D] bf16 in LDS, 16B chunks XOR-swizzled by
//     (row&15)<<4 -> conflict-free ds_read_b128 row fragments (guide T2/G4).
//   * tr images: [r/4][d/16][4][16]-blocked bf16 in LDS; ds_read_b64_tr_b16
//     delivers transposed fragments (lane gets column d, 4 rows per read).
//   * D-layout f32 regs -> contiguous-k bf16 fragments via pack +
//     permlane32_swap (guide T12).
//   * attention dropout = per-element splitmix hash on (bh, q, kv): fwd and
//     both bwd kernels regenerate identical masks in their own lane layouts.
//
// Forward saves O and per-row logsumexp.  Backward (flash-attention-2 style):
//   Drow = rowsum(dO*O);  P = exp(scale*S - lse)
//   dV = Pd^T dO;  dPd = dO V^T;  dS = scale * P (dPd*mask - Drow)
//   dK = dS^T Q;   dQ = dS K
// bwd_kv computes dK,dV (grid over kv tiles); bwd_q computes dQ (grid over
// q tiles); both recompute S on the fly.
//
// Tile classes.  All three kernels sort each 32-row sub-tile, once and with a
// wave-uniform scalar condition (the wave's base row goes through
// readfirstlane), into
//   interior: every (q, kv) pair visible -- all q rows < Sq, all kv rows <
//             sk_eff, under `causal` lowest q >= highest kv, under WINDOW the
//             farthest pair inside the band, under DOCS all keys inside the
//             document of every query;
//   edge:     everything else (diagonal, ragged, padded, band border).
// One generic lambda per kernel, instantiated on `MASKED`, gives both bodies.
// The interior body has no validity compares, selects or sentinel guards; the
// edge body keeps sentinel scores and exact zeros for masked P and dS, by
// selects / bitwise AND masks, never by per-element exec branches.  Visible
// entries are computed expression for expression alike in both, so the class
// of a tile never changes a result bit.  Accumulators and MFMAs stay outside
// the class branch: only the element values merge after it (accumulators
// merged through the branch cost 400-600 B/lane of scratch).
#include "common.h"
#include "launchers.h"

#include <type_traits>

namespace {

typedef __bf16 bf16_t;
typedef __bf16 bf16x8_t __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x4_t __attribute__((ext_vector_type(4)));
typedef float f32x16_t __attribute__((ext_vector_type(16)));

#define QB 32    // rows per wave
#define NW 4     // waves per workgroup
#define QBLK (QB * NW)
#define KVB 64   // kv rows per LDS tile (forward)

// A/B experiment knob (guide T5: s_setprio around MFMA clusters; measured
// slower on these lockstep 4-wave blocks, profiles/pmc_flash_attention.md).
#ifdef FLASH_SETPRIO
#define PRIO_HI() __builtin_amdgcn_s_setprio(1)
#define PRIO_LO() __builtin_amdgcn_s_setprio(0)
#else
#define PRIO_HI()
#define PRIO_LO()
#endif

// native bf16 converts (v_cvt_pk_bf16_f32-class) instead of the bit-manip
// RNE helper: the repack runs per score element and the manual rounding was
// ~6 VALU per value.
__device__ __forceinline__ uint32_t pack_bf16x2(float lo, float hi) {
  union {
    uint32_t u;
    bf16_t h[2];
  } r;
  r.h[0] = (bf16_t)lo;
  r.h[1] = (bf16_t)hi;
  return r.u;
}

// Edge-tile masking: x where the mask is all ones, an exact +0 where it is 0.
// A bitwise AND instead of `valid ? x : 0` keeps the backend from turning the
// select of an expensive operand (exp, LDS read) back into a per-element
// divergent branch, and also discards an inf/NaN of a masked entry.
__device__ __forceinline__ float and_f32(float x, uint32_t m) {
  return __uint_as_float(__float_as_uint(x) & m);
}

// Contraction is pinned by hand where the backward kernels form dS, so that
// every instantiation and both tile-class bodies round alike, whatever the
// compiler would pick per body: bwd_kv rounds the product dPd * keep before
// subtracting Drow, bwd_q fuses it (explicit fmaf at its call site) -- each as
// its single body always compiled.
__device__ __forceinline__ float mul_then_sub(float a, float b, float c) {
#pragma clang fp contract(off)
  return a * b - c;
}

// D-layout regs (8 consecutive: rows {0..3}+4hi and {8..11}+4hi of a 16-row
// chunk) -> one contiguous-k bf16x8 fragment.
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

// ---- LDS images -----------------------------------------------------------

// row image write: 16B chunk of row `row` at col chunk col8*8, swizzled
template <int D>
__device__ __forceinline__ void row_img_write(bf16_t* lds, int row, int col8,
                                              bf16x8_t val) {
  int byte = (row * D + col8 * 8) * 2;
  byte ^= (row & 15) << 4;
  *(bf16x8_t*)((char*)lds + byte) = val;
}

// row fragment: element [row][c*16 + hi*8 .. +8]
template <int D>
__device__ __forceinline__ bf16x8_t row_img_frag(const bf16_t* lds, int row, int c,
                                                 int hi) {
  int byte = (row * D + c * 16 + hi * 8) * 2;
  byte ^= (row & 15) << 4;
  return *(const bf16x8_t*)((const char*)lds + byte);
}

// tr image write: 16B chunk (row, 8 cols at d0)
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

// cooperative staging of a [ROWS][D] global tile into row and/or tr images
template <int ROWS, int D, bool ROW_IMG, bool TR_IMG>
__device__ __forceinline__ void stage_tile(bf16_t* row_lds, bf16_t* tr_lds,
                                           const bf16_t* gp, int row0, int bound,
                                           int64_t stride, int tid) {
  constexpr int CHUNKS_TOTAL = ROWS * D / 8;
  constexpr int ITER = CDIV(CHUNKS_TOTAL, 256);
#pragma unroll
  for (int cc = 0; cc < ITER; ++cc) {
    const int flat = tid + cc * 256;
    if (flat >= CHUNKS_TOTAL) break;
    const int row = flat / (D / 8);
    const int col8 = flat % (D / 8);
    const int gr = row0 + row;
    bf16x8_t val =
        (gr < bound) ? *(const bf16x8_t*)(gp + (int64_t)gr * stride + col8 * 8)
                     : bf16x8_t{};
    if (ROW_IMG) row_img_write<D>(row_lds, row, col8, val);
    if (TR_IMG) tr_img_write<D>(tr_lds, row, col8 * 8, val);
  }
}

// Attention dropout: ONE 32-bit hash keyed on (bh, q, kv>>2) yields four
// byte-granular keep decisions (kv&3 selects the byte; p quantized to 1/256,
// well below dropout's statistical resolution).  The forward and dQ backward
// iterate kv in aligned 4-runs at fixed q, so they amortize the hash 4x; the
// dK/dV backward (q-major layout) pays one hash per element.
// 32-bit keying: (q*Sk4 + kv4) is collision-free below 2^32 (seq up to ~128k)
// and avoids gfx950's emulated 64-bit multiplies in the per-element bwd path;
// the head index feeds the mixer's second word.
__device__ __forceinline__ uint32_t drop_hash4(uint64_t seed, uint64_t bh,
                                               int64_t Sq, int64_t Sk4, int q,
                                               int kv4) {
  (void)Sq;
  return rnd_hash2(seed, (uint32_t)q * (uint32_t)Sk4 + (uint32_t)kv4,
                   (uint32_t)bh);
}

__device__ __forceinline__ float drop_keep_byte(uint32_t h4, int kv_lo,
                                                uint32_t thr8, float ks) {
  return (((h4 >> (kv_lo * 8)) & 0xFFu) >= thr8) ? ks : 0.f;
}

__device__ __forceinline__ float drop_keep(uint64_t seed, uint64_t bh, int64_t Sq,
                                           int64_t Sk, int q, int kv, uint32_t thr8,
                                           float ks) {
  uint32_t h = drop_hash4(seed, bh, Sq, Sk >> 2, q, kv >> 2);
  return drop_keep_byte(h, kv & 3, thr8, ks);
}

// Which tile a workgroup works on.  Workgroups are dealt round-robin over the
// chip's 8 XCDs by their linear id x + gridDim.x * y, so with the plain map
// tile = blockIdx.x and 8 tiles per (batch, head) (S = 1024) every XCD gets
// ONE tile index of every head.  Under `causal` a tile's work grows linearly
// with its index (forward, bwd_q) or falls with it (bwd_kv), so one XCD then
// gets all the heaviest tiles, 16/9 of the mean, and the kernel lasts as long
// as that XCD.  Rotating the tile index by the head index deals every XCD
// every tile index in turn.  Only the assignment of tiles to workgroups
// changes: every tile is computed as before, bit for bit.
__device__ __forceinline__ int block_tile() {
  return (int)((blockIdx.x + blockIdx.y) % gridDim.x);
}

// ===========================================================================
// forward
// ===========================================================================
// The kernels are templated on one FlashVariant V (common.h; the variants do
// not combine) and derive the four switches below from it.
// ALIBI: compile-time variant that adds slope[h] * (kv - q) to every
// pre-softmax score (fp32, one slope per QUERY head).  The (kv - q) form is
// row-shift-equivalent to BLOOM's slope * kv under softmax, is bounded by the
// sequence length and is <= 0 under the causal mask.  The ALIBI=false
// instantiations never touch the pointer.
// WINDOW: compile-time variant for causal sliding-window attention: query i
// sees key j iff j <= i and i - j < window (window keys, the query's own
// included).  Besides the in-register predicate, the kv loops skip every tile
// that lies entirely below the band, so a q block reads about window + QBLK
// keys.  The WINDOW=false instantiations never read `window`.
// RELB: compile-time variant for a learned Toeplitz bias (T5 relative
// positions): rel_bias is fp32 [H, Sq + Sk - 1], one row per QUERY head, and
// the score of (q, kv) gets rel_bias[h][kv - q + Sq - 1] added in fp32 before
// the masks.  Each kernel stages the diagonals its current tile can touch
// into a small LDS table (global index clamped while staging, so the lookups
// themselves are in range for every lane, padded rows included).  bwd_q also
// reduces the bias gradient (see there).  The RELB=false instantiations never
// touch the pointers.
// DOCS: compile-time variant for packed samples (Megatron's
// reset_attention_mask, flash-attn's varlen): causal attention with Sq == Sk
// that stays inside the query's own document.  doc_start / doc_end are int32
// [B, S]: the first token of, and one past the last token of, the document
// that holds token i.  Query i sees key j iff doc_start[i] <= j <= i, which
// for contiguous documents equals j <= i < doc_end[j].  A lane of the forward
// and of bwd_q owns one query and carries the lower bound, a lane of bwd_kv
// owns one key and carries the upper bound.  Both tables are monotone along
// the sequence, so the tile skips and the tile class of WINDOW carry over
// with other scalars.  Every value read is clamped (lower bound into [0, q],
// upper bound into [kv + 1, Sq]): a malformed table gives wrong numbers, never
// an out-of-range loop or a barrier that part of a workgroup skips.  The
// DOCS=false instantiations never touch the pointers.
__device__ __forceinline__ int doc_lo_load(const int* __restrict__ row, int i,
                                           int S) {
  return min(max(row[min(i, S - 1)], 0), i);
}

__device__ __forceinline__ int doc_hi_load(const int* __restrict__ row, int i,
                                           int S) {
  return min(max(row[min(i, S - 1)], i + 1), S);
}

#define RELB_LOG2E 1.4426950408889634f

// global diagonal index -> staged value; out-of-table diagonals (only padded
// rows / keys reach them) read a clamped neighbour that is never used
__device__ __forceinline__ float relb_load(const float* __restrict__ row, int t,
                                           int n_diag) {
  return row[min(max(t, 0), n_diag - 1)];
}

// bwd_q keeps the gradient sums of the diagonals it is working on in an LDS
// ring: block diagonal a (see the kernel) lives in slot a & (RELB_RING - 1).
// A kv tile touches fewer than RELB_RING consecutive diagonals, and each one
// is flushed before the ring wraps onto its slot.
#define RELB_RING 256

// thread `tid` adds the sum of block diagonal a0 + tid (global diagonal
// a0 + tid + t_off) to the global gradient and clears the slot.  Diagonals
// outside the table, and diagonals no visible pair touched, hold an exact
// zero and issue nothing.
__device__ __forceinline__ void relb_flush(float* ring, float* __restrict__ grow,
                                           int tid, int count, int a0, int t_off,
                                           int n_diag) {
  if (tid < count) {
    const int a = a0 + tid;
    const float g = ring[a & (RELB_RING - 1)];
    ring[a & (RELB_RING - 1)] = 0.f;
    const int t = a + t_off;
    if (g != 0.f && t >= 0 && t < n_diag) atomicAdd(grow + t, g);
  }
}

// OFFS: compile-time switch for a query chunk behind cached keys (inference,
// forward only): query row i of the call sits at key position q_off + i, so
// the causal mask, the window band and the ALiBi distance are taken at
// q_off + i while loads, stores and lse keep the row index i.  q_off = Sk - Sq
// is the bottom-right alignment a cat([past, new]) cache needs.  Instantiated
// for the plain, ALiBi and window variants; every use of q_off sits under
// `if constexpr (OFFS)` (at_pos below), so the OFFS=false instantiations keep
// their instruction streams and keep the top-left alignment for Sq != Sk.
template <int D, FlashVariant V, bool OFFS = false>
__global__ __launch_bounds__(256, D == 64 ? 3 : 2) void flash_fwd_kernel(
    const bf16_t* __restrict__ q, const bf16_t* __restrict__ k,
    const bf16_t* __restrict__ v, bf16_t* __restrict__ o, float* __restrict__ lse,
    const int* __restrict__ kv_len, int64_t q_sb, int64_t q_ss, int64_t q_sh,
    int64_t k_sb, int64_t k_ss, int64_t k_sh, int64_t v_sb, int64_t v_ss,
    int64_t v_sh, int64_t o_sb, int64_t o_ss, int64_t o_sh, int H, int Sq, int Sk,
    float scale, float p_drop, uint64_t seed, int causal, int kv_group,
    const float* __restrict__ alibi_slopes, int window,
    const float* __restrict__ rel_bias, const int* __restrict__ doc_start,
    int q_off) {
  constexpr bool ALIBI = V == FlashVariant::kAlibi,
                 WINDOW = V == FlashVariant::kWindow,
                 RELB = V == FlashVariant::kRelBias, DOCS = V == FlashVariant::kDocs;
  static_assert(!OFFS || !(RELB || DOCS), "no query offset for rel_bias / documents");
  constexpr int DT = D / 32;
  constexpr int KC = D / 16;
  // key position of query row `row` (q_off is a kernel argument: adding it
  // keeps a wave-uniform row wave-uniform)
  auto at_pos = [&](int row) {
    if constexpr (OFFS) return row + q_off;
    else return row;
  };

  // 2 x KVB rows staged per barrier round: halves barrier count per unit of
  // compute (PMC: 43% of forward wave cycles were barrier/wait-parked)
  __shared__ __align__(16) bf16_t k_lds[2 * KVB * D];
  __shared__ __align__(16) bf16_t v_lds[2 * KVB * D];
  // RELB: the 2*KVB + QBLK - 1 diagonals of one round, times log2e; entry
  // (kv - kvR) + (QBLK - 1) - (q - q_block)
  constexpr int FWD_DIAGS = 2 * KVB + QBLK - 1;
  __shared__ float rb_lds[RELB ? FWD_DIAGS : 1];

  const int tid = threadIdx.x;
  const int wave = tid >> 6;
  const int lane = tid & 63;
  const int l31 = lane & 31;
  const int hi = lane >> 5;

  const int bh = blockIdx.y;
  const int b = bh / H, h = bh % H;
  const int q_block = block_tile() * QBLK;
  // wave-uniform by construction; readfirstlane tells the compiler, so the
  // sub-tile skips and the tile-class test become scalar branches
  const int q_base = __builtin_amdgcn_readfirstlane(q_block + wave * QB);

  const int hk = h / kv_group;  // GQA: query head -> its kv head
  const bf16_t* qp = q + b * q_sb + h * q_sh;
  const bf16_t* kp = k + b * k_sb + hk * k_sh;
  const bf16_t* vp = v + b * v_sb + hk * v_sh;

  // Q fragments pre-scaled by scale*log2e: scores come out of the MFMA
  // already in the exp2 domain, saving a mul per score element and the
  // exp->exp2 conversion mul (softmax runs on v_exp_f32 directly).
  const float qscale = scale * 1.4426950408889634f;
  bf16x8_t qfrag[KC];
  {
    const int qrow = min(q_base + l31, Sq - 1);
#pragma unroll
    for (int c = 0; c < KC; ++c) {
      bf16x8_t raw = *(const bf16x8_t*)(qp + (int64_t)qrow * q_ss + c * 16 + hi * 8);
#pragma unroll
      for (int j = 0; j < 8; ++j) raw[j] = (bf16_t)((float)raw[j] * qscale);
      qfrag[c] = raw;
    }
  }

  f32x16_t oacc[DT];
#pragma unroll
  for (int t = 0; t < DT; ++t) oacc[t] = f32x16_t{};
  float m_run = -3.0e38f, l_run = 0.f;

  // right-padding support: keys at/after kv_len[b] are masked out (BERT-style
  // per-sequence valid length; replaces the reference's additive -10000 pad
  // mask, attention.py:221-226)
  const int sk_eff = (kv_len != nullptr) ? kv_len[b] : Sk;
  // positions of the block's first row, the wave's first row and the lane's
  // row: what the masks compare keys with (the rows themselves without OFFS)
  const int p_block = at_pos(q_block), p_base = at_pos(q_base);
  const int kv_end = causal ? min(sk_eff, p_block + QBLK) : sk_eff;
  const int n_rounds = CDIV(kv_end, 2 * KVB);
  const float ks = (p_drop > 0.f) ? 1.0f / (1.0f - p_drop) : 1.0f;
  const int qg = q_base + l31;
  const int pg = at_pos(qg);
  // scores live in the exp2 domain, so the slope is pre-multiplied by log2e
  float slope2 = 0.f;
  if constexpr (ALIBI) slope2 = alibi_slopes[h] * 1.4426950408889634f;

  // sliding window: the first staging round is the one holding the lowest
  // key any query of this block can see (uniform across the workgroup)
  int round0 = 0;
  if constexpr (WINDOW) round0 = max(0, p_block - window + 1) / (2 * KVB);
  // packed documents: lane's lower bound; the block's lowest bound (its first
  // query's: doc_start is non-decreasing) picks the first staging round, the
  // wave's first and last queries give the sub-tile skip and the tile class
  int doc_lo = 0, doc_lo_w = 0, doc_lo_top = 0;
  if constexpr (DOCS) {
    const int* dsp = doc_start + (int64_t)b * Sq;
    doc_lo = doc_lo_load(dsp, qg, Sq);
    round0 = __builtin_amdgcn_readfirstlane(doc_lo_load(dsp, q_block, Sq)) /
             (2 * KVB);
    doc_lo_w = __builtin_amdgcn_readfirstlane(doc_lo_load(dsp, q_base, Sq));
    doc_lo_top =
        __builtin_amdgcn_readfirstlane(doc_lo_load(dsp, q_base + QB - 1, Sq));
  }
  const int n_diag = Sq + Sk - 1;
  const float* rbp = nullptr;
  if constexpr (RELB) rbp = rel_bias + (int64_t)h * n_diag;
  // lane's table entry for the first key of a round
  const int rb_lane = (QBLK - 1) - (qg - q_block);

  for (int round = round0; round < n_rounds; ++round) {
    const int kvR = round * 2 * KVB;
    __syncthreads();
    stage_tile<2 * KVB, D, true, false>(k_lds, nullptr, kp, kvR, Sk, k_ss, tid);
    stage_tile<2 * KVB, D, false, true>(nullptr, v_lds, vp, kvR, Sk, v_ss, tid);
    if constexpr (RELB) {
      if (tid < FWD_DIAGS)
        rb_lds[tid] =
            relb_load(rbp, kvR - q_block - (QBLK - 1) + tid + (Sq - 1), n_diag) *
            RELB_LOG2E;
    }
    __syncthreads();

    for (int sub = 0; sub < 2; ++sub) {
    const int kv0 = kvR + sub * KVB;
    const int ro = sub * KVB;  // row offset inside the staged images
    if (kv0 >= kv_end || (causal && kv0 > p_base + QB - 1)) continue;
    if constexpr (WINDOW) {  // sub-tile entirely below this wave's band
      if (kv0 + KVB - 1 < p_base - window + 1) continue;
    }
    if constexpr (DOCS) {  // sub-tile entirely before this wave's documents
      if (kv0 + KVB - 1 < doc_lo_w) continue;
    }

    // S = K x Q^T : two 32x32 tiles
    f32x16_t s0{}, s1{};
    PRIO_HI();
#pragma unroll
    for (int c = 0; c < KC; ++c) {
      bf16x8_t ka = row_img_frag<D>(k_lds, ro + l31, c, hi);
      s0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ka, qfrag[c], s0, 0, 0, 0);
      bf16x8_t kb = row_img_frag<D>(k_lds, ro + l31 + 32, c, hi);
      s1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kb, qfrag[c], s1, 0, 0, 0);
    }
    PRIO_LO();

    // scores are already in the exp2 domain (Q pre-scale); m/l run in it too
    float sv[2][16];
    // Tile class (wave-uniform, scalar branch): an interior sub-tile has every
    // (q, kv) pair visible -- all keys < sk_eff, all rows < Sq, under causal
    // its lowest q >= its highest kv, under WINDOW its farthest pair inside
    // the band -- and runs the body without compares, selects or sentinels.
    bool interior = kv0 + KVB <= sk_eff && q_base + QB <= Sq &&
                    (!causal || p_base >= kv0 + KVB - 1);
    if constexpr (WINDOW) interior = interior && (p_base + QB - 1 - kv0 < window);
    if constexpr (DOCS) interior = interior && (kv0 >= doc_lo_top);
    auto softmax_tile = [&](auto masked_c) {
      constexpr bool MASKED = decltype(masked_c)::value;
      float pmax = -3.0e38f;
      // kv - q of this lane's first score; the per-register offsets below are
      // compile-time constants (exact in fp32)
      float rel0 = 0.f;
      if constexpr (ALIBI) rel0 = (float)(kv0 + 4 * hi - pg);
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        int kva = kv0 + (r & 3) + 8 * (r >> 2) + 4 * hi;
        int kvb = kva + 32;
        float a = s0[r], bb = s1[r];
        if constexpr (ALIBI) {  // before the masks: masked entries keep the sentinel
          const float off = (float)((r & 3) + 8 * (r >> 2));
          a = fmaf(slope2, rel0 + off, a);
          bb = fmaf(slope2, rel0 + (off + 32.f), bb);
        }
        if constexpr (RELB) {  // before the masks, as ALiBi
          const int e = rb_lane + ro + (r & 3) + 8 * (r >> 2) + 4 * hi;
          a += rb_lds[e];
          bb += rb_lds[e + 32];
        }
        if constexpr (MASKED) {
          if (kva >= sk_eff || (causal && kva > pg)) a = -3.0e38f;
          if (kvb >= sk_eff || (causal && kvb > pg)) bb = -3.0e38f;
          if constexpr (WINDOW) {
            if (pg - kva >= window) a = -3.0e38f;
            if (pg - kvb >= window) bb = -3.0e38f;
          }
          if constexpr (DOCS) {
            if (kva < doc_lo) a = -3.0e38f;
            if (kvb < doc_lo) bb = -3.0e38f;
          }
        }
        sv[0][r] = a;
        sv[1][r] = bb;
        pmax = fmaxf(pmax, fmaxf(a, bb));
      }
      pmax = fmaxf(pmax, __shfl_xor(pmax, 32));

      const float m_new = fmaxf(m_run, pmax);
      // interior: m_new is finite, so a first-tile m_run of -3.0e38 gives
      // exp2(-3.0e38) = 0 without the guard, and every score is finite
      float alpha = __builtin_amdgcn_exp2f(m_run - m_new);
      if constexpr (MASKED) alpha = (m_run <= -3.0e38f) ? 0.f : alpha;
      m_run = m_new;
      float lsum = 0.f;
#pragma unroll
      for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          float e = __builtin_amdgcn_exp2f(sv[t][r] - m_new);
          if constexpr (MASKED) e = (sv[t][r] <= -3.0e38f) ? 0.f : e;
          sv[t][r] = e;
          lsum += e;
        }
      lsum += __shfl_xor(lsum, 32);
      l_run = l_run * alpha + lsum;
      return alpha;
    };
    // the accumulators stay out of the two-way branch (only sv, m, l and
    // alpha merge after it)
    const float alpha = interior ? softmax_tile(std::false_type{})
                                 : softmax_tile(std::true_type{});
#pragma unroll
    for (int t = 0; t < DT; ++t)
#pragma unroll
      for (int r = 0; r < 16; ++r) oacc[t][r] *= alpha;

    if (p_drop > 0.f) {
      const uint32_t thr8 = drop_threshold_u8(p_drop);
#pragma unroll
      for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int r4 = 0; r4 < 4; ++r4) {
          // regs r4*4..r4*4+3 cover kv run kvb..kvb+3 (4-aligned)
          const int kvb = kv0 + t * 32 + 8 * r4 + 4 * hi;
          const uint32_t h = drop_hash4(seed, bh, Sq, Sk >> 2, qg, kvb >> 2);
#pragma unroll
          for (int j = 0; j < 4; ++j)
            sv[t][r4 * 4 + j] *= drop_keep_byte(h, j, thr8, ks);
        }
    }

    // PV: O^T[d][q] += V^T x P
    PRIO_HI();
#pragma unroll
    for (int t = 0; t < 2; ++t) {
#pragma unroll
      for (int c16 = 0; c16 < 2; ++c16) {
        bf16x8_t pfrag = repack_chunk(&sv[t][c16 * 8]);
        const int kvc = t * 32 + c16 * 16;
#pragma unroll
        for (int dt = 0; dt < DT; ++dt) {
          bf16x8_t vfrag = tr_img_frag<D>(v_lds, ro + kvc, dt, lane);
          oacc[dt] =
              __builtin_amdgcn_mfma_f32_32x32x16_bf16(vfrag, pfrag, oacc[dt], 0, 0, 0);
        }
      }
    }
    PRIO_LO();
    }  // sub
  }

  const float inv_l = (l_run > 0.f) ? 1.0f / l_run : 0.f;
  bf16_t* op = o + b * o_sb + h * o_sh + (int64_t)qg * o_ss;
  if (qg < Sq) {
#pragma unroll
    for (int dt = 0; dt < DT; ++dt)
#pragma unroll
      for (int r4 = 0; r4 < 4; ++r4) {
        bf16x4_t pk;
#pragma unroll
        for (int j = 0; j < 4; ++j) pk[j] = (bf16_t)(oacc[dt][r4 * 4 + j] * inv_l);
        *(bf16x4_t*)(op + dt * 32 + 8 * r4 + 4 * hi) = pk;
      }
    if (hi == 0 && lse != nullptr)  // convert the exp2-domain max back to ln
      lse[((int64_t)bh * Sq) + qg] =
          m_run * 0.6931471805599453f + __logf(l_run > 0.f ? l_run : 1.f);
  }
}

// ===========================================================================
// Drow = rowsum(dO * O): one wave per 8 rows (8 lanes x 8 elems for D=64)
// out layout [B*H, Sq] (matches lse); inputs [B, Sq, H, D] strided
// ===========================================================================
template <int D>
__global__ void rowdot_kernel(const bf16_t* __restrict__ dout,
                              const bf16_t* __restrict__ o, float* __restrict__ drow,
                              int64_t sb, int64_t ss, int64_t sh, int H, int Sq,
                              int64_t nrows) {
  constexpr int LPR = D / 8;   // lanes per row
  constexpr int RPW = 64 / LPR;  // rows per wave
  const int64_t wave_id = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / 64;
  const int lane = threadIdx.x & 63;
  const int64_t row = wave_id * RPW + lane / LPR;  // flat (b*Sq+q)*H+h
  if (row >= nrows) return;
  const int64_t BSH = (int64_t)Sq * H;
  const int64_t b = row / BSH;
  const int64_t rem = row % BSH;
  const int64_t qi = rem / H;
  const int64_t h = rem % H;
  const bf16_t* dp = dout + b * sb + qi * ss + h * sh + (lane % LPR) * 8;
  const bf16_t* op = o + b * sb + qi * ss + h * sh + (lane % LPR) * 8;
  u16x8 dv = *(const u16x8*)dp;
  u16x8 ov = *(const u16x8*)op;
  float s = 0.f;
#pragma unroll
  for (int j = 0; j < 8; ++j) s += bf2f(dv[j]) * bf2f(ov[j]);
#pragma unroll
  for (int off = LPR / 2; off > 0; off >>= 1) s += __shfl_xor(s, off, 64);
  if (lane % LPR == 0) drow[(b * H + h) * Sq + qi] = s;
}

// ===========================================================================
// backward over kv tiles: dK, dV   (block = 128 kv rows, wave owns 32)
// ===========================================================================
// Every instantiation targets 2 waves/SIMD.  At D=64 that leaves room to hold
// the lane's K and V row fragments in registers (32 VGPRs), so the S/dPd
// chain has no operand fetch left in it: 188 VGPRs, no scratch.  The 3-wave
// form of the plain instantiation (159 VGPRs, no scratch, K/V re-read from L2
// per sub-tile) measured 2 % slower end to end (profiles/flash_tile_classes.md).
// D=128 (128 accumulator VGPRs) re-reads K/V per use and sits at 244-256.
//
// q-tile loop.  D=128 has no register left and keeps the plain form
//   for each q tile: barrier; stage; barrier; compute.
// D=64 (PIPE) prefetches on the registers that 2 waves/SIMD leave free: the
// global loads of tile qt+1 (Q, dO, lse, Drow and the RELB diagonals: 18-19
// VGPRs) are issued before the compute of tile qt and stored to LDS after it,
//   stage(first); barrier;
//   for each q tile: load(next); compute; barrier; write(next); barrier
// so their latency hides under 32 MFMAs per wave and the exp/dropout work.
// (stage() itself waits for each 16-byte load before it issues the next one:
// five round trips per tile in the plain form.)  The pipeline drains and
// restarts per GQA query head; all its conditions are workgroup-uniform.  The
// staged values, the compute body and their order are those of the plain
// loop, so dK and dV do not change by a bit.
template <int D, FlashVariant V>
__global__ __launch_bounds__(256, 2) void flash_bwd_kv_kernel(
    const bf16_t* __restrict__ q, const bf16_t* __restrict__ k,
    const bf16_t* __restrict__ v, const bf16_t* __restrict__ dout,
    const float* __restrict__ lse, const float* __restrict__ drow,
    const int* __restrict__ kv_len, bf16_t* __restrict__ dk,
    bf16_t* __restrict__ dv, int64_t q_sb, int64_t q_ss,
    int64_t q_sh, int64_t k_sb, int64_t k_ss, int64_t k_sh, int64_t v_sb,
    int64_t v_ss, int64_t v_sh, int64_t do_sb, int64_t do_ss, int64_t do_sh,
    int64_t dk_sb, int64_t dk_ss, int64_t dk_sh, int64_t dv_sb, int64_t dv_ss,
    int64_t dv_sh, int H, int Sq, int Sk, float scale, float p_drop, uint64_t seed,
    int causal, int kv_group, const float* __restrict__ alibi_slopes,
    int window, const float* __restrict__ rel_bias,
    const int* __restrict__ doc_end) {
  constexpr bool ALIBI = V == FlashVariant::kAlibi,
                 WINDOW = V == FlashVariant::kWindow,
                 RELB = V == FlashVariant::kRelBias, DOCS = V == FlashVariant::kDocs;
  constexpr int DT = D / 32;
  constexpr int KC = D / 16;
  // D=64: 64-row staging tiles.  D=128: 32-row tiles.
  constexpr int QTILE = (D == 64) ? 2 * QB : QB;
  constexpr int NSUB = QTILE / QB;
  // RELB: the QBLK + QTILE - 1 diagonals of one staged q tile (natural
  // domain), stored descending: entry (q - q0) + (QBLK - 1) - (kv - kv_block).
  // A lane's registers walk q, so its lookups are one loop-invariant address
  // plus non-negative immediates
  constexpr int KV_DIAGS = QBLK + QTILE - 1;
  __shared__ float rb_lds[RELB ? KV_DIAGS : 1];

  __shared__ __align__(16) bf16_t q_row[QTILE * D];
  __shared__ __align__(16) bf16_t q_tr[QTILE * D];
  __shared__ __align__(16) bf16_t do_row[QTILE * D];
  __shared__ __align__(16) bf16_t do_tr[QTILE * D];
  // row constants, 16B-aligned: a D-layout register run covers 4 consecutive
  // q rows, so each run takes its lse/Drow with one unconditional ds_read_b128
  __shared__ __align__(16) float lse_lds[QTILE];
  __shared__ __align__(16) float drow_lds[QTILE];
  constexpr bool PIPE = D == 64;

  const int tid = threadIdx.x;
  const int wave = tid >> 6;
  const int lane = tid & 63;
  const int l31 = lane & 31;
  const int hi = lane >> 5;

  // GQA: grid.y spans B * H_kv; each kv head's dK/dV accumulates the
  // contributions of its kv_group query heads (looped below)
  const int Hkv = H / kv_group;
  const int bhk = blockIdx.y;
  const int b = bhk / Hkv, hk = bhk % Hkv;
  const int kv_block = block_tile() * QBLK;   // 128 kv rows per block
  // this wave's 32 kv rows; wave-uniform (scalar skips and tile-class branch)
  const int kv_base = __builtin_amdgcn_readfirstlane(kv_block + wave * QB);
  const int kvg = kv_base + l31;            // lane's kv row

  const bf16_t* kp = k + b * k_sb + hk * k_sh;
  const bf16_t* vp = v + b * v_sb + hk * v_sh;

  // per-lane K and V row fragments (B-operands: lane j = kv), loop-invariant.
  // D=64 holds them in registers; D=128 re-reads them from global per use
  // (L2-resident: one K row per lane; register budget, see above).
  constexpr bool KV_PERSIST = D == 64;
  const int kvr_ld = min(kvg, Sk - 1);
  auto load_kf = [&](int c) {
    return *(const bf16x8_t*)(kp + (int64_t)kvr_ld * k_ss + c * 16 + hi * 8);
  };
  auto load_vf = [&](int c) {
    return *(const bf16x8_t*)(vp + (int64_t)kvr_ld * v_ss + c * 16 + hi * 8);
  };
  bf16x8_t kf[KV_PERSIST ? KC : 1], vf[KV_PERSIST ? KC : 1];
  if constexpr (KV_PERSIST) {
#pragma unroll
    for (int c = 0; c < KC; ++c) {
      kf[c] = load_kf(c);
      vf[c] = load_vf(c);
    }
  }
  auto get_kf = [&](int c) {
    if constexpr (KV_PERSIST) return kf[c];
    else return load_kf(c);
  };
  auto get_vf = [&](int c) {
    if constexpr (KV_PERSIST) return vf[c];
    else return load_vf(c);
  };

  f32x16_t dk_acc[DT], dv_acc[DT];
#pragma unroll
  for (int t = 0; t < DT; ++t) {
    dk_acc[t] = f32x16_t{};
    dv_acc[t] = f32x16_t{};
  }

  const float ks = (p_drop > 0.f) ? 1.0f / (1.0f - p_drop) : 1.0f;
  const int sk_eff = (kv_len != nullptr) ? kv_len[b] : Sk;
  const int qt_start = causal ? (kv_block / QTILE) : 0;
  // fully-padded kv block: accumulators stay zero, skip straight to the
  // (zero) writes.  kv_block is uniform across the block, so this does not
  // break the __syncthreads inside the loop.
  // sliding window: the last query that sees a key of this block is
  // kv_block + QBLK - 1 + window - 1, so the q-tile loop stops after the tile
  // holding it (uniform across the workgroup; the launcher clamps window to
  // the sequence length, so the sum cannot overflow)
  int q_hi = Sq;
  if constexpr (WINDOW) q_hi = min(Sq, kv_block + QBLK + window - 1);
  // packed documents: lane's upper bound; the block's highest bound (its last
  // valid key's: doc_end is non-decreasing) ends the q-tile loop for the whole
  // workgroup, the wave's last and first keys give the skip and the tile class
  int doc_hi = 0, doc_hi_w = 0, doc_hi_bot = 0;
  if constexpr (DOCS) {
    const int* dep = doc_end + (int64_t)b * Sk;
    doc_hi = doc_hi_load(dep, kvg, Sk);
    const int k_last = max(min(kv_block + QBLK, min(Sk, sk_eff)) - 1, 0);
    q_hi = min(Sq, __builtin_amdgcn_readfirstlane(doc_hi_load(dep, k_last, Sk)));
    doc_hi_w =
        __builtin_amdgcn_readfirstlane(doc_hi_load(dep, kv_base + QB - 1, Sk));
    doc_hi_bot = __builtin_amdgcn_readfirstlane(doc_hi_load(dep, kv_base, Sk));
  }
  const int n_qtiles = (kv_block < sk_eff) ? CDIV(q_hi, QTILE) : 0;

  // Dropout key of element (q, kv4), first mixer word, mod 2^32:
  //   (q * Sk4 + kv4) * LO_MUL = q_run * sk4_mul + hkey_lane
  // with q = q_run + 4 * hi + (l31 & 3).  q_run is wave-uniform, so each run
  // costs one scalar multiply and one add on a single loop-invariant VGPR
  // (written as in drop_hash4 the compiler keeps one pre-multiplied VGPR base
  // per run of the unrolled tile: 8 registers, spilled).
  const uint32_t sk4_mul = (uint32_t)(Sk >> 2) * RND_HASH_LO_MUL;
  const uint32_t hkey_lane =
      (uint32_t)(4 * hi + (l31 & 3)) * sk4_mul +
      (uint32_t)((kv_base + (l31 & ~3)) >> 2) * RND_HASH_LO_MUL;

  for (int g = 0; g < kv_group; ++g) {
  const int h = hk * kv_group + g;
  const int bh = b * H + h;  // q-head index: lse/drow rows + dropout key
  const uint32_t hkey_head = (uint32_t)seed ^ ((uint32_t)bh * RND_HASH_HI_MUL) ^
                             (uint32_t)(seed >> 32);
  const bf16_t* qp = q + b * q_sb + h * q_sh;
  const bf16_t* dop = dout + b * do_sb + h * do_sh;
  // ALiBi slope of THIS query head (the grid spans kv heads)
  float slope = 0.f;
  if constexpr (ALIBI) slope = alibi_slopes[h];
  // relative-position row of THIS query head
  const int n_diag = Sq + Sk - 1;
  const float* rbp = nullptr;
  if constexpr (RELB) rbp = rel_bias + (int64_t)h * n_diag;
  // lane's table entry for the first row of a staged q tile
  const float* rb_lane = rb_lds + ((QBLK - 1) - (kvg - kv_block) + 4 * hi);

  auto stage_all = [&](int qt) {
    const int q0 = qt * QTILE;
    stage_tile<QTILE, D, true, true>(q_row, q_tr, qp, q0, Sq, q_ss, tid);
    stage_tile<QTILE, D, true, true>(do_row, do_tr, dop, q0, Sq, do_ss, tid);
    if (tid < QTILE) {
      int qr = min(q0 + tid, Sq - 1);  // clamped: every staged row is readable
      lse_lds[tid] = lse[(int64_t)bh * Sq + qr];
      drow_lds[tid] = drow[(int64_t)bh * Sq + qr];
    }
    if constexpr (RELB) {
      if (tid < KV_DIAGS)
        rb_lds[tid] = relb_load(
            rbp, kv_block - q0 + (QBLK - 1) - tid + (Sq - 1), n_diag);
    }
  };

  // PIPE: stage_all split in two.  load_tile issues the global loads of tile
  // qt into registers (same clamping: rows >= Sq are zeros, lse/Drow and the
  // diagonals read a clamped neighbour) and does not wait for them;
  // write_tile stores them to LDS, which is where the wait for them lands.
  constexpr int PF = QTILE * D / 8 / 256;  // 16B chunks per thread and tensor
  bf16x8_t pf_q[PF], pf_do[PF];
  float pf_lse = 0.f, pf_drow = 0.f, pf_rb = 0.f;
  auto load_tile = [&](int qt) {
    const int q0 = qt * QTILE;
#pragma unroll
    for (int cc = 0; cc < PF; ++cc) {
      const int flat = tid + cc * 256;
      const int gr = q0 + flat / (D / 8);
      const int col8 = flat % (D / 8);
      pf_q[cc] = (gr < Sq)
                     ? *(const bf16x8_t*)(qp + (int64_t)gr * q_ss + col8 * 8)
                     : bf16x8_t{};
      pf_do[cc] = (gr < Sq)
                      ? *(const bf16x8_t*)(dop + (int64_t)gr * do_ss + col8 * 8)
                      : bf16x8_t{};
    }
    if (tid < QTILE) {
      int qr = min(q0 + tid, Sq - 1);
      pf_lse = lse[(int64_t)bh * Sq + qr];
      pf_drow = drow[(int64_t)bh * Sq + qr];
    }
    if constexpr (RELB) {
      if (tid < KV_DIAGS)
        pf_rb = relb_load(
            rbp, kv_block - q0 + (QBLK - 1) - tid + (Sq - 1), n_diag);
    }
  };
  auto write_tile = [&] {
#pragma unroll
    for (int cc = 0; cc < PF; ++cc) {
      const int flat = tid + cc * 256;
      const int row = flat / (D / 8);
      const int col8 = flat % (D / 8);
      row_img_write<D>(q_row, row, col8, pf_q[cc]);
      tr_img_write<D>(q_tr, row, col8 * 8, pf_q[cc]);
      row_img_write<D>(do_row, row, col8, pf_do[cc]);
      tr_img_write<D>(do_tr, row, col8 * 8, pf_do[cc]);
    }
    if (tid < QTILE) {
      lse_lds[tid] = pf_lse;
      drow_lds[tid] = pf_drow;
    }
    if constexpr (RELB) {
      if (tid < KV_DIAGS) rb_lds[tid] = pf_rb;
    }
  };
  // s_waitcnt vmcnt(0) alone (expcnt and lgkmcnt fields all ones).  Placed
  // where no load is in flight any more, so it costs nothing; it tells the
  // compiler on EVERY path into compute_tile that the K/V fragment loads from
  // the kernel's top are done.  Without it the path that issues no prefetch
  // (last tile) leaves them pending in the compiler's model, and the counted
  // waits it then puts in front of the S/dPd MFMAs (vmcnt(7) ... vmcnt(0))
  // also wait for the prefetch that was issued behind them.
  auto vm_drain = [] { __builtin_amdgcn_s_waitcnt(0x0F70); };

  auto compute_tile = [&](int q0) {
    if (causal && q0 + QTILE - 1 < kv_base) return;  // entirely above diag
    if constexpr (WINDOW) {  // entirely below this wave's band
      if (q0 - (kv_base + QB - 1) >= window) return;
    }
    if constexpr (DOCS) {  // entirely behind this wave's documents
      if (q0 >= doc_hi_w) return;
    }

    // rolled: one copy of the four element bodies, and no per-sub-tile set of
    // hoisted addresses (unrolled, D=64 took 254 VGPRs instead of 188)
#pragma unroll 1
    for (int sub = 0; sub < NSUB; ++sub) {
      const int q0s = q0 + sub * QB;
      if (causal && q0s + QB - 1 < kv_base) continue;
      if constexpr (WINDOW) {
        if (q0s - (kv_base + QB - 1) >= window) continue;
      }
      if constexpr (DOCS) {
        if (q0s >= doc_hi_w) continue;
      }
      const int ro = sub * QB;  // row offset inside the staged images

      // S[q][kv] = Q x K^T  (lane col = kv)
      f32x16_t s{};
      f32x16_t dpd{};
      PRIO_HI();
#pragma unroll
      for (int c = 0; c < KC; ++c) {
        bf16x8_t qa = row_img_frag<D>(q_row, ro + l31, c, hi);
        s = __builtin_amdgcn_mfma_f32_32x32x16_bf16(qa, get_kf(c), s, 0, 0, 0);
        bf16x8_t da = row_img_frag<D>(do_row, ro + l31, c, hi);
        dpd = __builtin_amdgcn_mfma_f32_32x32x16_bf16(da, get_vf(c), dpd, 0, 0, 0);
      }
      PRIO_LO();

      // tile class, as in the forward (wave-uniform, scalar branch; the
      // ds_read_b64_tr_b16 reads below need EXEC all ones)
      bool interior = q0s + QB <= Sq && kv_base + QB <= sk_eff &&
                      (!causal || q0s >= kv_base + QB - 1);
      if constexpr (WINDOW)
        interior = interior && (q0s + QB - 1 - kv_base < window);
      if constexpr (DOCS) interior = interior && (q0s + QB - 1 < doc_hi_bot);

      // per-chunk: compute Pd/dS for 8 regs, repack, feed the MFMAs (short
      // lifetimes).  The element body is instantiated on MASKED (tile class)
      // and on DROP, so that no uniform branch on p_drop splits a body; only
      // pd8/ds8 merge after the branch, the accumulators never enter it.
#pragma unroll
      for (int c16 = 0; c16 < 2; ++c16) {
        float pd8[8], ds8[8];
        auto elems = [&](auto masked_c, auto drop_c) {
        constexpr bool MASKED = decltype(masked_c)::value;
        constexpr bool DROP = decltype(drop_c)::value;
        // dropout hashes, quad-distributed: each element needs the draw for
        // (its qrow, lane's kv4); the 4 lanes of a quad share kv4 and the 4
        // qrows of a run are consecutive, so lane (l&3) computes the run's
        // (qbase + l&3) hash and DPP quad-perm broadcasts each one back.
        // (A straight per-element hash makes the compiler hoist 16 hash
        // bases per subtile -> 25+ VGPR spills into the hot loop.)
        const uint32_t thr8 = drop_threshold_u8(p_drop);
        const int byte_sh = (l31 & 3) * 8;
#pragma unroll
        for (int r4 = 0; r4 < 2; ++r4) {
          const int qbase = q0s + c16 * 16 + 8 * r4 + 4 * hi;
          // the run's four row constants, one unconditional 16B read each
          const float4 lse4 = *(const float4*)__builtin_assume_aligned(
              &lse_lds[qbase - q0], 16);
          const float4 drow4 = *(const float4*)__builtin_assume_aligned(
              &drow_lds[qbase - q0], 16);
          const float lse_r[4] = {lse4.x, lse4.y, lse4.z, lse4.w};
          const float drow_r[4] = {drow4.x, drow4.y, drow4.z, drow4.w};
          const float* rb_run = rb_lane + (qbase - 4 * hi - q0);
          uint32_t hq = 0;
          if constexpr (DROP)  // == drop_hash4(.., qbase + (l31 & 3), kv4q)
            hq = rnd_hash_mix(
                hkey_head ^
                (__builtin_amdgcn_readfirstlane(
                     (uint32_t)(q0s + c16 * 16 + 8 * r4) * sk4_mul) +
                 hkey_lane));
          uint32_t hqj[4];
          hqj[0] = (uint32_t)__builtin_amdgcn_mov_dpp((int)hq, 0x00, 0xF, 0xF, true);
          hqj[1] = (uint32_t)__builtin_amdgcn_mov_dpp((int)hq, 0x55, 0xF, 0xF, true);
          hqj[2] = (uint32_t)__builtin_amdgcn_mov_dpp((int)hq, 0xAA, 0xF, 0xF, true);
          hqj[3] = (uint32_t)__builtin_amdgcn_mov_dpp((int)hq, 0xFF, 0xF, 0xF, true);
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const int k = r4 * 4 + j;
            const int r = c16 * 8 + k;
            const int qrow = qbase + j;
            // x = scale * s (+ bias) - lse, the exp argument.  (kv - q) is
            // recomputed per element: nothing extra stays live across the
            // subtile on this kernel's register budget
            float x;
            if constexpr (ALIBI)
              x = fmaf(slope, (float)(kvg - qrow), s[r] * scale) - lse_r[j];
            else if constexpr (RELB)  // a zero table gives the plain bits
              x = fmaf(s[r], scale, rb_run[j] - lse_r[j]);
            else
              x = fmaf(s[r], scale, -lse_r[j]);
            float keep = 1.f;
            if constexpr (DROP)
              keep = (((hqj[j] >> byte_sh) & 0xFFu) >= thr8) ? ks : 0.f;
            if constexpr (MASKED) {
              // select-based: masked P and dS are exact zeros
              bool valid =
                  qrow < Sq && kvg < sk_eff && (!causal || qrow >= kvg);
              if constexpr (WINDOW) valid = valid && (qrow - kvg < window);
              if constexpr (DOCS) valid = valid && (qrow < doc_hi);
              const uint32_t vm = valid ? 0xFFFFFFFFu : 0u;
              const float p = and_f32(__expf(x), vm);
              pd8[k] = p * keep;
              ds8[k] = and_f32(
                  scale * p * mul_then_sub(dpd[r], keep, drow_r[j]), vm);
            } else {
              const float p = __expf(x);
              pd8[k] = p * keep;
              ds8[k] = scale * p * mul_then_sub(dpd[r], keep, drow_r[j]);
            }
          }
        }
        };  // elems
        if (p_drop > 0.f) {
          if (interior) elems(std::false_type{}, std::true_type{});
          else elems(std::true_type{}, std::true_type{});
        } else {
          if (interior) elems(std::false_type{}, std::false_type{});
          else elems(std::true_type{}, std::false_type{});
        }
        bf16x8_t pdf = repack_chunk(pd8);
        bf16x8_t dsf = repack_chunk(ds8);
        const int qc = ro + c16 * 16;
        PRIO_HI();
#pragma unroll
        for (int dt = 0; dt < DT; ++dt) {
          bf16x8_t dof = tr_img_frag<D>(do_tr, qc, dt, lane);
          dv_acc[dt] =
              __builtin_amdgcn_mfma_f32_32x32x16_bf16(dof, pdf, dv_acc[dt], 0, 0, 0);
          bf16x8_t qtf = tr_img_frag<D>(q_tr, qc, dt, lane);
          dk_acc[dt] =
              __builtin_amdgcn_mfma_f32_32x32x16_bf16(qtf, dsf, dk_acc[dt], 0, 0, 0);
        }
        PRIO_LO();
      }
    }
  };  // compute_tile

  if constexpr (PIPE) {
    // n_qtiles == 0 (fully padded kv block) and a window that ends the loop
    // early skip whole iterations: qt_start and n_qtiles are workgroup-uniform
    if (qt_start < n_qtiles) {
      // the images are free: the previous head's last compute ended in a barrier
      stage_all(qt_start);
      __syncthreads();
    }
    for (int qt = qt_start; qt < n_qtiles; ++qt) {
      const bool more = qt + 1 < n_qtiles;
      vm_drain();
      if (more) load_tile(qt + 1);
      compute_tile(qt * QTILE);
      __syncthreads();  // every wave has read tile qt
      if (more) {
        write_tile();
        __syncthreads();
      }
    }
  } else {
    for (int qt = qt_start; qt < n_qtiles; ++qt) {
      __syncthreads();
      stage_all(qt);
      __syncthreads();
      compute_tile(qt * QTILE);
    }
  }

  }  // group loop (GQA)

  // write dK, dV rows (lane owns kv row kvg; d in 4-element runs)
  if (kvg < Sk) {
    bf16_t* dkp = dk + b * dk_sb + hk * dk_sh + (int64_t)kvg * dk_ss;
    bf16_t* dvp = dv + b * dv_sb + hk * dv_sh + (int64_t)kvg * dv_ss;
#pragma unroll
    for (int dt = 0; dt < DT; ++dt)
#pragma unroll
      for (int r4 = 0; r4 < 4; ++r4) {
        bf16x4_t a, c;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          a[j] = (bf16_t)dk_acc[dt][r4 * 4 + j];
          c[j] = (bf16_t)dv_acc[dt][r4 * 4 + j];
        }
        *(bf16x4_t*)(dkp + dt * 32 + 8 * r4 + 4 * hi) = a;
        *(bf16x4_t*)(dvp + dt * 32 + 8 * r4 + 4 * hi) = c;
      }
  }
}

// ===========================================================================
// backward over q tiles: dQ   (block = 128 q rows, wave owns 32; fwd-like)
// ===========================================================================
// RELB: this kernel also reduces the bias gradient, dS without `scale`
// summed along diagonals.  A lane owns one query and its registers walk kv,
// so for a fixed register the lanes of a wave hit consecutive diagonals.  A
// sub-tile's 16 registers are first summed along the diagonals with lane
// rotations (see ds_tile); the two LDS float atomics per lane that remain
// collide two-way at most (hi = 0/1).  The sums live in a ring
// indexed by the block diagonal a = kv + (QBLK - 1) - (q - q_block): the tile
// at kv0 touches a in [kv0, kv0 + KVTILE + QBLK - 2], so once a tile is done
// the diagonals below the next kv0 are complete.  They are flushed at the top
// of the next staging round, between the two barriers the loop already has,
// and the rest behind the loop: one global fp32 atomic per (workgroup,
// touched diagonal), whatever the sequence length.
template <int D, FlashVariant V>
__global__ __launch_bounds__(256, 2) void flash_bwd_q_kernel(
    const bf16_t* __restrict__ q, const bf16_t* __restrict__ k,
    const bf16_t* __restrict__ v, const bf16_t* __restrict__ dout,
    const float* __restrict__ lse, const float* __restrict__ drow,
    const int* __restrict__ kv_len, bf16_t* __restrict__ dq, int64_t q_sb,
    int64_t q_ss, int64_t q_sh, int64_t k_sb,
    int64_t k_ss, int64_t k_sh, int64_t v_sb, int64_t v_ss, int64_t v_sh,
    int64_t do_sb, int64_t do_ss, int64_t do_sh, int64_t dq_sb, int64_t dq_ss,
    int64_t dq_sh, int H, int Sq, int Sk, float scale, float p_drop, uint64_t seed,
    int causal, int kv_group, const float* __restrict__ alibi_slopes,
    int window, const float* __restrict__ rel_bias,
    float* __restrict__ d_rel_bias, const int* __restrict__ doc_start) {
  constexpr bool ALIBI = V == FlashVariant::kAlibi,
                 WINDOW = V == FlashVariant::kWindow,
                 RELB = V == FlashVariant::kRelBias, DOCS = V == FlashVariant::kDocs;
  constexpr int DT = D / 32;
  constexpr int KC = D / 16;
  constexpr int KVTILE = (D == 64) ? 2 * QB : QB;
  constexpr int NSUB = KVTILE / QB;

  __shared__ __align__(16) bf16_t k_row[KVTILE * D];
  __shared__ __align__(16) bf16_t k_tr[KVTILE * D];
  __shared__ __align__(16) bf16_t v_row[KVTILE * D];
  // RELB: the KVTILE + QBLK - 1 diagonals of one staged kv tile, entry
  // (kv - kv0) + (QBLK - 1) - (q - q_block); and the ring of gradient sums
  constexpr int Q_DIAGS = KVTILE + QBLK - 1;
  static_assert(Q_DIAGS <= RELB_RING, "a tile's diagonals must fit the ring");
  __shared__ float rb_lds[RELB ? Q_DIAGS : 1];
  __shared__ float drb_lds[RELB ? RELB_RING : 1];

  const int tid = threadIdx.x;
  const int wave = tid >> 6;
  const int lane = tid & 63;
  const int l31 = lane & 31;
  const int hi = lane >> 5;

  const int bh = blockIdx.y;
  const int b = bh / H, h = bh % H;
  const int q_block = block_tile() * QBLK;
  // wave-uniform: scalar sub-tile skips and tile-class branch (see forward)
  const int q_base = __builtin_amdgcn_readfirstlane(q_block + wave * QB);
  const int qg = q_base + l31;

  const int hk = h / kv_group;  // GQA
  const bf16_t* qp = q + b * q_sb + h * q_sh;
  const bf16_t* kp = k + b * k_sb + hk * k_sh;
  const bf16_t* vp = v + b * v_sb + hk * v_sh;
  const bf16_t* dop = dout + b * do_sb + h * do_sh;

  // per-lane Q and dO row fragments (B-operands: lane j = q), loop-invariant
  // and held in registers at both head dims.  At D=128 that is 64 VGPRs and
  // 2 waves/SIMD (223-249 VGPRs, no scratch): re-reading them from global in
  // front of each MFMA of the S/dPd chain measured 2-3x slower, at 2 waves
  // and at 3 (profiles/flash_tile_classes.md).
  const int qr_ld = min(qg, Sq - 1);
  bf16x8_t qf[KC], dof[KC];
#pragma unroll
  for (int c = 0; c < KC; ++c) {
    qf[c] = *(const bf16x8_t*)(qp + (int64_t)qr_ld * q_ss + c * 16 + hi * 8);
    dof[c] = *(const bf16x8_t*)(dop + (int64_t)qr_ld * do_ss + c * 16 + hi * 8);
  }
  const float lse_lane = lse[(int64_t)bh * Sq + min(qg, Sq - 1)];
  const float drow_lane = drow[(int64_t)bh * Sq + min(qg, Sq - 1)];
  float slope = 0.f;
  if constexpr (ALIBI) slope = alibi_slopes[h];

  f32x16_t dq_acc[DT];
#pragma unroll
  for (int t = 0; t < DT; ++t) dq_acc[t] = f32x16_t{};

  const float ks = (p_drop > 0.f) ? 1.0f / (1.0f - p_drop) : 1.0f;
  const int sk_eff = (kv_len != nullptr) ? kv_len[b] : Sk;
  const int kv_end = causal ? min(sk_eff, q_block + QBLK) : sk_eff;
  const int n_tiles = CDIV(kv_end, KVTILE);

  // sliding window: start at the tile holding the block's lowest visible key
  int tile0 = 0;
  if constexpr (WINDOW) tile0 = max(0, q_block - window + 1) / KVTILE;
  // packed documents: as in the forward
  int doc_lo = 0, doc_lo_w = 0, doc_lo_top = 0;
  if constexpr (DOCS) {
    const int* dsp = doc_start + (int64_t)b * Sq;
    doc_lo = doc_lo_load(dsp, qg, Sq);
    tile0 = __builtin_amdgcn_readfirstlane(doc_lo_load(dsp, q_block, Sq)) / KVTILE;
    doc_lo_w = __builtin_amdgcn_readfirstlane(doc_lo_load(dsp, q_base, Sq));
    doc_lo_top =
        __builtin_amdgcn_readfirstlane(doc_lo_load(dsp, q_base + QB - 1, Sq));
  }

  const int n_diag = Sq + Sk - 1;
  const float* rbp = nullptr;
  float* drbp = nullptr;
  if constexpr (RELB) {
    rbp = rel_bias + (int64_t)h * n_diag;
    drbp = d_rel_bias + (int64_t)h * n_diag;
    drb_lds[tid] = 0.f;  // 256 threads, RELB_RING slots
  }
  // lane's table entry for the first key of a tile
  const int rb_lane = (QBLK - 1) - (qg - q_block);
  // global diagonal of a tile's entry 0, minus the tile's first key
  const int rb_t0 = (Sq - 1) - q_block - (QBLK - 1);

  for (int tile = tile0; tile < n_tiles; ++tile) {
    const int kv0 = tile * KVTILE;
    __syncthreads();
    stage_tile<KVTILE, D, true, true>(k_row, k_tr, kp, kv0, Sk, k_ss, tid);
    stage_tile<KVTILE, D, true, false>(v_row, nullptr, vp, kv0, Sk, v_ss, tid);
    if constexpr (RELB) {
      if (tile > tile0)  // the diagonals the previous tile completed
        relb_flush(drb_lds, drbp, tid, KVTILE, kv0 - KVTILE, rb_t0, n_diag);
      if (tid < Q_DIAGS)
        rb_lds[tid] = relb_load(rbp, kv0 + rb_t0 + tid, n_diag);
    }
    __syncthreads();

    if (causal && kv0 > q_base + QB - 1) continue;

#pragma unroll
    for (int sub = 0; sub < NSUB; ++sub) {
      const int kv0s = kv0 + sub * QB;
      if (kv0s >= kv_end || (causal && kv0s > q_base + QB - 1)) continue;
      if constexpr (WINDOW) {  // sub-tile entirely below this wave's band
        if (kv0s + QB - 1 < q_base - window + 1) continue;
      }
      if constexpr (DOCS) {  // sub-tile entirely before this wave's documents
        if (kv0s + QB - 1 < doc_lo_w) continue;
      }
      const int ro = sub * QB;

      // S^T[kv][q] = K x Q^T ;  dPd^T[kv][q] = V x dO^T   (lane col = q)
      f32x16_t st{};
      f32x16_t dpdt{};
      PRIO_HI();
#pragma unroll
      for (int c = 0; c < KC; ++c) {
        bf16x8_t ka = row_img_frag<D>(k_row, ro + l31, c, hi);
        st = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ka, qf[c], st, 0, 0, 0);
        bf16x8_t va = row_img_frag<D>(v_row, ro + l31, c, hi);
        dpdt = __builtin_amdgcn_mfma_f32_32x32x16_bf16(va, dof[c], dpdt, 0, 0, 0);
      }
      PRIO_LO();

      float ds[16];
      // tile class, as in the forward (wave-uniform, scalar branch)
      bool interior = kv0s + QB <= sk_eff && q_base + QB <= Sq &&
                      (!causal || q_base >= kv0s + QB - 1);
      if constexpr (WINDOW)
        interior = interior && (q_base + QB - 1 - kv0s < window);
      if constexpr (DOCS) interior = interior && (kv0s >= doc_lo_top);
      auto ds_tile = [&](auto masked_c) {
        constexpr bool MASKED = decltype(masked_c)::value;
        const uint32_t thr8 = drop_threshold_u8(p_drop);
        // kv - q of this lane's first score (ALiBi)
        float rel0 = 0.f;
        if constexpr (ALIBI) rel0 = (float)(kv0s + 4 * hi - qg);
        // RELB: the sub-tile's sums are formed in registers first.  Register r
        // of lane l31 sits on diagonal (register 0's) + sh - l31 with
        // sh = (r & 3) + 8 * (r >> 2), so rotating it down by sh lanes inside
        // the 32-lane half puts it on the receiving lane's register-0
        // diagonal, or 32 above it where the rotation wrapped.  Two LDS
        // atomics per lane and sub-tile then replace sixteen, which measured
        // 6x the whole plain kernel.  D=128 has no registers for the fifteen
        // rotation addresses (256 VGPRs, 40 B/lane of scratch, reloads in the
        // tile loop) and keeps one atomic per element.
        constexpr bool PRE_REDUCE = D == 64;
        // register 0's block diagonal in the gradient ring
        const int slot0 = (rb_lane + kv0s + 4 * hi) & (RELB_RING - 1);
        float g_main = 0.f, g_wrap = 0.f;
        auto diag_add = [&](int r, float gv) {
          const int sh = (r & 3) + 8 * (r >> 2);
          if constexpr (!PRE_REDUCE) {
            atomicAdd(&drb_lds[(slot0 + sh) & (RELB_RING - 1)], gv);
          } else if (sh == 0) {
            g_main = gv;
          } else {
            const float t = __shfl(gv, ((l31 + sh) & 31) | (lane & 32));
            const bool wrapped = l31 + sh >= 32;
            g_main += wrapped ? 0.f : t;
            g_wrap += wrapped ? t : 0.f;
          }
        };
#pragma unroll
        for (int r4 = 0; r4 < 4; ++r4) {
          const int kvb = kv0s + 8 * r4 + 4 * hi;  // 4-aligned kv run
          const uint32_t h = (p_drop > 0.f)
                                 ? drop_hash4(seed, bh, Sq, Sk >> 2, qg, kvb >> 2)
                                 : 0;
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const int r = r4 * 4 + j;
            const int kv = kvb + j;
            float x;  // scale * s (+ bias) - lse, the exp argument
            // this element's table entry (in range for every lane)
            int e = 0;
            if constexpr (RELB) e = rb_lane + (kv - kv0);
            if constexpr (ALIBI)
              x = fmaf(slope, rel0 + (float)(8 * r4 + j), st[r] * scale) - lse_lane;
            else if constexpr (RELB)  // a zero table gives the plain bits
              x = fmaf(st[r], scale, rb_lds[e] - lse_lane);
            else
              x = fmaf(st[r], scale, -lse_lane);
            // RELB: dS without `scale` goes to the diagonal's sum (the bias
            // enters after the scaling, so `scale` must not reach it)
            if constexpr (MASKED) {
              bool valid = kv < sk_eff && qg < Sq && (!causal || kv <= qg);
              if constexpr (WINDOW) valid = valid && (qg - kv < window);
              if constexpr (DOCS) valid = valid && (kv >= doc_lo);
              const uint32_t vm = valid ? 0xFFFFFFFFu : 0u;
              float p = and_f32(__expf(x), vm);
              float keep = (p_drop > 0.f) ? drop_keep_byte(h, j, thr8, ks) : 1.f;
              // (scale * p) * dd, the product formed first as it always was
              const float sp = scale * p;
              const float dd = fmaf(dpdt[r], keep, -drow_lane);
              ds[r] = and_f32(sp * dd, vm);
              if constexpr (RELB) diag_add(r, and_f32(p * dd, vm));
            } else {
              float p = __expf(x);
              float keep = (p_drop > 0.f) ? drop_keep_byte(h, j, thr8, ks) : 1.f;
              const float sp = scale * p;
              const float dd = fmaf(dpdt[r], keep, -drow_lane);
              ds[r] = sp * dd;
              if constexpr (RELB) diag_add(r, p * dd);
            }
          }
        }
        if constexpr (RELB && PRE_REDUCE) {  // slot0 and the one 32 above it
          atomicAdd(&drb_lds[slot0], g_main);
          atomicAdd(&drb_lds[(slot0 + 32) & (RELB_RING - 1)], g_wrap);
        }
      };
      if (interior) ds_tile(std::false_type{});
      else ds_tile(std::true_type{});

      // dQ^T[d][q] += K^T x dS^T
      PRIO_HI();
#pragma unroll
      for (int c16 = 0; c16 < 2; ++c16) {
        bf16x8_t dsf = repack_chunk(&ds[c16 * 8]);
        const int kvc = ro + c16 * 16;
#pragma unroll
        for (int dt = 0; dt < DT; ++dt) {
          bf16x8_t ktf = tr_img_frag<D>(k_tr, kvc, dt, lane);
          dq_acc[dt] =
              __builtin_amdgcn_mfma_f32_32x32x16_bf16(ktf, dsf, dq_acc[dt], 0, 0, 0);
        }
      }
      PRIO_LO();
    }
  }

  if constexpr (RELB) {  // the diagonals still open after the last tile
    __syncthreads();
    if (n_tiles > tile0)
      relb_flush(drb_lds, drbp, tid, Q_DIAGS, (n_tiles - 1) * KVTILE, rb_t0,
                 n_diag);
  }

  if (qg < Sq) {
    bf16_t* dqp = dq + b * dq_sb + h * dq_sh + (int64_t)qg * dq_ss;
#pragma unroll
    for (int dt = 0; dt < DT; ++dt)
#pragma unroll
      for (int r4 = 0; r4 < 4; ++r4) {
        bf16x4_t a;
#pragma unroll
        for (int j = 0; j < 4; ++j) a[j] = (bf16_t)dq_acc[dt][r4 * 4 + j];
        *(bf16x4_t*)(dqp + dt * 32 + 8 * r4 + 4 * hi) = a;
      }
  }
}

// dropout-mask application for external recompute paths / tests
template <class E>
__global__ void attn_dropout_apply_kernel(typename E::T* __restrict__ x, int64_t BH,
                                          int64_t Sq, int64_t Sk, float p,
                                          float keep_scale, uint64_t seed) {
  const int64_t total = BH * Sq * Sk;
  const uint32_t thr8 = drop_threshold_u8(p);
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total;
       i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t row = i / Sk;
    const int kv = (int)(i % Sk);
    uint32_t h = rnd_hash2(seed, (uint32_t)(row % Sq) * (uint32_t)(Sk >> 2) +
                                     (uint32_t)(kv >> 2),
                           (uint32_t)(row / Sq));
    float kp = drop_keep_byte(h, kv & 3, thr8, keep_scale);
    x[i] = E::from_f(E::to_f(x[i]) * kp);
  }
}

}  // namespace

// the kernels take typed pointers; the ABI struct carries void*
static const bf16_t* in(const StridedBSHD& t) { return (const bf16_t*)t.ptr; }
static bf16_t* out(const StridedBSHD& t) { return (bf16_t*)t.ptr; }

// same mask, no overflow in the kernels' row arithmetic
static int clamp_window(int window, int Sq, int Sk) {
  return window > 0 ? min(window, max(Sq, Sk)) : 0;
}

extern "C" void flash_fwd_bf16(const FlashFwdArgs& a, hipStream_t stream) {
  const dim3 grid(CDIV(a.Sq, QBLK), a.B * a.H), block(256);
  const int window = clamp_window(a.window, a.Sq, a.Sk);
  const FlashVariant variant =
      flash_variant(a.alibi_slopes, window, a.rel_bias, a.doc_start);
  flash_dispatch(a.D, variant, [&](auto dc, auto vc) {
    constexpr int DD = decltype(dc)::value;
    constexpr FlashVariant VV = decltype(vc)::value;
    auto launch = [&](auto offs) {
      flash_fwd_kernel<DD, VV, decltype(offs)::value>
          <<<grid, block, 0, stream>>>(
              in(a.q), in(a.k), in(a.v), out(a.o), a.lse, a.kv_len,
              a.q.sb, a.q.ss, a.q.sh,
              a.k.sb, a.k.ss, a.k.sh,
              a.v.sb, a.v.ss, a.v.sh,
              a.o.sb, a.o.ss, a.o.sh,
              a.H, a.Sq, a.Sk, a.scale, a.p_drop, a.seed, a.causal, a.kv_group,
              a.alibi_slopes, window, a.rel_bias, a.doc_start, a.q_off);
    };
    // the offset instantiations exist for plain, ALiBi and window only (the
    // binding rejects an offset with the other two)
    if constexpr (VV == FlashVariant::kPlain || VV == FlashVariant::kAlibi ||
                  VV == FlashVariant::kWindow) {
      if (a.q_off > 0) {
        launch(std::true_type{});
        return;
      }
    }
    launch(std::false_type{});
  });
}

extern "C" void flash_bwd_bf16(const FlashBwdArgs& a, hipStream_t stream) {
  const dim3 block(256);
  const int Hkv = a.H / a.kv_group;  // bwd_kv grid spans the KV heads
  const dim3 grid_kv(CDIV(a.Sk, QBLK), a.B * Hkv), grid_q(CDIV(a.Sq, QBLK), a.B * a.H);
  const int window = clamp_window(a.window, a.Sq, a.Sk);
  const FlashVariant variant =
      flash_variant(a.alibi_slopes, window, a.rel_bias, a.doc_start);
  // Drow = rowsum(dO * O)  (dO and O share layout; use dO's strides for both:
  // the wrapper guarantees o was allocated with the same layout)
  const int rpw = 64 / (a.D / 8);
  const int64_t rows = (int64_t)a.B * a.Sq * a.H;
  const uint32_t rowdot_blocks = (uint32_t)CDIV(CDIV(rows, rpw) * 64, 256);
  flash_dispatch(a.D, variant, [&](auto dc, auto vc) {
    constexpr int DD = decltype(dc)::value;
    constexpr FlashVariant VV = decltype(vc)::value;
    rowdot_kernel<DD><<<dim3(rowdot_blocks), 256, 0, stream>>>(
        in(a.dout), in(a.o), a.drow_ws, a.dout.sb, a.dout.ss, a.dout.sh, a.H, a.Sq,
        rows);
    flash_bwd_kv_kernel<DD, VV><<<grid_kv, block, 0, stream>>>(
        in(a.q), in(a.k), in(a.v), in(a.dout), a.lse, a.drow_ws, a.kv_len,
        out(a.dk), out(a.dv),
        a.q.sb, a.q.ss, a.q.sh,
        a.k.sb, a.k.ss, a.k.sh,
        a.v.sb, a.v.ss, a.v.sh,
        a.dout.sb, a.dout.ss, a.dout.sh,
        a.dk.sb, a.dk.ss, a.dk.sh,
        a.dv.sb, a.dv.ss, a.dv.sh,
        a.H, a.Sq, a.Sk, a.scale, a.p_drop, a.seed, a.causal, a.kv_group,
        a.alibi_slopes, window, a.rel_bias, a.doc_end);
    flash_bwd_q_kernel<DD, VV><<<grid_q, block, 0, stream>>>(
        in(a.q), in(a.k), in(a.v), in(a.dout), a.lse, a.drow_ws, a.kv_len,
        out(a.dq),
        a.q.sb, a.q.ss, a.q.sh,
        a.k.sb, a.k.ss, a.k.sh,
        a.v.sb, a.v.ss, a.v.sh,
        a.dout.sb, a.dout.ss, a.dout.sh,
        a.dq.sb, a.dq.ss, a.dq.sh,
        a.H, a.Sq, a.Sk, a.scale, a.p_drop, a.seed, a.causal, a.kv_group,
        a.alibi_slopes, window, a.rel_bias, a.d_rel_bias, a.doc_start);
  });
}

#define ATTN_DROP_LAUNCHER(SUFF, ETYPE)                                            \
  extern "C" void attn_dropout_apply_##SUFF(void* x, int64_t BH, int64_t Sq,       \
                                            int64_t Sk, float p, uint64_t seed,    \
                                            hipStream_t stream) {                  \
    int64_t n = BH * Sq * Sk;                                                      \
    int64_t g = CDIV(n, 256);                                                      \
    if (g > 4096) g = 4096;                                                        \
    attn_dropout_apply_kernel<ETYPE><<<dim3((uint32_t)g), dim3(256), 0, stream>>>( \
        (ETYPE::T*)x, BH, Sq, Sk, p, 1.0f / (1.0f - p), seed);                     \
  }

ATTN_DROP_LAUNCHER(bf16, BF16Elem)
ATTN_DROP_LAUNCHER(f32, F32Elem)
