// Mixture-of-Experts routing, dispatch and combine for gfx950 (top-k,
// dropless).  Replaces the torch chain around the expert GEMMs in
// layers/moe.py: softmax / topk / renormalise / histogram, the stable argsort,
// repeat_interleave + gather, the inverse-permutation gather and the gated
// bf16 sum.
//
//   moe_route_kernel      fp32 softmax over E experts, top-k on the raw logits,
//                         renormalised gates; per-block expert histogram and
//                         softmax column sums
//   moe_scan_kernel       one workgroup: histogram -> per-block slot bases,
//                         counts, expert offsets, folded column sums
//   moe_plan_kernel       stable counting sort: slot[f] and its inverse
//   moe_route_bwd_kernel  dlogits from dgates and dpsum (softmax recomputed)
//   moe_permute_kernel    xk[s] = x[row_of_slot[s] / k]
//   moe_combine_kernel    y[i] = sum_j gates[i,j] * yk[slot[i*k+j]] (+ res[i]);
//                         without gates it is the permute backward
//   moe_combine_bwd_kernel  dyk[s] = g * dy[i], dgates = <dy[i], yk[s]>
//
// Work split of the routing kernels: a token is served by a lane group of
// G = max(4, pow2ceil(min(E, 64))) lanes, lane gl holding experts gl, gl + G,
// ... (EPL = ceil(E / 64) of them when E > 64), so at E = 8 a wave routes 8
// tokens at once and every reduction of a row is a shuffle inside the group.
// A workgroup owns a CONTIGUOUS range of `tpb` tokens; the plan kernel uses
// the same range, which is what makes (block, wave, lane) order equal to
// ascending copy index f = i * k + j and the counting sort stable.
//
// Determinism: no float atomics.  A lane sums the probabilities of its own
// experts over the tokens it serves, the groups of a wave fold by shuffles,
// the waves of a block fold through LDS in wave order, and the scan kernel
// folds the blocks' rows in block order (the res_norm.hip convention).  The
// sort is integer arithmetic only.  Every output element of the permute and
// combine kernels has exactly one writer (gather form).
//
// Packed fp32 VALU forms are off for every kernel of this file; a function
// with other target features is not inlined into them, so the few wave
// primitives used are written on the builtins here and not taken from the HIP
// headers or common.h.
#include "common.h"
#include "launchers.h"

namespace {

#if defined(__HIP_DEVICE_COMPILE__)  // the host pass does not know the feature
#define MOE_TARGET __attribute__((target("no-packed-fp32-ops")))
#else
#define MOE_TARGET
#endif
#define MOE_DEV __device__ __forceinline__ MOE_TARGET
#define MOE_KERNEL __global__ MOE_TARGET void __launch_bounds__(256)

constexpr int kThreads = 256;  // 4 waves, all kernels of this file
constexpr int kWaves = kThreads / 64;
constexpr int kMaxE = 256;
constexpr int kNoExpert = 0x7fffffff;

MOE_DEV int tid_x() { return (int)__builtin_amdgcn_workitem_id_x(); }
MOE_DEV int bid_x() { return (int)__builtin_amdgcn_workgroup_id_x(); }

MOE_DEV void block_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_s_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

MOE_DEV int shfl_xor_i(int v, int lane, int mask) {
  return __builtin_amdgcn_ds_bpermute((lane ^ mask) << 2, v);
}
MOE_DEV float shfl_xor_f(float v, int lane, int mask) {
  return __builtin_bit_cast(
      float, shfl_xor_i(__builtin_bit_cast(int, v), lane, mask));
}
MOE_DEV int shfl_i(int v, int src) {
  return __builtin_amdgcn_ds_bpermute(src << 2, v);
}
MOE_DEV float shfl_f(float v, int src) {
  return __builtin_bit_cast(float, shfl_i(__builtin_bit_cast(int, v), src));
}

MOE_DEV float wave_sum(float v, int lane) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += shfl_xor_f(v, lane, off);
  return v;
}

MOE_DEV float elem_to_f(uint16_t h) {
  return __builtin_bit_cast(float, ((uint32_t)h) << 16);
}
MOE_DEV float elem_to_f(float x) { return x; }
MOE_DEV void elem_from_f(uint16_t& o, float x) {
  o = __builtin_bit_cast(uint16_t, (__bf16)x);
}
MOE_DEV void elem_from_f(float& o, float x) { o = x; }

// exp(d) for d <= 0 on the hardware exp2: t = d * log2(e) rounded, the
// rounding error of that product and the low part of log2(e) folded back in
// to first order.  An exact 0 for d = -inf.
MOE_DEV float exp_neg(float d) {
  const float kL = 1.4426950408889634f, kLlo = 1.9259629911266175e-8f;
  const float kLn2 = 0.6931471805599453f;
  const float t = d * kL;
  const float c = __builtin_fmaf(d, kL, -t) + d * kLlo;
  const float p = __builtin_amdgcn_exp2f(t);
  return t > -150.f ? __builtin_fmaf(p, c * kLn2, p) : 0.f;
}

// ---------------------------------------------------------------------------
// routing
// ---------------------------------------------------------------------------

// a row's logits into registers (a NaN counts as -inf, so that the k argmax
// rounds always see a total order and pick an expert below E), its max, and
// p = exp(x - max); returns sum(p) over the group
template <int G, int EPL>
MOE_DEV float load_softmax(const float* __restrict__ logits, int64_t i, bool tok,
                           int E, int gl, int lane, float (&x)[EPL],
                           float (&p)[EPL], float& mx) {
  const float ninf = -__builtin_inff();
  mx = ninf;
#pragma unroll
  for (int m = 0; m < EPL; ++m) {
    const int e = gl + m * G;
    float v = ninf;
    if (tok && e < E) v = logits[i * E + e];
    x[m] = v == v ? v : ninf;
    mx = __builtin_fmaxf(mx, x[m]);
  }
#pragma unroll
  for (int off = G / 2; off > 0; off >>= 1)
    mx = __builtin_fmaxf(mx, shfl_xor_f(mx, lane, off));
  float sum = 0.f;
#pragma unroll
  for (int m = 0; m < EPL; ++m) {
    p[m] = (gl + m * G < E) ? exp_neg(x[m] - mx) : 0.f;
    sum += p[m];
  }
#pragma unroll
  for (int off = G / 2; off > 0; off >>= 1) sum += shfl_xor_f(sum, lane, off);
  return sum;
}

template <int G, int EPL>
MOE_KERNEL moe_route_kernel(const float* __restrict__ logits,
                            float* __restrict__ gates, int* __restrict__ idx,
                            int* __restrict__ hist, float* __restrict__ psum_part,
                            int n, int E, int k, int tpb) {
  constexpr int TPW = 64 / G;  // tokens per wave and pass
  __shared__ float s_p[kWaves][EPL * G];
  __shared__ int s_h[kWaves][EPL * G];
  const int tid = tid_x(), lane = tid & 63, wave = tid >> 6;
  const int gl = lane & (G - 1), grp = lane / G;
  const int t0 = bid_x() * tpb;
  const int t1 = t0 + tpb < n ? t0 + tpb : n;
  const float ninf = -__builtin_inff();

  float pacc[EPL];
  int hacc[EPL];
#pragma unroll
  for (int m = 0; m < EPL; ++m) {
    pacc[m] = 0.f;
    hacc[m] = 0;
  }

  for (int tb = t0 + wave * TPW; tb < t1; tb += kWaves * TPW) {  // wave-uniform
    const int i = tb + grp;
    const bool tok = i < t1;
    float x[EPL], p[EPL], mx;
    const float sum = load_softmax<G, EPL>(logits, i, tok, E, gl, lane, x, p, mx);
    if (tok) {
#pragma unroll
      for (int m = 0; m < EPL; ++m) pacc[m] += p[m] / sum;
    }

    // k argmax rounds over the experts not taken yet: larger logit first, the
    // lower index on an exact tie.  (cv, ci) is uniform in the group after
    // the reduction; lane j of the group keeps the j-th choice.
    uint32_t taken = 0;
    float myv = 0.f, den = 0.f;
    int myi = 0;
    for (int j = 0; j < k; ++j) {
      float cv = ninf;
      int ci = kNoExpert;
#pragma unroll
      for (int m = 0; m < EPL; ++m) {
        const int e = gl + m * G;
        if (e < E && !((taken >> m) & 1u) && (ci == kNoExpert || x[m] > cv)) {
          cv = x[m];
          ci = e;
        }
      }
#pragma unroll
      for (int off = G / 2; off > 0; off >>= 1) {
        const float ov = shfl_xor_f(cv, lane, off);
        const int oi = shfl_xor_i(ci, lane, off);
        if (ov > cv || (ov == cv && oi < ci)) {
          cv = ov;
          ci = oi;
        }
      }
#pragma unroll
      for (int m = 0; m < EPL; ++m) {
        if (gl + m * G == ci) {
          taken |= 1u << m;
          if (tok) hacc[m] += 1;
        }
      }
      if (gl == j) {
        myv = cv;
        myi = ci;
      }
      den += exp_neg(cv - mx);
    }
    if (tok && gl < k) {
      gates[(int64_t)i * k + gl] = exp_neg(myv - mx) / den;
      idx[(int64_t)i * k + gl] = myi;
    }
  }

  // groups of the wave (lanes with equal gl), then the waves in wave order
#pragma unroll
  for (int m = 0; m < EPL; ++m) {
#pragma unroll
    for (int off = 32; off >= G; off >>= 1) {
      pacc[m] += shfl_xor_f(pacc[m], lane, off);
      hacc[m] += shfl_xor_i(hacc[m], lane, off);
    }
    if (grp == 0) {
      s_p[wave][gl + m * G] = pacc[m];
      s_h[wave][gl + m * G] = hacc[m];
    }
  }
  block_sync();
  if (tid < E) {
    float ps = s_p[0][tid];
    int h = s_h[0][tid];
#pragma unroll
    for (int w = 1; w < kWaves; ++w) {
      ps += s_p[w][tid];
      h += s_h[w][tid];
    }
    psum_part[(int64_t)bid_x() * E + tid] = ps;
    hist[(int64_t)bid_x() * E + tid] = h;
  }
}

// dlogits[i,e] = p_e * (dpsum_e - sum_e' p_e' dpsum_e')
//              + [e is the j-th choice] g_j * (dgates_j - sum_j' g_j' dgates_j')
template <int G, int EPL>
MOE_KERNEL moe_route_bwd_kernel(const float* __restrict__ logits,
                                const int* __restrict__ idx,
                                const float* __restrict__ gates,
                                const float* __restrict__ dgates,
                                const float* __restrict__ dpsum,
                                float* __restrict__ dlogits, int n, int E, int k,
                                int tpb) {
  constexpr int TPW = 64 / G;
  const int tid = tid_x(), lane = tid & 63, wave = tid >> 6;
  const int gl = lane & (G - 1), grp = lane / G;
  const int t0 = bid_x() * tpb;
  const int t1 = t0 + tpb < n ? t0 + tpb : n;

  float dps[EPL];
#pragma unroll
  for (int m = 0; m < EPL; ++m) dps[m] = (gl + m * G < E) ? dpsum[gl + m * G] : 0.f;

  for (int tb = t0 + wave * TPW; tb < t1; tb += kWaves * TPW) {
    const int i = tb + grp;
    const bool tok = i < t1;
    float x[EPL], p[EPL], mx;
    const float sum = load_softmax<G, EPL>(logits, i, tok, E, gl, lane, x, p, mx);
    float s1 = 0.f;
#pragma unroll
    for (int m = 0; m < EPL; ++m) {
      p[m] = p[m] / sum;
      s1 += p[m] * dps[m];
    }
    float g = 0.f, dg = 0.f;
    int ie = kNoExpert;
    if (tok && gl < k) {
      g = gates[(int64_t)i * k + gl];
      dg = dgates[(int64_t)i * k + gl];
      ie = idx[(int64_t)i * k + gl];
    }
    float s2 = g * dg;
#pragma unroll
    for (int off = G / 2; off > 0; off >>= 1) {
      s1 += shfl_xor_f(s1, lane, off);
      s2 += shfl_xor_f(s2, lane, off);
    }
    float dl[EPL];
#pragma unroll
    for (int m = 0; m < EPL; ++m) dl[m] = p[m] * (dps[m] - s1);
    const float mine = g * (dg - s2);
    for (int j = 0; j < k; ++j) {  // lane j of the group holds the j-th choice
      const int src = (lane & ~(G - 1)) + j;
      const int ej = shfl_i(ie, src);
      const float vj = shfl_f(mine, src);
#pragma unroll
      for (int m = 0; m < EPL; ++m)
        if (gl + m * G == ej) dl[m] += vj;
    }
    if (tok) {
#pragma unroll
      for (int m = 0; m < EPL; ++m)
        if (gl + m * G < E) dlogits[(int64_t)i * E + gl + m * G] = dl[m];
    }
  }
}

// One workgroup, thread e owns expert e.  Turns hist[b, e] in place into
// base[b, e] = expert_offset[e] + sum_{b' < b} hist[b', e] and folds the
// blocks' psum rows in block order.
MOE_KERNEL moe_scan_kernel(int* __restrict__ hist,
                           const float* __restrict__ psum_part,
                           int* __restrict__ counts, int* __restrict__ offsets,
                           float* __restrict__ psum, int nblocks, int E) {
  __shared__ int s_cnt[kMaxE];
  const int e = tid_x();
  int cnt = 0;
  if (e < E) {
#pragma unroll 8
    for (int b = 0; b < nblocks; ++b) cnt += hist[(int64_t)b * E + e];
    s_cnt[e] = cnt;
    counts[e] = cnt;
  }
  block_sync();
  if (e < E) {
    int off = 0;
    for (int q = 0; q < e; ++q) off += s_cnt[q];
    offsets[e] = off;
    if (e == E - 1) offsets[E] = off + cnt;
    float ps = 0.f;
#pragma unroll 8
    for (int b = 0; b < nblocks; ++b) {
      const int h = hist[(int64_t)b * E + e];
      hist[(int64_t)b * E + e] = off;
      off += h;
      ps += psum_part[(int64_t)b * E + e];
    }
    psum[e] = ps;
  }
}

// Stable counting sort.  Lanes hold consecutive copies f; a copy's slot is
// base[block, e] + (copies of e earlier in the block) + (its rank among the
// copies of e in its wave).  The rank in the wave comes from ballots, one per
// distinct expert present; the earlier waves and passes from LDS counters.
MOE_KERNEL moe_plan_kernel(const int* __restrict__ idx, const int* __restrict__ base,
                           int* __restrict__ slot, int* __restrict__ row_of_slot,
                           int n, int E, int k, int tpb) {
  __shared__ int s_run[kMaxE];
  __shared__ int s_wcnt[kWaves][kMaxE];
  const int tid = tid_x(), lane = tid & 63, wave = tid >> 6;
  const int t0 = bid_x() * tpb;
  const int t1 = t0 + tpb < n ? t0 + tpb : n;
  const int f0 = t0 * k, f1 = t1 * k;  // n * k < 2^31 (checked by the binding)
  const uint64_t lt = (1ull << lane) - 1ull;

  s_run[tid] = tid < E ? base[(int64_t)bid_x() * E + tid] : 0;
#pragma unroll
  for (int w = 0; w < kWaves; ++w) s_wcnt[w][tid] = 0;
  block_sync();

  for (int fb = f0; fb < f1; fb += kThreads) {  // block-uniform
    const int f = fb + tid;
    int e = f < f1 ? idx[f] : -1;
    const bool valid = (unsigned)e < (unsigned)E;
    int rank = 0;
    uint64_t todo = __builtin_amdgcn_ballot_w64(valid);
    while (todo) {  // wave-uniform: one round per distinct expert present
      const int lead = __builtin_amdgcn_readfirstlane(__builtin_ctzll(todo));
      const int e0 = __builtin_amdgcn_readlane(e, lead);
      const uint64_t m = __builtin_amdgcn_ballot_w64(valid && e == e0);
      if (valid && e == e0) rank = __builtin_popcountll(m & lt);
      if (lane == lead) s_wcnt[wave][e0] = __builtin_popcountll(m);
      todo &= ~m;
    }
    block_sync();
    if (valid) {
      int s = s_run[e] + rank;
      for (int w = 0; w < wave; ++w) s += s_wcnt[w][e];
      slot[f] = s;
      row_of_slot[s] = f;
    }
    block_sync();
    if (tid < E) {
      int add = 0;
#pragma unroll
      for (int w = 0; w < kWaves; ++w) {
        add += s_wcnt[w][tid];
        s_wcnt[w][tid] = 0;
      }
      s_run[tid] += add;
    }
    block_sync();
  }
}

// ---------------------------------------------------------------------------
// dispatch and combine: one wave per row, 16-byte accesses, waves stride rows
// ---------------------------------------------------------------------------
template <class E>
MOE_KERNEL moe_permute_kernel(const typename E::T* __restrict__ x,
                              const int* __restrict__ row_of_slot,
                              typename E::T* __restrict__ xk, int nk, int k, int H,
                              int nwaves) {
  using VecT = typename E::VecT;
  constexpr int NV = 4;  // loads in flight per lane
  const int lane = tid_x() & 63;
  const int nvec = H / E::VEC;
  for (int s = bid_x() * kWaves + (tid_x() >> 6); s < nk; s += nwaves) {
    const VecT* src = (const VecT*)(x + (int64_t)(row_of_slot[s] / k) * H);
    VecT* dst = (VecT*)(xk + (int64_t)s * H);
    for (int c0 = lane; c0 < nvec; c0 += 64 * NV) {
      VecT v[NV];
#pragma unroll
      for (int q = 0; q < NV; ++q)
        if (c0 + q * 64 < nvec) v[q] = src[c0 + q * 64];
#pragma unroll
      for (int q = 0; q < NV; ++q)
        if (c0 + q * 64 < nvec) dst[c0 + q * 64] = v[q];
    }
  }
}

// K = compile-time bound of k (1, 2, 4, 8): the k row loads of a pass are all
// issued before the first product.  GATED = false sums the rows unweighted
// (the permute backward).
template <class E, int K, bool GATED>
MOE_KERNEL moe_combine_kernel(const typename E::T* __restrict__ yk,
                              const float* __restrict__ gates,
                              const int* __restrict__ slot,
                              const typename E::T* __restrict__ residual,
                              typename E::T* __restrict__ y, int n, int k, int H,
                              int nwaves) {
  using VecT = typename E::VecT;
  constexpr int V = E::VEC;
  const int lane = tid_x() & 63;
  const int nvec = H / V;
  for (int i = bid_x() * kWaves + (tid_x() >> 6); i < n; i += nwaves) {
    const VecT* rows[K];
    float g[K];
#pragma unroll
    for (int j = 0; j < K; ++j) {
      const bool on = j < k;
      rows[j] = (const VecT*)(yk + (int64_t)(on ? slot[(int64_t)i * k + j] : 0) * H);
      g[j] = on ? (GATED ? gates[(int64_t)i * k + j] : 1.f) : 0.f;
    }
    for (int c = lane; c < nvec; c += 64) {
      VecT v[K], r;
#pragma unroll
      for (int j = 0; j < K; ++j)
        if (j < k) v[j] = rows[j][c];
      if (residual != nullptr) r = ((const VecT*)(residual + (int64_t)i * H))[c];
      VecT o;
#pragma unroll
      for (int q = 0; q < V; ++q) {
        float acc = 0.f;
#pragma unroll
        for (int j = 0; j < K; ++j)
          if (j < k) acc = __builtin_fmaf(g[j], elem_to_f(v[j][q]), acc);
        if (residual != nullptr) acc += elem_to_f(r[q]);
        typename E::T t;
        elem_from_f(t, acc);
        o[q] = t;
      }
      ((VecT*)(y + (int64_t)i * H))[c] = o;
    }
  }
}

// one wave per slot s = copy (i, j): dyk[s] = gates[i,j] * dy[i] and
// dgates[i,j] = sum_h dy[i,h] * yk[s,h]
template <class E>
MOE_KERNEL moe_combine_bwd_kernel(const typename E::T* __restrict__ dy,
                                  const typename E::T* __restrict__ yk,
                                  const float* __restrict__ gates,
                                  const int* __restrict__ row_of_slot,
                                  typename E::T* __restrict__ dyk,
                                  float* __restrict__ dgates, int nk, int k, int H,
                                  int nwaves) {
  using VecT = typename E::VecT;
  constexpr int V = E::VEC;
  const int lane = tid_x() & 63;
  const int nvec = H / V;
  for (int s = bid_x() * kWaves + (tid_x() >> 6); s < nk; s += nwaves) {
    const int f = row_of_slot[s];
    const float g = gates[f];
    const VecT* dyr = (const VecT*)(dy + (int64_t)(f / k) * H);
    const VecT* ykr = (const VecT*)(yk + (int64_t)s * H);
    float dot = 0.f;
    for (int c = lane; c < nvec; c += 64) {
      const VecT a = dyr[c], b = ykr[c];
      VecT o;
#pragma unroll
      for (int q = 0; q < V; ++q) {
        const float d = elem_to_f(a[q]);
        dot = __builtin_fmaf(d, elem_to_f(b[q]), dot);
        typename E::T t;
        elem_from_f(t, g * d);
        o[q] = t;
      }
      ((VecT*)(dyk + (int64_t)s * H))[c] = o;
    }
    dot = wave_sum(dot, lane);
    if (lane == 0) dgates[f] = dot;
  }
}

// enough waves to fill the chip several times over, few enough that the row
// loop amortises the launch
inline int row_grid(int64_t rows) {
  int64_t g = CDIV(rows, (int64_t)kWaves);
  if (g > 16384) g = 16384;
  return (int)(g < 1 ? 1 : g);
}

// calls f(integral_constant<int, G>, integral_constant<int, EPL>) for E experts
template <class F>
void route_dispatch(int E, F&& f) {
#define ROUTE_CASE(G_, EPL_) \
  f(std::integral_constant<int, G_>{}, std::integral_constant<int, EPL_>{})
  if (E <= 4) ROUTE_CASE(4, 1);
  else if (E <= 8) ROUTE_CASE(8, 1);
  else if (E <= 16) ROUTE_CASE(16, 1);
  else if (E <= 32) ROUTE_CASE(32, 1);
  else if (E <= 64) ROUTE_CASE(64, 1);
  else if (E <= 128) ROUTE_CASE(64, 2);
  else if (E <= 192) ROUTE_CASE(64, 3);
  else ROUTE_CASE(64, 4);
#undef ROUTE_CASE
}

}  // namespace

// tokens per workgroup of the route, plan and route-backward kernels: whole
// waves of tokens at every group width, at most 512 workgroups (the scan
// kernel walks them serially)
extern "C" int moe_tokens_per_block(int64_t n) {
  const int64_t t = CDIV(CDIV(n, (int64_t)512), (int64_t)64) * 64;
  return (int)(t < 64 ? 64 : t);
}

// hist and psum_part are [nblocks, E] workspaces, nblocks = ceil(n / tpb);
// on return hist holds the per-block slot bases
extern "C" void moe_route_f32(const float* logits, float* gates, int* idx, int* hist,
                              float* psum_part, int* counts, int* offsets,
                              float* psum, int* slot, int* row_of_slot, int n, int E,
                              int k, hipStream_t stream) {
  const int tpb = moe_tokens_per_block(n);
  const int nblocks = (int)CDIV((int64_t)n, (int64_t)tpb);
  route_dispatch(E, [&](auto g, auto epl) {
    moe_route_kernel<decltype(g)::value, decltype(epl)::value>
        <<<dim3(nblocks), dim3(kThreads), 0, stream>>>(logits, gates, idx, hist,
                                                       psum_part, n, E, k, tpb);
  });
  moe_scan_kernel<<<dim3(1), dim3(kThreads), 0, stream>>>(hist, psum_part, counts,
                                                          offsets, psum, nblocks, E);
  moe_plan_kernel<<<dim3(nblocks), dim3(kThreads), 0, stream>>>(
      idx, hist, slot, row_of_slot, n, E, k, tpb);
}

extern "C" void moe_route_bwd_f32(const float* logits, const int* idx,
                                  const float* gates, const float* dgates,
                                  const float* dpsum, float* dlogits, int n, int E,
                                  int k, hipStream_t stream) {
  const int tpb = moe_tokens_per_block(n);
  const int nblocks = (int)CDIV((int64_t)n, (int64_t)tpb);
  route_dispatch(E, [&](auto g, auto epl) {
    moe_route_bwd_kernel<decltype(g)::value, decltype(epl)::value>
        <<<dim3(nblocks), dim3(kThreads), 0, stream>>>(logits, idx, gates, dgates,
                                                       dpsum, dlogits, n, E, k, tpb);
  });
}

template <class E, bool GATED>
static void launch_combine(const void* yk, const float* gates, const int* slot,
                           const void* residual, void* y, int n, int k, int H,
                           hipStream_t stream) {
  using T = typename E::T;
  const int g = row_grid(n);
#define COMBINE_K(K_)                                                          \
  moe_combine_kernel<E, K_, GATED><<<dim3(g), dim3(kThreads), 0, stream>>>(    \
      (const T*)yk, gates, slot, (const T*)residual, (T*)y, n, k, H, g * kWaves)
  if (k <= 1) COMBINE_K(1);
  else if (k <= 2) COMBINE_K(2);
  else if (k <= 4) COMBINE_K(4);
  else COMBINE_K(8);
#undef COMBINE_K
}

#define MOE_LAUNCHERS(SUFF, ETYPE)                                                   \
  extern "C" void moe_permute_##SUFF(const void* x, const int* row_of_slot,          \
                                     void* xk, int n, int k, int H,                  \
                                     hipStream_t stream) {                           \
    const int g = row_grid((int64_t)n * k);                                          \
    moe_permute_kernel<ETYPE><<<dim3(g), dim3(kThreads), 0, stream>>>(               \
        (const ETYPE::T*)x, row_of_slot, (ETYPE::T*)xk, n * k, k, H, g * kWaves);    \
  }                                                                                  \
  extern "C" void moe_combine_##SUFF(const void* yk, const float* gates,             \
                                     const int* slot, const void* residual, void* y, \
                                     int n, int k, int H, hipStream_t stream) {      \
    if (gates != nullptr)                                                            \
      launch_combine<ETYPE, true>(yk, gates, slot, residual, y, n, k, H, stream);    \
    else                                                                             \
      launch_combine<ETYPE, false>(yk, gates, slot, residual, y, n, k, H, stream);   \
  }                                                                                  \
  extern "C" void moe_combine_bwd_##SUFF(                                            \
      const void* dy, const void* yk, const float* gates, const int* row_of_slot,    \
      void* dyk, float* dgates, int n, int k, int H, hipStream_t stream) {           \
    const int g = row_grid((int64_t)n * k);                                          \
    moe_combine_bwd_kernel<ETYPE><<<dim3(g), dim3(kThreads), 0, stream>>>(           \
        (const ETYPE::T*)dy, (const ETYPE::T*)yk, gates, row_of_slot,                \
        (ETYPE::T*)dyk, dgates, n * k, k, H, g * kWaves);                            \
  }

MOE_LAUNCHERS(bf16, BF16Elem)
MOE_LAUNCHERS(f32, F32Elem)
