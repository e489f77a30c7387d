// sgiformer.hip -- kernels of the SGIFormer-v1m1 query decoder (pointcept/models/sgiformer/sgiformer_v1m1_base.py, loss.py):
//   a. ragged masked multi-head attention, forward and backward (head dim 32), for the four attentions of a decoder layer;
//   b. the bit-packed attention mask of forward_head (:372-378);
//   c. the Hungarian matcher's cost matrices (loss.py:15-52, :331-429) of every scene of a level in one launch;
//   d. prepare_target (:517-585): instance x superpoint counts, bit-packed ground-truth masks, instance classes.
//
// Attention.  One wave owns 16 query rows of one head and walks the keys of its scene 32 at a time with an online softmax; the dK / dV
// kernel mirrors it (16 keys, 32 queries at a time).  All products are v_mfma_f32_16x16x32_bf16 (head dim 32 = one contraction; one MFMA
// per product for bf16 rows, three on two-term bf16 operands for fp32 rows, see SgiFrag):
//   S^T = K Q^T          A = 16 key rows, B = 16 query rows, both read straight from memory (8 contiguous channels per lane);
//                        D[key][query] leaves query (lane & 15) in every lane: the softmax statistics are per lane + two shuffles.
//   O^T = V^T P^T        B = P^T is the S^T accumulator as it stands: the contraction index of lane group g, element m is DEFINED as
//                        key 16 (m / 4) + 4 g + (m % 4), which is where the two S^T tiles left the probabilities; A = V^T gathers the
//                        same keys (one channel per lane, 16 consecutive channels per key across the lanes of a group).
// Nothing of size Lq x Lk exists in memory; the backward recomputes the probabilities from the stored row log-sum-exp.  dQ is reduced
// by the wave that owns the query rows, dK / dV by the wave that owns the key rows, each over its tiles in index order: no atomics,
// bit-reproducible.
#include "mma.h"
#include <math.h>

#define SGI_D 32
#define SGI_LOG2E 1.4426950408889634f
#define SGI_LN2 0.6931471805599453f
#define SGI_LARGE 1e6f

// ------------------------------------------------------------------------------------------------ operand loads
__device__ __forceinline__ s16x8 sgi_pack8(const float* f) {
  uint32_t w[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) w[i] = ptc_pack_bf16x2(f[2 * i], f[2 * i + 1]);
  s16x8 r;
  __builtin_memcpy(&r, w, sizeof(r));
  return r;
}

// One MFMA operand.  bf16 rows: the 8 values as they are.  fp32 rows: every value as TWO bf16 terms, hi = bf16(x) and lo = bf16(x - hi),
// and every product as three MFMAs (lo hi + hi lo + hi hi; lo lo is below 2^-16 of the product): bf16 MFMA operands with an operand
// error of 2^-17 instead of 2^-9, which is what lets an fp32 model on these kernels reproduce an fp32 reference.
template <bool SPLIT> struct SgiFrag { s16x8 hi, lo; };

template <bool SPLIT>
__device__ __forceinline__ SgiFrag<SPLIT> sgi_split8(const float* f) {
  SgiFrag<SPLIT> r;
  r.hi = sgi_pack8(f);
  r.lo = r.hi;
  if constexpr (SPLIT) {
    float d[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) d[i] = f[i] - __uint_as_float(((uint32_t)(uint16_t)r.hi[i]) << 16);
    r.lo = sgi_pack8(d);
  }
  return r;
}

template <bool SPLIT>
__device__ __forceinline__ f32x4 sgi_mma(const SgiFrag<SPLIT>& a, const SgiFrag<SPLIT>& b, f32x4 c) {
  if constexpr (SPLIT) {
    c = Mma<bf16_t>::mma(a.lo, b.hi, c);
    c = Mma<bf16_t>::mma(a.hi, b.lo, c);
  }
  return Mma<bf16_t>::mma(a.hi, b.hi, c);
}

// 8 consecutive channels of one row (zeros when the row does not exist)
__device__ __forceinline__ SgiFrag<true> sgi_ld8(const float* p, bool ok) {
  float f[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  if (ok) {
    const float4 a = *reinterpret_cast<const float4*>(p), b = *reinterpret_cast<const float4*>(p + 4);
    f[0] = a.x; f[1] = a.y; f[2] = a.z; f[3] = a.w; f[4] = b.x; f[5] = b.y; f[6] = b.z; f[7] = b.w;
  }
  return sgi_split8<true>(f);
}
__device__ __forceinline__ SgiFrag<false> sgi_ld8(const bf16_t* p, bool ok) {
  uint4 v = make_uint4(0u, 0u, 0u, 0u);
  if (ok) v = *reinterpret_cast<const uint4*>(p);
  SgiFrag<false> r;
  __builtin_memcpy(&r.hi, &v, sizeof(r.hi));
  r.lo = r.hi;
  return r;
}

// channel `ch` of the 8 rows  row0 + 16 (m / 4) + 4 g + (m % 4),  m = 0..7  (the contraction order of the second product); rows at or
// past `len` read as zero.  `base` points at channel 0 of local row 0 of this head; `ld` = elements between rows.
template <typename T>
__device__ __forceinline__ SgiFrag<std::is_same<T, float>::value> sgi_gather8(const T* base, size_t ld, int row0, int g, int len, int ch) {
  float f[8];
#pragma unroll
  for (int m = 0; m < 8; ++m) {
    const int row = row0 + 16 * (m >> 2) + 4 * g + (m & 3);
    f[m] = row < len ? ptc_to_float(base[(size_t)row * ld + ch]) : 0.f;
  }
  return sgi_split8<std::is_same<T, float>::value>(f);
}

// block -> (scene, tile of `rows` rows) over a ragged batch; false past the last tile
__device__ __forceinline__ bool sgi_find_tile(const int* cu, int S, int rows, int tile, int& s, int& r0, int& len, int& t) {
  for (s = 0; s < S; ++s) {
    r0 = cu[s];
    len = cu[s + 1] - r0;
    const int nt = (len + rows - 1) / rows;
    if (tile < nt) { t = tile; return true; }
    tile -= nt;
  }
  return false;
}

// ------------------------------------------------------------------------------------------------ a. attention forward
template <typename T>
__global__ __launch_bounds__(64) void sgi_attn_fwd_kernel(const T* __restrict__ q, const T* __restrict__ k, const T* __restrict__ v,
                                                          const int* __restrict__ cu_q, const int* __restrict__ cu_k, int S, int H,
                                                          const uint32_t* __restrict__ mask, const int64_t* __restrict__ mask_row_off,
                                                          float scale, T* __restrict__ out, float* __restrict__ lse) {
  int s, q0, Lq, tile;
  if (!sgi_find_tile(cu_q, S, 16, (int)blockIdx.x, s, q0, Lq, tile)) return;
  const int h = blockIdx.y, lane = threadIdx.x & 63, j = lane & 15, g = lane >> 4;
  const int k0 = cu_k[s], Lk = cu_k[s + 1] - k0;
  const size_t ld = (size_t)H * SGI_D;
  const int qrow = tile * 16 + j;
  const bool qok = qrow < Lq;
  const auto qf = sgi_ld8(q + (size_t)(q0 + qrow) * ld + h * SGI_D + 8 * g, qok);
  const uint32_t* mrow = (mask && qok) ? mask + mask_row_off[s] + (int64_t)qrow * ((Lk + 31) >> 5) : nullptr;
  const T* kbase = k + (size_t)k0 * ld + h * SGI_D;
  const T* vbase = v + (size_t)k0 * ld + h * SGI_D;
  const float sl2 = scale * SGI_LOG2E;
  const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
  float m = -INFINITY, l = 0.f;
  f32x4 o0 = zero, o1 = zero;
  for (int kb = 0; kb < Lk; kb += 32) {
    f32x4 st[2];
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      const int key = kb + 16 * t + j;
      const auto kf = sgi_ld8(kbase + (size_t)key * ld + 8 * g, key < Lk);
      st[t] = sgi_mma(kf, qf, zero);
    }
    const uint32_t w = mrow ? mrow[kb >> 5] : 0u;
    float p[8], mx = m;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int bit = 16 * (i >> 2) + 4 * g + (i & 3);
      const bool dead = kb + bit >= Lk || ((w >> bit) & 1u);
      p[i] = dead ? -INFINITY : st[i >> 2][i & 3] * sl2;
      mx = fmaxf(mx, p[i]);
    }
    mx = fmaxf(mx, __shfl_xor(mx, 16));
    mx = fmaxf(mx, __shfl_xor(mx, 32));
    const float ms = mx == -INFINITY ? 0.f : mx;        // nothing open so far: every exponent below is 2^-inf = 0
    const float alpha = exp2f(m - ms);
    float rs = 0.f;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      p[i] = exp2f(p[i] - ms);
      rs += p[i];
    }
    rs += __shfl_xor(rs, 16);
    rs += __shfl_xor(rs, 32);
    l = l * alpha + rs;
    m = mx;
    const auto pf = sgi_split8<std::is_same<T, float>::value>(p);
    o0 *= alpha;
    o1 *= alpha;
    o0 = sgi_mma(sgi_gather8(vbase, ld, kb, g, Lk, j), pf, o0);
    o1 = sgi_mma(sgi_gather8(vbase, ld, kb, g, Lk, j + 16), pf, o1);
  }
  if (!qok) return;
  const float inv = l > 0.f ? 1.f / l : 0.f;
  T* orow = out + (size_t)(q0 + qrow) * ld + h * SGI_D + 4 * g;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    orow[e] = ptc_from_float<T>(o0[e] * inv);
    orow[16 + e] = ptc_from_float<T>(o1[e] * inv);
  }
  if (g == 0) lse[(size_t)(q0 + qrow) * H + h] = l > 0.f ? (m + log2f(l)) * SGI_LN2 : -INFINITY;
}

// ------------------------------------------------------------------------------------------------ a. attention backward
// delta [Tq, H] = sum_d dO O
template <typename T>
__global__ void sgi_attn_delta_kernel(const T* __restrict__ o, const T* __restrict__ dout, int64_t rows, float* __restrict__ delta) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= rows) return;
  const T* a = o + i * SGI_D;
  const T* b = dout + i * SGI_D;
  float acc = 0.f;
#pragma unroll
  for (int d = 0; d < SGI_D; ++d) acc = fmaf(ptc_to_float(a[d]), ptc_to_float(b[d]), acc);
  delta[i] = acc;
}

// dQ: the forward's walk.  dS^T = P^T (dP^T - delta), dP^T = V dO^T;  dQ^T = K^T dS^T.
template <typename T>
__global__ __launch_bounds__(64) void sgi_attn_dq_kernel(const T* __restrict__ q, const T* __restrict__ k, const T* __restrict__ v,
                                                         const T* __restrict__ dout, const float* __restrict__ lse,
                                                         const float* __restrict__ delta, const int* __restrict__ cu_q,
                                                         const int* __restrict__ cu_k, int S, int H, const uint32_t* __restrict__ mask,
                                                         const int64_t* __restrict__ mask_row_off, float scale, T* __restrict__ dq) {
  int s, q0, Lq, tile;
  if (!sgi_find_tile(cu_q, S, 16, (int)blockIdx.x, s, q0, Lq, tile)) return;
  const int h = blockIdx.y, lane = threadIdx.x & 63, j = lane & 15, g = lane >> 4;
  const int k0 = cu_k[s], Lk = cu_k[s + 1] - k0;
  const size_t ld = (size_t)H * SGI_D;
  const int qrow = tile * 16 + j;
  const bool qok = qrow < Lq;
  const size_t qoff = (size_t)(q0 + qrow) * ld + h * SGI_D + 8 * g;
  const auto qf = sgi_ld8(q + qoff, qok);
  const auto dof = sgi_ld8(dout + qoff, qok);
  const float lse2 = qok ? lse[(size_t)(q0 + qrow) * H + h] * SGI_LOG2E : 0.f;
  const float dl = qok ? delta[(size_t)(q0 + qrow) * H + h] : 0.f;
  const bool live = qok && lse2 != -INFINITY;
  const uint32_t* mrow = (mask && qok) ? mask + mask_row_off[s] + (int64_t)qrow * ((Lk + 31) >> 5) : nullptr;
  const T* kbase = k + (size_t)k0 * ld + h * SGI_D;
  const T* vbase = v + (size_t)k0 * ld + h * SGI_D;
  const float sl2 = scale * SGI_LOG2E;
  const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
  f32x4 a0 = zero, a1 = zero;
  for (int kb = 0; kb < Lk; kb += 32) {
    f32x4 st[2], dp[2];
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      const int key = kb + 16 * t + j;
      st[t] = sgi_mma(sgi_ld8(kbase + (size_t)key * ld + 8 * g, key < Lk), qf, zero);
      dp[t] = sgi_mma(sgi_ld8(vbase + (size_t)key * ld + 8 * g, key < Lk), dof, zero);
    }
    const uint32_t w = mrow ? mrow[kb >> 5] : 0u;
    float ds[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int bit = 16 * (i >> 2) + 4 * g + (i & 3);
      const bool dead = !live || kb + bit >= Lk || ((w >> bit) & 1u);
      const float p = dead ? 0.f : exp2f(st[i >> 2][i & 3] * sl2 - lse2);
      ds[i] = p * (dp[i >> 2][i & 3] - dl);
    }
    const auto dsf = sgi_split8<std::is_same<T, float>::value>(ds);
    a0 = sgi_mma(sgi_gather8(kbase, ld, kb, g, Lk, j), dsf, a0);
    a1 = sgi_mma(sgi_gather8(kbase, ld, kb, g, Lk, j + 16), dsf, a1);
  }
  if (!qok) return;
  T* row = dq + (size_t)(q0 + qrow) * ld + h * SGI_D + 4 * g;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    row[e] = ptc_from_float<T>(a0[e] * scale);
    row[16 + e] = ptc_from_float<T>(a1[e] * scale);
  }
}

// dK, dV: 16 keys per wave, the queries of the scene 32 at a time in index order.  S = Q K^T leaves key (lane & 15) in every lane;
// dV^T = dO^T P, dK^T = Q^T dS with the queries in the contraction order of sgi_gather8.
template <typename T>
__global__ __launch_bounds__(64) void sgi_attn_dkv_kernel(const T* __restrict__ q, const T* __restrict__ k, const T* __restrict__ v,
                                                          const T* __restrict__ dout, const float* __restrict__ lse,
                                                          const float* __restrict__ delta, const int* __restrict__ cu_q,
                                                          const int* __restrict__ cu_k, int S, int H, const uint32_t* __restrict__ mask,
                                                          const int64_t* __restrict__ mask_row_off, float scale, T* __restrict__ dk,
                                                          T* __restrict__ dv) {
  int s, k0, Lk, tile;
  if (!sgi_find_tile(cu_k, S, 16, (int)blockIdx.x, s, k0, Lk, tile)) return;
  const int h = blockIdx.y, lane = threadIdx.x & 63, j = lane & 15, g = lane >> 4;
  const int q0 = cu_q[s], Lq = cu_q[s + 1] - q0;
  const size_t ld = (size_t)H * SGI_D;
  const int key = tile * 16 + j;
  const bool kok = key < Lk;
  const size_t koff = (size_t)(k0 + key) * ld + h * SGI_D + 8 * g;
  const auto kf = sgi_ld8(k + koff, kok);
  const auto vf = sgi_ld8(v + koff, kok);
  const int W = (Lk + 31) >> 5;
  const uint32_t* mcol = (mask && kok) ? mask + mask_row_off[s] + (key >> 5) : nullptr;
  const T* qbase = q + (size_t)q0 * ld + h * SGI_D;
  const T* dobase = dout + (size_t)q0 * ld + h * SGI_D;
  const float* lbase = lse + (size_t)q0 * H + h;
  const float* dbase = delta + (size_t)q0 * H + h;
  const float sl2 = scale * SGI_LOG2E;
  const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
  f32x4 dk0 = zero, dk1 = zero, dv0 = zero, dv1 = zero;
  for (int qb = 0; qb < Lq; qb += 32) {
    f32x4 st[2], dp[2];
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      const int qi = qb + 16 * t + j;
      st[t] = sgi_mma(sgi_ld8(qbase + (size_t)qi * ld + 8 * g, qi < Lq), kf, zero);
      dp[t] = sgi_mma(sgi_ld8(dobase + (size_t)qi * ld + 8 * g, qi < Lq), vf, zero);
    }
    float p[8], ds[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int qi = qb + 16 * (i >> 2) + 4 * g + (i & 3);
      bool dead = !kok || qi >= Lq;
      float lse2 = 0.f, dl = 0.f;
      if (!dead) {
        lse2 = lbase[(size_t)qi * H] * SGI_LOG2E;
        dl = dbase[(size_t)qi * H];
        if (mcol) dead = (mcol[(size_t)qi * W] >> (key & 31)) & 1u;
        dead = dead || lse2 == -INFINITY;
      }
      p[i] = dead ? 0.f : exp2f(st[i >> 2][i & 3] * sl2 - lse2);
      ds[i] = p[i] * (dp[i >> 2][i & 3] - dl);
    }
    const auto pf = sgi_split8<std::is_same<T, float>::value>(p), dsf = sgi_split8<std::is_same<T, float>::value>(ds);
    dv0 = sgi_mma(sgi_gather8(dobase, ld, qb, g, Lq, j), pf, dv0);
    dv1 = sgi_mma(sgi_gather8(dobase, ld, qb, g, Lq, j + 16), pf, dv1);
    dk0 = sgi_mma(sgi_gather8(qbase, ld, qb, g, Lq, j), dsf, dk0);
    dk1 = sgi_mma(sgi_gather8(qbase, ld, qb, g, Lq, j + 16), dsf, dk1);
  }
  if (!kok) return;
  T* krow = dk + (size_t)(k0 + key) * ld + h * SGI_D + 4 * g;
  T* vrow = dv + (size_t)(k0 + key) * ld + h * SGI_D + 4 * g;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    krow[e] = ptc_from_float<T>(dk0[e] * scale);
    krow[16 + e] = ptc_from_float<T>(dk1[e] * scale);
    vrow[e] = ptc_from_float<T>(dv0[e]);
    vrow[16 + e] = ptc_from_float<T>(dv1[e]);
  }
}

// ------------------------------------------------------------------------------------------------ b. mask bit-pack
// One wave per query row: bit c of the row = sigmoid(x_c) < 0.5 (the reference's expression, not x_c < 0: sigmoid rounds to exactly
// 0.5 for tiny negative x), and a row whose bits would all be set is cleared.  Bits past M in the last word are written as zero.
__device__ __forceinline__ bool sgi_masked(float x) { return 1.f / (1.f + expf(-x)) < 0.5f; }

__global__ __launch_bounds__(64) void sgi_pack_mask_kernel(const float* __restrict__ logits, const int64_t* __restrict__ logit_off,
                                                           const int* __restrict__ cu_q, const int* __restrict__ cu_k, int S,
                                                           const int64_t* __restrict__ mask_row_off, uint32_t* __restrict__ words) {
  int s, q0, Lq, r;
  if (!sgi_find_tile(cu_q, S, 1, (int)blockIdx.x, s, q0, Lq, r)) return;
  const int lane = threadIdx.x & 63;
  const int M = cu_k[s + 1] - cu_k[s];
  const int W = (M + 31) >> 5;
  const float* x = logits + logit_off[s] + (int64_t)r * M;
  uint32_t* out = words + mask_row_off[s] + (int64_t)r * W;
  bool full = true;
  for (int c0 = 0; c0 < M; c0 += 64) {
    const int c = c0 + lane;
    const unsigned long long b = __ballot(c < M && sgi_masked(x[c < M ? c : 0]));
    const int n = M - c0 < 64 ? M - c0 : 64;
    const unsigned long long valid = n == 64 ? ~0ull : ((1ull << n) - 1ull);
    full = full && b == valid;
  }
  for (int c0 = 0; c0 < M; c0 += 64) {
    const int c = c0 + lane;
    const unsigned long long b = __ballot(c < M && sgi_masked(x[c < M ? c : 0]));
    if (lane < 2 && (c0 >> 5) + lane < W) out[(c0 >> 5) + lane] = full ? 0u : (uint32_t)(b >> (32 * lane));
  }
}

// ------------------------------------------------------------------------------------------------ c. matcher cost
// One wave per query row of a scene with instances.  softplus(-x) = softplus(x) - x, so
//   BCE(q, g)  = (sum_c softplus(x_c) - sum_{c in g} x_c) / M
//   dice(q, g) = 1 - (2 sum_{c in g} sigmoid(x_c) + 1) / (sum_c sigmoid(x_c) + |g| + 1)
// need the row sums once and, per instance, sums over its set bits only.  fp32 in and out, the sums and the transcendental functions in
// double (the reference's fp32 expression is the less exact of the two).  A row with a non-finite logit, and any non-finite entry,
// becomes 1e6 (loss.py:421-429: inf * 0 in the reference's einsum makes such a row NaN throughout).
__device__ __forceinline__ double sgi_wave_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}
__device__ __forceinline__ double sgi_wave_max(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o));
  return v;
}
__device__ __forceinline__ double sgi_softplus(double x) { return fmax(x, 0.0) + log1p(exp(-fabs(x))); }
__device__ __forceinline__ double sgi_sigmoid(double x) { return 1.0 / (1.0 + exp(-x)); }

__global__ __launch_bounds__(64) void sgi_match_cost_kernel(const float* __restrict__ logits, const int64_t* __restrict__ logit_off,
                                                            const float* __restrict__ cls, int C, const int* __restrict__ cu_q,
                                                            const int* __restrict__ cu_k, const int* __restrict__ cu_g, int S,
                                                            const uint32_t* __restrict__ gt_words, const int64_t* __restrict__ gt_word_off,
                                                            const int64_t* __restrict__ gt_cls, const int64_t* __restrict__ cost_off,
                                                            float w_cls, float w_bce, float w_dice, float* __restrict__ cost) {
  int s, q0, Lq, r;
  if (!sgi_find_tile(cu_q, S, 1, (int)blockIdx.x, s, q0, Lq, r)) return;
  const int g0 = cu_g[s], G = cu_g[s + 1] - g0;
  if (G <= 0) return;
  const int lane = threadIdx.x & 63;
  const int M = cu_k[s + 1] - cu_k[s];
  const int W = (M + 31) >> 5;
  const float* x = logits + logit_off[s] + (int64_t)r * M;
  const float* crow = cls + (size_t)(q0 + r) * C;
  double sp = 0.0, sg = 0.0;
  int bad = 0;
  for (int c = lane; c < M; c += 64) {
    const float xv = x[c];
    if (!isfinite(xv)) bad = 1;
    sp += sgi_softplus((double)xv);
    sg += sgi_sigmoid((double)xv);
  }
  bad = __ballot(bad) != 0ull;
  sp = sgi_wave_sum(sp);
  sg = sgi_wave_sum(sg);
  double cm = -INFINITY;
  for (int c = lane; c < C; c += 64) cm = fmax(cm, (double)crow[c]);
  cm = sgi_wave_max(cm);
  double ce = 0.0;
  for (int c = lane; c < C; c += 64) ce += exp((double)crow[c] - cm);
  ce = sgi_wave_sum(ce);
  float* orow = cost + cost_off[s] + (int64_t)r * G;
  for (int gi = lane; gi < G; gi += 64) {
    const uint32_t* gw = gt_words + gt_word_off[s] + (int64_t)gi * W;
    double sx = 0.0, ss = 0.0;
    int cnt = 0;
    for (int wi = 0; wi < W; ++wi) {
      uint32_t b = gw[wi];
      if (wi == W - 1 && (M & 31)) b &= (1u << (M & 31)) - 1u;
      cnt += __popc(b);
      while (b) {
        const int c = wi * 32 + (__ffs((int)b) - 1);
        b &= b - 1u;
        const double xv = bad ? 0.0 : (double)x[c];
        sx += xv;
        ss += sgi_sigmoid(xv);
      }
    }
    const int64_t gc = gt_cls[g0 + gi];
    float val = SGI_LARGE;
    if (!bad && gc >= 0 && gc < C) {
      const double c_cls = -exp((double)crow[gc] - cm) / ce;
      const double c_bce = (sp - sx) / (double)M;
      const double c_dice = 1.0 - (2.0 * ss + 1.0) / (sg + (double)cnt + 1.0);
      val = (float)((double)w_cls * c_cls + (double)w_bce * c_bce + (double)w_dice * c_dice);
      if (!isfinite(val)) val = SGI_LARGE;
    }
    orow[gi] = val;
  }
}

// ------------------------------------------------------------------------------------------------ d. targets
__global__ void sgi_fill_i64_kernel(int64_t* p, int64_t n, int64_t v) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) p[i] = v;
}

// one thread per point: superpoint sizes, instance x superpoint counts, instance class (integer atomics: order-free)
__global__ void sgi_target_count_kernel(const int64_t* __restrict__ instance, const int64_t* __restrict__ segment,
                                        const int64_t* __restrict__ sp_inverse, const int64_t* __restrict__ offset, int S, int64_t n,
                                        const int* __restrict__ cu_k, const int* __restrict__ cu_g, const int64_t* __restrict__ cnt_off,
                                        int* __restrict__ sp_size, int* __restrict__ counts, int64_t* __restrict__ inst_cls) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  int s = 0;
  while (s < S - 1 && i >= offset[s]) ++s;
  const int m0 = cu_k[s], M = cu_k[s + 1] - m0;
  const int64_t sp = sp_inverse[i] - m0;
  if (sp < 0 || sp >= M) return;
  atomicAdd(&sp_size[m0 + sp], 1);
  const int64_t inst = instance[i];
  const int G = cu_g[s + 1] - cu_g[s];
  if (inst < 0 || inst >= G) return;
  atomicAdd(&counts[cnt_off[s] + inst * M + sp], 1);
  atomicMax((long long*)&inst_cls[cu_g[s] + inst], (long long)segment[i]);
}

// one thread per mask word: bit = 2 count > superpoint size (the reference's mean > 0.5)
__global__ void sgi_target_pack_kernel(const int* __restrict__ sp_size, const int* __restrict__ counts, int S, const int* __restrict__ cu_k,
                                       const int64_t* __restrict__ cnt_off, const int64_t* __restrict__ word_off, int64_t total_words,
                                       uint32_t* __restrict__ words) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total_words) return;
  int s = 0;
  while (s < S - 1 && i >= word_off[s + 1]) ++s;
  const int m0 = cu_k[s], M = cu_k[s + 1] - m0;
  const int W = (M + 31) >> 5;
  const int64_t local = i - word_off[s];
  const int64_t gi = local / W;
  const int wi = (int)(local % W);
  const int* crow = counts + cnt_off[s] + gi * M;
  uint32_t b = 0u;
  for (int t = 0; t < 32 && wi * 32 + t < M; ++t) {
    const int c = wi * 32 + t;
    if (2 * crow[c] > sp_size[m0 + c]) b |= 1u << t;
  }
  words[i] = b;
}

// an instance id below the scene's maximum that no point carries: torch_scatter's max leaves 0 there
__global__ void sgi_target_cls_kernel(int64_t* inst_cls, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n && inst_cls[i] == INT64_MIN) inst_cls[i] = 0;
}

// ------------------------------------------------------------------------------------------------ entry points
extern "C" int ptc_sgi_attn_supported(int d) { return d == SGI_D; }

// fp32 or bf16 rows (sgi_attn_check has refused everything else)
#define SGI_DISPATCH(dtype, T, ...)                          \
  do {                                                       \
    if ((dtype) == PTC_F32) { using T = float; __VA_ARGS__; } \
    else { using T = bf16_t; __VA_ARGS__; }                   \
  } while (0)

static int sgi_attn_check(const char* what, int dtype, int s, int64_t tq, int64_t tk, int h, int d) {
  PTC_REQUIRE(d == SGI_D, PTC_EUNSUPPORTED, "%s: head dim %d (only %d)", what, d, SGI_D);
  PTC_REQUIRE(dtype == PTC_F32 || dtype == PTC_BF16, PTC_EUNSUPPORTED, "%s: dtype %d (fp32 or bf16)", what, dtype);
  PTC_REQUIRE(s >= 1 && tq >= 0 && tk >= 0 && h >= 1 && h <= 65535, PTC_EINVAL, "%s: s=%d tq=%lld tk=%lld h=%d", what, s, (long long)tq,
              (long long)tk, h);
  PTC_REQUIRE(tq < (1ll << 30) && tk < (1ll << 30), PTC_EUNSUPPORTED, "%s: more than 2^30 rows", what);
  return PTC_OK;
}

extern "C" size_t ptc_sgi_attn_workspace_bytes(int64_t tq, int h) { return tq > 0 && h > 0 ? (size_t)tq * h * 4 : 0; }

extern "C" int ptc_sgi_attn_fwd(const void* q, const void* k, const void* v, int dtype, const int32_t* cu_q, const int32_t* cu_k, int s,
                                int64_t tq, int64_t tk, int h, int d, const uint32_t* mask, const int64_t* mask_row_off, float scale, void* out,
                                float* lse, ptc_stream_t stream) {
  if (int rc = sgi_attn_check("ptc_sgi_attn_fwd", dtype, s, tq, tk, h, d)) return rc;
  if (tq == 0) return PTC_OK;
  PTC_REQUIRE(q && out && lse && cu_q && cu_k && ((k && v) || tk == 0), PTC_EINVAL, "ptc_sgi_attn_fwd: null buffer");
  PTC_REQUIRE(!mask || mask_row_off, PTC_EINVAL, "ptc_sgi_attn_fwd: a mask without row offsets");
  const dim3 grid((unsigned)(ptc_cdiv(tq, 16) + s), (unsigned)h);
  SGI_DISPATCH(dtype, T,
                     hipLaunchKernelGGL(sgi_attn_fwd_kernel<T>, grid, dim3(64), 0, (hipStream_t)stream, (const T*)q, (const T*)k, (const T*)v,
                                        cu_q, cu_k, s, h, mask, mask_row_off, scale, (T*)out, lse));
  PTC_CHECK_LAUNCH("sgi_attn_fwd_kernel");
  return PTC_OK;
}

extern "C" int ptc_sgi_attn_bwd(const void* q, const void* k, const void* v, const void* out, const void* dout, const float* lse, int dtype,
                                const int32_t* cu_q, const int32_t* cu_k, int s, int64_t tq, int64_t tk, int h, int d, const uint32_t* mask,
                                const int64_t* mask_row_off, float scale, void* dq, void* dk, void* dv, void* workspace, size_t workspace_bytes,
                                ptc_stream_t stream) {
  if (int rc = sgi_attn_check("ptc_sgi_attn_bwd", dtype, s, tq, tk, h, d)) return rc;
  PTC_REQUIRE(cu_q && cu_k, PTC_EINVAL, "ptc_sgi_attn_bwd: null offsets");
  PTC_REQUIRE(!mask || mask_row_off, PTC_EINVAL, "ptc_sgi_attn_bwd: a mask without row offsets");
  PTC_REQUIRE(workspace_bytes >= ptc_sgi_attn_workspace_bytes(tq, h), PTC_EWORKSPACE, "ptc_sgi_attn_bwd: workspace too small");
  hipStream_t st = (hipStream_t)stream;
  if (tq > 0) PTC_REQUIRE(q && out && dout && lse && dq && workspace && ((k && v) || tk == 0), PTC_EINVAL, "ptc_sgi_attn_bwd: null buffer");
  if (tk > 0) PTC_REQUIRE(k && v && dk && dv && ((q && dout && lse && workspace) || tq == 0), PTC_EINVAL, "ptc_sgi_attn_bwd: null buffer");
  float* delta = (float*)workspace;
  if (tq > 0) {
    const int64_t rows = tq * h;
    const dim3 grid((unsigned)(ptc_cdiv(tq, 16) + s), (unsigned)h);
    SGI_DISPATCH(dtype, T, {
      hipLaunchKernelGGL(sgi_attn_delta_kernel<T>, dim3((unsigned)ptc_cdiv(rows, 256)), dim3(256), 0, st, (const T*)out, (const T*)dout, rows,
                         delta);
      hipLaunchKernelGGL(sgi_attn_dq_kernel<T>, grid, dim3(64), 0, st, (const T*)q, (const T*)k, (const T*)v, (const T*)dout, lse, delta, cu_q,
                         cu_k, s, h, mask, mask_row_off, scale, (T*)dq);
    });
    PTC_CHECK_LAUNCH("sgi_attn_dq_kernel");
  }
  if (tk > 0) {
    const dim3 grid((unsigned)(ptc_cdiv(tk, 16) + s), (unsigned)h);
    SGI_DISPATCH(dtype, T,
                       hipLaunchKernelGGL(sgi_attn_dkv_kernel<T>, grid, dim3(64), 0, st, (const T*)q, (const T*)k, (const T*)v, (const T*)dout,
                                          lse, delta, cu_q, cu_k, s, h, mask, mask_row_off, scale, (T*)dk, (T*)dv));
    PTC_CHECK_LAUNCH("sgi_attn_dkv_kernel");
  }
  return PTC_OK;
}

extern "C" int ptc_sgi_pack_mask(const float* logits, const int64_t* logit_off, const int32_t* cu_q, const int32_t* cu_k, int s, int64_t tq,
                                 const int64_t* mask_row_off, uint32_t* words, ptc_stream_t stream) {
  PTC_REQUIRE(s >= 1 && tq >= 0 && tq < (1ll << 31) - 1, PTC_EINVAL, "ptc_sgi_pack_mask: s=%d tq=%lld", s, (long long)tq);
  if (tq == 0) return PTC_OK;
  PTC_REQUIRE(logit_off && cu_q && cu_k && mask_row_off, PTC_EINVAL, "ptc_sgi_pack_mask: null offsets");
  hipLaunchKernelGGL(sgi_pack_mask_kernel, dim3((unsigned)tq), dim3(64), 0, (hipStream_t)stream, logits, logit_off, cu_q, cu_k, s, mask_row_off,
                     words);
  PTC_CHECK_LAUNCH("sgi_pack_mask_kernel");
  return PTC_OK;
}

extern "C" int ptc_sgi_match_cost(const float* logits, const int64_t* logit_off, const float* cls, int c, const int32_t* cu_q,
                                  const int32_t* cu_k, const int32_t* cu_g, int s, int64_t tq, const uint32_t* gt_words,
                                  const int64_t* gt_word_off, const int64_t* gt_cls, const int64_t* cost_off, float w_cls, float w_bce,
                                  float w_dice, float* cost, ptc_stream_t stream) {
  PTC_REQUIRE(s >= 1 && tq >= 0 && tq < (1ll << 31) - 1 && c >= 1, PTC_EINVAL, "ptc_sgi_match_cost: s=%d tq=%lld c=%d", s, (long long)tq, c);
  if (tq == 0) return PTC_OK;
  PTC_REQUIRE(logit_off && cls && cu_q && cu_k && cu_g && gt_word_off && cost_off, PTC_EINVAL, "ptc_sgi_match_cost: null buffer");
  hipLaunchKernelGGL(sgi_match_cost_kernel, dim3((unsigned)tq), dim3(64), 0, (hipStream_t)stream, logits, logit_off, cls, c, cu_q, cu_k, cu_g, s,
                     gt_words, gt_word_off, gt_cls, cost_off, w_cls, w_bce, w_dice, cost);
  PTC_CHECK_LAUNCH("sgi_match_cost_kernel");
  return PTC_OK;
}

extern "C" int ptc_sgi_targets(const int64_t* instance, const int64_t* segment, const int64_t* sp_inverse, const int64_t* offset, int s,
                               int64_t n, const int32_t* cu_k, const int32_t* cu_g, const int64_t* cnt_off, const int64_t* word_off,
                               int64_t total_sp, int64_t total_inst, int64_t total_counts, int64_t total_words, int32_t* sp_size,
                               int32_t* counts, uint32_t* gt_words, int64_t* inst_cls, ptc_stream_t stream) {
  PTC_REQUIRE(s >= 1 && n >= 0 && total_sp >= 0 && total_inst >= 0 && total_counts >= 0 && total_words >= 0, PTC_EINVAL,
              "ptc_sgi_targets: s=%d n=%lld", s, (long long)n);
  PTC_REQUIRE(offset && cu_k && cu_g && cnt_off && word_off, PTC_EINVAL, "ptc_sgi_targets: null offsets");
  hipStream_t st = (hipStream_t)stream;
  if (total_sp > 0) PTC_HIP(hipMemsetAsync(sp_size, 0, (size_t)total_sp * 4, st));
  if (total_counts > 0) PTC_HIP(hipMemsetAsync(counts, 0, (size_t)total_counts * 4, st));
  if (total_inst > 0) {
    hipLaunchKernelGGL(sgi_fill_i64_kernel, dim3((unsigned)ptc_cdiv(total_inst, 256)), dim3(256), 0, st, inst_cls, total_inst, INT64_MIN);
    PTC_CHECK_LAUNCH("sgi_fill_i64_kernel");
  }
  if (n > 0) {
    PTC_REQUIRE(instance && segment && sp_inverse && sp_size, PTC_EINVAL, "ptc_sgi_targets: null buffer");
    hipLaunchKernelGGL(sgi_target_count_kernel, dim3((unsigned)ptc_cdiv(n, 256)), dim3(256), 0, st, instance, segment, sp_inverse, offset, s, n,
                       cu_k, cu_g, cnt_off, sp_size, counts, inst_cls);
    PTC_CHECK_LAUNCH("sgi_target_count_kernel");
  }
  if (total_words > 0) {
    hipLaunchKernelGGL(sgi_target_pack_kernel, dim3((unsigned)ptc_cdiv(total_words, 256)), dim3(256), 0, st, sp_size, counts, s, cu_k, cnt_off,
                       word_off, total_words, gt_words);
    PTC_CHECK_LAUNCH("sgi_target_pack_kernel");
  }
  if (total_inst > 0) {
    hipLaunchKernelGGL(sgi_target_cls_kernel, dim3((unsigned)ptc_cdiv(total_inst, 256)), dim3(256), 0, st, inst_cls, total_inst);
    PTC_CHECK_LAUNCH("sgi_target_cls_kernel");
  }
  return PTC_OK;
}
