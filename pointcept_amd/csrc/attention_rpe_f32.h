// attention_rpe_f32.h -- the RPE window attention of attention_rpe.h in fp32 arithmetic (included by attention.hip).
//
// The reference's dense branch without autocast (point_transformer_v3m1_base.py:190-206 on fp32 q / k / v): fp32 operands, logits, bias,
// softmax, accumulation and outputs; nothing is rounded to 16 bits.  Matrix products are v_mfma_f32_16x16x4_f32 (exact fp32 products,
// fp32 accumulate).  Layout of that instruction: A[i][k] in lane i + 16 k, B[k][j] in lane j + 16 k, D[i][j] in lane j + 16 (i / 4)
// element i % 4.  Everything is written so that a lane (j = lane & 15, g = lane >> 4) holds ONE row of the stationary side (query in the
// forward and dQ kernels, key in the dK/dV kernel) and the four other-side rows 4 g + r, r = 0..3, of a 16-row tile in its 4 elements:
//   * the head_dim-16 contraction is four MFMAs whose A / B operands are the float4 [4 g, 4 g + 4) of a row (k = g, element s), so a
//     stationary row is one float4 in registers and a streamed row is one ds_read_b128;
//   * the 16-row contraction of the second product (P V, dS K, ...) is four MFMAs, MFMA r pairing the streamed rows 4 k + r with the
//     lane's element r: the P / dS registers ARE the B operand, and the A operand is a column read (4 ds_read_b32) of the same
//     row-major image;
//   * the result lands as the float4 [4 g, 4 g + 4) of the lane's stationary row: one 16-byte store.
// Per-row softmax state lives replicated in the four lanes of a row (two xor shuffles per reduction).  Bias, tables, masking, the
// exp2-domain online softmax and the lse [H, T] output are those of attention_rpe.h (ar_pack / ar_bias / ar_stage).
//
// LDS (whole windows, one workgroup per CU; Lp = max_seqlen rounded up to 32, 1024 at most; R = 2 pos_bnd + 1 <= 65):
//   forward:  K [Lp][16] f32 64 KB | V [Lp][16] f32 64 KB | coords 8 KB | table 3R f32                    <= 137 KB
//   dQ:       K 64 KB | V 64 KB | coords 8 KB | table | d table 3R i64 | 8 floats                         <= 139 KB
//   dK / dV:  Q 64 KB | dO 64 KB | lse2 4 KB | delta 4 KB | coords 8 KB | table                           <= 145 KB
// of the 160 KB of a CU.  The four images of a backward (Q, dO, K, V: 256 KB) do not fit together, so the backward keeps the two-kernel
// split of the 16-bit kernels: each pass stages the two images it streams, and reads its stationary rows (one float4 each) from global
// memory (L2).
//
// Table gradient: d table[a R + idx][h] += dS[i][j] in 2^-44 FIXED POINT (resolution 5.7e-14: a 1e-9 addend keeps 4 1/2 digits, the
// sum of many keeps fp32 accuracy), 64-bit integer atomics in LDS per workgroup and one 64-bit global atomic per entry at the end, as
// the 16-bit kernels do at 2^-24 -- integer sums do not depend on the order of the additions, so the result is bit-reproducible.
// Range: +-2^19 = 5.2e5 per table entry.  Every partial sum of an entry is bounded by the head's sum of |dS| over all pairs, which
// the dQ pass accumulates alongside (per lane, per workgroup, one float atomic per workgroup and head); the conversion launch writes
// NaN to every entry of a head whose bound reaches 2^18 (a 2x margin over the fp32 rounding of the bound): out of range is a loud
// NaN in the gradient, never a silent wrap.

#include "mma.h"

#define AR32_FIX_SCALE 17592186044416.f   // 2^44
#define AR32_FIX_LIMIT 262144.f           // 2^18: largest head sum of |dS| converted (the int64 range is 2^63 / 2^44 = 2^19)

__device__ __forceinline__ f32x4 ar32_splat(float v) { return (f32x4){v, v, v, v}; }
// the float4 [4 g, 4 g + 4) of a 16-float row (zero when !valid)
__device__ __forceinline__ f32x4 ar32_ld(const float* __restrict__ row, int g, bool valid) {
  return valid ? *reinterpret_cast<const f32x4*>(row + 4 * g) : ar32_splat(0.f);
}
// stationary x streamed over head_dim 16: D[i][j] += sum_d A-row i [d] * B-row j [d] (both operands float4 [4 g, 4 g + 4) of a row)
__device__ __forceinline__ f32x4 ar32_dot16(f32x4 a, f32x4 b, f32x4 c) {
  c = ptc_mfma_f32_4(a[0], b[0], c);
  c = ptc_mfma_f32_4(a[1], b[1], c);
  c = ptc_mfma_f32_4(a[2], b[2], c);
  return ptc_mfma_f32_4(a[3], b[3], c);
}
// sum over the 16 streamed rows of a tile: D[ch][j] += sum_r img[base + 4 k + r][ch] * w[r]  (lane = ch + 16 k reads the column)
__device__ __forceinline__ f32x4 ar32_acc16(const float* img, int base, int lane, f32x4 w, f32x4 c) {
  const float* col = img + (size_t)(base + 4 * (lane >> 4)) * 16 + (lane & 15);
  c = ptc_mfma_f32_4(col[0], w[0], c);
  c = ptc_mfma_f32_4(col[16], w[1], c);
  c = ptc_mfma_f32_4(col[32], w[2], c);
  return ptc_mfma_f32_4(col[48], w[3], c);
}
// rows [0, Lp) of a [*, 16] fp32 source with the given row stride into a dense [Lp][16] image (zeros beyond L)
__device__ __forceinline__ void ar32_stage(const float* __restrict__ src, int64_t row_stride, int L, int Lp, float* img) {
  for (int i = threadIdx.x; i < Lp * 4; i += AR_THREADS) {
    const int row = i >> 2, part = i & 3;
    f32x4 v = ar32_splat(0.f);
    if (row < L) v = *reinterpret_cast<const f32x4*>(src + (int64_t)row * row_stride + 4 * part);
    *reinterpret_cast<f32x4*>(img + i * 4) = v;
  }
}
// NaN into rows [0, L) (16 floats each) and the side vector: a window longer than max_seqlen (see at_poison_rows)
__device__ __forceinline__ void ar32_poison_rows(float* rows, int64_t row_stride, int L, float* side) {
  const float nan = __uint_as_float(0x7FC00000u);
  for (int i = threadIdx.x; i < L * 4; i += AR_THREADS) {
    *reinterpret_cast<f32x4*>(rows + (int64_t)(i >> 2) * row_stride + 4 * (i & 3)) = ar32_splat(nan);
    if (side && (i & 3) == 0) side[i >> 2] = nan;
  }
}
static size_t ar32_fwd_lds(int lp_max, int R) { return (size_t)lp_max * 136 + (size_t)((3 * R + 3) & ~3) * 4; }
static size_t ar32_dq_lds(int lp_max, int R) { return (size_t)lp_max * 136 + (size_t)((3 * R + 3) & ~3) * 12 + 32; }
static size_t ar32_dkv_lds(int lp_max, int R) { return (size_t)lp_max * 144 + (size_t)((3 * R + 3) & ~3) * 4; }

// ------------------------------------------------------------------------------------------------ forward
// LDS: K | V | coords | table.  A wave owns 16-query tiles; per 32 keys: S^T = K (q c)^T (two independent 16-key products), bias,
// online softmax, O^T += V^T P^T (two accumulators).
__global__ void __launch_bounds__(AR_THREADS, 1)
attn_rpe_fwd_f32_kernel(const float* __restrict__ qkv, const int32_t* __restrict__ cu, const int32_t* __restrict__ gc,
                        const float* __restrict__ table, int R, int B, int H, float scale, int64_t total, int lp_max, int n_units,
                        float* __restrict__ out, float* __restrict__ lse) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int unit = at_unit(n_units);
  if (unit >= n_units) return;
  const int seq = unit / H, head = unit % H;
  const int a = cu[seq], L = cu[seq + 1] - a;
  if (L <= 0) return;
  const int Lp = (L + 31) & ~31;
  if (Lp > lp_max) {
    ar32_poison_rows(out + ((int64_t)a * H + head) * 16, (int64_t)H * 16, L, lse + (int64_t)head * total + a);
    return;
  }
  float* Ksm = reinterpret_cast<float*>(smem);
  float* Vsm = Ksm + (size_t)lp_max * 16;
  uint2* coords = reinterpret_cast<uint2*>(Vsm + (size_t)lp_max * 16);
  float* tl = reinterpret_cast<float*>(coords + lp_max);
  const int64_t rs = (int64_t)3 * H * 16;
  ar32_stage(qkv + qkv_off(a, 1, H, head), rs, L, Lp, Ksm);
  ar32_stage(qkv + qkv_off(a, 2, H, head), rs, L, Lp, Vsm);
  ar_stage(gc, a, L, Lp, table, H, head, R, coords, tl, nullptr);
  __syncthreads();

  const int lane = ptc_lane(), wave = threadIdx.x >> 6;
  const int j = lane & 15, g = lane >> 4;
  const float c = scale * AT_LOG2E;
  const float* tb = tl + B;
  for (int qt = wave; qt < (Lp >> 4); qt += AT_WAVES) {
    const int q = qt * 16 + j;
    const f32x4 qf = ar32_ld(qkv + qkv_off(a + q, 0, H, head), g, q < L) * c;
    const uint2 qc = coords[q];
    const int qx = (int)(qc.x & 0xffffu), qy = (int)(qc.x >> 16), qz = (int)qc.y;
    f32x4 acc0 = ar32_splat(0.f), acc1 = ar32_splat(0.f);
    float m = -INFINITY, l = 0.f;
    for (int kt = 0; kt < Lp; kt += 32) {
      f32x4 s[2];
      s[0] = ar32_dot16(*reinterpret_cast<const f32x4*>(Ksm + (size_t)(kt + j) * 16 + 4 * g), qf, ar32_splat(0.f));
      s[1] = ar32_dot16(*reinterpret_cast<const f32x4*>(Ksm + (size_t)(kt + 16 + j) * 16 + 4 * g), qf, ar32_splat(0.f));
      float mt = -INFINITY;
#pragma unroll
      for (int h = 0; h < 2; ++h)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int key = kt + 16 * h + 4 * g + r;
          int ix, iy, iz;
          s[h][r] += ar_bias(qx, qy, qz, coords[key], tb, R, B, ix, iy, iz);
          if (key >= L) s[h][r] = -INFINITY;
          mt = fmaxf(mt, s[h][r]);
        }
      mt = fmaxf(mt, __shfl_xor(mt, 16, 64));
      mt = fmaxf(mt, __shfl_xor(mt, 32, 64));
      const float m_new = fmaxf(m, mt);            // finite: key 0 of the first tile is valid
      const float alpha = __builtin_amdgcn_exp2f(m - m_new);
      m = m_new;
      acc0 *= alpha;
      acc1 *= alpha;
      l *= alpha;
      f32x4 p[2];
#pragma unroll
      for (int h = 0; h < 2; ++h)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          p[h][r] = __builtin_amdgcn_exp2f(s[h][r] - m);
          l += p[h][r];
        }
      acc0 = ar32_acc16(Vsm, kt, lane, p[0], acc0);
      acc1 = ar32_acc16(Vsm, kt + 16, lane, p[1], acc1);
    }
    l += __shfl_xor(l, 16, 64);
    l += __shfl_xor(l, 32, 64);
    if (q < L) {
      *reinterpret_cast<f32x4*>(out + ((int64_t)(a + q) * H + head) * 16 + 4 * g) = (acc0 + acc1) * (1.f / l);
      if (g == 0) lse[(int64_t)head * total + a + q] = m * AT_LN2 + __logf(l);
    }
  }
}

// ------------------------------------------------------------------------------------------------ backward: dQ, delta, d table
// LDS: K | V | coords | table | d table (i64) | 8 floats (sum of |dS| per wave).  A wave owns 16-query tiles; per 16 keys:
// S^T = K (q c)^T - lse2, dP^T = V dO^T - delta, dS = P dP, dQ^T += K^T dS^T.
__global__ void __launch_bounds__(AR_THREADS, 1)
attn_rpe_bwd_dq_f32_kernel(const float* __restrict__ qkv, const float* __restrict__ out, const float* __restrict__ dout,
                           const float* __restrict__ lse, const int32_t* __restrict__ cu, const int32_t* __restrict__ gc,
                           const float* __restrict__ table, int R, int B, int H, float scale, int64_t total, int lp_max, int n_units,
                           float* __restrict__ dqkv, float* __restrict__ delta, unsigned long long* __restrict__ dtable_fix,
                           float* __restrict__ abs_sum) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int unit = at_unit(n_units);
  if (unit >= n_units) return;
  const int seq = unit / H, head = unit % H;
  const int a = cu[seq], L = cu[seq + 1] - a;
  if (L <= 0) return;
  const int Lp = (L + 31) & ~31;
  if (Lp > lp_max) {
    ar32_poison_rows(dqkv + qkv_off(a, 0, H, head), (int64_t)3 * H * 16, L, nullptr);
    return;
  }
  float* Ksm = reinterpret_cast<float*>(smem);
  float* Vsm = Ksm + (size_t)lp_max * 16;
  uint2* coords = reinterpret_cast<uint2*>(Vsm + (size_t)lp_max * 16);
  float* tl = reinterpret_cast<float*>(coords + lp_max);
  unsigned long long* dtl = reinterpret_cast<unsigned long long*>(tl + ((3 * R + 3) & ~3));   // 16-byte aligned: lp_max * 136 + 16 k
  float* red = reinterpret_cast<float*>(dtl + ((3 * R + 3) & ~3));
  const int64_t rs = (int64_t)3 * H * 16;
  ar32_stage(qkv + qkv_off(a, 1, H, head), rs, L, Lp, Ksm);
  ar32_stage(qkv + qkv_off(a, 2, H, head), rs, L, Lp, Vsm);
  ar_stage(gc, a, L, Lp, table, H, head, R, coords, tl, dtl);
  __syncthreads();

  const int lane = ptc_lane(), wave = threadIdx.x >> 6;
  const int j = lane & 15, g = lane >> 4;
  const float c = scale * AT_LOG2E;
  const float* tb = tl + B;
  unsigned long long* dtb = dtl + B;
  float asum = 0.f;
  for (int qt = wave; qt < (Lp >> 4); qt += AT_WAVES) {
    const int q = qt * 16 + j;
    const bool qv = q < L;
    const f32x4 qf = ar32_ld(qkv + qkv_off(a + q, 0, H, head), g, qv) * c;
    const int64_t orow = ((int64_t)(a + q) * H + head) * 16;
    const f32x4 dof = ar32_ld(dout + orow, g, qv), of = ar32_ld(out + orow, g, qv);
    float dl = dof[0] * of[0] + dof[1] * of[1] + dof[2] * of[2] + dof[3] * of[3];
    dl += __shfl_xor(dl, 16, 64);
    dl += __shfl_xor(dl, 32, 64);
    const float l2 = qv ? lse[(int64_t)head * total + a + q] * AT_LOG2E : INFINITY;
    if (qv && g == 0) delta[(int64_t)head * total + a + q] = dl;
    const uint2 qc = coords[q];
    const int qx = (int)(qc.x & 0xffffu), qy = (int)(qc.x >> 16), qz = (int)qc.y;
    f32x4 acc0 = ar32_splat(0.f), acc1 = ar32_splat(0.f);
    for (int kt = 0; kt < Lp; kt += 16) {
      const f32x4 s = ar32_dot16(*reinterpret_cast<const f32x4*>(Ksm + (size_t)(kt + j) * 16 + 4 * g), qf, ar32_splat(-l2));
      const f32x4 dp = ar32_dot16(*reinterpret_cast<const f32x4*>(Vsm + (size_t)(kt + j) * 16 + 4 * g), dof, ar32_splat(-dl));
      f32x4 ds;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int key = kt + 4 * g + r;
        int ix, iy, iz;
        const float b = ar_bias(qx, qy, qz, coords[key], tb, R, B, ix, iy, iz);
        // keys >= L: k = 0 and v = 0 give a finite P; it must reach neither dQ nor the table gradient
        ds[r] = (qv && key < L) ? __builtin_amdgcn_exp2f(s[r] + b) * dp[r] : 0.f;
        asum += fabsf(ds[r]);
        const unsigned long long fx = (unsigned long long)__float2ll_rn(ds[r] * AR32_FIX_SCALE);   // |ds| < 2^18 while in range
        if (fx != 0ull) {
          atomicAdd(dtb + ix, fx);
          atomicAdd(dtb + iy, fx);
          atomicAdd(dtb + iz, fx);
        }
      }
      if ((kt & 16) == 0) acc0 = ar32_acc16(Ksm, kt, lane, ds, acc0);
      else acc1 = ar32_acc16(Ksm, kt, lane, ds, acc1);
    }
    if (qv) *reinterpret_cast<f32x4*>(dqkv + qkv_off(a + q, 0, H, head) + 4 * g) = (acc0 + acc1) * scale;
  }
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) asum += __shfl_xor(asum, o, 64);
  if (lane == 0) red[wave] = asum;
  __syncthreads();
  if (threadIdx.x == 0) {
    float t = 0.f;
    for (int w = 0; w < AT_WAVES; ++w) t += red[w];
    atomicAdd(abs_sum + head, t);
  }
  for (int i = threadIdx.x; i < 3 * R; i += AR_THREADS)
    if (dtl[i] != 0ull) atomicAdd(dtable_fix + (int64_t)i * H + head, dtl[i]);
}

__global__ void attn_rpe_table_finish_f32_kernel(const unsigned long long* __restrict__ fix, const float* __restrict__ abs_sum, int H,
                                                 int64_t n, float* __restrict__ dtable) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n)
    dtable[i] = abs_sum[i % H] < AR32_FIX_LIMIT ? (float)((double)(long long)fix[i] * (1.0 / (double)AR32_FIX_SCALE))
                                                : __uint_as_float(0x7FC00000u);
}

// ------------------------------------------------------------------------------------------------ backward: dK, dV
// LDS: Q | dO | lse2 | delta | coords | table.  A wave owns 16-key tiles; per 16 queries: S = Q (k c)^T - lse2, dP = dO v^T - delta,
// dS = P dP, dV^T += dO^T P, dK^T += Q^T dS.
__global__ void __launch_bounds__(AR_THREADS, 1)
attn_rpe_bwd_dkv_f32_kernel(const float* __restrict__ qkv, const float* __restrict__ dout, const float* __restrict__ lse,
                            const float* __restrict__ delta, const int32_t* __restrict__ cu, const int32_t* __restrict__ gc,
                            const float* __restrict__ table, int R, int B, int H, float scale, int64_t total, int lp_max, int n_units,
                            float* __restrict__ dqkv) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int unit = at_unit(n_units);
  if (unit >= n_units) return;
  const int seq = unit / H, head = unit % H;
  const int a = cu[seq], L = cu[seq + 1] - a;
  if (L <= 0) return;
  const int Lp = (L + 31) & ~31;
  if (Lp > lp_max) {
    ar32_poison_rows(dqkv + qkv_off(a, 1, H, head), (int64_t)3 * H * 16, L, nullptr);
    ar32_poison_rows(dqkv + qkv_off(a, 2, H, head), (int64_t)3 * H * 16, L, nullptr);
    return;
  }
  float* Qsm = reinterpret_cast<float*>(smem);
  float* dOsm = Qsm + (size_t)lp_max * 16;
  float* l2s = dOsm + (size_t)lp_max * 16;
  float* dls = l2s + lp_max;
  uint2* coords = reinterpret_cast<uint2*>(dls + lp_max);
  float* tl = reinterpret_cast<float*>(coords + lp_max);
  ar32_stage(qkv + qkv_off(a, 0, H, head), (int64_t)3 * H * 16, L, Lp, Qsm);
  ar32_stage(dout + ((int64_t)a * H + head) * 16, (int64_t)H * 16, L, Lp, dOsm);
  for (int q = threadIdx.x; q < Lp; q += AR_THREADS) {
    l2s[q] = q < L ? lse[(int64_t)head * total + a + q] * AT_LOG2E : AT_PAD_LSE;   // padding queries: exp2(s - 1e30) = 0
    dls[q] = q < L ? delta[(int64_t)head * total + a + q] : 0.f;
  }
  ar_stage(gc, a, L, Lp, table, H, head, R, coords, tl, nullptr);
  __syncthreads();

  const int lane = ptc_lane(), wave = threadIdx.x >> 6;
  const int j = lane & 15, g = lane >> 4;
  const float c = scale * AT_LOG2E;
  const float* tb = tl + B;
  for (int kt = wave; kt < (Lp >> 4); kt += AT_WAVES) {
    const int key = kt * 16 + j;
    const bool kv = key < L;
    const f32x4 kf = ar32_ld(qkv + qkv_off(a + key, 1, H, head), g, kv) * c;
    const f32x4 vf = ar32_ld(qkv + qkv_off(a + key, 2, H, head), g, kv);
    const uint2 kc = coords[key];
    f32x4 dv = ar32_splat(0.f), dk = ar32_splat(0.f);
    for (int qt = 0; qt < Lp; qt += 16) {
      const f32x4 nl2 = -*reinterpret_cast<const f32x4*>(l2s + qt + 4 * g);
      const f32x4 ndl = -*reinterpret_cast<const f32x4*>(dls + qt + 4 * g);
      const f32x4 s = ar32_dot16(*reinterpret_cast<const f32x4*>(Qsm + (size_t)(qt + j) * 16 + 4 * g), kf, nl2);
      const f32x4 dp = ar32_dot16(*reinterpret_cast<const f32x4*>(dOsm + (size_t)(qt + j) * 16 + 4 * g), vf, ndl);
      f32x4 p, ds;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const uint2 qc = coords[qt + 4 * g + r];                 // the QUERY of this element; the lane's key is kc
        int ix, iy, iz;
        const float b = ar_bias((int)(qc.x & 0xffffu), (int)(qc.x >> 16), (int)qc.y, kc, tb, R, B, ix, iy, iz);
        p[r] = __builtin_amdgcn_exp2f(s[r] + b);
        ds[r] = p[r] * dp[r];
      }
      dv = ar32_acc16(dOsm, qt, lane, p, dv);
      dk = ar32_acc16(Qsm, qt, lane, ds, dk);
    }
    if (kv) {
      *reinterpret_cast<f32x4*>(dqkv + qkv_off(a + key, 1, H, head) + 4 * g) = dk * scale;
      *reinterpret_cast<f32x4*>(dqkv + qkv_off(a + key, 2, H, head) + 4 * g) = dv;
    }
  }
}
