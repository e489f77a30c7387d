// cac.hip -- the context-aware classifier's own hot path (pointcept/models/context_aware_classifier/context_aware_classifier_v1m1_base.py,
// "CAC-v1m1"): weighted prototype pooling, the segmented cosine classifier and the distillation loss.  fp32, gfx950.
//
//  * ptc_cac_pool_{fwd,bwd}: proto[s, k, :] = sum_i w_ik x_i / (sum_i w_ik + eps) for the two weight sources of the file --
//    soft: softmax(logits_i) times the confidence gate, rows segmented by scene (post_refine_proto_batch, :98-150);
//    hard: onehot(target_i), one segment (get_adaptive_perspective, :73-96).  The weights live in LDS only.
//  * ptc_cac_cos_{fwd,bwd}: out[i, k] = cos_temp * normalize(x_i) . normalize(proto[s(i), k]) (get_pred, :66-71).
//  * ptc_cac_distill_{fwd,bwd}: get_distill_loss (:152-199) in one pass over the rows plus per-class sums.
//
// The products [K x rows] x [rows x C], [rows x C] x [C x K] and [rows x K] x [K x C] run on v_mfma_f32_16x16x4_f32 (exact fp32
// products, fp32 accumulation; operand layout as in attention_rpe_f32.h: A[i][r] in lane i + 16 r, B[r][j] in lane j + 16 r,
// D[i][j] in lane j + 16 (i / 4), element i % 4), 32 rows at a time, the row-side operands staged in LDS.
// No float atomics: whatever is reduced over rows (prototypes, weight sums, d proto, the per-class loss sums) is accumulated by a
// workgroup over a FIXED row range in row order, written as a partial, and the partials are added in index order by a finishing
// kernel -- the results are the same bits on every run.  Nothing of size [N, K] is saved between forward and backward: the
// backward kernels recompute the softmax rows.
#include "mma.h"

#define CAC_ROWS 32          // rows per tile
#define CAC_THREADS 256
#define CAC_MAX_K 256
#define CAC_MAX_C 128
#define CAC_NORM_EPS 1e-12f  // F.normalize's clamp

static inline int cac_kp(int k) { return (k + 15) / 16 * 16; }
// LDS row strides (in floats) of a [32][dim] tile, dim a multiple of 16.  ld_m: the tile's rows are the M side of the product (lane i
// reads row i): stride % 32 == 4 puts the 64 lanes on 32 banks twice.  ld_r: its rows are the reduction side (lane i reads column i).
__host__ __device__ static inline int cac_ld_m(int dim) { return dim + ((dim & 31) == 0 ? 4 : 20); }
__host__ __device__ static inline int cac_ld_r(int dim) { return dim + ((dim & 31) == 0 ? 16 : 0); }

// how many fixed row ranges a segment is cut into by the kernels that reduce over rows
static inline int cac_parts(int64_t n, int s) {
  int64_t p = ptc_cdiv(n > 0 ? n : 1, (int64_t)s * 256);
  const int64_t cap = 512 / s > 1 ? 512 / s : 1;
  return (int)(p < 1 ? 1 : p > cap ? cap : p);
}

__device__ __forceinline__ void cac_segment(const int64_t* __restrict__ offset, int s, int64_t n, int64_t& beg, int64_t& end) {
  beg = (offset && s > 0) ? offset[s - 1] : 0;
  end = offset ? offset[s] : n;
  beg = beg < 0 ? 0 : beg > n ? n : beg;
  end = end < beg ? beg : end > n ? n : end;
}

// max and sum exp(v - max) of a row of K values held by 8 consecutive lanes (lane q takes classes q, q + 8, ...); every lane of the
// wave calls this (the shuffles are not under a branch)
__device__ __forceinline__ void cac_row_stats(const float* __restrict__ row, int K, int q, bool live, float& mx, float& sum) {
  float m = -INFINITY;
  if (live) for (int k = q; k < K; k += 8) m = fmaxf(m, row[k]);
  m = fmaxf(m, __shfl_xor(m, 1, 64));
  m = fmaxf(m, __shfl_xor(m, 2, 64));
  m = fmaxf(m, __shfl_xor(m, 4, 64));
  float s = 0.f;
  if (live) for (int k = q; k < K; k += 8) s += expf(row[k] - m);
  s += __shfl_xor(s, 1, 64);
  s += __shfl_xor(s, 2, 64);
  s += __shfl_xor(s, 4, 64);
  mx = m;
  sum = s;
}
__device__ __forceinline__ float cac_sum8(float v) {
  v += __shfl_xor(v, 1, 64);
  v += __shfl_xor(v, 2, 64);
  v += __shfl_xor(v, 4, 64);
  return v;
}

// rows [t0, t0 + 32) of x [n, C] -> tile [32][ld], zero past r1
__device__ __forceinline__ void cac_stage_rows(const float* __restrict__ x, int C, int64_t t0, int64_t r1, float* __restrict__ tile, int ld) {
  const int c4n = C >> 2;
  for (int v = threadIdx.x; v < CAC_ROWS * c4n; v += CAC_THREADS) {
    const int r = v / c4n, c4 = (v - r * c4n) << 2;
    f32x4 val = {0.f, 0.f, 0.f, 0.f};
    if (t0 + r < r1) val = *reinterpret_cast<const f32x4*>(x + (t0 + r) * C + c4);
    *reinterpret_cast<f32x4*>(tile + r * ld + c4) = val;
  }
}

// ------------------------------------------------------------------------------------------------ pooling, forward
// grid (P, S): workgroup (j, s) owns rows [beg_s + j per, beg_s + (j + 1) per) of segment s and leaves part[s][j][Kp][C], wpart[s][j][Kp]
// (the weight sums) and ppart[s][j] (rows that carry weight: passed the gate / have a label).  Wave w holds the output tiles
// w, w + 4, ... of the (Kp / 16) x (C / 16) grid in registers across its whole range.
template <bool HARD, int MAXT>
__global__ void __launch_bounds__(CAC_THREADS)
cac_pool_fwd_kernel(const float* __restrict__ x, const float* __restrict__ logits, const int64_t* __restrict__ target,
                    const int64_t* __restrict__ offset, int64_t n, int K, int C, int Kp, float thresh, float* __restrict__ part,
                    double* __restrict__ wpart, int* __restrict__ ppart) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  float* cac_smem = reinterpret_cast<float*>(smem);
  const int ldw = cac_ld_r(Kp), ldx = cac_ld_r(C);
  float* Wl = cac_smem;
  float* Xl = Wl + CAC_ROWS * ldw;
  int* cnt = reinterpret_cast<int*>(Xl + CAC_ROWS * ldx);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 15, lk = lane >> 4;
  const int s = blockIdx.y, P = gridDim.x, j = blockIdx.x;
  int64_t beg, end;
  cac_segment(offset, s, n, beg, end);
  const int64_t per = ((end - beg + P - 1) / P + CAC_ROWS - 1) / CAC_ROWS * CAC_ROWS;
  const int64_t r0 = beg + (int64_t)j * per, r1 = (r0 + per < end) ? r0 + per : end;
  const int CT = C >> 4, ntile = (Kp >> 4) * CT;
  f32x4 acc[MAXT];
#pragma unroll
  for (int t = 0; t < MAXT; ++t) acc[t] = (f32x4){0.f, 0.f, 0.f, 0.f};
  double colsum = 0.0;          // the weight sums in double: exact to the rounding of the result, whatever the range's length
  int passed = 0;
  if (tid == 0) cnt[0] = 0;
  const int row = tid >> 3, q = tid & 7;
  for (int64_t t0 = r0; t0 < r1; t0 += CAC_ROWS) {
    const int64_t gi = t0 + row;
    const bool live = gi < r1;
    if constexpr (HARD) {
      const int64_t tg = live ? target[gi] : -1;
      const bool ok = tg >= 0 && tg < K;
      for (int k = q; k < Kp; k += 8) Wl[row * ldw + k] = (ok && tg == k) ? 1.f : 0.f;
      passed += (q == 0 && ok) ? 1 : 0;
    } else {
      const float* lr = logits + (live ? gi : 0) * K;
      float m, sum;
      cac_row_stats(lr, K, q, live, m, sum);
      const bool gate = live && (thresh <= 0.f || 1.f / sum >= thresh);      // the row's largest probability is exp(0) / sum
      for (int k = q; k < Kp; k += 8) Wl[row * ldw + k] = (gate && k < K) ? expf(lr[k] - m) / sum : 0.f;
      passed += (q == 0 && gate) ? 1 : 0;
    }
    cac_stage_rows(x, C, t0, r1, Xl, ldx);
    __syncthreads();
    if (tid < Kp) {
#pragma unroll 8
      for (int r = 0; r < CAC_ROWS; ++r) colsum += (double)Wl[r * ldw + tid];
    }
#pragma unroll
    for (int t = 0; t < MAXT; ++t) {
      const int id = wave + 4 * t;
      if (id < ntile) {
        const int kt = id / CT, ct = id - kt * CT;
        const float* a = Wl + lk * ldw + kt * 16 + li;
        const float* b = Xl + lk * ldx + ct * 16 + li;
#pragma unroll
        for (int r4 = 0; r4 < CAC_ROWS / 4; ++r4) acc[t] = ptc_mfma_f32_4(a[4 * r4 * ldw], b[4 * r4 * ldx], acc[t]);
      }
    }
    __syncthreads();
  }
  float* out = part + ((int64_t)s * P + j) * Kp * C;
#pragma unroll
  for (int t = 0; t < MAXT; ++t) {
    const int id = wave + 4 * t;
    if (id < ntile) {
      const int kt = id / CT, ct = id - kt * CT;
#pragma unroll
      for (int e = 0; e < 4; ++e) out[(kt * 16 + 4 * lk + e) * C + ct * 16 + li] = acc[t][e];
    }
  }
  if (tid < Kp) wpart[((int64_t)s * P + j) * Kp + tid] = colsum;
  if (passed) atomicAdd(cnt, passed);          // an integer count: exact in any order
  __syncthreads();
  if (tid == 0) ppart[s * P + j] = cnt[0];
}

__global__ void __launch_bounds__(256)
cac_pool_finish_kernel(const float* __restrict__ part, const double* __restrict__ wpart, const int* __restrict__ ppart, int S, int P, int K,
                       int C, int Kp, float eps, float* __restrict__ proto, float* __restrict__ wsum, int64_t* __restrict__ count,
                       int64_t* __restrict__ passed) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (int64_t)S * K * C) return;
  const int c = (int)(idx % C), k = (int)((idx / C) % K), s = (int)(idx / ((int64_t)C * K));
  double w = 0.0;          // the partial sums are exact integers in hard mode: their double sum is the class count
  float acc = 0.f;
  for (int j = 0; j < P; ++j) {
    w += wpart[((int64_t)s * P + j) * Kp + k];
    acc += part[(((int64_t)s * P + j) * Kp + k) * C + c];
  }
  proto[idx] = acc / ((float)w + eps);
  if (c == 0) {
    wsum[s * K + k] = (float)w;
    if (count) count[s * K + k] = (int64_t)w;
    if (k == 0) {
      int64_t p = 0;
      for (int j = 0; j < P; ++j) p += ppart[s * P + j];
      passed[s] = p;
    }
  }
}

// ------------------------------------------------------------------------------------------------ pooling, backward
// hard: dx_i = dproto[target_i] / (count + eps), a gather
__global__ void __launch_bounds__(256)
cac_pool_bwd_hard_kernel(const int64_t* __restrict__ target, int64_t n, int K, int C, float eps, const float* __restrict__ wsum,
                         const float* __restrict__ dproto, float* __restrict__ dx) {
  const int c4n = C >> 2;
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= n * c4n) return;
  const int64_t i = idx / c4n;
  const int c4 = (int)(idx - i * c4n) << 2;
  const int64_t t = target[i];
  f32x4 v = {0.f, 0.f, 0.f, 0.f};
  if (t >= 0 && t < K) {
    const float inv = 1.f / (wsum[t] + eps);
    v = *reinterpret_cast<const f32x4*>(dproto + t * C + c4) * inv;
  }
  *reinterpret_cast<f32x4*>(dx + i * C + c4) = v;
}

// soft: grid (T, S), workgroup (t, s) walks the 32-row tiles t, t + T, ... of segment s.
//   u_ik = x_i . dproto_k (MFMA 1);  g_ik = gate_i (u_ik - proto_k . dproto_k) / (S_k + eps);  dlogit_i = p_i (g_i - p_i . g_i);
//   dx_i = sum_k gate_i p_ik / (S_k + eps) dproto_k (MFMA 2).  dlogits == nullptr: only dx.
__global__ void __launch_bounds__(CAC_THREADS)
cac_pool_bwd_soft_kernel(const float* __restrict__ x, const float* __restrict__ logits, const int64_t* __restrict__ offset, int64_t n, int K,
                         int C, int Kp, float thresh, float eps, const float* __restrict__ proto, const float* __restrict__ wsum,
                         const float* __restrict__ dproto, float* __restrict__ dx, float* __restrict__ dlogits) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  float* cac_smem = reinterpret_cast<float*>(smem);
  const int ldx = cac_ld_m(C), ldk = cac_ld_m(Kp);
  float* Xl = cac_smem;
  float* Gl = Xl + CAC_ROWS * ldx;
  float* invS = Gl + CAC_ROWS * ldk;
  double* pd = reinterpret_cast<double*>(invS + Kp);      // proto_k . dproto_k in double: u_ik - pd_k cancels (exactly, in a one-row scene)
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 15, lk = lane >> 4;
  const int s = blockIdx.y;
  int64_t beg, end;
  cac_segment(offset, s, n, beg, end);
  const float* dps = dproto + (int64_t)s * K * C;
  const float* ps = proto + (int64_t)s * K * C;
  for (int k = tid; k < Kp; k += CAC_THREADS) {
    double d = 0.0;
    if (k < K) for (int c = 0; c < C; ++c) d += (double)ps[k * C + c] * (double)dps[k * C + c];
    pd[k] = d;
    invS[k] = k < K ? 1.f / (wsum[s * K + k] + eps) : 0.f;
  }
  __syncthreads();
  const int row = tid >> 3, q = tid & 7, CT = C >> 4, KT = Kp >> 4;
  for (int64_t t0 = beg + (int64_t)blockIdx.x * CAC_ROWS; t0 < end; t0 += (int64_t)gridDim.x * CAC_ROWS) {
    cac_stage_rows(x, C, t0, end, Xl, ldx);
    __syncthreads();
    if (dlogits) {
      for (int id = wave; id < 2 * KT; id += 4) {
        const int mt = id & 1, nt = id >> 1;
        const float* a = Xl + (mt * 16 + li) * ldx + lk;
        const bool bk = nt * 16 + li < K;
        const float* b = dps + (bk ? nt * 16 + li : 0) * C + lk;
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
        for (int r4 = 0; r4 < C / 4; ++r4) acc = ptc_mfma_f32_4(a[4 * r4], bk ? b[4 * r4] : 0.f, acc);
#pragma unroll
        for (int e = 0; e < 4; ++e) Gl[(mt * 16 + 4 * lk + e) * ldk + nt * 16 + li] = acc[e];
      }
      __syncthreads();
    }
    {
      const int64_t gi = t0 + row;
      const bool live = gi < end;
      const float* lr = logits + (live ? gi : 0) * K;
      float m, sum;
      cac_row_stats(lr, K, q, live, m, sum);
      const bool gate = live && (thresh <= 0.f || 1.f / sum >= thresh);
      float* gr = Gl + row * ldk;
      if (dlogits) {
        float dot = 0.f;
        if (gate) for (int k = q; k < K; k += 8) {
          const float g = (float)((double)gr[k] - pd[k]) * invS[k];
          gr[k] = g;
          dot += expf(lr[k] - m) / sum * g;
        }
        dot = cac_sum8(dot);
        if (live) for (int k = q; k < K; k += 8) dlogits[gi * K + k] = gate ? expf(lr[k] - m) / sum * (gr[k] - dot) : 0.f;
      }
      for (int k = q; k < Kp; k += 8) gr[k] = (gate && k < K) ? expf(lr[k] - m) / sum * invS[k] : 0.f;
    }
    __syncthreads();
    for (int id = wave; id < 2 * CT; id += 4) {
      const int mt = id & 1, nt = id >> 1;
      const float* a = Gl + (mt * 16 + li) * ldk + lk;
      const float* b = dps + nt * 16 + li;
      f32x4 acc = {0.f, 0.f, 0.f, 0.f};
      for (int r4 = 0; r4 < Kp / 4; ++r4) {
        const int k = 4 * r4 + lk;
        acc = ptc_mfma_f32_4(a[4 * r4], k < K ? b[k * C] : 0.f, acc);
      }
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int64_t gi = t0 + mt * 16 + 4 * lk + e;
        if (gi < end) dx[gi * C + nt * 16 + li] = acc[e];
      }
    }
    __syncthreads();
  }
}

// ------------------------------------------------------------------------------------------------ cosine classifier
// phat[s][Kp][C] = proto / max(|proto|, 1e-12) (rows k >= K zero), pnorm[s][Kp] = |proto|: one wave per row
__global__ void __launch_bounds__(64)
cac_cos_prep_kernel(const float* __restrict__ proto, int K, int C, int Kp, float* __restrict__ phat, float* __restrict__ pnorm) {
  const int k = blockIdx.x, s = blockIdx.y, lane = threadIdx.x;
  const float* p = proto + ((int64_t)s * K + k) * C;
  float* o = phat + ((int64_t)s * Kp + k) * C;
  float v0 = 0.f, v1 = 0.f;
  if (k < K) {
    v0 = lane < C ? p[lane] : 0.f;
    v1 = lane + 64 < C ? p[lane + 64] : 0.f;
  }
  float ss = v0 * v0 + v1 * v1;
#pragma unroll
  for (int w = 1; w < 64; w <<= 1) ss += __shfl_xor(ss, w, 64);
  const float nrm = sqrtf(ss), d = fmaxf(nrm, CAC_NORM_EPS);
  if (lane < C) o[lane] = v0 / d;
  if (lane + 64 < C) o[lane + 64] = v1 / d;
  if (lane == 0) pnorm[s * Kp + k] = nrm;
}

// 1 / max(|x_i|, 1e-12) of the 32 staged rows (8 lanes per row), and whether the clamp is active
__device__ __forceinline__ void cac_row_norms(const float* __restrict__ Xl, int ldx, int C, float* __restrict__ rinv, float* __restrict__ clamped) {
  const int row = threadIdx.x >> 3, q = threadIdx.x & 7;
  float ss = 0.f;
  for (int c = q; c < C; c += 8) ss += Xl[row * ldx + c] * Xl[row * ldx + c];
  ss = cac_sum8(ss);
  const float nrm = sqrtf(ss);
  if (q == 0) {
    rinv[row] = 1.f / fmaxf(nrm, CAC_NORM_EPS);
    if (clamped) clamped[row] = nrm > CAC_NORM_EPS ? 0.f : 1.f;
  }
}

// grid (T, S): out[i, k] = cos_temp * (x_i . phat_k) / max(|x_i|, 1e-12)
__global__ void __launch_bounds__(CAC_THREADS)
cac_cos_fwd_kernel(const float* __restrict__ x, const float* __restrict__ phat, const int64_t* __restrict__ offset, int64_t n, int K, int C,
                   int Kp, float cos_temp, float* __restrict__ out) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  float* cac_smem = reinterpret_cast<float*>(smem);
  const int ldx = cac_ld_m(C);
  float* Xl = cac_smem;
  float* rinv = Xl + CAC_ROWS * ldx;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 15, lk = lane >> 4;
  const int s = blockIdx.y, KT = Kp >> 4;
  int64_t beg, end;
  cac_segment(offset, s, n, beg, end);
  const float* ph = phat + (int64_t)s * Kp * C;
  for (int64_t t0 = beg + (int64_t)blockIdx.x * CAC_ROWS; t0 < end; t0 += (int64_t)gridDim.x * CAC_ROWS) {
    cac_stage_rows(x, C, t0, end, Xl, ldx);
    __syncthreads();
    cac_row_norms(Xl, ldx, C, rinv, nullptr);
    __syncthreads();
    for (int id = wave; id < 2 * KT; id += 4) {
      const int mt = id & 1, nt = id >> 1;
      const float* a = Xl + (mt * 16 + li) * ldx + lk;
      const float* b = ph + (nt * 16 + li) * C + lk;
      f32x4 acc = {0.f, 0.f, 0.f, 0.f};
      for (int r4 = 0; r4 < C / 4; ++r4) acc = ptc_mfma_f32_4(a[4 * r4], b[4 * r4], acc);
      const int col = nt * 16 + li;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int r = mt * 16 + 4 * lk + e;
        if (t0 + r < end && col < K) out[(t0 + r) * K + col] = acc[e] * rinv[r] * cos_temp;
      }
    }
    __syncthreads();
  }
}

// grid (P, S), fixed row ranges as in the pooling forward.  Per tile: D = cos_temp dout, xh = x / max(|x|, eps);
//   y_i = sum_k D_ik phat_k (MFMA),  dx_i = (y_i - xh_i (xh_i . y_i)) / |x_i|   (the clamp active: y_i / eps);
//   dphat_k += sum_i D_ik xh_i (MFMA, accumulated over the range) -> part[s][j][Kp][C].
template <int MAXT>
__global__ void __launch_bounds__(CAC_THREADS)
cac_cos_bwd_kernel(const float* __restrict__ x, const float* __restrict__ phat, const int64_t* __restrict__ offset, int64_t n, int K, int C,
                   int Kp, float cos_temp, const float* __restrict__ dout, float* __restrict__ dx, float* __restrict__ part) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  float* cac_smem = reinterpret_cast<float*>(smem);
  const int ldx = cac_ld_m(C), ldk = cac_ld_m(Kp);
  float* Xl = cac_smem;
  float* Yl = Xl + CAC_ROWS * ldx;
  float* Dl = Yl + CAC_ROWS * ldx;
  float* rinv = Dl + CAC_ROWS * ldk;
  float* clamped = rinv + CAC_ROWS;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 15, lk = lane >> 4;
  const int s = blockIdx.y, P = gridDim.x, j = blockIdx.x;
  int64_t beg, end;
  cac_segment(offset, s, n, beg, end);
  const int64_t per = ((end - beg + P - 1) / P + CAC_ROWS - 1) / CAC_ROWS * CAC_ROWS;
  const int64_t r0 = beg + (int64_t)j * per, r1 = (r0 + per < end) ? r0 + per : end;
  const float* ph = phat + (int64_t)s * Kp * C;
  const int CT = C >> 4, ntile = (Kp >> 4) * CT;
  f32x4 acc[MAXT];
#pragma unroll
  for (int t = 0; t < MAXT; ++t) acc[t] = (f32x4){0.f, 0.f, 0.f, 0.f};
  const int row = tid >> 3, q = tid & 7;
  for (int64_t t0 = r0; t0 < r1; t0 += CAC_ROWS) {
    cac_stage_rows(x, C, t0, r1, Xl, ldx);
    {
      const int64_t gi = t0 + row;
      for (int k = q; k < Kp; k += 8) Dl[row * ldk + k] = (gi < r1 && k < K) ? dout[gi * K + k] * cos_temp : 0.f;
    }
    __syncthreads();
    cac_row_norms(Xl, ldx, C, rinv, clamped);
    __syncthreads();
    for (int c = q; c < C; c += 8) Xl[row * ldx + c] *= rinv[row];
    for (int id = wave; id < 2 * CT; id += 4) {          // y = D phat
      const int mt = id & 1, nt = id >> 1;
      const float* a = Dl + (mt * 16 + li) * ldk + lk;
      const float* b = ph + lk * C + nt * 16 + li;
      f32x4 y = {0.f, 0.f, 0.f, 0.f};
      for (int r4 = 0; r4 < Kp / 4; ++r4) y = ptc_mfma_f32_4(a[4 * r4], b[4 * r4 * C], y);
#pragma unroll
      for (int e = 0; e < 4; ++e) Yl[(mt * 16 + 4 * lk + e) * ldx + nt * 16 + li] = y[e];
    }
    __syncthreads();
    {
      float dot = 0.f;
      for (int c = q; c < C; c += 8) dot += Xl[row * ldx + c] * Yl[row * ldx + c];
      dot = cac_sum8(dot);
      if (clamped[row] != 0.f) dot = 0.f;
      const int64_t gi = t0 + row;
      if (gi < r1) for (int c = q; c < C; c += 8) dx[gi * C + c] = (Yl[row * ldx + c] - Xl[row * ldx + c] * dot) * rinv[row];
    }
#pragma unroll
    for (int t = 0; t < MAXT; ++t) {                     // dphat += D^T xh
      const int id = wave + 4 * t;
      if (id < ntile) {
        const int kt = id / CT, ct = id - kt * CT;
        const float* a = Dl + lk * ldk + kt * 16 + li;
        const float* b = Xl + lk * ldx + ct * 16 + li;
#pragma unroll
        for (int r4 = 0; r4 < CAC_ROWS / 4; ++r4) acc[t] = ptc_mfma_f32_4(a[4 * r4 * ldk], b[4 * r4 * ldx], acc[t]);
      }
    }
    __syncthreads();
  }
  float* out = part + ((int64_t)s * P + j) * Kp * C;
#pragma unroll
  for (int t = 0; t < MAXT; ++t) {
    const int id = wave + 4 * t;
    if (id < ntile) {
      const int kt = id / CT, ct = id - kt * CT;
#pragma unroll
      for (int e = 0; e < 4; ++e) out[(kt * 16 + 4 * lk + e) * C + ct * 16 + li] = acc[t][e];
    }
  }
}

// one wave per (k, s): dphat_k = sum_j part;  dproto_k = (dphat_k - phat_k (phat_k . dphat_k)) / |proto_k|   (clamped: dphat_k / eps)
__global__ void __launch_bounds__(64)
cac_cos_finish_kernel(const float* __restrict__ part, const float* __restrict__ phat, const float* __restrict__ pnorm, int P, int K, int C,
                      int Kp, float* __restrict__ dproto) {
  const int k = blockIdx.x, s = blockIdx.y, lane = threadIdx.x;
  float d0 = 0.f, d1 = 0.f;
  for (int j = 0; j < P; ++j) {
    const float* p = part + (((int64_t)s * P + j) * Kp + k) * C;
    if (lane < C) d0 += p[lane];
    if (lane + 64 < C) d1 += p[lane + 64];
  }
  const float* h = phat + ((int64_t)s * Kp + k) * C;
  const float h0 = lane < C ? h[lane] : 0.f, h1 = lane + 64 < C ? h[lane + 64] : 0.f;
  float dot = h0 * d0 + h1 * d1;
#pragma unroll
  for (int w = 1; w < 64; w <<= 1) dot += __shfl_xor(dot, w, 64);
  const float nrm = pnorm[s * Kp + k];
  if (!(nrm > CAC_NORM_EPS)) dot = 0.f;
  const float inv = 1.f / fmaxf(nrm, CAC_NORM_EPS);
  float* o = dproto + ((int64_t)s * K + k) * C;
  if (lane < C) o[lane] = (d0 - h0 * dot) * inv;
  if (lane + 64 < C) o[lane + 64] = (d1 - h1 * dot) * inv;
}

// ------------------------------------------------------------------------------------------------ distillation loss
struct CacRowLoss { float loss, ent, lsum; };

// the row quantities of get_distill_loss for 8 lanes per row: loss_i = -sum_k log_softmax(pred)_k label_k, ent_i = -sum_k q_k log(q_k + 1e-4),
// lsum = sum_k label_k; label = smoothness q + (1 - smoothness) onehot(t0), then the eps branch.  t0: the row's class (0 for ignored rows).
__device__ __forceinline__ float cac_label(float qk, bool hot, float smooth, float eps, int K) {
  float l = smooth * qk + (1.f - smooth) * (hot ? 1.f : 0.f);
  if (eps > 0.f) l = l * (1.f - eps) + (1.f - l) * eps / (float)(K - 1);
  return l;
}
__device__ __forceinline__ CacRowLoss cac_row_loss(const float* __restrict__ pr, const float* __restrict__ sr, int K, int q, bool live, int t0,
                                                   float smooth, float eps, float& m1, float& lse1, float& m2, float& s2) {
  float s1;
  cac_row_stats(pr, K, q, live, m1, s1);
  cac_row_stats(sr, K, q, live, m2, s2);
  lse1 = logf(s1);
  CacRowLoss r = {0.f, 0.f, 0.f};
  if (live) for (int k = q; k < K; k += 8) {
    const float qk = expf(sr[k] - m2) / s2;
    const float l = cac_label(qk, k == t0, smooth, eps, K);
    r.loss -= (pr[k] - m1 - lse1) * l;
    r.ent -= qk * logf(qk + 1e-4f);
    r.lsum += l;
  }
  r.loss = cac_sum8(r.loss);
  r.ent = cac_sum8(r.ent);
  r.lsum = cac_sum8(r.lsum);
  return r;
}

// grid G: workgroup g owns a fixed row range and leaves part[g][3][Kp] = per-class sums of loss * entropy, entropy, row counts
__global__ void __launch_bounds__(CAC_THREADS)
cac_distill_fwd_kernel(const float* __restrict__ pred, const float* __restrict__ soft, const int64_t* __restrict__ target, int64_t n, int K,
                       int Kp, float smooth, float eps, float* __restrict__ part) {
  __shared__ float rl[CAC_ROWS], re[CAC_ROWS];
  __shared__ int rt[CAC_ROWS];
  const int tid = threadIdx.x, row = tid >> 3, q = tid & 7, G = gridDim.x;
  const int64_t per = ((n + G - 1) / G + CAC_ROWS - 1) / CAC_ROWS * CAC_ROWS;
  const int64_t r0 = (int64_t)blockIdx.x * per, r1 = (r0 + per < n) ? r0 + per : n;
  float a = 0.f, e = 0.f, c = 0.f;
  for (int64_t t0 = r0; t0 < r1; t0 += CAC_ROWS) {
    const int64_t gi = t0 + row;
    const bool live = gi < r1;
    const int64_t tg = live ? target[gi] : -1;
    const bool valid = tg >= 0 && tg < K;
    float m1, lse1, m2, s2;
    const CacRowLoss r = cac_row_loss(pred + (live ? gi : 0) * K, soft + (live ? gi : 0) * K, K, q, live, valid ? (int)tg : 0, smooth, eps, m1,
                                      lse1, m2, s2);
    if (q == 0) {
      rt[row] = valid ? (int)tg : -1;
      re[row] = valid ? r.ent : 0.f;
      rl[row] = valid ? r.loss * r.ent : 0.f;
    }
    __syncthreads();
    if (tid < K) {
#pragma unroll 8
      for (int r_ = 0; r_ < CAC_ROWS; ++r_) {
        if (rt[r_] == tid) { a += rl[r_]; e += re[r_]; c += 1.f; }
      }
    }
    __syncthreads();
  }
  if (tid < Kp) {
    float* o = part + (int64_t)blockIdx.x * 3 * Kp;
    o[tid] = a;
    o[Kp + tid] = e;
    o[2 * Kp + tid] = c;
  }
}

// one workgroup: stats[3][K] = the sums over the partials in index order; loss = sum_{k present} A_k / (E_k + 1e-4) / (n_present + 1e-4)
__global__ void __launch_bounds__(CAC_THREADS)
cac_distill_finish_kernel(const float* __restrict__ part, int G, int K, int Kp, float* __restrict__ stats, float* __restrict__ loss) {
  __shared__ float term[CAC_MAX_K], present[CAC_MAX_K];
  const int k = threadIdx.x;
  if (k < K) {
    float a = 0.f, e = 0.f;
    double c = 0.0;
    for (int g = 0; g < G; ++g) {
      const float* p = part + (int64_t)g * 3 * Kp;
      a += p[k];
      e += p[Kp + k];
      c += (double)p[2 * Kp + k];
    }
    stats[k] = a;
    stats[K + k] = e;
    stats[2 * K + k] = (float)c;
    present[k] = c > 0.0 ? 1.f : 0.f;
    term[k] = c > 0.0 ? a / (e + 1e-4f) : 0.f;
  }
  __syncthreads();
  if (k == 0) {
    float tot = 0.f, np = 0.f;
    for (int i = 0; i < K; ++i) { tot += term[i]; np += present[i]; }
    loss[0] = np > 0.f ? tot / (np + 1e-4f) : 0.f;
  }
}

// dpred_ij = dloss * ent_i / (E_t + 1e-4) / (n_present + 1e-4) * (lsum_i softmax(pred_i)_j - label_ij); ignored rows: 0
__global__ void __launch_bounds__(CAC_THREADS)
cac_distill_bwd_kernel(const float* __restrict__ pred, const float* __restrict__ soft, const int64_t* __restrict__ target, int64_t n, int K,
                       float smooth, float eps, const float* __restrict__ stats, const float* __restrict__ dloss, float* __restrict__ dpred) {
  __shared__ float npres;
  const int tid = threadIdx.x, row = tid >> 3, q = tid & 7;
  if (tid == 0) {
    float np = 0.f;
    for (int i = 0; i < K; ++i) np += stats[2 * K + i] > 0.f ? 1.f : 0.f;
    npres = np;
  }
  __syncthreads();
  const float g = dloss[0] / (npres + 1e-4f);
  for (int64_t t0 = (int64_t)blockIdx.x * CAC_ROWS; t0 < n; t0 += (int64_t)gridDim.x * CAC_ROWS) {
    const int64_t gi = t0 + row;
    const bool live = gi < n;
    const int64_t tg = live ? target[gi] : -1;
    const bool valid = tg >= 0 && tg < K;
    const float* pr = pred + (live ? gi : 0) * K;
    const float* sr = soft + (live ? gi : 0) * K;
    float m1, lse1, m2, s2;
    const CacRowLoss r = cac_row_loss(pr, sr, K, q, live, valid ? (int)tg : 0, smooth, eps, m1, lse1, m2, s2);
    if (!live) continue;
    const float coef = valid ? g * r.ent / (stats[K + tg] + 1e-4f) : 0.f;
    for (int k = q; k < K; k += 8) {
      const float l = cac_label(expf(sr[k] - m2) / s2, valid && k == (int)tg, smooth, eps, K);
      dpred[gi * K + k] = valid ? coef * (r.lsum * expf(pr[k] - m1 - lse1) - l) : 0.f;
    }
  }
}

// ------------------------------------------------------------------------------------------------ entry points
static int cac_check(const char* what, int64_t n, int s, int k, int c) {
  PTC_REQUIRE(n >= 0 && s >= 1, PTC_EINVAL, "%s: n=%lld s=%d", what, (long long)n, s);
  PTC_REQUIRE(s <= 512, PTC_EUNSUPPORTED, "%s: %d segments (at most 512)", what, s);
  PTC_REQUIRE(k >= 2 && k <= CAC_MAX_K, PTC_EUNSUPPORTED, "%s: K=%d classes (2 .. %d)", what, k, CAC_MAX_K);
  PTC_REQUIRE(c >= 16 && c <= CAC_MAX_C && (c & 15) == 0, PTC_EUNSUPPORTED, "%s: C=%d is not a multiple of 16 in [16, %d]", what, c, CAC_MAX_C);
  return PTC_OK;
}

extern "C" int ptc_cac_supported(int k, int c) { return k >= 2 && k <= CAC_MAX_K && c >= 16 && c <= CAC_MAX_C && (c & 15) == 0; }

static inline unsigned cac_tile_grid(int64_t n, int s) {
  int64_t t = ptc_cdiv(n > 0 ? n : 1, CAC_ROWS);
  int64_t cap = 2048 / s > 1 ? 2048 / s : 1;
#ifndef __HIPCC__
  if (const char* e = getenv("PTC_EMU_CAC_TILE_WGS")) { const int v = atoi(e); if (v > 0) cap = v; }   // host emulation only: several tiles per workgroup at test sizes
#endif
  return (unsigned)(t > cap ? cap : t);
}

struct CacPoolWs { float* part; double* wpart; int* ppart; size_t total; int P; };
static CacPoolWs cac_pool_ws(void* base, int64_t n, int s, int k, int c) {
  CacPoolWs W;
  const int Kp = cac_kp(k);
  W.P = cac_parts(n, s);
  PtcArena A(base);          // s, P >= 1 and Kp, c >= 16: no piece is empty
  W.part = A.take_as<float>((size_t)s * W.P * Kp * c * 4);
  W.wpart = A.take_as<double>((size_t)s * W.P * Kp * 8);
  W.ppart = A.take_as<int>((size_t)s * W.P * 4);
  W.total = A.total;
  return W;
}

extern "C" size_t ptc_cac_pool_workspace_bytes(int64_t n, int s, int k, int c) {
  if (n < 0 || s < 1 || s > 512 || !ptc_cac_supported(k, c)) return 0;
  return cac_pool_ws(nullptr, n, s, k, c).total;
}

extern "C" int ptc_cac_pool_fwd(const float* x, const float* logits, const int64_t* target, const int64_t* offset, int64_t n, int s, int k, int c,
                                float conf_thresh, float eps, float* proto, float* wsum, int64_t* count, int64_t* passed, void* workspace,
                                size_t workspace_bytes, ptc_stream_t stream) {
  if (int rc = cac_check("ptc_cac_pool_fwd", n, s, k, c)) return rc;
  const bool hard = target != nullptr;
  PTC_REQUIRE(hard != (logits != nullptr), PTC_EINVAL, "ptc_cac_pool_fwd: exactly one of logits / target");
  PTC_REQUIRE(!hard || (s == 1 && count), PTC_EINVAL, "ptc_cac_pool_fwd: hard weights take one segment and a count buffer");
  PTC_REQUIRE(s == 1 || offset, PTC_EINVAL, "ptc_cac_pool_fwd: %d segments without offsets", s);
  PTC_REQUIRE((x || n == 0) && proto && wsum && passed && workspace, PTC_EINVAL, "ptc_cac_pool_fwd: null buffer");
  const CacPoolWs W = cac_pool_ws(workspace, n, s, k, c);
  PTC_REQUIRE(workspace_bytes >= W.total, PTC_EWORKSPACE, "ptc_cac_pool_fwd: workspace %zu < %zu", workspace_bytes, W.total);
  hipStream_t st = (hipStream_t)stream;
  const int Kp = cac_kp(k), ntile = (Kp / 16) * (c / 16);
  const size_t lds = (size_t)CAC_ROWS * (cac_ld_r(Kp) + cac_ld_r(c)) * 4 + 16;
  const dim3 grid((unsigned)W.P, (unsigned)s);
#define CAC_POOL_LAUNCH(HARD, MAXT)                                                                                                      \
  do {                                                                                                                                   \
    if (int rc = ptc_allow_lds(cac_pool_fwd_kernel<HARD, MAXT>, lds)) return rc;                                                         \
    hipLaunchKernelGGL((cac_pool_fwd_kernel<HARD, MAXT>), grid, dim3(CAC_THREADS), lds, st, x, logits, target, offset, n, k, c, Kp,      \
                       conf_thresh, W.part, W.wpart, W.ppart);                                                                           \
  } while (0)
  if (hard) { if (ntile <= 32) CAC_POOL_LAUNCH(true, 8); else CAC_POOL_LAUNCH(true, 32); }
  else { if (ntile <= 32) CAC_POOL_LAUNCH(false, 8); else CAC_POOL_LAUNCH(false, 32); }
#undef CAC_POOL_LAUNCH
  PTC_CHECK_LAUNCH("cac_pool_fwd_kernel");
  const int64_t tot = (int64_t)s * k * c;
  hipLaunchKernelGGL(cac_pool_finish_kernel, dim3((unsigned)ptc_cdiv(tot, 256)), dim3(256), 0, st, W.part, W.wpart, W.ppart, s, W.P, k, c, Kp, eps,
                     proto, wsum, hard ? count : nullptr, passed);
  PTC_CHECK_LAUNCH("cac_pool_finish_kernel");
  return PTC_OK;
}

extern "C" int ptc_cac_pool_bwd(const float* x, const float* logits, const int64_t* target, const int64_t* offset, int64_t n, int s, int k, int c,
                                float conf_thresh, float eps, const float* proto, const float* wsum, const float* dproto, float* dx,
                                float* dlogits, ptc_stream_t stream) {
  if (int rc = cac_check("ptc_cac_pool_bwd", n, s, k, c)) return rc;
  const bool hard = target != nullptr;
  PTC_REQUIRE(hard != (logits != nullptr), PTC_EINVAL, "ptc_cac_pool_bwd: exactly one of logits / target");
  PTC_REQUIRE(!hard || s == 1, PTC_EINVAL, "ptc_cac_pool_bwd: hard weights take one segment");
  PTC_REQUIRE(s == 1 || offset, PTC_EINVAL, "ptc_cac_pool_bwd: %d segments without offsets", s);
  if (n == 0) return PTC_OK;
  PTC_REQUIRE(x && proto && wsum && dproto && dx, PTC_EINVAL, "ptc_cac_pool_bwd: null buffer");
  hipStream_t st = (hipStream_t)stream;
  if (hard) {
    hipLaunchKernelGGL(cac_pool_bwd_hard_kernel, dim3((unsigned)ptc_cdiv(n * (c / 4), 256)), dim3(256), 0, st, target, n, k, c, eps, wsum, dproto, dx);
    PTC_CHECK_LAUNCH("cac_pool_bwd_hard_kernel");
    return PTC_OK;
  }
  const int Kp = cac_kp(k);
  const size_t lds = ((size_t)CAC_ROWS * (cac_ld_m(c) + cac_ld_m(Kp)) + Kp) * 4 + (size_t)Kp * 8;
  if (int rc = ptc_allow_lds(cac_pool_bwd_soft_kernel, lds)) return rc;
  hipLaunchKernelGGL(cac_pool_bwd_soft_kernel, dim3(cac_tile_grid(n, s), (unsigned)s), dim3(CAC_THREADS), lds, st, x, logits, offset, n, k, c, Kp,
                     conf_thresh, eps, proto, wsum, dproto, dx, dlogits);
  PTC_CHECK_LAUNCH("cac_pool_bwd_soft_kernel");
  return PTC_OK;
}

struct CacCosWs { float* phat; float* pnorm; float* part; size_t total; int P; };
static CacCosWs cac_cos_ws(void* base, int64_t n, int s, int k, int c) {
  CacCosWs W;
  const int Kp = cac_kp(k);
  W.P = cac_parts(n, s);
  PtcArena A(base);          // no piece is empty, as above
  W.phat = A.take_as<float>((size_t)s * Kp * c * 4);
  W.pnorm = A.take_as<float>((size_t)s * Kp * 4);
  W.part = A.take_as<float>((size_t)s * W.P * Kp * c * 4);
  W.total = A.total;
  return W;
}

extern "C" size_t ptc_cac_cos_workspace_bytes(int64_t n, int s, int k, int c) {
  if (n < 0 || s < 1 || s > 512 || !ptc_cac_supported(k, c)) return 0;
  return cac_cos_ws(nullptr, n, s, k, c).total;
}

extern "C" int ptc_cac_cos_fwd(const float* x, const float* proto, const int64_t* offset, int64_t n, int s, int k, int c, float cos_temp, float* out,
                               void* workspace, size_t workspace_bytes, ptc_stream_t stream) {
  if (int rc = cac_check("ptc_cac_cos_fwd", n, s, k, c)) return rc;
  PTC_REQUIRE(s == 1 || offset, PTC_EINVAL, "ptc_cac_cos_fwd: %d segments without offsets", s);
  if (n == 0) return PTC_OK;
  PTC_REQUIRE(x && proto && out && workspace, PTC_EINVAL, "ptc_cac_cos_fwd: null buffer");
  const CacCosWs W = cac_cos_ws(workspace, n, s, k, c);
  PTC_REQUIRE(workspace_bytes >= W.total, PTC_EWORKSPACE, "ptc_cac_cos_fwd: workspace %zu < %zu", workspace_bytes, W.total);
  hipStream_t st = (hipStream_t)stream;
  const int Kp = cac_kp(k);
  hipLaunchKernelGGL(cac_cos_prep_kernel, dim3((unsigned)Kp, (unsigned)s), dim3(64), 0, st, proto, k, c, Kp, W.phat, W.pnorm);
  PTC_CHECK_LAUNCH("cac_cos_prep_kernel");
  const size_t lds = ((size_t)CAC_ROWS * cac_ld_m(c) + CAC_ROWS) * 4;
  hipLaunchKernelGGL(cac_cos_fwd_kernel, dim3(cac_tile_grid(n, s), (unsigned)s), dim3(CAC_THREADS), lds, st, x, W.phat, offset, n, k, c, Kp, cos_temp,
                     out);
  PTC_CHECK_LAUNCH("cac_cos_fwd_kernel");
  return PTC_OK;
}

extern "C" int ptc_cac_cos_bwd(const float* x, const float* proto, const int64_t* offset, int64_t n, int s, int k, int c, float cos_temp,
                               const float* dout, float* dx, float* dproto, void* workspace, size_t workspace_bytes, ptc_stream_t stream) {
  if (int rc = cac_check("ptc_cac_cos_bwd", n, s, k, c)) return rc;
  PTC_REQUIRE(s == 1 || offset, PTC_EINVAL, "ptc_cac_cos_bwd: %d segments without offsets", s);
  PTC_REQUIRE(proto && dproto && workspace && ((x && dout && dx) || n == 0), PTC_EINVAL, "ptc_cac_cos_bwd: null buffer");
  const CacCosWs W = cac_cos_ws(workspace, n, s, k, c);
  PTC_REQUIRE(workspace_bytes >= W.total, PTC_EWORKSPACE, "ptc_cac_cos_bwd: workspace %zu < %zu", workspace_bytes, W.total);
  hipStream_t st = (hipStream_t)stream;
  const int Kp = cac_kp(k), ntile = (Kp / 16) * (c / 16);
  hipLaunchKernelGGL(cac_cos_prep_kernel, dim3((unsigned)Kp, (unsigned)s), dim3(64), 0, st, proto, k, c, Kp, W.phat, W.pnorm);
  PTC_CHECK_LAUNCH("cac_cos_prep_kernel");
  const size_t lds = ((size_t)CAC_ROWS * (2 * cac_ld_m(c) + cac_ld_m(Kp)) + 2 * CAC_ROWS) * 4;
  const dim3 grid((unsigned)W.P, (unsigned)s);
  if (ntile <= 32) {
    if (int rc = ptc_allow_lds(cac_cos_bwd_kernel<8>, lds)) return rc;
    hipLaunchKernelGGL(cac_cos_bwd_kernel<8>, grid, dim3(CAC_THREADS), lds, st, x, W.phat, offset, n, k, c, Kp, cos_temp, dout, dx, W.part);
  } else {
    if (int rc = ptc_allow_lds(cac_cos_bwd_kernel<32>, lds)) return rc;
    hipLaunchKernelGGL(cac_cos_bwd_kernel<32>, grid, dim3(CAC_THREADS), lds, st, x, W.phat, offset, n, k, c, Kp, cos_temp, dout, dx, W.part);
  }
  PTC_CHECK_LAUNCH("cac_cos_bwd_kernel");
  hipLaunchKernelGGL(cac_cos_finish_kernel, dim3((unsigned)k, (unsigned)s), dim3(64), 0, st, W.part, W.phat, W.pnorm, W.P, k, c, Kp, dproto);
  PTC_CHECK_LAUNCH("cac_cos_finish_kernel");
  return PTC_OK;
}

static inline int cac_distill_grid(int64_t n) {
  const int64_t g = ptc_cdiv(n > 0 ? n : 1, 4 * CAC_ROWS);
  return (int)(g > 1024 ? 1024 : g);
}

extern "C" size_t ptc_cac_distill_workspace_bytes(int64_t n, int k) {
  if (n < 0 || k < 2 || k > CAC_MAX_K) return 0;
  return (size_t)cac_distill_grid(n) * 3 * cac_kp(k) * 4;
}

extern "C" int ptc_cac_distill_fwd(const float* pred, const float* soft, const int64_t* target, int64_t n, int k, float smoothness, float eps,
                                   float* loss, float* stats, void* workspace, size_t workspace_bytes, ptc_stream_t stream) {
  PTC_REQUIRE(n >= 0, PTC_EINVAL, "ptc_cac_distill_fwd: n < 0");
  PTC_REQUIRE(k >= 2 && k <= CAC_MAX_K, PTC_EUNSUPPORTED, "ptc_cac_distill_fwd: K=%d classes (2 .. %d)", k, CAC_MAX_K);
  PTC_REQUIRE(loss && stats && workspace && ((pred && soft && target) || n == 0), PTC_EINVAL, "ptc_cac_distill_fwd: null buffer");
  PTC_REQUIRE(workspace_bytes >= ptc_cac_distill_workspace_bytes(n, k), PTC_EWORKSPACE, "ptc_cac_distill_fwd: workspace too small");
  hipStream_t st = (hipStream_t)stream;
  const int G = cac_distill_grid(n), Kp = cac_kp(k);
  hipLaunchKernelGGL(cac_distill_fwd_kernel, dim3((unsigned)G), dim3(CAC_THREADS), 0, st, pred, soft, target, n, k, Kp, smoothness, eps,
                     (float*)workspace);
  PTC_CHECK_LAUNCH("cac_distill_fwd_kernel");
  hipLaunchKernelGGL(cac_distill_finish_kernel, dim3(1), dim3(CAC_THREADS), 0, st, (const float*)workspace, G, k, Kp, stats, loss);
  PTC_CHECK_LAUNCH("cac_distill_finish_kernel");
  return PTC_OK;
}

extern "C" int ptc_cac_distill_bwd(const float* pred, const float* soft, const int64_t* target, int64_t n, int k, float smoothness, float eps,
                                   const float* stats, const float* dloss, float* dpred, ptc_stream_t stream) {
  PTC_REQUIRE(n >= 0, PTC_EINVAL, "ptc_cac_distill_bwd: n < 0");
  PTC_REQUIRE(k >= 2 && k <= CAC_MAX_K, PTC_EUNSUPPORTED, "ptc_cac_distill_bwd: K=%d classes (2 .. %d)", k, CAC_MAX_K);
  if (n == 0) return PTC_OK;
  PTC_REQUIRE(pred && soft && target && stats && dloss && dpred, PTC_EINVAL, "ptc_cac_distill_bwd: null buffer");
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(cac_distill_bwd_kernel, dim3(cac_tile_grid(n, 1)), dim3(CAC_THREADS), 0, st, pred, soft, target, n, k, smoothness, eps, stats,
                     dloss, dpred);
  PTC_CHECK_LAUNCH("cac_distill_bwd_kernel");
  return PTC_OK;
}
