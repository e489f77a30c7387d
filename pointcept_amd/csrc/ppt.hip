// ppt.hip -- the language-guided head of Point Prompt Training (pointcept/models/point_prompt_training/
// point_prompt_training_v1m1_language_guided.py:98-107, point_prompt_training_v1m3_neo.py:117-129), gfx950:
//     h = x W^T + b   [N, D];   logits = scale * (h / max(|h|, eps)) e^T   [N, K]
// with D = 512 (CLIP ViT-B/16) and K = 13 .. 200 classes.  h never reaches memory.
//
//  * ptc_ppt_head_fwd: a wave owns 32 rows (two 16-row tiles) whose x fragments stay in registers.  Per 16 columns of D it forms the
//    TRANSPOSED block h^T = W_blk x^T (W the M side, the rows the N side: v_mfma_f32_16x16x32_{bf16,f16} for 16-bit x and W, the exact
//    v_mfma_f32_16x16x4_f32 for fp32), which leaves a lane with four consecutive d of ONE row -- the B-operand layout of the second
//    product logits^T += e_blk h^T, run on the exact fp32 MFMA with h kept in fp32.  |h|^2 is summed from the same registers (the norm of
//    h itself, not the quadratic form in x: that loses cond(W)^2).  W, b and e are read from global memory: together <= 1.3 MB, L2 resident.
//  * ptc_ppt_head_bwd: no D-wide work.  With a_i = scale inv_i dlogits_i [K], rho_i = (dlogits_i . logits_i) inv_i^2 (0 where the
//    clamp max(|h|, eps) is active) and the host-side G = e W [K, C] (fp32), M = W^T W [C, C], u = W^T b [C] (both formed and passed in double):
//        dx_i = a_i G - rho_i (M x_i + u);   A = sum_i a_i x_i^T,  Bm = sum_i rho_i x_i x_i^T,  v = sum_i rho_i x_i,  asum = sum_i a_i,
//        rsum = sum_i rho_i       (dW = e^T A - W Bm - b v^T,  db = e^T asum - W v - b rsum: closed by the caller)
//    on the exact fp32 MFMA over 32-row tiles staged in LDS (layouts as in cac.hip), except M x_i + u, which is accumulated in double.
//    No atomics: a workgroup reduces a FIXED row range in row order into a partial, a finishing kernel adds the partials in index
//    order -- the same bits on every run.
#include "mma.h"

#define PPT_THREADS 256
#define PPT_WAVE_ROWS 32                       // forward: rows per wave and pass (two MFMA row tiles)
#define PPT_FWD_ROWS (4 * PPT_WAVE_ROWS)       // forward: rows per workgroup and pass
#define PPT_ROWS 32                            // backward: rows per tile
#define PPT_MAX_C 128
#define PPT_MAX_D 1024
#define PPT_MAX_K 256
#define PPT_LDS_BUDGET (156 * 1024)             // of the 160 KB of a CU

static inline int ppt_kp(int k) { return (k + 15) / 16 * 16; }
__host__ __device__ static inline int ppt_ld(int dim) { return dim + 4; }      // LDS row stride (floats) of a [32][dim] tile, dim % 16 == 0

extern "C" int ptc_ppt_head_supported(int c, int d, int k, int dtype) {
  return c >= 32 && c <= PPT_MAX_C && (c & 31) == 0 && d >= 64 && d <= PPT_MAX_D && (d & 63) == 0 && k >= 1 && k <= PPT_MAX_K &&
         (dtype == PTC_F32 || dtype == PTC_F16 || dtype == PTC_BF16);
}

// ------------------------------------------------------------------------------------------------ forward
// grid G: workgroup g takes the 128-row passes g, g + G, ...; wave w of a pass the rows [32 w, 32 w + 32) of it.  KT: 16-class tiles held.
template <typename T, int KT>
__global__ void __launch_bounds__(PPT_THREADS)
ppt_head_fwd_kernel(const T* __restrict__ x, const T* __restrict__ w, const float* __restrict__ b, const float* __restrict__ e, int64_t n, int C,
                    int D, int K, float scale, float eps, float* __restrict__ logits, float* __restrict__ inv_norm) {
  using M = Mma<T>;
  constexpr int KS = M::KS, EPL = M::EPL, CSMAX = PPT_MAX_C / KS;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 15, lk = lane >> 4;
  const int cs = C / KS, ktn = (K + 15) >> 4;
  const int64_t npass = (n + PPT_FWD_ROWS - 1) / PPT_FWD_ROWS;
  for (int64_t pass = blockIdx.x; pass < npass; pass += gridDim.x) {
    const int64_t w0 = pass * PPT_FWD_ROWS + wave * PPT_WAVE_ROWS;
    if (w0 >= n) continue;          // the whole wave: no barrier in this kernel
    // x as the N side: row li of tile rt, channels [s KS + lk EPL, + EPL)
    typename M::frag xf[2][CSMAX];
#pragma unroll
    for (int rt = 0; rt < 2; ++rt) {
      const int64_t row = w0 + rt * 16 + li;
#pragma unroll
      for (int s = 0; s < CSMAX; ++s) {
        xf[rt][s] = M::zero();
        if (s < cs && row < n) xf[rt][s] = ld_frag<T>(x + row * C + s * KS + lk * EPL);
      }
    }
    f32x4 acc[2][KT];
#pragma unroll
    for (int rt = 0; rt < 2; ++rt)
#pragma unroll
      for (int kt = 0; kt < KT; ++kt) acc[rt][kt] = (f32x4){0.f, 0.f, 0.f, 0.f};
    float nsq0 = 0.f, nsq1 = 0.f;
    for (int d0 = 0; d0 < D; d0 += 16) {
      // h^T block [16 d][16 rows]: lane (li, lk) ends with d = d0 + 4 lk + {0..3} of row li; the bias starts the accumulator
      f32x4 h0 = *reinterpret_cast<const f32x4*>(b + d0 + 4 * lk), h1 = h0;
      const T* wr = w + (int64_t)(d0 + li) * C + lk * EPL;
#pragma unroll
      for (int s = 0; s < CSMAX; ++s) {
        if (s < cs) {
          const typename M::frag wf = ld_frag<T>(wr + s * KS);
          h0 = M::mma(wf, xf[0][s], h0);
          h1 = M::mma(wf, xf[1][s], h1);
        }
      }
      nsq0 += h0[0] * h0[0] + h0[1] * h0[1] + h0[2] * h0[2] + h0[3] * h0[3];
      nsq1 += h1[0] * h1[0] + h1[1] * h1[1] + h1[2] * h1[2] + h1[3] * h1[3];
      // logits^T [16 classes][16 rows] += e_blk h^T: step j contracts d = d0 + 4 lk + j on both operands
#pragma unroll
      for (int kt = 0; kt < KT; ++kt) {
        if (kt < ktn) {
          const int k = kt * 16 + li;
          f32x4 ef = {0.f, 0.f, 0.f, 0.f};
          if (k < K) ef = *reinterpret_cast<const f32x4*>(e + (int64_t)k * D + d0 + 4 * lk);
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            acc[0][kt] = ptc_mfma_f32_4(ef[j], h0[j], acc[0][kt]);
            acc[1][kt] = ptc_mfma_f32_4(ef[j], h1[j], acc[1][kt]);
          }
        }
      }
    }
    // the four lanes li, li + 16, li + 32, li + 48 hold the four quarters of row li's sum
    nsq0 += __shfl_xor(nsq0, 16, 64);
    nsq0 += __shfl_xor(nsq0, 32, 64);
    nsq1 += __shfl_xor(nsq1, 16, 64);
    nsq1 += __shfl_xor(nsq1, 32, 64);
#pragma unroll
    for (int rt = 0; rt < 2; ++rt) {
      const int64_t row = w0 + rt * 16 + li;
      const float inv = 1.f / fmaxf(sqrtf(rt ? nsq1 : nsq0), eps);
      if (row < n) {
        if (lk == 0) inv_norm[row] = inv;
#pragma unroll
        for (int kt = 0; kt < KT; ++kt) {
          if (kt < ktn) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
              const int k = kt * 16 + 4 * lk + j;          // acc: class 16 kt + 4 lk + j of row li
              if (k < K) logits[row * K + k] = scale * acc[rt][kt][j] * inv;
            }
          }
        }
      }
    }
  }
}

// ------------------------------------------------------------------------------------------------ backward
__device__ __forceinline__ float ppt_sum8(float v) {
  v += __shfl_xor(v, 1, 64);
  v += __shfl_xor(v, 2, 64);
  v += __shfl_xor(v, 4, 64);
  return v;
}

// Yl[r][c] = (M x_r + u)_c = (W^T h_r)_c for the 32 staged rows, in DOUBLE from the double M and u: where h is small against |W| |x| (an
// ill-conditioned W) the sum cancels, and an fp32 M or an fp32 accumulation would leave dx with cond(W)^2 times the rounding of the torch
// expression, which forms W^T dh from h.  C^2 multiply-adds per row, nothing D-wide.  Thread (rg, cl): rows 4 rg .. 4 rg + 3, columns
// cl + 32 j.  M is symmetric: row c is read, the lanes on consecutive columns (LDS: no bank conflict; global: coalesced).
__device__ __forceinline__ void ppt_mx_rows(const double* __restrict__ M, const double* __restrict__ u, const float* __restrict__ Xl,
                                            float* __restrict__ Yl, int C, int ldx) {
  const int rg = threadIdx.x >> 5, cl = threadIdx.x & 31, cj = C >> 5;
  double y[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int jj = 0; jj < 4; ++jj) y[i][jj] = 0.0;
  const float* xr = Xl + 4 * rg * ldx;
#pragma unroll 4
  for (int c = 0; c < C; ++c) {
    const double x0 = (double)xr[c], x1 = (double)xr[ldx + c], x2 = (double)xr[2 * ldx + c], x3 = (double)xr[3 * ldx + c];
#pragma unroll
    for (int jj = 0; jj < 4; ++jj) {
      if (jj < cj) {
        const double m = M[c * C + cl + 32 * jj];
        y[0][jj] = fma(x0, m, y[0][jj]);
        y[1][jj] = fma(x1, m, y[1][jj]);
        y[2][jj] = fma(x2, m, y[2][jj]);
        y[3][jj] = fma(x3, m, y[3][jj]);
      }
    }
  }
#pragma unroll
  for (int jj = 0; jj < 4; ++jj) {
    if (jj < cj) {
      const double uc = u[cl + 32 * jj];
#pragma unroll
      for (int i = 0; i < 4; ++i) Yl[(4 * rg + i) * ldx + cl + 32 * jj] = (float)(y[i][jj] + uc);
    }
  }
}

// grid P: workgroup j owns the rows [j per, (j + 1) per) and leaves its partials; wave w holds the output tiles w, w + 4, ... of A's
// (Kp / 16) x (C / 16) grid and of Bm's (C / 16)^2 grid in registers across its whole range.
template <typename T, int MAXA, int MAXB>
__global__ void __launch_bounds__(PPT_THREADS)
ppt_head_bwd_kernel(const T* __restrict__ x, const float* __restrict__ dlogits, const float* __restrict__ logits,
                    const float* __restrict__ inv_norm, const float* __restrict__ G, const double* __restrict__ Mm, const double* __restrict__ u,
                    int64_t n, int C, int K, int Kp, int mlds, float scale, float eps, T* __restrict__ dx, float* __restrict__ partA,
                    float* __restrict__ partB, double* __restrict__ partv, double* __restrict__ partas, double* __restrict__ partr) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  double* Ml = reinterpret_cast<double*>(smem);          // [C][C] M, when it fits beside the tiles (mlds): read C / 32 times per row
  float* ppt_smem = reinterpret_cast<float*>(Ml + (mlds ? C * C : 0));
  const int ldx = ppt_ld(C), ldk = ppt_ld(Kp);
  float* Xl = ppt_smem;                     // [32][ldx] the rows, fp32
  float* Dl = Xl + PPT_ROWS * ldx;          // [32][ldk] a_i
  float* Yl = Dl + PPT_ROWS * ldk;          // [32][ldx] M x_i + u, formed in double
  float* rho = Yl + PPT_ROWS * ldx;         // [32]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 15, lk = lane >> 4;
  const int P = gridDim.x, j = blockIdx.x;
  const int64_t per = ((n + P - 1) / P + PPT_ROWS - 1) / PPT_ROWS * PPT_ROWS;
  const int64_t r0 = (int64_t)j * per < n ? (int64_t)j * per : n, r1 = (r0 + per < n) ? r0 + per : n;
  const int CT = C >> 4, ntA = (Kp >> 4) * CT, ntB = CT * CT;
  const float inv_eps = eps > 0.f ? 1.f / eps : INFINITY;
  f32x4 accA[MAXA], accB[MAXB];
#pragma unroll
  for (int t = 0; t < MAXA; ++t) accA[t] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int t = 0; t < MAXB; ++t) accB[t] = (f32x4){0.f, 0.f, 0.f, 0.f};
  double asum = 0.0, vsum = 0.0, rsum = 0.0;          // thread k < Kp: sum_i a_ik; thread c < C: sum_i rho_i x_ic; thread 0: sum_i rho_i
  const int row = tid >> 3, q = tid & 7, c4n = C >> 2;
  if (mlds) for (int i = tid; i < C * C; i += PPT_THREADS) Ml[i] = Mm[i];          // visible after the first barrier below
  for (int64_t t0 = r0; t0 < r1; t0 += PPT_ROWS) {
    for (int v = tid; v < PPT_ROWS * c4n; v += PPT_THREADS) {
      const int r = v / c4n, c4 = (v - r * c4n) << 2;
      f32x4 val = {0.f, 0.f, 0.f, 0.f};
      if (t0 + r < r1) {
        const T* p = x + (t0 + r) * C + c4;
        val = (f32x4){ptc_to_float(p[0]), ptc_to_float(p[1]), ptc_to_float(p[2]), ptc_to_float(p[3])};
      }
      *reinterpret_cast<f32x4*>(Xl + r * ldx + c4) = val;
    }
    {
      const int64_t gi = t0 + row;
      const bool live = gi < r1;
      const float inv = live ? inv_norm[gi] : 0.f;
      const float* dr = dlogits + (live ? gi : 0) * K;
      const float* lr = logits + (live ? gi : 0) * K;
      float rr = 0.f;
      if (live) for (int k = q; k < K; k += 8) rr += dr[k] * lr[k];          // dsim . sim: the scale cancels
      rr = ppt_sum8(rr);
      const float coef = scale * inv;
      for (int k = q; k < Kp; k += 8) Dl[row * ldk + k] = (live && k < K) ? dr[k] * coef : 0.f;
      if (q == 0) rho[row] = (live && inv < inv_eps) ? rr * inv * inv : 0.f;      // clamp active: h / eps, no radial term
    }
    __syncthreads();
    if (tid < Kp) {
#pragma unroll 8
      for (int r = 0; r < PPT_ROWS; ++r) asum += (double)Dl[r * ldk + tid];
    }
    if (tid < C) {
#pragma unroll 8
      for (int r = 0; r < PPT_ROWS; ++r) vsum += (double)rho[r] * (double)Xl[r * ldx + tid];
    }
    if (tid == 0) {
      for (int r = 0; r < PPT_ROWS; ++r) rsum += (double)rho[r];
    }
    if (mlds) ppt_mx_rows(Ml, u, Xl, Yl, C, ldx);
    else ppt_mx_rows(Mm, u, Xl, Yl, C, ldx);
    __syncthreads();
    for (int id = wave; id < 2 * CT; id += 4) {          // dx = a G - rho y
      const int mt = id & 1, nt = id >> 1;
      const float* a = Dl + (mt * 16 + li) * ldk + lk;
      const float* bg = G + lk * C + nt * 16 + li;
      f32x4 ag = {0.f, 0.f, 0.f, 0.f};
      for (int r4 = 0; r4 < Kp / 4; ++r4) {
        const int k = 4 * r4 + lk;
        ag = ptc_mfma_f32_4(a[4 * r4], k < K ? bg[4 * r4 * C] : 0.f, ag);
      }
      const int col = nt * 16 + li;
#pragma unroll
      for (int e4 = 0; e4 < 4; ++e4) {
        const int r = mt * 16 + 4 * lk + e4;
        if (t0 + r < r1) dx[(t0 + r) * C + col] = ptc_from_float<T>(ag[e4] - rho[r] * Yl[r * ldx + col]);
      }
    }
#pragma unroll
    for (int t = 0; t < MAXA; ++t) {                     // A += a^T x
      const int id = wave + 4 * t;
      if (id < ntA) {
        const int kt = id / CT, ct = id - kt * CT;
        const float* a = Dl + lk * ldk + kt * 16 + li;
        const float* bx = Xl + lk * ldx + ct * 16 + li;
#pragma unroll
        for (int r4 = 0; r4 < PPT_ROWS / 4; ++r4) accA[t] = ptc_mfma_f32_4(a[4 * r4 * ldk], bx[4 * r4 * ldx], accA[t]);
      }
    }
#pragma unroll
    for (int t = 0; t < MAXB; ++t) {                     // Bm += (rho x)^T x
      const int id = wave + 4 * t;
      if (id < ntB) {
        const int c1 = id / CT, c2 = id - c1 * CT;
        const float* a = Xl + lk * ldx + c1 * 16 + li;
        const float* bx = Xl + lk * ldx + c2 * 16 + li;
#pragma unroll
        for (int r4 = 0; r4 < PPT_ROWS / 4; ++r4) accB[t] = ptc_mfma_f32_4(rho[lk + 4 * r4] * a[4 * r4 * ldx], bx[4 * r4 * ldx], accB[t]);
      }
    }
    __syncthreads();
  }
  float* oa = partA + (int64_t)j * Kp * C;
#pragma unroll
  for (int t = 0; t < MAXA; ++t) {
    const int id = wave + 4 * t;
    if (id < ntA) {
      const int kt = id / CT, ct = id - kt * CT;
#pragma unroll
      for (int e4 = 0; e4 < 4; ++e4) oa[(kt * 16 + 4 * lk + e4) * C + ct * 16 + li] = accA[t][e4];
    }
  }
  float* ob = partB + (int64_t)j * C * C;
#pragma unroll
  for (int t = 0; t < MAXB; ++t) {
    const int id = wave + 4 * t;
    if (id < ntB) {
      const int c1 = id / CT, c2 = id - c1 * CT;
#pragma unroll
      for (int e4 = 0; e4 < 4; ++e4) ob[(c1 * 16 + 4 * lk + e4) * C + c2 * 16 + li] = accB[t][e4];
    }
  }
  if (tid < Kp) partas[(int64_t)j * Kp + tid] = asum;
  if (tid < C) partv[(int64_t)j * C + tid] = vsum;
  if (tid == 0) partr[j] = rsum;
}

// the partials added in index order: A [K, C], Bm [C, C], v [C], asum [K], rsum [1]
__global__ void __launch_bounds__(256)
ppt_head_finish_kernel(const float* __restrict__ partA, const float* __restrict__ partB, const double* __restrict__ partv,
                       const double* __restrict__ partas, const double* __restrict__ partr, int P, int K, int C, int Kp, float* __restrict__ A,
                       float* __restrict__ Bm, float* __restrict__ v, float* __restrict__ asum, float* __restrict__ rsum) {
  const int nA = K * C, nB = C * C;
  int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx < nA) {
    float s = 0.f;
    for (int j = 0; j < P; ++j) s += partA[(int64_t)j * Kp * C + idx];
    A[idx] = s;
    return;
  }
  idx -= nA;
  if (idx < nB) {
    float s = 0.f;
    for (int j = 0; j < P; ++j) s += partB[(int64_t)j * nB + idx];
    Bm[idx] = s;
    return;
  }
  idx -= nB;
  if (idx < C) {
    double s = 0.0;
    for (int j = 0; j < P; ++j) s += partv[(int64_t)j * C + idx];
    v[idx] = (float)s;
    return;
  }
  idx -= C;
  if (idx < K) {
    double s = 0.0;
    for (int j = 0; j < P; ++j) s += partas[(int64_t)j * Kp + idx];
    asum[idx] = (float)s;
    return;
  }
  idx -= K;
  if (idx == 0) {
    double s = 0.0;
    for (int j = 0; j < P; ++j) s += partr[j];
    rsum[0] = (float)s;
  }
}

// ------------------------------------------------------------------------------------------------ entry points
static inline int ppt_parts(int64_t n) {
  const int64_t p = ptc_cdiv(n > 0 ? n : 1, 8 * PPT_ROWS);
  return (int)(p > 512 ? 512 : p);
}

struct PptWs { float* partA; float* partB; double* partv; double* partas; double* partr; size_t total; int P; };
static PptWs ppt_ws(void* base, int64_t n, int c, int k) {
  PptWs W;
  const int Kp = ppt_kp(k);
  W.P = ppt_parts(n);
  PtcArena A(base);          // P >= 1, Kp >= 16, c >= 32: no piece is empty
  W.partA = A.take_as<float>((size_t)W.P * Kp * c * 4);
  W.partB = A.take_as<float>((size_t)W.P * c * c * 4);
  W.partv = A.take_as<double>((size_t)W.P * c * 8);
  W.partas = A.take_as<double>((size_t)W.P * Kp * 8);
  W.partr = A.take_as<double>((size_t)W.P * 8);
  W.total = A.total;
  return W;
}

extern "C" size_t ptc_ppt_head_workspace_bytes(int64_t n, int c, int d, int k) {
  if (n < 0 || !ptc_ppt_head_supported(c, d, k, PTC_F32)) return 0;
  return ppt_ws(nullptr, n, c, k).total;
}

template <typename T>
static int ppt_fwd_launch(const void* x, const void* w, const float* b, const float* e, int64_t n, int c, int d, int k, float scale, float eps,
                          float* logits, float* inv_norm, hipStream_t st) {
  const int64_t passes = ptc_cdiv(n, PPT_FWD_ROWS);
  const int64_t g = ptc_cdiv(passes, 2);          // two passes per workgroup up to 2048 workgroups, then a longer loop
  const dim3 grid((unsigned)(g > 2048 ? 2048 : g));
  const int ktn = ppt_kp(k) / 16;
#define PPT_FWD_LAUNCH(KT)                                                                                                              \
  hipLaunchKernelGGL((ppt_head_fwd_kernel<T, KT>), grid, dim3(PPT_THREADS), 0, st, (const T*)x, (const T*)w, b, e, n, c, d, k, scale, eps, \
                     logits, inv_norm)
  if (ktn <= 2) PPT_FWD_LAUNCH(2);
  else if (ktn <= 4) PPT_FWD_LAUNCH(4);
  else if (ktn <= 8) PPT_FWD_LAUNCH(8);
  else PPT_FWD_LAUNCH(16);
#undef PPT_FWD_LAUNCH
  PTC_CHECK_LAUNCH("ppt_head_fwd_kernel");
  return PTC_OK;
}

extern "C" int ptc_ppt_head_fwd(const void* x, const void* w, const float* b, const float* e, int64_t n, int c, int d, int k, int dtype,
                                float scale, float eps, float* logits, float* inv_norm, ptc_stream_t stream) {
  PTC_REQUIRE(n >= 0, PTC_EINVAL, "ptc_ppt_head_fwd: n=%lld", (long long)n);
  PTC_REQUIRE(ptc_ppt_head_supported(c, d, k, dtype), PTC_EUNSUPPORTED,
              "ptc_ppt_head_fwd: C=%d D=%d K=%d dtype=%d (C a multiple of 32 up to %d, D a multiple of 64 up to %d, K 1 .. %d)", c, d, k, dtype,
              PPT_MAX_C, PPT_MAX_D, PPT_MAX_K);
  PTC_REQUIRE(eps >= 0.f, PTC_EINVAL, "ptc_ppt_head_fwd: eps < 0");
  if (n == 0) return PTC_OK;
  PTC_REQUIRE(x && w && b && e && logits && inv_norm, PTC_EINVAL, "ptc_ppt_head_fwd: null buffer");
  hipStream_t st = (hipStream_t)stream;
  PTC_DISPATCH_DTYPE(dtype, T, return ppt_fwd_launch<T>(x, w, b, e, n, c, d, k, scale, eps, logits, inv_norm, st));
  return PTC_OK;
}

template <typename T>
static int ppt_bwd_launch(const void* x, const float* dlogits, const float* logits, const float* inv_norm, const float* G, const double* Mm,
                          const double* u, int64_t n, int c, int k, float scale, float eps, void* dx, const PptWs& W, hipStream_t st) {
  const int Kp = ppt_kp(k), ntA = (Kp / 16) * (c / 16), ntB = (c / 16) * (c / 16);
  const size_t tiles = ((size_t)PPT_ROWS * (2 * ppt_ld(c) + ppt_ld(Kp)) + PPT_ROWS) * 4, mbytes = (size_t)c * c * 8;
  const int mlds = tiles + mbytes <= PPT_LDS_BUDGET;          // C <= 96: M beside the tiles; C = 128 reads it from global memory (L2)
  const size_t lds = tiles + (mlds ? mbytes : 0);
#define PPT_BWD_LAUNCH(MAXA, MAXB)                                                                                                       \
  do {                                                                                                                                   \
    if (int rc = ptc_allow_lds(ppt_head_bwd_kernel<T, MAXA, MAXB>, lds)) return rc;                                                      \
    hipLaunchKernelGGL((ppt_head_bwd_kernel<T, MAXA, MAXB>), dim3((unsigned)W.P), dim3(PPT_THREADS), lds, st, (const T*)x, dlogits, logits, \
                       inv_norm, G, Mm, u, n, c, k, Kp, mlds, scale, eps, (T*)dx, W.partA, W.partB, W.partv, W.partas, W.partr);               \
  } while (0)
  if (ntA <= 32 && ntB <= 16) PPT_BWD_LAUNCH(8, 4);          // C <= 64 and Kp C <= 8192
  else if (ntA <= 32) PPT_BWD_LAUNCH(8, 16);
  else PPT_BWD_LAUNCH(32, 16);
#undef PPT_BWD_LAUNCH
  PTC_CHECK_LAUNCH("ppt_head_bwd_kernel");
  return PTC_OK;
}

extern "C" int ptc_ppt_head_bwd(const void* x, const float* dlogits, const float* logits, const float* inv_norm, const float* G, const double* M,
                                const double* u, int64_t n, int c, int d, int k, int dtype, float scale, float eps, void* dx, float* A, float* Bm,
                                float* v, float* asum, float* rsum, void* workspace, size_t workspace_bytes, ptc_stream_t stream) {
  PTC_REQUIRE(n >= 0, PTC_EINVAL, "ptc_ppt_head_bwd: n=%lld", (long long)n);
  PTC_REQUIRE(ptc_ppt_head_supported(c, d, k, dtype), PTC_EUNSUPPORTED, "ptc_ppt_head_bwd: C=%d D=%d K=%d dtype=%d", c, d, k, dtype);
  PTC_REQUIRE(eps >= 0.f, PTC_EINVAL, "ptc_ppt_head_bwd: eps < 0");
  PTC_REQUIRE(G && M && u && A && Bm && v && asum && rsum && workspace && ((x && dlogits && logits && inv_norm && dx) || n == 0), PTC_EINVAL,
              "ptc_ppt_head_bwd: null buffer");
  const PptWs W = ppt_ws(workspace, n, c, k);
  PTC_REQUIRE(workspace_bytes >= W.total, PTC_EWORKSPACE, "ptc_ppt_head_bwd: workspace %zu < %zu", workspace_bytes, W.total);
  hipStream_t st = (hipStream_t)stream;
  PTC_DISPATCH_DTYPE(dtype, T, if (int rc = ppt_bwd_launch<T>(x, dlogits, logits, inv_norm, G, M, u, n, c, k, scale, eps, dx, W, st)) return rc);
  const int tot = k * c + c * c + c + k + 1;
  hipLaunchKernelGGL(ppt_head_finish_kernel, dim3((unsigned)ptc_cdiv(tot, 256)), dim3(256), 0, st, W.partA, W.partB, W.partv, W.partas, W.partr, W.P,
                     k, c, ppt_kp(k), A, Bm, v, asum, rsum);
  PTC_CHECK_LAUNCH("ppt_head_finish_kernel");
  return PTC_OK;
}
