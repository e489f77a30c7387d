// criteria.hip -- a whole `criteria=[...]` list of row-local segmentation losses in ONE forward and ONE backward pass over the seg
// logits [N, C] (pointcept/models/losses/misc.py; builder.py:22-31 sums the terms):
//   a. CrossEntropyLoss(weight, label_smoothing, reduction = mean | sum)      (misc.py:14-39 -> nn.CrossEntropyLoss)
//   b. FocalLoss(gamma, alpha float | list, reduction = mean)                 (misc.py:96-172, the per-element sigmoid form)
//   c. DiceLoss(smooth, exponent 1 | 2 | 3)                                   (misc.py:175-223)
// each switched by a wave-uniform run-time flag, all sharing one ignore_index.  One thread owns one point, the row lives in registers
// (loss_rows.h, C <= LR_CP); the logits are read once per direction and dlogits written once, through LDS, whatever the list holds.
// x = the row, p = softmax(x), t = the label; a row is COUNTED iff t != ignore_index && 0 <= t < C.
//   a. row loss (1-eps) w[t] (lse - x[t]) + (eps/C) sum_c w[c] (lse - x[c]);  mean divides by sum_counted w[t] (also with eps > 0, as ATen).
//      d/dx_c = s [((1-eps) w[t] + (eps/C) W) p_c - (1-eps) w[t] [c==t] - (eps/C) w[c]],  W = sum w;  p_t - 1 is taken from expm1.
//   b. per element (counted rows x C): y = [c==t], z = y ? -x : x:  alpha_y sigma(z)^gamma softplus(z), alpha_y = y ? alpha_c : 1 - alpha_c;
//      mean over counted rows x C.  sigma(+-z) and softplus(+-z) come from e = exp(-|z|) without a subtraction, sigma(z)^gamma =
//      exp(-gamma softplus(-z));  d/dz = alpha_y sigma(z)^gamma (gamma sigma(-z) softplus(z) + sigma(z)),  dz/dx = y ? -1 : 1.
//   c. rows with t != ignore_index take part, their label CLAMPED into [0, C-1] (the reference's quirk);  per class A_c = sum p_ic [t_i==c],
//      B_c = sum p_ic^e, T_c = #[t_i==c];  loss = (1/C) sum_{c != ignore_index} 1 - (2 A_c + smooth) / (B_c + T_c + smooth).
//      Forward: the workgroup's 256 x C tile of p^e goes to LDS, lane j sums column j in a fixed order (8 groups of 32 rows, then the 8
//      groups), one partial row [3C] per workgroup; the host wrapper sums the partial rows in double in a fixed order.  Backward: the
//      finish kernel leaves ca_c = 2 / (C den_c) and cb_c = e num_c / (C den_c^2); q_c = cb_c p_c^(e-1) - ca_c [t==c] is dL/dp_c and
//      the row applies the softmax Jacobian p_c (q_c - sum_k p_k q_k).
// No atomics anywhere: run-to-run bit-reproducible.  No host read: the means' denominators stay on the device (ptc_criteria_finish).
// LR_CP < C <= PTC_CRITERIA_CE_MAX_C: term a alone, on element-wise kernels in the style of loss.hip's ce_fwd_kernel / ce_bwd_kernel.
#include "ptc_common.h"
#include "loss_rows.h"
#include <math.h>

#define CR_CE PTC_CRITERIA_CE          // enum ptc_criteria_term (include/ptcore.h)
#define CR_FOCAL PTC_CRITERIA_FOCAL
#define CR_DICE PTC_CRITERIA_DICE
#define CR_HEAD 4          // partial row: ce loss, ce denominator, focal sum, focal rows; then with CR_DICE A[c], B[c], T[c]
#define CR_GROUPS 8        // the Dice column sums: 8 groups of 32 rows

struct CrArgs {
  int flags, c, dice_exp;
  float ce_eps, focal_gamma, focal_alpha;
  const float* ce_w;               // [c] or NULL (all ones)
  const float* focal_alpha_vec;    // [c] or NULL (focal_alpha)
  int64_t ignore_index;
};

// one element of term b at z: loss = a sigma(z)^gamma softplus(z) and its derivative in z
__device__ __forceinline__ void cr_focal(float z, float a, float gamma, float& loss, float& dz) {
  const float e = expf(-fabsf(z));
  const float l1 = log1pf(e);
  const float r = 1.f / (1.f + e);
  const float sp = fmaxf(z, 0.f) + l1;             // softplus(z)
  const float sn = fmaxf(-z, 0.f) + l1;            // softplus(-z) = -log sigma(z)
  const float sg = z >= 0.f ? r : e * r;           // sigma(z)
  const float sgn = z >= 0.f ? e * r : r;          // sigma(-z)
  const float mod = gamma == 0.f ? 1.f : expf(-gamma * sn);
  loss = a * mod * sp;
  dz = a * mod * (gamma * sgn * sp + sg);
}

__device__ __forceinline__ float cr_pow(float p, int e) { return e == 1 ? p : e == 2 ? p * p : p * p * p; }

// the four scalar sums of a workgroup, fixed order -> partial[0..4)
__device__ __forceinline__ void cr_reduce_head(float v0, float v1, float v2, float v3, float* __restrict__ out) {
  __shared__ float red[4][4];
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    v0 += __shfl_xor(v0, o, 64);
    v1 += __shfl_xor(v1, o, 64);
    v2 += __shfl_xor(v2, o, 64);
    v3 += __shfl_xor(v3, o, 64);
  }
  const int wave = threadIdx.x >> 6;
  if (ptc_lane() == 0) { red[0][wave] = v0; red[1][wave] = v1; red[2][wave] = v2; red[3][wave] = v3; }
  __syncthreads();
  if (threadIdx.x < 4) out[threadIdx.x] = (red[threadIdx.x][0] + red[threadIdx.x][1]) + (red[threadIdx.x][2] + red[threadIdx.x][3]);
}

template <typename T, int VB>
__global__ void __launch_bounds__(LR_THREADS)
crit_fwd_rows_kernel(const T* __restrict__ logits, int64_t row_stride, const int64_t* __restrict__ target, int64_t n, CrArgs a,
                     float* __restrict__ lsum, float* __restrict__ partial, int pw) {
  // CR_DICE: [256][c | 1] p^e, [256] p at the label, [256] label (-1: no part), [8][3][32] group sums; nothing otherwise
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int c = a.c, S = c | 1, tid = (int)threadIdx.x;
  const bool dice = (a.flags & CR_DICE) != 0;
  float* tile = reinterpret_cast<float*>(smem);
  float* pt = tile + LR_THREADS * S;
  int* cls = reinterpret_cast<int*>(pt + LR_THREADS);
  float* grp = reinterpret_cast<float*>(cls + LR_THREADS);
  const int64_t i = (int64_t)blockIdx.x * LR_THREADS + tid;
  float ce = 0.f, den = 0.f, fo = 0.f, rows = 0.f, dpt = 0.f;
  int dcls = -1;
  if (i < n) {
    float v[LR_CP];
    lr_load_row<T, VB>(logits + i * row_stride, c, v);
    float m = -INFINITY;
#pragma unroll
    for (int j = 0; j < LR_CP; ++j) if (j < c) m = fmaxf(m, v[j]);
    float ssum = 0.f;
#pragma unroll
    for (int j = 0; j < LR_CP; ++j) if (j < c) ssum += expf(v[j] - m);
    const float l = logf(ssum);       // log sum exp(x - m): -log p_j = l - (x_j - m), no rounding at the size of m
    lsum[i] = l;
    const int64_t t = target[i];
    const bool counted = t != a.ignore_index && t >= 0 && t < c;
    if ((a.flags & CR_CE) && counted) {
      const float wt = a.ce_w ? a.ce_w[t] : 1.f;
      ce = (1.f - a.ce_eps) * wt * (l - (lr_pick(v, (int)t) - m));
      if (a.ce_eps > 0.f) {
        float sm = 0.f;
#pragma unroll
        for (int j = 0; j < LR_CP; ++j) if (j < c) sm += (a.ce_w ? a.ce_w[j] : 1.f) * (l - (v[j] - m));
        ce += a.ce_eps / (float)c * sm;
      }
      den = wt;
    }
    if ((a.flags & CR_FOCAL) && counted) {
#pragma unroll
      for (int j = 0; j < LR_CP; ++j) {
        if (j < c) {
          const bool y = j == (int)t;
          const float al = a.focal_alpha_vec ? a.focal_alpha_vec[j] : a.focal_alpha;
          float lo, dz;
          cr_focal(y ? -v[j] : v[j], y ? al : 1.f - al, a.focal_gamma, lo, dz);
          fo += lo;
        }
      }
      rows = 1.f;
    }
    if (dice) {
      const bool part = t != a.ignore_index;
      const int tc = (int)(t < 0 ? 0 : t > c - 1 ? c - 1 : t);
#pragma unroll
      for (int j = 0; j < LR_CP; ++j) {
        if (j < c) {
          const float p = expf((v[j] - m) - l);
          tile[tid * S + j] = part ? cr_pow(p, a.dice_exp) : 0.f;
          dpt = j == tc ? p : dpt;
        }
      }
      dcls = part ? tc : -1;
    }
  } else if (dice) {
    for (int j = 0; j < c; ++j) tile[tid * S + j] = 0.f;
  }
  cr_reduce_head(ce, den, fo, rows, partial + (int64_t)blockIdx.x * pw);
  if (!dice) return;       // wave-uniform, and uniform over the workgroup
  pt[tid] = dpt;
  cls[tid] = dcls;
  __syncthreads();
  const int j = tid & 31, g = tid >> 5;
  float sa = 0.f, sb = 0.f, st = 0.f;
  if (j < c) {
    for (int r = g * 32; r < g * 32 + 32; ++r) {
      sb += tile[r * S + j];
      if (cls[r] == j) { sa += pt[r]; st += 1.f; }
    }
  }
  grp[(g * 3 + 0) * 32 + j] = sa;
  grp[(g * 3 + 1) * 32 + j] = sb;
  grp[(g * 3 + 2) * 32 + j] = st;
  __syncthreads();
  if (tid < 96 && j < c) {      // thread (q = tid / 32, j): quantity q of class j over the 8 groups, in order
    const int q = tid >> 5;
    float s = 0.f;
#pragma unroll
    for (int k = 0; k < CR_GROUPS; ++k) s += grp[(k * 3 + q) * 32 + j];
    partial[(int64_t)blockIdx.x * pw + CR_HEAD + q * c + j] = s;
  }
}

// coef: [0] s_ce  [1] s_focal  [2] W  [3] s_dice  [4, 4+c) ca  [4+c, 4+2c) cb   (ptc_criteria_finish); gscale[0] = the upstream gradient
template <typename T, int VB>
__global__ void __launch_bounds__(LR_THREADS)
crit_bwd_rows_kernel(const T* __restrict__ logits, int64_t row_stride, const int64_t* __restrict__ target, const float* __restrict__ lsum,
                     const float* __restrict__ coef, const float* __restrict__ gscale, int64_t n, CrArgs a, T* __restrict__ dlogits, int a16) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];       // [256][c] T: this workgroup's chunk of dlogits (dense rows)
  const int c = a.c;
  const int64_t row0 = (int64_t)blockIdx.x * LR_THREADS, i = row0 + threadIdx.x;
  if (i < n) {
    float v[LR_CP], p[LR_CP];
    lr_load_row<T, VB>(logits + i * row_stride, c, v);
    const int64_t t = target[i];
    const float l = lsum[i], g = gscale[0];
    float m = -INFINITY;
#pragma unroll
    for (int j = 0; j < LR_CP; ++j) if (j < c) m = fmaxf(m, v[j]);
    const bool counted = t != a.ignore_index && t >= 0 && t < c;
    const bool do_ce = (a.flags & CR_CE) && counted, do_focal = (a.flags & CR_FOCAL) && counted;
    const bool do_dice = (a.flags & CR_DICE) && t != a.ignore_index;
    const int tc = (int)(t < 0 ? 0 : t > c - 1 ? c - 1 : t);
#pragma unroll
    for (int j = 0; j < LR_CP; ++j) p[j] = j < c ? expf((v[j] - m) - l) : 0.f;
    const float* ca = coef + 4;
    const float* cb = coef + 4 + c;
    // Dice: p_c (q_c - sum_k p_k q_k).  A confident row (p_m ~ 1 at its largest logit, class jm) cancels in q_m - p_m q_m: there the
    // difference is q_m (1 - p_m) - rest with rest = sum_{k != jm} p_k q_k and 1 - p_m = sum_{k != jm} p_k; elsewhere q_c - (p_m q_m + rest)
    float rest = 0.f, pq_m = 0.f, omp_m = 0.f;
    int jm = 0;
    if (do_dice) {
#pragma unroll
      for (int j = LR_CP - 1; j >= 0; --j) if (j < c) jm = v[j] == m ? j : jm;
#pragma unroll
      for (int j = 0; j < LR_CP; ++j) {
        if (j < c) {
          const float pe1 = a.dice_exp == 1 ? 1.f : a.dice_exp == 2 ? p[j] : p[j] * p[j];
          const float pq = p[j] * (cb[j] * pe1 - (j == tc ? ca[j] : 0.f));
          pq_m = j == jm ? pq : pq_m;
          rest += j == jm ? 0.f : pq;
          omp_m += j == jm ? 0.f : p[j];
        }
      }
    }
    const float s_ce = coef[0] * g, s_focal = coef[1] * g, s_dice = coef[3] * g, ec = a.ce_eps / (float)c;
    // k_t (p_c - [c==t]) + k_w p_c - ec w_c, with p_t - 1 from expm1: a confident row's gradient is that small difference
    float k_w = 0.f, k_t = 0.f, pm1 = 0.f;
    if (do_ce) {
      const float wt = a.ce_w ? a.ce_w[t] : 1.f;
      k_t = (1.f - a.ce_eps) * wt;
      k_w = ec * coef[2];
      pm1 = expm1f((lr_pick(v, (int)t) - m) - l);
    }
    T* drow = reinterpret_cast<T*>(smem) + (int)threadIdx.x * c;
#pragma unroll
    for (int j = 0; j < LR_CP; ++j) {
      if (j < c) {
        float d = 0.f;
        if (do_ce) {
          float q = k_t * (j == (int)t ? pm1 : p[j]);
          if (a.ce_eps > 0.f) q += k_w * p[j] - ec * (a.ce_w ? a.ce_w[j] : 1.f);
          d = s_ce * q;
        }
        if (do_focal) {
          const bool y = j == (int)t;
          const float al = a.focal_alpha_vec ? a.focal_alpha_vec[j] : a.focal_alpha;
          float lo, dz;
          cr_focal(y ? -v[j] : v[j], y ? al : 1.f - al, a.focal_gamma, lo, dz);
          d += s_focal * (y ? -dz : dz);
        }
        if (do_dice) {
          const float pe1 = a.dice_exp == 1 ? 1.f : a.dice_exp == 2 ? p[j] : p[j] * p[j];
          const float q = cb[j] * pe1 - (j == tc ? ca[j] : 0.f);
          d += s_dice * p[j] * (j == jm ? q * omp_m - rest : q - (pq_m + rest));
        }
        drow[j] = ptc_from_float<T>(d);
      }
    }
  }
  __syncthreads();
  const int64_t rows = (n - row0) < LR_THREADS ? (n - row0) : LR_THREADS;
  lr_copy_out<T>(smem, dlogits + row0 * c, (int)rows * c, a16 != 0);
}

// LR_CP < C <= PTC_CRITERIA_CE_MAX_C: term a alone, element-wise over the row in global memory (three passes, as ce_fwd_kernel)
template <typename T>
__global__ void __launch_bounds__(256)
crit_ce_fwd_kernel(const T* __restrict__ logits, int64_t row_stride, const int64_t* __restrict__ target, int64_t n, CrArgs a,
                   float* __restrict__ lsum, float* __restrict__ partial, int pw) {
  const int c = a.c;
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  float ce = 0.f, den = 0.f;
  if (i < n) {
    const T* row = logits + i * row_stride;
    float m = -INFINITY;
    for (int j = 0; j < c; ++j) m = fmaxf(m, ptc_to_float(row[j]));
    double ssum = 0.;         // up to 1024 terms: the running sums are kept in double
    for (int j = 0; j < c; ++j) ssum += (double)expf(ptc_to_float(row[j]) - m);
    const float l = logf((float)ssum);
    lsum[i] = l;
    const int64_t t = target[i];
    if (t != a.ignore_index && t >= 0 && t < c) {
      const float wt = a.ce_w ? a.ce_w[t] : 1.f;
      ce = (1.f - a.ce_eps) * wt * (l - (ptc_to_float(row[t]) - m));
      if (a.ce_eps > 0.f) {
        double sm = 0.;
        for (int j = 0; j < c; ++j) sm += (double)((a.ce_w ? a.ce_w[j] : 1.f) * (l - (ptc_to_float(row[j]) - m)));
        ce += a.ce_eps / (float)c * (float)sm;
      }
      den = wt;
    }
  }
  cr_reduce_head(ce, den, 0.f, 0.f, partial + (int64_t)blockIdx.x * pw);
}

template <typename T>
__global__ void __launch_bounds__(256)
crit_ce_bwd_kernel(const T* __restrict__ logits, int64_t row_stride, const int64_t* __restrict__ target, const float* __restrict__ lsum,
                   const float* __restrict__ coef, const float* __restrict__ gscale, int64_t n, CrArgs a, T* __restrict__ dlogits) {
  const int c = a.c;
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const T* row = logits + i * row_stride;
  T* drow = dlogits + i * c;
  const int64_t t = target[i];
  const bool counted = t != a.ignore_index && t >= 0 && t < c;
  const float l = lsum[i], ec = a.ce_eps / (float)c;
  float m = -INFINITY;
  if (counted) for (int j = 0; j < c; ++j) m = fmaxf(m, ptc_to_float(row[j]));
  const float s = counted ? coef[0] * gscale[0] : 0.f;
  const float k_t = counted ? (1.f - a.ce_eps) * (a.ce_w ? a.ce_w[t] : 1.f) : 0.f;
  const float k_w = ec * coef[2];
  for (int j = 0; j < c; ++j) {
    float d = 0.f;
    if (counted) {
      const float z = (ptc_to_float(row[j]) - m) - l;
      float q = k_t * (j == t ? expm1f(z) : expf(z));
      if (a.ce_eps > 0.f) q += k_w * expf(z) - ec * (a.ce_w ? a.ce_w[j] : 1.f);
      d = s * q;
    }
    drow[j] = ptc_from_float<T>(d);
  }
}

// sums [pw] double (the partial rows summed by the caller) -> out[4] = total, ce, focal, dice (each already times its loss_weight) and
// coef [4 + 2c] for the backward.  One thread: C <= 1024 values.
__global__ void __launch_bounds__(64)
crit_finish_kernel(const double* __restrict__ sums, CrArgs a, int ce_sum, double lw_ce, double lw_focal, double lw_dice, double smooth,
                   float* __restrict__ out, float* __restrict__ coef) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  const int c = a.c;
  double l_ce = 0., l_focal = 0., l_dice = 0., s_ce = 0., s_focal = 0., w_sum = (double)c;
  if (a.flags & CR_CE) {
    if (a.ce_w) {
      w_sum = 0.;
      for (int j = 0; j < c; ++j) w_sum += (double)a.ce_w[j];
    }
    // mean over a zero denominator (nothing counted, or zero-weight classes only): ATen's weighted mean is 0 / 0 there, so the loss is
    // nan -- with smoothing too -- and so is the gradient of every counted row
    const bool empty = !ce_sum && sums[1] == 0.;
    l_ce = empty ? (double)NAN : lw_ce * (ce_sum ? sums[0] : sums[0] / sums[1]);
    s_ce = empty ? (double)NAN : ce_sum ? lw_ce : lw_ce / sums[1];
  }
  if (a.flags & CR_FOCAL) {
    const double cnt = sums[3] * (double)c;
    s_focal = cnt > 0. ? lw_focal / cnt : 0.;
    l_focal = s_focal * sums[2];
  }
  if (a.flags & CR_DICE) {
    const double* A = sums + CR_HEAD;
    const double* B = A + c;
    const double* Tc = B + c;
    double acc = 0.;
    for (int j = 0; j < c; ++j) {
      double ca = 0., cb = 0.;
      if ((int64_t)j != a.ignore_index) {
        const double num = 2. * A[j] + smooth, den = B[j] + Tc[j] + smooth;
        acc += 1. - num / den;
        ca = 2. / ((double)c * den);
        cb = (double)a.dice_exp * num / ((double)c * den * den);
      }
      coef[4 + j] = (float)ca;
      coef[4 + c + j] = (float)cb;
    }
    l_dice = lw_dice * acc / (double)c;
  }
  coef[0] = (float)s_ce;
  coef[1] = (float)s_focal;
  coef[2] = (float)w_sum;
  coef[3] = (float)lw_dice;
  out[0] = (float)(l_ce + l_focal + l_dice);
  out[1] = (float)l_ce;
  out[2] = (float)l_focal;
  out[3] = (float)l_dice;
}

// ------------------------------------------------------------------------------------------------
static inline size_t cr_fwd_lds(int c, int flags) {
  if (!(flags & CR_DICE)) return 0;
  return ((size_t)LR_THREADS * (size_t)(c | 1) + 2 * LR_THREADS + CR_GROUPS * 3 * 32) * sizeof(float);
}

static int cr_check(const char* who, int64_t n, int c, int64_t row_stride, int flags, int dice_exp) {
  PTC_REQUIRE(n >= 0 && c >= 1 && row_stride >= c, PTC_EINVAL, "%s: bad sizes", who);
  PTC_REQUIRE(c <= PTC_CRITERIA_CE_MAX_C, PTC_EINVAL, "%s: %d classes (at most %d)", who, c, PTC_CRITERIA_CE_MAX_C);
  PTC_REQUIRE(flags > 0 && flags <= (CR_CE | CR_FOCAL | CR_DICE), PTC_EINVAL, "%s: bad term flags %d", who, flags);
  PTC_REQUIRE(c <= LR_CP || flags == CR_CE, PTC_EINVAL, "%s: more than %d classes take the cross-entropy term alone", who, LR_CP);
  PTC_REQUIRE(!(flags & CR_DICE) || (dice_exp >= 1 && dice_exp <= 3), PTC_EINVAL, "%s: Dice exponent %d (1, 2 or 3)", who, dice_exp);
  return PTC_OK;
}

static inline CrArgs cr_args(int c, int flags, int64_t ignore_index, const float* ce_w, double ce_eps, const float* alpha_vec, double alpha,
                             double gamma, int dice_exp) {
  CrArgs a;
  a.flags = flags;
  a.c = c;
  a.dice_exp = dice_exp;
  a.ce_eps = (float)ce_eps;
  a.focal_gamma = (float)gamma;
  a.focal_alpha = (float)alpha;
  a.ce_w = (flags & CR_CE) ? ce_w : nullptr;
  a.focal_alpha_vec = (flags & CR_FOCAL) ? alpha_vec : nullptr;
  a.ignore_index = ignore_index;
  return a;
}

extern "C" int64_t ptc_criteria_partials(int64_t n) { return n > 0 ? ptc_cdiv(n, LR_THREADS) : 1; }

extern "C" int64_t ptc_criteria_partial_width(int c, int flags) { return CR_HEAD + ((flags & CR_DICE) ? 3 * (int64_t)c : 0); }

extern "C" int ptc_criteria_fwd(const void* logits, int64_t row_stride, const int64_t* target, int64_t n, int c, int dtype,
                                int64_t ignore_index, int flags, const float* ce_weight, double label_smoothing, const float* focal_alpha_vec,
                                double focal_alpha, double focal_gamma, int dice_exponent, float* lsum, float* partial, ptc_stream_t stream) {
  if (int rc = cr_check("ptc_criteria_fwd", n, c, row_stride, flags, dice_exponent)) return rc;
  PTC_REQUIRE(partial != nullptr, PTC_EINVAL, "ptc_criteria_fwd: null buffer");
  hipStream_t s = (hipStream_t)stream;
  const int pw = (int)ptc_criteria_partial_width(c, flags);
  if (n == 0) {
    PTC_HIP(hipMemsetAsync(partial, 0, (size_t)pw * sizeof(float), s));
    return PTC_OK;
  }
  PTC_REQUIRE(logits && target && lsum, PTC_EINVAL, "ptc_criteria_fwd: null buffer");
  const CrArgs a = cr_args(c, flags, ignore_index, ce_weight, label_smoothing, focal_alpha_vec, focal_alpha, focal_gamma, dice_exponent);
  const unsigned grid = (unsigned)ptc_cdiv(n, LR_THREADS);
  if (c <= LR_CP) {
    const int vb = lr_vec_bytes(logits, row_stride, c, ptc_dtype_size(dtype));
    const size_t lds = cr_fwd_lds(c, flags);
    PTC_DISPATCH_DTYPE(dtype, T, LR_DISPATCH_VB(vb, VB, hipLaunchKernelGGL((crit_fwd_rows_kernel<T, VB>), dim3(grid), dim3(LR_THREADS), lds, s,
                                                                         (const T*)logits, row_stride, target, n, a, lsum, partial, pw)));
    PTC_CHECK_LAUNCH("crit_fwd_rows_kernel");
    return PTC_OK;
  }
  PTC_DISPATCH_DTYPE(dtype, T, hipLaunchKernelGGL(crit_ce_fwd_kernel<T>, dim3(grid), dim3(256), 0, s, (const T*)logits, row_stride, target, n,
                                                   a, lsum, partial, pw));
  PTC_CHECK_LAUNCH("crit_ce_fwd_kernel");
  return PTC_OK;
}

extern "C" int ptc_criteria_finish(const double* sums, int c, int flags, int64_t ignore_index, const float* ce_weight, int ce_reduction_sum,
                                   double ce_loss_weight, double focal_loss_weight, double dice_loss_weight, double dice_smooth,
                                   int dice_exponent, float* out, float* coef, ptc_stream_t stream) {
  if (int rc = cr_check("ptc_criteria_finish", 0, c, c, flags, dice_exponent)) return rc;
  PTC_REQUIRE(sums && out && coef, PTC_EINVAL, "ptc_criteria_finish: null buffer");
  const CrArgs a = cr_args(c, flags, ignore_index, ce_weight, 0., nullptr, 0., 0., dice_exponent);
  hipLaunchKernelGGL(crit_finish_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, sums, a, ce_reduction_sum, ce_loss_weight,
                     focal_loss_weight, dice_loss_weight, dice_smooth, out, coef);
  PTC_CHECK_LAUNCH("crit_finish_kernel");
  return PTC_OK;
}

extern "C" int ptc_criteria_bwd(const void* logits, int64_t row_stride, const int64_t* target, const float* lsum, const float* coef,
                                const float* gscale, int64_t n, int c, int dtype, int64_t ignore_index, int flags, const float* ce_weight,
                                double label_smoothing, const float* focal_alpha_vec, double focal_alpha, double focal_gamma,
                                int dice_exponent, void* dlogits, ptc_stream_t stream) {
  if (int rc = cr_check("ptc_criteria_bwd", n, c, row_stride, flags, dice_exponent)) return rc;
  if (n == 0) return PTC_OK;
  PTC_REQUIRE(logits && target && lsum && coef && gscale && dlogits, PTC_EINVAL, "ptc_criteria_bwd: null buffer");
  const CrArgs a = cr_args(c, flags, ignore_index, ce_weight, label_smoothing, focal_alpha_vec, focal_alpha, focal_gamma, dice_exponent);
  hipStream_t s = (hipStream_t)stream;
  const unsigned grid = (unsigned)ptc_cdiv(n, LR_THREADS);
  if (c <= LR_CP) {
    const int vb = lr_vec_bytes(logits, row_stride, c, ptc_dtype_size(dtype));
    const int a16 = ((uintptr_t)dlogits & 15) == 0;
    const size_t lds = (size_t)LR_THREADS * c * ptc_dtype_size(dtype);
    PTC_DISPATCH_DTYPE(dtype, T, LR_DISPATCH_VB(vb, VB, hipLaunchKernelGGL((crit_bwd_rows_kernel<T, VB>), dim3(grid), dim3(LR_THREADS), lds, s,
                                                                         (const T*)logits, row_stride, target, lsum, coef, gscale, n, a,
                                                                         (T*)dlogits, a16)));
    PTC_CHECK_LAUNCH("crit_bwd_rows_kernel");
    return PTC_OK;
  }
  PTC_DISPATCH_DTYPE(dtype, T, hipLaunchKernelGGL(crit_ce_bwd_kernel<T>, dim3(grid), dim3(256), 0, s, (const T*)logits, row_stride, target, lsum,
                                                   coef, gscale, n, a, (T*)dlogits));
  PTC_CHECK_LAUNCH("crit_ce_bwd_kernel");
  return PTC_OK;
}
