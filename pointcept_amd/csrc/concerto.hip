// concerto.hip -- the 2D-3D alignment branch of Concerto-v1m1 (pointcept/models/concerto/concerto_v1m1_base.py:528-573, :745-866).
//
//   cc_pool_corr_kernel      pool_corr for ONE pooling level and ALL images: a thread owns (cluster, image), walks the cluster's members
//                            in the order of the cluster CSR and sums in double -- at the first level (integer pixel coordinates) the
//                            sums are exact and the one division rounds as fp32's own does (a double quotient of two fp32 values
//                            rounded to fp32 is the correctly rounded fp32 quotient: 53 >= 2 * 24 + 2).
//   cc_pair_keys_kernel      the patch key of every (point, image) pair of the selected rows, or `sentinel` (above every key) for a
//                            pair that is invalid or lies outside its image / its scene's images; the engine's radix sort and the
//                            run-numbering kernels of the pooling maps (maps.hip) turn the keys into unique ids + CSR.
//   cc_patch_mean_bwd_kernel d feat3d[p] = sum over p's at most V patches of d mean3d[u] / count[u]: gather form, no atomics.
//   cc_align_kernel          10 * mean_u (1 - cos(x_u - mean x_u, y_u - mean y_u)) with x_u = feature2d[ids[u]] read through the index.
//                            ONE WAVE owns a row: lane l holds the 8-value groups l, l + 64, ... of both rows in registers (16-byte
//                            loads where D is a multiple of 8 and the rows are 16-byte aligned, scalar loads otherwise), the two
//                            means, the centred dot and the two squared norms are xor butterflies (no LDS), 1 - cos goes to row[u]
//                            and dy -- closed form, below -- is written from the same registers.  cos follows ATen's
//                            cosine_similarity: sum_j (x_j / max(|x|, eps)) (y_j / max(|y|, eps)), each norm clamped on its own, and
//                            the clamp passes the gradient when |y| >= eps.
//                                a = xc / max(|xc|, eps), cy = max(|yc|, eps), k = |yc| >= eps ? cos / (cy |yc|) : 0
//                                g = a / cy - k yc;  with the shift g <- g - mean(g);  dy = -(10 / U) g
//   cc_sum_rows_kernel       the [U] buffer summed in a fixed order (per-thread strided sums in double, then a tree): reproducible.
#include "ptc_common.h"

#include <math.h>

#define CC_THREADS 256
#define CC_GROUP 8                      // values of one register group (16 bytes of a 16-bit row, 32 of an fp32 row)
#define CC_MAX_NP 4                     // groups per lane: D <= 64 * 8 * 4
#define CC_MAX_D (PTC_WAVE * CC_GROUP * CC_MAX_NP)

// ------------------------------------------------------------------------------------------------ pooled correspondence
template <typename T>
__global__ void __launch_bounds__(CC_THREADS)
cc_pool_corr_kernel(const T* __restrict__ corr, int64_t n, int v, const int64_t* __restrict__ perm, const int64_t* __restrict__ idx_ptr,
                    int64_t m, float* __restrict__ out) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= m * v) return;
  const int64_t cl = t / v;
  const int vi = (int)(t - cl * v);
  const int64_t r0 = idx_ptr[cl], r1 = idx_ptr[cl + 1];
  double s0 = 0.0, s1 = 0.0;
  int64_t cnt = 0;
  const T none = (T)-1;
  for (int64_t r = r0; r < r1; ++r) {
    const int64_t p = perm ? perm[r] : r;
    if ((uint64_t)p >= (uint64_t)n) continue;
    const T a = corr[(p * v + vi) * 2], b = corr[(p * v + vi) * 2 + 1];
    const bool va = a != none, vb = b != none;
    cnt += (va && vb) ? 1 : 0;
    s0 += va ? (double)a : 0.0;          // the reference zeroes the -1 entries one by one: a half-valid pair still adds its other half
    s1 += vb ? (double)b : 0.0;
  }
  out[t * 2] = cnt ? (float)(s0 / (double)cnt) : -1.f;
  out[t * 2 + 1] = cnt ? (float)(s1 / (double)cnt) : -1.f;
}

// ------------------------------------------------------------------------------------------------ patch keys
__global__ void __launch_bounds__(CC_THREADS)
cc_pair_keys_kernel(const float* __restrict__ corr, int64_t n, const int64_t* __restrict__ rows, const int64_t* __restrict__ scene,
                    const int64_t* __restrict__ img_offset, const int64_t* __restrict__ img_num, int64_t ns, int nb, int v, int ph, int pw,
                    int64_t sentinel, int64_t* __restrict__ keys) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= ns * v) return;
  const int64_t i = t / v;
  const int vi = (int)(t - i * v);
  const int64_t p = rows ? rows[i] : i;
  const int64_t sc = scene[i];
  int64_t key = sentinel;
  if ((uint64_t)p < (uint64_t)n && (uint64_t)sc < (uint64_t)nb) {
    const float a = corr[(p * v + vi) * 2], b = corr[(p * v + vi) * 2 + 1];
    const bool valid = a != -1.f || b != -1.f;
    // trunc(a) in [0, ph)  <=>  -1 < a < ph (a NaN fails both)
    const bool inside = a > -1.f && a < (float)ph && b > -1.f && b < (float)pw && (int64_t)vi < img_num[sc];
    if (valid && inside) key = ((img_offset[sc] + vi) * ph + (int64_t)truncf(a)) * pw + (int64_t)truncf(b);
  }
  keys[t] = key;
}

// ------------------------------------------------------------------------------------------------ patch means, backward
template <typename T, int W> struct alignas(sizeof(T) * W) CcPack { T v[W]; };

template <typename T, int W>
__global__ void __launch_bounds__(CC_THREADS)
cc_patch_mean_bwd_kernel(const T* __restrict__ dmean, const int64_t* __restrict__ pair_patch, const int64_t* __restrict__ indptr,
                         const int64_t* __restrict__ rows, int64_t ns, int64_t n_out, int v, int c, int64_t u, T* __restrict__ dfeat) {
  const int cpr = c / W;
  const int64_t total = ns * cpr;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += stride) {
    const int64_t i = t / cpr;
    const int ch = (int)(t - i * cpr) * W;
    const int64_t p = rows ? rows[i] : i;
    if ((uint64_t)p >= (uint64_t)n_out) continue;
    float acc[W];
#pragma unroll
    for (int j = 0; j < W; ++j) acc[j] = 0.f;
    for (int vi = 0; vi < v; ++vi) {
      const int64_t q = pair_patch[i * v + vi];
      if ((uint64_t)q >= (uint64_t)u) continue;
      const float inv = 1.f / (float)(indptr[q + 1] - indptr[q]);
      const CcPack<T, W> g = *reinterpret_cast<const CcPack<T, W>*>(dmean + q * c + ch);
#pragma unroll
      for (int j = 0; j < W; ++j) acc[j] = fmaf(ptc_to_float(g.v[j]), inv, acc[j]);
    }
    CcPack<T, W> o;
#pragma unroll
    for (int j = 0; j < W; ++j) o.v[j] = ptc_from_float<T>(acc[j]);
    *reinterpret_cast<CcPack<T, W>*>(dfeat + p * c + ch) = o;
  }
}

// ------------------------------------------------------------------------------------------------ centred cosine
__device__ __forceinline__ float cc_wave_sum(float v) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off);
  return v;
}

// the lane's groups of a row: group i covers the columns (i * 64 + lane) * 8 .. + 7; columns at or past d read as 0
template <typename T, int NP>
__device__ __forceinline__ void cc_load_row(const T* __restrict__ row, int d, bool vec, int lane, float (&o)[NP * CC_GROUP]) {
#pragma unroll
  for (int i = 0; i < NP; ++i) {
    const int col = (i * PTC_WAVE + lane) * CC_GROUP;
    if (vec) {
      if (col < d) {
        constexpr int H = 16 / sizeof(T);        // values of one 16-byte load
#pragma unroll
        for (int h = 0; h < CC_GROUP / H; ++h) {
          const CcPack<T, H> q = *reinterpret_cast<const CcPack<T, H>*>(row + col + h * H);
#pragma unroll
          for (int j = 0; j < H; ++j) o[i * CC_GROUP + h * H + j] = ptc_to_float(q.v[j]);
        }
      } else {
#pragma unroll
        for (int j = 0; j < CC_GROUP; ++j) o[i * CC_GROUP + j] = 0.f;
      }
    } else {
#pragma unroll
      for (int j = 0; j < CC_GROUP; ++j) o[i * CC_GROUP + j] = (col + j < d) ? ptc_to_float(row[col + j]) : 0.f;
    }
  }
}

template <typename T, int NP>
__device__ __forceinline__ void cc_store_row(T* __restrict__ row, int d, bool vec, int lane, const float (&o)[NP * CC_GROUP]) {
#pragma unroll
  for (int i = 0; i < NP; ++i) {
    const int col = (i * PTC_WAVE + lane) * CC_GROUP;
    if (vec) {
      if (col < d) {
        constexpr int H = 16 / sizeof(T);
#pragma unroll
        for (int h = 0; h < CC_GROUP / H; ++h) {
          CcPack<T, H> q;
#pragma unroll
          for (int j = 0; j < H; ++j) q.v[j] = ptc_from_float<T>(o[i * CC_GROUP + h * H + j]);
          *reinterpret_cast<CcPack<T, H>*>(row + col + h * H) = q;
        }
      }
    } else {
#pragma unroll
      for (int j = 0; j < CC_GROUP; ++j)
        if (col + j < d) row[col + j] = ptc_from_float<T>(o[i * CC_GROUP + j]);
    }
  }
}

template <typename TX, typename TY, int NP>
__global__ void __launch_bounds__(CC_THREADS)
cc_align_kernel(const TX* __restrict__ x, int64_t nx, const int64_t* __restrict__ ids, const TY* __restrict__ y, int64_t u, int d, int shift,
                float eps, float scale, bool vec_x, bool vec_y, float* __restrict__ row_out, TY* __restrict__ dy) {
  constexpr int NV = NP * CC_GROUP;
  const int lane = threadIdx.x & 63;
  const int64_t r = (int64_t)blockIdx.x * (CC_THREADS / PTC_WAVE) + (threadIdx.x >> 6);
  const bool in = r < u;                                   // wave-uniform; a wave past the end computes on zeros and stores nothing
  const int64_t id = in ? ids[r] : -1;
  const bool live = (uint64_t)id < (uint64_t)nx;
  float xv[NV], yv[NV];
  cc_load_row<TX, NP>(x + (live ? id : 0) * d, live ? d : 0, vec_x, lane, xv);
  cc_load_row<TY, NP>(y + (in ? r : 0) * d, live ? d : 0, vec_y, lane, yv);
  const float fd = (float)d;
  if (shift) {
    float sx = 0.f, sy = 0.f;
#pragma unroll
    for (int j = 0; j < NV; ++j) { sx += xv[j]; sy += yv[j]; }
    // a true division: a constant row (exact sum) must centre to exactly zero, as it does in torch -- with sum * (1 / d) it centres
    // to 1e-8, which the eps clamp then divides by 1e-6
    const float mx = cc_wave_sum(sx) / fd, my = cc_wave_sum(sy) / fd;
#pragma unroll
    for (int i = 0; i < NP; ++i) {
#pragma unroll
      for (int j = 0; j < CC_GROUP; ++j) {
        const bool on = live && (i * PTC_WAVE + lane) * CC_GROUP + j < d;
        xv[i * CC_GROUP + j] = on ? xv[i * CC_GROUP + j] - mx : 0.f;
        yv[i * CC_GROUP + j] = on ? yv[i * CC_GROUP + j] - my : 0.f;
      }
    }
  }
  float dot = 0.f, xx = 0.f, yy = 0.f;
#pragma unroll
  for (int j = 0; j < NV; ++j) {
    dot = fmaf(xv[j], yv[j], dot);
    xx = fmaf(xv[j], xv[j], xx);
    yy = fmaf(yv[j], yv[j], yy);
  }
  dot = cc_wave_sum(dot);
  xx = cc_wave_sum(xx);
  yy = cc_wave_sum(yy);
  const float nxn = sqrtf(xx), nyn = sqrtf(yy);
  const float cx = fmaxf(nxn, eps), cy = fmaxf(nyn, eps);
  const float cosv = dot / (cx * cy);
  if (in && lane == 0) row_out[r] = live ? 1.f - cosv : 0.f;
  if (!dy) return;
  const float k = (nyn >= eps && nyn > 0.f) ? cosv / (cy * nyn) : 0.f;
  const float ia = 1.f / (cx * cy);
  float sg = 0.f;
#pragma unroll
  for (int j = 0; j < NV; ++j) {
    yv[j] = xv[j] * ia - k * yv[j];
    sg += yv[j];
  }
  const float mg = shift ? cc_wave_sum(sg) / fd : 0.f;
#pragma unroll
  for (int j = 0; j < NV; ++j) yv[j] = live ? -scale * (yv[j] - mg) : 0.f;
  if (in) cc_store_row<TY, NP>(dy + r * d, d, vec_y, lane, yv);
}

__global__ void __launch_bounds__(CC_THREADS)
cc_sum_rows_kernel(const float* __restrict__ row, int64_t u, double scale, float* __restrict__ loss) {
  __shared__ double red[CC_THREADS];
  double s = 0.0;
  for (int64_t i = threadIdx.x; i < u; i += CC_THREADS) s += (double)row[i];
  red[threadIdx.x] = s;
  __syncthreads();
  for (int half = CC_THREADS / 2; half >= 1; half >>= 1) {
    if ((int)threadIdx.x < half) red[threadIdx.x] += red[threadIdx.x + half];
    __syncthreads();
  }
  if (threadIdx.x == 0) loss[0] = (float)(red[0] * scale);
}

// ------------------------------------------------------------------------------------------------ entry points
static inline unsigned cc_grid(int64_t total) {
  const int64_t g = ptc_cdiv(total, CC_THREADS);
  return (unsigned)(g < 1 ? 1 : g);
}

extern "C" int ptc_concerto_pool_corr(const void* corr, int ctype, int64_t n, int v, const int64_t* perm, const int64_t* idx_ptr, int64_t m,
                                      float* out, ptc_stream_t stream) {
  PTC_REQUIRE(n >= 0 && m >= 0 && v >= 0, PTC_EINVAL, "ptc_concerto_pool_corr: n=%lld m=%lld v=%d", (long long)n, (long long)m, v);
  PTC_REQUIRE(ctype >= PTC_CORR_F32 && ctype <= PTC_CORR_I64, PTC_EINVAL, "ptc_concerto_pool_corr: correspondence type %d (enum ptc_corr_type)", ctype);
  PTC_REQUIRE(m * (int64_t)v < ((int64_t)1 << 31) * CC_THREADS, PTC_EINVAL, "ptc_concerto_pool_corr: too many (cluster, image) pairs");
  if (m == 0 || v == 0) return PTC_OK;
  PTC_REQUIRE((corr || n == 0) && idx_ptr && out, PTC_EINVAL, "ptc_concerto_pool_corr: null buffer");
  hipStream_t st = (hipStream_t)stream;
  const unsigned g = cc_grid(m * v);
  if (ctype == PTC_CORR_F32)
    hipLaunchKernelGGL(cc_pool_corr_kernel<float>, dim3(g), dim3(CC_THREADS), 0, st, (const float*)corr, n, v, perm, idx_ptr, m, out);
  else if (ctype == PTC_CORR_I32)
    hipLaunchKernelGGL(cc_pool_corr_kernel<int32_t>, dim3(g), dim3(CC_THREADS), 0, st, (const int32_t*)corr, n, v, perm, idx_ptr, m, out);
  else
    hipLaunchKernelGGL(cc_pool_corr_kernel<int64_t>, dim3(g), dim3(CC_THREADS), 0, st, (const int64_t*)corr, n, v, perm, idx_ptr, m, out);
  PTC_CHECK_LAUNCH("cc_pool_corr_kernel");
  return PTC_OK;
}

extern "C" int ptc_concerto_pair_keys(const float* corr, int64_t n, const int64_t* rows, const int64_t* scene, const int64_t* img_offset,
                                      const int64_t* img_num, int64_t ns, int nb, int v, int patch_h, int patch_w, int64_t sentinel,
                                      int64_t* keys, ptc_stream_t stream) {
  PTC_REQUIRE(n >= 0 && ns >= 0 && nb >= 0 && v >= 0 && patch_h >= 1 && patch_w >= 1, PTC_EINVAL, "ptc_concerto_pair_keys: bad sizes");
  PTC_REQUIRE(ns * (int64_t)v < ((int64_t)1 << 31) * CC_THREADS, PTC_EINVAL, "ptc_concerto_pair_keys: too many pairs");
  if (ns == 0 || v == 0) return PTC_OK;
  PTC_REQUIRE(corr && scene && img_offset && img_num && keys, PTC_EINVAL, "ptc_concerto_pair_keys: null buffer");
  hipLaunchKernelGGL(cc_pair_keys_kernel, dim3(cc_grid(ns * v)), dim3(CC_THREADS), 0, (hipStream_t)stream, corr, n, rows, scene, img_offset,
                     img_num, ns, nb, v, patch_h, patch_w, sentinel, keys);
  PTC_CHECK_LAUNCH("cc_pair_keys_kernel");
  return PTC_OK;
}

template <typename T>
static int cc_mean_bwd(const void* dmean, const int64_t* pair_patch, const int64_t* indptr, const int64_t* rows, int64_t ns, int64_t n_out,
                       int v, int c, int64_t u, void* dfeat, hipStream_t st) {
  const bool vec = c % 4 == 0 && ((uintptr_t)dmean | (uintptr_t)dfeat) % (sizeof(T) * 4) == 0;
  const int64_t total = ns * (vec ? c / 4 : c);
  int64_t g = ptc_cdiv(total, CC_THREADS);
  g = g < 1 ? 1 : (g > 65536 ? 65536 : g);
  if (vec)
    hipLaunchKernelGGL((cc_patch_mean_bwd_kernel<T, 4>), dim3((unsigned)g), dim3(CC_THREADS), 0, st, (const T*)dmean, pair_patch, indptr, rows,
                       ns, n_out, v, c, u, (T*)dfeat);
  else
    hipLaunchKernelGGL((cc_patch_mean_bwd_kernel<T, 1>), dim3((unsigned)g), dim3(CC_THREADS), 0, st, (const T*)dmean, pair_patch, indptr, rows,
                       ns, n_out, v, c, u, (T*)dfeat);
  PTC_CHECK_LAUNCH("cc_patch_mean_bwd_kernel");
  return PTC_OK;
}

extern "C" int ptc_concerto_patch_mean_bwd(const void* dmean, int dtype, const int64_t* pair_patch, const int64_t* indptr, const int64_t* rows,
                                           int64_t ns, int64_t n_out, int v, int c, int64_t u, void* dfeat, ptc_stream_t stream) {
  PTC_REQUIRE(ns >= 0 && n_out >= 0 && v >= 0 && c >= 1 && u >= 0, PTC_EINVAL, "ptc_concerto_patch_mean_bwd: bad sizes");
  if (ns == 0) return PTC_OK;
  PTC_REQUIRE((dmean || u == 0) && (pair_patch || v == 0) && indptr && dfeat, PTC_EINVAL, "ptc_concerto_patch_mean_bwd: null buffer");
  PTC_DISPATCH_DTYPE(dtype, T, return cc_mean_bwd<T>(dmean, pair_patch, indptr, rows, ns, n_out, v, c, u, dfeat, (hipStream_t)stream));
  return PTC_OK;
}

extern "C" int ptc_concerto_align_supported(int d) { return d >= 1 && d <= CC_MAX_D; }

#define CC_DISPATCH_NP(d, NP, ...)                                                    \
  switch (((d) + PTC_WAVE * CC_GROUP - 1) / (PTC_WAVE * CC_GROUP)) {                  \
    case 1: { constexpr int NP = 1; __VA_ARGS__; } break;                             \
    case 2: { constexpr int NP = 2; __VA_ARGS__; } break;                             \
    case 3: { constexpr int NP = 3; __VA_ARGS__; } break;                             \
    default: { constexpr int NP = 4; __VA_ARGS__; } break;                            \
  }

extern "C" int ptc_concerto_align(const void* x, int xdtype, int64_t nx, const int64_t* ids, const void* y, int ydtype, int64_t u, int d,
                                  int shift, double eps, float* row, float* loss, void* dy, ptc_stream_t stream) {
  PTC_REQUIRE(ptc_concerto_align_supported(d), PTC_EUNSUPPORTED, "ptc_concerto_align: D=%d is not in [1, %d]", d, CC_MAX_D);
  PTC_REQUIRE(u >= 1 && nx >= 0 && eps > 0.0, PTC_EINVAL, "ptc_concerto_align: u=%lld rows=%lld eps=%g", (long long)u, (long long)nx, eps);
  PTC_REQUIRE(u < ((int64_t)1 << 31), PTC_EINVAL, "ptc_concerto_align: too many patches");
  PTC_REQUIRE((x || nx == 0) && ids && y && row && loss, PTC_EINVAL, "ptc_concerto_align: null buffer");
  hipStream_t st = (hipStream_t)stream;
  const bool vec_x = d % CC_GROUP == 0 && (uintptr_t)x % 16 == 0;
  const bool vec_y = d % CC_GROUP == 0 && ((uintptr_t)y | (uintptr_t)dy) % 16 == 0;
  const unsigned g = (unsigned)ptc_cdiv(u, CC_THREADS / PTC_WAVE);
  const float scale = (float)(10.0 / (double)u);
  PTC_DISPATCH_DTYPE(xdtype, TX, PTC_DISPATCH_DTYPE(ydtype, TY, CC_DISPATCH_NP(d, NP,
      hipLaunchKernelGGL((cc_align_kernel<TX, TY, NP>), dim3(g), dim3(CC_THREADS), 0, st, (const TX*)x, nx, ids, (const TY*)y, u, d, shift,
                         (float)eps, scale, vec_x, vec_y, row, (TY*)dy))));
  PTC_CHECK_LAUNCH("cc_align_kernel");
  hipLaunchKernelGGL(cc_sum_rows_kernel, dim3(1), dim3(CC_THREADS), 0, st, (const float*)row, u, 10.0 / (double)u, loss);
  PTC_CHECK_LAUNCH("cc_sum_rows_kernel");
  return PTC_OK;
}
