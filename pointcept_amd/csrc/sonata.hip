// sonata.hip -- Sonata-v1m1's teacher-centred distillation loss (pointcept/models/sonata/sonata_v1m1_base.py:267-291, :443-454):
// Sinkhorn-Knopp over the gathered teacher logits and the soft cross entropy against the student, without the M x K matrix.
//
// With e_ik = exp(t_ik / temp) the matrix after any Sinkhorn step is e_ik a_k b_i, so an iteration is two vectors:
//     r_k = sum_i e_ik b_i,  a_k = 1 / (K r_k)          (the prototype normalisation; the first one has b = 1 -- the reference's global
//     c_i = sum_k e_ik a_k,  b_i = 1 / (n c_i)            normalisation scales every r_k alike and cancels in a_k)
// and the final assignment is target_ik = e_ik a_k / c_i (sums to 1 over k).  exp(1.01 / 0.04) = 9.2e10 and its sums over 10^6 rows
// stay far inside fp32, so no constant is taken off the exponent.  Every pass streams the teacher rows THROUGH match_index[:, 1]
// (16-byte loads for fp32, 8-byte for bf16 / fp16, converted in the load; all arithmetic fp32) and recomputes e.
//
// Layout of every pass: 256 threads, thread t owns the four columns 1024 j + 4 t .. + 3 of each 1024-column chunk j (NCH = 1, 4 or 8
// chunks, K <= 1024 NCH, K a multiple of 64), a tile is R = 16 / NCH rows, so a thread holds 4 NCH x R = 64 values of a tile in
// registers -- a row stays there between its row sum and the column sums it feeds.  A workgroup walks the tiles
// blockIdx.x, + gridDim.x, ...; column sums are kept per thread (fp32 within a tile, double across tiles), written as ONE partial row
// per workgroup and summed over the workgroups in index order by a second kernel: no atomics, bit-reproducible.  Row sums go
// through a shuffle butterfly and one LDS exchange between the four waves.
//
// A pair whose teacher or student row lies outside the tensor contributes nothing (c = b = 0, no gradient): the kernels never
// read or write out of bounds whatever match_index holds.
#include "ptc_common.h"

#include <math.h>

#define SN_THREADS 256
#define SN_CHUNK (SN_THREADS * 4)
#define SN_MAX_K 8192
#define SN_TILE_VALUES 16        // NCH * R
#define SN_DEFAULT_GROUPS 256    // one workgroup per CU: the partials of a pass are SN_DEFAULT_GROUPS x K floats
#define SN_BWD_GROUPS 2048
#define SN_MAX_SCENES 65535

template <typename T> struct alignas(sizeof(T) * 4) SnPack { T v[4]; };

template <typename T> __device__ __forceinline__ void sn_load4(const T* __restrict__ p, float (&v)[4]) {
  const SnPack<T> q = *reinterpret_cast<const SnPack<T>*>(p);
#pragma unroll
  for (int j = 0; j < 4; ++j) v[j] = ptc_to_float(q.v[j]);
}
template <typename T> __device__ __forceinline__ void sn_store4(T* __restrict__ p, const float (&v)[4]) {
  SnPack<T> q;
#pragma unroll
  for (int j = 0; j < 4; ++j) q.v[j] = ptc_from_float<T>(v[j]);
  *reinterpret_cast<SnPack<T>*>(p) = q;
}

// x / temp with one rounding: 1 / temp is carried as an fp32 pair (hi, lo) made on the host in double
__device__ __forceinline__ float sn_scaled(float x, float hi, float lo) { return fmaf(x, lo, x * hi); }

// v[j] <- the sum (or max) of v[j] over the 256 threads, the same bits in every thread: xor butterfly inside a wave, then the four
// waves' values in index order.  red: 4 * NV floats of LDS.
template <int NV, bool MAX> __device__ __forceinline__ void sn_block_reduce(float (&v)[NV], float* red) {
#pragma unroll
  for (int j = 0; j < NV; ++j) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
      const float o = __shfl_xor(v[j], off);
      v[j] = MAX ? fmaxf(v[j], o) : v[j] + o;
    }
  }
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int j = 0; j < NV; ++j) red[wave * NV + j] = v[j];
  }
  __syncthreads();
#pragma unroll
  for (int j = 0; j < NV; ++j) {
    const float w0 = red[j], w1 = red[NV + j], w2 = red[2 * NV + j], w3 = red[3 * NV + j];
    v[j] = MAX ? fmaxf(fmaxf(w0, w1), fmaxf(w2, w3)) : (w0 + w1) + (w2 + w3);
  }
  __syncthreads();
}

// the thread's columns of a K-vector (0 past K)
template <int NCH> __device__ __forceinline__ void sn_load_vec(const float* __restrict__ a, int K, float (&av)[NCH * 4]) {
#pragma unroll
  for (int ch = 0; ch < NCH; ++ch) {
    const int col = ch * SN_CHUNK + threadIdx.x * 4;
    float t[4] = {0.f, 0.f, 0.f, 0.f};
    if (col < K) sn_load4<float>(a + col, t);
#pragma unroll
    for (int j = 0; j < 4; ++j) av[ch * 4 + j] = t[j];
  }
}

// ROW = false (column sums):  part[g][k] = sum over the workgroup's rows of e_ik b_i      (vec = b [m], or NULL: b = 1)
// ROW = true  (row pass):     c_i = sum_k e_ik a_k, b_i = 1 / (n c_i)                      (vec = a [K]); with part != NULL the column
//                             sums of e_ik b_i as well, from the registers that made c_i
template <typename T, int NCH, bool ROW>
__global__ void __launch_bounds__(SN_THREADS)
sn_pass_kernel(const T* __restrict__ teacher, int64_t nt, const int64_t* __restrict__ mi, int64_t m, int K, float ih, float il,
               const float* __restrict__ vec, float n, float* __restrict__ c_out, float* __restrict__ b_out, float* __restrict__ part) {
  constexpr int R = SN_TILE_VALUES / NCH, NV = NCH * 4;
  __shared__ float red[4 * R];
  const int tid = threadIdx.x;
  float av[NV];
  if (ROW) sn_load_vec<NCH>(vec, K, av);
  double acc[NV];
#pragma unroll
  for (int j = 0; j < NV; ++j) acc[j] = 0.0;
  const int64_t ntile = (m + R - 1) / R;
  for (int64_t tile = blockIdx.x; tile < ntile; tile += gridDim.x) {
    float e[R][NV], rs[R], bi[R];
    bool live[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const int64_t i = tile * R + r;
      const int64_t idx = i < m ? mi[2 * i + 1] : -1;
      live[r] = (uint64_t)idx < (uint64_t)nt;
      const T* row = teacher + (live[r] ? idx : 0) * K;
      rs[r] = 0.f;
#pragma unroll
      for (int ch = 0; ch < NCH; ++ch) {
        const int col = ch * SN_CHUNK + tid * 4;
        float t[4] = {0.f, 0.f, 0.f, 0.f};
        const bool on = live[r] && col < K;
        if (on) sn_load4<T>(row + col, t);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          e[r][ch * 4 + j] = on ? expf(sn_scaled(t[j], ih, il)) : 0.f;
          if (ROW) rs[r] = fmaf(e[r][ch * 4 + j], av[ch * 4 + j], rs[r]);
        }
      }
    }
    if (ROW) {
      sn_block_reduce<R, false>(rs, red);
#pragma unroll
      for (int r = 0; r < R; ++r) {
        bi[r] = live[r] ? 1.f / (n * rs[r]) : 0.f;
        const int64_t i = tile * R + r;
        if (tid == 0 && i < m) {
          c_out[i] = live[r] ? rs[r] : 0.f;
          b_out[i] = bi[r];
        }
      }
    } else {
#pragma unroll
      for (int r = 0; r < R; ++r) {
        const int64_t i = tile * R + r;
        bi[r] = live[r] ? (vec ? vec[i] : 1.f) : 0.f;
      }
    }
    if (part) {
#pragma unroll
      for (int j = 0; j < NV; ++j) {
        float s = 0.f;
#pragma unroll
        for (int r = 0; r < R; ++r) s = fmaf(e[r][j], bi[r], s);
        acc[j] += (double)s;
      }
    }
  }
  if (part) {
#pragma unroll
    for (int ch = 0; ch < NCH; ++ch) {
      const int col = ch * SN_CHUNK + tid * 4;
      if (col < K) {
        const float o[4] = {(float)acc[ch * 4], (float)acc[ch * 4 + 1], (float)acc[ch * 4 + 2], (float)acc[ch * 4 + 3]};
        sn_store4<float>(part + (int64_t)blockIdx.x * K + col, o);
      }
    }
  }
}

// r[k] = the partial rows summed in index order (double)
__global__ void __launch_bounds__(SN_THREADS)
sn_colsum_finish_kernel(const float* __restrict__ part, int G, int K, float* __restrict__ r) {
  const int k = blockIdx.x * SN_THREADS + threadIdx.x;
  if (k >= K) return;
  double s = 0.0;
  for (int g = 0; g < G; ++g) s += (double)part[(int64_t)g * K + k];
  r[k] = (float)s;
}

// The last row pass and the loss: c_i, lse_i = logsumexp_k(s_ik / student_temp), row_loss_i = lse_i - sum_k target_ik s_ik / student_temp
template <typename T, typename S, int NCH>
__global__ void __launch_bounds__(SN_THREADS)
sn_distill_fwd_kernel(const T* __restrict__ teacher, int64_t nt, const S* __restrict__ student, int64_t ns, const int64_t* __restrict__ mi,
                      int64_t m, int K, float ih, float il, float sh, float sl, const float* __restrict__ a, float* __restrict__ c_out,
                      float* __restrict__ lse_out, float* __restrict__ loss_out) {
  constexpr int R = SN_TILE_VALUES / NCH, NV = NCH * 4;
  __shared__ float red[4 * 3 * R];
  const int tid = threadIdx.x;
  float av[NV];
  sn_load_vec<NCH>(a, K, av);
  const int64_t ntile = (m + R - 1) / R;
  for (int64_t tile = blockIdx.x; tile < ntile; tile += gridDim.x) {
    float sx[R][NV], mx[R], sum[3 * R];
    bool live[R];
    int64_t trow[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const int64_t i = tile * R + r;
      const int64_t si = i < m ? mi[2 * i] : -1;
      trow[r] = i < m ? mi[2 * i + 1] : -1;
      live[r] = (uint64_t)si < (uint64_t)ns && (uint64_t)trow[r] < (uint64_t)nt;
      const S* row = student + (live[r] ? si : 0) * K;
      mx[r] = live[r] ? -INFINITY : 0.f;
#pragma unroll
      for (int ch = 0; ch < NCH; ++ch) {
        const int col = ch * SN_CHUNK + tid * 4;
        float t[4] = {0.f, 0.f, 0.f, 0.f};
        const bool on = live[r] && col < K;
        if (on) sn_load4<S>(row + col, t);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          sx[r][ch * 4 + j] = sn_scaled(t[j], sh, sl);
          if (on) mx[r] = fmaxf(mx[r], sx[r][ch * 4 + j]);
        }
      }
    }
    sn_block_reduce<R, true>(mx, red);
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const T* row = teacher + (live[r] ? trow[r] : 0) * K;
      float se = 0.f, pc = 0.f, pd = 0.f;
#pragma unroll
      for (int ch = 0; ch < NCH; ++ch) {
        const int col = ch * SN_CHUNK + tid * 4;
        float t[4] = {0.f, 0.f, 0.f, 0.f};
        const bool on = live[r] && col < K;
        if (on) sn_load4<T>(row + col, t);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const float x = sx[r][ch * 4 + j];
          const float w = on ? expf(sn_scaled(t[j], ih, il)) * av[ch * 4 + j] : 0.f;
          se += on ? expf(x - mx[r]) : 0.f;
          pc += w;
          pd = fmaf(w, x, pd);
        }
      }
      sum[3 * r] = se;
      sum[3 * r + 1] = pc;
      sum[3 * r + 2] = pd;
    }
    sn_block_reduce<3 * R, false>(sum, red);
    if (tid == 0) {
#pragma unroll
      for (int r = 0; r < R; ++r) {
        const int64_t i = tile * R + r;
        if (i < m) {
          const float lse = mx[r] + logf(sum[3 * r]);
          c_out[i] = live[r] ? sum[3 * r + 1] : 0.f;
          lse_out[i] = live[r] ? lse : 0.f;
          loss_out[i] = live[r] ? lse - sum[3 * r + 2] / sum[3 * r + 1] : 0.f;
        }
      }
    }
  }
}

// the scene of pair i (pairs are listed by ascending scene, as torch_scatter.segment_coo requires of its index)
__device__ __forceinline__ int64_t sn_scene_of(const int64_t* __restrict__ mi, const int64_t* __restrict__ batch, int64_t ns, int64_t i) {
  const int64_t si = mi[2 * i];
  return (uint64_t)si < (uint64_t)ns ? batch[si] : INT64_MAX;
}
__device__ __forceinline__ int64_t sn_lower_bound(const int64_t* __restrict__ mi, const int64_t* __restrict__ batch, int64_t ns, int64_t m,
                                                  int64_t key) {
  int64_t lo = 0, hi = m;
  while (lo < hi) {
    const int64_t mid = lo + (hi - lo) / 2;
    if (sn_scene_of(mi, batch, ns, mid) < key) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// workgroup s: the mean of row_loss over the pairs of scene s (0 without pairs) and their weight 1 / (pairs of the scene x scenes),
// scenes = the scene of the last pair + 1 (segment_coo without dim_size)
__global__ void __launch_bounds__(SN_THREADS)
sn_scene_kernel(const float* __restrict__ row_loss, const int64_t* __restrict__ mi, const int64_t* __restrict__ batch, int64_t ns, int64_t m,
                float* __restrict__ roww, float* __restrict__ scene_mean) {
  __shared__ double red[SN_THREADS];
  const int tid = threadIdx.x;
  const int64_t s = blockIdx.x;
  const int64_t lo = sn_lower_bound(mi, batch, ns, m, s), hi = sn_lower_bound(mi, batch, ns, m, s + 1);
  const int64_t scenes = sn_scene_of(mi, batch, ns, m - 1) + 1;
  const float w = hi > lo ? (float)(1.0 / ((double)(hi - lo) * (double)scenes)) : 0.f;
  double p = 0.0;
  for (int64_t i = lo + tid; i < hi; i += SN_THREADS) {
    p += (double)row_loss[i];
    roww[i] = w;
  }
  red[tid] = p;
  __syncthreads();
  for (int off = SN_THREADS / 2; off >= 1; off >>= 1) {
    if (tid < off) red[tid] += red[tid + off];
    __syncthreads();
  }
  if (tid == 0) scene_mean[s] = hi > lo ? (float)(red[0] / (double)(hi - lo)) : 0.f;
}

// loss = the mean of scene_mean over the scenes up to the last matched one
__global__ void __launch_bounds__(64)
sn_loss_kernel(const float* __restrict__ scene_mean, int num_scenes, const int64_t* __restrict__ mi, const int64_t* __restrict__ batch,
               int64_t ns, int64_t m, float* __restrict__ loss) {
  if (threadIdx.x != 0) return;
  const int64_t scenes = sn_scene_of(mi, batch, ns, m - 1) + 1;
  double s = 0.0;
  for (int64_t i = 0; i < scenes && i < num_scenes; ++i) s += (double)scene_mean[i];
  loss[0] = (float)(s / (double)scenes);
}

// dpred[student row of pair i] = dloss w_i / student_temp (softmax(s_i / student_temp) - target_i); nothing else is written
template <typename T, typename S, int NCH>
__global__ void __launch_bounds__(SN_THREADS)
sn_distill_bwd_kernel(const T* __restrict__ teacher, int64_t nt, const S* __restrict__ student, int64_t ns, const int64_t* __restrict__ mi,
                      int64_t m, int K, float ih, float il, float sh, float sl, const float* __restrict__ a, const float* __restrict__ c,
                      const float* __restrict__ lse, const float* __restrict__ roww, const float* __restrict__ dloss, S* __restrict__ dpred) {
  constexpr int NV = NCH * 4;
  const int tid = threadIdx.x;
  float av[NV];
  sn_load_vec<NCH>(a, K, av);
  const float g0 = dloss[0] * sn_scaled(1.f, sh, sl);
  for (int64_t i = blockIdx.x; i < m; i += gridDim.x) {
    const int64_t si = mi[2 * i], ti = mi[2 * i + 1];
    if (!((uint64_t)si < (uint64_t)ns && (uint64_t)ti < (uint64_t)nt)) continue;
    const float g = g0 * roww[i], l = lse[i], ic = 1.f / c[i];
#pragma unroll
    for (int ch = 0; ch < NCH; ++ch) {
      const int col = ch * SN_CHUNK + tid * 4;
      if (col < K) {
        float t[4], x[4], o[4];
        sn_load4<T>(teacher + ti * K + col, t);
        sn_load4<S>(student + si * K + col, x);
#pragma unroll
        for (int j = 0; j < 4; ++j)
          o[j] = g * (expf(sn_scaled(x[j], sh, sl) - l) - expf(sn_scaled(t[j], ih, il)) * av[ch * 4 + j] * ic);
        sn_store4<S>(dpred + si * K + col, o);
      }
    }
  }
}

// ------------------------------------------------------------------------------------------------ entry points
extern "C" int ptc_sonata_supported(int k) { return k >= 64 && k <= SN_MAX_K && (k & 63) == 0; }

static inline int sn_nch(int k) { return k <= SN_CHUNK ? 1 : k <= 4 * SN_CHUNK ? 4 : 8; }

static inline int64_t sn_groups(int64_t m, int k, int max_groups, int dflt) {
  const int64_t ntile = ptc_cdiv(m > 0 ? m : 1, SN_TILE_VALUES / sn_nch(k));
  const int64_t cap = max_groups > 0 ? max_groups : dflt;
  return ntile < cap ? ntile : cap;
}

extern "C" int64_t ptc_sonata_groups(int64_t m, int k, int max_groups) {
  if (m < 0 || !ptc_sonata_supported(k)) return 0;
  return sn_groups(m, k, max_groups, SN_DEFAULT_GROUPS);
}

static int sn_check(const char* what, int64_t nt, int64_t m, int k, double temp) {
  PTC_REQUIRE(ptc_sonata_supported(k), PTC_EUNSUPPORTED, "%s: K=%d is not a multiple of 64 in [64, %d]", what, k, SN_MAX_K);
  PTC_REQUIRE(m >= 0 && nt >= 0, PTC_EINVAL, "%s: m=%lld rows=%lld", what, (long long)m, (long long)nt);
  PTC_REQUIRE(temp > 0.0, PTC_EINVAL, "%s: temperature %g", what, temp);
  return PTC_OK;
}

struct SnInv { float hi, lo; };
static inline SnInv sn_inv(double temp) {
  SnInv r;
  r.hi = (float)(1.0 / temp);
  r.lo = (float)(1.0 / temp - (double)r.hi);
  return r;
}

#define SN_DISPATCH_NCH(k, NCH, ...)                        \
  switch (sn_nch(k)) {                                      \
    case 1: { constexpr int NCH = 1; __VA_ARGS__; } break;  \
    case 4: { constexpr int NCH = 4; __VA_ARGS__; } break;  \
    default: { constexpr int NCH = 8; __VA_ARGS__; } break; \
  }

template <bool ROW>
static int sn_pass(const char* what, const void* teacher, int tdtype, int64_t nt, const int64_t* mi, int64_t m, int k, double temp,
                   const float* vec, double n, float* c, float* b, int max_groups, float* part, float* r, hipStream_t st) {
  const SnInv it = sn_inv(temp);
  const int G = (int)sn_groups(m, k, max_groups, SN_DEFAULT_GROUPS);
  PTC_DISPATCH_DTYPE(tdtype, T, SN_DISPATCH_NCH(k, NCH,
      hipLaunchKernelGGL((sn_pass_kernel<T, NCH, ROW>), dim3((unsigned)G), dim3(SN_THREADS), 0, st, (const T*)teacher, nt, mi, m, k, it.hi, it.lo,
                         vec, (float)n, c, b, part)));
  PTC_CHECK_LAUNCH(what);
  if (part) {
    hipLaunchKernelGGL(sn_colsum_finish_kernel, dim3((unsigned)ptc_cdiv(k, SN_THREADS)), dim3(SN_THREADS), 0, st, part, G, k, r);
    PTC_CHECK_LAUNCH("sn_colsum_finish_kernel");
  }
  return PTC_OK;
}

extern "C" int ptc_sonata_colsum(const void* teacher, int tdtype, int64_t nt, const int64_t* match_index, int64_t m, int k, double temp,
                                 const float* b, int max_groups, float* partials, float* r, ptc_stream_t stream) {
  if (int rc = sn_check("ptc_sonata_colsum", nt, m, k, temp)) return rc;
  if (m == 0) return PTC_OK;
  PTC_REQUIRE(teacher && match_index && partials && r, PTC_EINVAL, "ptc_sonata_colsum: null buffer");
  return sn_pass<false>("sn_pass_kernel(colsum)", teacher, tdtype, nt, match_index, m, k, temp, b, 1.0, nullptr, nullptr, max_groups, partials, r,
                        (hipStream_t)stream);
}

extern "C" int ptc_sonata_rowpass(const void* teacher, int tdtype, int64_t nt, const int64_t* match_index, int64_t m, int k, double temp,
                                  const float* a, double n, float* c, float* b, int max_groups, float* partials, float* r,
                                  ptc_stream_t stream) {
  if (int rc = sn_check("ptc_sonata_rowpass", nt, m, k, temp)) return rc;
  PTC_REQUIRE(n > 0.0, PTC_EINVAL, "ptc_sonata_rowpass: n=%g rows", n);
  if (m == 0) return PTC_OK;
  PTC_REQUIRE(teacher && match_index && a && c && b && (!partials || r), PTC_EINVAL, "ptc_sonata_rowpass: null buffer");
  return sn_pass<true>("sn_pass_kernel(rowpass)", teacher, tdtype, nt, match_index, m, k, temp, a, n, c, b, max_groups, partials, r,
                       (hipStream_t)stream);
}

#define SN_DISPATCH_TS(tdtype, sdtype, T, S, ...) PTC_DISPATCH_DTYPE(tdtype, T, PTC_DISPATCH_DTYPE(sdtype, S, __VA_ARGS__))

extern "C" int ptc_sonata_distill_fwd(const void* teacher, int tdtype, int64_t nt, const void* student, int sdtype, int64_t ns,
                                      const int64_t* match_index, const int64_t* student_batch, int num_scenes, int64_t m, int k, double temp,
                                      double student_temp, const float* a, int max_groups, float* c, float* lse, float* row_loss, float* roww,
                                      float* scene_mean, float* loss, ptc_stream_t stream) {
  if (int rc = sn_check("ptc_sonata_distill_fwd", nt, m, k, temp)) return rc;
  PTC_REQUIRE(student_temp > 0.0 && ns >= 0, PTC_EINVAL, "ptc_sonata_distill_fwd: student_temp=%g rows=%lld", student_temp, (long long)ns);
  PTC_REQUIRE(num_scenes >= 1 && num_scenes <= SN_MAX_SCENES, PTC_EINVAL, "ptc_sonata_distill_fwd: %d scenes", num_scenes);
  if (m == 0) return PTC_OK;
  PTC_REQUIRE(teacher && student && match_index && student_batch && a && c && lse && row_loss && roww && scene_mean && loss, PTC_EINVAL,
              "ptc_sonata_distill_fwd: null buffer");
  hipStream_t st = (hipStream_t)stream;
  const SnInv it = sn_inv(temp), is = sn_inv(student_temp);
  const int G = (int)sn_groups(m, k, max_groups, SN_DEFAULT_GROUPS);
  SN_DISPATCH_TS(tdtype, sdtype, T, S, SN_DISPATCH_NCH(k, NCH,
      hipLaunchKernelGGL((sn_distill_fwd_kernel<T, S, NCH>), dim3((unsigned)G), dim3(SN_THREADS), 0, st, (const T*)teacher, nt, (const S*)student,
                         ns, match_index, m, k, it.hi, it.lo, is.hi, is.lo, a, c, lse, row_loss)));
  PTC_CHECK_LAUNCH("sn_distill_fwd_kernel");
  hipLaunchKernelGGL(sn_scene_kernel, dim3((unsigned)num_scenes), dim3(SN_THREADS), 0, st, row_loss, match_index, student_batch, ns, m, roww,
                     scene_mean);
  PTC_CHECK_LAUNCH("sn_scene_kernel");
  hipLaunchKernelGGL(sn_loss_kernel, dim3(1), dim3(64), 0, st, scene_mean, num_scenes, match_index, student_batch, ns, m, loss);
  PTC_CHECK_LAUNCH("sn_loss_kernel");
  return PTC_OK;
}

extern "C" int ptc_sonata_distill_bwd(const void* teacher, int tdtype, int64_t nt, const void* student, int sdtype, int64_t ns,
                                      const int64_t* match_index, int64_t m, int k, double temp, double student_temp, const float* a,
                                      const float* c, const float* lse, const float* roww, const float* dloss, int max_groups, void* dpred,
                                      ptc_stream_t stream) {
  if (int rc = sn_check("ptc_sonata_distill_bwd", nt, m, k, temp)) return rc;
  PTC_REQUIRE(student_temp > 0.0 && ns >= 0, PTC_EINVAL, "ptc_sonata_distill_bwd: student_temp=%g rows=%lld", student_temp, (long long)ns);
  if (m == 0) return PTC_OK;
  PTC_REQUIRE(teacher && student && match_index && a && c && lse && roww && dloss && dpred, PTC_EINVAL, "ptc_sonata_distill_bwd: null buffer");
  hipStream_t st = (hipStream_t)stream;
  const SnInv it = sn_inv(temp), is = sn_inv(student_temp);
  const int64_t cap = max_groups > 0 ? max_groups : SN_BWD_GROUPS;
  const unsigned G = (unsigned)(m < cap ? m : cap);
  SN_DISPATCH_TS(tdtype, sdtype, T, S, SN_DISPATCH_NCH(k, NCH,
      hipLaunchKernelGGL((sn_distill_bwd_kernel<T, S, NCH>), dim3(G), dim3(SN_THREADS), 0, st, (const T*)teacher, nt, (const S*)student, ns,
                         match_index, m, k, it.hi, it.lo, is.hi, is.lo, a, c, lse, roww, dloss, (S*)dpred)));
  PTC_CHECK_LAUNCH("sn_distill_bwd_kernel");
  return PTC_OK;
}
