// cluster_agg.hip -- OA-CNNs' adaptive aggregation (pointcept/models/oacnns/oacnns_v1m1_base.py:87-111, 160-164).
//
// 1a  grid-cluster maps of a DonwBlock: the clusters of torch_cluster.grid_cluster on [coord | batch] (anchored at the GLOBAL per-axis
//     minimum, cell = trunc((c - min) / size) in fp32, x fastest, batch slowest) numbered as torch.unique numbers them.  One key pass
//     for all levels, then ptc_sort_keys (one row per level) and ptc_pool_maps_count(shift 0) per level; ptc_pool_maps_fill builds the
//     CSR after the caller's single read of the cluster counts.  A key packs (batch, cz, cy, cx) in bit fields sized from the
//     spatial shape, so ascending keys are ascending linearised cell ids (only their order reaches torch.unique).
// 1b  segmented centering y = x - mean_c(x)[c] for all levels in one launch (its backward is the same operator on dy).
// 1c  out[n] = sum_i softmax(a[n])_i S_i[c_i(n)],  S_i[c] = sum_{m in c} v_i[m] e_i[m] / (sum_{m in c} e_i[m] + 1e-6),
//     e_i = exp(u_i - max(u_i)) with ONE max over the whole [N, C] tensor of level i, as the reference takes it.
//
// Determinism: no float atomics anywhere.  Every cluster is reduced by ONE workgroup in a fixed order (row slots, then a sequential sum
// over the slots in LDS); the global max is an integer atomicMax of an order-preserving encoding (the maximum does not depend on the
// order of the updates); the gradient of the max is reduced per level by one workgroup in a fixed order and spread evenly over the
// elements equal to the max, as torch's backward of a full max() does.
//
// Thread layout of the cluster and row kernels (256 threads): G = next power of two >= C / 4 threads per row, each holding 4
// consecutive channels (fp32 arithmetic, 16- or 8-byte loads), R = 256 / G row slots.  C % 4 == 0 and C <= 256 (G <= 64: a row lies
// inside one wave, so the row kernels reduce over channels with shuffles).
#include "ptc_common.h"

#define CA_THREADS 256
#define CA_MAX_LEVELS 8
#define CA_EPS 1e-6f

namespace {

struct CaLevels {
  const void* u[CA_MAX_LEVELS];
  const void* v[CA_MAX_LEVELS];
  void* du[CA_MAX_LEVELS];
  void* dv[CA_MAX_LEVELS];
  const int64_t* perm[CA_MAX_LEVELS];
  const int64_t* indptr[CA_MAX_LEVELS];
  const int64_t* cluster[CA_MAX_LEVELS];
  int64_t off[CA_MAX_LEVELS + 1];   // first global cluster index of level l; off[L] = total
  int L;
};

// element l of a kernel-argument array with a wave-uniform l, without a runtime-indexed (scratch) copy of the array
template <typename P>
__device__ __forceinline__ P ca_pick(const P (&arr)[CA_MAX_LEVELS], int l) {
  P r = arr[0];
  ptc_static_for<CA_MAX_LEVELS>([&](auto I) {
    if (I.value == l) r = arr[I.value];
  });
  return r;
}

__device__ __forceinline__ int ca_level_of(const CaLevels& P, int64_t g) {
  int l = 0;
  ptc_static_for<CA_MAX_LEVELS - 1>([&](auto I) {
    if (I.value + 1 < P.L && g >= P.off[I.value + 1]) l = I.value + 1;
  });
  return l;
}

__device__ __forceinline__ void ca_ld4(const float* p, float (&f)[4]) {
  const float4 q = *reinterpret_cast<const float4*>(p);
  f[0] = q.x; f[1] = q.y; f[2] = q.z; f[3] = q.w;
}
__device__ __forceinline__ void ca_ld4(const bf16_t* p, float (&f)[4]) {
  const uint2 q = *reinterpret_cast<const uint2*>(p);
  f[0] = __uint_as_float(q.x << 16); f[1] = __uint_as_float(q.x & 0xffff0000u);
  f[2] = __uint_as_float(q.y << 16); f[3] = __uint_as_float(q.y & 0xffff0000u);
}
__device__ __forceinline__ void ca_ld4(const f16_t* p, float (&f)[4]) {
  const uint2 q = *reinterpret_cast<const uint2*>(p);
  f16_t e[4];
  __builtin_memcpy(e, &q, 8);
  f[0] = (float)e[0].x; f[1] = (float)e[1].x; f[2] = (float)e[2].x; f[3] = (float)e[3].x;
}
__device__ __forceinline__ void ca_st4(float* p, const float (&f)[4]) {
  *reinterpret_cast<float4*>(p) = make_float4(f[0], f[1], f[2], f[3]);
}
__device__ __forceinline__ void ca_st4(bf16_t* p, const float (&f)[4]) {
  *reinterpret_cast<uint2*>(p) = make_uint2(ptc_pack_bf16x2(f[0], f[1]), ptc_pack_bf16x2(f[2], f[3]));
}
__device__ __forceinline__ void ca_st4(f16_t* p, const float (&f)[4]) {
  f16_t e[4];
  for (int k = 0; k < 4; ++k) e[k] = ptc_from_float<f16_t>(f[k]);
  uint2 q;
  __builtin_memcpy(&q, e, 8);
  *reinterpret_cast<uint2*>(p) = q;
}

// softmax of the L logits of row n (fp32)
template <typename T>
__device__ __forceinline__ void ca_softmax(const T* __restrict__ a, int64_t n, int L, float (&p)[CA_MAX_LEVELS]) {
  float mx = -INFINITY;
  ptc_static_for<CA_MAX_LEVELS>([&](auto I) {
    if (I.value < L) {
      p[I.value] = ptc_to_float(a[n * L + I.value]);
      mx = fmaxf(mx, p[I.value]);
    }
  });
  float s = 0.f;
  ptc_static_for<CA_MAX_LEVELS>([&](auto I) {
    if (I.value < L) {
      p[I.value] = expf(p[I.value] - mx);
      s += p[I.value];
    }
  });
  const float inv = 1.f / s;
  ptc_static_for<CA_MAX_LEVELS>([&](auto I) {
    if (I.value < L) p[I.value] *= inv;
  });
}

struct CaLayout {
  int G, R, cg;
};
__host__ __device__ __forceinline__ CaLayout ca_layout(int c) {
  CaLayout y;
  y.cg = c / 4;
  y.G = 1;
  while (y.G < y.cg) y.G <<= 1;
  y.R = CA_THREADS / y.G;
  return y;
}

// Sequential sum over the R row slots of `k` floats per thread (red[slot][G][k]); the result for channel group j lands in slot 0.
template <int K>
__device__ __forceinline__ void ca_slot_reduce(float* red, const CaLayout& Y, int s, int j, float (&acc)[K]) {
  for (int k = 0; k < K; ++k) red[(s * Y.G + j) * K + k] = acc[k];
  __syncthreads();
  if (s == 0) {
    for (int r = 1; r < Y.R; ++r)
      for (int k = 0; k < K; ++k) acc[k] += red[(r * Y.G + j) * K + k];
  }
  __syncthreads();
}

// ------------------------------------------------------------------------------------------------------------------------------------
// 1a. grid-cluster keys
// ------------------------------------------------------------------------------------------------------------------------------------
struct CaKeyLevels {
  float size[CA_MAX_LEVELS];
  int bx[CA_MAX_LEVELS], by[CA_MAX_LEVELS], bz[CA_MAX_LEVELS];
  int L;
};

__global__ void __launch_bounds__(256) ca_coord_min_kernel(const int32_t* __restrict__ ind, int64_t n, int32_t* __restrict__ mn) {
  int32_t m[4] = {INT_MAX, INT_MAX, INT_MAX, INT_MAX};
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < n; r += stride) {
    const int4 q = *reinterpret_cast<const int4*>(ind + r * 4);
    m[0] = min(m[0], q.x); m[1] = min(m[1], q.y); m[2] = min(m[2], q.z); m[3] = min(m[3], q.w);
  }
  for (int a = 0; a < 4; ++a)
    for (int o = 32; o >= 1; o >>= 1) m[a] = min(m[a], __shfl_xor(m[a], o));
  if (ptc_lane() == 0)
    for (int a = 0; a < 4; ++a) atomicMin(mn + a, m[a]);   // integer minimum: independent of the update order
}

__global__ void __launch_bounds__(256) ca_keys_kernel(const int32_t* __restrict__ ind, int64_t n, const int32_t* __restrict__ mn,
                                                      CaKeyLevels lv, int64_t* __restrict__ keys) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < n; r += stride) {
    const int4 q = *reinterpret_cast<const int4*>(ind + r * 4);
    // voxel_grid's p - start in the coordinates' fp32 (exact below 2^24), then trunc(p / size) per axis; the batch axis has size 1
    const uint64_t b = (uint64_t)(int64_t)((float)q.x - (float)mn[0]);
    const float px = (float)q.y - (float)mn[1], py = (float)q.z - (float)mn[2], pz = (float)q.w - (float)mn[3];
    ptc_static_for<CA_MAX_LEVELS>([&](auto I) {
      constexpr int l = I.value;
      if (l < lv.L) {
        const float sz = lv.size[l];
        const uint64_t cx = (uint64_t)(int64_t)(px / sz), cy = (uint64_t)(int64_t)(py / sz), cz = (uint64_t)(int64_t)(pz / sz);
        keys[(int64_t)l * n + r] = (int64_t)((((((b << lv.bz[l]) | cz) << lv.by[l]) | cy) << lv.bx[l]) | cx);
      }
    });
  }
}

static int ca_bits(int64_t v) {   // bits to hold 0..v
  int b = 0;
  while (b < 63 && (v >> b) > 0) ++b;
  return b;
}

struct CaMapLayout {
  size_t mn, keys, scratch, total;
};
static CaMapLayout ca_map_layout(int64_t n, int L) {
  CaMapLayout y;
  y.mn = 0;
  y.keys = 256;
  y.scratch = ptc_align_up(y.keys + (size_t)L * n * 8, 256);
  size_t s = ptc_sort_keys_workspace_bytes(n, L), p = ptc_pool_maps_workspace_bytes(n);
  y.total = y.scratch + (s > p ? s : p);
  return y;
}

// ------------------------------------------------------------------------------------------------------------------------------------
// 1b. segmented centering, all levels in one launch: one workgroup per cluster
// ------------------------------------------------------------------------------------------------------------------------------------
template <typename T>
__global__ void __launch_bounds__(CA_THREADS) ca_center_kernel(CaLevels P, int c) {
  __shared__ float red[CA_THREADS * 4];
  const CaLayout Y = ca_layout(c);
  const int64_t g = blockIdx.x;
  const int l = ca_level_of(P, g);
  const int64_t cl = g - P.off[l];
  const T* x = (const T*)ca_pick(P.u, l);
  T* y = (T*)ca_pick(P.du, l);
  const int64_t* perm = ca_pick(P.perm, l);
  const int64_t* ip = ca_pick(P.indptr, l);
  const int64_t beg = ip[cl], end = ip[cl + 1];
  const int j = threadIdx.x % Y.G, s = threadIdx.x / Y.G;
  const bool act = j < Y.cg;
  float acc[4] = {0.f, 0.f, 0.f, 0.f};
  if (act)
    for (int64_t r = beg + s; r < end; r += Y.R) {
      float f[4];
      ca_ld4(x + perm[r] * c + 4 * j, f);
      for (int k = 0; k < 4; ++k) acc[k] += f[k];
    }
  ca_slot_reduce<4>(red, Y, s, j, acc);
  if (s == 0)
    for (int k = 0; k < 4; ++k) red[j * 4 + k] = acc[k] / (float)(end - beg);
  __syncthreads();
  if (!act) return;
  float mean[4];
  for (int k = 0; k < 4; ++k) mean[k] = red[j * 4 + k];
  for (int64_t r = beg + s; r < end; r += Y.R) {
    const int64_t m = perm[r];
    float f[4];
    ca_ld4(x + m * c + 4 * j, f);
    for (int k = 0; k < 4; ++k) f[k] -= mean[k];
    ca_st4(y + m * c + 4 * j, f);
  }
}

// ------------------------------------------------------------------------------------------------------------------------------------
// 1c. adaptive aggregation.  State (fp32, kept by the caller between forward and backward): S [total, c], D [total, c] (= the
// denominator + 1e-6), then L encoded maxima.
// ------------------------------------------------------------------------------------------------------------------------------------
template <typename T>
__global__ void __launch_bounds__(256) ca_max_kernel(CaLevels P, int64_t nc, uint32_t* __restrict__ mx) {
  const int l = blockIdx.y;
  const T* u = (const T*)ca_pick(P.u, l);
  uint32_t m = 0;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nc / 4; i += stride) {
    float f[4];
    ca_ld4(u + 4 * i, f);
    for (int k = 0; k < 4; ++k) m = max(m, ptc_float_enc(f[k]));
  }
  for (int o = 32; o >= 1; o >>= 1) m = max(m, (uint32_t)__shfl_xor((int)m, o));
  if (ptc_lane() == 0) atomicMax(mx + l, m);    // integer maximum: independent of the update order
}

template <typename T>
__global__ void __launch_bounds__(CA_THREADS) ca_agg_cluster_fwd_kernel(CaLevels P, int c, float* __restrict__ S, float* __restrict__ D,
                                                                        const uint32_t* __restrict__ mx) {
  __shared__ float red[CA_THREADS * 8];
  const CaLayout Y = ca_layout(c);
  const int64_t g = blockIdx.x;
  const int l = ca_level_of(P, g);
  const int64_t cl = g - P.off[l];
  const T* u = (const T*)ca_pick(P.u, l);
  const T* v = (const T*)ca_pick(P.v, l);
  const int64_t* perm = ca_pick(P.perm, l);
  const int64_t* ip = ca_pick(P.indptr, l);
  const int64_t beg = ip[cl], end = ip[cl + 1];
  const float M = ptc_float_dec(mx[l]);
  const int j = threadIdx.x % Y.G, s = threadIdx.x / Y.G;
  const bool act = j < Y.cg;
  float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};   // den[4], num[4]
  if (act)
    for (int64_t r = beg + s; r < end; r += Y.R) {
      const int64_t m = perm[r];
      float fu[4], fv[4];
      ca_ld4(u + m * c + 4 * j, fu);
      ca_ld4(v + m * c + 4 * j, fv);
      for (int k = 0; k < 4; ++k) {
        const float e = expf(fu[k] - M);
        acc[k] += e;
        acc[4 + k] += fv[k] * e;
      }
    }
  ca_slot_reduce<8>(red, Y, s, j, acc);
  if (s == 0 && act) {
    float sv[4], dv[4];
    for (int k = 0; k < 4; ++k) {
      dv[k] = acc[k] + CA_EPS;
      sv[k] = acc[4 + k] / dv[k];
    }
    ca_st4(S + g * c + 4 * j, sv);
    ca_st4(D + g * c + 4 * j, dv);
  }
}

// out[n] = sum_i p_i(n) S_i[c_i(n)]   (one row per G threads)
template <typename T>
__global__ void __launch_bounds__(CA_THREADS) ca_agg_rows_fwd_kernel(CaLevels P, const T* __restrict__ a, int64_t n, int c,
                                                                     const float* __restrict__ S, T* __restrict__ out) {
  const CaLayout Y = ca_layout(c);
  const int j = threadIdx.x % Y.G, s = threadIdx.x / Y.G;
  if (j >= Y.cg) return;
  for (int64_t row = (int64_t)blockIdx.x * Y.R + s; row < n; row += (int64_t)gridDim.x * Y.R) {
    float p[CA_MAX_LEVELS];
    ca_softmax(a, row, P.L, p);
    float o[4] = {0.f, 0.f, 0.f, 0.f};
    ptc_static_for<CA_MAX_LEVELS>([&](auto I) {
      constexpr int l = I.value;
      if (l < P.L) {
        float f[4];
        ca_ld4(S + (P.off[l] + P.cluster[l][row]) * c + 4 * j, f);
        for (int k = 0; k < 4; ++k) o[k] += p[l] * f[k];
      }
    });
    ca_st4(out + row * c + 4 * j, o);
  }
}

// da[n] = p (dp - sum_i p_i dp_i),  dp_i = dout[n] . S_i[c_i(n)]
template <typename T>
__global__ void __launch_bounds__(CA_THREADS) ca_agg_rows_bwd_kernel(CaLevels P, const T* __restrict__ a, const T* __restrict__ dout,
                                                                     int64_t n, int c, const float* __restrict__ S, T* __restrict__ da) {
  const CaLayout Y = ca_layout(c);
  const int j = threadIdx.x % Y.G, s = threadIdx.x / Y.G;
  const int64_t rows_per_pass = (int64_t)gridDim.x * Y.R;
  const int64_t n_pass = (n + rows_per_pass - 1) / rows_per_pass;
  for (int64_t it = 0; it < n_pass; ++it) {      // uniform trip count: every lane reaches the shuffles
    const int64_t row = it * rows_per_pass + (int64_t)blockIdx.x * Y.R + s;
    const bool live = row < n && j < Y.cg;
    float dp[CA_MAX_LEVELS];
    float g[4] = {0.f, 0.f, 0.f, 0.f};
    if (live) ca_ld4(dout + row * c + 4 * j, g);
    ptc_static_for<CA_MAX_LEVELS>([&](auto I) {
      constexpr int l = I.value;
      dp[l] = 0.f;
      if (l < P.L) {
        if (live) {
          float f[4];
          ca_ld4(S + (P.off[l] + P.cluster[l][row]) * c + 4 * j, f);
          dp[l] = g[0] * f[0] + g[1] * f[1] + g[2] * f[2] + g[3] * f[3];
        }
        for (int o = Y.G >> 1; o >= 1; o >>= 1) dp[l] += __shfl_xor(dp[l], o);
      }
    });
    if (live && j == 0) {
      float p[CA_MAX_LEVELS];
      ca_softmax(a, row, P.L, p);
      float t = 0.f;
      ptc_static_for<CA_MAX_LEVELS>([&](auto I) {
        if (I.value < P.L) t += p[I.value] * dp[I.value];
      });
      ptc_static_for<CA_MAX_LEVELS>([&](auto I) {
        if (I.value < P.L) da[row * P.L + I.value] = ptc_from_float<T>(p[I.value] * (dp[I.value] - t));
      });
    }
  }
}

// Per cluster: dS = sum_{n in c} p_i(n) dout[n];  dv[m] = dS e[m] / D;  du[m] = e[m] (dS / D) (v[m] - S)  (the gradient through the
// max comes after); part[g] = sum of this cluster's du, cnt[g] = its number of elements equal to the max.
template <typename T>
__global__ void __launch_bounds__(CA_THREADS) ca_agg_cluster_bwd_kernel(CaLevels P, const T* __restrict__ a, const T* __restrict__ dout,
                                                                        int c, const float* __restrict__ S, const float* __restrict__ D,
                                                                        const uint32_t* __restrict__ mx, float* __restrict__ part,
                                                                        int32_t* __restrict__ cnt) {
  __shared__ float red[CA_THREADS * 4];
  const CaLayout Y = ca_layout(c);
  const int64_t g = blockIdx.x;
  const int l = ca_level_of(P, g);
  const int64_t cl = g - P.off[l];
  const T* u = (const T*)ca_pick(P.u, l);
  const T* v = (const T*)ca_pick(P.v, l);
  T* du = (T*)ca_pick(P.du, l);
  T* dv = (T*)ca_pick(P.dv, l);
  const int64_t* perm = ca_pick(P.perm, l);
  const int64_t* ip = ca_pick(P.indptr, l);
  const int64_t beg = ip[cl], end = ip[cl + 1];
  const uint32_t Menc = mx[l];
  const float M = ptc_float_dec(Menc);
  const int j = threadIdx.x % Y.G, s = threadIdx.x / Y.G;
  const bool act = j < Y.cg;
  float ds[4] = {0.f, 0.f, 0.f, 0.f};
  if (act)
    for (int64_t r = beg + s; r < end; r += Y.R) {
      const int64_t m = perm[r];
      float p[CA_MAX_LEVELS];
      ca_softmax(a, m, P.L, p);
      const float pl = ca_pick(p, l);
      float f[4];
      ca_ld4(dout + m * c + 4 * j, f);
      for (int k = 0; k < 4; ++k) ds[k] += pl * f[k];
    }
  ca_slot_reduce<4>(red, Y, s, j, ds);
  if (s == 0)
    for (int k = 0; k < 4; ++k) red[j * 4 + k] = ds[k];
  __syncthreads();
  float sum = 0.f;
  int n_max = 0;
  if (act) {
    float gq[4], sv[4], dd[4];
    ca_ld4(S + g * c + 4 * j, sv);
    ca_ld4(D + g * c + 4 * j, dd);
    for (int k = 0; k < 4; ++k) gq[k] = red[j * 4 + k] / dd[k];
    for (int64_t r = beg + s; r < end; r += Y.R) {
      const int64_t m = perm[r];
      float fu[4], fv[4], gu[4], gv[4];
      ca_ld4(u + m * c + 4 * j, fu);
      ca_ld4(v + m * c + 4 * j, fv);
      for (int k = 0; k < 4; ++k) {
        const float e = expf(fu[k] - M);
        gv[k] = gq[k] * e;
        gu[k] = gv[k] * (fv[k] - sv[k]);
        sum += gu[k];
        n_max += ptc_float_enc(fu[k]) == Menc;
      }
      ca_st4(dv + m * c + 4 * j, gv);
      ca_st4(du + m * c + 4 * j, gu);
    }
  }
  __syncthreads();
  red[threadIdx.x] = sum;
  red[CA_THREADS + threadIdx.x] = (float)n_max;    // exact: < 2^24 elements per thread
  __syncthreads();
  if (threadIdx.x == 0) {
    float t = 0.f, q = 0.f;
    for (int i = 0; i < CA_THREADS; ++i) {
      t += red[i];
      q += red[CA_THREADS + i];
    }
    part[g] = t;
    cnt[g] = (int32_t)q;
  }
}

// One workgroup per level: q[l] = -(sum of the level's du) / (number of elements equal to the max)  (fixed order)
__global__ void __launch_bounds__(CA_THREADS) ca_agg_max_grad_kernel(CaLevels P, const float* __restrict__ part,
                                                                     const int32_t* __restrict__ cnt, float* __restrict__ q) {
  __shared__ float rs[CA_THREADS];
  __shared__ int64_t rc[CA_THREADS];
  const int l = blockIdx.x;
  const int64_t b = P.off[l], e = P.off[l + 1];
  float t = 0.f;
  int64_t k = 0;
  for (int64_t i = b + threadIdx.x; i < e; i += CA_THREADS) {
    t += part[i];
    k += cnt[i];
  }
  rs[threadIdx.x] = t;
  rc[threadIdx.x] = k;
  __syncthreads();
  for (int o = CA_THREADS / 2; o >= 1; o >>= 1) {
    if ((int)threadIdx.x < o) {
      rs[threadIdx.x] += rs[threadIdx.x + o];
      rc[threadIdx.x] += rc[threadIdx.x + o];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) q[l] = rc[0] > 0 ? -rs[0] / (float)rc[0] : 0.f;
}

// du += q[l] on the elements equal to the max (only the clusters that hold one do any work)
template <typename T>
__global__ void __launch_bounds__(CA_THREADS) ca_agg_max_fix_kernel(CaLevels P, int c, const uint32_t* __restrict__ mx,
                                                                    const int32_t* __restrict__ cnt, const float* __restrict__ q) {
  const int64_t g = blockIdx.x;
  if (cnt[g] == 0) return;
  const CaLayout Y = ca_layout(c);
  const int l = ca_level_of(P, g);
  const int64_t cl = g - P.off[l];
  const T* u = (const T*)ca_pick(P.u, l);
  T* du = (T*)ca_pick(P.du, l);
  const int64_t* perm = ca_pick(P.perm, l);
  const int64_t* ip = ca_pick(P.indptr, l);
  const uint32_t Menc = mx[l];
  const float ql = q[l];
  const int j = threadIdx.x % Y.G, s = threadIdx.x / Y.G;
  if (j >= Y.cg) return;
  for (int64_t r = ip[cl] + s; r < ip[cl + 1]; r += Y.R) {
    const int64_t m = perm[r];
    float fu[4];
    ca_ld4(u + m * c + 4 * j, fu);
    bool hit = false;
    for (int k = 0; k < 4; ++k) hit |= ptc_float_enc(fu[k]) == Menc;
    if (!hit) continue;
    float gu[4];
    ca_ld4(du + m * c + 4 * j, gu);
    for (int k = 0; k < 4; ++k)
      if (ptc_float_enc(fu[k]) == Menc) gu[k] += ql;
    ca_st4(du + m * c + 4 * j, gu);
  }
}

// host side --------------------------------------------------------------------------------------------------------------------------
static int ca_levels(CaLevels& P, const char* who, int L, int64_t n, int c, const void* const* u, const void* const* v, void* const* du,
                     void* const* dv, const int64_t* const* perm, const int64_t* const* indptr, const int64_t* const* cluster,
                     const int64_t* n_cluster) {
  PTC_REQUIRE(L >= 1 && L <= CA_MAX_LEVELS, PTC_EINVAL, "%s: n_levels=%d outside [1, %d]", who, L, CA_MAX_LEVELS);
  PTC_REQUIRE(n >= 1, PTC_EINVAL, "%s: n=%lld", who, (long long)n);
  PTC_REQUIRE(c >= 4 && c <= 256 && c % 4 == 0, PTC_EUNSUPPORTED, "%s: c=%d (multiples of 4 up to 256)", who, c);
  PTC_REQUIRE(perm && indptr && n_cluster, PTC_EINVAL, "%s: null level arrays", who);
  P = CaLevels{};
  P.L = L;
  P.off[0] = 0;
  for (int l = 0; l < L; ++l) {
    PTC_REQUIRE(perm[l] && indptr[l] && n_cluster[l] >= 1 && n_cluster[l] <= n, PTC_EINVAL, "%s: level %d: bad maps (n_cluster %lld)",
                who, l, (long long)n_cluster[l]);
    P.u[l] = u ? u[l] : nullptr;
    P.v[l] = v ? v[l] : nullptr;
    P.du[l] = du ? du[l] : nullptr;
    P.dv[l] = dv ? dv[l] : nullptr;
    P.perm[l] = perm[l];
    P.indptr[l] = indptr[l];
    P.cluster[l] = cluster ? cluster[l] : nullptr;
    P.off[l + 1] = P.off[l] + n_cluster[l];
  }
  for (int l = L; l < CA_MAX_LEVELS; ++l) P.off[l + 1] = P.off[L];
  PTC_REQUIRE(P.off[L] < (1ll << 31), PTC_EUNSUPPORTED, "%s: %lld clusters", who, (long long)P.off[L]);
  return PTC_OK;
}

static int ca_rows_grid(int64_t n, int c) {
  int64_t gr = ptc_cdiv(n, ca_layout(c).R);
  return (int)(gr > 8192 ? 8192 : gr);
}

}  // namespace

// ------------------------------------------------------------------------------------------------------------------------------------
extern "C" size_t ptc_grid_cluster_workspace_bytes(int64_t n, int n_levels) { return ca_map_layout(n, n_levels).total; }

extern "C" int ptc_grid_cluster_count(const int32_t* indices, int64_t n, const int* sizes, int n_levels, const int* spatial_shape,
                                      int batch_size, int64_t* order, int64_t* cluster, int64_t* n_cluster, void* workspace,
                                      size_t workspace_bytes, ptc_stream_t stream) {
  PTC_REQUIRE(n >= 1 && n < (1ll << 32), PTC_EINVAL, "ptc_grid_cluster_count: n=%lld", (long long)n);
  PTC_REQUIRE(n_levels >= 1 && n_levels <= CA_MAX_LEVELS, PTC_EINVAL, "ptc_grid_cluster_count: n_levels=%d", n_levels);
  PTC_REQUIRE(indices && sizes && spatial_shape && order && cluster && n_cluster && workspace, PTC_EINVAL,
              "ptc_grid_cluster_count: null buffer");
  PTC_REQUIRE(batch_size >= 1, PTC_EINVAL, "ptc_grid_cluster_count: batch_size=%d", batch_size);
  const CaMapLayout Y = ca_map_layout(n, n_levels);
  PTC_REQUIRE(workspace_bytes >= Y.total, PTC_EWORKSPACE, "ptc_grid_cluster_count: workspace %zu < %zu", workspace_bytes, Y.total);
  CaKeyLevels lv{};
  lv.L = n_levels;
  int end_bit = 0;
  const int bb = ca_bits(batch_size - 1);
  for (int l = 0; l < n_levels; ++l) {
    PTC_REQUIRE(sizes[l] >= 1, PTC_EINVAL, "ptc_grid_cluster_count: size[%d]=%d", l, sizes[l]);
    lv.size[l] = (float)sizes[l];
    // coordinates lie in [0, spatial_shape): every cell index is at most (shape - 1) / size, whatever the minimum
    lv.bx[l] = ca_bits((spatial_shape[0] - 1) / sizes[l]);
    lv.by[l] = ca_bits((spatial_shape[1] - 1) / sizes[l]);
    lv.bz[l] = ca_bits((spatial_shape[2] - 1) / sizes[l]);
    const int tot = bb + lv.bx[l] + lv.by[l] + lv.bz[l];
    PTC_REQUIRE(tot <= 64, PTC_EUNSUPPORTED, "ptc_grid_cluster_count: level %d needs %d key bits", l, tot);
    end_bit = tot > end_bit ? tot : end_bit;
  }
  hipStream_t s = (hipStream_t)stream;
  char* ws = (char*)workspace;
  int32_t* mn = (int32_t*)(ws + Y.mn);
  int64_t* keys = (int64_t*)(ws + Y.keys);
  PTC_HIP(hipMemsetAsync(mn, 0x7f, 16, s));
  int64_t grid = ptc_cdiv(n, 256);
  if (grid > 1024) grid = 1024;
  hipLaunchKernelGGL(ca_coord_min_kernel, dim3((unsigned)grid), dim3(256), 0, s, indices, n, mn);
  PTC_CHECK_LAUNCH("ca_coord_min_kernel");
  hipLaunchKernelGGL(ca_keys_kernel, dim3((unsigned)grid), dim3(256), 0, s, indices, n, (const int32_t*)mn, lv, keys);
  PTC_CHECK_LAUNCH("ca_keys_kernel");
  const size_t sws = workspace_bytes - Y.scratch;
  int rc = ptc_sort_keys(keys, n, n_levels, 0, end_bit > 0 ? end_bit : 1, order, nullptr, ws + Y.scratch, sws, stream);
  if (rc != PTC_OK) return rc;
  for (int l = 0; l < n_levels; ++l) {
    rc = ptc_pool_maps_count(keys + (int64_t)l * n, order + (int64_t)l * n, n, 0, cluster + (int64_t)l * n, n_cluster + l,
                             ws + Y.scratch, sws, stream);
    if (rc != PTC_OK) return rc;
  }
  return PTC_OK;
}

extern "C" int ptc_cluster_center(const void* const* x, const int64_t* const* perm, const int64_t* const* indptr, const int64_t* n_cluster,
                                  int n_levels, int64_t n, int c, int dtype, void* const* y, ptc_stream_t stream) {
  CaLevels P;
  int rc = ca_levels(P, "ptc_cluster_center", n_levels, n, c, x, nullptr, y, nullptr, perm, indptr, nullptr, n_cluster);
  if (rc != PTC_OK) return rc;
  for (int l = 0; l < n_levels; ++l) PTC_REQUIRE(x[l] && y[l], PTC_EINVAL, "ptc_cluster_center: null tensor at level %d", l);
  PTC_DISPATCH_DTYPE(dtype, T, {
    hipLaunchKernelGGL(ca_center_kernel<T>, dim3((unsigned)P.off[n_levels]), dim3(CA_THREADS), 0, (hipStream_t)stream, P, c);
    PTC_CHECK_LAUNCH("ca_center_kernel");
  });
  return PTC_OK;
}

extern "C" size_t ptc_cluster_agg_state_bytes(int64_t n_cluster_total, int c) {
  return (size_t)2 * n_cluster_total * c * 4 + (size_t)CA_MAX_LEVELS * 4;
}

extern "C" size_t ptc_cluster_agg_workspace_bytes(int64_t n_cluster_total) {
  return ptc_align_up((size_t)n_cluster_total * 4, 256) * 2 + (size_t)CA_MAX_LEVELS * 4;
}

extern "C" int ptc_cluster_agg_fwd(const void* const* u, const void* const* v, const void* a, const int64_t* const* perm,
                                   const int64_t* const* indptr, const int64_t* const* cluster, const int64_t* n_cluster, int n_levels,
                                   int64_t n, int c, int dtype, void* out, void* state, size_t state_bytes, ptc_stream_t stream) {
  CaLevels P;
  int rc = ca_levels(P, "ptc_cluster_agg_fwd", n_levels, n, c, u, v, nullptr, nullptr, perm, indptr, cluster, n_cluster);
  if (rc != PTC_OK) return rc;
  PTC_REQUIRE(a && out && state && cluster, PTC_EINVAL, "ptc_cluster_agg_fwd: null buffer");
  for (int l = 0; l < n_levels; ++l)
    PTC_REQUIRE(u[l] && v[l] && cluster[l], PTC_EINVAL, "ptc_cluster_agg_fwd: null tensor at level %d", l);
  const int64_t tot = P.off[n_levels];
  PTC_REQUIRE(state_bytes >= ptc_cluster_agg_state_bytes(tot, c), PTC_EWORKSPACE, "ptc_cluster_agg_fwd: state %zu bytes",
              state_bytes);
  hipStream_t s = (hipStream_t)stream;
  float* S = (float*)state;
  float* D = S + tot * c;
  uint32_t* mx = (uint32_t*)(D + tot * c);
  PTC_HIP(hipMemsetAsync(mx, 0, CA_MAX_LEVELS * 4, s));
  int64_t mg = ptc_cdiv(n * c / 4, 256);
  if (mg > 512) mg = 512;
  PTC_DISPATCH_DTYPE(dtype, T, {
    hipLaunchKernelGGL(ca_max_kernel<T>, dim3((unsigned)mg, (unsigned)n_levels), dim3(256), 0, s, P, n * c, mx);
    PTC_CHECK_LAUNCH("ca_max_kernel");
    hipLaunchKernelGGL(ca_agg_cluster_fwd_kernel<T>, dim3((unsigned)tot), dim3(CA_THREADS), 0, s, P, c, S, D, (const uint32_t*)mx);
    PTC_CHECK_LAUNCH("ca_agg_cluster_fwd_kernel");
    hipLaunchKernelGGL(ca_agg_rows_fwd_kernel<T>, dim3((unsigned)ca_rows_grid(n, c)), dim3(CA_THREADS), 0, s, P, (const T*)a, n, c,
                       (const float*)S, (T*)out);
    PTC_CHECK_LAUNCH("ca_agg_rows_fwd_kernel");
  });
  return PTC_OK;
}

extern "C" int ptc_cluster_agg_bwd(const void* const* u, const void* const* v, const void* a, const void* dout, const int64_t* const* perm,
                                   const int64_t* const* indptr, const int64_t* const* cluster, const int64_t* n_cluster, int n_levels,
                                   int64_t n, int c, int dtype, const void* state, size_t state_bytes, void* const* du, void* const* dv,
                                   void* da, void* workspace, size_t workspace_bytes, ptc_stream_t stream) {
  CaLevels P;
  int rc = ca_levels(P, "ptc_cluster_agg_bwd", n_levels, n, c, u, v, du, dv, perm, indptr, cluster, n_cluster);
  if (rc != PTC_OK) return rc;
  PTC_REQUIRE(a && dout && state && da && workspace && cluster && du && dv, PTC_EINVAL, "ptc_cluster_agg_bwd: null buffer");
  for (int l = 0; l < n_levels; ++l)
    PTC_REQUIRE(u[l] && v[l] && cluster[l] && du[l] && dv[l], PTC_EINVAL, "ptc_cluster_agg_bwd: null tensor at level %d", l);
  const int64_t tot = P.off[n_levels];
  PTC_REQUIRE(state_bytes >= ptc_cluster_agg_state_bytes(tot, c), PTC_EWORKSPACE, "ptc_cluster_agg_bwd: state %zu bytes",
              state_bytes);
  PTC_REQUIRE(workspace_bytes >= ptc_cluster_agg_workspace_bytes(tot), PTC_EWORKSPACE, "ptc_cluster_agg_bwd: workspace %zu bytes",
              workspace_bytes);
  hipStream_t s = (hipStream_t)stream;
  const float* S = (const float*)state;
  const float* D = S + tot * c;
  const uint32_t* mx = (const uint32_t*)(D + tot * c);
  char* ws = (char*)workspace;
  float* part = (float*)ws;
  int32_t* cnt = (int32_t*)(ws + ptc_align_up((size_t)tot * 4, 256));
  float* q = (float*)(ws + 2 * ptc_align_up((size_t)tot * 4, 256));
  PTC_DISPATCH_DTYPE(dtype, T, {
    hipLaunchKernelGGL(ca_agg_rows_bwd_kernel<T>, dim3((unsigned)ca_rows_grid(n, c)), dim3(CA_THREADS), 0, s, P, (const T*)a,
                       (const T*)dout, n, c, S, (T*)da);
    PTC_CHECK_LAUNCH("ca_agg_rows_bwd_kernel");
    hipLaunchKernelGGL(ca_agg_cluster_bwd_kernel<T>, dim3((unsigned)tot), dim3(CA_THREADS), 0, s, P, (const T*)a, (const T*)dout, c, S, D,
                       mx, part, cnt);
    PTC_CHECK_LAUNCH("ca_agg_cluster_bwd_kernel");
    hipLaunchKernelGGL(ca_agg_max_grad_kernel, dim3((unsigned)n_levels), dim3(CA_THREADS), 0, s, P, (const float*)part,
                       (const int32_t*)cnt, q);
    PTC_CHECK_LAUNCH("ca_agg_max_grad_kernel");
    hipLaunchKernelGGL(ca_agg_max_fix_kernel<T>, dim3((unsigned)tot), dim3(CA_THREADS), 0, s, P, c, mx, (const int32_t*)cnt,
                       (const float*)q);
    PTC_CHECK_LAUNCH("ca_agg_max_fix_kernel");
  });
  return PTC_OK;
}
